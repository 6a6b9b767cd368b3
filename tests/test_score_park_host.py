"""Which batches the scoring plan (nanomotif_amd/csrc/nmscore_plan.h) sends to the parked class kernel, and what that kernel's seven
resident workgroups a CU do to the launch grid — on the CPU, through tools/plan_check/driver.cpp: ``plan_check park`` plans the cases
(checking each against the driver's restatement as it goes) and prints one line per batch, which is read here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tools", "plan_check", "driver.cpp")
CXX = os.environ.get("CXX", "g++")

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")

SIZES = [1, 28, 29, 32, 33, 56, 57, 64, 65]
UNPARKED = {29, 30, 31, 32} | set(range(57, 65))       # ceil(n / 28) != ceil(n / 32)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_check") / "plan_check")
    built = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Wextra", DRIVER, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("NM_")}
    done = subprocess.run([exe, "park"], capture_output=True, text=True, timeout=300, env=env)
    assert done.returncode == 0 and "plan_check ok" in done.stdout, done.stdout[-2000:] + done.stderr
    out = []
    for line in done.stdout.splitlines():
        f = line.split()
        if f and f[0] == "park":
            out.append({"what": f[1], **{k: int(v) for k, v in zip(f[2::2], f[3::2])}})
    return out


def of(lines, what):
    got = {r["size"]: r for r in lines if r["what"] == what}
    assert got
    return got


def test_the_rule_is_the_pass_count():
    assert {n for n in range(1, 85) if -(-n // 28) != -(-n // 32)} == UNPARKED


@pytest.mark.parametrize("size", SIZES)
def test_park_rule_at_group_size(lines, size):
    r = of(lines, "rule")[size]
    assert r["classes"] == 1
    assert r["parked"] == (0 if size in UNPARKED else 1) and r["fits"] == r["parked"]


def test_more_passes_at_84_and_beyond(lines):
    rule = of(lines, "rule")
    assert [rule[n]["parked"] for n in (84, 85, 96, 97)] == [1, 0, 0, 1]


@pytest.mark.parametrize("size", SIZES)
def test_switch_zero_never_parks(lines, size):
    r = of(lines, "switch0")[size]
    assert r["classes"] == 1 and r["parked"] == 0
    assert r["fits"] == (0 if size in UNPARKED else 1)          # (the rule is still worked out)


@pytest.mark.parametrize("size", SIZES)
def test_per_contig_and_8_plane_batches_never_park(lines, size):
    assert of(lines, "per_contig")[size]["classes"] == 1 and of(lines, "per_contig")[size]["parked"] == 0
    assert of(lines, "classes0")[size]["classes"] == 0 and of(lines, "classes0")[size]["parked"] == 0


@pytest.mark.parametrize("what", ["light", "literal", "wide"])
def test_other_kernels_never_park(lines, what):
    (r,) = of(lines, what).values()
    assert r["classes"] == 0 and r["parked"] == 0 and r["fits"] == 1


def grid(r, per_cu):
    """plan_geometry for a heavy batch of one slot, every bin active, one group a bin: {split_log2, j_big, gx}."""
    resident, est = r["n_cus"] * per_cu, r["n_segments"]
    assert r["gy"] == 1 and r["n_groups"] == r["size"]
    split = 0 if est >= 2 * resident else 1 if 2 * est >= 2 * resident else 2
    per_run = ((r["n_segments"] << split) + 7) // 8
    fine = 2 - split
    tail = min(per_run, (resident + 7) // 8) if fine else 0
    return {"split_log2": split, "fine_log2": fine, "pieces_per_run": per_run, "j_big": per_run - tail, "gx": (per_run - tail + (tail << fine)) * 8}


@pytest.mark.parametrize("bins", [120, 208, 400])
def test_seven_against_six_resident(lines, bins):
    parked, plain = of(lines, "grid")[bins], of(lines, "grid0")[bins]
    assert parked["parked"] == 1 and plain["parked"] == 0 and parked["n_segments"] == plain["n_segments"]
    for r, per_cu in ((parked, 7), (plain, 6)):
        want = grid(r, per_cu)
        assert {k: r[k] for k in want} == want
    # 208 bins: between two rounds of 6 x 256 and two of 7 x 256 workgroups, the parked batch alone halves its pieces
    assert (parked["split_log2"], plain["split_log2"]) == {120: (1, 1), 208: (1, 0), 400: (0, 0)}[bins]
    assert parked["j_big"] != plain["j_big"] and parked["gx"] != plain["gx"]
    if parked["split_log2"] == plain["split_log2"]:          # 32 more pieces a run go in finer parts
        assert plain["j_big"] - parked["j_big"] == 32 and parked["gx"] > plain["gx"]
