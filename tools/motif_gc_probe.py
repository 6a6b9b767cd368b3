"""Measurements of motif methylation by local GC content (tools/gpu_motif_gc.sh; results: profiles/r22/motif_gc.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_gc` twice, one cold process each; wall clocks, the split the command records
               (ingest / engine / text), the flags and the sizes of the four files
  trace DIR    the count passes only, one process on the files of DIR with the state planes AND the read statistics resident, two
               repetitions each, in this order: on the candidates of bin-motifs.tsv `motif_site_counts` (sites_kernel's count pass, the
               yardstick: the same loads and walks), `motif_fractions` at 20 bins (the other LDS histogram) and `motif_gc` at half 1, 15
               and 31 (W = 3, 31, 63: the cost per site must not depend on W); then on the one-letter background candidates (every A /
               every C of every bin: dense sites) `motif_site_counts` and `motif_gc` at the three halves.  The order of the calls goes to
               DIR/calls.json for the reader of the kernel trace; every gc table is compared with the site counts first
One JSON line per mode on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motif_compare_probe import cli      # noqa: E402  (the same directory)
from motif_fractions_probe import load   # noqa: E402

HALVES = (1, 15, 31)
GC = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "gc"]
NAMES = ("motif-gc.tsv", "motif-gc-bins.tsv", "motif-gc-contigs.tsv", "motif-gc-summary.tsv")


def files(tmp, total_bp):
    import torch
    from nanomotif_amd import e2e_synth, synth
    spec = synth.config("cfg3") if total_bp == 100_000_000 else synth.SynthSpec(
        n_contigs=max(8, total_bp // 100_000), total_bp=total_bp, n_bins=max(2, total_bp // 2_000_000), mod_types=("a", "m"), seed=1)
    mg = synth.make_metagenome(spec)
    t0 = time.perf_counter()
    sizes = e2e_synth.write_text_inputs(mg, tmp, torch.device("cuda", 0))
    out = {"mode": "files", "total_bp": total_bp, "rows": sizes["rows"], "bed_bytes": sizes["bed_bytes"], "written_in_s": time.perf_counter() - t0}
    torch.cuda.empty_cache()
    out["motif_discovery_wall_s"] = cli(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    out["motif_rows"] = len(open(os.path.join(tmp, "out", "bin-motifs.tsv")).read().splitlines()) - 1
    for rep in ("cold", "again"):
        wall = cli(tmp, "motif_gc", GC)
        t = json.load(open(os.path.join(tmp, "gc", "logs", "timings.motif_gc.json")))
        out["motif_gc_" + rep] = dict(wall_s=wall, **t)
    rows = [l.split("\t") for l in open(os.path.join(tmp, "gc", "motif-gc-summary.tsv")).read().splitlines()]
    col = {name: j for j, name in enumerate(rows[0])}
    zs = sorted(abs(float(r[col["trend_z_within"]])) for r in rows[1:])
    deltas = sorted(abs(float(r[col["delta"]])) for r in rows[1:] if r[col["delta"]])
    out.update(candidates=len(rows) - 1, flags={f: sum(r[-1] == f for r in rows[1:]) for f in ("none", "gc_dependent", "few_sites")},
               flagged_rows=[r for r in rows[1:] if r[-1] == "gc_dependent"][:20], abs_z_within_max=zs[-1] if zs else None,
               abs_z_within_median=zs[len(zs) // 2] if zs else None, abs_delta_max=deltas[-1] if deltas else None,
               out_bytes={n: os.path.getsize(os.path.join(tmp, "gc", n)) for n in NAMES})
    return out


def trace(tmp):
    from nanomotif_amd import loading
    from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL, Motif
    eng, cands, ingest_s, readstats_s, _ = load(tmp, "pileup.bed")
    flat = [c.engine_candidate() for c in cands]
    mod_types = loading.kept_mod_types(eng)
    background = [(Motif(MOD_TYPE_TO_CANONICAL[mt], 0), mt, b) for b in sorted(eng.bin_index) if eng.bin_contigs(b) for mt in mod_types]
    out = {"mode": "trace", "ingest_s": ingest_s, "readstats_s": readstats_s, "candidates": len(flat), "background_candidates": len(background), "halves": list(HALVES)}
    calls = [("motifs_site_counts", "sites_kernel", lambda: eng.motif_site_counts(flat)),
             ("motifs_fractions_b20", "fractions_kernel", lambda: list(eng.motif_fractions(flat, bins=20)))]
    calls += [(f"motifs_gc_half{h}", "gc_kernel", lambda h=h: list(eng.motif_gc(flat, half=h))) for h in HALVES]
    calls += [("background_site_counts", "sites_kernel", lambda: eng.motif_site_counts(background))]
    calls += [(f"background_gc_half{h}", "gc_kernel", lambda h=h: list(eng.motif_gc(background, half=h))) for h in HALVES]
    res, order = {}, []
    for name, kernel, fn in calls:
        ts = []
        for rep in range(2):
            before = eng.stats()["launches"]
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
            order.append({"call": name, "rep": rep, "kernel": kernel, "launches": eng.stats()["launches"] - before})
        out[name + "_s"] = ts
    with open(os.path.join(tmp, "calls.json"), "w") as f:
        json.dump(order, f)
    for group in ("motifs", "background"):
        six = [t for _, t in res[group + "_site_counts"]]
        ok = all(np.array_equal(t.sum(axis=-1).reshape(len(t), 6), s) for h in HALVES for (_, t), s in zip(res[f"{group}_gc_half{h}"], six))
        out[group + "_gc_sums_equal_site_counts"] = bool(ok)
        out[group + "_sites"] = int(sum(int(s.sum()) for s in six))
        out[group + "_edge_sites_half31"] = int(sum(int(t[..., -1].sum()) for _, t in res[group + "_gc_half31"]))
    eng.close()
    return out


def table(tmp, trace_csv):
    """The dispatches of the three count kernels in time order against calls.json: per call and repetition the summed kernel time (us)."""
    import csv
    calls = json.load(open(os.path.join(tmp, "calls.json")))
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    kernels = ("sites_kernel", "fractions_kernel", "gc_kernel")
    disp = [(next(k for k in kernels if k in r["Kernel_Name"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            for r in rows if any(k in r["Kernel_Name"] for k in kernels)]
    at, out = 0, {}
    for c in calls:
        ns = 0
        for _ in range(c["launches"]):
            assert disp[at][0] == c["kernel"], (c, at, disp[at])
            ns += disp[at][1]
            at += 1
        out.setdefault(c["call"], []).append(round(ns / 1000.0, 1))
    assert at == len(disp), (at, len(disp))
    return {"mode": "table", "kernel_us": out}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace", "table"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    ap.add_argument("--trace-csv", default=None)
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir) if a.mode == "trace" else table(a.dir, a.trace_csv)), flush=True)
