"""Heavy batches (more than six candidates per (bin, mod type): the non-CF scoring kernels) read only the forward half of a
candidate's program and derive every reverse-strand constraint from it: complemented plane, mirrored word-group, shift
32 - r (r = 0: the next word-group, unshifted).  Bit-exact against the oracle for every plane at every offset, every
constraint count, the reach edges of the wide kernels, non-compact batches, both canonical bases and per-contig counters."""
import numpy as np
import pytest

from helpers import oracle_bin_inputs
from nanomotif_amd import synth
from nanomotif_amd.motif import Motif

pytestmark = pytest.mark.gpu

# one set per plane of the 8-plane tile: the four literals (is-X) and the four 3-sets (valid and not X)
PLANE_SETS = ["A", "C", "G", "T", "[CGT]", "[AGT]", "[ACT]", "[ACG]"]
CANONICAL = {"a": "A", "m": "C"}


@pytest.fixture(scope="module")
def scene():
    from nanomotif_amd.engine import ScanEngine
    spec = synth.SynthSpec(n_contigs=4, total_bp=64_000, n_bins=2, mod_types=("a", "m"), seed=77, min_contig_bp=10_000,
                           fixed_motifs=(("GATC", 1, "a"), ("CCWGG", 1, "m")))
    mg = synth.make_metagenome(spec)
    eng = ScanEngine(0)
    eng.upload_assembly(mg.names, [mg.contig_ascii(i) for i in range(len(mg.names))], mg.bin_names)
    for mt in ("a", "m"):
        cols = mg.pileup_columns(mt)
        keep = cols["nvalid"] > 5
        eng.upload_pileup(mt, cols["contig_id"][keep], cols["position"][keep], cols["strand"][keep], cols["fraction_mod"][keep])
    bins = sorted(set(mg.bin_names))
    inputs = {}
    for b in bins:
        idx = [i for i, x in enumerate(mg.bin_names) if x == b]
        for mt in ("a", "m"):
            inputs[(b, mt)] = (idx, oracle_bin_inputs(mg, mt, contigs=idx))
    yield mg, eng, bins, inputs
    eng.close()


def _motif(mod_set, others):
    """(motif string, mod_position): `mod_set` at the modified position, (offset from it, set) for the rest."""
    lo = min([0] + [d for d, _ in others])
    hi = max([0] + [d for d, _ in others])
    pos = ["."] * (hi - lo + 1)
    pos[-lo] = mod_set
    for d, s in others:
        pos[d - lo] = s
    return "".join(pos), -lo


def _check(scene, zoo, per_contig=False):
    """zoo: (string, mod_position, mod_type); every bin scores the whole zoo in ONE batch (a heavy one: > 6 per group)."""
    from oracle.scan import score_candidates
    mg, eng, bins, inputs = scene
    per_type = [sum(t == mt for _, _, t in zoo) for mt in ("a", "m")]
    assert all(n == 0 or n > 6 for n in per_type)
    cands = [(Motif(s, p), mt, b) for b in bins for s, p, mt in zoo]
    if per_contig:
        from oracle.contig_methylation import per_contig_counts
        got = eng.score_per_contig(cands)
        k = 0
        for b in bins:
            for s, p, mt in zoo:
                idx, (pile, seqs) = inputs[(b, mt)]
                names, table = got[k]
                want = per_contig_counts(pile, seqs, s, p)
                assert table.tolist() == [list(want[n]) for n in names], (b, s, p, mt)
                k += 1
        return
    got = eng.score(cands)
    want = []
    for b in bins:
        for s, p, mt in zoo:
            idx, (pile, seqs) = inputs[(b, mt)]
            want.append(score_candidates(pile, seqs, [(s, p)])[0])
    want = np.asarray(want)
    bad = [(cands[i][0].string, cands[i][0].mod_position, cands[i][1], cands[i][2], got[i].tolist(), want[i].tolist())
           for i in range(len(cands)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:10]
    assert want.sum() > 0


@pytest.mark.parametrize("mt", ["a", "m"])
def test_every_plane_at_every_narrow_offset(scene, mt):
    """Compact narrow batches (the headline kernel): one constraint per strand, every plane, offsets -31..31."""
    zoo = []
    for d in range(-31, 32):
        if d == 0:
            continue
        for s in PLANE_SETS:
            string, mp = _motif(CANONICAL[mt], [(d, s)])
            zoo.append((string, mp, mt))
    _check(scene, zoo)


def test_every_constraint_count_odd_and_even(scene):
    """1..12 constraints per strand (literals and 3-sets; a 2-set counts twice), both canonical bases in one batch."""
    rng = np.random.default_rng(5)
    zoo = []
    offsets = [d for d in range(-31, 32) if d != 0]
    for n in range(1, 13):
        for rep in range(3):
            for mt in ("a", "m"):
                ds = rng.choice(offsets, size=n, replace=False)
                sets = [PLANE_SETS[int(rng.integers(0, 4))] if rng.random() < 0.8 else PLANE_SETS[int(rng.integers(4, 8))] for _ in ds]
                string, mp = _motif(CANONICAL[mt], list(zip(ds.tolist(), sets)))
                zoo.append((string, mp, mt))
    # two constraints from one position (2-sets) and neighbours on the same plane word
    for mt in ("a", "m"):
        zoo.append((_motif(CANONICAL[mt], [(-1, "[AG]"), (1, "[CT]"), (2, "G")]) + (mt,)))
        zoo.append((_motif(CANONICAL[mt], [(d, "G") for d in (1, 2, 3, 5, 8, 13, 21)]) + (mt,)))
        zoo.append((_motif(CANONICAL[mt], [(-d, "T") for d in (1, 2, 3, 5, 8, 13, 21, 31)]) + (mt,)))
    _check(scene, zoo)
    # literals only: the 4-plane kernel
    lit = []
    for n in range(1, 13):
        for mt in ("a", "m"):
            ds = rng.choice(offsets, size=n, replace=False)
            lit.append(_motif(CANONICAL[mt], [(d, PLANE_SETS[int(rng.integers(0, 4))]) for d in ds.tolist()]) + (mt,))
    _check(scene, lit * 2)


@pytest.mark.parametrize("edge", [32, 63, 64, 95])
def test_reach_edges_of_the_wide_kernels(scene, edge):
    """Offsets at the word-group boundaries of the wide kernels (r = 0 at +-32 and +-64), every plane, both directions."""
    zoo = []
    for mt in ("a", "m"):
        for s in PLANE_SETS:
            for d in (edge, -edge, edge - 1, -(edge - 1), 1 - edge, edge // 2, -(edge // 2), 31, -31, 32, -32):
                if d == 0 or abs(d) > edge:
                    continue
                string, mp = _motif(CANONICAL[mt], [(d, s), (edge if d != edge else -edge, "G")])
                zoo.append((string, mp, mt))
    _check(scene, zoo)


@pytest.mark.parametrize("reach", [20, 40, 90])
def test_non_canonical_modified_position(scene, reach):
    """Non-compact batches: the modified position carries a set that is not the slot's canonical literal, so it is a
    constraint of the program (r = 0 at d = 0) — narrow, wide and extra-wide kernels."""
    zoo = []
    for mt in ("a", "m"):
        for mod_set in ("[AG]", "[ACT]", "G", CANONICAL[mt]):
            for s in PLANE_SETS:
                for d in (1, -1, reach, -reach, 32 if reach > 32 else 5, -32 if reach > 32 else -5):
                    string, mp = _motif(mod_set, [(d, s)])
                    zoo.append((string, mp, mt))
    _check(scene, zoo)


@pytest.mark.parametrize("reach", [25, 60])
def test_per_contig_counters(scene, reach):
    """Per-contig mode (the PC kernels) on compact and non-compact batches."""
    rng = np.random.default_rng(reach)
    zoo = []
    for mt in ("a", "m"):
        for mod_set in (CANONICAL[mt], "[AG]"):
            for n in range(1, 9):
                ds = rng.choice([d for d in range(-reach, reach + 1) if d != 0], size=n, replace=False)
                sets = [PLANE_SETS[int(rng.integers(0, 8))] for _ in ds]
                string, mp = _motif(mod_set, list(zip(ds.tolist(), sets)))
                zoo.append((string, mp, mt))
    _check(scene, zoo, per_contig=True)
