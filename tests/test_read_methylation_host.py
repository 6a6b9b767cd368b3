"""Host side of the per-contig READ methylation table (no GPU): the brute force ``tests/test_gpu_read_methylation.py`` compares
``nm_readstats_upload`` / ``nm_contig_methylation`` (csrc/nmmeth.hip) against — built only from ``oracle.scan.subseq_indices`` and
``oracle.motif.Motif`` plus plain numpy for the filters, the sums and the median — the geometry input it runs on, the conditions that make
that input worth running, and the agreement of the brute force with ``oracle.contig_methylation.read_methylation`` (so the two restatements
pin each other; parity with epimetheus itself stays unpinned).

The brute force is the definition.  A record is kept iff ``n_valid >= min_cov and n_valid > 0`` and, when ``n_diff`` is given,
``n_valid / (n_valid + n_diff) >= min_frac`` in float64.  Per (motif, contig), over the sites of the stripped motif on '+' and of its reverse
complement on '-' (``mod_position' = len - 1 - mod_position``) that carry a kept record of the motif's code: ``n_motif_obs``,
``mean_read_cov = sum(cov) / n``, the median of ``mod / cov`` (mean of the two middle values for an even ``n``) and ``sum(mod) / sum(cov)``."""
import functools

import numpy as np

from nanomotif_amd.motif import regex_to_iupac
from test_gpu_motif_compare import reach_class
from test_motif_strands_host import GEOMETRY_MOTIFS, geometry_input

MIN_COV, MIN_FRAC = 3, 0.8
CODES = ("a", "m")
SEED = 7
PLUS, MINUS = ord("+"), ord("-")


# ------------------------------------------------------------------------------------------------ the brute force
def kept_mask(r, min_cov=MIN_COV, min_frac=MIN_FRAC, use_diff=True):
    nv = r["n_valid"].astype(np.int64)
    keep = (nv >= min_cov) & (nv > 0)
    if use_diff:
        with np.errstate(invalid="ignore", divide="ignore"):
            keep &= nv.astype(np.float64) / (nv.astype(np.float64) + r["n_diff"].astype(np.float64)) >= min_frac
    return keep


def site_positions(seq, motif, pos):
    """(positions of the modified base on '+', on '-') of one motif (regex form) on one contig."""
    from oracle.motif import Motif as OMotif
    from oracle.scan import subseq_indices
    st = OMotif(motif, pos).new_stripped_motif()
    rc = st.reverse_compliment()
    assert rc.mod_position == len(st.split()) - 1 - st.mod_position
    return subseq_indices(st.string, seq) + st.mod_position, subseq_indices(rc.string, seq) + rc.mod_position


def median_of(frac):
    s = sorted(frac)
    n = len(s)
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


class Segment:
    """One (motif, contig) with at least one site that carries a kept record."""

    def __init__(self, cov, mod):
        self.cov, self.mod = [int(x) for x in cov], [int(x) for x in mod]
        self.n = len(self.cov)
        self.cov_sum, self.mod_sum = sum(self.cov), sum(self.mod)
        self.frac = sorted(float(m) / float(c) for m, c in zip(self.mod, self.cov))
        self.mean_read_cov = float(self.cov_sum) / self.n
        self.median = median_of(self.frac)
        self.weighted_mean = float(self.mod_sum) / float(self.cov_sum)


def brute_force(seqs, records, motifs, min_cov=MIN_COV, min_frac=MIN_FRAC, use_diff=True):
    """seqs: name -> str (in engine order); records: {(name, code): columns}; motifs: (regex motif, code, mod position) triples.
    -> {(motif index, contig name): Segment}."""
    dense = {}
    for (name, code), r in records.items():
        keep = kept_mask(r, min_cov, min_frac, use_diff)
        cov = np.full((2, len(seqs[name])), -1, dtype=np.int64)
        mod = np.zeros((2, len(seqs[name])), dtype=np.int64)
        s = (r["strand"][keep] == MINUS).astype(np.int64)
        assert ((r["strand"] == PLUS) | (r["strand"] == MINUS)).all()
        cov[s, r["position"][keep]] = r["n_valid"][keep]
        mod[s, r["position"][keep]] = r["n_mod"][keep]
        dense[(name, code)] = (cov, mod)
    out = {}
    for k, (motif, code, pos) in enumerate(motifs):
        for name, seq in seqs.items():
            if (name, code) not in dense:
                continue
            cov, mod = dense[(name, code)]
            c, m = [], []
            for s, sites in enumerate(site_positions(seq, motif, pos)):
                have = cov[s, sites] >= 0
                c += cov[s, sites[have]].tolist()
                m += mod[s, sites[have]].tolist()
            if c:
                out[(k, name)] = Segment(c, m)
    return out


def rows_of(segments, seqs, names, output_type):
    """The rows ``read_methylation_table`` returns for ``names`` = [(IUPAC motif, code, mod position)] (in the order of the motifs
    ``segments`` was computed for): motif-major, contigs in engine order."""
    rows = []
    for k, (iupac, code, pos) in enumerate(names):
        for name in seqs:
            g = segments.get((k, name))
            if g is not None:
                rows.append((name, iupac, code, pos, g.median if output_type == "median" else g.weighted_mean, g.mean_read_cov, g.n))
    return rows


# ------------------------------------------------------------------------------------------------ the geometry input (shared with the GPU suite)
LONG_A = (511, 32_767, 36_863)          # '+' A of the planted GATC of `long`: last bit of a rank block, of a round of 64 rank blocks (and of a
#                                         chunk), of a lane and a rank block; the '-' partners sit at 512, 32 768 and 36 864, so 32 767 | 32 768
#                                         are the two sides of the carry.  (GATC cannot put a '+' A on 32 767 and on 32 768: the '+' plane's
#                                         first bit of block 64 is the record on the T of that site, which T @ 0 reads.)
LANES_BLOCK = 40 * 512                  # the 512-bp block of `long` with kept records in all four lanes and a GATC site in the last one
LANES_KEPT = (LANES_BLOCK + 5, LANES_BLOCK + 130, LANES_BLOCK + 260)
LANES_SITE = LANES_BLOCK + 400          # its '+' A
# (contig, position, strand) -> (coverage, modified) of the hand-planted kept records
PLANTED = {("long", 511, PLUS): (11, 3), ("long", 512, MINUS): (12, 12), ("long", 32_767, PLUS): (13, 0), ("long", 32_768, MINUS): (14, 7),
           ("long", 32_768, PLUS): (9, 2), ("long", 36_863, PLUS): (15, 15), ("long", 36_864, MINUS): (16, 1), ("long", LANES_SITE, PLUS): (17, 5),
           ("long", LANES_SITE + 1, MINUS): (18, 9)}
PLANTED_SITES = [k for k in PLANTED if k[1:] != (32_768, PLUS)]          # the GATC sites among them: '+' A and '-' partner of four occurrences
for _p in LANES_KEPT:
    PLANTED[("long", _p, PLUS)] = (20, 10)


@functools.lru_cache(maxsize=None)
def meth_input():
    """(names, seqs, records): the contigs of ``test_motif_strands_host.geometry_input`` followed by `long` (40 000 bp, GATC on the rank-table
    borders), `norec` (sites, no records), `endGA` | `startTC` (GATC only across the contig border).  records: {(name, code): columns} in
    ascending (position, strand) order; every (position, strand) carries a record with probability 0.6 (code a) / 0.25 (code m) whatever
    the base; tiny1 and tiny3 carry dropped records only, norec none at all."""
    _, base, _, _, _, _ = geometry_input()
    rng = np.random.default_rng(SEED)
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    long_ = list(rand(40_000))
    for a in LONG_A + (LANES_SITE,):
        long_[a - 1:a + 3] = "GATC"
    norec = list(rand(3_000))
    norec[100:104] = "GATC"
    norec[2_996:3_000] = "GATC"
    end_ga = list(rand(600))
    end_ga[300:304] = "GATC"
    end_ga[-2:] = "GA"
    start_tc = list(rand(700))
    start_tc[400:404] = "GATC"
    start_tc[:2] = "TC"
    seqs = dict(base)
    seqs.update({"long": "".join(long_), "norec": "".join(norec), "endGA": "".join(end_ga), "startTC": "".join(start_tc)})
    names = list(seqs)
    records = {}
    for code, density in (("a", 0.6), ("m", 0.25)):
        for name in names:
            if name == "norec":
                continue
            L = len(seqs[name])
            p, s = np.nonzero(rng.random((L, 2)) < density)              # ascending position, '+' before '-'
            if name in ("endGA", "startTC", "tiny2"):                    # every position of the border, both strands
                p, s = np.repeat(np.arange(L), 2), np.tile(np.arange(2), L)
            n = len(p)
            nv = rng.integers(0, 31, size=n)
            u = rng.random(n)
            nm = np.where(u < 0.2, 0, np.where(u < 0.4, nv, rng.integers(0, 31, size=n) % (nv + 1)))
            nd = np.where(rng.random(n) < 0.15, rng.integers(1, 7, size=n), 0)
            nd[nv == 4] = 1                                              # 4 / (4 + 1) = 0.8 exactly: kept
            nd[(nv == 8) & (p % 2 == 0)] = 2                             # 8 / (8 + 2) = 0.8 exactly: kept
            nd[(nv == 8) & (p % 2 == 1)] = 3                             # 8 / (8 + 3): dropped
            if name in ("tiny1", "tiny3"):
                nv, nm = np.minimum(nv, 2), np.zeros(n, np.int64)        # records, none of them kept
            if name in ("endGA", "startTC", "tiny2"):
                nv, nd = np.maximum(nv, 3), np.zeros(n, np.int64)
                nm = np.minimum(nm, nv)
            st = np.where(s == 0, PLUS, MINUS).astype(np.uint8)
            if code == "a" and name == "long":
                cols = {(int(a), int(b)): (int(c), int(d), int(e)) for a, b, c, d, e in zip(p, st, nv, nm, nd)}
                for (_, pos, strand), (cov, mod) in PLANTED.items():
                    cols[(pos, strand)] = (cov, mod, 0)
                for _, pos, strand in PLANTED_SITES:
                    cols[(pos - 1, strand)] = (2, 1, 0)                  # a dropped record immediately before it
                keys = sorted(cols)
                p = np.array([k[0] for k in keys])
                st = np.array([k[1] for k in keys], dtype=np.uint8)
                nv, nm, nd = (np.array([cols[k][i] for k in keys]) for i in range(3))
            records[(name, code)] = dict(position=p.astype(np.int64), strand=st, n_valid=nv.astype(np.int64), n_mod=nm.astype(np.int64),
                                         n_diff=nd.astype(np.int64))
    for r in records.values():
        for a in r.values():
            a.setflags(write=False)
    return names, seqs, records


_FLANKS = ("", "A", "C", "G", "T", "R", "Y", "S", "W")
FAMILY = [(x + "GATC" + y, "a", len(x) + 1) for x in _FLANKS for y in _FLANKS if x or y]         # 80 reach-0 motifs around one A
GEOMETRY = list(dict.fromkeys((regex_to_iupac(m), "a", i) for m, i, _ in GEOMETRY_MOTIFS))
CODE_M = [("CCWGG", "m", 1), ("C", "m", 0), ("GATC", "m", 3), ("C" + "N" * 40 + "G", "m", 0), ("C" + "N" * 90 + "G", "m", 0),
          ("G" + "N" * 50 + "C", "m", 51)]


def request():
    """[(IUPAC motif, code, mod position)]: the reach-0 family with the geometry motifs (every fourth place) and the motifs of code m
    (every thirteenth) dealt in between, a reach-2 motif of code m in front: no motif but the first sits in its batch where it sits in
    the request, and (a, reach 0) spans three batches."""
    geo, cm = list(GEOMETRY), list(CODE_M)
    out = [cm.pop(4)]
    for i, f in enumerate(FAMILY):
        out.append(f)
        if i % 4 == 1 and geo:
            out.append(geo.pop(0))
        if i % 13 == 5 and cm:
            out.append(cm.pop(0))
    assert not geo and not cm and len(set(out)) == len(out)
    return out


def regex_triples(names):
    from nanomotif_amd.motif import iupac_to_regex
    return [(iupac_to_regex(m), code, pos) for m, code, pos in names]


def groups_of(names):
    """(code, reach class) -> indices into the request, in request order: the groups nm_contig_methylation cuts into batches of 32."""
    g = {}
    for k, (m, code, pos) in enumerate(regex_triples(names)):
        g.setdefault((code, reach_class(m, pos)), []).append(k)
    return g


@functools.lru_cache(maxsize=None)
def expected(use_diff=True):
    """{(index into request(), contig): Segment} on the geometry input."""
    _, seqs, records = meth_input()
    return brute_force(seqs, records, regex_triples(request()), use_diff=use_diff)


def n_kept_of(records, code, use_diff=True, min_cov=MIN_COV, min_frac=MIN_FRAC):
    return sum(int(kept_mask(r, min_cov, min_frac, use_diff).sum()) for (_, c), r in records.items() if c == code)


# ------------------------------------------------------------------------------------------------ the tests
def test_the_brute_force_on_a_hand_case():
    """GATC x 3: '+' A at 1, 5, 9, '-' A at 2, 6, 10.  Kept: (1 +) 10/4, (2 -) 5/5, (5 +) 8/2 with n_diff 2; dropped: (6 -) coverage 2,
    (9 +) 8 / (8 + 3); (3 +) 9/9 sits on a C."""
    col = lambda *x: np.array(x, dtype=np.int64)
    rec = {("c", "a"): dict(position=col(1, 2, 3, 5, 6, 9), strand=np.frombuffer(b"+-++-+", np.uint8), n_valid=col(10, 5, 9, 8, 2, 8),
                            n_mod=col(4, 5, 9, 2, 1, 8), n_diff=col(0, 0, 0, 2, 0, 3))}
    g = brute_force({"c": "GATC" * 3}, rec, [("GATC", "a", 1)])[(0, "c")]
    assert (g.n, g.cov_sum, g.mod_sum, g.frac) == (3, 23, 11, [0.25, 0.4, 1.0])
    assert (g.mean_read_cov, g.median, g.weighted_mean) == (23 / 3, 0.4, 11 / 23)
    g = brute_force({"c": "GATC" * 3}, rec, [("GATC", "a", 1)], use_diff=False)[(0, "c")]
    assert (g.n, g.frac, g.median) == (4, [0.25, 0.4, 1.0, 1.0], 0.7)
    assert brute_force({"c": "GATC" * 3}, rec, [("GATC", "a", 1)], min_cov=11) == {}
    assert median_of([0.5]) == 0.5 and median_of([1.0, 0.0]) == 0.5 and median_of([0.2, 0.2, 0.2]) == 0.2


def test_the_input_is_not_degenerate():
    names, seqs, records = meth_input()
    req = request()
    exp = expected()
    assert names == ["big", "tiny1", "tiny2", "tiny3", "small", "edge", "mid", "long", "norec", "endGA", "startTC"]
    assert (len(seqs["long"]), len(seqs["edge"]), len(seqs["norec"])) == (40_000, 8192, 3_000)
    n_rec = {c: sum(len(r["position"]) for (_, k), r in records.items() if k == c) for c in CODES}
    kept = {c: n_kept_of(records, c) for c in CODES}
    segs = list(exp.values())
    odd = [g for g in segs if g.n % 2]
    even = [g for g in segs if g.n % 2 == 0]
    print("motifs", len(req), "segments", len(segs), "odd", len(odd), "even", len(even), "n = 1:", sum(g.n == 1 for g in segs), "n = 2:",
          sum(g.n == 2 for g in segs), "records", n_rec, "kept", kept, "kept without the ratio filter", {c: n_kept_of(records, c, False) for c in CODES})
    assert all(0 < kept[c] < n_kept_of(records, c, False) < n_rec[c] for c in CODES)
    assert any(g.n == 1 for g in segs) and any(g.n == 2 for g in segs) and len(odd) >= 10 and len(even) >= 10
    differ = [g for g in even if g.frac[g.n // 2 - 1] != g.frac[g.n // 2]]
    print("even segments whose middle fractions differ", len(differ), "medians of 0.0:", sum(g.median == 0.0 for g in segs), "of 1.0:",
          sum(g.median == 1.0 for g in segs), "all fractions equal:", sum(g.n > 1 and g.frac[0] == g.frac[-1] for g in segs))
    assert len(differ) >= 5
    assert any(g.median == 0.0 for g in segs) and any(g.median == 1.0 for g in segs)
    assert any(g.n > 1 and g.frac[0] == g.frac[-1] for g in segs)                                   # all-equal fractions
    assert any(0.0 in g.frac and 1.0 in g.frac for g in segs)
    # the filters: 0, values below min_cov and the exact ratios all occur
    a = {k: np.concatenate([r[k] for (_, c), r in records.items() if c == "a"]) for k in ("n_valid", "n_diff", "n_mod")}
    assert (a["n_valid"] == 0).any() and ((a["n_valid"] > 0) & (a["n_valid"] < MIN_COV)).any() and a["n_valid"].max() == 30
    for nv, nd, keep in ((4, 1, True), (8, 2, True), (8, 3, False)):
        sel = (a["n_valid"] == nv) & (a["n_diff"] == nd)
        assert sel.any() and (nv / (nv + nd) >= MIN_FRAC) == keep
    assert 0.10 < (a["n_diff"] > 0).mean() < 0.25
    # rows on every contig that holds the motif and has records; none on norec (no records), tiny1 and tiny3 (dropped records only)
    gatc = req.index(("GATC", "a", 1))
    holds = [n for n in names if "GATC" in seqs[n]]
    assert holds == ["big", "small", "edge", "mid", "long", "norec", "endGA", "startTC"]
    assert [n for n in names if (gatc, n) in exp] == [n for n in holds if n != "norec"]
    assert not any(n in ("norec", "tiny1", "tiny3") for _, n in exp)
    assert ("tiny1", "a") in records and ("tiny3", "a") in records and not kept_mask(records[("tiny3", "a")]).any()
    assert (req.index(("A", "a", 0)), "tiny2") in exp
    # the planted sites carry the planted values, and the dropped rows before them shifted their rank
    r = records[("long", "a")]
    keep = kept_mask(r)
    fwd, rev = site_positions(seqs["long"], "GATC", 1)
    g = exp[(gatc, "long")]
    pairs = sorted(zip(g.cov, g.mod))
    for (_, pos, strand), (cov, mod) in PLANTED.items():
        i = int(np.flatnonzero((r["position"] == pos) & (r["strand"] == strand))[0])
        assert keep[i] and (int(r["n_valid"][i]), int(r["n_mod"][i])) == (cov, mod)
        before = (r["position"] < pos) & (r["strand"] == strand)
        assert int((before & keep).sum()) != int(before.sum())
        if ("long", pos, strand) not in PLANTED_SITES:
            continue
        assert pos in (fwd if strand == PLUS else rev) and (cov, mod) in pairs
        j = int(np.flatnonzero((r["position"] == pos - 1) & (r["strand"] == strand))[0])
        assert not keep[j] and int(r["n_valid"][j]) == 2
    assert {511, 32_767, 36_863, LANES_SITE} <= set(fwd.tolist()) and {512, 32_768, 36_864, LANES_SITE + 1} <= set(rev.tolist())
    assert 511 % 512 == 511 and 32_767 // 512 == 63 and 32_768 // 512 == 64 and 36_863 % 512 == 511 and 36_863 % 128 == 127 and 32_767 % 8192 == 8191
    assert seqs["long"][32_768] == "T"                                  # T @ 0 reads the '+' record on the first bit behind the carry
    assert [p // 128 - LANES_BLOCK // 128 for p in LANES_KEPT + (LANES_SITE,)] == [0, 1, 2, 3] and LANES_BLOCK % 512 == 0
    # the last position of a contig carries a kept record that a motif reads
    assert exp[(req.index(("A", "a", 0)), "endGA")].n == seqs["endGA"].count("A") + seqs["endGA"].count("T") and seqs["endGA"][-1] == "A"
    rr = records[("endGA", "a")]
    assert kept_mask(rr).all() and set(rr["position"][-4:].tolist()) == {598, 599} and set(records[("startTC", "a")]["position"][:4].tolist()) == {0, 1}
    # all three reach classes produce rows on big and on long
    groups = groups_of(req)
    for n in ("big", "long"):
        assert {cls for (code, cls), ks in groups.items() if code == "a" and any((k, n) in exp for k in ks)} == {0, 1, 2}
    sizes = {key: len(ks) for key, ks in groups.items()}
    print("group sizes", sizes)
    assert set(sizes) == {(c, cls) for c in CODES for cls in (0, 1, 2)} and sizes[("a", 0)] > 64 and min(sizes.values()) >= 1
    assert all(ks[j] != j for ks in groups.values() for j in range(len(ks)) if ks[j] != 0)       # batch[k] != k but for the first motif
    # no site lies across endGA | startTC, although the two together spell one
    from oracle.scan import subseq_indices
    assert len(seqs["endGA"]) - 2 in subseq_indices("GATC", seqs["endGA"] + seqs["startTC"]).tolist()
    fwd, _ = site_positions(seqs["endGA"], "GATC", 1)
    _, rev = site_positions(seqs["startTC"], "GATC", 1)
    assert len(seqs["endGA"]) - 1 not in fwd.tolist() and 0 not in rev.tolist()
    for n in ("endGA", "startTC"):                                       # every position carries a kept record: both strands of every whole site
        assert exp[(gatc, n)].n == 2 * seqs[n].count("GATC") > 0


def test_the_brute_force_agrees_with_the_restated_oracle():
    """``oracle.contig_methylation.read_methylation`` (np.isin over regex matches) and the brute force above (dense per-position tables)
    give the same rows on the geometry input: the whole request as medians, its head as weighted means and under other read filters."""
    from oracle.contig_methylation import read_methylation
    _, seqs, records = meth_input()
    req = request()
    triples = regex_triples(req)
    old = read_methylation(records, seqs, triples, MIN_COV, MIN_FRAC, "median")
    got = [(r["contig"],) + req[r["motif"]] + (r["methylation_value"], r["mean_read_cov"], r["n_motif_obs"]) for r in old]
    assert got == rows_of(expected(), seqs, req, "median") and len(got) > 500
    sub = req[:24]                                                       # (the sums differ from the medians in the last step only)
    old = read_methylation(records, seqs, regex_triples(sub), MIN_COV, MIN_FRAC, "weighted-mean")
    got = [(r["contig"],) + sub[r["motif"]] + (r["methylation_value"], r["mean_read_cov"], r["n_motif_obs"]) for r in old]
    assert got == rows_of(expected(), seqs, sub, "weighted-mean")
    sub = req[:12]
    old = read_methylation(records, seqs, regex_triples(sub), 12, 0.95, "median")
    got = [(r["contig"],) + sub[r["motif"]] + (r["methylation_value"], r["mean_read_cov"], r["n_motif_obs"]) for r in old]
    assert got == rows_of(brute_force(seqs, records, regex_triples(sub), 12, 0.95), seqs, sub, "median")


def swapped_strands(records):
    """The same records with '+' and '-' exchanged."""
    return {k: dict(r, strand=np.where(r["strand"] == PLUS, MINUS, PLUS).astype(np.uint8)) for k, r in records.items()}


def test_identities_hold_in_the_brute_force():
    """A motif reads on '+' what its reverse complement with the mirrored mod position reads on '-': the two give identical rows once the
    strands of the records are exchanged (and different ones on the same records); the one-letter motifs partition the kept records
    that sit on a base."""
    from oracle.motif import Motif as OMotif
    _, seqs, records = meth_input()
    other = swapped_strands(records)
    for m, pos in (("GAAG", 1), ("A" + "." * 40 + "C", 0), ("[AG]GATC", 2)):
        rc = OMotif(m, pos).reverse_compliment()
        a = brute_force(seqs, records, [(m, "a", pos)])
        b = brute_force(seqs, other, [(rc.string, "a", rc.mod_position)])
        assert a.keys() == b.keys() and len(a) >= 4
        assert all((a[k].frac, a[k].cov_sum, a[k].mod_sum) == (b[k].frac, b[k].cov_sum, b[k].mod_sum) for k in a)
        c = brute_force(seqs, records, [(rc.string, "a", rc.mod_position)])
        assert any(a[k].frac != c[k].frac for k in a)
    one = brute_force(seqs, records, [(b, "a", 0) for b in "ACGT"])
    assert sum(g.n for g in one.values()) == n_kept_of(records, "a") - kept_on_n(seqs, records, "a")
    assert kept_on_n(seqs, records, "a") > 0


def kept_on_n(seqs, records, code):
    """Kept records of ``code`` that sit on an N of the assembly."""
    n = 0
    for (name, c), r in records.items():
        if c == code:
            is_n = np.frombuffer(seqs[name].encode(), np.uint8) == ord("N")
            n += int(is_n[r["position"][kept_mask(r)]].sum())
    return n
