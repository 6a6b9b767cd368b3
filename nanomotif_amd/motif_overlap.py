"""``nanomotif motif_overlap``: how the motifs of one bin RELATE on the sequence — which sites two motifs share, which motif's sites
lie inside another's, and how methylated a motif is OUTSIDE the motifs nested in it.

Discovery routinely leaves ``GATC`` beside ``RGATCY``, ``CCWGG`` beside ``CCAGG``, or two half-overlapping spellings of one
methyltransferase's site.  The reference settles these by the motifs' spelling (``remove_sub_motifs`` / ``merge_motifs``,
postprocess.py).  What decides such a case is a count no marginal gives: ``GATC`` at 60 % with ``RGATCY`` at 98 % and ``GATC`` outside
``RGATCY`` at 15 % is a spurious parent; ``GATC`` outside ``RGATCY`` at 97 % makes ``RGATCY`` a redundant sub-motif.  This command
reports; it does not rewrite ``bin-motifs.tsv``.

Definition.  A site of a candidate is a (contig, position of the modified base, strand) that ``motif_sites`` writes with all three
states; two motifs of one (bin, mod type) share a site when both have it.  The state belongs to the position, so a shared site has
one state and ``a_only = own_a - shared`` is exact per state.  Pairs are formed inside one (bin, mod type) only.  As everywhere in the
engine a motif is read without its leading and trailing ``N``: ``GATCN`` IS ``GATC``.

Arguments, ingest and candidates are those of ``motif_sites`` (complements included, duplicates dropped); sets are (bin, mod type)
as ``motif_coverage.build_sets`` orders them, motifs in file order.  Two engine calls (``ScanEngine.motif_overlap``):
  1. every motif with all other motifs of its set as partners: the pair table — twice, through different walk orders and widths;
     the command checks that it is symmetric and fails loudly if not — and, as the rest, the sites only this motif has;
  2. every motif that has a child, with exactly its children as partners: the rest is the parent outside the union of its children
     (children may overlap each other: no inclusion-exclusion gives this).

Files (tab-separated, header line; pooled over contigs and strands):
  ``motif-overlap.tsv``         one row per unordered pair (a before b in set order) with a shared site, with ``--all_pairs`` the
                                disjoint ones too: ``n_a`` / ``n_b`` (sites in any state), the shared sites by state, ``share_of_a`` =
                                shared / n_a, ``share_of_b``, ``jaccard``; ``frac_mod_shared`` / ``frac_mod_a_only`` /
                                ``frac_mod_b_only`` = mod / (mod + nomod) of the three parts, each with its called count;
                                ``relation`` by counts, exactly: ``identical``, ``a_in_b`` (shared == n_a < n_b), ``b_in_a``,
                                ``overlapping``, ``disjoint``, ``no_sites`` when either motif has none; ``symbolic``: the same question
                                answered from the IUPAC sets aligned on the modified base, positions outside a motif counted as N:
                                ``a_in_b`` / ``b_in_a`` / ``identical`` / ``none``
  ``motif-overlap-motifs.tsv``  one row per motif: its counts, ``n_overlapping`` (partners with a shared site), ``children`` /
                                ``parents`` / ``duplicates`` by counts (names joined with ``,``), ``n_mod_only`` / ``n_nomod_only`` (sites
                                no other motif of the set has), the counts and ``frac_mod_outside_children`` outside the union of its
                                children (its own, without children), ``frac_mod_in_children`` and ``flag``, the first that applies of
                                ``few_sites`` (called < ``--min_called``), ``duplicate`` (identical to an earlier motif of the set),
                                ``carried_by_children`` (children, at least ``--min_called`` called sites outside them,
                                frac_mod_outside_children <= ``--max_outside`` and frac_mod_in_children >= ``--min_frac``),
                                ``submotif`` (some parent p has at least ``--min_called`` called sites in p \\ this and frac_mod(p \\ this)
                                >= ``--min_frac``), ``none``

Fractions are ``%.6f``, ``nan`` for 0 / 0.  ``--max_outside`` 0.3 and ``--min_frac`` 0.7 are the pileup's call thresholds reused, and
``--min_called`` 20 is the neighbouring commands': design choices, pinned on hand-made tables (``tests/test_motif_overlap_host.py``),
not on real data.
"""
from __future__ import annotations

import os
import time

import numpy as np

from .export_run import closing, finish, open_run, resident_bins, split_known, table_text, write_texts
from .loading import kept_mod_types
from .motif import ANY, Motif, iupac_to_regex
from .motif_coverage import build_sets

PAIRS_NAME = "motif-overlap.tsv"
MOTIFS_NAME = "motif-overlap-motifs.tsv"
PAIRS_HEADER = ["bin", "mod_type", "motif_a", "mod_position_a", "motif_b", "mod_position_b", "n_a", "n_b", "shared_mod", "shared_nomod", "shared_nocall",
                "share_of_a", "share_of_b", "jaccard", "frac_mod_shared", "called_shared", "frac_mod_a_only", "called_a_only", "frac_mod_b_only",
                "called_b_only", "relation", "symbolic"]
MOTIFS_HEADER = ["bin", "mod_type", "motif", "mod_position", "n_mod", "n_nomod", "n_nocall", "n_overlapping", "children", "parents", "duplicates", "n_mod_only",
                 "n_nomod_only", "n_mod_outside_children", "n_nomod_outside_children", "frac_mod_outside_children", "frac_mod_in_children", "flag"]
RELATIONS = ("identical", "a_in_b", "b_in_a", "overlapping", "disjoint", "no_sites")
SYMBOLIC = ("identical", "a_in_b", "b_in_a", "none")
FLAGS = ("few_sites", "duplicate", "carried_by_children", "submotif", "none")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_overlap.json)


def ratio_text(num: int, den: int) -> str:
    """num / den as ``%.6f``; ``nan`` for 0 / 0 (and for any empty denominator)."""
    return "%.6f" % (int(num) / int(den)) if int(den) else "nan"


def frac_mod(three) -> float:
    """mod / (mod + nomod) of (mod, nomod, nocall); nan when nothing is called."""
    called = int(three[0]) + int(three[1])
    return int(three[0]) / called if called else float("nan")


def relation(n_a: int, n_b: int, shared: int) -> str:
    """How the site sets of a and b relate, decided by counts alone (sites in any state)."""
    n_a, n_b, shared = int(n_a), int(n_b), int(shared)
    if n_a == 0 or n_b == 0:
        return "no_sites"
    if shared == 0:
        return "disjoint"
    if shared == n_a == n_b:
        return "identical"
    if shared == n_a:
        return "a_in_b"
    if shared == n_b:
        return "b_in_a"
    return "overlapping"


def aligned_sets(motif: str, mod_position: int) -> dict:
    """offset from the modified base -> base set (4-bit mask) of an IUPAC motif, N left out."""
    sets, mp = Motif(iupac_to_regex(motif), int(mod_position)).stripped_sets()
    return {j - int(mp): int(m) for j, m in enumerate(sets.tolist()) if int(m) != ANY}


def symbolic(a, b) -> str:
    """The nesting of two candidates (``SiteCandidate``: ``motif``, ``mod_position``) read off their IUPAC sets aligned on the modified
    base, positions outside a motif counted as N: ``a_in_b`` when every sequence a matches b matches too."""
    sa, sb = aligned_sets(a.motif, a.mod_position), aligned_sets(b.motif, b.mod_position)
    a_in_b = all((sa.get(d, ANY) & ~m) == 0 for d, m in sb.items())
    b_in_a = all((sb.get(d, ANY) & ~m) == 0 for d, m in sa.items())
    return "identical" if a_in_b and b_in_a else "a_in_b" if a_in_b else "b_in_a" if b_in_a else "none"


def pooled(table) -> np.ndarray:
    """int64[P + 2, n_contigs, 2, 3] of one candidate -> int64[P + 2, 3] over contigs and strands."""
    t = np.asarray(table, dtype=np.int64)
    return t.reshape(t.shape[0], -1, 3).sum(axis=1)


class SetStats:
    """The pair table of one set of n motifs, pooled: ``own`` int64[n, 3] (mod, nomod, nocall), ``shared`` int64[n, n, 3] (the diagonal is
    ``own``), ``only`` int64[n, 3] (sites no other motif of the set has), ``outside`` int64[n, 3] (outside the union of its children;
    ``own`` without children, filled by ``add_outside``)."""

    def __init__(self, own, shared, only):
        self.own, self.shared, self.only = own, shared, only
        self.outside = own.copy()

    def __len__(self):
        return len(self.own)


def set_stats(tables, names=None) -> SetStats:
    """``tables[i]``: the int64[n + 1, n_contigs, 2, 3] of motif i of a set of n with ALL OTHER motifs of the set as partners, in set
    order (``ScanEngine.motif_overlap``).  The pair table comes out twice — (i, j) from i's walk, (j, i) from j's; a difference, on any
    contig, strand or state, is a RuntimeError naming the pair."""
    n = len(tables)
    names = names or [str(i) for i in range(n)]
    full = [np.asarray(t, dtype=np.int64) for t in tables]
    own = np.zeros((n, 3), dtype=np.int64)
    only = np.zeros((n, 3), dtype=np.int64)
    shared = np.zeros((n, n, 3), dtype=np.int64)
    block = lambda i, j: full[i][1 + (j if j < i else j - 1)]             # i's partners: the set without i
    for i in range(n):
        if full[i].shape[0] != n + 1:
            raise ValueError(f"motif {names[i]}: {full[i].shape[0]} blocks for a set of {n}")
        p = pooled(full[i])
        own[i], only[i], shared[i, i] = p[0], p[n], p[0]
        for j in range(n):
            if j != i:
                shared[i, j] = p[1 + (j if j < i else j - 1)]
    for i in range(n):
        for j in range(i + 1, n):
            if not np.array_equal(block(i, j), block(j, i)):
                raise RuntimeError(f"motif_overlap: the pair table is not symmetric: {names[i]} shares {shared[i, j].tolist()} (mod, nomod, nocall) with "
                                   f"{names[j]}, {names[j]} shares {shared[j, i].tolist()} with {names[i]}")
    return SetStats(own, shared, only)


def nesting(st: SetStats):
    """(children, parents, duplicates): per motif the indices of the motifs of its set nested in it, it is nested in, and identical to
    it — by counts (``relation``)."""
    n = len(st)
    tot, sh = st.own.sum(axis=1), st.shared.sum(axis=2)
    children, parents, duplicates = ([[] for _ in range(n)] for _ in range(3))
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            r = relation(tot[i], tot[j], sh[i, j])
            if r == "b_in_a":
                children[i].append(j)
            elif r == "a_in_b":
                parents[i].append(j)
            elif r == "identical":
                duplicates[i].append(j)
    return children, parents, duplicates


def add_outside(st: SetStats, children, tables):
    """``tables``: index of a motif that has children -> its int64[len(children) + 2, n_contigs, 2, 3] with exactly its children as
    partners; the rest block is the motif outside the union of its children."""
    for i, t in tables.items():
        p = pooled(t)
        if p.shape[0] != len(children[i]) + 2 or not np.array_equal(p[0], st.own[i]):
            raise RuntimeError(f"motif_overlap: the table of motif {i} against its children does not belong to it")
        st.outside[i] = p[-1]


def flag_of(i: int, st: SetStats, children, parents, duplicates, min_called=20, max_outside=0.3, min_frac=0.7) -> str:
    """The flag of motif i of a set: the first that applies of few_sites, duplicate, carried_by_children, submotif, none."""
    called = lambda three: int(three[0]) + int(three[1])
    if called(st.own[i]) < int(min_called):
        return "few_sites"
    if any(j < i for j in duplicates[i]):
        return "duplicate"
    inside = st.own[i] - st.outside[i]
    if children[i] and called(st.outside[i]) >= int(min_called) and frac_mod(st.outside[i]) <= float(max_outside) and called(inside) \
            and frac_mod(inside) >= float(min_frac):
        return "carried_by_children"
    for p in parents[i]:
        rest = st.own[p] - st.shared[p, i]
        if called(rest) >= int(min_called) and frac_mod(rest) >= float(min_frac):
            return "submotif"
    return "none"


def format_pairs(sets, stats, all_pairs=False) -> str:
    """motif-overlap.tsv of ``sets`` (``motif_coverage.CoverageSet``) and their ``SetStats``."""
    rows = []
    for s, st in zip(sets, stats):
        tot = st.own.sum(axis=1)
        for i in range(len(st)):
            for j in range(i + 1, len(st)):
                a, b, sh = s.candidates[i], s.candidates[j], st.shared[i, j]
                n_sh = int(sh.sum())
                rel = relation(tot[i], tot[j], n_sh)
                if n_sh == 0 and not all_pairs:
                    continue
                a_only, b_only = st.own[i] - sh, st.own[j] - sh
                parts = []
                for three in (sh, a_only, b_only):
                    parts += [ratio_text(three[0], three[0] + three[1]), int(three[0] + three[1])]
                rows.append([s.bin, s.mod_type, a.motif, a.mod_position, b.motif, b.mod_position, int(tot[i]), int(tot[j])] + [int(x) for x in sh] +
                            [ratio_text(n_sh, tot[i]), ratio_text(n_sh, tot[j]), ratio_text(n_sh, tot[i] + tot[j] - n_sh)] + parts + [rel, symbolic(a, b)])
    return table_text(PAIRS_HEADER, rows)


def format_motifs(sets, stats, min_called=20, max_outside=0.3, min_frac=0.7) -> str:
    """motif-overlap-motifs.tsv of ``sets`` and their ``SetStats`` (``outside`` filled in)."""
    rows = []
    for s, st in zip(sets, stats):
        children, parents, duplicates = nesting(st)
        sh = st.shared.sum(axis=2)
        for i, c in enumerate(s.candidates):
            named = lambda idx: ",".join(s.candidates[j].name for j in idx)
            out, inside = st.outside[i], st.own[i] - st.outside[i]
            rows.append([c.bin, c.mod_type, c.motif, c.mod_position] + [int(x) for x in st.own[i]] +
                        [sum(1 for j in range(len(st)) if j != i and sh[i, j] > 0), named(children[i]), named(parents[i]), named(duplicates[i]),
                         int(st.only[i][0]), int(st.only[i][1]), int(out[0]), int(out[1]), ratio_text(out[0], out[0] + out[1]),
                         ratio_text(inside[0], inside[0] + inside[1]), flag_of(i, st, children, parents, duplicates, min_called, max_outside, min_frac)])
    return table_text(MOTIFS_HEADER, rows)


def overlap_stats(eng, sets) -> list:
    """The ``SetStats`` of ``sets`` from the two engine calls of this command."""
    flat, partners, where = [], [], []
    for si, s in enumerate(sets):
        motifs = [c.engine_candidate()[0] for c in s.candidates]
        for i, c in enumerate(s.candidates):
            flat.append(c.engine_candidate())
            partners.append(motifs[:i] + motifs[i + 1:])
            where.append(si)
    per_set = [[] for _ in sets]
    for si, (_, t) in zip(where, eng.motif_overlap(flat, partners)):
        per_set[si].append(t)
    stats = [set_stats(t, [c.name for c in s.candidates]) for s, t in zip(sets, per_set)]
    flat, partners, where = [], [], []
    kids = [nesting(st)[0] for st in stats]
    for si, s in enumerate(sets):
        motifs = [c.engine_candidate()[0] for c in s.candidates]
        for i, c in enumerate(s.candidates):
            if kids[si][i]:
                flat.append(c.engine_candidate())
                partners.append([motifs[j] for j in kids[si][i]])
                where.append((si, i))
    outside = [{} for _ in sets]
    for (si, i), (_, t) in zip(where, eng.motif_overlap(flat, partners)):
        outside[si][i] = t
    for st, ch, tables in zip(stats, kids, outside):
        add_outside(st, ch, tables)
    return stats


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    eng, cands, status = open_run("motif_overlap", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        mod_types = kept_mod_types(eng)
        sets = [s for s in build_sets(resident_bins(eng), mod_types, split_known(cands, eng, mod_types)) if s.candidates]
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        stats = overlap_stats(eng, sets)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        write_texts(args.out, (PAIRS_NAME, MOTIFS_NAME), (format_pairs(sets, stats, bool(args.all_pairs)),
                                                          format_motifs(sets, stats, int(args.min_called), float(args.max_outside), float(args.min_frac))))
        finish("motif_overlap", TIMINGS, t_eng, time.perf_counter() - t0, sets=len(sets), candidates=sum(len(s.candidates) for s in sets),
               pairs=sum(len(s.candidates) * (len(s.candidates) - 1) // 2 for s in sets))
    return 0
