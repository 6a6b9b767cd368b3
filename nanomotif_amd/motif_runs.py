"""``nanomotif motif_runs``: RUNS OF SAME-STATE SITES of the motifs of a ``bin-motifs.tsv`` along the contigs — the ORDER of a motif's
sites, which none of the other exports looks at.  A protein that sits on the DNA protects its sites from the methyltransferase:
footprints of three to ten consecutive unmethylated GATC in an otherwise methylated genome are how regulatory regions and phase-variable
operons show in a pileup.  The other tail is a caller with a strand bias, which makes the states of a palindrome alternate.

Definition.  A candidate is (bin, motif, mod_type, mod_position); its sites and their states (mod / nomod / nocall) are those of
``motif_sites`` (same ingest, ``loading.load_engine``).  On one contig the sites of both strands are taken by ascending position of the
modified base.  The SEQUENCE is the called sites (mod, nomod): a nocall site is transparent, it neither extends nor breaks anything; with
``--nocall_breaks`` all three states take part and a nocall site ends a run like any change of state.  A RUN is a maximal stretch of
consecutive sequence elements of one state within one contig (``ScanEngine.motif_run_counts`` / ``motif_runs``, nm_motif_runs_*).

Every bin with a contig also gets its background, the one-letter candidates "every A" / "every C" per mod type of the pileup, in the same
engine calls: without it "clustered" means nothing.

Files (tab-separated, header line; candidates in file order):
  ``motif-runs.tsv``          per candidate: ``n_mod`` / ``n_nomod`` / ``n_nocall`` sites, ``frac_mod``, the runs (``runs_mod`` /
                              ``runs_nomod``), the longest (``longest_mod`` / ``longest_nomod``) and the mean run length per state;
                              the Wald-Wolfowitz runs test on the called sequence with n1 mod, n2 nomod, n = n1 + n2:
                              mu = 1 + 2 n1 n2 / n, var = 2 n1 n2 (2 n1 n2 - n) / (n^2 (n - 1)).  ``expected_runs`` = mu and ``runs_z`` are
                              taken on the totals as if they were one sequence; ``runs_z_within`` = (sum R_c - sum mu_c) /
                              sqrt(sum var_c) over the contigs that have both outcomes — ``motif_gc``'s argument: a contaminant contig of
                              another methylation level must not pass as clustering; ``runs_p`` = erfc(|z_within| / sqrt 2);
                              ``bg_runs_z_within``: the same of the bin's background in the candidate's mod type; ``flag`` =
                              ``few_sites`` below ``--min_called`` called sites, ``clustered`` when runs_z_within <= -``--min_z``,
                              ``alternating`` when >= +``--min_z``, else ``none``
  ``motif-runs-contigs.tsv``  the same per (candidate, contig); runs_z_within is that contig's z (0 with one outcome only)
  ``motif-runs-hist.tsv``     long form, per candidate, state and run length: the non-zero cells; the last bucket is labelled ``R+``
  ``motif-runs-bins.tsv``     the background rows (every A / every C per bin and mod type), with the columns of motif-runs.tsv
  ``motif-runs.bed``          (``--runs``) one line per run whose state is in ``--states`` (default nomod) and that holds at least
                              ``--min_run`` (default 3) sites: contig, start, end = last + 1, motif_modtype_modposition, n_sites, ``.``,
                              state, bin

With ``--nocall_breaks`` the runs test is still taken on the mod / nomod runs AS COUNTED: a nocall site between two methylated sites
makes two mod runs of them, so R grows against the mu of the called sites and the statistic leans towards ``alternating``.

``--min_z`` 5 is ``motif_gc``'s, reused as a design choice: it is pinned on hand-made tables (``tests/test_motif_runs_host.py``), not on
real data.
"""
from __future__ import annotations

import logging as log
import os
import time

import numpy as np

from . import fasta
from .engine import RUNS_MAX_MAX_RUN, RUNS_MIN_MAX_RUN, SITE_STATES
from .export_run import background_candidates, bin_mod_keys, closing, finish, frac_text, open_run, parse_int_in, split_known, table_text, write_texts
from .loading import kept_mod_types
from .motif import MOD_TYPE_TO_CANONICAL
from .motif_gc import trend_p, z_of
from .motif_sites import parse_states

MAIN_NAME = "motif-runs.tsv"
CONTIGS_NAME = "motif-runs-contigs.tsv"
HIST_NAME = "motif-runs-hist.tsv"
BINS_NAME = "motif-runs-bins.tsv"
BED_NAME = "motif-runs.bed"
KEY_COLUMNS = ["bin", "motif", "mod_type", "mod_position"]
STAT_COLUMNS = ["n_mod", "n_nomod", "n_nocall", "frac_mod", "runs_mod", "runs_nomod", "longest_mod", "longest_nomod", "mean_run_mod", "mean_run_nomod",
                "expected_runs", "runs_z", "runs_z_within", "runs_p", "bg_runs_z_within", "flag"]
MAIN_HEADER = KEY_COLUMNS + STAT_COLUMNS
CONTIGS_HEADER = KEY_COLUMNS + ["contig"] + STAT_COLUMNS
HIST_HEADER = KEY_COLUMNS + ["state", "run_length", "runs"]
FLAGS = ("none", "clustered", "alternating", "few_sites")
TIMINGS = {}          # seconds per phase of the last run in this process (written to OUT/logs/timings.motif_runs.json)


def parse_max_run(value) -> int:
    """``--max_run``: an integer in 2..64; ValueError otherwise."""
    return parse_int_in("--max_run", value, RUNS_MIN_MAX_RUN, RUNS_MAX_MAX_RUN)


def parse_min_run(value) -> int:
    """``--min_run``: an integer of at least 1; ValueError otherwise."""
    return parse_int_in("--min_run", value, 1)


def parse_run_states(text) -> tuple:
    """``--states``: ``motif_sites.parse_states`` (whether nocall may be asked for depends on ``--nocall_breaks``: ``run`` checks)."""
    return parse_states(text)


def runs_terms(n1: int, n2: int):
    """(mu, var) of the number of runs of a sequence of n1 and n2 elements of two kinds under the Wald-Wolfowitz null; (0, 0) when one
    kind is missing (the number of runs is not random then)."""
    n1, n2 = int(n1), int(n2)
    n = n1 + n2
    if n1 == 0 or n2 == 0:
        return 0.0, 0.0
    return 1.0 + 2.0 * n1 * n2 / n, 2.0 * n1 * n2 * (2.0 * n1 * n2 - n) / (float(n) * n * (n - 1))


def runs_z(n1: int, n2: int, runs: int) -> float:
    """The runs statistic of one sequence; 0 when it is undefined."""
    mu, var = runs_terms(n1, n2)
    return z_of(int(runs) - mu, var)


def runs_z_within(rows) -> float:
    """The statistic with R, mu and var summed per contig — ``rows``: (n1, n2, runs) per contig — over the contigs that have both
    outcomes."""
    r_sum = mu_sum = var_sum = 0.0
    for n1, n2, runs in rows:
        if int(n1) > 0 and int(n2) > 0:
            mu, var = runs_terms(n1, n2)
            r_sum += int(runs)
            mu_sum += mu
            var_sum += var
    return z_of(r_sum - mu_sum, var_sum)


def flag_of(n_called: int, z_within: float, min_called=20, min_z=5.0) -> str:
    if int(n_called) < int(min_called):
        return "few_sites"
    if z_within <= -float(min_z):
        return "clustered"
    if z_within >= float(min_z):
        return "alternating"
    return "none"


def mean_text(sites: int, runs: int) -> str:
    return "%.3f" % (int(sites) / int(runs)) if int(runs) else ""


def stat_columns(table, bg_z, min_called=20, min_z=5.0) -> list:
    """The ``STAT_COLUMNS`` of one candidate or one contig.  ``table``: int64[n_contigs, 3, 3 + R]; ``bg_z``: the text of the
    background's runs_z_within."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, 3, np.shape(table)[-1])
    sites, runs = t[:, :, 1].sum(axis=0), t[:, :, 0].sum(axis=0)
    longest = t[:, :, 2].max(axis=0) if len(t) else np.zeros(3, dtype=np.int64)
    n1, n2 = int(sites[0]), int(sites[1])
    mu, _ = runs_terms(n1, n2)
    z = runs_z(n1, n2, int(runs[0] + runs[1]))
    zw = runs_z_within([(int(c[0, 1]), int(c[1, 1]), int(c[0, 0] + c[1, 0])) for c in t])
    return [n1, n2, int(sites[2]), frac_text(n1, n2), int(runs[0]), int(runs[1]), int(longest[0]), int(longest[1]), mean_text(n1, runs[0]), mean_text(n2, runs[1]),
            "%.3f" % mu, "%.3f" % z, "%.3f" % zw, "%.3e" % trend_p(zw), bg_z, flag_of(n1 + n2, zw, min_called, min_z)]


def hist_rows(key, table) -> list:
    """The rows of one candidate in motif-runs-hist.tsv: the non-zero cells of its histogram over contigs."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, 3, np.shape(table)[-1]).sum(axis=0)
    r = t.shape[-1] - 3
    return [list(key) + [SITE_STATES[s], f"{r}+" if j == r - 1 else j + 1, int(t[s, 3 + j])] for s in range(3) for j in range(r) if t[s, 3 + j]]


def format_files(cands, results, bg_keys, bg_results, min_called=20, min_z=5.0):
    """(motif-runs.tsv, motif-runs-contigs.tsv, motif-runs-hist.tsv, motif-runs-bins.tsv) as text.  ``cands``: ``SiteCandidate`` in file
    order with ``results`` = their (contig names, int64[n_contigs, 3, 3 + R]) of ``ScanEngine.motif_run_counts``; ``bg_keys`` = [(bin,
    mod type)] with ``bg_results``, the same of the one-letter candidates."""
    bg_z, bins_rows = {}, []
    for (b, mt), (_, t) in zip(bg_keys, bg_results):
        cols = stat_columns(t, "", min_called, min_z)
        bg_z[(b, mt)] = cols[STAT_COLUMNS.index("runs_z_within")]
        bins_rows.append([b, MOD_TYPE_TO_CANONICAL[mt], mt, 0] + cols)
    main_rows, contigs_rows, hist = [], [], []
    for c, (names, t) in zip(cands, results):
        key = [c.bin, c.motif, c.mod_type, c.mod_position]
        bz = bg_z.get((c.bin, c.mod_type), "")
        main_rows.append(key + stat_columns(t, bz, min_called, min_z))
        for name, row in zip(names, t):
            contigs_rows.append(key + [fasta.original_name(name)] + stat_columns(row[None], bz, min_called, min_z))
        hist += hist_rows(key, t)
    return table_text(MAIN_HEADER, main_rows), table_text(CONTIGS_HEADER, contigs_rows), table_text(HIST_HEADER, hist), table_text(MAIN_HEADER, bins_rows)


def format_runs(records, cands, contig_names) -> str:
    """The lines of motif-runs.bed for ``records`` (``engine.RUN_DTYPE``; ``candidate`` indexes ``cands``): contig, start, end,
    motif_modtype_modposition, n_sites, ``.``, state, bin."""
    out = []
    for cand, contig, pos, code, last, n in zip(*(records[f].tolist() for f in ("candidate", "contig", "pos", "code", "last", "n_sites"))):
        c = cands[cand]
        out.append(f"{contig_names[contig]}\t{pos}\t{last + 1}\t{c.name}\t{n}\t.\t{SITE_STATES[code]}\t{c.bin}\n")
    return "".join(out)


def write_run_batches(batches, cands, contig_names, bed_file) -> int:
    """The batch-to-BED loop, as ``motif_sites.write_site_batches`` has it: the batches are written as they arrive.  Returns the records."""
    n = 0
    for sb in batches:
        bed_file.write(format_runs(sb.records, cands, contig_names))
        n += len(sb.records)
    return n


def run(args) -> int:
    """The command.  Returns the process's exit status."""
    max_run, min_run = parse_max_run(args.max_run), parse_min_run(args.min_run)
    states = args.states if isinstance(args.states, tuple) else parse_run_states(args.states)
    nocall_breaks = bool(args.nocall_breaks)
    if args.runs and "nocall" in states and not nocall_breaks:
        log.error("motif_runs: --states nocall needs --nocall_breaks (a nocall site is transparent without it)")
        return 2
    eng, cands, status = open_run("motif_runs", args, TIMINGS)
    if eng is None:
        return status
    with closing(eng):
        mod_types = kept_mod_types(eng)
        known = split_known(cands, eng, mod_types)
        bg_keys = bin_mod_keys(eng, mod_types)
        os.makedirs(args.out, exist_ok=True)
        t0 = time.perf_counter()
        # the background's one-letter candidates ride in the same engine calls as the motifs
        engine_cands = [c.engine_candidate() for c in known] + background_candidates(bg_keys)
        results = eng.motif_run_counts(engine_cands, max_run=max_run, nocall_breaks=nocall_breaks)
        n = len(known)
        n_records = 0
        if args.runs:
            contig_names = [fasta.original_name(x) for x in eng.contig_names]
            with open(os.path.join(args.out, BED_NAME), "w") as bed:
                n_records = write_run_batches(eng.motif_runs(engine_cands[:n], states=states, min_run=min_run, nocall_breaks=nocall_breaks), known, contig_names, bed)
        t_eng = time.perf_counter() - t0
        t0 = time.perf_counter()
        write_texts(args.out, (MAIN_NAME, CONTIGS_NAME, HIST_NAME, BINS_NAME),
                    format_files(known, results[:n], bg_keys, results[n:], int(args.min_called), float(args.min_z)))
        finish("motif_runs", TIMINGS, t_eng, time.perf_counter() - t0, candidates=n, background_candidates=len(bg_keys), max_run=max_run, runs=n_records)
    return 0
