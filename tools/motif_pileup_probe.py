"""Measurements of the per-site read counts (tools/gpu_motif_pileup.sh; results: profiles/r26/motif_pileup.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_pileup` with and without --all_occurrences, one cold process each; wall clocks,
               the split the command records (ingest / engine / text), the lines and bytes of the two files
  trace DIR    one process on the files of DIR with the state planes AND the read statistics resident, REPS repetitions each on the
               candidates of bin-motifs.tsv: `motif_fractions` at 20 bins (fractions_kernel: the yardstick of the count pass — the same
               prologue, and it gathers every site's values), `motif_pileup_counts` (pileup_kernel<G, false>), `motif_sites` of all three
               states (sites_kernel<G, true>: the yardstick of the fill pass — every occurrence a record of three columns) and
               `motif_pileup` of sites and bare occurrences (pileup_kernel<G, true>: every occurrence a record of five columns, a gather
               per site); the count tables and the records' positions are compared first
  table CSV    no GPU: the kernel trace of the `trace` run, per kernel the number of dispatches and the median, least and largest
               duration in microseconds
One JSON line per mode on stdout.  NM_LIB=<path> runs `files` and `trace` on another build of the library."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motif_compare_probe import cli      # noqa: E402  (the same directory)
from motif_fractions_probe import load   # noqa: E402

REPS = 5
PILEUP = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "pu"]
NAMES = ("motif-pileup.bed", "motif-pileup-summary.tsv")
KERNELS = ("pileup_kernel", "fractions_kernel", "sites_kernel")


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
    for what, more in (("sites", []), ("sites_again", []), ("all_occurrences", ["--all_occurrences"])):
        wall = cli(tmp, "motif_pileup", PILEUP + more)
        t = json.load(open(os.path.join(tmp, "pu", "logs", "timings.motif_pileup.json")))
        with open(os.path.join(tmp, "pu", NAMES[0]), "rb") as f:
            lines = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b""))
        out["motif_pileup_" + what] = dict(wall_s=wall, **t, bed_lines=lines, out_bytes={n: os.path.getsize(os.path.join(tmp, "pu", n)) for n in NAMES})
    return out


def trace(tmp):
    eng, cands, ingest_s, readstats_s, kept = load(tmp, "pileup.bed")
    flat = [c.engine_candidate() for c in cands]
    out = {"mode": "trace", "lib": os.environ.get("NM_LIB", ""), "ingest_s": ingest_s, "readstats_s": readstats_s, "kept": kept, "candidates": len(cands),
           "reps": REPS}
    both = ("site", "bare")
    calls = [("motif_fractions_b20", lambda: list(eng.motif_fractions(flat, bins=20))),
             ("motif_pileup_counts", lambda: eng.motif_pileup_counts(flat)),
             ("motif_sites", lambda: np.concatenate([sb.records for sb in eng.motif_sites(flat)])),
             ("motif_pileup", lambda: np.concatenate([sb.records for sb in eng.motif_pileup(flat, select=both)]))]
    res = {}
    for name, fn in calls:
        ts = []
        for rep in range(REPS):
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    # equality first: the four counts against the fractions table, the records' places against motif_sites'
    four = np.concatenate([t for _, t in res["motif_pileup_counts"]])
    fr = np.concatenate([t for _, _, t in res["motif_fractions_b20"]]).astype(np.int64)
    sites, pile = res["motif_sites"], res["motif_pileup"]
    out.update(occurrences=int(four.sum()), sites=int(four[:, [0, 2]].sum()), records=int(len(pile)),
               counts_equal=bool(np.array_equal(four[:, [0, 2]], fr[:, :, :20].sum(axis=2)) and np.array_equal(four[:, [0, 2]] + four[:, [1, 3]], fr[:, :, 20])),
               places_equal=bool(len(sites) == len(pile) and all(np.array_equal(sites[f], pile[f]) for f in ("candidate", "contig", "pos")) and
                                 np.array_equal(sites["code"] & 4, pile["code"] & 4)),
               sums_equal=bool(int(pile["n_valid"].sum(dtype=np.int64)) == int(fr[:, :, 21].sum()) and int(pile["n_mod"].sum(dtype=np.int64)) == int(fr[:, :, 22].sum())))
    eng.close()
    return out


def table(path):
    """Per kernel of KERNELS (with its template arguments): dispatches, median / least / largest duration in microseconds."""
    durations = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"(\w+_kernel)<([^>]*)>", r["Kernel_Name"])
        if m and m.group(1) in KERNELS:
            durations.setdefault(f"{m.group(1)}<{m.group(2)}>", []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {"mode": "table", "kernels": {k: dict(dispatches=len(v), median_us=float(np.median(v)), min_us=min(v), max_us=max(v)) for k, v in sorted(durations.items())}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace", "table"])
    ap.add_argument("dir", help="the directory of the files; for `table` the kernel trace (csv)")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir) if a.mode == "trace" else table(a.dir)), flush=True)
