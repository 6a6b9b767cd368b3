"""Measurements of the runs of same-state motif sites (tools/gpu_motif_runs.sh; results: profiles/r31/motif_runs.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_runs --runs` twice, one cold process each; wall clocks, the split the command
               records (ingest / engine / text), the flags and the sizes of the five files
  trace DIR    one process on the files of DIR, ONE run of each call, in this order, first on the candidates of bin-motifs.tsv and then on
               the one-letter background candidates (every A / every C of every bin: dense sites): `motif_site_counts` (sites_kernel's
               count pass, the yardstick: the same loads and walks), `motif_run_counts` (runs_kernel's count pass + the stitch) and
               `motif_runs` (the records: count + stitch for the totals, then count + stitch + prefix + fill per window).  The order of the
               calls goes to DIR/calls.json for the reader of the kernel trace; the site counts of the run table are compared with
               motif_site_counts' and the records with the run table
  table DIR    the dispatches of the kernel trace as PASSES — maximal stretches of consecutive dispatches of one family (sites_kernel,
               runs_kernel count, runs_stitch_kernel, runs_kernel fill) — in time order, each with its summed time (no GPU)
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

RUNS = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--runs", "--out", "runs"]
NAMES = ("motif-runs.tsv", "motif-runs-contigs.tsv", "motif-runs-hist.tsv", "motif-runs-bins.tsv", "motif-runs.bed")
FLAGS = ("none", "clustered", "alternating", "few_sites")


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
        wall = cli(tmp, "motif_runs", RUNS)
        t = json.load(open(os.path.join(tmp, "runs", "logs", "timings.motif_runs.json")))
        out["motif_runs_" + rep] = dict(wall_s=wall, **t)
    for name in NAMES[:1] + NAMES[3:4]:
        table = [l.split("\t") for l in open(os.path.join(tmp, "runs", name)).read().splitlines()]
        col = {n: j for j, n in enumerate(table[0])}
        zs = sorted(float(r[col["runs_z_within"]]) for r in table[1:])
        out[name] = dict(rows=len(table) - 1, flags={f: sum(r[-1] == f for r in table[1:]) for f in FLAGS}, z_min=zs[0] if zs else None,
                         z_median=zs[len(zs) // 2] if zs else None, z_max=zs[-1] if zs else None)
    out["out_bytes"] = {n: os.path.getsize(os.path.join(tmp, "runs", n)) for n in NAMES}
    return out


def trace(tmp):
    from nanomotif_amd import loading
    from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL, Motif
    eng, cands, ingest_s, _, _ = load(tmp, "pileup.bed")
    flat = [c.engine_candidate() for c in cands]
    mod_types = loading.kept_mod_types(eng)
    background = [(Motif(MOD_TYPE_TO_CANONICAL[mt], 0), mt, b) for b in sorted(eng.bin_index) if eng.bin_contigs(b) for mt in mod_types]
    out = {"mode": "trace", "ingest_s": ingest_s, "candidates": len(flat), "background_candidates": len(background),
           "chunks_of_the_longest_contig": int(-(-int(max(eng.contig_lengths)) // 8192))}
    order = []

    def timed(name, fn):
        before = eng.stats()["launches"]
        t0 = time.perf_counter()
        res = fn()
        out[name + "_s"] = time.perf_counter() - t0
        order.append({"call": name, "launches": eng.stats()["launches"] - before})
        return res
    for group, cs in (("motifs", flat), ("background", background)):
        six = timed(f"{group}_site_counts", lambda: eng.motif_site_counts(cs))
        tables = timed(f"{group}_run_counts", lambda: eng.motif_run_counts(cs))
        rec = timed(f"{group}_runs", lambda: [sb.records for sb in eng.motif_runs(cs)])
        rec = np.concatenate(rec) if rec else np.zeros(0, dtype=[("n_sites", "u4")])
        out[f"{group}_sites"] = int(sum(int(s.sum()) for _, s in six))
        out[f"{group}_runs_mod_nomod"] = [int(sum(int(t[:, s, 0].sum()) for _, t in tables)) for s in (0, 1)]
        out[f"{group}_longest_mod_nomod"] = [int(max([int(t[:, s, 2].max()) for _, t in tables if len(t)] or [0])) for s in (0, 1)]
        out[f"{group}_records"] = int(len(rec))
        out[f"{group}_equal_site_counts"] = bool(all(np.array_equal(t[:, :, 1], s[:, :3] + s[:, 3:]) for (_, t), (_, s) in zip(tables, six)))
        # runs of three or more unmethylated sites = the nomod runs less those of one and of two sites
        out[f"{group}_records_equal_table"] = bool(len(rec) == sum(int(t[:, 1, 0].sum() - t[:, 1, 3].sum() - t[:, 1, 4].sum()) for _, t in tables))
    with open(os.path.join(tmp, "calls.json"), "w") as f:
        json.dump(order, f)
    eng.close()
    return out


def family(name):
    if "sites_kernel" in name:
        return "sites_kernel"
    if "runs_stitch_kernel" in name:
        return "runs_stitch_kernel"
    if "runs_kernel" in name:
        return "runs_kernel fill" if "true" in name.split("runs_kernel", 1)[1].split(">", 1)[0] else "runs_kernel count"
    return None


def table(tmp, trace_csv):
    """The passes of the traced kernels in time order: [family, dispatches, summed time in us]."""
    import csv
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    passes = []
    for r in rows:
        fam = family(r["Kernel_Name"])
        if fam is None:
            continue
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if passes and passes[-1][0] == fam and fam != "runs_stitch_kernel":
            passes[-1][1] += 1
            passes[-1][2] += ns
        else:
            passes.append([fam, 1, ns])
    return {"mode": "table", "calls": json.load(open(os.path.join(tmp, "calls.json"))), "passes": [[f, n, round(ns / 1000.0, 1)] for f, n, ns in passes]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace", "table"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    ap.add_argument("--trace-csv", default=None)
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir) if a.mode == "trace" else table(a.dir, a.trace_csv)), flush=True)
