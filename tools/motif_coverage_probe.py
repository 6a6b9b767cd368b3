"""Measurements of the coverage report (tools/gpu_motif_coverage.sh; results: profiles/r7/motif_coverage.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), then the two commands, one cold
               process each: `motif_discovery` (its bin-motifs.tsv names the motifs) and `motif_coverage --unexplained_sites` twice;
               wall clocks and the split `motif_coverage` records (ingest / kernels / text)
  engine DIR   one process on the files of DIR, ingested the way the command does: the figures of ALL (bin, mod type) sets the only way
               the code had before — `ScanEngine.motif_sites` of every candidate, records to the host, numpy unions per set against
               `confident_rows()` (which lists the methylated calls only: mod_total, mod_explained, nomod_covered, nocall_covered, the
               exclusive counts and the unexplained positions can be had that way, nomod_total cannot) — against
               `ScanEngine.motif_coverage` + `unexplained_sites` (one call each), two repetitions each, results compared for equality
  trace DIR    the count passes only: `motif_site_counts` of all candidates, then `motif_coverage` of all sets (what one
               `rocprofv3 --kernel-trace --stats` run looks at)
One JSON line per mode on stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cli(tmp, command, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "nanomotif_amd", command] + args, cwd=tmp, env=env, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if r.returncode:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(r.returncode)
    return wall


def files(tmp, total_bp):
    import torch
    from nanomotif_amd import e2e_synth, synth
    spec = synth.config("cfg3") if total_bp == 100_000_000 else synth.SynthSpec(
        n_contigs=max(8, total_bp // 100_000), total_bp=total_bp, n_bins=max(2, total_bp // 2_000_000), mod_types=("a", "m"), seed=1)
    t0 = time.perf_counter()
    sizes = e2e_synth.write_text_inputs(synth.make_metagenome(spec), tmp, torch.device("cuda", 0))
    out = {"mode": "files", "total_bp": total_bp, "rows": sizes["rows"], "bed_bytes": sizes["bed_bytes"], "written_in_s": time.perf_counter() - t0}
    torch.cuda.empty_cache()
    out["motif_discovery_wall_s"] = cli(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    out["motif_rows"] = len(open(os.path.join(tmp, "out", "bin-motifs.tsv")).read().splitlines()) - 1
    for rep in ("cold", "again"):
        wall = cli(tmp, "motif_coverage", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "cov",
                                           "--unexplained_sites"])
        t = json.load(open(os.path.join(tmp, "cov", "logs", "timings.motif_coverage.json")))
        out["motif_coverage_" + rep] = dict(wall_s=wall, **t)
    rows = [l.split("\t") for l in open(os.path.join(tmp, "cov", "motif-coverage.tsv")).read().splitlines()[1:]]
    out.update(sets=len(rows), sets_without_motifs=sum(r[2] == "0" for r in rows), n_mod=sum(int(r[3]) for r in rows),
               n_mod_explained=sum(int(r[4]) for r in rows), bed_out_bytes=os.path.getsize(os.path.join(tmp, "cov", "unexplained-sites.bed")))
    return out


def load(tmp):
    from nanomotif_amd import loading, motif_coverage as mc, motif_sites as ms
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=os.path.join(tmp, "pileup.bed"), contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0)
    ingest_s = time.perf_counter() - t0
    cands = ms.candidates_of_bin_motifs(os.path.join(tmp, "out", "bin-motifs.tsv"))
    mod_types = loading.kept_mod_types(eng)
    sets = mc.build_sets([b for b in eng.bin_index if eng.bin_contigs(b)], mod_types, cands)
    return eng, sets, ingest_s


def key(contig, pos, minus):
    """One 64-bit key per (contig, position, strand)."""
    return (np.asarray(contig).astype(np.int64) << 33) | (np.asarray(pos).astype(np.int64) << 1) | np.asarray(minus).astype(np.int64)


def host_path(eng, sets):
    """The parent commit's only way: every site of every candidate to the host, then set algebra in numpy.  Returns (per set
    [mod_total, mod_explained, nomod_covered, nocall_covered] per strand = int64[n_sets, 8], exclusive int64[n_cand, 4], the sorted
    unexplained keys per set)."""
    from nanomotif_amd import pileup as pileup_mod
    flat = [c.engine_candidate() for s in sets for c in s.candidates]
    rec = np.concatenate([sb.records for sb in eng.motif_sites(flat)])
    off = np.searchsorted(rec["candidate"], np.arange(len(flat) + 1))
    cc, cp, cs, cm = eng.confident_rows()
    minus = (cs == ord("-")) | (cs == 1)
    order = np.argsort(cc, kind="stable")
    cc, ck, cm = cc[order], key(cc, cp, minus)[order], cm[order]
    tables, excl, unexplained, k = np.zeros((len(sets), 8), np.int64), np.zeros((len(flat), 4), np.int64), [], 0
    for si, s in enumerate(sets):
        code = pileup_mod.MOD_TYPES.index(s.mod_type)
        parts = []
        for n in eng.bin_contigs(s.bin):
            i = eng.contig_index[n]
            a, b = np.searchsorted(cc, i), np.searchsorted(cc, i + 1)
            parts.append(ck[a:b][cm[a:b] == code])
        M = np.unique(np.concatenate(parts))
        per_k, per_state = [], []
        for j in range(len(s.candidates)):
            r = rec[off[k + j]:off[k + j + 1]]
            per_k.append(key(r["contig"], r["pos"], (r["code"] >> 2) & 1))
            per_state.append(r["code"] & 3)
        allk = np.concatenate(per_k) if per_k else np.zeros(0, np.int64)
        alls = np.concatenate(per_state) if per_state else np.zeros(0, np.uint8)
        cover, first, times = np.unique(allk, return_index=True, return_counts=True)
        state = alls[first]
        for strand in (0, 1):
            on = (cover & 1) == strand
            tables[si, 4 * strand:4 * strand + 4] = (((M & 1) == strand).sum(), (on & (state == 0)).sum(), (on & (state == 1)).sum(), (on & (state == 2)).sum())
        once = cover[times == 1]
        for j, c in enumerate(per_k):
            e = np.isin(c, once, assume_unique=True)
            st, minus_j = per_state[j][e], c[e] & 1
            excl[k + j] = (((st == 0) & (minus_j == 0)).sum(), ((st == 1) & (minus_j == 0)).sum(), ((st == 0) & (minus_j == 1)).sum(),
                           ((st == 1) & (minus_j == 1)).sum())
        unexplained.append(np.setdiff1d(M, cover, assume_unique=True))
        k += len(s.candidates)
    return tables, excl, unexplained


def new_path(eng, sets):
    esets = [s.engine_set() for s in sets]
    res = eng.motif_coverage(esets)
    tables = np.array([t.sum(axis=0) for _, t, _ in res], dtype=np.int64).reshape(len(sets), 10)
    excl = np.array([t.sum(axis=0) for _, _, per in res for t in per], dtype=np.int64).reshape(-1, 4)
    rec = np.concatenate(list(eng.unexplained_sites(esets)))
    return tables, excl, rec


def engine(tmp):
    eng, sets, ingest_s = load(tmp)
    out = {"mode": "engine", "ingest_s": ingest_s, "sets": len(sets), "candidates": sum(len(s.candidates) for s in sets)}
    old_s, new_s = [], []
    for rep in range(2):
        t0 = time.perf_counter()
        old = host_path(eng, sets)
        old_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        new = new_path(eng, sets)
        new_s.append(time.perf_counter() - t0)
    keys = key(new[2]["contig"], new[2]["pos"], new[2]["code"] >> 2)
    cut = np.searchsorted(new[2]["set"], np.arange(len(sets) + 1))
    same_rec = all(np.array_equal(np.sort(keys[cut[i]:cut[i + 1]]), old[2][i]) for i in range(len(sets)))
    out.update(host_path_s=old_s, new_path_s=new_s, ratio=min(old_s) / min(new_s),
               same_set_tables=bool(np.array_equal(old[0], new[0][:, [0, 1, 3, 4, 5, 6, 8, 9]])), same_exclusive=bool(np.array_equal(old[1], new[1])),
               same_unexplained=bool(same_rec), unexplained_records=int(len(new[2])), n_mod=int(new[0][:, [0, 5]].sum()),
               n_mod_explained=int(new[0][:, [1, 6]].sum()))
    eng.close()
    return out


def trace(tmp):
    eng, sets, ingest_s = load(tmp)
    flat = eng.make_batch([c.engine_candidate() for s in sets for c in s.candidates])
    esets = [s.engine_set() for s in sets]
    out = {"mode": "trace", "ingest_s": ingest_s, "candidates": len(flat), "sets": len(sets)}
    for name, fn in (("motif_site_counts", lambda: eng.motif_site_counts(flat)), ("motif_coverage", lambda: eng.motif_coverage(esets))):
        ts = []
        for rep in range(3):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "engine", "trace"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    a = ap.parse_args()
    res = files(a.dir, a.total_bp) if a.mode == "files" else engine(a.dir) if a.mode == "engine" else trace(a.dir)
    print(json.dumps(res), flush=True)
