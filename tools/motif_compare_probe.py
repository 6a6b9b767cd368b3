"""Measurements of the two-sample comparison (tools/gpu_motif_compare.sh; results: profiles/r7/motif_compare.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs): pileup.bed (sample A) and a derived
               pileup_b.bed (sample B: of A's rows a seeded 6 % flipped across both thresholds, 5 % dropped, 4 % moved between the
               thresholds), then `motif_discovery` on A (its bin-motifs.tsv names the motifs) and `motif_compare --switched_sites` twice,
               one cold process each; wall clocks and the split `motif_compare` records (ingest A / ingest B / kernels / text)
  engine DIR   one process on the files of DIR, both pileups resident: the joint table the only way the code had before —
               `ScanEngine.motif_sites` of every candidate on each sample's slot, records to the host, a numpy join on 64-bit (contig,
               position, strand) keys per candidate — against `ScanEngine.motif_compare_counts`, two repetitions each, compared for equality
  trace DIR    the count passes only: `motif_site_counts` of all candidates on sample A's slots, on sample B's slots, then
               `motif_compare_counts`, two repetitions each (what one `rocprofv3 --kernel-trace --stats` run looks at)
One JSON line per mode on stdout."""
import argparse
import ctypes as C
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


def write_sample_b(mg, tmp, device):
    """pileup_b.bed: sample A's rows (the metagenome's own) under a seeded perturbation, written by the native bedMethyl writer."""
    import torch
    from nanomotif_amd import e2e_synth, synth
    _, _, _, _, _, cat = e2e_synth.generate_raw(mg, device)
    torch.cuda.synchronize(device)
    host = {k: v.cpu().numpy() for k, v in cat.items()}
    del cat
    torch.cuda.empty_cache()
    pct = np.rint(host["frac"] * 10000.0).astype(np.int32)
    u = np.random.default_rng(2).random(len(pct), dtype=np.float32)
    flip = (u >= 0.05) & (u < 0.11)
    pct[flip] = 10000 - pct[flip]
    move = (u >= 0.11) & (u < 0.15)
    called = (pct <= 3000) | (pct >= 7000)
    pct[move & called] = 5000
    pct[move & ~called] = 9000
    keep = u >= 0.05
    names = "".join(mg.names).encode()
    off = np.zeros(len(mg.names) + 1, dtype=np.uint32)
    np.cumsum([len(x) for x in mg.names], out=off[1:])
    col = lambda k, dt: np.ascontiguousarray(host[k][keep], dtype=dt)
    cid, pos, mod, st, nv, pct = col("contig", np.uint32), col("position", np.uint32), col("mod", np.int8), col("strand", np.uint8), col("nvalid", np.int32), \
        np.ascontiguousarray(pct[keep])
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    lib = e2e_synth.synth_lib()
    bed = os.path.join(tmp, "pileup_b.bed")
    if lib.nm_synth_write_bed(bed.encode(), len(cid), len(mg.names), names, p(off, C.c_uint32), p(cid, C.c_uint32), p(pos, C.c_uint32), p(mod, C.c_int8),
                              p(st, C.c_uint8), p(nv, C.c_int32), p(pct, C.c_int32), 0):
        raise RuntimeError(lib.nm_synth_last_error().decode())
    return {"rows_b": int(len(cid)), "bed_b_bytes": os.path.getsize(bed), "flipped": int(flip.sum()), "moved": int(move.sum())}


COMPARE = ["assembly.fasta", "pileup.bed", "pileup_b.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "cmp", "--switched_sites"]


def files(tmp, total_bp):
    import torch
    from nanomotif_amd import e2e_synth, synth
    spec = synth.config("cfg3") if total_bp == 100_000_000 else synth.SynthSpec(
        n_contigs=max(8, total_bp // 100_000), total_bp=total_bp, n_bins=max(2, total_bp // 2_000_000), mod_types=("a", "m"), seed=1)
    mg = synth.make_metagenome(spec)
    t0 = time.perf_counter()
    sizes = e2e_synth.write_text_inputs(mg, tmp, torch.device("cuda", 0))
    out = {"mode": "files", "total_bp": total_bp, "rows": sizes["rows"], "bed_bytes": sizes["bed_bytes"], "written_in_s": time.perf_counter() - t0}
    t0 = time.perf_counter()
    out.update(write_sample_b(mg, tmp, torch.device("cuda", 0)))
    out["sample_b_written_in_s"] = time.perf_counter() - t0
    torch.cuda.empty_cache()
    out["motif_discovery_wall_s"] = cli(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    out["motif_rows"] = len(open(os.path.join(tmp, "out", "bin-motifs.tsv")).read().splitlines()) - 1
    for rep in ("cold", "again"):
        wall = cli(tmp, "motif_compare", COMPARE)
        t = json.load(open(os.path.join(tmp, "cmp", "logs", "timings.motif_compare.json")))
        out["motif_compare_" + rep] = dict(wall_s=wall, **t)
    rows = [l.split("\t") for l in open(os.path.join(tmp, "cmp", "motif-compare.tsv")).read().splitlines()[1:]]
    out.update(candidates=len(rows), transitions=[sum(int(r[4 + t]) for r in rows) for t in range(9)],
               bed_out_bytes=os.path.getsize(os.path.join(tmp, "cmp", "switched-sites.bed")))
    return out


def load(tmp):
    from nanomotif_amd import loading, motif_compare as mc, motif_sites as ms
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=None, contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0, pileups=[(os.path.join(tmp, "pileup.bed"), None), (os.path.join(tmp, "pileup_b.bed"), lambda mt: mt + mc.SAMPLE_B_SUFFIX)])
    ingest_s = time.perf_counter() - t0
    mod_types = loading.kept_mod_types(eng)
    cands = [c for c in ms.candidates_of_bin_motifs(os.path.join(tmp, "out", "bin-motifs.tsv")) if c.bin in eng.bin_index and c.mod_type in mod_types]
    return eng, cands, ingest_s


def key(contig, pos, minus):
    """One 64-bit key per (contig, position, strand)."""
    return (np.asarray(contig).astype(np.int64) << 33) | (np.asarray(pos).astype(np.int64) << 1) | np.asarray(minus).astype(np.int64)


def host_path(eng, cands):
    """The parent commit's only way: every site of every candidate on each sample's slot to the host, then a join per candidate on
    the keys.  Returns the int64[rows, 18] table in the row layout of ``motif_compare_counts``."""
    from nanomotif_amd import motif_compare as mc
    sides = []
    for side in (0, 1):
        flat = [(c.engine_candidate()[0], mc.labels_of(c.mod_type)[side], c.bin) for c in cands]
        rec = np.concatenate([sb.records for sb in eng.motif_sites(flat)])
        sides.append((rec, np.searchsorted(rec["candidate"], np.arange(len(cands) + 1))))
    rank = np.zeros(len(eng.contig_names), dtype=np.int64)
    for b in {c.bin for c in cands}:
        for r, n in enumerate(eng.bin_contigs(b)):
            rank[eng.contig_index[n]] = r
    tables = []
    for k, c in enumerate(cands):
        (ra, oa), (rb, ob) = sides
        a, b = ra[oa[k]:oa[k + 1]], rb[ob[k]:ob[k + 1]]
        _, ia, ib = np.intersect1d(key(a["contig"], a["pos"], a["code"] >> 2), key(b["contig"], b["pos"], b["code"] >> 2), assume_unique=True,
                                   return_indices=True)
        assert len(ia) == len(a) == len(b)
        n = len(eng.bin_contigs(c.bin))
        cell = rank[a["contig"][ia]] * 18 + 9 * (a["code"][ia] >> 2).astype(np.int64) + 3 * (a["code"][ia] & 3).astype(np.int64) + (b["code"][ib] & 3)
        tables.append(np.bincount(cell, minlength=n * 18).reshape(n, 18))
    return np.concatenate(tables) if tables else np.zeros((0, 18), np.int64)


def engine(tmp):
    from nanomotif_amd import motif_compare as mc
    eng, cands, ingest_s = load(tmp)
    flat = [c.engine_candidate() for c in cands]
    out = {"mode": "engine", "ingest_s": ingest_s, "ingest_a_s": eng.pileup_ingests[0]["seconds"], "ingest_b_s": eng.pileup_ingests[1]["seconds"],
           "candidates": len(cands)}
    old_s, new_s = [], []
    for rep in range(2):
        t0 = time.perf_counter()
        old = host_path(eng, cands)
        old_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        new = np.concatenate([t for _, t in eng.motif_compare_counts(flat, mc.labels_of)])
        new_s.append(time.perf_counter() - t0)
    t = new.sum(axis=0)
    out.update(host_path_s=old_s, new_path_s=new_s, ratio=min(old_s) / min(new_s), same_tables=bool(np.array_equal(old, new)), rows=int(len(new)),
               occurrences=int(new.sum()), transitions=(t[:9] + t[9:]).tolist())
    eng.close()
    return out


def trace(tmp):
    from nanomotif_amd import motif_compare as mc
    eng, cands, ingest_s = load(tmp)
    flat = [c.engine_candidate() for c in cands]
    sides = [eng.make_batch([(c.engine_candidate()[0], mc.labels_of(c.mod_type)[side], c.bin) for c in cands]) for side in (0, 1)]
    out = {"mode": "trace", "ingest_s": ingest_s, "candidates": len(cands)}
    calls = (("motif_site_counts_a", lambda: eng.motif_site_counts(sides[0])), ("motif_site_counts_b", lambda: eng.motif_site_counts(sides[1])),
             ("motif_compare_counts", lambda: eng.motif_compare_counts(flat, mc.labels_of)))
    res = {}
    for name, fn in calls:
        ts = []
        for rep in range(2):
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    # equality first: the marginals of the joint table are the two six-column tables
    joint = np.concatenate([t for _, t in res["motif_compare_counts"]]).reshape(-1, 2, 3, 3)
    out["marginals_equal"] = bool(np.array_equal(joint.sum(axis=3).reshape(-1, 6), np.concatenate([t for _, t in res["motif_site_counts_a"]]))
                                  and np.array_equal(joint.sum(axis=2).reshape(-1, 6), np.concatenate([t for _, t in res["motif_site_counts_b"]])))
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
