"""Measurements of the both-strand site state (tools/gpu_motif_strands.sh; results: profiles/r10/motif_strands.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_strands --hemi_sites` twice, one cold process each; wall clocks and the split
               the command records (ingest / kernels / text)
  engine DIR   one process on the files of DIR: the joint table the only way the code had before — `ScanEngine.motif_sites` of every
               candidate and of (its reverse complement, partner position), records to the host, a numpy join per candidate on 64-bit
               (contig, position +- d, other strand) keys — against `ScanEngine.motif_strand_counts`, two repetitions each, compared for
               equality
  trace DIR    the count passes only: `motif_compare_counts` of all candidates with both slots equal (the same sequence loads, eight
               state-plane loads), then `motif_strand_counts` (four plus four shifted ones), two repetitions each (what one
               `rocprofv3 --kernel-trace --stats` run looks at)
One JSON line per mode on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motif_compare_probe import cli, key      # noqa: E402  (the same directory)

STRANDS = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "st", "--hemi_sites"]


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
        wall = cli(tmp, "motif_strands", STRANDS)
        t = json.load(open(os.path.join(tmp, "st", "logs", "timings.motif_strands.json")))
        out["motif_strands_" + rep] = dict(wall_s=wall, **t)
    rows = [l.split("\t") for l in open(os.path.join(tmp, "st", "motif-strands.tsv")).read().splitlines()[1:]]
    out.update(candidates=len(rows), palindromes=sum(int(r[5]) for r in rows), pairs=[sum(int(r[6 + t]) for r in rows) for t in range(9)],
               bed_out_bytes=os.path.getsize(os.path.join(tmp, "st", "hemi-sites.bed")))
    return out


def load(tmp):
    from nanomotif_amd import loading, motif_sites as ms, motif_strands as mst
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=os.path.join(tmp, "pileup.bed"), contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0, None)
    ingest_s = time.perf_counter() - t0
    paths = [os.path.join(tmp, "out", "bin-motifs.tsv")]
    cands = [c for c in mst.strand_candidates(ms.candidates_of_files(paths), mst.complement_partners(paths)) if c.bin in eng.bin_index and c.mod_type in eng.slot_of_mod]
    return eng, cands, ingest_s


def host_path(eng, cands):
    """The parent commit's only way: every site of every candidate, and of its reverse complement at the partner position, to the host;
    then per candidate a join of (contig, own position +- d, other strand) on the partner's keys.  Returns the int64[rows, 18] table in the
    row layout of ``motif_strand_counts``."""
    from nanomotif_amd.motif import Motif
    sides = []
    for flat in ([c.engine_candidate()[:3] for c in cands],
                 [(Motif(c.engine_candidate()[0].reverse_compliment().string, c.partner_position), c.mod_type, c.bin) for c in cands]):
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
        minus = (a["code"] >> 2).astype(np.int64)
        at = a["pos"].astype(np.int64) + np.where(minus == 1, -c.offset, c.offset)
        _, ia, ib = np.intersect1d(key(a["contig"], at, 1 - minus), key(b["contig"], b["pos"], b["code"] >> 2), assume_unique=True, return_indices=True)
        assert len(ia) == len(a) == len(b)
        n = len(eng.bin_contigs(c.bin))
        cell = rank[a["contig"][ia]] * 18 + 9 * minus[ia] + 3 * (a["code"][ia] & 3).astype(np.int64) + (b["code"][ib] & 3)
        tables.append(np.bincount(cell, minlength=n * 18).reshape(n, 18))
    return np.concatenate(tables) if tables else np.zeros((0, 18), np.int64)


def engine(tmp):
    eng, cands, ingest_s = load(tmp)
    flat = [c.engine_candidate() for c in cands]
    out = {"mode": "engine", "ingest_s": ingest_s, "candidates": len(cands)}
    old_s, new_s = [], []
    for rep in range(2):
        t0 = time.perf_counter()
        old = host_path(eng, cands)
        old_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        new = np.concatenate([t for _, t in eng.motif_strand_counts(flat)])
        new_s.append(time.perf_counter() - t0)
    t = new.sum(axis=0)
    out.update(host_path_s=old_s, new_path_s=new_s, ratio=min(old_s) / min(new_s), same_tables=bool(np.array_equal(old, new)), rows=int(len(new)),
               occurrences=int(new.sum()), pairs=(t[:9] + t[9:]).tolist())
    eng.close()
    return out


def trace(tmp):
    eng, cands, ingest_s = load(tmp)
    flat = [c.engine_candidate() for c in cands]
    out = {"mode": "trace", "ingest_s": ingest_s, "candidates": len(cands), "offsets": sorted({c.offset for c in cands})}
    calls = (("motif_compare_counts_same_slot", lambda: eng.motif_compare_counts([f[:3] for f in flat], lambda mt: (mt, mt))),
             ("motif_strand_counts", lambda: eng.motif_strand_counts(flat)))
    res = {}
    for name, fn in calls:
        ts = []
        for rep in range(2):
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    # equality first: summed over the partner's state the joint table is the diagonal of compare(A, A)
    joint = np.concatenate([t for _, t in res["motif_strand_counts"]]).reshape(-1, 2, 3, 3)
    diag = np.concatenate([t for _, t in res["motif_compare_counts_same_slot"]]).reshape(-1, 2, 3, 3)
    out["marginals_equal"] = bool(np.array_equal(joint.sum(axis=3), np.diagonal(diag, axis1=2, axis2=3)))
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
