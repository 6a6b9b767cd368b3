"""Measurements of the read-fraction histograms (tools/gpu_motif_fractions.sh; results: profiles/r13/motif_fractions.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs): pileup.bed (the synthetic pileup, its
               fractions spread over [0, 1]) and a derived pileup_bimodal.bed (every record none or all of its reads modified), then
               `motif_discovery` on pileup.bed (its bin-motifs.tsv names the motifs) and `motif_fractions` on either pileup at --bins 20 and
               64, one cold process each; wall clocks, the split the command records (ingest / engine / statistics and text), the flags
  trace DIR    the count passes only, one process on the files of DIR (--pileup names the pileup): the state planes AND the read statistics
               of the one pileup resident, `motif_site_counts` of the candidates of bin-motifs.tsv — `sites_kernel`'s count pass, the
               yardstick: the same loads and walks, six counts per contig — then `motif_fractions` of the same candidates at 20 and 64
               bins, two repetitions each (what one `rocprofv3 --kernel-trace --stats` run looks at); the occurrences of every row are
               compared with the site counts first
One JSON line per mode on stdout.  NM_LIB=<path> runs either mode on another build of the library (A/B of a kernel variant)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motif_compare_probe import cli      # noqa: E402  (the same directory)

BINS = (20, 64)
PILEUPS = ("pileup.bed", "pileup_bimodal.bed")
FRACTIONS = ["-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "fr"]


def write_bimodal(mg, tmp, device):
    """pileup_bimodal.bed: the metagenome's own rows with every fraction moved to the nearer of 0 and 1 (native bedMethyl writer)."""
    import torch
    from nanomotif_amd import e2e_synth
    _, _, _, _, _, cat = e2e_synth.generate_raw(mg, device)
    torch.cuda.synchronize(device)
    host = {k: v.cpu().numpy() for k, v in cat.items()}
    del cat
    torch.cuda.empty_cache()
    pct = np.where(np.rint(host["frac"] * 10000.0) >= 5000, 10000, 0).astype(np.int32)
    names = "".join(mg.names).encode()
    off = np.zeros(len(mg.names) + 1, dtype=np.uint32)
    np.cumsum([len(x) for x in mg.names], out=off[1:])
    col = lambda k, dt: np.ascontiguousarray(host[k], dtype=dt)
    cid, pos, mod, st, nv = col("contig", np.uint32), col("position", np.uint32), col("mod", np.int8), col("strand", np.uint8), col("nvalid", np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    lib = e2e_synth.synth_lib()
    bed = os.path.join(tmp, PILEUPS[1])
    if lib.nm_synth_write_bed(bed.encode(), len(cid), len(mg.names), names, p(off, C.c_uint32), p(cid, C.c_uint32), p(pos, C.c_uint32), p(mod, C.c_int8),
                              p(st, C.c_uint8), p(nv, C.c_int32), p(pct, C.c_int32), 0):
        raise RuntimeError(lib.nm_synth_last_error().decode())
    return {"rows_bimodal": int(len(cid)), "bed_bimodal_bytes": os.path.getsize(bed), "share_full": float((pct == 10000).mean())}


def files(tmp, total_bp):
    import torch
    from nanomotif_amd import e2e_synth, synth
    spec = synth.config("cfg3") if total_bp == 100_000_000 else synth.SynthSpec(
        n_contigs=max(8, total_bp // 100_000), total_bp=total_bp, n_bins=max(2, total_bp // 2_000_000), mod_types=("a", "m"), seed=1)
    mg = synth.make_metagenome(spec)
    t0 = time.perf_counter()
    sizes = e2e_synth.write_text_inputs(mg, tmp, torch.device("cuda", 0))
    out = {"mode": "files", "total_bp": total_bp, "rows": sizes["rows"], "bed_bytes": sizes["bed_bytes"], "written_in_s": time.perf_counter() - t0}
    out.update(write_bimodal(mg, tmp, torch.device("cuda", 0)))
    torch.cuda.empty_cache()
    out["motif_discovery_wall_s"] = cli(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    out["motif_rows"] = len(open(os.path.join(tmp, "out", "bin-motifs.tsv")).read().splitlines()) - 1
    for pileup in PILEUPS:
        for b in BINS:
            wall = cli(tmp, "motif_fractions", ["assembly.fasta", pileup] + FRACTIONS + ["--bins", str(b)])
            t = json.load(open(os.path.join(tmp, "fr", "logs", "timings.motif_fractions.json")))
            rows = [l.split("\t") for l in open(os.path.join(tmp, "fr", "motif-fractions.tsv")).read().splitlines()]
            flag = rows[0].index("flag")
            out[f"motif_fractions_{pileup}_b{b}"] = dict(
                wall_s=wall, **t, flags={f: sum(r[flag] == f for r in rows[1:]) for f in ("few_sites", "methylated", "unmethylated", "bimodal", "partial")},
                out_bytes={n: os.path.getsize(os.path.join(tmp, "fr", n)) for n in ("motif-fractions.tsv", "motif-fractions-contigs.tsv", "motif-fractions-hist.tsv")})
    return out


def load(tmp, pileup):
    from nanomotif_amd import contig_methylation as cm, loading, motif_sites as ms
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=os.path.join(tmp, pileup), contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0, None)
    ingest_s = time.perf_counter() - t0
    cands = [c for c in ms.candidates_of_files([os.path.join(tmp, "out", "bin-motifs.tsv")]) if c.bin in eng.bin_index and c.mod_type in eng.slot_of_mod]
    t0 = time.perf_counter()
    kept = cm.read_statistics_device(eng, eng.lib, args.pileup, 0, {n: i for i, n in enumerate(eng.contig_names)}, {c.mod_type for c in cands}, True, 5, 0.8)
    return eng, cands, ingest_s, time.perf_counter() - t0, kept


def trace(tmp, pileup):
    eng, cands, ingest_s, readstats_s, kept = load(tmp, pileup)
    flat = [c.engine_candidate() for c in cands]
    out = {"mode": "trace", "pileup": pileup, "lib": os.environ.get("NM_LIB", ""), "ingest_s": ingest_s, "readstats_s": readstats_s, "kept": kept,
           "candidates": len(cands), "bins": list(BINS)}
    calls = [("motif_site_counts", lambda: eng.motif_site_counts(flat))]
    calls += [(f"motif_fractions_b{b}", lambda b=b: list(eng.motif_fractions(flat, bins=b))) for b in BINS]
    res = {}
    for name, fn in calls:
        ts = []
        for rep in range(2):
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    # equality first: the occurrences of a row are the six site counts of the same row
    six = np.concatenate([t for _, t in res["motif_site_counts"]]).astype(np.int64)
    out["occurrences"] = int(six.sum())
    for b in BINS:
        t = np.concatenate([t for _, _, t in res[f"motif_fractions_b{b}"]]).astype(np.int64)
        out[f"occurrences_equal_b{b}"] = bool(np.array_equal(t[:, :, b], np.stack([six[:, :3].sum(axis=1), six[:, 3:].sum(axis=1)], axis=1)))
        out[f"sites_b{b}"] = int(t[:, :, :b].sum())
        out[f"end_bins_share_b{b}"] = float((t[:, :, 0].sum() + t[:, :, b - 1].sum()) / max(1, t[:, :, :b].sum()))
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    ap.add_argument("--pileup", default=PILEUPS[0])
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir, a.pileup)), flush=True)
