"""Measurements of motif methylation along contigs (tools/gpu_motif_tracks.sh; results: profiles/r12/motif_tracks.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_tracks --tracks` at --window 128, 4096 and 65536, one cold process each; wall
               clocks, the split the command records (ingest / engine / segmentation and text) and what it found
  trace DIR    the count passes only, one process on the files of DIR: `motif_site_counts` of the candidates of bin-motifs.tsv —
               `sites_kernel`'s count pass, the yardstick: the same loads and walks, one row per contig — then `motif_tracks` of the same
               candidates at the three window sizes, two repetitions each (what one `rocprofv3 --kernel-trace --stats` run looks at);
               every table's windows are summed per contig and compared with the site counts first
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

WINDOWS = (128, 4096, 65536)
TRACKS = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "tr", "--tracks"]


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
    for w in WINDOWS:
        wall = cli(tmp, "motif_tracks", TRACKS + ["--window", str(w)])
        t = json.load(open(os.path.join(tmp, "tr", "logs", "timings.motif_tracks.json")))
        rows = [l.split("\t") for l in open(os.path.join(tmp, "tr", "motif-tracks-contigs.tsv")).read().splitlines()[1:]]
        out[f"motif_tracks_w{w}"] = dict(wall_s=wall, **t, contig_rows=len(rows), flags={f: sum(r[-1] == f for r in rows) for f in ("uniform", "breakpoint", "islands")},
                                         out_bytes={n: os.path.getsize(os.path.join(tmp, "tr", n))
                                                    for n in ("motif-tracks-contigs.tsv", "motif-tracks-segments.tsv", "motif-tracks.tsv")})
    return out


def load(tmp):
    from nanomotif_amd import loading, motif_sites as ms
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=os.path.join(tmp, "pileup.bed"), contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0, None)
    ingest_s = time.perf_counter() - t0
    cands = [c for c in ms.candidates_of_files([os.path.join(tmp, "out", "bin-motifs.tsv")]) if c.bin in eng.bin_index and c.mod_type in eng.slot_of_mod]
    return eng, cands, ingest_s


def trace(tmp):
    eng, cands, ingest_s = load(tmp)
    flat = [c.engine_candidate() for c in cands]
    out = {"mode": "trace", "ingest_s": ingest_s, "candidates": len(cands), "windows": list(WINDOWS)}
    calls = [("motif_site_counts", lambda: eng.motif_site_counts(flat))]
    calls += [(f"motif_tracks_w{w}", lambda w=w: list(eng.motif_tracks(flat, window=w))) for w in WINDOWS]
    res = {}
    for name, fn in calls:
        ts = []
        for rep in range(2):
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    # equality first: a contig's windows sum to its row of the site counts
    six = np.concatenate([t for _, t in res["motif_site_counts"]])
    out["occurrences"] = int(six.sum())
    for w in WINDOWS:
        sums = np.concatenate([np.add.reduceat(t.astype(np.int64), p[:-1], axis=0) for _, p, t in res[f"motif_tracks_w{w}"]])
        out[f"sums_equal_w{w}"] = bool(np.array_equal(sums, six))
        out[f"rows_w{w}"] = int(sum(len(t) for _, _, t in res[f"motif_tracks_w{w}"]))
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir)), flush=True)
