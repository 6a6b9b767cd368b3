"""Measurements of the per-site export (tools/gpu_motif_sites.sh; results: profiles/r7/motif_sites.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), then the two commands, one
               cold process each: `motif_discovery` (its bin-motifs.tsv names the motifs) and `motif_sites` on them, all states;
               wall clocks and the split `motif_sites` records (ingest / kernels / text)
  engine DIR   one process on the files of DIR, ingested the way the command does: the per-site data of the first 8 bins the only
               way the code had before — `ScanEngine.hit_positions` per (motif, contig, which) — against `ScanEngine.motif_sites` on
               the same candidates (states mod + nomod: the same data), two repetitions each, results compared; then all bins and
               all states, the count pass alone against `score_per_contig` on the same candidates
  trace DIR    the second half of `engine` only (what one `rocprofv3 --kernel-trace --stats` run looks at)
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
        wall = cli(tmp, "motif_sites", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "sites"])
        t = json.load(open(os.path.join(tmp, "sites", "logs", "timings.motif_sites.json")))
        out["motif_sites_" + rep] = dict(wall_s=wall, **t)
    out["bed_out_bytes"] = os.path.getsize(os.path.join(tmp, "sites", "motif-sites.bed"))
    with open(os.path.join(tmp, "sites", "motif-sites.bed"), "rb") as f:
        out["bed_out_lines"] = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(64 << 20), b""))
    return out


def engine(tmp, with_loop):
    from nanomotif_amd import loading, motif_sites as ms
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=os.path.join(tmp, "pileup.bed"), contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0)
    out = {"mode": "engine" if with_loop else "trace", "ingest_s": time.perf_counter() - t0}
    cands = [c for c in ms.candidates_of_bin_motifs(os.path.join(tmp, "out", "bin-motifs.tsv")) if c.bin in eng.bin_index and c.mod_type in eng.slot_of_mod]
    first_bins = list(dict.fromkeys(c.bin for c in cands))[:8]
    some = [c for c in cands if c.bin in first_bins]
    out.update(candidates=len(cands), candidates_first_8_bins=len(some))
    if with_loop:
        ecands = [c.engine_candidate() for c in some]
        old_s, new_s, n_calls = [], [], 0
        for rep in range(2):
            t0 = time.perf_counter()
            old, n_calls = [], 0
            for m, mt, b in ecands:
                for contig in eng.bin_contigs(b):
                    for which in range(4):
                        old.append(eng.hit_positions(contig, mt, m, which))
                        n_calls += 1
            old_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            rec = np.concatenate([sb.records for sb in eng.motif_sites(ecands, states=("mod", "nomod"))])
            new_s.append(time.perf_counter() - t0)
        # the same data: per (candidate, contig, which) the positions in order
        at, same = 0, True
        off = np.searchsorted(rec["candidate"], np.arange(len(ecands) + 1))
        for k, (m, mt, b) in enumerate(ecands):
            r = rec[off[k]:off[k + 1]]
            for contig in eng.bin_contigs(b):
                rc = r[r["contig"] == eng.contig_index[contig]]
                for which in range(4):
                    same &= np.array_equal(rc["pos"][rc["code"] == (which // 2) * 4 + which % 2].astype(np.int64), old[at])
                    at += 1
        out.update(hit_positions_loop_s=old_s, hit_positions_calls=n_calls, motif_sites_s=new_s, records=int(len(rec)), same_data=bool(same),
                   ratio=min(old_s) / min(new_s))
    ecands = [c.engine_candidate() for c in cands]
    b = eng.make_batch(ecands)
    for name, fn in (("score_per_contig", lambda: eng.score_per_contig(b)), ("motif_site_counts", lambda: eng.motif_site_counts(b))):
        ts = []
        for rep in range(3):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    t0 = time.perf_counter()
    n = sum(len(sb.records) for sb in eng.motif_sites(b))
    out.update(all_bins_all_states_s=time.perf_counter() - t0, all_bins_all_states_records=int(n), record_bytes=9 * int(n))
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "engine", "trace"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    a = ap.parse_args()
    res = files(a.dir, a.total_bp) if a.mode == "files" else engine(a.dir, a.mode == "engine")
    print(json.dumps(res), flush=True)
