"""Measurements of the methylation profile around motif sites (tools/gpu_motif_profile.sh; results: profiles/r11/motif_profile.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_profile --radius 10` twice, one cold process each; wall clocks and the split
               the command records (ingest / engine / text)
  trace DIR    the count passes only, one process on the files of DIR: `motif_strand_counts` of the candidates of bin-motifs.tsv under
               the partner rule — the existing kernel that reads ONE shifted position of one slot — then `motif_profile` of the same
               candidates at radius 10 under every mod type the pileup holds, two repetitions each (what one
               `rocprofv3 --kernel-trace --stats` run looks at); the partner cell of the profile is compared with the strands table
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
from motif_strands_probe import load     # noqa: E402

RADIUS = 10
PROFILE = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "pr", "--radius", str(RADIUS)]


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
        wall = cli(tmp, "motif_profile", PROFILE)
        t = json.load(open(os.path.join(tmp, "pr", "logs", "timings.motif_profile.json")))
        out["motif_profile_" + rep] = dict(wall_s=wall, **t)
    rows = [l.split("\t") for l in open(os.path.join(tmp, "pr", "motif-profile-summary.tsv")).read().splitlines()[1:]]
    out.update(candidates=len(rows), flags={f: sum(r[-1] == f for r in rows) for f in ("none", "shifted", "other_mod_type")},
               out_bytes={n: os.path.getsize(os.path.join(tmp, "pr", n)) for n in ("motif-profile.tsv", "motif-profile-bins.tsv", "motif-profile-summary.tsv")})
    return out


def trace(tmp):
    from nanomotif_amd import loading
    eng, cands, ingest_s = load(tmp)
    flat = [c.engine_candidate() for c in cands]
    targets = loading.kept_mod_types(eng)
    out = {"mode": "trace", "ingest_s": ingest_s, "candidates": len(cands), "targets": targets, "radius": RADIUS,
           "cells_per_candidate": len(targets) * (2 * RADIUS + 1) * 2}
    calls = (("motif_strand_counts", lambda: eng.motif_strand_counts(flat)),
             ("motif_profile", lambda: eng.motif_profile([f[:3] for f in flat], targets=targets, radius=RADIUS)))
    res = {}
    for name, fn in calls:
        ts = []
        for rep in range(2):
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    # equality first: the cell (own target, opposite, d) of the profile holds the partner marginals of the strands table
    _, sites, table = res["motif_profile"]
    same = True
    for k, c in enumerate(cands):
        if abs(c.offset) > RADIUS:
            continue
        marg = res["motif_strand_counts"][k][1].sum(axis=0).reshape(2, 3, 3).sum(axis=1)
        cell = table[k, targets.index(c.mod_type), RADIUS + c.offset, :, 1]
        same &= bool(np.array_equal(cell[:, :2], marg[:, :2]) and np.array_equal(cell[:, 2] + cell[:, 3], marg[:, 2]))
    out.update(partner_cells_equal=same, occurrences=int(sites.sum()))
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir)), flush=True)
