"""Measurements of the sequence context of motif sites (tools/gpu_motif_context.sh; results: profiles/r15/motif_context.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_context --radius 10` twice, one cold process each; wall clocks, the split the
               command records (ingest / engine / text) and the rows that are flagged `underspecified`
  trace DIR    the count passes only, one process on the files of DIR and the candidates of bin-motifs.tsv, two repetitions each, in this
               order: `motif_site_counts` (sites_kernel's count pass), `motif_profile` at radius 10 with ONE target (12 counters a shift:
               the yardstick), `motif_context` at radius 10 (24 counters a shift) through the workgroup's LDS sum, and the same with
               NM_CONTEXT_WAVE_ATOMICS=1 (what one `rocprofv3 --kernel-trace --stats` run looks at); the two context tables are compared
               with each other and their `states` with the sites table first
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
CONTEXT = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "cx", "--radius", str(RADIUS)]
NAMES = ("motif-context.tsv", "motif-context-bins.tsv", "motif-context-summary.tsv")


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
        wall = cli(tmp, "motif_context", CONTEXT)
        t = json.load(open(os.path.join(tmp, "cx", "logs", "timings.motif_context.json")))
        out["motif_context_" + rep] = dict(wall_s=wall, **t)
    rows = [l.split("\t") for l in open(os.path.join(tmp, "cx", "motif-context-summary.tsv")).read().splitlines()[1:]]
    gains = sorted(float(r[9]) for r in rows)
    out.update(candidates=len(rows), flags={f: sum(r[-1] == f for r in rows) for f in ("none", "underspecified", "few_sites")},
               flagged_rows=[r for r in rows if r[-1] == "underspecified"][:20], best_gain_max=gains[-1] if gains else None,
               best_gain_median=gains[len(gains) // 2] if gains else None,
               out_bytes={n: os.path.getsize(os.path.join(tmp, "cx", n)) for n in NAMES})
    return out


def trace(tmp):
    from nanomotif_amd import loading
    eng, cands, ingest_s = load(tmp)
    flat = [c.engine_candidate()[:3] for c in cands]
    targets = loading.kept_mod_types(eng)
    out = {"mode": "trace", "ingest_s": ingest_s, "candidates": len(cands), "profile_target": targets[0], "radius": RADIUS}

    def wave_atomics():
        os.environ["NM_CONTEXT_WAVE_ATOMICS"] = "1"
        try:
            return eng.motif_context(flat, radius=RADIUS)
        finally:
            del os.environ["NM_CONTEXT_WAVE_ATOMICS"]
    calls = (("motif_site_counts", lambda: eng.motif_site_counts(flat)),
             ("motif_profile_one_target", lambda: eng.motif_profile(flat, targets=targets[:1], radius=RADIUS)),
             ("motif_context", lambda: eng.motif_context(flat, radius=RADIUS)),
             ("motif_context_wave_atomics", wave_atomics))
    res = {}
    for name, fn in calls:
        ts = []
        for rep in range(2):
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = ts
    states, table = res["motif_context"]
    s_w, t_w = res["motif_context_wave_atomics"]
    six = np.array([t.sum(axis=0).reshape(2, 3) for _, t in res["motif_site_counts"]], dtype=np.int64).reshape(-1, 2, 3)
    out.update(variants_equal=bool(np.array_equal(states, s_w) and np.array_equal(table, t_w)), states_equal_site_counts=bool(np.array_equal(states, six)),
               rows_sum_to_states=bool(np.array_equal(table.sum(axis=-1), np.broadcast_to(states[:, None], table.shape[:-1]))),
               occurrences=int(states.sum()), without_letter=int(table[..., 4].sum()))
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir)), flush=True)
