"""Measurements of motif overlap (tools/gpu_motif_overlap.sh; results: profiles/r24/motif_overlap.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs) and `motif_overlap --all_pairs` twice, one cold process each; wall clocks, the split the
               command records (ingest / engine / text), the relations, the flags and the sizes of the two files
  trace DIR    the count passes only, one process on the files of DIR, two repetitions each, in this order on the candidates of
               bin-motifs.tsv: `motif_site_counts` (sites_kernel's count pass, the yardstick: the same loads and the same two walks),
               `motif_overlap` without partners (what the kernel costs beside the walks: two more blocks), with all other motifs of the
               set as partners (the command's first call), and with PADDED partner lists of 4 and of 16 motifs — the set's other motifs
               repeated, the rest unrelated — where by walk count the kernel should cost (1 + P) count passes.  The order of the calls
               goes to DIR/calls.json for the reader of the kernel trace; block 0 of every table is compared with the site counts first
  table DIR    the dispatches of the two kernels in the trace against calls.json: per call and repetition the summed kernel time
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

OVERLAP = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--out", "ov", "--all_pairs"]
NAMES = ("motif-overlap.tsv", "motif-overlap-motifs.tsv")
PADDED = (4, 16)
UNRELATED = ("GTAC", 2), ("CTAG", 2), ("ACGT", 0), ("TGCA", 3)          # partners that share next to nothing with a discovered motif


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
        wall = cli(tmp, "motif_overlap", OVERLAP)
        t = json.load(open(os.path.join(tmp, "ov", "logs", "timings.motif_overlap.json")))
        out["motif_overlap_" + rep] = dict(wall_s=wall, **t)
    pairs = [l.split("\t") for l in open(os.path.join(tmp, "ov", NAMES[0])).read().splitlines()[1:]]
    motifs = [l.split("\t") for l in open(os.path.join(tmp, "ov", NAMES[1])).read().splitlines()[1:]]
    count = lambda rows, j: {v: sum(r[j] == v for r in rows) for v in sorted({r[j] for r in rows})}
    out.update(pairs=len(pairs), motifs=len(motifs), relations=count(pairs, -2), symbolic=count(pairs, -1), flags=count(motifs, -1),
               flagged_rows=[r for r in motifs if r[-1] not in ("none", "few_sites")][:20],
               out_bytes={n: os.path.getsize(os.path.join(tmp, "ov", n)) for n in NAMES})
    return out


def load(tmp):
    from nanomotif_amd import loading, motif_sites as ms
    from nanomotif_amd.motif_coverage import build_sets
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=os.path.join(tmp, "pileup.bed"), contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0, None)
    ingest_s = time.perf_counter() - t0
    cands = ms.candidates_of_files([os.path.join(tmp, "out", "bin-motifs.tsv")])
    bins = [b for b in eng.bin_index if eng.bin_contigs(b)]
    sets = [s for s in build_sets(bins, loading.kept_mod_types(eng), cands) if s.candidates]
    return eng, sets, ingest_s


def trace(tmp):
    from nanomotif_amd.motif import Motif
    eng, sets, ingest_s = load(tmp)
    flat, others = [], []
    for s in sets:
        motifs = [c.engine_candidate()[0] for c in s.candidates]
        for i, c in enumerate(s.candidates):
            flat.append(c.engine_candidate())
            others.append(motifs[:i] + motifs[i + 1:])
    fill = [Motif(m, p) for m, p in UNRELATED]

    def padded(n):
        return [(p * n + fill * n)[:n] if p else (fill * n)[:n] for p in others]
    mean_p = float(np.mean([len(p) for p in others])) if others else 0.0
    out = {"mode": "trace", "ingest_s": ingest_s, "sets": len(sets), "candidates": len(flat), "mean_partners_all_others": mean_p, "padded": list(PADDED)}
    calls = [("site_counts", "sites_kernel", lambda: eng.motif_site_counts(flat)),
             ("overlap_no_partner", "overlap_kernel", lambda: list(eng.motif_overlap(flat, [[] for _ in flat]))),
             ("overlap_all_others", "overlap_kernel", lambda: list(eng.motif_overlap(flat, others)))]
    calls += [(f"overlap_padded_{n}", "overlap_kernel", lambda n=n: list(eng.motif_overlap(flat, padded(n)))) for n in PADDED]
    res, order = {}, []
    for name, kernel, fn in calls:
        ts = []
        for rep in range(2):
            before = eng.stats()["launches"]
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
            order.append({"call": name, "rep": rep, "kernel": kernel, "launches": eng.stats()["launches"] - before})
        out[name + "_s"] = ts
    with open(os.path.join(tmp, "calls.json"), "w") as f:
        json.dump(order, f)
    six = [t for _, t in res["site_counts"]]
    for name in [c[0] for c in calls[1:]]:
        out[name + "_block0_equals_site_counts"] = bool(all(np.array_equal(t[0].reshape(len(s), 6), s) for (_, t), s in zip(res[name], six)))
    out["no_partner_rest_equals_own"] = bool(all(np.array_equal(t[0], t[1]) for _, t in res["overlap_no_partner"]))
    out["sites"] = int(sum(int(s.sum()) for s in six))
    out["shared_sites_all_others"] = int(sum(int(t[1:-1].sum()) for _, t in res["overlap_all_others"]))
    eng.close()
    return out


def table(tmp, trace_csv):
    """The dispatches of the two count kernels in time order against calls.json: per call and repetition the summed kernel time (us)."""
    import csv
    calls = json.load(open(os.path.join(tmp, "calls.json")))
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    kernels = ("sites_kernel", "overlap_kernel")
    disp = [(next(k for k in kernels if k in r["Kernel_Name"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            for r in rows if any(k in r["Kernel_Name"] for k in kernels)]
    at, out = 0, {}
    for c in calls:
        ns = 0
        for _ in range(c["launches"]):
            assert disp[at][0] == c["kernel"], (c, at, disp[at])
            ns += disp[at][1]
            at += 1
        out.setdefault(c["call"], []).append(round(ns / 1000.0, 1))
    assert at == len(disp), (at, len(disp))
    return {"mode": "table", "kernel_us": out}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace", "table"])
    ap.add_argument("dir")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    ap.add_argument("--trace-csv", default=None)
    a = ap.parse_args()
    print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir) if a.mode == "trace" else table(a.dir, a.trace_csv)), flush=True)
