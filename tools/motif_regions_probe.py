"""Measurements of motif methylation inside annotated regions (tools/gpu_motif_regions.sh; results: profiles/r30/motif_regions.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs), `motif_discovery` on them (its
               bin-motifs.tsv names the motifs), an annotation regions.bed made from the contig lengths (``annotation``: a sparse class
               `island`, one interval on every tenth contig; a dense class `gene`, 900 bp of every 1000, stranded) and `motif_regions
               --upstream 50 --region_sites --intervals` twice, one cold process each; wall clocks, the split the command records (ingest
               / engine / text), the flags and the sizes of the five files
  trace DIR    the count passes only, one process on the files of DIR, two repetitions each, in this order: `upload_regions` of no
               interval, of the sparse class alone, of the file's three classes and of eight dense classes (regions_raster_kernel), each
               followed on the candidates of bin-motifs.tsv and on the one-letter background candidates (every A / every C of every bin:
               dense sites) by `motif_site_counts` (sites_kernel's count pass, the yardstick: the same loads and walks) and
               `motif_regions_counts`.  The order of the calls goes to DIR/calls.json for the reader of the kernel trace; with no
               interval the outside cell is compared with the site counts, with classes the cells of a class that covers every contig
  table DIR    the dispatches of the kernel trace against calls.json: per call and repetition the summed kernel time (no GPU)
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

REGIONS = ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--bin_motifs", "out/bin-motifs.tsv", "--regions", "regions.bed", "--upstream", "50", "--region_sites",
           "--intervals", "--out", "regions"]
NAMES = ("motif-regions.tsv", "motif-regions-contigs.tsv", "motif-regions-bins.tsv", "region-sites.bed", "motif-regions-intervals.tsv")
KERNELS = ("sites_kernel", "regions_kernel", "regions_raster_kernel", "regions_covered_kernel")


def annotation(names, lengths):
    """[(contig, start, end, class, strand)]: `island` = the second tenth of every tenth contig; `gene` = [1000 k + 50, 1000 k + 950) all
    along every contig, strands alternating."""
    rows = []
    for i, (n, length) in enumerate(zip(names, lengths)):
        if i % 10 == 0 and length >= 10:
            rows.append((n, length // 10, length // 5, "island", "."))
        rows += [(n, s + 50, min(s + 950, length), "gene", "+-"[(s // 1000) % 2]) for s in range(0, length - 60, 1000)]
    return rows


def files(tmp, total_bp):
    import torch
    from nanomotif_amd import e2e_synth, synth
    spec = synth.config("cfg3") if total_bp == 100_000_000 else synth.SynthSpec(
        n_contigs=max(8, total_bp // 100_000), total_bp=total_bp, n_bins=max(2, total_bp // 2_000_000), mod_types=("a", "m"), seed=1)
    mg = synth.make_metagenome(spec)
    t0 = time.perf_counter()
    sizes = e2e_synth.write_text_inputs(mg, tmp, torch.device("cuda", 0))
    rows = annotation(mg.names, [int(x) for x in mg.lengths])
    with open(os.path.join(tmp, "regions.bed"), "w") as f:
        f.write("".join(f"{n}\t{s}\t{e}\t{c}\t0\t{st}\n" for n, s, e, c, st in rows))
    out = {"mode": "files", "total_bp": total_bp, "rows": sizes["rows"], "bed_bytes": sizes["bed_bytes"], "intervals": len(rows), "written_in_s": time.perf_counter() - t0}
    torch.cuda.empty_cache()
    out["motif_discovery_wall_s"] = cli(tmp, "motif_discovery", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "out"])
    out["motif_rows"] = len(open(os.path.join(tmp, "out", "bin-motifs.tsv")).read().splitlines()) - 1
    for rep in ("cold", "again"):
        wall = cli(tmp, "motif_regions", REGIONS)
        t = json.load(open(os.path.join(tmp, "regions", "logs", "timings.motif_regions.json")))
        out["motif_regions_" + rep] = dict(wall_s=wall, **t)
    table = [l.split("\t") for l in open(os.path.join(tmp, "regions", "motif-regions.tsv")).read().splitlines()]
    col = {name: j for j, name in enumerate(table[0])}
    zs = sorted(abs(float(r[col["z"]])) for r in table[1:])
    out.update(rows_main=len(table) - 1, flags={f: sum(r[-1] == f for r in table[1:]) for f in ("none", "depleted", "enriched", "few_sites")},
               abs_z_max=zs[-1] if zs else None, abs_z_median=zs[len(zs) // 2] if zs else None,
               out_bytes={n: os.path.getsize(os.path.join(tmp, "regions", n)) for n in NAMES})
    return out


def trace(tmp):
    from nanomotif_amd import loading, regions
    from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL, Motif
    eng, cands, ingest_s, _, _ = load(tmp, "pileup.bed")
    flat = [c.engine_candidate() for c in cands]
    mod_types = loading.kept_mod_types(eng)
    background = [(Motif(MOD_TYPE_TO_CANONICAL[mt], 0), mt, b) for b in sorted(eng.bin_index) if eng.bin_contigs(b) for mt in mod_types]
    t0 = time.perf_counter()
    rs = regions.read_regions(os.path.join(tmp, "regions.bed"), eng.contig_index, eng.contig_lengths)
    out = {"mode": "trace", "ingest_s": ingest_s, "read_regions_s": time.perf_counter() - t0, "candidates": len(flat), "background_candidates": len(background),
           "intervals": len(rs), "classes": rs.class_names}
    n = len(eng.contig_names)
    whole = (np.arange(n), np.zeros(n, np.uint64), eng.contig_lengths)
    island = rs.cls == rs.class_names.index("island")
    sets = {"none": ([], [], [], [], ["island"]),
            "sparse": (rs.contig[island], rs.start[island], rs.end[island], np.zeros(int(island.sum()), np.uint8), ["island"]),
            "file": (rs.contig, rs.start, rs.end, rs.cls, rs.class_names),
            "dense8": (np.tile(whole[0], 8), np.tile(whole[1], 8), np.tile(whole[2], 8), np.repeat(np.arange(8), n), [f"c{c}" for c in range(8)])}
    res, order = {}, []

    def timed(name, kernel, fn, reps=2):
        ts = []
        for rep in range(reps):
            before = eng.stats()["launches"]
            t0 = time.perf_counter()
            res[name] = fn()
            ts.append(time.perf_counter() - t0)
            order.append({"call": name, "rep": rep, "kernel": kernel, "launches": eng.stats()["launches"] - before})
        out[name + "_s"] = ts
    for key, args in sets.items():
        timed(f"upload_{key}", "regions_raster_kernel", lambda a=args: eng.upload_regions(*a))
        out[f"pieces_{key}"] = regions.piece_count(args[1], args[2])
        out[f"covered_bp_{key}"] = int(eng.region_covered().sum())
        for group, cs in (("motifs", flat), ("background", background)):
            timed(f"{group}_site_counts_{key}", "sites_kernel", lambda cs=cs: eng.motif_site_counts(cs))
            timed(f"{group}_regions_counts_{key}", "regions_kernel", lambda cs=cs: list(eng.motif_regions_counts(cs)))
            six = [t for _, t in res[f"{group}_site_counts_{key}"]]
            cell = {"none": 1, "dense8": 7}.get(key)
            if cell is not None:
                out[f"{group}_{key}_equal_site_counts"] = bool(all(np.array_equal(t[:, cell].reshape(len(t), 6), s)
                                                                   for (_, t), s in zip(res[f"{group}_regions_counts_{key}"], six)))
            out[f"{group}_sites"] = int(sum(int(s.sum()) for s in six))
    with open(os.path.join(tmp, "calls.json"), "w") as f:
        json.dump(order, f)
    eng.close()
    return out


def table(tmp, trace_csv):
    """The dispatches of the traced kernels in time order against calls.json: per call and repetition the summed kernel time (us).
    regions_covered_kernel (the probe reads the covered positions after every upload) belongs to no call and is left out."""
    import csv
    calls = json.load(open(os.path.join(tmp, "calls.json")))
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    disp = [(next(k for k in KERNELS if k in r["Kernel_Name"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            for r in rows if any(k in r["Kernel_Name"] for k in KERNELS)]
    disp = [d for d in disp if d[0] != "regions_covered_kernel"]
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
