"""Measurements of the k-mer methylation table (tools/gpu_motif_kmers.sh; results: profiles/r20/motif_kmers.md).

  files DIR    BASELINE cfg 3 (100 Mbp, 1000 contigs, 50 bins, 6mA + 5mC) as FILES in DIR (a tmpfs) and `motif_kmers` (default shape) as a
               cold process; the wall clock and the split the command records (ingest / engine / text)
  trace DIR    one process on the files of DIR under `rocprofv3 --kernel-trace`: for every bin x kept mod type the count pass of
               sites_kernel on the one-letter motifs (`motif_site_counts`: the yardstick of every earlier unit), then `kmer_methylation` at
               F = 0, 3, 5, 6 through the workgroup's LDS table and with NM_KMER_GLOBAL_ATOMICS=1, and at F = 7, 10 (global only; F = 10 on
               the first ten bins, with a yardstick of its own), each at NM_KMER_RUN_CHUNKS = 4, 16, 64, two repetitions.  Then the same
               on an input made in memory where half of the one bin is a homopolymer: one hot cell.  Every table is compared with the
               first one of its shape.  The calls and their launch counts go to DIR/calls.json in order.
  table DIR CSV  no GPU: the kernel trace's dispatches matched to calls.json in order, as the markdown table of the profile
One JSON line per mode on stdout."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {0: "*", 3: "N*NN", 5: "NN*NNN", 6: "NNN*NNN", 7: "NNNN*NNN", 10: "NNNNN*NNNNN"}
RUNS = (4, 16, 64)
F10_BINS = 10
HOMOPOLYMER_BP = 8_000_000


def files(tmp, total_bp):
    import torch
    from motif_compare_probe import cli
    from nanomotif_amd import e2e_synth, synth
    spec = synth.config("cfg3") if total_bp == 100_000_000 else synth.SynthSpec(
        n_contigs=max(8, total_bp // 100_000), total_bp=total_bp, n_bins=max(2, total_bp // 2_000_000), mod_types=("a", "m"), seed=1)
    mg = synth.make_metagenome(spec)
    t0 = time.perf_counter()
    sizes = e2e_synth.write_text_inputs(mg, tmp, torch.device("cuda", 0))
    out = {"mode": "files", "total_bp": total_bp, "rows": sizes["rows"], "bed_bytes": sizes["bed_bytes"], "written_in_s": time.perf_counter() - t0}
    torch.cuda.empty_cache()
    wall = cli(tmp, "motif_kmers", ["assembly.fasta", "pileup.bed", "-c", "contig_bin.tsv", "--out", "km"])
    out["motif_kmers_cold"] = dict(wall_s=wall, **json.load(open(os.path.join(tmp, "km", "logs", "timings.motif_kmers.json"))))
    out["out_bytes"] = {n: os.path.getsize(os.path.join(tmp, "km", n)) for n in os.listdir(os.path.join(tmp, "km")) if n.endswith(".tsv")}
    return out


def sweep(eng, label, requests, calls):
    """Every configuration on one resident input; appends (label, kernel, launches) to ``calls``.  Returns whether all tables agree."""
    from nanomotif_amd.motif import MOD_TYPE_TO_CANONICAL, Motif
    ok = True

    def yardstick(reqs, tag):
        for rep in range(2):
            before = eng.stats()["launches"]
            eng.motif_site_counts([(Motif(MOD_TYPE_TO_CANONICAL[mt], 0), mt, b) for mt, b in reqs])
            calls.append({"input": label, "call": "sites_count" + tag, "kernel": "sites_kernel", "launches": eng.stats()["launches"] - before})
    yardstick(requests, "")
    few = [r for r in requests if r[1] in sorted({b for _, b in requests})[:F10_BINS]]
    if len(few) != len(requests):
        yardstick(few, "_f10_bins")
    for flanks, shape in SHAPES.items():
        reqs = few if flanks == 10 else requests
        first = None
        for path in (("lds", "global") if flanks <= 6 else ("global",)):
            for run in RUNS:
                os.environ["NM_KMER_RUN_CHUNKS"] = str(run)
                if path == "global":
                    os.environ["NM_KMER_GLOBAL_ATOMICS"] = "1"
                try:
                    for rep in range(2):
                        before = eng.stats()["launches"]
                        totals, table = eng.kmer_methylation(reqs, shape)
                        calls.append({"input": label, "call": f"F={flanks} {path} R={run}", "kernel": "kmer_kernel", "launches": eng.stats()["launches"] - before})
                finally:
                    os.environ.pop("NM_KMER_RUN_CHUNKS", None)
                    os.environ.pop("NM_KMER_GLOBAL_ATOMICS", None)
                if first is None:
                    first = (totals, table)
                ok = ok and np.array_equal(first[0], totals) and np.array_equal(first[1], table)
                del totals, table
    return ok


def homopolymer_engine():
    """One bin in memory: eight random 1 Mbp contigs and one 8 Mbp run of A; 30 % of the (position, strand) pairs carry a call."""
    from nanomotif_amd.engine import ScanEngine
    rng = np.random.default_rng(5)
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1_000_000)] for _ in range(8)] + [np.full(HOMOPOLYMER_BP, ord("A"), np.uint8)]
    names = [f"c{i}" for i in range(len(seqs))]
    eng = ScanEngine()
    eng.upload_assembly(names, seqs, ["hot"] * len(seqs))
    cid, pos, st, fr = [], [], [], []
    for i, s in enumerate(seqs):
        p, strand = np.nonzero(rng.random((len(s), 2)) < 0.3)
        cid.append(np.full(len(p), i, np.uint32)); pos.append(p.astype(np.uint32))
        st.append(np.where(strand == 0, ord("+"), ord("-")).astype(np.uint8)); fr.append(rng.choice([0.0, 0.5, 1.0], size=len(p)))
    eng.upload_pileup("a", np.concatenate(cid), np.concatenate(pos), np.concatenate(st), np.concatenate(fr))
    return eng


def trace(tmp):
    from nanomotif_amd import loading
    eng, _, ingest_s = load_files(tmp)
    mod_types = loading.kept_mod_types(eng)
    requests = [(mt, b) for b in sorted(b for b in eng.bin_index if eng.bin_contigs(b)) for mt in mod_types]
    calls = []
    out = {"mode": "trace", "ingest_s": ingest_s, "requests": len(requests)}
    out["cfg3_tables_agree"] = bool(sweep(eng, "cfg3", requests, calls))
    eng.close()
    hot = homopolymer_engine()
    out["homopolymer_tables_agree"] = bool(sweep(hot, "homopolymer", [("a", "hot")], calls))
    hot.close()
    json.dump(calls, open(os.path.join(tmp, "calls.json"), "w"))
    return out


def load_files(tmp):
    """The engine on the files of ``tmp`` (no bin-motifs.tsv is needed)."""
    from nanomotif_amd import loading
    args = argparse.Namespace(assembly=os.path.join(tmp, "assembly.fasta"), pileup=os.path.join(tmp, "pileup.bed"), contig_bin=os.path.join(tmp, "contig_bin.tsv"),
                              files=None, directory=None, extension=".fasta", threads=1, methylation_threshold_low=0.3, methylation_threshold_high=0.7)
    t0 = time.perf_counter()
    eng = loading.load_engine(args, 0, None)
    return eng, None, time.perf_counter() - t0


def table(tmp, trace_csv):
    """The dispatches of kmer_kernel and of sites_kernel in time order against calls.json: per call the summed kernel time of its best
    repetition (us) and its ratio to the input's yardstick."""
    calls = json.load(open(os.path.join(tmp, "calls.json")))
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    disp = [(("kmer_kernel" if "kmer_kernel" in r["Kernel_Name"] else "sites_kernel"), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            for r in rows if "kmer_kernel" in r["Kernel_Name"] or "sites_kernel" in r["Kernel_Name"]]
    at, best = 0, {}
    for c in calls:
        ns = 0
        for _ in range(c["launches"]):
            assert disp[at][0] == c["kernel"], (c, at)
            ns += disp[at][1]
            at += 1
        key = (c["input"], c["call"])
        best[key] = min(best.get(key, ns), ns)
    assert at == len(disp), (at, len(disp))
    lines = ["| input | call | kernel time, us | / sites count pass |", "|---|---|---:|---:|"]
    for (inp, call), ns in best.items():
        yard = best[(inp, "sites_count_f10_bins")] if call.startswith("F=10") and (inp, "sites_count_f10_bins") in best else best[(inp, "sites_count")]
        lines.append(f"| {inp} | {call} | {ns / 1000:.1f} | {ns / yard:.2f} |")
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["files", "trace", "table"])
    ap.add_argument("dir")
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--total-bp", type=int, default=100_000_000)
    a = ap.parse_args()
    if a.mode == "table":
        print(table(a.dir, a.csv))
    else:
        print(json.dumps(files(a.dir, a.total_bp) if a.mode == "files" else trace(a.dir)), flush=True)
