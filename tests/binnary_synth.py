"""A synthetic metagenome for the binnary commands: three bins with distinct planted motifs (one 6mA and one 5mC motif each).
In the contig-bin file one contig of bin A is listed under bin B (a contaminant of B) and one contig of bin A is left out
(an unbinned contig that belongs to A)."""
import os

import numpy as np
import pandas as pd

from nanomotif_amd import synth

BIN_MOTIFS = {
    "bin_000": [("GATC", 1, "a"), ("CCWGG", 1, "m")],
    "bin_001": [("GAATTC", 2, "a"), ("GCGC", 1, "m")],
    "bin_002": [("ACCCA", 4, "a"), ("CCGG", 1, "m")],
}
BIN_A, BIN_B = "bin_000", "bin_001"


def make_metagenome():
    mg = synth.make_metagenome(synth.SynthSpec(n_contigs=18, total_bp=540_000, n_bins=3, mod_types=("a", "m"), seed=21,
                                               lognormal_sigma=0.3, min_contig_bp=10_000))
    mg.bin_motifs = {b: list(m) for b, m in BIN_MOTIFS.items()}
    return mg


def layout(mg):
    """(moved contig, unbinned contig, contig -> listed bin): the moved contig is bin A's shortest (bin B's own cluster keeps the
    >= 85 % of B's length that detection needs), the unbinned one its longest."""
    a = sorted([i for i, b in enumerate(mg.bin_names) if b == BIN_A], key=lambda i: int(mg.lengths[i]))
    moved, unbinned = mg.names[a[0]], mg.names[a[-1]]
    listed = {n: (BIN_B if n == moved else b) for n, b in zip(mg.names, mg.bin_names) if n != unbinned}
    return moved, unbinned, listed


def write_inputs(mg, out_dir):
    """assembly.fasta, pileup.bed, contig_bin.tsv (the layout above), bin-motifs.tsv (the planted motifs) -> their paths."""
    os.makedirs(out_dir, exist_ok=True)
    paths = {k: os.path.join(out_dir, f) for k, f in (("assembly", "assembly.fasta"), ("pileup", "pileup.bed"),
                                                       ("contig_bins", "contig_bin.tsv"), ("bin_motifs", "bin-motifs.tsv"))}
    mg.write_fasta(paths["assembly"])
    mg.write_bed(paths["pileup"])
    _, _, listed = layout(mg)
    with open(paths["contig_bins"], "w") as f:
        for n, b in listed.items():
            f.write(f"{n}\t{b}\n")
    rows = [dict(bin=b, mod_type=mt, motif=m, mod_position=p, n_mod_bin=900, n_nomod_bin=100) for b, ms in BIN_MOTIFS.items() for m, p, mt in ms]
    pd.DataFrame(rows).to_csv(paths["bin_motifs"], sep="\t", index=False)
    return paths


def oracle_table(mg, output_type="median"):
    """The read-methylation table by the CPU oracle (oracle/contig_methylation.read_methylation) on the rows write_bed writes."""
    from nanomotif_amd.motif import iupac_to_regex
    from oracle.contig_methylation import read_methylation
    records = {}
    for i, name in enumerate(mg.names):
        for mt in mg.spec.mod_types:
            p = mg.contig_pileup(i, mt)
            cov = p["nvalid"].astype(np.int64)
            nmod = np.array([int(round(c * q / 10000)) for c, q in zip(cov.tolist(), p["pct_hundredths"].tolist())], dtype=np.int64)
            records[(name, mt)] = dict(position=p["position"], strand=p["strand"], n_valid=cov, n_mod=nmod, n_diff=np.zeros_like(cov))
    contigs = {n: mg.contig_str(i) for i, n in enumerate(mg.names)}
    motifs = [m for ms in BIN_MOTIFS.values() for m in ms]
    rows = read_methylation(records, contigs, [(iupac_to_regex(m), mt, p) for m, p, mt in motifs], output_type=output_type)
    return pd.DataFrame([dict(contig=r["contig"], motif=motifs[r["motif"]][0], mod_type=motifs[r["motif"]][2], mod_position=motifs[r["motif"]][1],
                              methylation_value=r["methylation_value"], mean_read_cov=r["mean_read_cov"], n_motif_obs=r["n_motif_obs"])
                         for r in rows])
