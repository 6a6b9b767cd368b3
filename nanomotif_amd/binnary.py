"""Bin contamination and contig inclusion from contig methylation ("binnary"; reference: nanomotif/binnary/data_processing.py,
detect_contamination.py, include_contigs.py).

The reference works on polars frames; this port uses pandas / numpy and keeps every ordering the results depend on: the
clustering and the classifiers see the same matrices (rows: contigs in the order of the (bin, contig, motif_mod) sort, columns:
motif_mod sorted), the pseudo-methylation of unbinned contigs draws from numpy's GLOBAL legacy generator over the sorted
(contig, motif_mod) cross join, and the output frames carry polars' column order.  Where polars' own order is unspecified (a sort
with equal keys) the rows keep the order the methods were listed in (stable sorts).

The models are scikit-learn's, imported when a function needs them so that ``motif_discovery`` never imports scikit-learn.
HDBSCAN: the reference uses the ``hdbscan`` package with ``min_samples=3``; ``sklearn.cluster.HDBSCAN`` counts the point itself
in ``min_samples`` and the package does not, so the same clustering is ``min_samples=4`` here (HDBSCAN_PARAMS)."""
from __future__ import annotations

import gzip
import logging
import os

import numpy as np
import pandas as pd

UNBINNED = "unbinned"
CONTAMINATION_COLUMNS = ["contig", "bin", "method", "cluster", "bin_cluster", "bin_length", "n_contigs_bin", "fraction_contigs",
                         "fraction_length"]
INCLUDE_COLUMNS = ["contig", "bin", "assigned_bin", "method", "prob", "mean_prob", "confidence"]
# the package's HDBSCAN(min_samples=3, ...) (detect_contamination.py:57) in scikit-learn's convention
HDBSCAN_PARAMS = dict(min_samples=4, min_cluster_size=2, metric="euclidean", allow_single_cluster=False)
PCA_VARIANCE = 0.90

log = logging.getLogger(__name__)


# ---- input ----------------------------------------------------------------------------------------------------------------
def load_contig_bins(path) -> pd.DataFrame:
    """The contig-bin file: two tab-separated columns without a header (data_processing.py:24-28); read as text."""
    df = pd.read_csv(path, sep="\t", header=None, dtype=str, keep_default_na=False, usecols=[0, 1])
    df.columns = ["contig", "bin"]
    return df


def motif_mods_of_bin_motifs(path) -> list:
    """The unique ``motif_mod`` strings (motif_modtype_position) of a bin-motifs.tsv (main.py:129-133), first-seen order."""
    bm = pd.read_csv(path, sep="\t", dtype={"motif": str, "mod_type": str})
    mm = bm["motif"].astype(str) + "_" + bm["mod_type"].astype(str) + "_" + bm["mod_position"].astype(int).astype(str)
    return list(dict.fromkeys(mm.tolist()))


def read_fasta(path) -> dict:
    """record id -> sequence text as in the file, like ``{r.id: str(r.seq) for r in SeqIO.parse(handle, "fasta")}``
    (data_processing.py:34-52): the id is the header up to the first whitespace, the sequence the record's lines joined with
    spaces and carriage returns removed, a repeated id keeps the last record."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"File not found: {path}")
    valid = [".fasta", ".fa", ".fna", ".gz"]
    if not any(str(path).endswith(e) for e in valid):
        raise ValueError(f"Unsupported file extension. Please provide a FASTA file with one of the following extensions: {', '.join(valid)}")
    opener = gzip.open if str(path).endswith(".gz") else open
    out, name, lines = {}, None, []
    with opener(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    out[name] = "".join(lines).replace(" ", "").replace("\r", "")
                title = line[1:].rstrip()
                name = title.split(None, 1)[0] if title.split() else ""
                lines = []
            elif name is not None:
                lines.append(line.rstrip())
    if name is not None:
        out[name] = "".join(lines).replace(" ", "").replace("\r", "")
    return out


def contig_lengths(assembly: dict) -> pd.DataFrame:
    return pd.DataFrame({"contig": list(assembly), "length": [len(s) for s in assembly.values()]})


# ---- table preparation (data_processing.py) -------------------------------------------------------------------------------
def filter_methylation(table: pd.DataFrame, methylation_threshold) -> pd.DataFrame:
    """Rows with n_motif_obs * mean_read_cov >= threshold (main.py:193)."""
    keep = table["n_motif_obs"].astype(np.float64) * table["mean_read_cov"].astype(np.float64) >= methylation_threshold
    return table[keep].reset_index(drop=True)


def add_bin(contig_methylation: pd.DataFrame, contig_bins: pd.DataFrame) -> pd.DataFrame:
    """data_processing.py:175-189: motif_mod, the bin of every contig ('unbinned' when it has none)."""
    cm = contig_methylation.copy()
    cm["motif_mod"] = cm["motif"].astype(str) + "_" + cm["mod_type"].astype(str) + "_" + cm["mod_position"].astype(int).astype(str)
    cm = cm.merge(contig_bins[["contig", "bin"]], on="contig", how="left")
    cm["bin"] = cm["bin"].fillna(UNBINNED)
    return cm.drop(columns=["mod_position", "mod_type", "motif"])


def impute_contig_methylation_within_bin(contig_methylation: pd.DataFrame) -> pd.DataFrame:
    """data_processing.py:192-223: every binned contig gets every motif_mod of its bin; a missing value is the bin's
    n_motif_obs-weighted mean.  Sorted by (bin, contig, motif_mod)."""
    cm = contig_methylation[contig_methylation["bin"] != UNBINNED]
    w = cm.assign(_wv=cm["methylation_value"] * cm["n_motif_obs"])
    g = w.groupby(["bin", "motif_mod"], sort=False)
    bin_methylation = (g["_wv"].sum() / g["n_motif_obs"].sum()).rename("mean_bin_methylation").reset_index()
    cross = cm[["contig", "bin"]].drop_duplicates()
    out = cross.merge(bin_methylation, on="bin", how="left").merge(cm, on=["bin", "contig", "motif_mod"], how="left")
    out = out.sort_values(["bin", "contig", "motif_mod"], kind="stable").reset_index(drop=True)
    out["methylation_value"] = out["methylation_value"].where(out["methylation_value"].notna(), out["mean_bin_methylation"])
    return out.drop(columns=["n_motif_obs"])


def impute_unbinned_contigs(contig_methylation: pd.DataFrame) -> pd.DataFrame:
    """data_processing.py:225-252: every unbinned contig gets every motif_mod of the table; a missing value is a draw of
    ``np.random.uniform(0.0, 0.15)`` (the global legacy generator) in (contig, motif_mod) order."""
    unb = contig_methylation[contig_methylation["bin"] == UNBINNED]
    motif_mods = pd.DataFrame({"motif_mod": contig_methylation["motif_mod"].unique()})
    contigs = pd.DataFrame({"contig": unb["contig"].unique()})
    cross = motif_mods.merge(contigs, how="cross")
    cross["bin"] = UNBINNED
    cross = cross.sort_values(["contig", "motif_mod"], kind="stable").reset_index(drop=True)
    cross["pseudo_methylation"] = np.random.uniform(0.0, 0.15, size=len(cross))
    out = cross.merge(unb, on=["contig", "motif_mod", "bin"], how="left")
    out["methylation_value"] = out["methylation_value"].where(out["methylation_value"].notna(), out["pseudo_methylation"])
    out = out.drop(columns=["pseudo_methylation"])
    return out.sort_values(["contig", "motif_mod"], kind="stable").reset_index(drop=True)


def create_matrix(contig_methylation: pd.DataFrame):
    """data_processing.py:255-269: contigs x motif_mod (rows in first-appearance order, columns sorted), missing = 0."""
    cm = contig_methylation[["contig", "motif_mod", "methylation_value"]]
    contigs = list(dict.fromkeys(cm["contig"].tolist()))
    if cm.duplicated(["contig", "motif_mod"]).any():
        raise ValueError("create_matrix: more than one value for a (contig, motif_mod)")
    m = cm.pivot(index="contig", columns="motif_mod", values="methylation_value")
    m = m.reindex(index=contigs, columns=sorted(m.columns)).astype(np.float64).fillna(0.0)
    return contigs, m.to_numpy()


def load_contamination_file(path) -> pd.DataFrame:
    contamination = pd.read_csv(path, sep="\t", dtype=str, keep_default_na=False)
    if "contig" not in contamination.columns:
        raise ValueError("The contamination file does not contain the required columns.")
    return contamination


def create_contig_bin_file(contig_bins: pd.DataFrame, contamination: pd.DataFrame, include: pd.DataFrame = None) -> pd.DataFrame:
    """data_processing.py:289-300: the contaminants out, the included contigs in, sorted by (bin, contig)."""
    contig_bins = contig_bins[~contig_bins["contig"].isin(contamination["contig"])]
    if include is not None:
        contig_bins = pd.concat([contig_bins, include[["contig", "bin"]]], ignore_index=True)
    return contig_bins.sort_values(by=["bin", "contig"], kind="stable")


def generate_output(df: pd.DataFrame, outdir, filename, header=True):
    if outdir and not os.path.exists(outdir):
        os.makedirs(outdir)
    df.to_csv(os.path.join(outdir, filename), sep="\t", index=False, header=header)


def write_bins_from_contigs(new_contig_bins: pd.DataFrame, assembly: dict, output_dir):
    """data_processing.py:55-93: OUT/<bin>.fa per bin, records as Biopython's FASTA writer lays them out (``>id``, 60 bases per
    line)."""
    os.makedirs(output_dir, exist_ok=True)
    for bin_name, group in new_contig_bins.groupby("bin"):
        n = 0
        with open(os.path.join(output_dir, f"{bin_name}.fa"), "w") as f:
            for contig in group["contig"]:
                if contig not in assembly:
                    continue
                seq = assembly[contig]
                f.write(f">{contig}\n")
                for i in range(0, len(seq), 60):
                    f.write(seq[i:i + 60] + "\n")
                n += 1
        log.info(f"Written {n} contigs to {bin_name}.fa")


# ---- the analyses -----------------------------------------------------------------------------------------------------------
def _bin_of(contig_methylation: pd.DataFrame) -> pd.DataFrame:
    return contig_methylation[["bin", "contig"]].drop_duplicates()


def detect_contamination(contig_methylation: pd.DataFrame, contig_lengths: pd.DataFrame, num_consensus=4, threads=1,
                         spectral_n_neighbors=10) -> pd.DataFrame:
    """detect_contamination.py:8-138: four clusterings of the binned contigs' methylation (PCA to 90 % of the variance); in
    every bin the cluster holding >= 85 % of its length is the bin's own; a contig outside it for >= num_consensus methods is
    a contaminant.  Returns its rows (CONTAMINATION_COLUMNS), sorted by (bin, contig)."""
    from sklearn.cluster import HDBSCAN, AgglomerativeClustering, SpectralClustering
    from sklearn.decomposition import PCA
    from sklearn.mixture import GaussianMixture

    log.info("Starting contamination detection analysis...")
    cm = impute_contig_methylation_within_bin(contig_methylation)
    n_contigs = _bin_of(cm).groupby("bin")["contig"].count()
    cm = cm[~cm["bin"].isin(n_contigs[n_contigs == 1].index)]         # one-contig bins have nothing to compare
    contig_names, matrix = create_matrix(cm)
    original = matrix.shape[1]
    pca = PCA(n_components=PCA_VARIANCE, svd_solver="full")
    matrix = pca.fit_transform(matrix)
    log.info(f"PCA reduced the feature space from {original} to {matrix.shape[1]} "
             f"(explained variance {pca.explained_variance_ratio_.sum():.2f})")
    n_bins = cm["bin"].nunique()
    labels = {
        "spectral": SpectralClustering(n_clusters=n_bins, affinity="nearest_neighbors", random_state=42, n_jobs=threads,
                                       n_neighbors=spectral_n_neighbors).fit_predict(matrix),
        "agg": AgglomerativeClustering(n_clusters=n_bins).fit(matrix).labels_,
        "hdbscan": HDBSCAN(**HDBSCAN_PARAMS).fit_predict(matrix),
    }
    gmm = GaussianMixture(n_components=n_bins, covariance_type="full", random_state=42)
    gmm.fit(matrix)
    labels["gmm"] = gmm.predict(matrix)

    contig_bin = _bin_of(cm)
    wide = pd.DataFrame({"contig": contig_names, **{k: np.asarray(v) for k, v in labels.items()}}).merge(contig_bin, on="contig")
    results = pd.concat([pd.DataFrame({"contig": wide["contig"], "bin": wide["bin"], "method": m, "cluster": wide[m].astype(np.int64)})
                         for m in ("spectral", "agg", "hdbscan", "gmm")], ignore_index=True)
    lengths = contig_lengths[["contig", "length"]]
    bin_size = contig_bin.merge(lengths, on="contig").groupby("bin", sort=False).agg(bin_length=("length", "sum"),
                                                                                     n_contigs_bin=("contig", "count")).reset_index()
    cluster_sizes = (results.merge(lengths, on="contig").groupby(["bin", "method", "cluster"], sort=False)
                     .agg(n_contigs=("contig", "count"), cluster_length=("length", "sum")).reset_index().merge(bin_size, on="bin"))
    cluster_sizes["fraction_contigs"] = cluster_sizes["n_contigs"] / cluster_sizes["n_contigs_bin"]
    cluster_sizes["fraction_length"] = cluster_sizes["cluster_length"] / cluster_sizes["bin_length"]
    largest = cluster_sizes.groupby(["method", "bin"], sort=False)["cluster_length"].max().reset_index()
    assigned = (largest.merge(cluster_sizes, on=["bin", "method", "cluster_length"], how="left").rename(columns={"cluster": "bin_cluster"})
                .drop(columns=["cluster_length", "n_contigs"]))
    assigned = assigned[assigned["fraction_length"] >= 0.85]
    results = results.merge(assigned, on=["bin", "method"]).sort_values(["bin", "contig"], kind="stable").reset_index(drop=True)
    votes = (results["bin_cluster"] != results["cluster"]).astype(np.int64).groupby(results["contig"]).sum()
    confident = votes[votes >= num_consensus].index
    out = results[results["contig"].isin(confident)].reset_index(drop=True)
    return out[CONTAMINATION_COLUMNS]


def include_contigs(contig_methylation: pd.DataFrame, contig_lengths: pd.DataFrame, mean_probability) -> pd.DataFrame:
    """include_contigs.py:12-166: LDA, KNN (k = 3) and a random forest, trained on the binned contigs (PCA to 90 %), assign every
    unbinned contig; all three agreeing: high (mean probability >= mean_probability) or medium confidence; two agreeing: low.
    Returns INCLUDE_COLUMNS sorted by (confidence, contig)."""
    from sklearn.decomposition import PCA
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.neighbors import KNeighborsClassifier

    log.info("Starting include_contigs analysis...")
    contig_bin = _bin_of(contig_methylation)
    binned = impute_contig_methylation_within_bin(contig_methylation)
    binned_names, binned_matrix = create_matrix(binned)
    pca = PCA(n_components=PCA_VARIANCE, svd_solver="full")
    binned_matrix = pca.fit_transform(binned_matrix)
    y = pd.DataFrame({"contig": binned_names}).merge(contig_bin, on="contig", how="left")["bin"].to_numpy()

    unbinned = impute_unbinned_contigs(contig_methylation)
    completions = (pd.DataFrame({"contig": unbinned["contig"].unique()})
                   .merge(pd.DataFrame({"motif_mod": binned["motif_mod"].unique()}), how="cross")
                   .merge(unbinned, on=["contig", "motif_mod"], how="left"))
    unbinned_names, unbinned_matrix = create_matrix(completions)
    if not unbinned_names:
        return pd.DataFrame({c: [] for c in INCLUDE_COLUMNS})
    unbinned_matrix = pca.transform(unbinned_matrix)

    models = {"lda": LinearDiscriminantAnalysis(), "knn": KNeighborsClassifier(n_neighbors=3),
              "rf": RandomForestClassifier(n_estimators=100, random_state=42)}
    pred, prob = {}, {}
    for name in ("lda", "knn", "rf"):                                    # (the reference fits them in this order)
        fitted = models[name].fit(binned_matrix, y)
        pred[name] = fitted.predict(unbinned_matrix)
        prob[name] = fitted.predict_proba(unbinned_matrix).max(axis=1)
    prob_df = pd.concat([pd.DataFrame({"contig": unbinned_names, "method": m, "pred": pred[m], "prob": prob[m]}) for m in ("rf", "knn", "lda")],
                        ignore_index=True)
    wide = pd.DataFrame({"contig": unbinned_names, **{m: pred[m] for m in ("lda", "knn", "rf")}}).merge(contig_bin, on="contig")
    results = pd.concat([pd.DataFrame({"contig": wide["contig"], "bin": wide["bin"], "method": m, "assigned_bin": wide[m]})
                         for m in ("lda", "knn", "rf")], ignore_index=True)
    n_assigned = results.groupby("contig")["assigned_bin"].nunique()

    high = results[results["contig"].isin(n_assigned[n_assigned == 1].index)].merge(prob_df, on=["contig", "method"])
    high = high.merge(high.groupby("contig")["prob"].mean().rename("mean_prob").reset_index(), on="contig")
    high["confidence"] = np.where(high["mean_prob"] >= mean_probability, "high_confidence", "medium_confidence")
    high = high.sort_values("contig", kind="stable")[INCLUDE_COLUMNS]

    low_rows = results[results["contig"].isin(n_assigned[n_assigned == 2].index)]
    pairs = low_rows.groupby(["contig", "assigned_bin"], sort=False).size().rename("n").reset_index()
    pairs = pairs[pairs["n"] == 2].drop(columns=["n"])
    low = pairs.merge(low_rows, on=["contig", "assigned_bin"]).merge(prob_df, on=["contig", "method"])
    low = low.merge(low.groupby("contig")["prob"].mean().rename("mean_prob").reset_index(), on="contig")
    low["confidence"] = "low_confidence"
    low = low.sort_values("contig", kind="stable")[INCLUDE_COLUMNS]
    out = pd.concat([high, low], ignore_index=True).sort_values(["confidence", "contig"], kind="stable")
    return out.reset_index(drop=True)
