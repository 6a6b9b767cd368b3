"""The binnary layer (nanomotif_amd/binnary.py) and the detect_contamination / include_contigs command line, on the CPU: the
reference's own binnary expectations (tests/binnary/*.py of the reference) on the same literal tables and on its data files
(tests/golden/binnary/: datasets/binnary_testdata of the reference)."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from nanomotif_amd import binnary as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binnary")


def _reference_table(with_unbinned):
    """tests/binnary/test_detect_contamination.py and test_include_contigs.py: three bins of four contigs, motifs m1 m2 m3;
    include_contigs' variant lists contig_3 as unbinned."""
    mv = [0.9, 0.85, 0.0, 0.9, 0.85, 0.001, 0.0, 0.001, 0.9, 0.99, 0.9, 0.05,
          0.04, 0.01, 0.9, 0.0, 0.0, 0.97, 0.1, 0.0, 0.9, 0.0, 0.01, 0.95,
          0.04, 0.9, 0.9, 0.0, 0.92, 0.97, 0.0, 0.99, 0.9, 0.01, 0.99, 0.95]
    bins = ["bin1"] * 12 + ["bin2"] * 12 + ["bin3"] * 12
    if with_unbinned:
        bins[6:9] = ["unbinned"] * 3
    cm = pd.DataFrame(dict(contig=[f"contig_{i}" for i in range(1, 13) for _ in range(3)], bin=bins, methylation_value=mv,
                           n_motif_obs=[1000, 500, 600, 270, 100, 50, 50, 100, 100, 1000, 500, 600] * 3, motif_mod=["m1", "m2", "m3"] * 12))
    lengths = pd.DataFrame(dict(contig=[f"contig_{i}" for i in range(1, 13)], length=[100000, 60000, 20000, 80000] * 3))
    return cm, lengths


def test_detect_contamination_reference_case():
    cm, lengths = _reference_table(False)
    c = bn.detect_contamination(cm, lengths, 4, 1, 10)
    assert c.shape[0] == 4 and c["contig"].unique().tolist() == ["contig_3"]
    assert list(c.columns) == ["contig", "bin", "method", "cluster", "bin_cluster", "bin_length", "n_contigs_bin", "fraction_contigs", "fraction_length"]
    assert c["method"].tolist() == ["spectral", "agg", "hdbscan", "gmm"]
    assert set(c["bin"]) == {"bin1"} and (c["cluster"] != c["bin_cluster"]).all()


def test_include_contigs_reference_case():
    np.random.seed(1)
    cm, lengths = _reference_table(True)
    inc = bn.include_contigs(cm, lengths, 0.80)
    assert inc.shape[0] == 3 and inc["contig"].unique().tolist() == ["contig_3"]
    assert inc["assigned_bin"].unique().tolist() == ["bin2"]
    assert list(inc.columns) == ["contig", "bin", "assigned_bin", "method", "prob", "mean_prob", "confidence"]
    assert set(inc["confidence"]) == {"high_confidence"} and set(inc["bin"]) == {"unbinned"}


def test_loaded_reference_data_and_add_bin():
    """test_data_processing_functions.py: test_feature_with_loaded_data, test_add."""
    contig_bins = bn.load_contig_bins(os.path.join(GOLDEN, "contig_bin.tsv"))
    assert set(contig_bins["bin"]) == {"b1", "b2", "b3", "b4"}
    assert set(contig_bins["contig"]) == {f"contig_{i}" for i in range(1, 14)} | {"contig_16"}
    bin_motifs = pd.read_csv(os.path.join(GOLDEN, "bin-motifs.tsv"), sep="\t")
    assert set(bin_motifs["bin"]) == {"b1", "b2", "b3"}
    scored = pd.read_csv(os.path.join(GOLDEN, "motifs-scored.tsv"), sep="\t")
    with_bin = bn.add_bin(scored, contig_bins)
    assert set(with_bin.columns) == {"contig", "methylation_value", "n_motif_obs", "motif_mod", "bin"}
    assert with_bin[with_bin["contig"] == "contig_1"]["bin"].unique().tolist() == ["b1"]
    assert set(bn.motif_mods_of_bin_motifs(os.path.join(GOLDEN, "bin-motifs.tsv"))) >= {"m1_a_1", "m3_a_1"}
    imputed = bn.impute_contig_methylation_within_bin(with_bin)
    assert set(imputed.columns) == {"contig", "bin", "motif_mod", "mean_bin_methylation", "methylation_value"}
    assert imputed["methylation_value"].notna().all()


def test_impute_contig_methylation_within_bin_values():
    """test_data_processing_functions.py::test_impute_contig_methylation_within_bin2."""
    cm = pd.DataFrame({"contig": ["contig_1", "contig_1", "contig_1", "contig_2", "contig_3"], "bin": ["bin1", "bin1", "bin1", "bin1", "bin2"],
                       "motif_mod": ["mod1", "mod2", "mod3", "mod3", "mod2"], "methylation_value": [0.5, 0.0, 0.9, 0.5, 0.9],
                       "n_motif_obs": [10, 5, 15, 20, 25]})
    out = bn.impute_contig_methylation_within_bin(cm)
    assert out["contig"].tolist() == ["contig_1", "contig_1", "contig_1", "contig_2", "contig_2", "contig_2", "contig_3"]
    assert out["bin"].tolist() == ["bin1"] * 6 + ["bin2"]
    assert out["motif_mod"].tolist() == ["mod1", "mod2", "mod3", "mod1", "mod2", "mod3", "mod2"]
    assert out["methylation_value"].tolist() == [0.5, 0.0, 0.9, 0.5, 0.0, 0.5, 0.9]      # contig_2: mod1, mod2 from the bin


def test_pseudo_methylation_draws_follow_the_global_generator():
    """data_processing.py:216-252: np.random.uniform(0, 0.15, n) of the global generator over the (contig, motif_mod) cross join
    sorted by (contig, motif_mod); observed values are kept."""
    cm = pd.DataFrame({"bin": ["unbinned", "binned", "unbinned", "binned", "unbinned"], "contig": ["contig_3", "contig_2", "contig_1", "contig_4", "contig_10"],
                       "motif_mod": ["mod1", "mod2", "mod1", "mod3", "mod3"], "methylation_value": [0.0, 0.3, 0.95, 0.5, 0.7]})
    np.random.seed(1)
    out = bn.impute_unbinned_contigs(cm)
    np.random.seed(1)
    draws = np.random.uniform(0, 0.15, 9)
    keys = [(c, m) for c in sorted(["contig_3", "contig_1", "contig_10"]) for m in ["mod1", "mod2", "mod3"]]
    assert list(zip(out["contig"], out["motif_mod"])) == keys
    observed = {("contig_3", "mod1"): 0.0, ("contig_1", "mod1"): 0.95, ("contig_10", "mod3"): 0.7}
    want = [observed.get(k, draws[i]) for i, k in enumerate(keys)]
    assert out["methylation_value"].tolist() == want
    assert set(out["bin"]) == {"unbinned"}


def test_create_matrix_orders():
    cm = pd.DataFrame({"contig": ["b", "b", "a"], "motif_mod": ["z_a_1", "c_m_0", "z_a_1"], "methylation_value": [0.1, 0.2, 0.3]})
    names, m = bn.create_matrix(cm)
    assert names == ["b", "a"] and m.tolist() == [[0.2, 0.1], [0.0, 0.3]]


def test_hdbscan_parameters_reproduce_the_hdbscan_package():
    """Two groups of three points, 10 apart.  The hdbscan package's min_samples=3 makes a point's core distance its 3rd nearest
    OTHER point, which lies in the other group; every mutual-reachability distance is then >= 9.8, the cheapest edge of the
    minimum spanning tree joins the two groups (9.8), and points only fall off the root one by one: the root is the one cluster,
    which allow_single_cluster=False forbids, so every point is noise.  scikit-learn counts the point itself: its min_samples=4
    is that clustering; its 3 would be the package's 2 and find the two groups."""
    from sklearn.cluster import HDBSCAN
    x = np.array([[0.0], [0.1], [0.2], [10.0], [10.1], [10.2]])
    assert bn.HDBSCAN_PARAMS == dict(min_samples=4, min_cluster_size=2, metric="euclidean", allow_single_cluster=False)
    assert HDBSCAN(**bn.HDBSCAN_PARAMS).fit_predict(x).tolist() == [-1] * 6
    assert HDBSCAN(**dict(bn.HDBSCAN_PARAMS, min_samples=3)).fit_predict(x).tolist() == [0, 0, 0, 1, 1, 1]


def test_contig_bin_files_and_fasta_output(tmp_path):
    bins = pd.DataFrame({"contig": ["c3", "c1", "c2", "c4"], "bin": ["b2", "b1", "b1", "b2"]})
    new = bn.create_contig_bin_file(bins, pd.DataFrame({"contig": ["c2"]}), include=pd.DataFrame({"contig": ["c9"], "bin": ["b1"]}))
    bn.generate_output(new, str(tmp_path), "new_contig_bin.tsv")
    assert (tmp_path / "new_contig_bin.tsv").read_text() == "contig\tbin\nc1\tb1\nc9\tb1\nc3\tb2\nc4\tb2\n"
    for name, cols in (("bin_contamination.tsv", bn.CONTAMINATION_COLUMNS), ("include_contigs.tsv", bn.INCLUDE_COLUMNS)):
        bn.generate_output(pd.DataFrame({c: [] for c in cols}), str(tmp_path), name)
        assert (tmp_path / name).read_text() == "\t".join(cols) + "\n"
    fa = tmp_path / "a.fasta"
    fa.write_text(">c1 some description\nACGTacgt\nNNNN\n>c9\n" + "A" * 130 + "\n>c3\n\n")
    asm = bn.read_fasta(str(fa))
    assert asm == {"c1": "ACGTacgtNNNN", "c9": "A" * 130, "c3": ""}
    assert bn.contig_lengths(asm)["length"].tolist() == [12, 130, 0]
    bn.write_bins_from_contigs(new, asm, str(tmp_path / "bins"))
    assert (tmp_path / "bins" / "b1.fa").read_text() == ">c1\nACGTacgtNNNN\n>c9\n" + "A" * 60 + "\n" + "A" * 60 + "\n" + "A" * 10 + "\n"
    assert (tmp_path / "bins" / "b2.fa").read_text() == ">c3\n"
    with pytest.raises(ValueError):
        bn.read_fasta(str(tmp_path / "new_contig_bin.tsv"))


def test_methylation_filter():
    t = pd.DataFrame({"n_motif_obs": [8, 3, 2], "mean_read_cov": [3.0, 8.0, 11.9]})
    assert bn.filter_methylation(t, 24)["n_motif_obs"].tolist() == [8, 3]


def _parse(argv):
    from nanomotif_amd.argparser import create_parser
    return create_parser().parse_args(argv)


FILES = ["--pileup", "p.bed", "--assembly", "a.fa", "--bin_motifs", "bm.tsv", "--contig_bins", "cb.tsv", "--out", "o"]


def test_argparse_binnary_subcommands():
    a = _parse(["detect_contamination"] + FILES + ["--contamination_file", "c.tsv"])
    assert (a.command, a.threads, a.min_valid_read_coverage, a.methylation_threshold, a.num_consensus, a.force, a.write_bins,
            a.methylation_output_type, a.contamination_file) == ("detect_contamination", 1, 3, 24, 4, False, False, "median", "c.tsv")
    a = _parse(["include_contigs"] + FILES + ["-t", "4", "--run_detect_contamination", "--mean_model_confidence", "0.9", "--force",
                                              "--write_bins", "--methylation_output_type", "weighted_mean", "--num_consensus", "3"])
    assert (a.threads, a.run_detect_contamination, a.mean_model_confidence, a.force, a.write_bins, a.methylation_output_type, a.num_consensus) == \
        (4, True, 0.9, True, True, "weighted_mean", 3)
    assert _parse(["include_contigs"] + FILES).mean_model_confidence == 0.8
    with pytest.raises(SystemExit):
        _parse(["include_contigs"] + FILES + ["--contamination_file", "c.tsv", "--run_detect_contamination"])
    with pytest.raises(SystemExit):
        _parse(["detect_contamination"] + FILES[:-2])                   # --out is required
    with pytest.raises(SystemExit):
        _parse(["detect_contamination"] + FILES + ["--methylation_output_type", "weighted-mean"])


def test_detect_contamination_help_exits_zero():
    env = dict(os.environ, PYTHONPATH=ROOT)
    for cmd in ("detect_contamination", "include_contigs"):
        r = subprocess.run([sys.executable, "-m", "nanomotif_amd", cmd, "-h"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--contig_bins" in r.stdout, r.stderr


def test_binnary_port_on_the_oracle_table_of_the_synthetic_layout():
    """The layout tests/test_gpu_binnary.py runs end to end, on the CPU oracle's read-methylation table: detection flags exactly
    the moved contig, inclusion (after detection) gives the unbinned contig to its own bin with high confidence."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import binnary_synth as bs
    mg = bs.make_metagenome()
    moved, unbinned, listed = bs.layout(mg)
    table = bn.filter_methylation(bs.oracle_table(mg), 24)
    bins = pd.DataFrame({"contig": list(listed), "bin": list(listed.values())})
    lengths = bn.contig_lengths({n: mg.contig_str(i) for i, n in enumerate(mg.names)})
    np.random.seed(1)
    cont = bn.detect_contamination(bn.add_bin(table, bins), lengths, 4, 1)
    assert set(cont["contig"]) == {moved} and len(cont) == 4
    inc = bn.include_contigs(bn.add_bin(table, bins[~bins["contig"].isin(cont["contig"])]), lengths, 0.8)
    mine = inc[inc["contig"] == unbinned]
    assert len(mine) == 3 and set(mine["assigned_bin"]) == {bs.BIN_A} and set(mine["confidence"]) == {"high_confidence"}
