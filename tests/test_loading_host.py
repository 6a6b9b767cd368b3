"""Host side of ``nanomotif_amd.loading`` (no GPU): ``PileupIngest`` down the host-parser path with an engine that only records what
``ingest_pileup`` is given — the contig look-up table, the labels, the second placement of a contig listed under two bins, and that a
second classification passes the same rows under other labels and thresholds; and the order in which ``main.find_motifs_bin`` makes
its device-touching calls through that path, with an engine that records them."""
import argparse

import numpy as np

from nanomotif_amd import fasta, loading
from nanomotif_amd import pileup as pp

NOT_HELD = 0xFFFFFFFF
COLUMNS = ("contig", "position", "mod_type", "strand", "fraction_mod", "nvalid_cov")


class RecordingEngine:
    """Stands in for ``ScanEngine``: keeps copies of the arguments of every ``ingest_pileup`` call (the columns are views into the
    reader's memory, gone with the table)."""

    def __init__(self):
        self.calls = []

    def ingest_pileup(self, contig, position, mod_type, strand, fraction_mod, nvalid_cov, labels, **kw):
        cols = dict(zip(COLUMNS, (contig, position, mod_type, strand, fraction_mod, nvalid_cov)))
        self.calls.append(dict(cols={k: np.array(v) for k, v in cols.items()}, identity={k: id(v) for k, v in cols.items()}, labels=dict(labels),
                               extra=[{k: np.array(v) for k, v in x.items()} for x in kw.pop("extra_parts")], **kw))
        return {"n_kept": len(contig), "kept": None}

    def ingest_device_pileup(self, *a, **kw):           # pragma: no cover - a host table must never come here
        raise AssertionError("a NativePileup went down the device path")


def _row(contig, pos, mod, strand, cov, percent):
    return f"{contig}\t{pos}\t{pos + 1}\t{mod}\t{cov}\t{strand}\t{pos}\t{pos + 1}\t255,0,0\t{cov}\t{percent:.2f}\t0\t{cov}\t0\t0\t0\t0\t0"


# a dozen rows: c2 first (the file's order is not the engine's), c3 is in no bin, c1 last
ROWS = [("c2", 3, "a", "+", 10, 90.0), ("c2", 4, "a", "-", 11, 5.0), ("c2", 9, "m", "+", 12, 80.0), ("c2", 12, "a", "+", 7, 50.0),
        ("c2", 20, "m", "-", 9, 0.0), ("c3", 1, "a", "+", 8, 100.0), ("c3", 2, "m", "-", 8, 25.0), ("c1", 0, "a", "+", 20, 75.0),
        ("c1", 5, "a", "-", 21, 10.0), ("c1", 6, "m", "+", 22, 95.0), ("c1", 7, "21839", "+", 23, 60.0), ("c1", 30, "a", "-", 24, 0.0)]


def _open(tmp_path):
    """The table of ROWS and the engine's contigs for a bin table that lists c2 under two bins."""
    bed = tmp_path / "p.bed"
    bed.write_text("\n".join(_row(*r) for r in ROWS) + "\n")
    (tmp_path / "cb.tsv").write_text("c1\tbin_a\nc2\tbin_a\nc2\tbin_b\n")
    bin_contig = fasta.generate_contig_bin(argparse.Namespace(contig_bin=str(tmp_path / "cb.tsv")))
    alias = "c2" + fasta.ALIAS_SEP + "bin_b"
    assert bin_contig == {"c1": "bin_a", "c2": "bin_a", alias: "bin_b"}
    assembly = {"c1": np.frombuffer(b"ACGT" * 10, dtype=np.uint8), "c2": np.frombuffer(b"GATC" * 10, dtype=np.uint8)}
    fasta.add_alias_sequences(assembly, bin_contig)
    names = [c for c in bin_contig if c in assembly]
    assert names == ["c1", "c2", alias]
    table = pp.NativePileup(str(bed))
    assert table.contig_names == ["c2", "c3", "c1"] and len(table) == len(ROWS)
    return table, names


def test_pileup_ingest_on_the_host_path(tmp_path, monkeypatch):
    monkeypatch.delenv("NANOMOTIF_INGEST_PART_ROWS", raising=False)
    table, names = _open(tmp_path)
    eng = RecordingEngine()
    ingest = loading.PileupIngest(eng, table, names)
    assert not ingest.on_device
    # the look-up table: the file's contig ids -> the engine's; a contig in no bin is not held
    assert ingest.lut.dtype == np.uint32 and ingest.lut.tolist() == [1, NOT_HELD, 0]
    res = ingest.classify(lambda mt: mt, 0.25, 0.75)
    assert res["n_kept"] == len(ROWS) and len(eng.calls) == 1
    first = eng.calls[0]
    assert first["labels"] == {0: ("m", "C"), 1: ("a", "A"), 2: ("21839", "C")}
    assert (first["low"], first["high"], first["want_rows"], first["max_part_rows"]) == (0.25, 0.75, False, 250_000_000)
    # every row of the file once, under the engine's contig ids and in the engine's types
    cols = first["cols"]
    assert cols["contig"].tolist() == [1] * 5 + [NOT_HELD] * 2 + [0] * 5
    assert cols["position"].tolist() == [r[1] for r in ROWS]
    assert cols["mod_type"].tolist() == [pp.MOD_TYPES.index(r[2]) for r in ROWS]
    assert cols["strand"].tolist() == [ord(r[3]) for r in ROWS]
    assert cols["nvalid_cov"].tolist() == [r[4] for r in ROWS]
    assert np.array_equal(cols["fraction_mod"], np.array([r[5] for r in ROWS]) / 100)
    assert [cols[k].dtype for k in COLUMNS] == [np.uint32, np.uint32, np.int8, np.uint8, np.float64, np.int32]
    # the contig listed under two bins: its rows once more, under the local id of its second placement
    assert len(first["extra"]) == 1
    extra = first["extra"][0]
    assert extra["contig"].dtype == np.uint32 and extra["contig"].tolist() == [2] * 5
    for k in COLUMNS[1:]:
        assert np.array_equal(extra[k], cols[k][:5]) and extra[k].dtype == cols[k].dtype, k

    # a second classification (the merge stage's, sample B's): the same rows, other labels and thresholds
    ingest.classify(lambda mt: (mt, "merge"), 0.3, 0.7)
    second = eng.calls[1]
    assert len(eng.calls) == 2 and second["identity"] == first["identity"]
    assert second["labels"] == {0: (("m", "merge"), "C"), 1: (("a", "merge"), "A"), 2: (("21839", "merge"), "C")}
    assert (second["low"], second["high"], second["want_rows"], second["max_part_rows"]) == (0.3, 0.7, False, 250_000_000)
    for k in COLUMNS:
        assert np.array_equal(second["cols"][k], cols[k]), k
        assert np.array_equal(second["extra"][0][k], extra[k]), k
    assert len(second["extra"]) == 1

    ingest.close()
    assert ingest.cols is None and ingest.extra == [] and not table._h


def test_pileup_ingest_takes_the_part_size_from_the_environment_and_needs_no_alias(tmp_path, monkeypatch):
    monkeypatch.setenv("NANOMOTIF_INGEST_PART_ROWS", "7")
    table, names = _open(tmp_path)
    eng = RecordingEngine()
    ingest = loading.PileupIngest(eng, table, names[:2])          # the engine of a run without the second placement
    assert ingest.lut.tolist() == [1, NOT_HELD, 0] and ingest.extra == []
    ingest.classify(lambda mt: mt + "@b", 0.3, 0.7)
    assert eng.calls[0]["max_part_rows"] == 7 and eng.calls[0]["extra"] == []
    assert eng.calls[0]["labels"] == {0: ("m@b", "C"), 1: ("a@b", "A"), 2: ("21839@b", "C")}
    ingest.close()


def test_parser_threads_and_wanted_contigs():
    assert [loading.parser_threads(argparse.Namespace(threads=t)) for t in (-3, 0, 1, 2, 16)] == [0, 0, 0, 2, 16]
    assert loading.parser_threads(argparse.Namespace()) == 0
    alias = "c2" + fasta.ALIAS_SEP + "bin_b"
    assert loading.wanted_contigs("p.bed", ["c1", "c2", alias]) is None
    assert loading.wanted_contigs("p.bed.gz", ["c1", "c2", alias, "c0"]) == ["c1", "c2", "c0"]


class CallOrderEngine(RecordingEngine):
    """Records the order of the device-touching calls ``main.find_motifs_bin`` makes (the ingest keeps nothing: the run ends there)."""

    def __init__(self, device, ctx=None):
        super().__init__()
        self.order, self.contig_names = ["context"], []

    def upload_assembly(self, names, seqs, bins, bin_names=None):
        self.order.append("upload")
        self.contig_names = list(names)

    def ingest_pileup(self, *a, **kw):
        super().ingest_pileup(*a, **kw)
        self.order.append(("classify", kw["low"], kw["high"], a[6][1][0]))
        return {"n_kept": 0, "kept": np.zeros((len(self.contig_names), 8), dtype=np.uint32)}

    def confident_rows(self):
        self.order.append("confident_rows")
        return tuple(np.zeros(0, dt) for dt in (np.uint32, np.uint32, np.uint8, np.int8))

    def alias_label(self, label, mod_type):
        self.order.append(("alias", label, mod_type))

    def close(self):
        self.order.append("close")


def test_motif_discovery_goes_through_the_shared_path_in_the_measured_order(tmp_path, monkeypatch):
    """The single-rank sequence of ``main.find_motifs_bin`` on the host readers: upload, first classification, window pipeline,
    ``confident_rows`` BEFORE the merge stage's classification (it speaks about the last ingest), and the engine closed on the early
    return; with the default thresholds the merge labels are aliases, with others a second classification at 0.3 / 0.7."""
    from nanomotif_amd import main as m
    from nanomotif_amd.argparser import create_parser
    engines = []
    monkeypatch.setattr(m, "ScanEngine", lambda device, ctx=None: engines.append(CallOrderEngine(device)) or engines[-1])
    monkeypatch.setattr(m._lib, "use_block_cache", lambda nbytes: None)
    monkeypatch.setattr(m, "device_window_pipeline", lambda eng, *a, **kw: eng.order.append("windows") or (None, None))
    for k, v in (("NANOMOTIF_HOST_FASTA", "1"), ("NANOMOTIF_HOST_PARSER", "1"), ("WORLD_SIZE", "1"), ("RANK", "0")):
        monkeypatch.setenv(k, v)
    bed = tmp_path / "p.bed"
    bed.write_text("\n".join(_row(*r) for r in ROWS) + "\n")
    (tmp_path / "cb.tsv").write_text("c1\tbin_a\nc2\tbin_a\nc2\tbin_b\n")
    (tmp_path / "a.fasta").write_text(">c1\n" + "ACGT" * 10 + "\n>c2\n" + "GATC" * 10 + "\n>c3\n" + "TTGCA" * 8 + "\n")
    for low, merge in ((0.3, [("alias", (mt, "merge"), mt) for mt in pp.MOD_TYPES]), (0.2, [("classify", 0.3, 0.7, ("a", "merge"))])):
        args = create_parser().parse_args(["motif_discovery", str(tmp_path / "a.fasta"), str(bed), "-c", str(tmp_path / "cb.tsv"), "--out",
                                           str(tmp_path / "out"), "--methylation_threshold_low", str(low)])
        assert m.find_motifs_bin(args) is None                      # "No pileup data after filtering"
        eng = engines.pop()
        assert eng.order == ["context", "upload", ("classify", low, 0.7, "a"), "windows", "confident_rows"] + merge + ["close"]
        assert eng.contig_names == ["c1", "c2", "c2" + fasta.ALIAS_SEP + "bin_b"]
        assert all(len(c["extra"]) == 1 and c["extra"][0]["contig"].tolist() == [2] * 5 for c in eng.calls)
        assert m.TIMINGS["pileup_parser"] == "host" and m.TIMINGS["pileup_rows"] == len(ROWS)
        assert {"assembly_s", "engine_start_s", "pileup_parse_s", "upload_filter_s"} <= set(m.TIMINGS)
        assert {"filters_" + k + "_s" for k in ("upload_assembly", "tables", "ingest", "window_pipeline", "table_close")} <= set(m.TIMINGS)
