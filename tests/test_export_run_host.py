"""Host side of what the twelve export commands share (no GPU, no library): the parser specs against a record of them
(``tests/data/export_cli_actions.json``, written by ``dump_actions`` below: run this module as a script to write it again), and
``nanomotif_amd/export_run.py`` — the known / skipped split, the closing of the engine, the order of the refusals at the opening, the
text helpers — and ``engine._table_groups`` with a stand-in for the library call."""
import argparse
import importlib
import json
import os
import types

import numpy as np
import pytest

from nanomotif_amd import engine, export_run, loading
from nanomotif_amd.argparser import create_parser
from nanomotif_amd.motif_sites import SiteCandidate

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "export_cli_actions.json")
EXPORTS = ("motif_sites", "motif_coverage", "motif_compare", "motif_strands", "motif_profile", "motif_tracks", "motif_fractions", "motif_pileup",
           "motif_context", "motif_gc", "motif_overlap", "motif_kmers")
RECORDED = EXPORTS + ("motif_discovery", "detect_contamination", "include_contigs")


# ------------------------------------------------------------------------------------------------ 1. the parser specs
def dump_actions(names=RECORDED) -> dict:
    """Per subparser: its actions in order (group title, option strings, dest, default, nargs, required, the action's class name, help, with
    SUPPRESS as argparse spells it), the positionals in order, and the mutually exclusive groups (required, members).  Through json, so
    that a tuple default compares as the list the fixture holds."""
    choices = create_parser()._subparsers._group_actions[0].choices
    out = {}
    for name in names:
        p = choices[name]
        title = {id(a): g.title for g in p._action_groups for a in g._group_actions}
        out[name] = {
            "actions": [[title.get(id(a)), list(a.option_strings), a.dest, a.default, a.nargs, a.required, type(a).__name__, a.help] for a in p._actions],
            "positionals": [a.dest for a in p._actions if not a.option_strings],
            "exclusive": [[g.required, [a.dest for a in g._group_actions]] for g in p._mutually_exclusive_groups]}
    return json.loads(json.dumps(out))


@pytest.mark.parametrize("name", RECORDED)
def test_the_parser_specs_are_the_recorded_ones(name):
    with open(FIXTURE) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(RECORDED)
    got = dump_actions([name])[name]
    assert got["positionals"] == recorded[name]["positionals"] and got["exclusive"] == recorded[name]["exclusive"]
    assert got["actions"] == recorded[name]["actions"]
    if name in EXPORTS:
        assert got["exclusive"] == [[True, ["contig_bin", "files", "directory"]]]


# ------------------------------------------------------------------------------------------------ 2. the split
def stub_engine(**more):
    """What the scaffold reads of an engine: bins b0 (two contigs) and b1 (none), mod type a."""
    eng = types.SimpleNamespace(bin_index={"b0": 0, "b1": 1}, slot_of_mod={"a": 0, "m": 1}, closed=0, **more)
    eng.bin_contigs = lambda b: ["c1", "c2"] if b in ("b0", 0) else []

    def close():
        eng.closed += 1
    eng.close = close
    return eng


CANDS = [SiteCandidate("b0", "GATC", "a", 1), SiteCandidate("gone", "GATC", "a", 1), SiteCandidate("b0", "CCWGG", "21839", 1),
         SiteCandidate("b1", "CCWGG", "m", 1), SiteCandidate("nowhere", "AC", "21839", 0)]
NO_BIN = "{!r}: the bin has no contig in the assembly; skipped"
NO_ROWS = "{!r}: the pileup holds no rows of mod type {}; skipped"
NO_KEPT_ROWS = "{!r}: the pileup holds no rows of mod type {} that pass the read filters; skipped"


@pytest.mark.parametrize("mod_types, suffix, wording, known, second", [
    (lambda eng: eng.slot_of_mod, "", None, [0, 3], NO_ROWS),                                                  # plain
    (lambda eng: ["a"], "", None, [0], NO_ROWS),                                                               # kept mod types
    (lambda eng: export_run.readstats_mod_types(eng), export_run.READ_FILTER_SUFFIX, None, [0], NO_KEPT_ROWS),   # read statistics
    (lambda eng: ["a"], "", "neither pileup holds rows", [0], "{!r}: neither pileup holds rows of mod type {}; skipped")])
def test_the_split_keeps_file_order_and_warns_once_per_skipped_candidate(mod_types, suffix, wording, known, second, caplog):
    eng = stub_engine(readstats_kept={"a": 7, "m": 0})
    kw = {} if wording is None else {"wording": wording}
    with caplog.at_level("WARNING"):
        got = export_run.split_known(CANDS, eng, mod_types(eng), suffix=suffix, **kw)
    assert got == [CANDS[k] for k in known]
    expect = [NO_BIN.format(c) if c.bin not in eng.bin_index else second.format(c, c.mod_type) for k, c in enumerate(CANDS) if k not in known]
    assert [r.getMessage() for r in caplog.records] == expect and len(expect) == len(CANDS) - len(known)
    assert all(r.levelname == "WARNING" for r in caplog.records)


def test_background_keys_and_candidates():
    eng = stub_engine()
    eng.bin_index = {"z": 2, "b1": 1, "b0": 0}
    eng.bin_contigs = lambda b: [] if b == "b1" else ["c"]
    assert export_run.bin_mod_keys(eng, ["m", "a"]) == [("b0", "m"), ("b0", "a"), ("z", "m"), ("z", "a")]
    assert export_run.background_keys(CANDS) == [("b0", "a"), ("gone", "a"), ("b0", "21839"), ("b1", "m"), ("nowhere", "21839")]
    (m, mt, b), (m2, mt2, b2) = export_run.background_candidates([("b0", "a"), ("z", "m")])
    assert (m.string, m.mod_position, mt, b) == ("A", 0, "a", "b0") and (m2.string, m2.mod_position, mt2, b2) == ("C", 0, "m", "z")
    from nanomotif_amd import motif_fractions, motif_tracks
    assert motif_tracks.background_keys is export_run.background_keys is motif_fractions.background_keys


# ------------------------------------------------------------------------------------------------ 3. closing
def test_the_engine_is_closed_once_when_the_body_returns_and_when_it_raises():
    eng = stub_engine()
    with export_run.closing(eng) as e:
        assert e is eng and eng.closed == 0
    assert eng.closed == 1
    eng = stub_engine()
    with pytest.raises(KeyError):
        with export_run.closing(eng):
            raise KeyError("x")
    assert eng.closed == 1


def test_motif_profile_without_a_target_closes_the_engine_once(tmp_path, monkeypatch, caplog):
    from nanomotif_amd import motif_profile
    eng = stub_engine(pileup_ingests=[{"kept": np.zeros((2, 8), dtype=np.uint32)}])
    monkeypatch.setattr(motif_profile, "open_run", lambda command, args, timings: (eng, [], 0))
    args = create_parser().parse_args(["motif_profile", "a.fasta", "p.bed", "-c", "cb.tsv", "--bin_motifs", "m.tsv", "--out", str(tmp_path / "out")])
    with caplog.at_level("ERROR"):
        assert motif_profile.run(args) == 2
    assert "motif_profile: the pileup holds no rows of any target mod type" in caplog.text
    assert eng.closed == 1 and not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------ 4. openings
BAD_EDGES = ["--methylation_threshold_low", "0.01"]


def command_args(command, tmp_path, bin_motifs=True, more=()):
    (tmp_path / "cb.tsv").write_text("c1\tbin_a\nc2\tbin_a\n")
    (tmp_path / "m.tsv").write_text("reference\tmotif\tmod_position\tmod_type\nbin_a\tGATC\t1\ta\n")
    pileups = [str(tmp_path / "p.bed")] * (2 if command == "motif_compare" else 1)
    argv = [command, str(tmp_path / "a.fasta"), *pileups, "-c", str(tmp_path / "cb.tsv"), "--out", str(tmp_path / "out"), *more]
    return create_parser().parse_args(argv + (["--bin_motifs", str(tmp_path / "m.tsv")] if bin_motifs else []))


@pytest.fixture
def loader_reached(monkeypatch):
    """``loading.ScanEngine`` raises ``Reached``: the opening got as far as making an engine."""
    class Reached(Exception):
        pass

    def no_engine(*a, **kw):
        raise Reached("an engine was asked for")
    monkeypatch.setattr(loading, "ScanEngine", no_engine)
    return Reached


@pytest.mark.parametrize("command", EXPORTS)
def test_the_openings_refuse_in_the_same_order(command, tmp_path, monkeypatch, caplog, loader_reached):
    run = importlib.import_module("nanomotif_amd." + command).run
    args = command_args(command, tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    (tmp_path / "m.tsv").write_text("not\ta\tbin-motifs\tfile\n")                # a multi-rank launch: status 2 before anything is read
    with caplog.at_level("ERROR"):
        assert run(args) == 2
    assert f"{command} runs on one GPU: start it without a multi-rank launcher (WORLD_SIZE is 2)" in caplog.text
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(ValueError, match=r"not a bin-motifs.tsv \(columns \['mod_position', 'mod_type', 'motif', 'reference'\] are required\)"):
        run(args)                                                                # --bin_motifs is read before anything is loaded
    with pytest.raises(loader_reached):
        run(command_args(command, tmp_path))                                     # (m.tsv is written anew) and then the loader
    assert not (tmp_path / "out").exists()


def test_motif_kmers_without_bin_motifs_reaches_the_loader_on_a_multi_rank_launch(tmp_path, monkeypatch, loader_reached):
    """The record of a known quirk: without --bin_motifs nothing refuses the multi-rank launch."""
    from nanomotif_amd import motif_kmers
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(loader_reached):
        motif_kmers.run(command_args("motif_kmers", tmp_path, bin_motifs=False))
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(loader_reached):
        motif_kmers.run(command_args("motif_kmers", tmp_path, bin_motifs=False))


def test_the_bad_edges_of_motif_fractions_come_before_the_multi_rank_refusal(tmp_path, monkeypatch, caplog, loader_reached):
    from nanomotif_amd import motif_fractions
    monkeypatch.setenv("WORLD_SIZE", "2")
    with caplog.at_level("ERROR"):
        assert motif_fractions.run(command_args("motif_fractions", tmp_path, more=BAD_EDGES)) == 2
    assert "bin edges 0 / 14 of 20" in caplog.text and "runs on one GPU" not in caplog.text


@pytest.mark.parametrize("command", ["motif_fractions", "motif_pileup"])
def test_the_read_statistics_opening_names_the_command_for_a_contig_under_two_bins(command, tmp_path, monkeypatch, caplog, loader_reached):
    run = importlib.import_module("nanomotif_amd." + command).run
    monkeypatch.setenv("WORLD_SIZE", "1")
    args = command_args(command, tmp_path)
    (tmp_path / "cb.tsv").write_text("c1\tbin_a\nc2\tbin_a\nc2\tbin_b\n")
    with caplog.at_level("ERROR"):
        assert run(args) == 2
    assert f"{command}: 1 contig(s) are listed under several bins (e.g. c2)" in caplog.text


def test_a_failing_library_is_reported_as_a_missing_gpu(tmp_path, monkeypatch):
    from nanomotif_amd import _lib, motif_sites

    def no_device(*a, **kw):
        raise _lib.NmScanError(-1, "no device")
    monkeypatch.setattr(loading, "ScanEngine", no_device)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for command in ("motif_sites", "motif_pileup", "motif_kmers"):
        run = importlib.import_module("nanomotif_amd." + command).run
        with pytest.raises(RuntimeError, match=r"nanomotif_amd needs an AMD GPU \(MI355X\); there is no CPU fallback \(.*no device"):
            run(command_args(command, tmp_path))
    assert motif_sites.open_run is export_run.open_run and motif_sites.open_candidates is export_run.open_candidates


# ------------------------------------------------------------------------------------------------ 5. helpers
def test_parse_int_in_is_the_five_range_parsers():
    from nanomotif_amd import motif_fractions, motif_gc, motif_profile, motif_tracks
    cases = [(motif_profile.parse_radius, ("0", " 31 ", 10), ("-1", "32", "x", "1.5"), "--radius takes an integer in 0..31; got {!r}"),
             (motif_gc.parse_half, ("0", "31", 7), ("-1", "32", "x"), "--half takes an integer in 0..31; got {!r}"),
             (motif_gc.parse_gc_bins, ("1", "8", 1000), ("0", "-3", "x"), "--gc_bins takes an integer of at least 1; got {!r}"),
             (motif_fractions.parse_bins, ("2", "64", 20), ("1", "65", "x", 0), "--bins takes a number in [2, 64]; got {!r}"),
             (motif_tracks.parse_window, ("128", "4096", 1 << 30), ("0", "64", "129", str((1 << 30) + 128), "x"),
              "--window takes a multiple of 128 in [128, 2^30]; got {!r}")]
    for parse, good, bad, text in cases:
        for value in good:
            assert parse(value) == int(str(value).strip())
        for value in bad:
            with pytest.raises(ValueError) as e:
                parse(value)
            assert str(e.value) == text.format(value)
    assert export_run.parse_int_in("--x", "5", 1, 9) == 5 and export_run.parse_int_in("--x", "6", 2, step=2) == 6
    with pytest.raises(ValueError, match=r"^--x takes an integer in 1\.\.9; got '10'$"):
        export_run.parse_int_in("--x", "10", 1, 9)


def test_the_text_helpers():
    assert export_run.table_text(["a", "b"], [[1, "x"], [2.5, ""]]) == "a\tb\n1\tx\n2.5\t\n" and export_run.table_text(["a"], []) == "a\n"
    assert export_run.frac_text(1, 2) == "0.333333" and export_run.frac_text(0, 0) == "" and export_run.frac_text(np.int64(3), np.int64(0)) == "1.000000"
    assert export_run.share_text(1, 3) == "0.333333" and export_run.share_text(5, 0) == "" and export_run.share_text(np.int64(2), np.uint64(4)) == "0.500000"
    from nanomotif_amd import motif_context, motif_gc, motif_profile, motif_sites
    assert motif_sites.table_text is export_run.table_text and motif_profile.frac_text is export_run.frac_text
    assert motif_context.share_text is export_run.share_text and motif_gc.frac_text is export_run.frac_text


def test_write_texts_skips_none(tmp_path):
    out = tmp_path / "deep" / "out"
    os.makedirs(out)
    export_run.write_texts(str(out), ("a.tsv", "b.tsv", "c.tsv", "never.tsv"), ("x\n", None, "z\n"))
    assert sorted(os.listdir(out)) == ["a.tsv", "c.tsv"] and (out / "c.tsv").read_text() == "z\n"


def test_finish_writes_its_keys_and_the_log_line(caplog):
    timings = {"ingest_s": 1.234}
    with caplog.at_level("INFO"):
        export_run.finish("motif_x", timings, 0.5, 0.25, candidates=3, radius=7)
        export_run.finish("motif_y", dict(timings), 0.5, 0.25, label="segmentation and text")
    assert timings == {"ingest_s": 1.234, "kernels_s": 0.5, "text_s": 0.25, "candidates": 3, "radius": 7}
    assert [r.getMessage() for r in caplog.records] == ["motif_x: ingest 1.23s, engine 0.50s, text 0.25s",
                                                        "motif_y: ingest 1.23s, engine 0.50s, segmentation and text 0.25s"]


# ------------------------------------------------------------------------------------------------ 6. the table groups
def batch_of(bins):
    n = len(bins)
    return engine.CandidateBatch(np.asarray(bins, dtype=np.uint32), np.zeros(n, np.uint8), np.ones(n, np.uint8), np.zeros(n, np.uint8),
                                 np.arange(n, dtype=np.uint32), np.zeros(n, np.uint8))


@pytest.mark.parametrize("bins", [[0], [1], [0, 1], [1, 1], [0, 1, 1, 0, 0], [1, 0, 0, 1, 0]])
def test_table_groups_yield_the_same_under_every_limit(bins):
    names = {0: ["c1", "c2", "c3"], 1: []}                                  # bin 1 holds no contig: its candidates have no row
    b = batch_of(bins)
    n_rows = [len(names[x]) for x in bins]
    row_bytes = 2 * 4 * 8
    one = max(n_rows) * row_bytes

    def collect(limit):
        groups, tables = [], []

        def call(k, e, sub, rows, table):
            assert e > k and len(sub) == e - k and list(sub.bins) == bins[k:e]
            assert rows.dtype == np.uint64 and rows.tolist() == np.concatenate([[0], np.cumsum(n_rows[k:e])]).tolist()
            assert table.shape == (max(int(rows[-1]), 1), 2, 4) and table.dtype == np.int64 and not table.any()
            for j in range(k, e):
                table[int(rows[j - k]):int(rows[j - k + 1])] = j + 1
            groups.append((k, e))
            tables.append(table)
        got = list(engine._table_groups(b, names, n_rows, row_bytes, limit, (2, 4), np.int64, call))
        assert [g[0] for g in groups] == [0] + [g[1] for g in groups[:-1]] and groups[-1][1] == len(bins)      # consecutive, none empty
        return got, groups

    results = {limit: collect(limit) for limit in (1, one, one + 1, max(sum(n_rows) * row_bytes, 1))}
    first = results[1][0]
    assert [j for j, _, _ in first] == list(range(len(bins)))
    for j, nm, t in first:
        assert nm == names[bins[j]] and t.shape == (n_rows[j], 2, 4) and (t == j + 1).all()
    for got, _ in results.values():
        assert [(j, nm) for j, nm, _ in got] == [(j, nm) for j, nm, _ in first]
        assert all(np.array_equal(t, u) for (_, _, t), (_, _, u) in zip(got, first))
    # below one candidate's cost a group still holds a candidate: never two that have rows (those without cost nothing and may share one)
    assert all(sum(1 for j in range(k, e) if n_rows[j]) <= 1 for k, e in results[1][1]) and len(results[1][1]) >= sum(1 for n in n_rows if n)
    assert len(results[max(sum(n_rows) * row_bytes, 1)][1]) == 1


def test_the_byte_limit():
    assert engine._byte_limit(None, 77) == 77 and engine._byte_limit("5", 77) == 5
    with pytest.raises(ValueError, match="max_bytes must be at least 1"):
        engine._byte_limit(0, 77)


if __name__ == "__main__":
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        json.dump(dump_actions(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
