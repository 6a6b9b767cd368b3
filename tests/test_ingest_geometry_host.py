"""The geometry input of tests/ingest_geometry.py holds, by count, every border it claims to hold, for each of the three grids the GPU test
runs it on (NM_INGEST_WALK_BLOCKS unset, 1, 3), and the oracle's result on it is not degenerate.  No GPU: tests/test_gpu_ingest_geometry.py
compares the device with the oracle on this input; this file proves that the comparison meets the code it is meant to meet."""
import numpy as np
import pytest

import ingest_geometry as ig


@pytest.fixture(scope="module")
def counts():
    g = ig.build_input()
    return {k: ig.census(g, g.table, k) for k in ig.GRIDS}


def test_wave_split_restated():
    """the figures of the rows-per-wave fact: every call of at most 2 097 152 rows walks 64 rows a wave unless the switch lowers the blocks"""
    assert [ig.wave_split(n)[1] for n in (40_000, 600_000, 2_097_152, 2_097_153, 10**9)] == [64, 64, 64, 128, 30_528]
    assert ig.wave_split(40_000, 1) == (4, 10_048) and ig.wave_split(40_000, 3) == (12, 3_392)
    assert ig.wave_split(ig.N_ROWS) == (940, 64) and ig.wave_split(ig.N_ROWS, 1) == (4, 15_040) and ig.wave_split(ig.N_ROWS, 3) == (12, 5_056)
    assert ig.wave_split(65, 1) == (4, 64) and ig.wave_split(1) == (4, 64) and ig.wave_split(257) == (8, 64)
    assert ig.wave_split(100, 7) == (4, 64)                              # the switch never raises the number of blocks
    for n, k in ((ig.N_ROWS, None), (ig.N_ROWS, 3), (257, None), (65, 1)):
        r = ig.wave_ranges(n, k)
        assert r[0][0] == 0 and r[-1][1] == n and all(a[1] == b[0] for a, b in zip(r, r[1:]))


def test_table_is_in_modkit_order_and_unique():
    g = ig.build_input()
    t = g.table
    assert 40_000 <= len(t["position"]) == ig.N_ROWS <= 60_000
    change = np.flatnonzero(t["contig"][1:] != t["contig"][:-1]) + 1
    assert len(set(t["contig"][np.concatenate([[0], change])].tolist())) == len(change) + 1          # every contig in one run
    assert ((np.diff(t["position"]) >= 0) | (t["contig"][1:] != t["contig"][:-1])).all()
    scored = np.isin(t["mod_type"], list(ig.SCORED))
    keys = set(zip(t["contig"][scored].tolist(), t["position"][scored].tolist(), t["strand"][scored].tolist(), t["mod_type"][scored].tolist()))
    assert len(keys) == int(scored.sum())                                # no duplicate row of a scored code
    assert set(t["mod_type"].tolist()) == {0, 1, 2, 3, 4, 9}
    assert (t["position"] < g.length[t["contig"]]).all() and (~g.resident).sum() == 2
    # the letter under (nearly) every row of a scored code is the one its strand implies: the compact planes hold the row
    seq_of = {int(c): g.seqs[int(g.lut[c])] for c in np.flatnonzero(g.resident)}
    right = wrong = 0
    for c, p, s, m in zip(t["contig"].tolist(), t["position"].tolist(), t["strand"].tolist(), t["mod_type"].tolist()):
        if m in ig.SCORED and c in seq_of:
            base = ig.SCORED[m][1]
            ok = seq_of[c][p] == (base if s == ig.PLUS else ig.COMPLEMENT[base])
            right += ok
            wrong += not ok
    assert wrong == 600 and right > 50_000                               # the stretch with both strands on every position: one letter suits one row
    # prefixes of 1 .. 257 rows: nothing survives the frequency filter
    for n in ig.PREFIXES:
        assert not ig.Fates({k: v[:n] for k, v in t.items()}).freq.any()


@pytest.mark.parametrize("k", ig.GRIDS, ids=["unset", "k1", "k3"])
def test_feature_a_piece_turn_and_wave_borders(counts, k):
    c = counts[k]
    assert c["border_at_offset_0"] >= 1 and c["border_mid_piece"] >= 2
    if k:                                                                # with 64 rows a wave there is no second piece
        assert c["border_at_offset_64"] >= 1 and c["border_at_offset_128"] >= 1 and c["border_at_offset_256"] >= 1
    assert c["failing_contig_inside_piece"] >= 1 and c["code8_piece_between"] >= 1 and c["absent_between_resident"] >= 1
    assert c["window_contig_change"] >= 1                                # a contig ends inside a wave's range, with bits in the window


@pytest.mark.parametrize("k", ig.GRIDS, ids=["unset", "k1", "k3"])
def test_feature_b_key_cache_and_strict_bounds(counts, k):
    c = counts[k]
    assert c["max_keys_in_a_wave"] >= 6                                  # more keys than the cache has entries
    if k:
        assert c["max_key_returns_in_a_wave"] >= 10                      # evicted and back, in one wave (a wave of one piece meets a key once)
    assert c["group_of_50_spread"] >= 1 and c["group_of_51_spread"] >= 1
    assert c["group_of_50_dropped"] >= 1 and c["group_of_51_kept"] >= 1 and not c["group_of_50_kept"] and not c["group_of_51_dropped"]
    assert c["exactly_0.7_in_bound_group"] >= 4 and c["coverage_5_in_bound_group"] >= 4 and c["coverage_6_in_bound_group"] >= 2


@pytest.mark.parametrize("k", ig.GRIDS, ids=["unset", "k1", "k3"])
def test_feature_c_window_of_the_store_path(counts, k):
    c = counts[k]
    for d in (15, 16, 17, 31):
        assert c["window_mine_%d" % d] >= 1, d                           # inside one piece
    for d in (32, 33):
        assert c["window_leader_later_%d" % d] >= 1, d                   # inside one piece: beyond the window, it slides in mid-piece
    if k:
        for d in (15, 16, 17, 31, 32, 33):
            assert c["window_leader_first_%d" % d] >= 1, d               # across pieces
        assert c["window_max_pieces"] >= 8                               # many pieces per window
    assert c["max_gap_bp"] >= 3000
    assert c["nomod_on_position_0"] >= 1 and c["nomod_on_last_position"] >= 1
    assert c["nomod_on_bits_31_32"] >= 1 and c["nomod_on_bits_8191_8192"] >= 1
    assert c["border_in_word_4_planes"] >= 1 and c["border_in_word_1_plane_of_2"] >= 1
    assert c["m_and_21839_on_one_cytosine"] >= 100


@pytest.mark.parametrize("k", ig.GRIDS, ids=["unset", "k1", "k3"])
def test_feature_d_candidates(counts, k):
    c = counts[k]
    assert c["candidate_run_of_64"] >= 1 and c["candidate_run_of_65"] >= 1
    if k == 1:
        assert c["max_candidate_run_in_a_wave"] >= 700 + 63 and c["turns_with_63_waiting"] >= 2
    if k:
        assert c["max_queue"] == 63 + 256                                # one short of the queue's capacity
        assert c["max_candidates_in_a_wave"] > 64                        # a list block and a pack of more than 64 entries
    else:
        assert c["max_queue"] == 64
    assert c["empty_wave_between_busy_waves"] >= 1
    for kind in ("same_8", "same_9", "other_strand_within_8"):
        assert c["pair_across_wave_" + kind] >= 1, kind
    for kind in ("same_8", "same_9", "other_strand_within_8", "other_code_8", "other_code_9", "tied_8"):
        assert c["pair_across_piece_" + kind] >= 1, kind
    assert c["candidates_below_8"] >= 2 and c["candidates_above_L_minus_9"] >= 2 and c["last_position_next_to_position_0"] >= 1
    assert c["null_next_to_kept_candidate"] >= 1 and c["stronger_coverage_5_next_to_kept_candidate"] >= 1


def test_oracle_result_is_not_degenerate(counts):
    c = counts[None]
    assert c["dropped_by_coverage"] >= 4 and c["dropped_by_frequency"] >= 100 and c["dropped_by_adjacency"] >= 20
    for code in ig.SCORED:
        for strand in ("plus", "minus"):
            for state in ("mod", "nomod", "nocall"):
                assert c["%s_%d_%s" % (state, code, strand)] >= 3, (state, code, strand)
    g = ig.build_input()
    e = ig.expected_of()
    assert 0 < e.n_kept < ig.N_ROWS and e.kept.sum() < e.n_kept          # a code >= 8 survives too: filtered with the rest, never reported
    assert e.n_candidates > 15_000 and len(e.confident) > 15_000
    assert all({s & 3 for _, _, s in rec} == {0, 1, 2} and {s >> 2 for _, _, s in rec} == {0, 1} for rec in e.sites.values())


def test_variants_are_one_edit_each_and_break_the_order():
    g = ig.build_input()
    base = g.table
    starts = {k: {a for a, _ in ig.wave_ranges(ig.N_ROWS, k)} for k in ig.GRIDS}
    for k in (1, 3):                                                     # a wave's first row, offsets 64 and 256, mid-piece
        assert {o for i in g.variant_rows for o in ig.VARIANT_OFFSETS if i - o in starts[k]} == set(ig.VARIANT_OFFSETS)
    assert sum(1 for i in g.variant_rows if i in starts[None]) >= 2 and sum(1 for i in g.variant_rows if i % 64) >= 2      # 64 rows a wave: first row, mid-piece
    names = ig.variant_names()
    assert len(names) == len(set(names)) == 14
    for name in names:
        t = ig.variant(name)
        i = int(name.split("@")[1])
        same_contig = t["contig"][1:] == t["contig"][:-1]
        down = np.flatnonzero(same_contig & (np.diff(t["position"]) < 0)) + 1
        first = np.concatenate([[0], np.flatnonzero(~same_contig) + 1])
        runs_of_k = int((t["contig"][first] == g.marks["K"]).sum())
        if name.startswith("down"):
            assert down.tolist() == [i] and runs_of_k == 1
            assert sum(int((t[c] != base[c]).sum()) for c in base if c != "fraction_mod") == 1
            # the displaced row is unmethylated, lands at least 40 plane words below the row before it, in a word that holds earlier bits
            assert t["fraction_mod"][i] <= ig.LOW and t["mod_type"][i] in ig.SCORED
            assert (t["position"][i - 1] >> 5) - (t["position"][i] >> 5) >= 40
            word = (base["contig"] == g.marks["K"]) & (base["position"] >> 5 == t["position"][i] >> 5) & (base["fraction_mod"] <= ig.LOW)
            assert word[:i].sum() >= 4
        else:
            assert len(down) == 0 and runs_of_k == 2 and i in first.tolist()
            assert sorted(zip(*[t[c].tolist() for c in ("contig", "position", "strand", "mod_type")])) == \
                sorted(zip(*[base[c].tolist() for c in ("contig", "position", "strand", "mod_type")]))
        # the edit changes what survives nowhere: the filters do not look at the order of the rows
        if name == names[-1]:
            assert ig.expected_of(name).confident == ig.expected_of().confident
    assert g.marks["contig_65"] and all(int((base["contig"] == c).sum()) == 65 and
                                        int(((base["contig"] == c) & (base["fraction_mod"] == 0.9)).sum()) == 60 for c in g.marks["contig_65"])
