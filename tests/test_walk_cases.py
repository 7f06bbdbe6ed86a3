"""The merge file walk's small cases (tests/walk_cases.py) on the CPU: the
census must reproduce the oracle's files in every case, keep its truncated
floating-point quantities away from integer boundaries, and show that the
case list reaches every path of merge_scan_apply, merge_walk_abs_kernel,
merge_walk_kernel and merge_emit_kernel that it claims to reach -- by name
and count, so that a later edit of a case cannot silently lose a path."""
import functools
import re

import numpy as np
import pytest

import pyoracle as ora
import walk_cases as wc

NAMES = [c.name for c in wc.CASES]


@functools.lru_cache(maxsize=None)
def census(name):
    return wc.census(wc.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def expected(name):
    return wc.expected(wc.BY_NAME[name], ora.TIE_INPUT)


@pytest.mark.parametrize("name", NAMES)
def test_census_matches_oracle(name):
    case, r = wc.BY_NAME[name], census(name)
    want, wstarts = expected(name)
    assert np.array_equal(r.starts, wstarts), (r.starts[:8], wstarts[:8])
    assert np.array_equal(r.out, want)
    assert r.nout == want.size and r.nfiles == wstarts.size - 1
    assert r.most == wc.most_pairs(wstarts)
    assert not r.out_past_nout
    assert len(r.paths) == r.nfiles and "?" not in r.paths
    assert r.margin >= wc.MARGIN, r.margin
    assert case.n <= wc.MAX_PAIRS
    assert case.nbytes() <= (1 << 20) or name == "extra_2p24"


def test_both_tie_orders_have_an_expected_output():
    """TIE_GOHEAP's expected files come from the oracle alone; in the cases
    with long duplicate groups the heap's order must differ from the input
    order somewhere, or the second tie mode would test nothing new."""
    differ = 0
    for name in ("ext_t253", "gen_w_chunk0_long_group", "emit_T1", "size_n1025"):
        a, _ = expected(name)
        b, _ = wc.expected(wc.BY_NAME[name], ora.TIE_GOHEAP)
        differ += not np.array_equal(a, b)
    assert differ >= 2


# (case, "codes" | "counts" | "paths", key, count): exact counts; for "paths"
# the key is a regular expression and the count the files it matches
COVERAGE = [
    # cand_ext's delta codes, each at a plateau a file really starts after
    ("ext_t0_level1", "codes", "ext:1", 1),
    ("ext_t1", "codes", "ext:2", 1),
    ("ext_t253", "codes", "ext:254", 1),
    ("ext_t253", "paths", r"general", 0),
    ("ext_t254", "codes", "ext:255", 1),
    ("ext_t254", "paths", r"general\(unresolved\)", 1),
    ("ext_t254", "counts", "general_group_len_255", 1),
    ("ext_none_inside", "codes", "ext:0", 1),
    ("ext_none_at_end", "codes", "ext:0", 1),
    ("ext_none_at_end", "counts", "abs_last_nothing", 1),
    ("ext_tile_last", "counts", "ext_tile_last", 1),
    ("ext_tile_last", "codes", "ext:4", 1),
    ("ext_odd_position", "counts", "ext_other_thread", 1),
    ("ext_t1", "counts", "ext_other_thread", 0),
    # the extra against the threshold
    ("extra_size_T-1", "codes", "extra:T-1", 1),
    ("extra_size_T-1", "paths", r"general", 0),
    ("extra_size_T", "codes", "extra:T", 1),
    ("extra_size_T", "paths", r"general\(extra>=T\)", 1),
    ("extra_size_T+1", "codes", "extra:T+1", 1),
    ("extra_size_T+1", "paths", r"general\(extra>=T\)", 1),
    ("dups_each_fill_a_file", "paths", r"general\(extra>=T\)", 1),
    ("dups_each_fill_a_file", "paths", r"general\(not a plateau start\)", 3),
    ("dups_each_fill_a_file", "counts", "general_extra_fills", 3),
    ("extra_2p24", "codes", "ext:255:2^24", 1),
    ("extra_2p24", "paths", r"general\(unresolved\)", 1),
    # phase 1
    ("abs_one_file", "codes", "head:kAbsLast", 1),
    ("abs_one_file", "counts", "abs_nres", 0),
    ("abs_nres1", "counts", "abs_nres", 1),
    ("abs_nres2", "counts", "abs_nres", 2),
    ("abs_nres63", "counts", "abs_nres", 63),
    ("abs_nres63", "counts", "abs_waves", 1),
    ("abs_nres64", "counts", "abs_nres", 64),
    ("abs_nres64", "counts", "abs_waves", 2),
    ("abs_nres65", "counts", "abs_nres", 65),
    ("abs_nres65", "counts", "abs_most_past_wave0", 1),
    ("abs_nres131", "counts", "abs_nres", 131),
    ("abs_nres131", "counts", "abs_waves", 3),
    ("abs_nres131", "counts", "abs_most_past_wave0", 1),
    ("abs_nres131", "codes", "abs:kAbsLast", 1),
    ("abs_nres131", "paths", r"abs", 132),
    ("abs_stop", "codes", "abs:kAbsStop", 1),
    ("abs_tail_of_dropped", "codes", "abs:kAbsLast", 1),
    ("abs_tail_of_dropped", "counts", "abs_last_nothing", 1),
    ("abs_window_limit", "counts", "abs_window_limit", 1),
    ("abs_window_limit", "paths", r"abs", 352),
    ("abs_window_limit", "paths", r"round\(32\)", 49),
    ("regime_small_to_large", "codes", "abs:kAbsMiss", 1),
    ("regime_small_to_large", "counts", "abs_nres", 2),
    ("regime_small_to_large", "counts", "abs_to_rounds_nres>0", 1),
    ("regime_small_to_large", "counts", "abs_to_rounds_span", 100),
    ("regime_large_to_small", "counts", "abs_pos0_rejected", 1),
    ("file0_miss", "codes", "head:kAbsMiss", 1),
    ("tiny_T_41", "counts", "abs_span_below_1", 1),
    ("tiny_T_41", "counts", "abs_b0_eq_b1", 128),
    ("tiny_T_41", "paths", r"abs", 41),
    ("ext_t254", "codes", "abs:kAbsGeneral", 1),
    # rounds
    ("abs_window_limit", "counts", "round_all_resolved_R32", 1),
    ("regime_small_to_large", "counts", "round_miss_nres>0", 2),
    ("regime_small_to_large", "counts", "round_miss_R32_to_R16", 1),
    ("regime_small_to_large", "counts", "round_miss_R16_to_R1", 1),
    ("regime_small_to_large", "counts", "round_doubling", 5),
    ("file0_miss", "counts", "round_miss_nres0", 1),
    ("file0_miss", "paths", r"general\(missed its window\)", 1),
    ("tiny_T_400_last", "codes", "succ:kSuccLast", 1),
    ("tiny_T_400_stop", "codes", "succ:kSuccStop", 1),
    ("tiny_T_400_general", "codes", "succ:kSuccGeneral", 2),
    ("round_offset0", "counts", "round_lo0_accepted", 1),
    ("round_offset0", "counts", "round_lo0_rejected", 1),
    ("round_offset0", "counts", "round_miss_R32_to_R8", 1),
    # the general step
    ("gen_len1023", "counts", "general_group_len_1023", 1),
    ("gen_len1023", "counts", "general_group_chunks_1", 1),
    ("gen_len1023", "counts", "general_w_chunk0", 1),
    ("gen_len1024", "counts", "general_group_len_1024", 1),
    ("gen_len1024", "counts", "general_group_chunks_2", 1),
    ("gen_len1024", "counts", "general_w_chunk0", 1),
    ("gen_len1025", "counts", "general_group_len_1025", 1),
    ("gen_len1025", "counts", "general_w_chunk1", 1),
    ("gen_len2102_w_chunk2", "counts", "general_group_chunks_3", 1),
    ("gen_len2102_w_chunk2", "counts", "general_w_chunk2", 1),
    ("gen_len2200_no_w", "counts", "general_group_chunks_3", 1),
    ("gen_len2200_no_w", "counts", "general_w_absent", 1),
    ("gen_w_chunk0_long_group", "counts", "general_group_chunks_3", 1),
    ("gen_w_chunk0_long_group", "counts", "general_w_chunk0", 1),
    ("gen_group_to_n", "counts", "general_group_to_n", 1),
    ("gen_group_to_n", "counts", "general_writes_last", 1),
    ("gen_group_to_n", "paths", r"general", 1),
    ("gen_nothing_left", "counts", "general_nothing_left", 1),
    ("gen_nothing_left", "paths", r"general", 0),
    ("ext_t254", "counts", "general_search_short", 1),
    ("file0_miss", "counts", "general_search_strided", 1),
    ("file0_miss_wide", "counts", "general_search_span_max", 19_998),
    # emit
    ("emit_T1", "counts", "emit_research", 344),
    ("emit_T1", "paths", r".", 634),
    ("abs_tail_of_dropped", "counts", "emit_block_past_last_start", 2),
    # sizes, empty keys, tombstones by level
    ("empty_keys_level6", "counts", "empty_key_candidates", 41),
    ("empty_keys_level5", "counts", "empty_key_candidates", 50),
    ("tombstones_level5", "paths", r".", 32),
    ("tombstones_level6", "paths", r".", 25),
]


@pytest.mark.parametrize("name,kind,key,count", COVERAGE,
                         ids=["%s-%s-%s" % (c, k, re.sub(r"\W+", "_", x)) for c, k, x, _ in COVERAGE])
def test_coverage(name, kind, key, count):
    r = census(name)
    if kind == "paths":
        got = sum(1 for p in r.paths if re.match(key, p))
    else:
        got = getattr(r, kind)[key]
    assert got == count, (name, kind, key, got, dict(r.codes), dict(r.counts))


def test_sizes_present():
    assert [wc.BY_NAME["size_n%d" % n].n for n in (1, 2, 511, 512, 513, 1024, 1025)] == \
        [1, 2, 511, 512, 513, 1024, 1025]


def test_general_search_span_departure():
    """A search over more than 1,024 x 1,023 positions needs over a million
    pairs; the widest the 20,000-pair limit allows is the one recorded."""
    assert max(census(n).counts["general_search_span_max"] for n in NAMES) == 19_998


@pytest.mark.parametrize("m", wc.MUTANTS)
def test_mutant_model(m):
    """The model of each mutant turns exactly the recorded cases red, stays in
    the device's buffers, and ends; the recorded unsafe cases are the only
    ones in which it does not."""
    red, unsafe = set(), set()
    for name in NAMES:
        want, wstarts = expected(name)
        try:
            r = wc.census(wc.BY_NAME[name], m)
        except wc.Unsafe:
            unsafe.add(name)
            continue
        if not wc.agrees(r, want, wstarts):
            red.add(name)
    assert red == wc.MUTANT_RED[m]
    assert unsafe == wc.MUTANT_UNSAFE.get(m, set())
