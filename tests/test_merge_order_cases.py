"""The merge's ordering stage, case by case, on the CPU
(tests/merge_order_cases.py): in every case the census's perm must be the
stable sort by Go string order and its plan what the case's name claims; the
COVERAGE table pins, by tag and exact count, which branch of the key
statistics, the host's plan choice and the ordering kernels each case
reaches, so that a later edit of a case cannot lose a path silently."""
import functools
import re
from collections import Counter

import pytest

import pyoracle as ora
import merge_order_cases as mc

NAMES = [c.name for c in mc.CASES]


@functools.lru_cache(maxsize=None)
def census(name):
    return mc.census(mc.BY_NAME[name])


@pytest.mark.parametrize("name", NAMES)
def test_census_is_the_stable_order(name):
    case, r = mc.BY_NAME[name], census(name)
    assert r.perm == mc.stable_order(case)
    assert r.plan[:4] == mc.CLAIM[name], (r.plan, mc.CLAIM[name])
    assert r.plan[4] == (max(len(k) for k, _ in case.pairs) + 7) // 8
    assert case.n <= mc.MAX_PAIRS
    assert case.nbytes() <= mc.MAX_BYTES or name in mc.KEY_CAP_CASES
    # output_of (which says whether a mutant's order changes the output) is merge.go's loop
    want, wstarts = mc.expected(case, ora.TIE_INPUT)
    out, starts = mc.output_of(case, r.perm)
    assert out == want.tolist() and starts == wstarts.tolist()


def test_key_past_the_cap_is_einval():
    r = mc.census(mc.KEY_PAST_CAP)
    assert r.plan is None and r.tags["einval:key_past_cap"] == 1
    assert len(mc.KEY_PAST_CAP.pairs[0][0]) == mc.KEY_CAP + 9
    assert census("keycap_two_keys_1mib").plan[4] == 131_072


def test_sorting_cases_hold_straddling_duplicates_and_distinct_stretches():
    """Every case on the merge path has keys of the long run among the others
    on both sides of the tie (the other first in the input, the run pair
    first) wherever it has others on that side, and stretches of pairs whose
    keys are all distinct, so that a stability error and a misplaced pair each
    change the written indices."""
    for name in NAMES:
        r, case = census(name), mc.BY_NAME[name]
        if r.plan[0] != mc.ORDER_PATH or r.plan[2] == mc.OTHERS_NONE:
            continue
        rs, re_ = r.plan[5], r.plan[6]
        if rs > 0:
            assert r.tags["rank:other_before_equal_run_key"] >= 100, name
        if re_ < case.n:
            assert r.tags["rank:other_after_equal_run_key"] >= 100, name
        keys = [k for k, _ in case.pairs]
        assert sum(1 for c in Counter(keys).values() if c == 1) >= 1000, name
    # one k-way run against another: a key of three others-runs and the long run
    for name in ("path_no_4096_stride_1", "path_no_4097_stride_2", "path_no_8200_stride_3"):
        assert census(name).tags["kway:keys_in_3_runs_and_the_long_run"] >= 1


# (case, tag, exact count)
COVERAGE = [
    # plan boundaries
    ("n4095_radix", "passes:32", 1),
    ("n4096_path", "kway:R=3", 1),
    ("no_half_path", "kway:R=3", 1),
    ("no_half_plus1_radix", "passes:32", 1),
    ("bits32_path32", "all_bits=32", 1),
    ("bits33_path64", "all_bits=33", 1),
    ("bits64_one_field_path64", "all_bits=64", 1),
    ("bits64_one_field_path64", "fields=1", 1),
    ("bits65_len_bit_pass32_then_pass64", "all_bits=65", 1),
    ("bits65_len_bit_pass32_then_pass64", "passes:32,64", 1),
    ("bits65_len_bit_pass32_then_pass64", "group:cut_by_bits", 1),
    ("bits64_two_fields_path64", "all_bits=64", 1),
    ("bits64_two_fields_path64", "fields=2", 1),
    ("fields8_long_keys_path32", "fields=8", 1),
    ("fields8_long_keys_path32", "fields:from_long_stats", 4),
    ("fields8_long_keys_path32", "long_stats:chunks", 4),
    ("fields8_long_keys_path32", "cmp:full_past32", 935),
    ("fields9_long_keys_cut_by_fields", "fields=9", 1),
    ("fields9_long_keys_cut_by_fields", "group:cut_by_fields", 1),
    ("fields9_long_keys_cut_by_fields", "passes:64,32", 1),
    ("fields9_long_keys_cut_by_fields", "pass:fields=8", 1),
    ("fields9_long_keys_cut_by_fields", "fields:short_keys_hold_0", 1),
    ("groups_2x40_bits_cut_by_bits", "all_bits=80", 1),
    ("groups_2x40_bits_cut_by_bits", "passes:64,64", 1),
    ("groups_2x40_bits_cut_by_bits", "group:cut_by_bits", 1),
    ("three_passes", "passes:64,64,64", 1),
    ("three_passes", "group:cut_by_bits", 2),
    # no or trivial fields
    ("all_keys_equal", "iota_only", 1),
    ("all_keys_equal", "cmp:equal", 299),
    ("all_keys_empty", "iota_only", 1),
    ("only_length_varies", "fields=1", 1),
    ("only_length_varies", "all_bits=6", 1),
    ("only_length_varies", "fields:short_keys_hold_0", 5),
    ("only_length_varies", "cmp:full_lengths", 180),
    ("a_a0_a00_among_longer", "cmp:lengths", 6),
    ("a_a0_a00_among_longer", "pass:fields=2", 1),
    # stats and run detection
    ("descent_at_tile_first", "descent:tile_first", 1),
    ("descent_at_tile_last", "descent:tile_last", 1),
    ("descent_at_wave_lane0", "descent:wave_lane0", 1),
    ("run_spans_ten_tiles_equal_neighbours", "stitch:tile_without_descent", 10),
    ("run_spans_ten_tiles_equal_neighbours", "cmp:equal", 120),
    ("run_spans_ten_tiles_equal_neighbours", "run:from_open", 1),
    ("run_starts_at_0", "run:starts_at_0", 1),
    ("run_ends_at_N", "run:ends_at_N", 1),
    ("run_ends_at_N", "run:from_tail", 1),
    ("two_equal_runs_first_wins", "stitch:tie_first_wins", 1),
    ("two_equal_runs_first_wins", "run:starts_at_0", 1),
    ("tiles_with_1_64_65_descents", "tile:descents=1", 1),
    ("tiles_with_1_64_65_descents", "tile:descents=64", 1),
    ("tiles_with_1_64_65_descents", "tile:descents=65", 1),
    ("tiles_with_1_64_65_descents", "tile:inner_run", 1),
    ("tiles_with_1_64_65_descents", "tile:inner_run_skipped", 1),
    ("inner_run_is_the_longest", "run:from_inner", 1),
    ("inner_run_skipped_at_65_descents", "tile:descents=65", 1),
    ("inner_run_skipped_at_65_descents", "run:from_open", 1),
    ("descent_compare_branches", "cmp:prefix", 173),
    ("descent_compare_branches", "cmp:lengths", 25),
    ("descent_compare_branches", "cmp:equal", 26),
    ("descent_compare_branches", "cmp:full_one_side_le32", 42),
    ("descent_compare_branches", "cmp:full_past32", 129),
    ("descent_compare_branches", "cmp:full_lengths", 20),
    ("descent_compare_branches", "cmp:full_equal", 26),
    # the merge path
    ("path_no_others", "path:no_others", 1),
    ("path_no_others", "cmp:equal", 200),
    ("path_others_before_only", "path:others_before_only", 1),
    ("path_others_before_only", "kway:junction_start", 0),
    ("path_others_after_only", "path:others_after_only", 1),
    ("path_junction_descent", "path:junction_descent", 1),
    ("path_junction_descent", "kway:R=2", 1),
    ("path_junction_no_descent", "path:junction_no_descent", 1),
    ("path_junction_no_descent", "kway:R=2", 1),
    ("path_others_run_of_length_1", "kway:run_of_length_1", 1),
    ("path_others_run_of_length_1", "kway:R=4", 1),
    ("path_descents_10_kway", "kway:R=10", 1),
    ("path_descents_11_radix_others", "path:others_radix", 1),
    ("path_no_1024", "kway:workgroups", 1),
    ("path_no_1024", "path:rank_others_workgroups", 4),
    ("path_no_1025", "kway:workgroups", 2),
    ("path_no_1025", "path:rank_others_workgroups", 5),
    ("path_no_4096_stride_1", "kway:stride=1", 1),
    ("path_no_4096_stride_1", "kway:interval_searched", 0),
    ("path_no_4096_stride_1", "kway:probe_below_every_sample", 4),
    ("path_no_4096_stride_1", "kway:probe_equals_a_sample", 960),
    ("path_no_4096_stride_1", "kway:probe_above_every_sample", 3),
    ("path_no_4097_stride_2", "kway:stride=2", 1),
    ("path_no_4097_stride_2", "kway:interval_searched", 8183),
    ("path_no_4097_stride_2", "kway:interval_clipped_by_run_end", 7),
    ("path_no_4097_stride_2", "kway:run_length_multiple_of_stride", 0),
    ("path_no_4097_stride_2", "kway:probe_below_every_sample", 4),
    ("path_no_4097_stride_2", "kway:probe_equals_a_sample", 496),
    ("path_no_4097_stride_2", "kway:probe_above_every_sample", 7),
    ("path_no_8200_stride_3", "kway:stride=3", 1),
    ("path_no_8200_stride_3", "kway:interval_searched", 16388),
    ("path_no_8200_stride_3", "kway:interval_clipped_by_run_end", 6),
    ("path_no_8200_stride_3", "kway:run_length_multiple_of_stride", 0),
    ("path_no_8200_stride_3", "kway:probe_below_every_sample", 6),
    ("path_no_8200_stride_3", "kway:probe_equals_a_sample", 562),
    ("path_no_8200_stride_3", "kway:probe_above_every_sample", 6),
    # the key cap
    ("keycap_two_keys_1mib", "long_stats:chunks", 131_068),
    ("keycap_two_keys_1mib", "cmp:full_past32", 1),
]


@pytest.mark.parametrize("name,tag,count", COVERAGE,
                         ids=["%s-%s" % (c, re.sub(r"\W+", "_", t)) for c, t, _ in COVERAGE])
def test_coverage(name, tag, count):
    r = census(name)
    assert r.tags[tag] == count, (name, tag, r.tags[tag], dict(r.tags))


def test_plan_boundary_pairs_differ_only_at_the_boundary():
    """n4095 / n4096 and no == N/2 / N/2 + 1 are the same shapes a pair apart."""
    a, b = mc.BY_NAME["n4095_radix"], mc.BY_NAME["n4096_path"]
    assert (a.n, b.n) == (4095, 4096) and [k for k, _ in a.pairs] == [k for k, _ in b.pairs][:4095]
    a, b = census("no_half_path").plan, census("no_half_plus1_radix").plan
    assert a[6] - a[5] == 2048 and b[6] - b[5] == 2047
    assert mc.BY_NAME["no_half_path"].n == mc.BY_NAME["no_half_plus1_radix"].n == 4096
    assert census("path_descents_10_kway").plan[7] == 10 and census("path_descents_11_radix_others").plan[7] == 11
    for name, no in (("path_no_1024", 1024), ("path_no_1025", 1025), ("path_no_4096_stride_1", 4096),
                     ("path_no_4097_stride_2", 4097), ("path_no_8200_stride_3", 8200)):
        p = census(name).plan
        assert mc.BY_NAME[name].n - (p[6] - p[5]) == no


def test_inner_run_never_feeds_the_merge_path():
    """A run strictly inside a stats tile is shorter than chunk <= N / 16 and
    the merge path needs N / 2, so the tile's inner run (r[3], r[4]) is never
    the run the path uses; it can be the run lsm_merge_plan reports when the
    radix passes run (inner_run_is_the_longest)."""
    assert all(census(n).tags["path:run_from_inner"] == 0 for n in NAMES)
    assert census("inner_run_is_the_longest").plan[5:7] == (260, 480)


def test_largest_kway_run_count():
    """The k-way list cannot reach R = 11 or 12: the long run is maximal, so of
    the at most 10 descents the host admits at least one bounds the run, and
    the others hold at most 9 starts.  The largest R a case reaches is 10."""
    assert max(census(n).R for n in NAMES) == 10
    assert census("path_descents_10_kway").R == 10


@pytest.mark.parametrize("m", mc.MUTANTS)
def test_mutant_model(m):
    """The model of each mutant turns exactly the recorded cases red and is
    unsafe (a load or store out of the device's buffers, a slot ranked twice,
    no permutation) in exactly the recorded cases."""
    red, unsafe = set(), set()
    for name in NAMES:
        try:
            r = mc.census(mc.BY_NAME[name], m)
        except mc.Unsafe:
            unsafe.add(name)
            continue
        if not mc.agrees(r, mc.BY_NAME[name], census(name).plan):
            red.add(name)
    assert red == mc.MUTANT_RED[m]
    assert unsafe == mc.MUTANT_UNSAFE.get(m, set())


def test_mutants_run_on_the_gpu_were_cleared_and_did_what_the_model_says():
    for m, red in mc.MUTANT_GPU_RED.items():
        assert m in mc.CLEARED and red == mc.MUTANT_RED[m], m
