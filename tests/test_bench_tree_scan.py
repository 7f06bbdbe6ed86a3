"""bench_tree_scan.py's host side (no GPU): the tree's tables, the closed form
of which table answers an id, and the expected output of a range."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench_search
import bench_tree_scan
from lsmgpu import synth


def test_tree_is_bench_searchs():
    l0 = [np.array([1, 5, 9]), np.array([2, 5, 7]), np.array([5, 6, 9])]
    tabs = bench_tree_scan.tree_tables(l0)
    assert [L for L, _ in tabs] == [0] * 3 + [1] * 4 + [2] * 8 + [3] * 16 + [4] * 32
    want = [ids for L, c in enumerate(bench_search.LEVEL_TABLES, start=1) for ids in bench_search.level_ids(L, c)]
    assert all(np.array_equal(a[1], b) for a, b in zip(tabs[3:], want))


def test_answers_pick_the_first_table_of_the_trees_order():
    tabs = [(0, np.array([1, 5, 9])), (0, np.array([2, 5, 7])), (1, np.array([0, 1, 2])), (1, np.array([7, 8, 9]))]
    union, table, slot = bench_tree_scan.answers(tabs)
    assert union.tolist() == [0, 1, 2, 5, 7, 8, 9]
    assert table.tolist() == [2, 0, 1, 0, 1, 3, 0]
    assert slot.tolist() == [0, 0, 0, 1, 2, 1, 2]


def test_expected_output_of_a_range():
    union = np.array([0, 1, 2, 5, 7, 8, 9])
    lo = np.array([0, 3, 5, 8, 9, 10])
    count, more, first = bench_tree_scan.expected(union, lo, 2)
    assert first.tolist() == [0, 3, 3, 5, 6, 7]
    assert count.tolist() == [2, 2, 2, 2, 1, 0]
    assert more.tolist() == [1, 1, 1, 0, 0, 0]
    count, more, _ = bench_tree_scan.expected(union, lo, 100)
    assert count.tolist() == [7, 4, 4, 2, 1, 0] and not more.any()


def test_keys_sort_as_their_ids_and_lo_is_uniform():
    ids = np.array([0, 9, 10, 99, 100, 123456, 10 ** 9, 10 ** 12])
    keys = [k.tobytes() for k in synth.keys_for(ids)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    lo = bench_tree_scan.draw_lo(10_000, bench_search.SPACE, 1)
    assert lo.min() >= 0 and lo.max() < bench_search.SPACE
    assert np.array_equal(lo, bench_tree_scan.draw_lo(10_000, bench_search.SPACE, 1))
    hist = np.bincount(lo * 10 // bench_search.SPACE, minlength=10)
    assert hist.min() > 800 and hist.max() < 1200


def test_defaults():
    a = bench_tree_scan.parse([])
    assert (a.steps, a.warmup, a.repeats, a.ranges) == (10, 2, 5, 1 << 16)
    assert bench_tree_scan.LIMITS == (16, 100) and [m for _, m in bench_tree_scan.MODES] == [0, 1]
