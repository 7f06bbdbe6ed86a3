"""bench_search.py's host side (no GPU): the tree recipe's ranges and the
kernel-stats merge."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench_search


def test_levels_are_disjoint_inside_and_overlap_across():
    per_level = {}
    for L, c in enumerate(bench_search.LEVEL_TABLES, start=1):
        tabs = bench_search.level_ids(L, c)
        assert len(tabs) == c == 2 ** (L + 1) and all(t.size == bench_search.PER for t in tabs)
        ids = np.concatenate(tabs)
        assert (np.diff(ids) > 0).all() and 0 <= ids[0] and ids[-1] < bench_search.SPACE
        per_level[L] = (ids, [(int(t[0]), int(t[-1])) for t in tabs])
    for L in (1, 2, 3):  # a shallower table's range meets more than one deeper table's
        lo, hi = per_level[L][1][0]
        assert sum(1 for a, b in per_level[L + 1][1] if a <= hi and b >= lo) >= 2


def test_kstats_merge(tmp_path):
    csv = tmp_path / "k.csv"
    csv.write_text('"Name","Calls","TotalDurationNs","AverageNs"\n'
                   '"lsm::(anonymous namespace)::search_kernel(lsm::GetArgs)",6,3000000,500000\n'
                   '"void at::native::vectorized_elementwise_kernel<4>()",9,900,100\n')
    rep = tmp_path / "r.json"
    rep.write_text(json.dumps({"value": 1.0}))
    bench_search.main(["--kstats", str(csv), "--only", "search", "--steps", "6", "--into", str(rep)])
    got = json.loads(rep.read_text())
    assert got["value"] == 1.0
    assert got["kernels_search"]["per_kernel"] == [
        {"kernel": "search_kernel", "calls_per_step": 1.0, "avg_us": 500.0, "us_per_step": 500.0}]
