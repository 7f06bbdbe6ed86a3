"""bench_db_scan.py's host side (no GPU): the logs' closed form (the newest log
holding an id, its last record there), the database's union, and the expected
output of a range in both modes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench_db_scan
import bench_get
import bench_memtable
import memtable_search_ref as msr

REC, TOMB_REC = 8 + bench_db_scan.KEY_LEN + bench_db_scan.VAL_LEN, 8 + bench_db_scan.KEY_LEN + bench_db_scan.TOMB_LEN


def test_memtable_nodes_are_the_newest_logs_last_record():
    logs = [(np.array([5, 2, 5, 9]), np.array([False, True, False, False])),
            (np.array([2, 7]), np.array([False, True])),
            (np.array([9, 9, 3]), np.array([True, False, True]))]
    offs = [0, 1000, 2000]
    ids, log, rec_off, tomb = bench_db_scan.memtable_nodes(logs, offs)
    assert ids.tolist() == [2, 3, 5, 7, 9]
    assert log.tolist() == [1, 2, 0, 1, 2]
    assert tomb.tolist() == [False, True, False, True, False]
    assert rec_off.tolist() == [1000, 2000 + TOMB_REC + REC, REC + TOMB_REC, 1000 + REC, 2000 + TOMB_REC]
    # the same answer as the reference's walk over the logs, newest first
    recs = [[(b"%d" % i, bench_memtable.TOMBSTONE if t else b"v") for i, t in zip(a.tolist(), b.tolist())]
            for a, b in logs]
    for i, w, t in zip(ids.tolist(), log.tolist(), tomb.tolist()):
        res, lg, _, _ = msr.search(recs, b"%d" % i)
        assert (lg, res == msr.DELETED) == (w, t)


def test_memtable_nodes_agree_with_bench_gets_closed_form():
    logs = [bench_memtable.gen_log(20_000, 7 + w) for w in range(3)]
    offs = [0, 32_000, 64_000]
    ids, log, rec_off, tomb = bench_db_scan.memtable_nodes([(i, t) for _, i, t in logs], offs)
    res, lg, _, voff, _ = bench_get.expected_memtable([(i, t) for _, i, t in logs], offs, ids)
    assert (res != bench_get.MISS).all() and np.array_equal(lg, log)
    assert np.array_equal(res == bench_get.DELETED, tomb) and tomb.any() and not tomb.all()
    live = ~tomb
    assert np.array_equal(voff[live].astype(np.int64), rec_off[live] + 4 + bench_db_scan.KEY_LEN)
    # the record at rec_off is the id's key
    for i, w, o in list(zip(ids.tolist(), log.tolist(), rec_off.tolist()))[::50]:
        buf = logs[w][0]
        at = o - offs[w]
        assert buf[at + 4:at + 4 + 16].tobytes() == b"k%015d" % i


def test_database_union_prefers_the_memtables():
    union, mem_at, tree_at = bench_db_scan.database(np.array([2, 5, 9]), np.array([1, 2, 7, 9, 11]))
    assert union.tolist() == [1, 2, 5, 7, 9, 11]
    assert mem_at.tolist() == [-1, 0, 1, -1, 2, -1]
    assert tree_at.tolist() == [0, -1, -1, 2, -1, 4]


def test_expected_output_of_a_range_in_both_modes():
    union = np.array([0, 1, 2, 5, 7, 8, 9])
    lo = np.array([0, 3, 5, 8, 9, 10])
    none = np.zeros(7, bool)
    count, more, at = bench_db_scan.expected(union, none, lo, 2)
    assert count.tolist() == [2, 2, 2, 2, 1, 0] and more.tolist() == [1, 1, 1, 0, 0, 0]
    assert at.tolist() == [[0, 1], [3, 4], [3, 4], [5, 6], [6, -1], [-1, -1]]
    dead = np.array([False, True, False, True, False, False, True])   # 1, 5 and 9 are tombstones
    count, more, at = bench_db_scan.expected(union, dead, lo, 2)
    assert count.tolist() == [2, 2, 2, 1, 0, 0] and more.tolist() == [1, 0, 0, 0, 0, 0]
    assert at.tolist() == [[0, 2], [4, 5], [4, 5], [5, -1], [-1, -1], [-1, -1]]
    count, more, at = bench_db_scan.expected(union, np.ones(7, bool), lo, 2)
    assert not count.any() and not more.any() and (at == -1).all()


def test_defaults():
    a = bench_db_scan.parse([])
    assert (a.steps, a.warmup, a.repeats, a.ranges) == (10, 2, 5, 1 << 16)
    assert bench_db_scan.LIMITS == (16, 100) and [m for _, m in bench_db_scan.MODES] == [0, 1]
    assert (bench_get.NLOG, bench_get.LOG_BYTES) == (11, 2 << 20)
