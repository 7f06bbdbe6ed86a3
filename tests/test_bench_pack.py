"""bench_pack.py's host side (no GPU): the closed form of the packed arenas, the
bytes its roofline counts, and (a)'s verdict from the repeats."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench_db_scan
import bench_pack
from lsmgpu import synth


def test_expected_packed_values_by_answering_source():
    wal = (np.arange(300) % 251).astype(np.uint8)
    ids = np.array([3, 7, 9, 11, 3])
    is_mem = np.array([False, True, True, False, False])
    mem_off = np.array([0, 10, 60, 0, 0])
    mem_live = np.array([True, True, False, True, True])   # id 9: a tombstone the Get hides
    table = np.array([2, -1, -1, -1, 40])                  # id 11: a miss
    keys, koff, vals, voff = bench_pack.expected_packed(ids, is_mem, mem_off, mem_live, table, wal)
    assert voff.tolist() == [0, 100, 124, 124, 124, 224]
    assert koff.tolist() == [0, 16, 32, 48, 64, 80]
    assert keys.tobytes() == b"".join(b"k%015d" % i for i in ids)
    # a table's value: the generator's for id + (table + 1) * 10^9, as bench_db_scan.py builds every table
    assert vals[:100].tobytes() == synth.value_bytes(np.array([3 + 3 * 10 ** 9]), 100).tobytes()
    assert vals[124:].tobytes() == synth.value_bytes(np.array([3 + 41 * 10 ** 9]), 100).tobytes()
    assert vals[:100].tobytes() != vals[124:].tobytes()
    # a memtable's value: the 24 bytes behind the record's key in the log
    assert vals[100:124].tobytes() == wal[10 + 8 + 16:10 + 8 + 16 + 24].tobytes()
    k2, o2, v2, vo2 = bench_pack.expected_packed(ids, is_mem, mem_off, mem_live, table, wal, with_keys=False)
    assert k2 is None and o2 is None and v2.tobytes() == vals.tobytes() and vo2.tolist() == voff.tolist()


def test_expected_packed_across_chunks(monkeypatch):
    monkeypatch.setattr(bench_pack, "CHUNK", 7)
    rng = np.random.default_rng(5)
    wal = rng.integers(0, 256, 4000, dtype=np.uint8)
    n = 40
    ids = rng.integers(0, 1000, n)
    is_mem = rng.random(n) < 0.5
    mem_off = rng.integers(0, 3900, n)
    mem_live = rng.random(n) < 0.8
    table = np.where(rng.random(n) < 0.8, rng.integers(0, 60, n), -1)
    _, _, vals, voff = bench_pack.expected_packed(ids, is_mem, mem_off, mem_live, table, wal)
    for e in range(n):
        got = vals[int(voff[e]):int(voff[e + 1])].tobytes()
        if is_mem[e]:
            want = wal[mem_off[e] + 24:mem_off[e] + 48].tobytes() if mem_live[e] else b""
        elif table[e] >= 0:
            want = bench_pack.table_values([ids[e]], [table[e]]).tobytes()
        else:
            want = b""
        assert got == want, e


def test_roofline_bytes():
    # 2 rows of 3 slots, 4 entries, keys, sources and counts
    assert bench_pack.roofline_bytes(2, 3, 4, 64, 400, True, True, True) == \
        2 * 464 + 6 * 36 + 2 * 4 + (2 * 5 * 8 + 3 * 8 + 4 * 4)
    # the Get shape: one descriptor and the source word per key, no keys, no counts
    assert bench_pack.roofline_bytes(5, 1, 5, 0, 120, False, True, False) == 2 * 120 + 5 * 20 + (6 * 8 + 6 * 8 + 5 * 4)


def test_verdict():
    v = bench_pack.verdict([1.1, 1.1], [1.0, 1.05])
    assert v == {"ratio_pack_over_gather": round(1.1 / 1.025, 4), "gather_spread": 0.05, "margin": 0.15,
                 "inside_margin": True}
    v = bench_pack.verdict([1.3, 1.3, 1.3], [1.0, 1.0, 1.0])
    assert v["ratio_pack_over_gather"] == 1.3 and v["gather_spread"] == 0.0 and v["margin"] == 0.1
    assert v["inside_margin"] is False
    assert bench_pack.verdict([0.9], [1.0])["inside_margin"] is True


def test_defaults():
    a = bench_pack.parse([])
    assert (a.steps, a.warmup, a.repeats, a.ranges, a.keys) == (10, 2, 5, 1 << 16, 1 << 20)
    assert a.out.endswith(os.path.join("profiles", "bench_pack.json"))
    assert bench_pack.LIMITS == bench_db_scan.LIMITS == (16, 100)
    assert (bench_pack.KEY_LEN, bench_pack.MEM_VAL_LEN, bench_pack.TABLE_VAL_LEN) == (16, 24, 100)
    assert bench_pack.EXTRA_PASS_MARGIN == 0.10
