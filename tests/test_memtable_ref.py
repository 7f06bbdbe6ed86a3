"""Pins memtable_ref.order (the short form lsm_memtable_order is checked
against) to the literal restatement of go-lsm's skiplist, iterator and
RangeScan -- live (the ops applied to the skiplist) and replayed (AddPairs of
the WAL the same ops appended), which must agree: that is the argument that a
WAL image describes its memtable."""
import random

import pytest

import memtable_ref as ref

T = ref.TOMBSTONE


def norm(pairs):
    return [(k, b"" if v is None else bytes(v)) for k, v in pairs]


def short(wal, scan):
    return [(wal[p][0], b"" if wal[p][1] is None else wal[p][1]) for p in ref.order(wal, scan)]


def check(mem):
    """live == replayed == short form, for both scans."""
    back = ref.MemTable.recover(mem.wal, seed=99)
    assert norm(mem.entries.nodes()) == norm(back.entries.nodes()) == short(mem.wal, ref.ALL)
    assert norm(mem.entries.range_scan()) == norm(back.entries.range_scan()) == short(mem.wal, ref.RANGESCAN)
    return short(mem.wal, ref.ALL), short(mem.wal, ref.RANGESCAN)


def run_random(seed):
    rng = random.Random(seed)
    alphabet = [b"", b"a", b"aa", b"ab", b"b", b"ba", b"a\x00", b"\xff", b"abcdefgh", b"abcdefghi"]
    mem = ref.MemTable(seed)
    seen = {"overwrite": 0, "delete_live": 0, "delete_absent": 0}
    for _ in range(rng.randrange(1, 120)):
        key = rng.choice(alphabet)
        present = any(k == key for k, _ in mem.entries.nodes())
        if rng.random() < 0.3:
            seen["delete_live" if present else "delete_absent"] += 1
            before = len(mem.wal)
            mem.manager_delete(key)
            # the nil-value append only when the node existed (memtable.go:86-93)
            assert len(mem.wal) - before == (2 if present else 1)
        else:
            seen["overwrite"] += present
            mem.insert(key, rng.choice([b"", b"v", T, T + b"x", bytes(rng.randrange(256) for _ in range(5))]))
    check(mem)
    return seen


@pytest.mark.parametrize("seed", range(40))
def test_random_ops_live_replayed_and_short_form_agree(seed):
    run_random(seed)


def test_random_ops_cover_overwrites_and_both_kinds_of_delete():
    total = {}
    for seed in range(40):
        for k, v in run_random(seed).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 20 for v in total.values()), total


def test_manager_delete_appends_nil_then_the_tombstone():
    mem = ref.MemTable(1)
    mem.insert(b"k", b"1")
    mem.insert(b"k", b"2")           # overwrite
    mem.manager_delete(b"k")         # delete of a live key: nil, then the tombstone
    mem.manager_delete(b"absent")    # delete of an absent key: the tombstone only
    assert mem.wal == [(b"k", b"1"), (b"k", b"2"), (b"k", None), (b"k", T), (b"absent", T)]
    assert norm(mem.entries.nodes()) == [(b"absent", T), (b"k", T)]
    assert check(mem) == ([(b"absent", T), (b"k", T)], [])


def fixed(ops):
    mem = ref.MemTable(3)
    for key, value in ops:
        if value == "delete":
            mem.manager_delete(key)
        else:
            mem.insert(key, value)
    return check(mem)


def test_leading_tombstones_are_skipped():
    every, scan = fixed([(b"a", T), (b"b", T), (b"c", b"1"), (b"d", b"2")])
    assert every == [(b"a", T), (b"b", T), (b"c", b"1"), (b"d", b"2")]
    assert scan == [(b"c", b"1"), (b"d", b"2")]


def test_tombstone_in_the_middle_ends_the_scan():
    every, scan = fixed([(b"a", b"1"), (b"b", b"2"), (b"c", "delete"), (b"d", b"4"), (b"e", b"5")])
    assert [k for k, _ in every] == [b"a", b"b", b"c", b"d", b"e"]
    assert scan == [(b"a", b"1"), (b"b", b"2")]  # d and e never reach the SSTable


def test_leading_and_middle_tombstones():
    _, scan = fixed([(b"a", T), (b"b", b"1"), (b"c", T), (b"d", b"2")])
    assert scan == [(b"b", b"1")]


def test_only_tombstones():
    every, scan = fixed([(b"a", "delete"), (b"b", T)])
    assert every == [(b"a", T), (b"b", T)] and scan == []


def test_tombstone_overwritten_by_a_put():
    every, scan = fixed([(b"a", b"1"), (b"b", "delete"), (b"b", b"back"), (b"c", b"3")])
    assert every == scan == [(b"a", b"1"), (b"b", b"back"), (b"c", b"3")]


def test_empty_value_and_tombstone_plus_one_byte_are_ordinary():
    ops = [(b"a", b""), (b"b", T + b"!"), (b"c", T[:-1]), (b"d", b"x")]
    every, scan = fixed(ops)
    assert every == scan == ops


def test_empty_log():
    assert ref.order([], ref.ALL) == [] and ref.order([], ref.RANGESCAN) == []


def test_wal_bytes_round_trip():
    import numpy as np
    import pyoracle as ora
    wal = [(b"k", b"1"), (b"", None), (b"kk", T)]
    raw = ref.wal_bytes(wal)
    st, desc, _ = ora.decode_block(ora.GRAMMAR_KV, np.frombuffer(raw, np.uint8))
    assert st == 0 and desc["key_len"].tolist() == [1, 0, 2] and desc["val_len"].tolist() == [1, 0, 13]
