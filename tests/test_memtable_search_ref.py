"""Pins the short form of tests/memtable_search_ref.py (what the GPU is checked
against) to the literal restatement of SkipList.Search, Manager.Search and
database.Get in the same file, over random Insert / Manager.Delete sequences
spread over several memtables, both live and recovered from the WALs."""
import random

import pytest

import memtable_search_ref as ref
from memtable_ref import TOMBSTONE


def replayed(wal):
    """A WAL's records as wal.Recover delivers them: nil reads back empty."""
    return [(k, b"" if v is None else bytes(v)) for k, v in wal]


def random_manager(seed, nops=400, nkeys=60, p_full=0.02, max_tables=11):
    rng = random.Random(seed)
    m = ref.Manager(seed)
    for i in range(nops):
        key = b"k%03d" % rng.randrange(nkeys)
        full = rng.random() < p_full and len(m.tables()) < max_tables
        if rng.random() < 0.3:
            m.delete(key, full=full)
        else:
            m.insert(key, rng.choice([b"v%d" % i, b"", TOMBSTONE + b"!", TOMBSTONE[:-1]]), full=full)
    return m


def probes(nkeys=60):
    return [b"k%03d" % i for i in range(nkeys + 5)] + [b"", b"k", b"k000\x00", b"zzz"]


def check_against(manager, logs):
    """manager.search_where / search against the short form over logs."""
    tables = [ref.last_positions(lg) for lg in logs]
    seen = set()
    for key in probes():
        w, value, ok = manager.search_where(key)
        result, log, pos, short = ref.search(logs, key, tables)
        assert ok == (result != ref.MISS), key
        assert w == log, key
        assert value == short, key                       # nil for a tombstone and for a miss
        assert (result == ref.DELETED) == (ok and value is None), key
        assert manager.search(key) == short, key
        if result != ref.MISS:
            assert logs[log][pos][0] == key and pos == max(i for i, (k, _) in enumerate(logs[log]) if k == key)
        seen.add(result)
    return seen


@pytest.mark.parametrize("seed", range(8))
def test_short_form_equals_manager_search_live_and_recovered(seed):
    live = random_manager(seed)
    wals = [t.wal for t in live.tables()]
    logs = [replayed(w) for w in wals]
    assert len(logs) >= 2
    seen = check_against(live, logs)
    seen |= check_against(ref.Manager.recover(wals, seed=seed + 100), logs)
    assert seen == {ref.MISS, ref.VALUE, ref.DELETED}


def test_nil_value_live_falls_through_replayed_is_an_empty_value():
    m = ref.Manager()
    m.insert(b"k", None)
    assert m.search_where(b"k") == (0, None, True) and m.search(b"k") is None
    older = {b"k": (b"from-the-tables", None)}
    sst = lambda key: older.get(key, (None, None))  # noqa: E731
    assert ref.database_get(m.search, sst, b"k") == (b"from-the-tables", None)
    rec = ref.Manager.recover([m.mem.wal])
    assert rec.search_where(b"k") == (0, b"", True)
    assert ref.database_get(rec.search, sst, b"k") == (b"", None)  # non-nil: Get returns it
    logs = [replayed(m.mem.wal)]
    assert ref.search(logs, b"k") == (ref.VALUE, 0, 0, b"")
    for mode in (ref.EXACT, ref.TOMBSTONE_HIDES):
        assert ref.get(logs, sst, b"k", mode) == (ref.SRC_MEMTABLE, b"", None)


def test_tombstone_in_a_newer_memtable_hides_the_older_value():
    m = ref.Manager()
    m.insert(b"k", b"old")
    m.insert(b"other", b"x")
    m.delete(b"k", full=True)  # the full memtable is promoted, the new Mem holds the tombstone
    assert len(m.tables()) == 2
    # live: the old node is unlinked; replayed: the old log ends in (k, "")
    assert ref.skiplist_search(m.imems[0].entries, b"k") == (None, False)
    logs = [replayed(t.wal) for t in m.tables()]
    assert logs[0][-1] == (b"k", b"") and logs[1] == [(b"k", TOMBSTONE)]
    rec = ref.Manager.recover([t.wal for t in m.tables()])
    assert ref.skiplist_search(rec.imems[0].entries, b"k") == (b"", True)
    for mgr in (m, rec):  # the newer log is searched first: the same answer
        assert mgr.search_where(b"k") == (1, None, True) and mgr.search(b"k") is None
    assert ref.search(logs, b"k") == (ref.DELETED, 1, 0, None)
    assert ref.search(logs[:1], b"k") == (ref.VALUE, 0, 2, b"")  # without the newer log it differs
    # database.Get as written goes on to the tables and returns the older value there
    sst = lambda key: {b"k": (b"older-in-a-table", None)}.get(key, (None, None))  # noqa: E731
    assert ref.database_get(m.search, sst, b"k") == (b"older-in-a-table", None)
    assert ref.get(logs, sst, b"k", ref.EXACT) == (ref.SRC_SSTABLE, b"older-in-a-table", None)
    assert ref.get(logs, sst, b"k", ref.TOMBSTONE_HIDES) == (ref.SRC_MEMTABLE, None, None)
    # a table's tombstone bytes come back as an ordinary value
    sst2 = lambda key: (TOMBSTONE, None)  # noqa: E731
    assert ref.get(logs, sst2, b"k", ref.EXACT) == (ref.SRC_SSTABLE, TOMBSTONE, None)


@pytest.mark.parametrize("seed", range(4))
def test_exact_mode_equals_database_get(seed):
    rng = random.Random(1000 + seed)
    live = random_manager(50 + seed)
    wals = [t.wal for t in live.tables()]
    logs = [replayed(w) for w in wals]
    rec = ref.Manager.recover(wals)
    table = {}
    for key in probes():
        r = rng.random()
        if r < 0.4:
            table[key] = (b"t" + key, None)
        elif r < 0.5:
            table[key] = (None, "seek to offset failed")
        elif r < 0.6:
            table[key] = (TOMBSTONE, None)
    sst = lambda key: table.get(key, (None, None))  # noqa: E731
    srcs = set()
    for key in probes():
        src, value, err = ref.get(logs, sst, key, ref.EXACT)
        assert ref.database_get(rec.search, sst, key) == (value, err), key
        assert (src == ref.SRC_NONE) == (value is None and err is None)
        srcs.add(src)
        # the recommended mode differs only where the memtables hold a tombstone
        hid = ref.get(logs, sst, key, ref.TOMBSTONE_HIDES)
        if ref.search(logs, key)[0] == ref.DELETED:
            assert hid == (ref.SRC_MEMTABLE, None, None)
        else:
            assert hid == (src, value, err)
    assert srcs == {ref.SRC_NONE, ref.SRC_MEMTABLE, ref.SRC_SSTABLE}


def test_recover_keeps_mem_and_the_last_ten_imems():
    wals = [[(b"k", b"%d" % w)] + ([(b"only%d" % w, b"x")]) for w in range(13)]
    rec = ref.Manager.recover(wals)
    assert len(rec.tables()) == 11
    logs = [replayed(w) for w in wals[-11:]]
    assert rec.search_where(b"k") == (10, b"12", True) and ref.search(logs, b"k")[:2] == (ref.VALUE, 10)
    assert rec.search(b"only1") is None and ref.search(logs, b"only1")[0] == ref.MISS  # dropped with its log
    assert rec.search_where(b"only2")[0] == 0 and ref.search(logs, b"only2")[:2] == (ref.VALUE, 0)
