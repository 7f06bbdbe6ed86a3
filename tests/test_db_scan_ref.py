"""tests/db_scan_ref.py (the scan as lsm_memtable_search's answer, else
lsm_search's, for every key any source holds) against a literal k-way merge of
iterators: the restated skiplist of memtable_ref.py per log, newest first
(memtable.Manager.Search's order), entered at its first node with key >= lo and
walked along its level-0 links -- every node takes part, the tombstones too --
then tests/test_tree_scan_ref.py's Source walk per table source.  The two
agree on every case of tests/db_scan_cases.py, and no collected key is answered
ABSENT.  The merge also counts which paths its steps take; CENSUS pins those
counts per case, so that a case cannot silently lose what it was built for.
CPU only."""
import collections
import functools

import pytest

import db_scan_cases as cases
import pyoracle as ora
from db_scan_ref import LIVE, RAW, SRC_MEMTABLE, SRC_SSTABLE
from memtable_ref import MemTable, is_deleted
from test_tree_scan_ref import Source, go_value, plain_tables, prefix16


class MemIter:
    """The skiplist of one log as the scan walks it: Seek by SkipList.Search's
    descent (skiplist.go:60-79), then the level-0 links."""

    def __init__(self, records, seed):
        self.sl = MemTable.recover(records, seed).entries
        self.curr = None

    def seek(self, key):
        sl, curr = self.sl, self.sl.head
        for i in range(sl.level - 1, -1, -1):
            while curr.forward[i] is not None and curr.forward[i].key < key:
                curr = curr.forward[i]
        self.curr = curr.forward[0]

    def head(self):
        return None if self.curr is None else self.curr.key

    def next(self):
        self.curr = self.curr.forward[0]


def table_sources(tree, tabs, lo):
    """test_tree_scan_ref.walk's sources, each entered by Seek(lo)."""
    ls = tree.level_start
    sources = []
    for t in tabs[:int(ls[1])]:
        s = Source([(t["id"], t["entries"])] if t["ok"] else [], t["id"] + 1)
        s.seek(0, lo)
        sources.append(s)
    for L in range(1, cases.LEVELS):
        level = tabs[int(ls[L]):int(ls[L + 1])]
        part = [t for t in level if t["ok"]]
        s = Source([(t["id"], t["entries"]) for t in part], int(ls[L + 1]))
        if level:
            a, b = 0, len(level)
            while a < b:
                h = (a + b) >> 1
                if not level[h]["min"] > lo:
                    a = h + 1
                else:
                    b = h
            pick = level[a - 1 if a > 0 else 0]
            if pick["ok"]:
                s.seek(part.index(pick), lo)
            else:
                s.f, s.i = sum(1 for t in part if t["id"] < pick["id"]), 0
                s.settle()
        sources.append(s)
    return sources


def merge(db, tabs, lo, hi, no_upper, limit, mode, counts):
    """-> ([(key, src, log or table id, result, value bytes or None)], more)."""
    nlog = len(db.records)
    mems = []
    for s in range(nlog):                      # source s is log nlog - 1 - s
        w = nlog - 1 - s
        it = MemIter([] if db.ref_logs[w] is None else db.ref_logs[w], w)
        it.seek(lo)
        mems.append(it)
    sources = mems + table_sources(db.tree, tabs, lo)
    inside = lambda key: key is not None and (no_upper or key < hi)  # noqa: E731
    out, more, skipped_when_full = [], 0, 0
    empty_range = not no_upper and lo >= hi
    while not empty_range:
        heads = [s.head() for s in sources]
        live = [k for k in heads if inside(k)]
        if not live:
            break
        k = min(live)
        tied = [j for j, h in enumerate(heads) if h == k]
        first = tied[0]
        # the tie past 16 bytes: the lowest source among the equal prefixes leads
        same = [j for j, h in enumerate(heads) if inside(h) and prefix16(h) == prefix16(k)]
        if len(k) > 16 and len(set(heads[j] for j in same)) > 1:
            counts["tie:tail_mem_lead" if same[0] < nlog else "tie:tail_table_lead"] += 1
        if first < nlog:
            node = sources[first].curr
            src, where, res, value = SRC_MEMTABLE, nlog - 1 - first, ora.GET_FOUND, bytes(node.value)
            tomb = is_deleted(node.value)
        else:
            s = sources[first]
            tid, ent = s.tabs[s.f]
            res, view = go_value(tabs[tid]["file"], ent[s.i][1])
            value = tabs[tid]["file"][view[0] + 4:view[0] + 4 + view[1]] if view else None
            src, where, tomb = SRC_SSTABLE, tid, res == ora.GET_FOUND and is_deleted(value)
        if not (mode == LIVE and tomb):
            if len(out) == limit:
                more = 1
                break
            out.append((k, src, where, res, value))
            counts["entry:memtable" if src == SRC_MEMTABLE else "entry:table"] += 1
            if tomb:
                counts["tomb:raw_emitted"] += 1
            if src == SRC_MEMTABLE and any(j < nlog for j in tied[1:]):
                counts["shadow:mem_over_mem"] += 1
            if src == SRC_MEMTABLE and any(j >= nlog for j in tied[1:]):
                counts["shadow:mem_over_table"] += 1
        else:
            counts["tomb:live_skipped"] += 1
            counts["tomb:live_skipped:memtable" if src == SRC_MEMTABLE else "tomb:live_skipped:table"] += 1
            if len(tied) > 1:
                counts["tomb:live_hides_older"] += 1
            skipped_when_full += len(out) == limit
        for j in tied:
            sources[j].next()
    if more:
        counts["more:raw" if mode == RAW else "more:live"] += 1
    elif mode == LIVE and skipped_when_full:
        counts["live:tombstone_tail_more0"] += 1
    return out, more


@functools.lru_cache(maxsize=None)
def compared(name):
    case = cases.CASES[name]()
    db, ref = case.db, case.db.ref
    assert ref.absent == 0 and db.tree.ref.absent == 0
    tabs = plain_tables(db.tree)
    emitted, counts = 0, collections.Counter()
    for mode in (RAW, LIVE):
        for limit in case.limits:
            for lo, hi, nu in case.ranges:
                idx, more = ref.scan(lo, hi, nu, limit, mode)
                got, gmore = merge(db, tabs, lo, hi, nu, limit, mode, counts)
                assert gmore == more and len(got) == len(idx), (name, mode, limit, lo, hi, nu)
                for i, (k, src, where, res, value) in zip(idx, got):
                    assert ref.keys[i] == k and ref.src[i] == src, (name, k)
                    if src == SRC_MEMTABLE:
                        assert ref.log[i] == where and res == ora.GET_FOUND
                    else:
                        t = int(ref.tree[i])
                        assert db.tree.ref.table[t] == where and db.tree.ref.res[t] == res
                        assert res != ora.GET_ABSENT
                    assert ref.value(i, db.tree.buf) == value, (name, k)
                emitted += len(got)
    return emitted, counts


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_reference_matches_the_merge_of_iterators(name):
    emitted, _ = compared(name)
    assert emitted > 0 or name == "both_empty"


# (case, path, "==" | ">=", count): the census of the merge over every mode,
# limit and range of the case.  Exact counts, so that an edit of a case shows
# here; a path a case must not reach is 0.
CENSUS = [
    ("node_counts", "entry:memtable", "==", 66),
    ("node_counts", "entry:table", "==", 7),
    ("node_counts", "shadow:mem_over_mem", "==", 12),
    ("node_counts", "shadow:mem_over_table", "==", 20),
    ("shadowing", "entry:memtable", "==", 84),
    ("shadowing", "entry:table", "==", 13),
    ("shadowing", "shadow:mem_over_mem", "==", 32),
    ("shadowing", "shadow:mem_over_table", "==", 31),
    ("shadowing", "tomb:live_skipped:memtable", "==", 40),
    ("shadowing", "tomb:live_skipped:table", "==", 10),
    ("shadowing", "tomb:live_hides_older", "==", 24),
    ("shadowing", "tomb:raw_emitted", "==", 36),
    ("shadowing", "more:raw", "==", 10),
    ("shadowing", "more:live", "==", 4),
    ("shadowing", "live:tombstone_tail_more0", "==", 2),
    ("keys", "tie:tail_mem_lead", "==", 50),
    ("keys", "tie:tail_table_lead", "==", 5),
    ("keys", "shadow:mem_over_table", "==", 59),
    ("keys", "tomb:live_skipped:memtable", "==", 8),
    ("width_16", "entry:memtable", "==", 45),
    ("width_16", "entry:table", "==", 230),
    ("width_64", "tie:tail_mem_lead", "==", 161),
    ("width_64", "tie:tail_table_lead", "==", 6),
    ("width_64", "shadow:mem_over_mem", "==", 29),
    ("width_65", "tie:tail_mem_lead", "==", 163),
    ("width_65", "tie:tail_table_lead", "==", 2),
    ("width_65", "shadow:mem_over_mem", "==", 29),
    ("width_65", "tomb:live_skipped:memtable", "==", 23),
    ("wide_134", "entry:memtable", "==", 43),
    ("wide_134", "entry:table", "==", 8),
    ("wide_134", "shadow:mem_over_mem", "==", 36),
    ("wide_134", "shadow:mem_over_table", "==", 34),
    ("wide_134", "tie:tail_mem_lead", "==", 21),
    ("tree_alone", "entry:memtable", "==", 0),
    ("tree_alone", "entry:table", "==", 886),
    ("logs_alone", "entry:table", "==", 0),
    ("logs_alone", "entry:memtable", "==", 28),
    ("logs_alone", "tomb:live_skipped:memtable", "==", 9),
    ("both_empty", "entry:memtable", "==", 0),
    ("both_empty", "entry:table", "==", 0),
]


@pytest.mark.parametrize("name,path,op,count", CENSUS,
                         ids=["%s-%s" % (c, p.replace(":", "_")) for c, p, _, _ in CENSUS])
def test_census(name, path, op, count):
    counts = compared(name)[1]
    got = counts[path]
    assert got == count if op == "==" else got >= count, (name, path, got, dict(counts))


def test_what_the_cases_hold():
    c = cases.shadowing()
    ref = c.db.ref
    at = {k: i for i, k in enumerate(ref.keys)}
    assert ref.src[at[b"s"]] == SRC_MEMTABLE and ref.log[at[b"s"]] == 1 and ref.tomb[at[b"s"]]
    assert ref.src[at[b"t"]] == SRC_MEMTABLE and not ref.tomb[at[b"t"]]          # over the level-0 tombstone
    assert c.db.tree.ref.tomb[c.db.tree.ref.keys.index(b"t")]
    assert ref.value(at[b"e"], c.db.tree.buf) == b"" and not ref.tomb[at[b"e"]]   # (key, ""): found, length 0
    assert ref.tomb[at[b"del"]] and ref.log[at[b"del"]] == 1
    assert ref.scan(b"y", b"z", False, 1, RAW) == ([at[b"y1"]], 1)
    assert ref.scan(b"y", b"z", False, 1, LIVE) == ([at[b"y1"]], 0)
    assert [ref.keys[i] for i in ref.scan(b"s", b"u", False, 64, LIVE)[0]] == [b"t"]
    c = cases.node_counts()
    assert [None if lg is None else len(set(k for k, _ in lg)) for lg in c.db.ref_logs] == [5, 0, 1, None, 2, 1]
    assert b"q" not in c.db.ref.keys                                             # the failed log's key
    for name, nsrc in (("width_16", 16), ("width_17", 17), ("width_64", 64), ("width_65", 65), ("wide_134", 134)):
        db = cases.CASES[name]().db
        assert db.nsrc == nsrc
        assert all(2 <= len(set(k for k, _ in lg)) <= 6 for lg in db.records)
    assert len(cases.width_64().db.records) == 11 and len(cases.wide_134().db.records) == 70
    # lo and hi equal to memtable keys
    c = cases.keys_case()
    ref = c.db.ref
    out, _ = ref.scan(cases.LONG, cases.LONG + b"C", False, 64, RAW)
    assert ref.keys[out[0]] == cases.LONG and ref.src[out[0]] == SRC_MEMTABLE
    assert cases.LONG + b"C" not in [ref.keys[i] for i in out]
    assert ref.src[ref.keys.index(cases.LONG + b"C")] == SRC_MEMTABLE


def test_strides():
    t = cases.strides()
    assert t.nq == 2 * cases.tsc.WALK_STRIDE + 37 and len(t.db.records) == 3
    for mode in (RAW, LIVE):
        count, more, idx = t.want(mode)
        q = t.nq - 1
        out, m = t.db.ref.scan(*t.ranges[q], t.limit, mode)
        assert count[q] == len(out) and more[q] == m and list(idx[q, :len(out)]) == out
    count = t.want(RAW)[0][:len(t.pattern)]
    assert (count == t.limit).any() and (count == 0).sum() >= 2
    step = cases.tsc.WALK_STRIDE % len(t.pattern)
    assert step and all(t.pattern[i] != t.pattern[(i + step) % len(t.pattern)] for i in range(len(t.pattern)))
