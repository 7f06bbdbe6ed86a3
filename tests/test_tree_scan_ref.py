"""tests/tree_scan_ref.py (the scan of a range as Manager.Search applied to
every key the tree holds in it) against a direct restatement of the iterator
walk over plain Python tables: block.Iterator.Seek / Next / Valid / Key
(sstable/block/index.go:157-181) and sstable.Iterator (sstable/iterator.go:
9-73) per source, the sources in Manager.Search's order (manager.go:99-133),
the level's table picked by the sparse index (:186-192) and the boundary-key
rule, on the trees of tests/tree_scan_cases.py.  The two formulations agree,
and Search answers no collected key GET_ABSENT.  CPU only."""
import pytest

import pyoracle as ora
import tree_scan_cases as cases
import tree_scan_ref
from tree_scan_ref import LIVE, RAW


def go_seek(entries, key):
    """Iterator.Seek (index.go:157-181) -> left."""
    left, right = 0, len(entries)
    while left < right:
        mid = left + (right - left) // 2
        if entries[mid][0] < key:
            left = mid + 1
        else:
            right = mid
    return left


def go_value(file, off):
    """GetValueByOffset (sstable.go:271-296, kv.go:181-200) -> (result, view)."""
    if off < 0:
        return ora.GET_SEEK_FAILED, None
    rest = file[off:] if off < len(file) else b""
    if len(rest) < 4:
        return ora.GET_VALUE_LENGTH, None
    n = int.from_bytes(rest[:4], "little")
    if n > 1 << 30:
        return ora.GET_VALUE_TOO_LONG, None
    if len(rest) - 4 < n:
        return ora.GET_VALUE_SHORT, None
    return ora.GET_FOUND, (off, n)


class Source:
    """One level-0 table, or the participating tables of a level >= 1 walked
    one after the other.  tabs: [(table id, entries)] in sparse-index order."""

    def __init__(self, tabs):
        self.tabs, self.f, self.i = tabs, len(tabs), 0

    def seek(self, f, key):
        """Enter table position f (of tabs) by Seek(key)."""
        self.f, self.i = f, 0
        if f < len(self.tabs):
            self.i = go_seek(self.tabs[f][1], key)
        self.settle()

    def settle(self):
        while self.f < len(self.tabs):
            ent = self.tabs[self.f][1]
            if self.i >= len(ent):              # !Valid: the next table's entry 0
                self.f, self.i = self.f + 1, 0
                continue
            # the boundary key: the next table, the one the sparse index picks, answers
            if self.i == len(ent) - 1 and self.f + 1 < len(self.tabs) and \
                    self.tabs[self.f + 1][1][0][0] == ent[self.i][0]:
                self.f, self.i = self.f + 1, 0
                continue
            return

    def head(self):
        if self.f >= len(self.tabs):
            return None
        return self.tabs[self.f][1][self.i][0]

    def next(self):
        self.i += 1
        self.settle()


def plain_tables(tree):
    tabs = []
    for t, (im, d) in enumerate(zip(tree.images, tree.dec)):
        file = im.tobytes()
        meta, idesc, ival = d[1], d[2], d[3]
        ok = meta.stage == 0 and meta.nidx > 0
        tabs.append({
            "id": t, "file": file, "ok": ok,
            "min": file[int(meta.min_key_off):int(meta.min_key_off) + int(meta.min_key_len)],
            "entries": [(file[int(e["rec_off"]) + 4:int(e["rec_off"]) + 4 + int(e["key_len"])], int(v),
                         int(e["rec_off"]), int(e["key_len"])) for e, v in zip(idesc, ival)] if ok else []})
    return tabs


def walk(tree, tabs, lo, hi, no_upper, limit, mode):
    """-> ([(key, table id, result, view, key rec_off in the file, key_len)], more)."""
    ls = tree.level_start
    sources = []
    for t in tabs[:int(ls[1])]:                     # level 0, newest first
        s = Source([(t["id"], t["entries"])] if t["ok"] else [])
        s.seek(0, lo)
        sources.append(s)
    for L in range(1, cases.LEVELS):
        level = tabs[int(ls[L]):int(ls[L + 1])]
        part = [t for t in level if t["ok"]]
        s = Source([(t["id"], t["entries"]) for t in part])
        if level:
            a, b = 0, len(level)                    # manager.go:186 sort.Search(n, MinKey > key)
            while a < b:
                h = (a + b) >> 1
                if not level[h]["min"] > lo:
                    a = h + 1
                else:
                    b = h
            pick = level[a - 1 if a > 0 else 0]     # :189-191
            if pick["ok"]:
                s.seek(part.index(pick), lo)
            else:                                   # not loaded: the next table that is, from its entry 0
                s.f, s.i = sum(1 for t in part if t["id"] < pick["id"]), 0
                s.settle()
        sources.append(s)
    out, more = [], 0
    while True:
        heads = [s.head() for s in sources]
        live = [k for k in heads if k is not None and (no_upper or k < hi)]
        if not live:
            break
        k = min(live)
        s = sources[heads.index(k)]                 # the first source that holds the key
        tid, ent = s.tabs[s.f]
        _, off, rec_off, key_len = ent[s.i]
        res, view = go_value(tabs[tid]["file"], off)
        tomb = res == ora.GET_FOUND and \
            tabs[tid]["file"][view[0] + 4:view[0] + 4 + view[1]] == tree_scan_ref.TOMBSTONE
        if not (mode == LIVE and tomb):
            if len(out) == limit:
                more = 1
                break
            out.append((k, tid, res, view, rec_off, key_len))
        for x, h in zip(sources, heads):
            if h == k:
                x.next()
    return out, more


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_reference_matches_the_iterator_walk(name):
    case = cases.CASES[name]()
    tree, ref = case.tree, case.tree.ref
    assert ref.absent == 0          # a present key answered GET_ABSENT would hide a failure
    tabs = plain_tables(tree)
    emitted = 0
    for mode in (RAW, LIVE):
        for limit in case.limits:
            for lo, hi, nu in case.ranges:
                idx, more = ref.scan(lo, hi, nu, limit, mode)
                got, gmore = walk(tree, tabs, lo, hi, nu, limit, mode)
                assert gmore == more and len(got) == len(idx), (name, mode, limit, lo, hi, nu)
                for i, (k, tid, res, view, rec_off, key_len) in zip(idx, got):
                    assert ref.keys[i] == k and ref.table[i] == tid and ref.res[i] == res
                    assert ref.koff[i] == int(tree.offs[tid]) + rec_off and ref.klen[i] == key_len
                    if view:
                        assert ref.voff[i] == int(tree.offs[tid]) + view[0] and ref.vlen[i] == view[1]
                    else:
                        assert ref.voff[i] == 0 and ref.vlen[i] == 0
                emitted += len(got)
    assert emitted > 0 or name == "empty_tree"


def test_many_ranges_reference_agrees_on_a_sample():
    case = cases.many_ranges()
    tree, ref = case.tree, case.tree.ref
    tabs = plain_tables(tree)
    for lo, hi, nu in case.ranges[::250]:
        idx, more = ref.scan(lo, hi, nu, 8, LIVE)
        got, gmore = walk(tree, tabs, lo, hi, nu, 8, LIVE)
        assert gmore == more and [ref.keys[i] for i in idx] == [g[0] for g in got]


def test_what_the_cases_hold():
    """The properties the cases exist for, on the reference's answers."""
    c = cases.shadowing()
    ref = c.tree.ref
    i = ref.keys.index(b"s")
    assert ref.table[i] == 0                                   # level-0 table 0 of four holders
    assert ref.tomb[ref.keys.index(b"t")] and ref.table[ref.keys.index(b"t")] == 0
    assert ref.scan(b"w", b"z", False, 2, RAW)[1] == 1 and ref.scan(b"w", b"z", False, 2, LIVE)[1] == 0
    assert [ref.keys[j] for j in ref.scan(b"s", b"u", False, 64, LIVE)[0]] == [b"s"]
    c = cases.seams()
    ref = c.tree.ref
    i = ref.keys.index(b"m9")
    assert ref.table[i] == int(c.tree.level_start[2]) + 1      # the later table's entry
    assert ref.keys.count(b"m9") == 1
    c = cases.value_errors()
    ref = c.tree.ref
    assert ref.res[3] == ora.GET_SEEK_FAILED and ref.res[7] == ora.GET_VALUE_LENGTH
    assert ref.vlen[3] == 0 and ref.vlen[7] == 0 and (ref.table == 0).all()
    c = cases.wide_level0()
    assert int(c.tree.level_start[1]) == 70
    assert cases.mixed().tree.ref.absent == 0 and len(cases.mixed().tree.ref.keys) > 2000
