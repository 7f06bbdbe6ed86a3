"""tests/tree_scan_ref.py (the scan of a range as Manager.Search applied to
every key the tree holds in it) against a direct restatement of the iterator
walk over plain Python tables: block.Iterator.Seek / Next / Valid / Key
(sstable/block/index.go:157-181) and sstable.Iterator (sstable/iterator.go:
9-73) per source, the sources in Manager.Search's order (manager.go:99-133),
the level's table picked by the sparse index (:186-192) and the boundary-key
rule, on the trees of tests/tree_scan_cases.py.  The two formulations agree,
and Search answers no collected key GET_ABSENT.  The walk also counts, from
table sizes and source numbers alone, the path each step takes in
lsm_tree_scan's two forms (a lane per source up to 64 sources, rounds of 64
past that); COVERAGE pins those counts per case, so that a later edit of a
case cannot silently lose the path it was built for.  CPU only."""
import collections
import functools

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


WAVE = 64   # lanes: source s is lane s % 64 of round s // 64; a DPP row is 16 lanes


class Source:
    """One level-0 table, or the participating tables of a level >= 1 walked
    one after the other.  tabs: [(table id, entries)] in sparse-index order;
    end: the id one past the source's last table, participating or not.
    counts (a Counter, or None): the census of the paths taken."""

    def __init__(self, tabs, end=None, counts=None):
        self.tabs, self.f, self.i = tabs, len(tabs), 0
        self.end, self.counts = end, counts

    def seek(self, f, key):
        """Enter table position f (of tabs) by Seek(key)."""
        self.f, self.i = f, 0
        if f < len(self.tabs):
            self.i = go_seek(self.tabs[f][1], key)
        self.settle()

    def to_next_table(self, why):
        if self.counts is not None:
            self.counts[why] += 1
            here = self.tabs[self.f][0]
            there = self.tabs[self.f + 1][0] if self.f + 1 < len(self.tabs) else self.end
            if there is not None and there != here + 1:   # tables in between that do not take part
                self.counts["place:skip_nonparticipating"] += 1
                if self.f + 1 == len(self.tabs):
                    self.counts["place:skip_nonparticipating_to_the_end"] += 1
        self.f, self.i = self.f + 1, 0

    def settle(self):
        while self.f < len(self.tabs):
            ent = self.tabs[self.f][1]
            if self.i >= len(ent):              # !Valid: the next table's entry 0
                self.to_next_table("place:hop")
                continue
            # the boundary key: the next table, the one the sparse index picks, answers
            if self.i == len(ent) - 1 and self.f + 1 < len(self.tabs) and \
                    self.tabs[self.f + 1][1][0][0] == ent[self.i][0]:
                self.to_next_table("place:boundary")
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
        ok = tree_scan_ref.takes_part(meta)
        tabs.append({
            "id": t, "file": file, "ok": ok,
            "min": file[int(meta.min_key_off):int(meta.min_key_off) + int(meta.min_key_len)],
            "entries": [(file[int(e["rec_off"]) + 4:int(e["rec_off"]) + 4 + int(e["key_len"])], int(v),
                         int(e["rec_off"]), int(e["key_len"])) for e, v in zip(idesc, ival)] if ok else []})
    return tabs


def prefix16(key):
    """The 16-byte zero-padded prefix the merge compares first."""
    return key[:16].ljust(16, b"\x00")


def census_step(counts, heads, tied, k, wide):
    """What one step of the merge meets, from the sources' numbers and their
    heads alone: heads[s] is source s's key (None: exhausted or past the
    range's end), tied the sources that hold the least key k."""
    w = tied[0]
    counts["winner:row%d" % (w % WAVE // 16)] += 1
    counts["winner:round%d" % (w // WAVE)] += 1
    if len(set(s % WAVE for s in tied)) < len(tied):
        counts["lane_tie:two_rounds"] += 1
    counts["advance:sources:max"] = max(counts["advance:sources:max"], len(tied))
    if any(prefix16(k)[j:j + 4] == b"\xff" * 4 for j in (0, 4, 8, 12)):
        counts["key:ff_prefix"] += 1       # a prefix word equal to the reduction's "no candidate"
    # a lane's candidate: the least of its heads, the lower source on equal keys
    lane_key = {}
    for s, h in enumerate(heads):
        if h is None:
            continue
        lane = s % WAVE
        if lane in lane_key:
            b = lane_key[lane]
            if prefix16(h) == prefix16(b) and len(h) > 16 and len(b) > 16:
                counts["wide:lane_cmp_tail"] += 1
            if h < b:
                lane_key[lane] = h
        else:
            lane_key[lane] = h
        if wide and h != k and prefix16(h) == prefix16(k) and len(h) > 16 and len(k) > 16:
            counts["wide:advance_cmp_tail"] += 1   # the advance's compare decided past 16 bytes
    same = [(lane, key) for lane, key in sorted(lane_key.items()) if prefix16(key) == prefix16(k)]
    if len(set(key for _, key in same)) > 1:
        counts["tie:by_length" if len(k) <= 16 else "tie:tail"] += 1
    if len(k) > 16:
        # every tied key goes on past 16 bytes: the lead moves to the lowest lane with a smaller key
        lead, moves = same[0][1], 0
        while True:
            less = [key for _, key in same if key[16:] < lead[16:]]
            if not less:
                break
            lead, moves = less[0], moves + 1
        counts["tie:tail_lead_moves"] += moves
        counts["tie:tail_lead_moves:max"] = max(counts["tie:tail_lead_moves:max"], moves)


def walk(tree, tabs, lo, hi, no_upper, limit, mode, counts=None):
    """-> ([(key, table id, result, view, key rec_off in the file, key_len)], more).
    counts: a Counter that receives the census of the paths the kernel's step
    would take at each point (the register path up to 64 sources -- a table's
    entries but the last two advance without place() -- the workspace path
    past that), derived from table sizes and source numbers."""
    ls = tree.level_start
    wide = int(ls[1]) + cases.LEVELS - 1 > WAVE
    sources = []
    for t in tabs[:int(ls[1])]:                     # level 0, newest first
        s = Source([(t["id"], t["entries"])] if t["ok"] else [], t["id"] + 1, counts)
        s.seek(0, lo)
        sources.append(s)
    for L in range(1, cases.LEVELS):
        level = tabs[int(ls[L]):int(ls[L + 1])]
        part = [t for t in level if t["ok"]]
        s = Source([(t["id"], t["entries"]) for t in part], int(ls[L + 1]), counts)
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
                if counts is not None:
                    counts["seek:picked_nonparticipating"] += 1
                s.f, s.i = sum(1 for t in part if t["id"] < pick["id"]), 0
                s.settle()
        sources.append(s)
    inside = lambda key: key is not None and (no_upper or key < hi)
    out, more, skipped_when_full = [], 0, 0
    while True:
        heads = [s.head() for s in sources]
        live = [k for k in heads if inside(k)]
        if not live:
            break
        k = min(live)
        tied = [j for j, h in enumerate(heads) if h == k]
        s = sources[tied[0]]                        # the first source that holds the key
        if counts is not None:
            census_step(counts, [h if inside(h) else None for h in heads], tied, k, wide)
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
            if counts is not None and res != ora.GET_FOUND:
                counts["value_error:wide" if wide else "value_error:registers"] += 1
        elif counts is not None:
            counts["live:skipped"] += 1
            skipped_when_full += len(out) == limit
        for j in tied:
            x = sources[j]
            n = len(x.tabs[x.f][1])
            fast = not wide and x.i + 2 < n         # the next entry is not the table's last: no place()
            if counts is not None:
                counts["advance:fast" if fast else "advance:place"] += 1
                if fast:
                    counts["fast:from_len%d" % min(len(k), 18)] += 1
                    counts["fast:to_len%d" % min(len(x.tabs[x.f][1][x.i + 1][0]), 18)] += 1
            x.next()
            if counts is not None and x.head() is not None and not inside(x.head()):
                counts["hi:cut_in_fast" if fast else "hi:cut_in_place"] += 1
    if counts is not None:
        if more:
            counts["more:raw_at_limit" if mode == RAW else "more:live"] += 1
        elif mode == LIVE and skipped_when_full:
            counts["live:tombstone_tail_more0"] += 1
    return out, more


@functools.lru_cache(maxsize=None)
def compared(name):
    """The reference against the walk over every mode, limit and range of the
    case -> (entries emitted, the census of the walk's paths)."""
    case = cases.CASES[name]()
    tree, ref = case.tree, case.tree.ref
    assert ref.absent == 0          # a present key answered GET_ABSENT would hide a failure
    tabs = plain_tables(tree)
    emitted, counts = 0, collections.Counter()
    for mode in (RAW, LIVE):
        for limit in case.limits:
            for lo, hi, nu in case.ranges:
                idx, more = ref.scan(lo, hi, nu, limit, mode)
                got, gmore = walk(tree, tabs, lo, hi, nu, limit, mode, counts)
                assert gmore == more and len(got) == len(idx), (name, mode, limit, lo, hi, nu)
                for i, (k, tid, res, view, rec_off, key_len) in zip(idx, got):
                    assert ref.keys[i] == k and ref.table[i] == tid and ref.res[i] == res
                    assert ref.koff[i] == int(tree.offs[tid]) + rec_off and ref.klen[i] == key_len
                    if view:
                        assert ref.voff[i] == int(tree.offs[tid]) + view[0] and ref.vlen[i] == view[1]
                    else:
                        assert ref.voff[i] == 0 and ref.vlen[i] == 0
                emitted += len(got)
    return emitted, counts


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_reference_matches_the_iterator_walk(name):
    emitted, _ = compared(name)
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


# (case, path, "==" | ">=", count): the census of the walk over every mode,
# limit and range of the case.  Exact counts, so that an edit of a case shows
# here; ">=" for a maximum over the steps.  A path a case must not reach is 0.
COVERAGE = [
    # the width of the minimum: rows of 16 lanes, rounds of 64
    ("width_16", "winner:row0", "==", 418),
    ("width_16", "winner:row1", "==", 0),        # 16 sources: lanes >= 16 hold nothing
    ("width_16", "winner:row2", "==", 0),
    ("width_16", "winner:row3", "==", 0),
    ("width_17", "winner:row1", "==", 45),       # source 16, level 6, answers alone
    ("width_17", "winner:row2", "==", 0),
    ("width_64", "winner:row0", "==", 309),
    ("width_64", "winner:row1", "==", 117),
    ("width_64", "winner:row2", "==", 28),
    ("width_64", "winner:row3", "==", 7),
    ("width_64", "winner:round1", "==", 0),
    ("width_64", "lane_tie:two_rounds", "==", 0),
    ("width_64", "advance:sources:max", ">=", 17),
    ("width_65", "winner:round0", "==", 452),
    ("width_65", "winner:round1", "==", 13),     # level 6, alone in the second round
    ("width_65", "winner:round2", "==", 0),
    ("width_65", "lane_tie:two_rounds", "==", 34),
    ("width_65", "advance:sources:max", ">=", 17),
    ("wide_3rounds", "winner:round1", "==", 6),
    ("wide_3rounds", "winner:round2", "==", 18),
    ("wide_3rounds", "lane_tie:two_rounds", "==", 4),
    ("wide_3rounds", "advance:sources:max", ">=", 81),
    ("wide_level0", "winner:round2", "==", 0),
    # the advance: the register path's fast one, place() and its seams
    ("width_16", "advance:fast", "==", 825),
    ("width_16", "advance:place", "==", 301),
    ("width_64", "advance:fast", "==", 1792),
    ("width_64", "advance:place", "==", 966),
    ("width_64", "place:hop", "==", 1213),
    ("width_64", "place:boundary", "==", 34),
    ("width_64", "hi:cut_in_fast", "==", 126),
    ("width_64", "hi:cut_in_place", "==", 99),
    ("width_65", "advance:fast", "==", 0),       # the workspace path has none
    ("width_65", "advance:place", "==", 2811),
    ("width_65", "place:hop", "==", 1186),
    ("width_65", "place:boundary", "==", 30),
    ("width_65", "hi:cut_in_place", "==", 202),
    ("wide_3rounds", "advance:fast", "==", 0),
    ("wide_3rounds", "hi:cut_in_place", "==", 94),
    # tables that do not take part
    ("damaged", "seek:picked_nonparticipating", "==", 66),
    ("damaged", "place:skip_nonparticipating", "==", 28),
    ("damaged", "place:skip_nonparticipating_to_the_end", "==", 16),
    ("damaged", "place:boundary", "==", 4),      # into a stage-5 table
    ("damaged", "value_error:registers", "==", 34),   # the damaged record's own value
    ("mixed", "seek:picked_nonparticipating", "==", 0),
    ("width_64", "place:skip_nonparticipating", "==", 0),
    # equal prefixes
    ("width_64", "tie:by_length", "==", 27),
    ("width_64", "tie:tail", "==", 252),
    ("width_64", "tie:tail_lead_moves:max", ">=", 2),
    ("width_64", "key:ff_prefix", "==", 45),
    ("width_65", "tie:by_length", "==", 27),
    ("width_65", "tie:tail", "==", 257),
    ("width_65", "wide:lane_cmp_tail", "==", 95),
    ("width_65", "wide:advance_cmp_tail", "==", 9474),
    ("width_65", "key:ff_prefix", "==", 46),
    ("wide_3rounds", "tie:tail", "==", 21),
    ("wide_3rounds", "tie:tail_lead_moves:max", ">=", 2),
    ("wide_3rounds", "wide:lane_cmp_tail", "==", 508),
    ("wide_level0", "tie:tail", "==", 0),        # what the workspace path saw before these cases
    ("wide_level0", "wide:lane_cmp_tail", "==", 0),
    ("wide_level0", "live:skipped", "==", 0),
    ("wide_level0", "value_error:wide", "==", 0),
    # modes and values
    ("width_64", "live:skipped", "==", 43),
    ("width_65", "live:skipped", "==", 42),
    ("width_65", "more:raw_at_limit", "==", 12),
    ("width_65", "more:live", "==", 11),
    ("width_65", "value_error:wide", "==", 14),
    ("wide_3rounds", "live:skipped", "==", 17),
    ("wide_3rounds", "more:raw_at_limit", "==", 6),
    ("wide_3rounds", "more:live", "==", 4),
    ("wide_3rounds", "live:tombstone_tail_more0", "==", 1),
]


@pytest.mark.parametrize("name,path,op,count", COVERAGE,
                         ids=["%s-%s" % (c, p.replace(":", "_")) for c, p, _, _ in COVERAGE])
def test_coverage(name, path, op, count):
    counts = compared(name)[1]
    got = counts[path]
    assert got == count if op == "==" else got >= count, (name, path, got, dict(counts))


def test_fast_advance_meets_every_key_length():
    """width_64's register path forms the next head itself at every key length:
    it advances from keys of 0..17 bytes and to keys of 1..17 bytes (the empty
    key is a table's entry 0, never the entry after another), and past 17."""
    counts = compared("width_64")[1]
    assert all(counts["fast:from_len%d" % n] > 0 for n in range(19))
    assert all(counts["fast:to_len%d" % n] > 0 for n in range(1, 19))
    assert counts["fast:to_len0"] == 0
    assert sum(v for k, v in counts.items() if k.startswith("fast:to_len")) == counts["advance:fast"]


def test_what_the_new_cases_hold():
    """The properties the width, wide and damaged cases are built around."""
    for name, n0 in (("width_16", 10), ("width_17", 11), ("width_64", 58), ("width_65", 59),
                     ("wide_3rounds", 123)):
        tree = cases.CASES[name]().tree
        ls = tree.level_start
        assert int(ls[1]) == n0
        if name != "wide_3rounds":
            assert [int(ls[L + 1] - ls[L]) for L in range(1, cases.LEVELS)] == [3] * 6   # level 6 included
            frac = tree.ref.tomb.mean()
            assert 0.1 < frac < 0.4, frac
    assert set(cases.POOL) >= set(cases.LENGTHS) and len(cases.LENGTHS) >= 20
    for name in ("width_64", "width_65"):
        tree = cases.CASES[name]().tree
        sizes = [int(d[1].nidx) for d in tree.dec]
        assert sizes[3] >= 20 and max(sizes[int(tree.level_start[1]):]) >= 20
    # a key per 16-lane row that one source of the row holds alone
    c = cases.width_64()
    ref = c.tree.ref
    assert [int(ref.table[ref.keys.index(b"row%d" % r)]) for r in range(4)] == list(cases.ROW_TABLES)
    assert [t // 16 for t in cases.ROW_TABLES] == [0, 1, 2, 3]
    # sources 0 and 64 share "lane0"; the patched offsets are answered from level 1
    c = cases.width_65()
    ref = c.tree.ref
    holders = [t for t, d in enumerate(c.tree.dec) if any(
        c.tree.images[t][int(e["rec_off"]) + 4:int(e["rec_off"]) + 4 + int(e["key_len"])].tobytes() == b"lane0"
        for e in d[2])]
    assert holders[0] == 0 and int(c.tree.level_start[6]) <= holders[1] and len(holders) == 2
    assert ref.table[ref.keys.index(b"lane0")] == 0
    assert ref.table[ref.keys.index(b"only6")] >= c.tree.level_start[6]
    assert ref.res[ref.keys.index(b"verr-neg")] == ora.GET_SEEK_FAILED
    assert ref.res[ref.keys.index(b"verr-end")] == ora.GET_VALUE_LENGTH
    # three rounds, one live lane in the last; the tombstone tail
    c = cases.wide_3rounds()
    ref = c.tree.ref
    assert int(c.tree.level_start[1]) + cases.LEVELS - 1 == 2 * WAVE + 1
    assert ref.scan(b"zy", b"zzz", False, 1, RAW) == ([ref.keys.index(b"zy1")], 1)
    assert ref.scan(b"zy", b"zzz", False, 1, LIVE) == ([ref.keys.index(b"zy1")], 0)


def test_damaged_tables():
    """Each table's (stage, nidx) as the oracle decodes it; the scan holds what
    Search answers: the keys of the stage-5 and stage-6 tables, from those
    tables, and none of the keys only a stage-4 table holds."""
    c = cases.damaged()
    tree, ref = c.tree, c.tree.ref
    assert [(int(d[1].stage), int(d[1].nidx)) for d in tree.dec] == cases.DAMAGED_TABLES
    assert ref.absent == 0
    at = {k: i for i, k in enumerate(ref.keys)}
    assert ref.table[at[b"d11"]] == 0                 # the stage-5 table in front of the healthy one
    assert ref.table[at[b"d01"]] == 0 and ref.res[at[b"d01"]] == ora.GET_VALUE_TOO_LONG   # the damaged record
    assert ref.table[at[b"d12"]] == 5                 # the boundary key: the stage-5 table's entry
    assert ref.table[at[b"d21"]] == 5 and ref.table[at[b"d05"]] == 8    # keys only stage-5 tables hold
    assert ref.table[at[b"d60"]] == 9                 # the stage-6 table, over level 4
    assert ref.table[at[b"d42"]] == 10                # the entry the cut indexes lost: level 4's
    for k in (b"c01", b"c02", b"d40", b"d41", b"f00", b"f01", b"f20", b"f21"):
        assert k not in at                            # held by stage-4 tables alone
    only5 = [k for k in ref.keys if ref.table[at[k]] in (0, 3, 5, 8, 9)]
    assert len(only5) >= 10


def test_strides():
    """The tiled batches pass both grid strides, and their patterns mix full,
    partial and empty ranges and lo >= hi, so a head carried over from a
    wave's previous range would change some output."""
    w, s = cases.strides_walk(), cases.strides_seek()
    assert w.nq == 2 * cases.WALK_STRIDE + 37 and s.nq > cases.WALK_STRIDE
    nsrc = int(s.tree.level_start[1]) + cases.LEVELS - 1
    assert nsrc == 76 and cases.SEEK_STRIDE < s.nq * nsrc == 4_202_800
    assert s.nq * nsrc * 32 < 135 << 20
    for t in (w, s):
        for mode in (RAW, LIVE):
            count, more, idx = t.want(mode)
            assert count.shape == (t.nq,) and idx.shape == (t.nq, t.limit)
            q = t.nq - 1                                  # the tiling: range q is pattern entry q % P
            out, m = t.tree.ref.scan(*t.ranges[q], t.limit, mode)
            assert t.ranges[q] == t.pattern[q % len(t.pattern)]
            assert count[q] == len(out) and more[q] == m and list(idx[q, :len(out)]) == out
        count = t.want(RAW)[0][:len(t.pattern)]
        assert (count == t.limit).any() and ((count > 0) & (count < t.limit)).any() and (count == 0).sum() >= 2
        assert any(not nu and lo >= hi for lo, hi, nu in t.pattern)
        assert any(not nu and lo < hi and c == 0 for (lo, hi, nu), c in zip(t.pattern, count))
        # a wave's consecutive ranges differ
        step = cases.WALK_STRIDE % len(t.pattern)
        assert step and all(t.pattern[i] != t.pattern[(i + step) % len(t.pattern)] for i in range(len(t.pattern)))
