"""The trees and ranges of the lsm_tree_scan tests, built on the host with the
oracle's .sst builder: shared by tests/test_tree_scan_ref.py (the reference
against a restatement of the iterator walk, CPU) and tests/test_tree_scan_gpu.py
(the kernel against the reference).  Each case is computed once.
"""
import functools

import numpy as np

import pyoracle as ora
import search_ref
import tree_scan_ref
from search_ref import csr

LEVELS = search_ref.LEVELS
TOMB = tree_scan_ref.TOMBSTONE


def build(keys, vals, m=4096, k=4):
    kb, ko = csr(keys)
    vb, vo = csr(vals)
    img, _ = ora.build_sst(kb if kb.size else np.zeros(1, np.uint8), ko,
                           vb if vb.size else np.zeros(1, np.uint8), vo, 0, len(keys), m=m, k=k)
    return img.copy()


def patch_offset(img, j, off):
    """Index entry j's value offset := off (as tests/test_search_gpu.py patches)."""
    _, _, idesc, _, _ = ora.sst_decode(img)
    at = int(idesc["rec_off"][j]) + 4 + int(idesc["key_len"][j])
    img[at:at + 8] = np.frombuffer(int(off).to_bytes(8, "little", signed=True), np.uint8)


class HostTree:
    """levels: LEVELS lists of images -> one buffer (random gaps between the
    images), the oracle's decode and the reference's answers."""

    def __init__(self, seed, levels):
        assert len(levels) == LEVELS
        rng = np.random.default_rng(seed)
        self.images = [im for lv in levels for im in lv]
        self.level_start = search_ref.level_starts([len(lv) for lv in levels])
        offs, pos, parts = [], 0, []
        for im in self.images:
            gap = int(rng.integers(0, 23))
            parts += [np.zeros(gap, np.uint8), im]
            pos += gap
            offs.append(pos)
            pos += im.size
        self.buf = np.concatenate(parts + [np.zeros(16, np.uint8)])
        self.offs = np.array(offs, np.uint64)
        self.lens = np.array([im.size for im in self.images], np.uint64)
        self.dec = [ora.sst_decode(im) for im in self.images]
        self.ref = tree_scan_ref.TreeRef(self.buf, self.offs, self.lens, self.dec, self.level_start)


class Case:
    def __init__(self, tree, ranges, limits):
        self.tree, self.ranges, self.limits = tree, ranges, limits


def empty_levels():
    return [[] for _ in range(LEVELS)]


ALL_KEYS = [b"key%05d" % i for i in range(4000)]
MIXED_COUNTS = (2, 3, 5, 0, 2, 1, 0)


def mixed_levels(rng, counts=MIXED_COUNTS, per=300):
    """tests/test_search_gpu.py's recipe: `per` random ids of the 4,000 per
    table; a level >= 1 is one sorted draw cut into disjoint tables; two filter
    shapes alternate."""
    levels, t = [], 0
    for L, c in enumerate(counts):
        if L == 0:
            sets = [sorted(rng.choice(4000, per, replace=False).tolist()) for _ in range(c)]
        else:
            ids = sorted(rng.choice(4000, per * c, replace=False).tolist())
            sets = [ids[j * per:(j + 1) * per] for j in range(c)]
        lv = []
        for s in sets:
            m, k = (256, 2) if t % 2 == 0 else (16384, 6)
            lv.append(build([ALL_KEYS[i] for i in s], [b"L%d.t%d.%d" % (L, t, i) for i in s], m=m, k=k))
            t += 1
        levels.append(lv)
    return levels


@functools.lru_cache(maxsize=None)
def mixed():
    tree = HostTree(501, mixed_levels(np.random.default_rng(501)))
    keys = tree.ref.keys
    have = keys[len(keys) // 3]
    gone = next(k for k in ALL_KEYS[1500:] if k not in set(keys))  # between two keys of the tree
    ranges = [
        (b"", b"\xff", False),              # the whole space
        (b"key01000", b"", True),           # no upper bound, hi ignored
        (have, have, False),                # lo == hi
        (b"key03000", b"key02000", False),  # lo > hi
        (have, b"key9", False),             # lo an existing key
        (gone, b"key9", False),             # lo between keys
        (b"a", b"key00100", False),         # lo below all
        (b"zzz", b"", True),                # above all
        (b"key00000", have, False),         # hi an existing key: excluded
        (b"", keys[5], False),              # lo = ""
    ]
    return Case(tree, ranges, (1, 7, 64, 4096))


@functools.lru_cache(maxsize=None)
def many_ranges():
    """5,000 random ranges over the mixed tree."""
    tree = mixed().tree
    rng = np.random.default_rng(502)
    ranges = []
    for _ in range(5000):
        a, b = sorted(rng.integers(0, 4000, 2).tolist())
        lo = ALL_KEYS[a] + (b"\x00" if rng.random() < 0.2 else b"")
        kind = rng.random()
        if kind < 0.3:
            ranges.append((lo, b"", True))
        elif kind < 0.4:
            ranges.append((ALL_KEYS[b], ALL_KEYS[a], False))  # lo >= hi
        else:
            ranges.append((lo, ALL_KEYS[min(b, a + int(rng.integers(0, 40)))], False))
    return Case(tree, ranges, (8,))


@functools.lru_cache(maxsize=None)
def shadowing():
    """"s" in level-0 table 0, level-0 table 1, level 1 and level 3; a level-0
    tombstone for "t" over a value in level 2; "x1".."x3": tombstones after the
    live "w1", "w2"."""
    lv = empty_levels()
    lv[0] = [build([b"s", b"t", b"x2"], [b"zero-a", TOMB, TOMB]), build([b"s", b"w1"], [b"zero-b", b"w1.0"])]
    lv[1] = [build([b"s", b"w2", b"x1"], [b"one", b"w2.1", TOMB])]
    lv[2] = [build([b"t", b"x3"], [b"live", TOMB])]
    lv[3] = [build([b"r", b"s", b"x2"], [b"r3", b"three", b"x2 hidden"])]
    ranges = [(b"", b"", True), (b"s", b"u", False), (b"t", b"t\x00", False), (b"w", b"z", False),
              (b"x", b"", True)]
    return Case(HostTree(503, lv), ranges, (1, 2, 3, 64))


@functools.lru_cache(maxsize=None)
def seams():
    """Level 1: four tables with gaps, one of a single entry.  Level 2: two
    tables sharing the boundary key "m9" with different values, and a chain of
    one-entry tables that share their key."""
    lv = empty_levels()
    lv[1] = [build([b"a1", b"a3", b"a5"], [b"1", b"3", b"5"]), build([b"c1", b"c3"], [b"c1", b"c3"]),
             build([b"e1"], [b"only"]), build([b"g1", b"g2", b"g3"], [b"g1", b"g2", b"g3"])]
    lv[2] = [build([b"m1", b"m5", b"m9"], [b"m1", b"m5", b"first table"]),
             build([b"m9", b"n1"], [b"second table", b"n1"]),
             build([b"n1"], [b"n1 again"]), build([b"n1", b"n2"], [b"n1 third", b"n2"])]
    ranges = [
        (b"b", b"", True),        # lo in the gap between two tables
        (b"a5", b"", True),       # lo equal to a table's MaxKey
        (b"a3", b"g2", False),    # spanning three tables (and into a fourth)
        (b"e0", b"e2", False),    # the one-entry table
        (b"d", b"f", False),
        (b"m5", b"n0", False),    # across the boundary key
        (b"m9", b"", True),       # lo the boundary key
        (b"", b"", True),
        (b"g3\x00", b"m1", False),  # nothing between the levels' keys
    ]
    return Case(HostTree(504, lv), ranges, (1, 2, 64))


LONG = b"0123456789abcdef"  # 16 bytes


@functools.lru_cache(maxsize=None)
def keys_case():
    """Keys that agree in their first 16 bytes, in one source and across
    sources; a key that is a proper prefix of the next; the empty key."""
    lv = empty_levels()
    lv[0] = [build([b"", LONG + b"B", LONG + b"D", b"pre", b"pre\x00"], [b"empty", b"B0", b"D0", b"p", b"p0"]),
             build([LONG, LONG + b"A", LONG + b"D", b"prefix"], [b"16", b"A1", b"D1", b"px"])]
    lv[1] = [build([LONG + b"A", LONG + b"C", LONG + b"D\x00"], [b"A2", b"C2", b"D02"])]
    lv[2] = [build([b"", LONG[:15], LONG + b"C" * 30, b"pre\x00\x00"], [b"empty2", b"15", b"long", b"p00"])]
    ranges = [
        (b"", b"", True),
        (LONG + b"A" * 24, b"", True),          # a 40-byte lo
        (LONG, LONG + b"D", False),
        (LONG + b"B", LONG + b"C" * 30, False),
        (b"pre", b"prefix", False),
        (b"", b"\x00", False),                  # the empty key alone
        (b"\x00", LONG, False),
    ]
    return Case(HostTree(505, lv), ranges, (1, 3, 64))


@functools.lru_cache(maxsize=None)
def wide_level0():
    """70 level-0 tables of three overlapping keys each, over one level-1 table."""
    lv = empty_levels()
    lv[0] = [build([b"w%03d" % (t + j) for j in range(3)], [b"%d.%d" % (t, j) for j in range(3)], m=64, k=1)
             for t in range(70)]
    lv[1] = [build([b"w%03d" % i for i in range(0, 80, 7)], [b"deep%d" % i for i in range(0, 80, 7)])]
    ranges = [(b"", b"", True), (b"w010", b"w020", False), (b"w069", b"", True), (b"w0305", b"w031", False),
              (b"w072", b"w0777", False)]
    return Case(HostTree(506, lv), ranges, (1, 5, 128))


@functools.lru_cache(maxsize=None)
def value_errors():
    """A level-1 table with one value offset patched negative and one patched
    to the file's end; the same keys live at level 2."""
    keys = [b"e%02d" % i for i in range(12)]
    im1 = build(keys, [b"one%d" % i for i in range(12)])
    patch_offset(im1, 3, -5)
    patch_offset(im1, 7, im1.size)
    lv = empty_levels()
    lv[1] = [im1]
    lv[2] = [build(keys, [b"two%d" % i for i in range(12)])]
    return Case(HostTree(507, lv), [(b"", b"", True), (b"e03", b"e08", False)], (2, 64))


@functools.lru_cache(maxsize=None)
def empty_tree():
    return Case(HostTree(508, empty_levels()), [(b"", b"", True), (b"a", b"b", False)], (4,))


# ---- one case per path of the walk ------------------------------------------
# tests/test_tree_scan_ref.py counts, per case, the paths a step takes (its
# COVERAGE table), so that an edit here cannot silently lose one.

STEM = b"Wxyz123456789"


def key_pool():
    """The keys of the width and wide cases, sorted and distinct: every length
    0..16 of one 16-byte prefix; keys whose zero-padded prefixes are equal
    ("" , "\\0", "\\0\\0"); 40 keys and a 46-byte one that agree in their first
    16 bytes; 0xFF keys, whose prefix words equal the minimum reduction's "no
    candidate" value, around 16 bytes; and per prefix word a pair of keys that
    first differ inside it (bytes 1, 5, 9, 13)."""
    keys = [LONG[:k] for k in range(17)] + [b"\x00", b"\x00\x00"]
    keys += [LONG + b"%02d" % i for i in range(40)] + [LONG + b"C" * 30]
    keys += [b"\xff" * 15, b"\xff" * 16, b"\xff" * 16 + b"\x00", b"\xff" * 17, b"\xff" * 18, b"\xff" * 19]
    for at in (1, 5, 9, 13):
        keys += [STEM[:at] + b"a", STEM[:at] + b"b"]
    assert len(set(keys)) == len(keys)
    return sorted(keys)


POOL = key_pool()
# one table of these meets the fast advance at every key length 0..17, at the
# keys that share 16 bytes and at the 0xFF keys (its last two entries take place())
LENGTHS = sorted([LONG[:k] for k in range(17)] + [b"\x00", b"\x00\x00", LONG + b"00", LONG + b"07"] +
                 [k for k in POOL if k[:1] == b"\xff"])
LEVEL_DRAWS = (9, 12, 15, 21, 30, 66)   # pool keys of levels 1..6, each cut into three tables


def some_values(rng, tag, keys, tombs=0.25):
    return [TOMB if rng.random() < tombs else b"%s.%d" % (tag, j) for j in range(len(keys))]


def cut3(keys):
    """A level's sorted keys as three tables; the first two share a boundary
    key (the second table's entry answers), the last two do not."""
    a, b = len(keys) // 3, 2 * len(keys) // 3
    return [keys[:a + 1], keys[a:b], keys[b:]]


def width_case(seed, n0, per=5, big_table=None, extra0=None, extra_level=None, patch=None, draws=LEVEL_DRAWS,
               limits=(1, 3, 64), ranges=None):
    """n0 level-0 tables of `per` pool keys, every level 1..6 three tables of a
    sorted draw; about a quarter of the values are tombstones.  big_table: the
    level-0 table that holds LENGTHS.  extra0: {level-0 table: [key]} and
    extra_level: {level: [(key, value)]}: keys outside the pool, held where a
    case needs them.  patch: [(level, key, value offset or None for the file's
    end)] applied with patch_offset."""
    rng = np.random.default_rng(seed)
    extra0, extra_level = extra0 or {}, extra_level or {}
    lv = empty_levels()
    for t in range(n0):
        keys = LENGTHS if t == big_table else [POOL[i] for i in rng.choice(len(POOL), per, replace=False)]
        keys = sorted(set(keys) | set(extra0.get(t, [])))
        lv[0].append(build(keys, some_values(rng, b"t%d" % t, keys), m=64, k=1))
    boundary = None
    for L in range(1, LEVELS):
        if not draws[L - 1] and L not in extra_level:
            continue
        forced = dict(extra_level.get(L, []))
        keys = sorted(set(POOL[i] for i in rng.choice(len(POOL), draws[L - 1], replace=False)) | set(forced))
        tabs = cut3(keys)
        boundary = tabs[1][0]
        for j, tk in enumerate(tabs):
            vals = [forced.get(k, v) for k, v in zip(tk, some_values(rng, b"L%d.%d" % (L, j), tk))]
            im = build(tk, vals, m=64, k=1)
            for pl, pk, off in patch or []:
                if pl == L and pk in tk:
                    patch_offset(im, tk.index(pk), im.size if off is None else off)
            lv[L].append(im)
    if ranges is None:
        ranges = [
            (b"", b"", True),                                   # the whole space
            (LONG[:8], LONG + b"20x", False),                   # hi shares 16 bytes with the keys and is longer
            (LONG + b"30" + b"\x00" * 22, b"", True),           # a 40-byte lo
            (b"\xff" * 16, b"\xff" * 18, False),                # inside the 0xFF keys
            (boundary, b"", True),                              # lo = the deepest level's boundary key
            (b"X", b"Y", False),                                # lo < hi, nothing between
            (b"zz", b"a", False),                               # lo > hi
            (b"l", b"w", False),                                # the keys outside the pool
        ]
    return Case(HostTree(seed, lv), ranges, limits)


@functools.lru_cache(maxsize=None)
def width_16():
    """16 sources: the widest tree that takes the first row's four shifts alone."""
    return width_case(510, 10)


@functools.lru_cache(maxsize=None)
def width_17():
    """17 sources: the full 64-lane minimum, source 16 (level 6) in the second row."""
    return width_case(511, 11)


ROW_TABLES = (5, 21, 37, 53)


def with_many(extra0, tables):
    """"many" in each of `tables` (level 0): one step advances all of them."""
    for t in tables:
        extra0.setdefault(t, []).append(b"many")
    return extra0


@functools.lru_cache(maxsize=None)
def width_64():
    """64 sources, every lane of the register path live.  "row0".."row3" are
    each held by one level-0 table of that 16-lane row and by nothing else;
    "many" by the 26 tables 20..45."""
    return width_case(512, 58, big_table=3,
                      extra0=with_many({t: [b"row%d" % r] for r, t in enumerate(ROW_TABLES)}, range(20, 46)))


@functools.lru_cache(maxsize=None)
def width_65():
    """65 sources: the workspace path with level 6 alone in the second round,
    in lane 0 beside level-0 table 0.  "lane0" is held by those two only,
    "only6" by level 6 alone, "many" by the 26 level-0 tables 20..45; two
    level-1 entries that nothing above holds have their value offsets patched
    (negative; the file's end)."""
    return width_case(513, 59, big_table=3, extra0=with_many({0: [b"lane0"]}, range(20, 46)),
                      extra_level={6: [(b"lane0", b"deep lane0"), (b"only6", b"six")],
                                   1: [(b"verr-end", b"e"), (b"verr-neg", b"n")]},
                      patch=[(1, b"verr-neg", -5), (1, b"verr-end", None)])


@functools.lru_cache(maxsize=None)
def wide_3rounds():
    """129 sources, three rounds, level 6 alone in the last one.  Level 6 ends
    in "zy1" (live) and the tombstones "zz1".."zz3", which nothing else holds:
    past limit 1 of ["zy", "zzz") RAW has more, LIVE has none.  "many" is held
    by the 81 level-0 tables 30..110, in all three rounds of 17 lanes."""
    tail = [(b"zy1", b"live")] + [(b"zz%d" % i, TOMB) for i in (1, 2, 3)]
    ranges = [(b"", b"", True), (b"zy", b"zzz", False), (b"\xff" * 16, b"\xff" * 18, False),
              (LONG, LONG + b"2", False), (b"X", b"Y", False), (b"m", b"n", False)]
    return width_case(514, 123, per=2, extra0=with_many({}, range(30, 111)), extra_level={6: tail},
                      draws=(9, 0, 12, 0, 0, 6), limits=(1, 5), ranges=ranges)


def damage_data(img):
    """The first data record's length field := 0x7fffffff: DecodeDataBlock
    fails (stage 5), DecodeFrom does not read it; every index entry is kept."""
    at = int(ora.sst_decode(img)[1].data_off)
    img[at:at + 4] = np.frombuffer((0x7FFFFFFF).to_bytes(4, "little"), np.uint8)
    return img


def cut_index(img):
    """The footer's index size minus 3: the IndexBlock's last record is cut,
    DecodeFrom fails (stage 4); the entries before it are kept by the decode
    and belong to no table Go holds."""
    foot = img[-32:].view(np.int64).copy()
    foot[3] -= 3
    img[-32:] = foot.view(np.uint8)
    return img


def drop_last_value(img):
    """The footer's data size shrunk to the last record's start: one value
    fewer than index entries (stage 6, GetKeyValuePairs' mismatch)."""
    d = ora.sst_decode(img)
    foot = img[-32:].view(np.int64).copy()
    foot[1] = int(d[4]["rec_off"][-1]) - int(d[1].data_off)
    img[-32:] = foot.view(np.uint8)
    return img


# per table of `damaged`, in the tree's order: (stage, nidx)
DAMAGED_TABLES = [(5, 3), (0, 2), (4, 2),
                  (5, 3), (0, 3), (5, 3), (0, 3), (4, 2),
                  (5, 2),
                  (6, 3),
                  (0, 7),
                  (4, 2), (0, 2), (4, 2), (0, 2)]


@functools.lru_cache(maxsize=None)
def damaged():
    """Tables whose data block is damaged (stages 5 and 6: Go loads them,
    Search answers from them, they take part) among tables whose index is cut
    (stage 4: in no Manager, they stay out) and healthy ones.  A cut index
    loses its last entry; the healthy level 4 holds those lost keys and keys of
    the stage-5 tables.  Level 5 starts with a stage-4 table and has one between
    two healthy ones: a Seek the sparse index sends there goes on at the next
    table's entry 0, and the walk hops over it."""
    def tab(keys, tag):
        return build(keys, [b"%s.%d" % (tag, j) for j in range(len(keys))], m=64, k=1)
    lv = empty_levels()
    lv[0] = [damage_data(tab([b"d01", b"d11", b"d31"], b"z0")),      # answers d11 over the next table
             tab([b"d11", b"d50"], b"z1"),
             cut_index(tab([b"c01", b"c02", b"d42"], b"z2"))]
    lv[1] = [damage_data(tab([b"d00", b"d01", b"d02"], b"a0")),
             tab([b"d10", b"d11", b"d12"], b"a1"),
             damage_data(tab([b"d12", b"d21", b"d22"], b"a2")),      # its first key is a1's last
             tab([b"d30", b"d31", b"d32"], b"a3"),
             cut_index(tab([b"d40", b"d41", b"d42"], b"a4"))]
    lv[2] = [damage_data(tab([b"d05", b"d35"], b"b0"))]
    lv[3] = [drop_last_value(tab([b"d02", b"d21", b"d60"], b"c0"))]
    lv[4] = [tab([b"d00", b"d22", b"d35", b"d42", b"d43", b"d60", b"d61"], b"e0")]
    lv[5] = [cut_index(tab([b"f00", b"f01", b"f02"], b"f0")), tab([b"f10", b"f11"], b"f1"),
             cut_index(tab([b"f20", b"f21", b"f22"], b"f2")), tab([b"f30", b"f31"], b"f3")]
    ranges = [
        (b"", b"", True),             # the whole space
        (b"d405", b"", True),         # lo inside the stage-4 table's key range
        (b"d12", b"", True),          # lo = a stage-5 table's first key (the sparse index picks that table)
        (b"d00", b"d21", False),      # ending inside a stage-5 table
        (b"d33", b"", True),          # past everything of level 1 but its last, stage-4, table
        (b"d32", b"d36", False),      # level 1's last participating entry, then off its end
        (b"f01", b"", True),          # level 5: the sparse index picks its first, stage-4, table
        (b"f205", b"f31", False),     # ... and the one between the healthy two
    ]
    return Case(HostTree(515, lv), ranges, (1, 3, 64))


CASES = {"mixed": mixed, "shadowing": shadowing, "seams": seams, "keys": keys_case,
         "wide_level0": wide_level0, "value_errors": value_errors, "empty_tree": empty_tree,
         "width_16": width_16, "width_17": width_17, "width_64": width_64, "width_65": width_65,
         "wide_3rounds": wide_3rounds, "damaged": damaged}


# ---- the grid-stride loops --------------------------------------------------
WALK_STRIDE = 2048 * 4            # ranges one pass of the walk's waves takes
SEEK_STRIDE = 16384 * 256         # (range, source) pairs one pass of the Seeks takes


class Tiled:
    """A pattern of P <= 64 distinct ranges repeated to nq: range q is pattern
    entry q % P.  A wave's next range (q + WALK_STRIDE) is another entry of the
    pattern, so whatever it carried over from the last one would show."""

    def __init__(self, tree, pattern, nq, limit):
        assert len(set(pattern)) == len(pattern) <= 64 and WALK_STRIDE % len(pattern)
        self.tree, self.pattern, self.nq, self.limit = tree, pattern, nq, limit
        self.ranges = [pattern[q % len(pattern)] for q in range(nq)]

    def want(self, mode):
        """The reference's answer for the pattern, tiled -> scan_batch's triple."""
        count, more, idx = self.tree.ref.scan_batch(self.pattern, self.limit, mode)
        at = np.arange(self.nq) % len(self.pattern)
        return count[at], more[at], idx[at]


@functools.lru_cache(maxsize=None)
def strides_walk():
    """Over the mixed tree: each wave of the walk takes three ranges, the last
    pass is ragged."""
    c = mixed()
    one = c.tree.ref.keys[7]
    pattern = c.ranges + [(one, one + b"\x00", False), (b"a", b"b", False)]   # one key; lo < hi over nothing
    return Tiled(c.tree, pattern, WALK_STRIDE * 2 + 37, 2)


@functools.lru_cache(maxsize=None)
def strides_seek():
    """Over wide_level0's 76 sources: 55,300 ranges are 4,202,800 (range,
    source) pairs, just past one pass of the Seeks; the workspace is 134 MB."""
    c = wide_level0()
    pattern = c.ranges + [(b"w0305", b"w0306", False), (b"w050", b"w040", False)]
    return Tiled(c.tree, pattern, 55_300, 2)
