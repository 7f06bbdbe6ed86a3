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


CASES = {"mixed": mixed, "shadowing": shadowing, "seams": seams, "keys": keys_case,
         "wide_level0": wide_level0, "value_errors": value_errors, "empty_tree": empty_tree}
