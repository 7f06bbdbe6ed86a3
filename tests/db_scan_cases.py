"""The logs, trees and ranges of the lsm_db_scan tests, built on the host:
shared by tests/test_db_scan_ref.py (the reference against a literal merge of
iterators, CPU) and tests/test_db_scan_gpu.py (the kernels against the
reference).  Logs are memtable_ref.wal_bytes / test_memtable_gpu.rec records,
trees are tree_scan_cases.build images.  Each case is computed once.
"""
import functools

import numpy as np

import db_scan_ref
import tree_scan_cases as tsc
from memtable_ref import TOMBSTONE as TOMB, wal_bytes
from test_memtable_gpu import rec
from tree_scan_cases import LONG, POOL, HostTree, build, empty_levels

LEVELS = tsc.LEVELS


class HostDb:
    """logs: per log (OLDEST FIRST) its records [(key, value)] in append order
    (None: Go's nil, an empty value in the log's bytes).  failed: logs whose
    last record is cut short -- wal.Recover fails, the log has no nodes.
    wal: each log's bytes; ref: the reference's answers over `tree`."""

    def __init__(self, logs, tree, failed=()):
        self.records, self.tree, self.failed = logs, tree, set(failed)
        self.wal = []
        for w, lg in enumerate(logs):
            b = wal_bytes(lg)
            assert b == b"".join(rec(k, b"" if v is None else v) for k, v in lg)
            self.wal.append(b[:-3] if w in self.failed else b)
        self.ref_logs = [None if w in self.failed else [(k, b"" if v is None else v) for k, v in lg]
                         for w, lg in enumerate(logs)]
        self.ref = db_scan_ref.DbRef(self.ref_logs, tree.ref)
        self.nsrc = len(logs) + int(tree.level_start[1]) + LEVELS - 1


class Case:
    def __init__(self, db, ranges, limits, placement="offset", indexed_nodes=None):
        self.db, self.ranges, self.limits = db, ranges, limits
        self.placement = placement          # the replay's placement
        self.indexed_nodes = indexed_nodes  # nnode_max of the memtable index (None: every node)


def small_tree():
    """tree_scan_cases.shadowing's five tables: "s" in four of them, a level-0
    tombstone for "t" over a level-2 value, the tombstones "x1".."x3"."""
    return tsc.shadowing().tree


@functools.lru_cache(maxsize=None)
def node_counts():
    """Logs of 5, 0 (empty), 1, 0 (failed), 2 and 1 nodes, oldest first; the
    last log written twice to the same key."""
    logs = [[(b"n1", b"a"), (b"s", b"log0 s"), (b"n3", b"c"), (b"a0", b"first"), (b"zz", b"last"), (b"n1", b"a2")],
            [],
            [(b"r", b"log2 r")],
            [(b"n3", b"lost"), (b"q", b"lost too")],
            [(b"n3", b"log4 n3"), (b"t0", b"log4 t0")],
            [(b"w1", b"one"), (b"w1", b"two")]]
    ranges = [(b"", b"", True), (b"n", b"o", False), (b"n3", b"s", False), (b"r", b"w1", False),
              (b"zz", b"", True), (b"zz\x00", b"", True), (b"a0", b"a1", False)]
    return Case(HostDb(logs, small_tree(), failed={3}), ranges, (1, 2, 64))


@functools.lru_cache(maxsize=None)
def node_counts_plan():
    """The same logs replayed in the plan placement, the index holding the
    first six nodes only: logs 0 and 2 go through it, logs 4 and 5 do not."""
    c = node_counts()
    return Case(c.db, c.ranges, c.limits, placement="plan", indexed_nodes=6)


@functools.lru_cache(maxsize=None)
def shadowing():
    """Over the small tree.  "s": log 1's tombstone over log 0's value over
    level-0 table 0's.  "t": log 0's value over the level-0 tombstone.  "e": a
    (key, "") node.  "x2": a memtable value over a level-0 tombstone.  "y1"
    live, then the tombstones "y2", "y3" (memtable) and nothing else in ["y",
    "z"): past limit 1 RAW has more, LIVE has none.  "del": Delete's two
    records, nil then the tombstone."""
    logs = [[(b"s", b"mem old"), (b"t", b"mem t"), (b"e", b"x"), (b"y2", b"soon gone"), (b"r", TOMB)],
            [(b"s", TOMB), (b"e", b""), (b"x2", b"mem x2"), (b"y1", b"live"), (b"y3", TOMB), (b"y2", TOMB),
             (b"del", b"v"), (b"del", None), (b"del", TOMB)]]
    ranges = [(b"", b"", True), (b"s", b"u", False), (b"y", b"z", False), (b"e", b"e\x00", False),
              (b"x", b"", True), (b"d", b"f", False), (b"r", b"s", False)]
    return Case(HostDb(logs, small_tree()), ranges, (1, 2, 3, 64))


@functools.lru_cache(maxsize=None)
def keys_case():
    """tree_scan_cases.keys_case's tree (keys that agree in 16 bytes, a proper
    prefix, the empty key) under three logs that hold more of the same: equal
    16-byte prefixes in a memtable and a table (a memtable is the lower source
    of such a tie up to LONG + "C" * 30; from LONG + "D" on only tables hold the
    prefix), the empty key, 0xFF keys, proper prefixes."""
    tree = tsc.keys_case().tree
    logs = [[(LONG + b"A", b"m0 A"), (LONG + b"A\x00", b"m0 A0"), (b"", b"m0 empty"), (b"\xff" * 16, b"ff16"),
             (b"\xff" * 17, b"ff17")],
            [(LONG + b"C", b"m1 C"), (LONG, b"m1 16"), (b"pre", TOMB), (b"\xff" * 15, b"ff15"),
             (LONG + b"C" * 30, TOMB)],
            [(LONG + b"B\x00", b"m2 B0"), (LONG + b"B", b"m2 B"), (b"prefi", b"m2 prefi"), (b"\xff", b"ff1"),
             (LONG[:15], b"m2 15")]]
    ranges = [
        (b"", b"", True),
        (LONG + b"A" * 24, b"", True),          # a 40-byte lo
        (LONG, LONG + b"C", False),             # lo and hi memtable keys: lo included, hi excluded
        (LONG + b"B\x00", LONG + b"C" * 30, False),
        (b"pre", b"prefix", False),
        (b"", b"\x00", False),                  # the empty key alone
        (b"\xff", b"\xff" * 17, False),         # hi a memtable key
        (b"\xff" * 16, b"", True),
        (LONG + b"D", LONG + b"D", False),      # lo == hi
        (b"q", b"p", False),                    # lo > hi
    ]
    return Case(HostDb(logs, tree), ranges, (1, 3, 64))


def pool_logs(rng, nlog, extra=None):
    """nlog logs of 2-5 pool keys each, a quarter of the values tombstones, one
    key in three written twice.  extra: {log: [(key, value)]} appended."""
    logs = []
    for w in range(nlog):
        n = int(rng.integers(2, 6))
        keys = [POOL[i] for i in rng.choice(len(POOL), n, replace=False)]
        lg = [(k, b"old.%d" % w) for k in keys[:n // 3]]
        lg += [(k, TOMB if rng.random() < 0.25 else b"m%d.%d" % (w, j)) for j, k in enumerate(keys)]
        logs.append(lg + (extra or {}).get(w, []))
    return logs


WIDTH_RANGES = [
    (b"", b"", True),
    (LONG[:8], LONG + b"20x", False),
    (LONG + b"30" + b"\x00" * 22, b"", True),
    (b"\xff" * 16, b"\xff" * 18, False),
    (b"X", b"Y", False),
    (b"zz", b"a", False),
    (b"l", b"p", False),                                # "lone1" (level 1), "many", "only6" (level 6)
]


def width_case(seed, nlog, n0, limits=(1, 3, 64), per=5, draws=tsc.LEVEL_DRAWS, indexed_nodes=None):
    """nlog logs over a tree of n0 level-0 tables and six levels: nlog + n0 + 6
    sources.  "many" is in every third log and every fourth level-0 table;
    "lone1" and "only6" are held by level 1 and level 6 alone."""
    rng = np.random.default_rng(seed)
    tree = tsc.width_case(seed, n0, per=per, extra0=tsc.with_many({}, range(0, n0, 4)), draws=draws,
                          extra_level={1: [(b"lone1", b"one")], 6: [(b"only6", b"six")]}, limits=limits).tree
    logs = pool_logs(rng, nlog, extra={w: [(b"many", b"many.%d" % w)] for w in range(0, nlog, 3)})
    db = HostDb(logs, tree)
    assert db.nsrc == nlog + n0 + 6
    return Case(db, WIDTH_RANGES, limits, indexed_nodes=indexed_nodes)


@functools.lru_cache(maxsize=None)
def width_16():
    """16 sources: the widest scan that takes the first row's four shifts alone."""
    return width_case(520, 3, 7)


@functools.lru_cache(maxsize=None)
def width_17():
    """17 sources: the full 64-lane minimum."""
    return width_case(521, 3, 8)


@functools.lru_cache(maxsize=None)
def width_64():
    """64 sources, 11 memtables + 47 level-0 tables: every lane of the register path live."""
    return width_case(522, 11, 47, indexed_nodes=20)


@functools.lru_cache(maxsize=None)
def width_65():
    """65 sources, 11 memtables + 48 level-0 tables: the workspace path, level 6
    alone in the second round."""
    return width_case(523, 11, 48, indexed_nodes=20)


@functools.lru_cache(maxsize=None)
def wide_134():
    """134 sources with 70 logs: memtable lanes fill round 0 and spill into
    round 1, the tree's sources sit in rounds 1-2."""
    return width_case(524, 70, 58, limits=(1, 5), per=2, draws=(9, 0, 12, 0, 0, 6))


@functools.lru_cache(maxsize=None)
def tree_alone():
    """nlog == 0 over tree_scan_cases.mixed."""
    c = tsc.mixed()
    return Case(HostDb([], c.tree), c.ranges, (1, 7, 64))


@functools.lru_cache(maxsize=None)
def logs_alone():
    """An empty tree under three logs: the batched memtable range query."""
    logs = [[(b"a", b"0"), (b"c", b"0"), (b"e", TOMB)], [(b"b", b"1"), (b"c", TOMB)], [(b"a", b"2"), (b"d", b"2")]]
    ranges = [(b"", b"", True), (b"b", b"e", False), (b"c", b"c\x00", False), (b"f", b"", True)]
    return Case(HostDb(logs, HostTree(530, empty_levels())), ranges, (1, 2, 64))


@functools.lru_cache(maxsize=None)
def both_empty():
    return Case(HostDb([], HostTree(531, empty_levels())), [(b"", b"", True), (b"a", b"b", False)], (4,))


CASES = {"node_counts": node_counts, "node_counts_plan": node_counts_plan, "shadowing": shadowing,
         "keys": keys_case, "width_16": width_16, "width_17": width_17, "width_64": width_64,
         "width_65": width_65, "wide_134": wide_134, "tree_alone": tree_alone, "logs_alone": logs_alone,
         "both_empty": both_empty}


class Tiled:
    """A pattern of P <= 64 distinct ranges repeated to nq (tree_scan_cases.Tiled,
    over a HostDb)."""

    def __init__(self, db, pattern, nq, limit):
        assert len(set(pattern)) == len(pattern) <= 64 and tsc.WALK_STRIDE % len(pattern)
        self.db, self.pattern, self.nq, self.limit = db, pattern, nq, limit
        self.ranges = [pattern[q % len(pattern)] for q in range(nq)]

    def want(self, mode):
        count, more, idx = self.db.ref.scan_batch(self.pattern, self.limit, mode)
        at = np.arange(self.nq) % len(self.pattern)
        return count[at], more[at], idx[at]


@functools.lru_cache(maxsize=None)
def strides():
    """Three small logs over the small tree: each wave of the walk takes three
    ranges, the last pass is ragged."""
    c = shadowing()
    logs = c.db.records + [[(b"w2", b"newest w2"), (b"x1", b"newest x1")]]
    pattern = c.ranges + [(b"w", b"x", False), (b"a", b"b", False), (b"u", b"t", False)]
    return Tiled(HostDb(logs, small_tree()), pattern, tsc.WALK_STRIDE * 2 + 37, 2)
