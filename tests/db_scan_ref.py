"""The reference answer of lsm_db_scan, in its short form: the scan of a range
is, for every distinct key any source holds in [lo, hi), lsm_memtable_search's
answer when that is not MISS (memtable_search_ref.search: per log a dict of
last positions, walked newest first), else lsm_search's (tree_scan_ref.TreeRef)
-- then the range, the mode and the limit.
tests/test_db_scan_ref.py pins this against a literal k-way merge of iterators
(the restated skiplists newest first, then the tables' Source walk).
Logs are listed OLDEST FIRST; a log without nodes is None.
"""
import bisect

import numpy as np

import memtable_search_ref as msr
from memtable_ref import TOMBSTONE
from tree_scan_ref import LIVE, RAW  # noqa: F401

SRC_MEMTABLE, SRC_SSTABLE = msr.SRC_MEMTABLE, msr.SRC_SSTABLE


class DbRef:
    """The answer for every key the memtables and the tree hold, computed once.
    keys: the distinct keys, sorted.  Per key: src (SRC_MEMTABLE / SRC_SSTABLE);
    for a memtable's answer log and pos (the record's position in that log);
    for a table's answer tree (the key's index in tree_ref.keys); tomb: the
    answering entry is a tombstone."""

    def __init__(self, logs, tree_ref):
        self.logs, self.tree_ref = logs, tree_ref
        self.tables = [None if lg is None else msr.last_positions(lg) for lg in logs]
        mem_keys = set().union(*[t for t in self.tables if t is not None]) if logs else set()
        self.keys = sorted(mem_keys | set(tree_ref.keys))
        n = len(self.keys)
        self.src = np.zeros(n, np.int32)
        self.log = np.full(n, -1, np.int64)
        self.pos = np.full(n, -1, np.int64)
        self.tree = np.full(n, -1, np.int64)
        self.tomb = np.zeros(n, bool)
        tree_at = {k: i for i, k in enumerate(tree_ref.keys)}
        for i, k in enumerate(self.keys):
            res, w, pos, _ = msr.search(logs, k, self.tables)
            if res != msr.MISS:
                self.src[i], self.log[i], self.pos[i] = SRC_MEMTABLE, w, pos
                self.tomb[i] = res == msr.DELETED
            else:
                self.src[i], self.tree[i] = SRC_SSTABLE, tree_at[k]
                self.tomb[i] = tree_ref.tomb[tree_at[k]]
        self.absent = tree_ref.absent

    def value(self, i, tree_buf):
        """The answering entry's value bytes (None for a table's error code)."""
        if self.src[i] == SRC_MEMTABLE:
            v = self.logs[int(self.log[i])][int(self.pos[i])][1]
            return b"" if v is None else bytes(v)
        t, r = int(self.tree[i]), self.tree_ref
        if r.vlen[t] == 0 and r.voff[t] == 0:
            return None
        at = int(r.voff[t]) + 4
        return tree_buf[at:at + int(r.vlen[t])].tobytes()

    def scan(self, lo, hi, no_upper, limit, mode):
        """-> (indices into keys of the emitted entries, more)."""
        a = bisect.bisect_left(self.keys, lo)
        b = len(self.keys) if no_upper else bisect.bisect_left(self.keys, hi)
        out, more = [], 0
        for i in range(a, b):
            if mode == LIVE and self.tomb[i]:
                continue
            if len(out) == limit:
                more = 1
                break
            out.append(i)
        return out, more

    def scan_batch(self, ranges, limit, mode):
        """ranges: [(lo, hi, no_upper)] -> count uint32[nq], more uint8[nq] and
        idx int64[nq, limit] into keys, -1 past count."""
        nq = len(ranges)
        count = np.zeros(nq, np.uint32)
        more = np.zeros(nq, np.uint8)
        idx = np.full((nq, limit), -1, np.int64)
        for q, (lo, hi, nu) in enumerate(ranges):
            out, more[q] = self.scan(lo, hi, nu, limit, mode)
            count[q] = len(out)
            idx[q, :len(out)] = out
        return count, more, idx


assert TOMBSTONE == msr.TOMBSTONE
