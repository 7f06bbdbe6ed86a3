"""The reference answer of lsm_tree_scan: the scan of a range is Manager.Search
applied to every key the tree holds in that range.  The distinct keys of every
participating table's index entries (ora.sst_decode; takes_part: a stage Go's
DecodeFrom loads -- 0, 5 or 6 -- and nidx > 0) are sorted bytewise and answered once by search_ref.search -- what
tests/test_search_ref.py pins against the Go text -- then a range keeps the
keys in [lo, hi), applies the mode and the limit.
tests/test_tree_scan_ref.py pins this against a restatement of the iterator
walk.
"""
import bisect

import numpy as np

import pyoracle as ora
import search_ref
from search_ref import csr

RAW, LIVE = 0, 1
TOMBSTONE = "～DELETED～".encode()  # kv.DeletedValue, kv/kv.go:29-31
LOADED_STAGES = (0, 5, 6)   # SSTable.DecodeFrom (sstable.go:101-125) does not read the data block


def takes_part(meta):
    """A table Go would have loaded (stages 1-4 are DecodeFrom's failures; 5
    and 6 are damage to the data block, which only compaction reads) that has
    entries: what Manager.Search and sstable.Iterator see."""
    return meta.stage in LOADED_STAGES and meta.nidx > 0


class TreeRef:
    """Search's answer for every key of the tree, computed once.
    keys: the distinct keys, sorted; table / res / voff / vlen: search's answer
    per key; koff / klen: the answering entry's key view in buf (rec_off of the
    entry, as the decode's descriptor holds it) -- 0 where no table answered
    (res == GET_ABSENT, which the tests assert never happens); tomb: the answer
    is GET_FOUND with exactly the tombstone bytes."""

    def __init__(self, buf, offs, lens, dec, level_start):
        entry = []  # per table: key -> (rec_off in buf, key_len)
        for t, d in enumerate(dec):
            meta, idesc = d[1], d[2]
            e = {}
            if takes_part(meta):
                o = int(offs[t])
                for x in idesc:
                    at, kl = o + int(x["rec_off"]), int(x["key_len"])
                    e.setdefault(buf[at + 4:at + 4 + kl].tobytes(), (at, kl))
            entry.append(e)
        self.keys = sorted(set().union(*entry)) if entry else []
        n = len(self.keys)
        kb, ko = csr(self.keys)
        _, self.table, self.res, self.voff, self.vlen, _ = search_ref.search(
            buf, offs, lens, dec, level_start, kb, ko, n)
        self.koff = np.zeros(n, np.uint64)
        self.klen = np.zeros(n, np.uint32)
        self.tomb = np.zeros(n, bool)
        for i, k in enumerate(self.keys):
            t = int(self.table[i])
            if t >= 0:
                self.koff[i], self.klen[i] = entry[t][k]
            if self.res[i] == ora.GET_FOUND and self.vlen[i] == len(TOMBSTONE):
                at = int(self.voff[i]) + 4
                self.tomb[i] = buf[at:at + len(TOMBSTONE)].tobytes() == TOMBSTONE
        self.absent = int((self.res == ora.GET_ABSENT).sum())

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
        the entries' (q * limit + j) slots: idx int64[nq, limit] into keys, -1
        past count."""
        nq = len(ranges)
        count = np.zeros(nq, np.uint32)
        more = np.zeros(nq, np.uint8)
        idx = np.full((nq, limit), -1, np.int64)
        for q, (lo, hi, nu) in enumerate(ranges):
            out, more[q] = self.scan(lo, hi, nu, limit, mode)
            count[q] = len(out)
            idx[q, :len(out)] = out
        return count, more, idx
