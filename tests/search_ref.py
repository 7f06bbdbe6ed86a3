"""The reference answer of lsm_search: Manager.Search (sstable/manager.go:
99-133) composed per level from the oracle's pieces -- ora.level0_get for
level 0 (searchFromLevel0), ora.level_may_contain + ora.level_get for each
non-empty level >= 1 (searchFromLevelWithSparseIndex + searchFromTable); the
first result other than GET_ABSENT wins, an empty level is skipped.
tests/test_search_ref.py pins this composition against a direct restatement
of the Go text.
"""
import numpy as np

import pyoracle as ora

LEVELS = 7


def csr(items):
    data = b"".join(items)
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(data, np.uint8) if data else np.zeros(0, np.uint8), off


def level_starts(counts):
    """Tables per level -> level_start (LEVELS + 1 entries)."""
    assert len(counts) == LEVELS
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def search(buf, offs, lens, dec, level_start, kb, ko, n):
    """Search of probes [0, n) over the tree: tables [level_start[L],
    level_start[L + 1]) of (buf, offs, lens) are level L, dec[t] =
    ora.sst_decode of table t's image.
    -> (level, table, res, voff, vlen, stats); stats[L] = (probes level L
    answered, probes still pending at L that passed its MayContain and missed
    the Seek -- counted for L >= 1)."""
    level = np.full(n, -1, np.int32)
    table = np.full(n, -1, np.int32)
    res = np.full(n, ora.GET_ABSENT, np.int32)
    voff = np.zeros(n, np.uint64)
    vlen = np.zeros(n, np.uint32)
    stats = {}
    kb = kb if kb.size else np.zeros(1, np.uint8)
    for L in range(LEVELS):
        a, b = int(level_start[L]), int(level_start[L + 1])
        if a == b or n == 0:
            continue  # manager.go:121: `if len(m.levels[level]) == 0 { continue }`
        d = dec[a:b]
        metas, idesc, ival = [x[1] for x in d], [x[2] for x in d], [x[3] for x in d]
        pending = res == ora.GET_ABSENT
        if L == 0:
            t, r, o, l = ora.level0_get(buf, offs[a:b], lens[a:b], metas, idesc, ival, kb, ko, 0, n)
            fp = 0
        else:
            t, may = ora.level_may_contain(buf, offs[a:b], metas, kb, ko, 0, n)
            r, o, l = ora.level_get(buf, offs[a:b], lens[a:b], metas, idesc, ival, kb, ko, 0, n, t, may)
            fp = int((pending & (may != 0) & (r == ora.GET_ABSENT)).sum())
        take = pending & (r != ora.GET_ABSENT)
        level[take] = L
        table[take] = t[take] + a
        res[take] = r[take]
        voff[take] = o[take]
        vlen[take] = l[take]
        stats[L] = (int(take.sum()), fp)
    return level, table, res, voff, vlen, stats
