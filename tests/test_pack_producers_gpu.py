"""lsm_pack_results over what the four batched reads return, on one small
database: two logs in front of tree_scan_cases.value_errors' tree (a level-1
table with two broken value offsets over a level-2 table).  The packed bytes
are the host's WAL and image bytes sliced by the views the producers returned
(their D2H, existing code), and the keys and values the case expects."""
import bisect
import functools

import numpy as np
import pytest
import torch

import db_scan_cases as cases
import lsmgpu
import pack_ref
import pyoracle as ora
import tree_scan_cases as tsc
from db_scan_ref import LIVE, RAW, SRC_MEMTABLE
from search_ref import csr
from test_db_scan_gpu import device_db, scan
from test_search_gpu import to_batch
from test_tree_scan_gpu import to_ranges

pytestmark = pytest.mark.gpu

TOMB = cases.TOMB
LIMIT = 5


@functools.lru_cache(maxsize=None)
def small_db():
    """"e03" and "e07": level 1 answers with an error code.  "e05", "e02":
    memtable tombstones over table values.  "e09": a (key, "") node.  "zz": a
    memtable alone."""
    logs = [[(b"e01", b"mem e01 old"), (b"e05", TOMB), (b"zz", b"mem zz"), (b"e01", b"mem e01")],
            [(b"e02", TOMB), (b"e09", b""), (b"e10", b"a memtable value of 33 bytes ....!")]]
    ranges = [(b"", b"", True), (b"e03", b"e08", False), (b"q", b"p", False), (b"e10", b"", True),
              (b"a", b"e", False), (b"e00", b"e02", False)]
    return cases.Case(cases.HostDb(logs, tsc.value_errors().tree), ranges, (LIMIT,))


PROBES = [b"e%02d" % i for i in range(12)] + [b"zz", b"nope", b"", b"e1"]


def get_value(db, key):
    """The bytes database.Get returns for key in LSM_DBGET_TOMBSTONE_HIDES, b""
    for a miss, a memtable tombstone and a table's error code."""
    ref = db.ref
    i = bisect.bisect_left(ref.keys, key)
    if i == len(ref.keys) or ref.keys[i] != key:
        return b""
    if ref.src[i] == SRC_MEMTABLE and ref.tomb[i]:
        return b""
    v = ref.value(i, db.tree.buf)
    return b"" if v is None else v


def search_value(tree, key):
    """The bytes Manager.Search returns for key, b"" for a miss and an error code."""
    ref = tree.ref
    i = bisect.bisect_left(ref.keys, key)
    if i == len(ref.keys) or ref.keys[i] != key or ref.res[i] != ora.GET_FOUND:
        return b""
    at = int(ref.voff[i]) + 4
    return tree.buf[at:at + int(ref.vlen[i])].tobytes()


def host(t, dtype):
    return t.cpu().numpy().view(dtype).reshape(-1)


def strings(arena, off):
    b = arena.cpu().numpy().tobytes() if arena is not None else b""
    o = host(off, np.uint64)
    return [b[int(o[e]):int(o[e + 1])] for e in range(o.size - 1)]


def same_as_ref(p, want):
    assert host(p.counts, np.uint64).tolist() == want.counts.tolist()
    assert np.array_equal(host(p.row_start, np.uint64), want.row_start)
    assert np.array_equal(host(p.entry_slot, np.uint32), want.entry_slot)
    assert np.array_equal(host(p.voff, np.uint64), want.voff)
    assert p.vals.cpu().numpy().tobytes() == want.vals
    if want.koff is not None:
        assert np.array_equal(host(p.koff, np.uint64), want.koff)
        assert p.keys.cpu().numpy().tobytes() == want.keys


@pytest.mark.parametrize("mode", [RAW, LIVE])
def test_db_scan_then_pack(ctx, mode):
    case = small_db()
    dd = device_db(ctx, case)
    db = case.db
    batch, flags = to_ranges(ctx, case.ranges)
    out = scan(dd, batch, flags, LIMIT, mode, mem_index=dd.indexes[1], tree=dd.dt.tree)
    p = lsmgpu.pack_db_scan(ctx, dd.d_wal, dd.dt.d_img, out, LIMIT)
    torch.cuda.synchronize()
    nq = len(case.ranges)
    want = pack_ref.pack(dd.c.buf, db.tree.buf, host(out.src, np.int32), host(out.key, pack_ref.DESC),
                         host(out.value, pack_ref.DESC), host(out.count, np.uint32), nq, LIMIT,
                         key_cap=1 << 30, val_cap=1 << 30)
    same_as_ref(p, want)
    # and what the case expects: the keys of the reference's scan, each with its answering entry's value
    wc, _, widx = db.ref.scan_batch(case.ranges, LIMIT, mode)
    at = widx[widx >= 0]
    assert host(p.row_start, np.uint64).tolist() == np.concatenate([[0], np.cumsum(wc)]).tolist()
    assert strings(p.keys, p.koff) == [db.ref.keys[i] for i in at]
    assert strings(p.vals, p.voff) == [db.ref.value(i, db.tree.buf) or b"" for i in at]
    src = host(out.src, np.int32)[host(p.entry_slot, np.uint32)]
    assert (src == SRC_MEMTABLE).sum() >= 4 and (src != SRC_MEMTABLE).sum() >= 8
    if mode == RAW:
        assert TOMB in strings(p.vals, p.voff)
    else:
        assert TOMB not in strings(p.vals, p.voff)


def test_tree_scan_then_pack_equals_gather_kvs(ctx):
    case = small_db()
    dd = device_db(ctx, case)
    dt, tree = dd.dt, case.db.tree
    batch, flags = to_ranges(ctx, case.ranges)
    got = lsmgpu.tree_scan(ctx, dt.d_img, dt.r, tree.level_start, batch, flags, LIMIT, RAW, index=dt.index,
                           tree=dt.tree)
    count, _, key, value = got[:4]
    p = lsmgpu.pack_tree_scan(ctx, dt.d_img, got, LIMIT)
    E, K, V, over = host(p.counts, np.uint64).tolist()
    assert E == int(host(count, np.uint32).sum()) >= 12 and over == 0
    g = lsmgpu.gather_kvs(ctx, dt.d_img, key, value, p.entry_slot, E, K, V)
    torch.cuda.synchronize()
    assert torch.equal(g.koff[:E + 1], p.koff) and torch.equal(g.voff[:E + 1], p.voff)
    assert torch.equal(g.keys[:K], p.keys) and torch.equal(g.vals[:V], p.vals)
    wc, _, widx = tree.ref.scan_batch(case.ranges, LIMIT, RAW)
    assert strings(p.keys, p.koff) == [tree.ref.keys[i] for i in widx[widx >= 0]]
    assert strings(p.vals, p.voff) == [search_value(tree, tree.ref.keys[i]) for i in widx[widx >= 0]]
    # the two error codes are entries of the full range, with a key and no value
    assert strings(p.vals, p.voff)[3] == b"" and strings(p.keys, p.koff)[3] == b"e03"


def test_db_get_then_pack(ctx):
    case = small_db()
    dd = device_db(ctx, case)
    db, dt = case.db, dd.dt
    kb, ko = csr(PROBES)
    out = lsmgpu.db_get(ctx, dd.d_wal, dd.r, dd.mo, dt.d_img, dt.r, db.tree.level_start, to_batch(ctx, kb, ko),
                        mode=lsmgpu.DBGET_TOMBSTONE_HIDES, index=dt.index, mem_index=dd.indexes[1], tree=dt.tree)
    p = lsmgpu.pack_db_get(ctx, dd.d_wal, dt.d_img, out)
    torch.cuda.synchronize()
    n = len(PROBES)
    assert p.koff is None and p.keys is None
    assert host(p.row_start, np.uint64).tolist() == list(range(n + 1))
    assert host(p.entry_slot, np.uint32).tolist() == list(range(n))
    want = [get_value(db, k) for k in PROBES]
    assert strings(p.vals, p.voff) == want
    assert host(p.counts, np.uint64).tolist() == [n, 0, sum(len(v) for v in want), 0]
    by_key = dict(zip(PROBES, want))
    # a miss, a memtable tombstone over a table value, an error code, a (key, "") node: nothing packed
    assert by_key[b"nope"] == b"" and by_key[b"e05"] == b"" and by_key[b"e03"] == b"" and by_key[b"e09"] == b""
    assert by_key[b"e01"] == b"mem e01" and by_key[b"e04"] == b"one4" and by_key[b"zz"] == b"mem zz"
    res = host(out.result, np.int32)
    assert res[3] not in (ora.GET_FOUND, ora.GET_ABSENT) and host(out.src, np.int32)[13] == lsmgpu.SRC_NONE
    # the same through pack_ref, from the views the Get returned
    ref = pack_ref.pack(dd.c.buf, db.tree.buf, host(out.src, np.int32), None, host(out.value, pack_ref.DESC),
                        None, n, 1, val_cap=1 << 30)
    same_as_ref(p, ref)


def test_search_then_pack(ctx):
    case = small_db()
    dd = device_db(ctx, case)
    dt, tree = dd.dt, case.db.tree
    kb, ko = csr(PROBES)
    found = lsmgpu.search(ctx, dt.d_img, dt.r, tree.level_start, to_batch(ctx, kb, ko), index=dt.index,
                          tree=dt.tree)
    p = lsmgpu.pack_search(ctx, dt.d_img, found)
    torch.cuda.synchronize()
    n = len(PROBES)
    assert p.koff is None and p.keys is None
    assert host(p.row_start, np.uint64).tolist() == list(range(n + 1))
    want = [search_value(tree, k) for k in PROBES]
    assert strings(p.vals, p.voff) == want
    assert want[3] == b"" and want[7] == b"" and want[5] == b"one5" and want[12] == b"" and want[13] == b""
    ref = pack_ref.pack(None, tree.buf, None, None, host(found[3], pack_ref.DESC), None, n, 1, val_cap=1 << 30)
    same_as_ref(p, ref)
