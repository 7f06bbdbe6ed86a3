"""GPU parity of lsm_db_scan: the batched range scan over the memtables and the
tree against tests/db_scan_ref.py (lsm_memtable_search's answer, else
lsm_search's, for every key any source holds in the range; pinned against a
literal merge of iterators in tests/test_db_scan_ref.py).  Bit-exact on count,
more and, per entry, the key's view, the value's view, the source, the log or
table and the result code -- with and without the memtable index, with and
without the Seek tree, in both modes.  The cases are tests/db_scan_cases.py's.
"""
import dataclasses
import random
import types

import numpy as np
import pytest
import torch

import db_scan_cases as cases
import db_scan_ref
import lsmgpu
import pyoracle as ora
from db_scan_ref import LIVE, RAW, SRC_MEMTABLE, SRC_SSTABLE
from test_memtable_gpu import Case as Logs
from test_tree_scan_gpu import device_tree, to_ranges

pytestmark = pytest.mark.gpu

NO_LOGS = types.SimpleNamespace(nlog=0, nslot=0, idx=None, file_start=None)


def expected(ref, tree_ref, log_desc):
    """The eight output fields of every key of ref (a DbRef), as arrays over
    ref.keys.  log_desc[w]: log w's descriptors by record position."""
    n = len(ref.keys)
    e = {k: np.zeros(n, np.int64) for k in ("koff", "klen", "kvlen", "voff", "vlen", "table", "res", "src")}
    for i in range(n):
        if ref.src[i] == SRC_MEMTABLE:
            d = log_desc[int(ref.log[i])][int(ref.pos[i])]
            ro, kl, vl = int(d["rec_off"]), int(d["key_len"]), int(d["val_len"])
            row = (ro, kl, vl, ro + 4 + kl, vl, int(ref.log[i]), ora.GET_FOUND, SRC_MEMTABLE)
        else:
            t = int(ref.tree[i])
            row = (int(tree_ref.koff[t]), int(tree_ref.klen[t]), 8, int(tree_ref.voff[t]), int(tree_ref.vlen[t]),
                   int(tree_ref.table[t]), int(tree_ref.res[t]), SRC_SSTABLE)
        for k, v in zip(("koff", "klen", "kvlen", "voff", "vlen", "table", "res", "src"), row):
            e[k][i] = v
    return e


class DeviceDb:
    """A HostDb on the device: the tree (test_tree_scan_gpu's), the logs
    replayed and ordered, the memtable index over every node and, where the
    case asks, one over the first indexed_nodes nodes only."""

    def __init__(self, ctx, case):
        db = case.db
        self.ctx, self.db, self.case = ctx, db, case
        self.dt = device_tree(ctx, db.tree)
        self.indexes = [None]
        if db.wal:
            self.c = c = Logs(ctx, db.wal, case.placement)
            self.d_wal, self.r = c.d, c.r
            self.mo = lsmgpu.memtable_order(ctx, c.d, c.r, c.off, c.maxrec, lsmgpu.MEMTABLE_ALL)
            self.indexes.append(lsmgpu.memtable_search_index(ctx, c.d, c.r, self.mo))
            if case.indexed_nodes:
                nb = int(ctx.lib.lsm_memtable_search_index_bytes(case.indexed_nodes))
                small = torch.empty(nb, dtype=torch.uint8, device=ctx.torch_device)
                lsmgpu._lib.check(ctx.lib.lsm_memtable_search_index_build(
                    ctx.handle, c.d.data_ptr(), c.r.desc.data_ptr(), self.mo.idx.data_ptr(),
                    self.mo.file_start.data_ptr(), self.mo.nlog, case.indexed_nodes, small.data_ptr(), nb, None),
                    "lsm_memtable_search_index_build")
                self.indexes.append(small)
            log_desc = [ora.decode_block(ora.GRAMMAR_KV, c.buf, int(o), int(n))[1] for o, n in zip(c.offs, c.lens)]
            assert [st != 0 for st, _ in c.decoded] == [w in db.failed for w in range(len(db.wal))]
        else:
            self.d_wal, self.r, self.mo, log_desc = None, None, NO_LOGS, []
        self.want = expected(db.ref, db.tree.ref, log_desc)


_dbs = {}


def device_db(ctx, case):
    if id(case) not in _dbs:
        _dbs[id(case)] = DeviceDb(ctx, case)
    return _dbs[id(case)]


def scan(dd, batch, flags, limit, mode, mem_index=None, tree=None):
    dt = dd.dt
    return lsmgpu.db_scan(dd.ctx, dd.d_wal, dd.r, dd.mo, dt.d_img, dt.r, dd.db.tree.level_start, batch, flags,
                          limit, mode, index=dt.index, mem_index=mem_index, tree=tree)


def compare(out, nq, limit, wc, wm, widx, want, tag):
    count = out.count.cpu().numpy().view(np.uint32)
    more = out.more.cpu().numpy()
    assert (count == wc).all(), (tag, np.flatnonzero(count != wc)[:8], count[:8], wc[:8])
    assert (more == wm).all(), (tag, np.flatnonzero(more != wm)[:8])
    sel = widx >= 0
    at = widx[sel]
    key = out.key.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(nq, limit)[sel]
    value = out.value.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(nq, limit)[sel]
    got = {"koff": key["rec_off"], "klen": key["key_len"], "kvlen": key["val_len"], "voff": value["rec_off"],
           "vlen": value["val_len"], "table": out.table.cpu().numpy().reshape(nq, limit)[sel],
           "res": out.result.cpu().numpy().reshape(nq, limit)[sel],
           "src": out.src.cpu().numpy().reshape(nq, limit)[sel]}
    for name, g in got.items():
        bad = np.flatnonzero(g.astype(np.int64) != want[name][at])
        assert bad.size == 0, (tag, name, bad.size, [(int(i), int(g[i]), int(want[name][at[i]])) for i in bad[:4]])
    assert (value["key_len"] == 0).all()


def check(dd, ranges, limit, mode, batch=None, want=None):
    """lsm_db_scan with every memtable index and Seek tree the case has, and
    without, against the reference."""
    wc, wm, widx = want if want is not None else dd.db.ref.scan_batch(ranges, limit, mode)
    if batch is None:
        batch = to_ranges(dd.ctx, ranges)
    trees = (None, dd.dt.tree) if dd.dt.tree is not None else (None,)
    for mi, mem_index in enumerate(dd.indexes):
        for tree in trees:
            out = scan(dd, batch[0], batch[1], limit, mode, mem_index=mem_index, tree=tree)
            torch.cuda.synchronize()
            compare(out, len(ranges), limit, wc, wm, widx, dd.want, (mi, tree is not None, mode, limit))
    return wc, wm, widx


def run_case(ctx, case):
    dd = device_db(ctx, case)
    assert dd.db.ref.absent == 0
    batch = to_ranges(ctx, case.ranges)
    emitted = 0
    for mode in (RAW, LIVE):
        for limit in case.limits:
            wc, _, _ = check(dd, case.ranges, limit, mode, batch)
            emitted += int(wc.sum())
    return dd, emitted


def test_node_counts_offset_placement(ctx):
    """Logs of 5, 0 (empty), 1, 0 (failed), 2 and 1 nodes."""
    dd, emitted = run_case(ctx, cases.node_counts())
    torch.cuda.synchronize()
    assert [len(x) for x in dd.mo.result()[0]] == [5, 0, 1, 0, 2, 1]
    assert emitted > 50 and len(dd.indexes) == 2


def test_node_counts_plan_placement_and_a_short_index(ctx):
    """The plan placement; an index of the first six nodes: logs 4 and 5 lie
    past it and are searched and walked through d_idx."""
    dd, emitted = run_case(ctx, cases.node_counts_plan())
    fs = dd.mo.file_start.cpu().numpy()
    assert fs.tolist() == [0, 5, 5, 6, 6, 8, 9] and len(dd.indexes) == 3
    assert emitted > 50


def test_shadowing(ctx):
    case = cases.shadowing()
    dd, _ = run_case(ctx, case)
    ranges = [(b"s", b"u", False), (b"y", b"z", False), (b"e", b"f", False), (b"x2", b"x3", False)]
    batch, flags = to_ranges(ctx, ranges)
    got = {}
    for mode in (RAW, LIVE):
        out = scan(dd, batch, flags, 1, mode, mem_index=dd.indexes[1], tree=dd.dt.tree)
        torch.cuda.synchronize()
        value = out.value.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        src = out.src.cpu().numpy()
        vals = []
        for q in range(len(ranges)):
            buf = dd.c.buf if src[q] == SRC_MEMTABLE else dd.db.tree.buf
            o, n = int(value[q]["rec_off"]) + 4, int(value[q]["val_len"])
            vals.append(buf[o:o + n].tobytes() if out.count[q] else None)
        got[mode] = (out.count.cpu().tolist(), out.more.cpu().tolist(), vals, src.tolist(),
                     out.table.cpu().tolist())
    # "s": log 1's tombstone answers -- its 13 bytes in RAW (not log 0's value, not the table's); in LIVE
    # the range's first entry is "t", log 0's value over the level-0 tombstone
    assert got[RAW][2][0] == cases.TOMB and got[RAW][3][0] == SRC_MEMTABLE and got[RAW][4][0] == 1
    assert got[LIVE][2][0] == b"mem t" and got[LIVE][3][0] == SRC_MEMTABLE and got[LIVE][4][0] == 0
    # "y1" live, then memtable tombstones only: more differs
    assert got[RAW][0][1] == 1 and got[LIVE][0][1] == 1 and got[RAW][1][1] == 1 and got[LIVE][1][1] == 0
    # (key, ""): found, length 0, in both modes
    assert got[RAW][2][2] == b"" and got[LIVE][2][2] == b"" and got[LIVE][0][2] == 1
    # a memtable value over a table's tombstone
    assert got[LIVE][2][3] == b"mem x2" and got[LIVE][3][3] == SRC_MEMTABLE


def test_keys(ctx):
    """Equal 16-byte prefixes across memtables and tables, a proper prefix, the
    empty key, 0xFF keys; lo and hi equal to memtable keys, lo >= hi, NO_UPPER."""
    _, emitted = run_case(ctx, cases.keys_case())
    assert emitted > 100


@pytest.mark.parametrize("name,nlog,nsrc", [("width_16", 3, 16), ("width_17", 3, 17), ("width_64", 11, 64),
                                            ("width_65", 11, 65), ("wide_134", 70, 134)])
def test_widths(ctx, name, nlog, nsrc):
    """16: the first row's shifts alone; 17: the whole wave; 64: every lane of
    the register path; 65: the workspace path; 134: memtable lanes in two
    rounds, the tree's sources in the last two."""
    case = cases.CASES[name]()
    assert len(case.db.records) == nlog and case.db.nsrc == nsrc
    _, emitted = run_case(ctx, case)
    assert emitted > 50


def test_no_logs_equals_tree_scan(ctx):
    """nlog == 0: lsm_tree_scan's outputs on the mixed tree, every d_src SRC_SSTABLE."""
    case = cases.tree_alone()
    dd, emitted = run_case(ctx, case)
    assert emitted > 500
    dt = dd.dt
    batch, flags = to_ranges(ctx, case.ranges)
    for mode in (RAW, LIVE):
        out = scan(dd, batch, flags, 7, mode, tree=dt.tree)
        count, more, key, value, table, result = lsmgpu.tree_scan(
            ctx, dt.d_img, dt.r, case.db.tree.level_start, batch, flags, 7, mode, index=dt.index, tree=dt.tree)
        torch.cuda.synchronize()
        assert torch.equal(out.count, count) and torch.equal(out.more, more)
        sel = (torch.arange(7, device=count.device)[None, :] < count[:, None]).reshape(-1)
        for a, b in ((out.key, key), (out.value, value), (out.table, table), (out.result, result)):
            assert torch.equal(a[sel], b[sel])
        assert bool((out.src[sel] == SRC_SSTABLE).all()) and int(sel.sum()) > 20


def test_empty_tree_scans_the_memtables(ctx):
    dd, emitted = run_case(ctx, cases.logs_alone())
    assert emitted > 20 and dd.dt.r.nfile == 0


def test_both_empty(ctx):
    case = cases.both_empty()
    dd = device_db(ctx, case)
    batch, flags = to_ranges(ctx, case.ranges)
    for mode in (RAW, LIVE):
        out = scan(dd, batch, flags, 4, mode)
        torch.cuda.synchronize()
        assert out.count.cpu().tolist() == [0, 0] and out.more.cpu().tolist() == [0, 0]


def test_strides(ctx):
    """The walk's grid-stride loop iterates: each wave takes three ranges, the
    last pass ragged.  The reference is the pattern's, tiled."""
    tiled = cases.strides()
    dd = device_db(ctx, cases.Case(tiled.db, tiled.pattern, (tiled.limit,)))
    batch = to_ranges(ctx, tiled.ranges)
    for mode in (RAW, LIVE):
        want = tiled.want(mode)
        out = scan(dd, batch[0], batch[1], tiled.limit, mode, mem_index=dd.indexes[1], tree=dd.dt.tree)
        torch.cuda.synchronize()
        compare(out, tiled.nq, tiled.limit, *want, dd.want, ("strides", mode))
        assert want[0].size == tiled.nq == 2 * cases.tsc.WALK_STRIDE + 37


def test_edges(ctx):
    """nq == 0 leaves the outputs untouched; LSM_ESPACE for an index no node
    fits, a short tree buffer and a workspace one byte short; LSM_EINVAL for
    limit == 0, a bad mode, nq * limit == 2^32 and a decreasing level_start."""
    case = cases.shadowing()
    dd = device_db(ctx, case)
    dt, dev = dd.dt, ctx.torch_device
    batch, flags = to_ranges(ctx, case.ranges)
    flags = torch.from_numpy(flags).to(dev)
    nq = len(case.ranges)
    ls = case.db.tree.level_start

    def outputs(limit):
        full = lambda shape, dt=torch.int32: torch.full(shape, 77, dtype=dt, device=dev)  # noqa: E731
        return lsmgpu.DbScan(full((nq,)), full((nq,), torch.uint8), full((nq * limit, 4)), full((nq * limit, 4)),
                             full((nq * limit,)), full((nq * limit,)), full((nq * limit,)))

    def into(out, limit=4, mode=LIVE, ranges=batch, level_start=ls, **kw):
        lsmgpu.db_scan_into(ctx, dd.d_wal, dd.r, dd.mo, dt.d_img, dt.r, level_start, ranges, flags, limit, mode,
                            dt.index, out, **kw)

    out = outputs(4)
    untouched = lambda: all(bool((getattr(out, f.name) == 77).all()) for f in dataclasses.fields(out))  # noqa: E731
    into(out, ranges=dataclasses.replace(batch, n=0))
    torch.cuda.synchronize()
    assert untouched()
    with pytest.raises(RuntimeError, match="code -4"):
        into(out, mem_index=dd.indexes[1][:int(ctx.lib.lsm_memtable_search_index_bytes(1)) - 1])
    short = lsmgpu.SeekTree(dt.tree.data[:dt.tree.data.numel() // 2], dt.tree.max_nidx)
    with pytest.raises(RuntimeError, match="code -4"):
        into(out, tree=short)
    ws = lsmgpu.db_scan_workspace(ctx, dd.mo.nlog, ls, nq)
    assert ws.numel() == nq * (2 + int(ls[1]) + cases.LEVELS - 1) * 32
    with pytest.raises(RuntimeError, match="code -4"):
        into(out, ws=ws[:ws.numel() - 1])
    with pytest.raises(RuntimeError, match="code -1"):
        into(out, limit=0)
    with pytest.raises(RuntimeError, match="code -1"):
        into(out, mode=2)
    # nq * limit == 2^32: refused before anything is read, so the batch's claimed size is never used
    with pytest.raises(RuntimeError, match="code -1"):
        into(out, limit=1 << 16, ranges=dataclasses.replace(batch, n=1 << 16), ws=ws)
    down = np.array(ls).copy()
    down[3] = down[2] - 1
    assert down[-1] == dt.r.nfile
    with pytest.raises(RuntimeError, match="code -1"):
        into(out, level_start=down, ws=ws)
    torch.cuda.synchronize()
    assert untouched()


def test_after_db_write(ctx):
    """The logs lsm_db_write just produced (its descriptors and rec_base, no
    replay) scanned over the small tree, against the reference run on
    db_write_ref's logs."""
    from test_db_write_gpu import expected_desc, expected_layout, random_ops, run
    rng = random.Random(41)
    keys = [b"", b"r", b"s", b"t", b"w1", b"x2", b"y", cases.LONG + b"x", cases.LONG + b"y"]
    want, w, res = run(ctx, random_ops(rng, 120, keys=keys), 0, 250)
    assert res.nlog >= 4
    r, wal_off = w.replay(res.nlog)
    mo = lsmgpu.memtable_order(ctx, w.wal, r, wal_off, res.most_records, lsmgpu.MEMTABLE_ALL)
    mem_index = lsmgpu.memtable_search_index(ctx, w.wal, r, mo)
    tree = cases.small_tree()
    dt = device_tree(ctx, tree)
    logs = [[(k, b"" if v is None else v) for k, v in lg] for lg in want.logs]
    ref = db_scan_ref.DbRef(logs, tree.ref)
    desc = expected_desc(want, expected_layout(want, 16)[1])
    base = want.rec_base()
    exp = expected(ref, tree.ref, [desc[base[s]:base[s + 1]] for s in range(want.nlog)])
    ranges = [(b"", b"", True), (b"s", b"x", False), (cases.LONG, b"", True), (b"", b"\x00", False)]
    batch, flags = to_ranges(ctx, ranges)
    assert (ref.src == SRC_MEMTABLE).sum() >= 5 and (ref.src == SRC_SSTABLE).sum() >= 2 and ref.tomb.any()
    for mode in (RAW, LIVE):
        for limit in (2, 64):
            wc, wm, widx = ref.scan_batch(ranges, limit, mode)
            for mi in (None, mem_index):
                out = lsmgpu.db_scan(ctx, w.wal, r, mo, dt.d_img, dt.r, tree.level_start, batch, flags, limit, mode,
                                     index=dt.index, mem_index=mi, tree=dt.tree)
                torch.cuda.synchronize()
                compare(out, len(ranges), limit, wc, wm, widx, exp, ("db_write", mi is not None, mode, limit))
