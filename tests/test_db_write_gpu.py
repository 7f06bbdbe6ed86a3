"""GPU parity of lsm_db_write: database.Put / database.Delete of a batch, the
logs with memtable rotation and the descriptors of their records.

Every comparison is exact, against db_write_ref.write (the closed form,
pinned to the restated Manager in test_db_write_ref.py): the whole d_wal buffer
(the logs' bytes and the untouched fill between and behind them), d_log_start,
d_wal_off, d_wal_len, d_rec_base, d_counts, d_main_slot and d_desc; d_desc also
against lsm_wal_replay run on the produced bytes.  mem_max is small, so a
handful of ops rotates; one case passes the sort tile (1,024 ops in a log).
"""
import random

import numpy as np
import pytest
import torch

import db_write_ref as ref
import lsmgpu
from memtable_ref import wal_bytes
from test_db_write_ref import random_ops
from test_memtable_gpu import Case, csr

pytestmark = pytest.mark.gpu

TOMB = ref.TOMBSTONE
FILL = 0xA5
MISS, VALUE, DELETED = lsmgpu.MEM_MISS, lsmgpu.MEM_VALUE, lsmgpu.MEM_DELETED


def P(key, value=b""):
    return (ref.PUT, key, value)


def D(key, ignored=b""):
    return (ref.DELETE, key, ignored)


def to_device(ctx, ops):
    kb, ko = csr([k for _, k, _ in ops])
    vb, vo = csr([v for _, _, v in ops])
    batch = lsmgpu.batch_to_device(ctx, kb, ko, vb, vo)
    return batch, np.array([kind for kind, _, _ in ops], np.uint8)


def current(ctx, nodes):
    """The current memtable from a log of (key, value) records -> cur, the
    buffers kept alive with it."""
    c = Case(ctx, [wal_bytes(nodes)])
    mo = lsmgpu.memtable_order(ctx, c.d, c.r, c.off, c.maxrec, lsmgpu.MEMTABLE_ALL)
    torch.cuda.synchronize()
    per_log, _, over = mo.result()
    assert not over and len(per_log[0]) == len({k for k, _ in nodes})
    return (c.d, c.r.desc, mo.idx[:len(per_log[0])]), (c, mo)


def expected_layout(want, align):
    lens = [len(b) for b in want.log_bytes()]
    off = [0]
    for n in lens:
        off.append(off[-1] + (n + align - 1) // align * align)
    return lens, off


def expected_desc(want, off):
    out = []
    for s, lg in enumerate(want.logs):
        at = off[s]
        for k, v in lg:
            vl = 0 if v is None else len(v)
            out.append((at, len(k), vl))
            at += 8 + len(k) + vl
    return np.array(out, lsmgpu.DESC_DTYPE) if out else np.zeros(0, lsmgpu.DESC_DTYPE)


def replay_of(ctx, w, res):
    """lsm_wal_replay of the produced logs, rec_base placement over d_rec_base."""
    dev = ctx.torch_device
    nlog = res.nlog
    r = lsmgpu.codec.DecodeResult(desc=torch.zeros((max(res.nrec, 1), 4), dtype=torch.int32, device=dev),
                            nrec=torch.zeros(nlog, dtype=torch.int32, device=dev),
                            status=torch.full((nlog,), -1, dtype=torch.int32, device=dev),
                            rec_base=w.rec_base[:nlog + 1])
    max_len = int(res.wal_len.max())
    lsmgpu.wal_replay_into(ctx, w.wal, w.wal_off[:nlog], w.wal_len[:nlog], max_len, r,
                           lsmgpu.wal_workspace(ctx, nlog, max_len))
    torch.cuda.synchronize()
    return r


def run(ctx, ops, mem_size0=0, mem_max=1000, nodes=(), align=16, cur=None, **kw):
    """One call against the closed form -> (the closed form, DbWrite, its result)."""
    keep = None
    if nodes and cur is None:
        cur, keep = current(ctx, nodes)
    batch, kinds = to_device(ctx, ops)
    w = lsmgpu.db_write(ctx, batch, kinds, mem_size0=mem_size0, mem_max=mem_max, cur=cur, align=align, fill=FILL,
                        **kw)
    torch.cuda.synchronize()
    res = w.result()
    want = ref.write(ops, mem_size0, mem_max, [k for k, _ in nodes])
    lens, off = expected_layout(want, align)
    assert not res.overflow and res.nlog == want.nlog
    assert res.log_start.tolist() == want.log_start
    assert res.wal_len.tolist() == lens
    assert res.wal_off.tolist() == off
    assert res.rec_base.tolist() == want.rec_base()
    assert (res.nrec, res.nbytes, res.most_records, res.mem_size) == \
        (want.rec_base()[-1], off[-1], max(len(lg) for lg in want.logs), want.size)
    # the whole buffer: each log's bytes, the fill everywhere else
    image = np.full(w.wal.numel(), FILL, np.uint8)
    for s, b in enumerate(want.log_bytes()):
        image[off[s]:off[s] + len(b)] = np.frombuffer(b, np.uint8)
    got = w.wal.cpu().numpy()
    bad = np.flatnonzero(got != image)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), image[bad[:8]].tolist())
    if w.main_slot is not None:
        slots = w.main_slot[:len(ops)].cpu().numpy().view(np.uint32)
        assert slots.tolist() == [want.rec_base()[lg] + r for lg, r in want.main]
    if w.desc is not None:
        desc = w.desc[:res.nrec].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        assert np.array_equal(desc, expected_desc(want, off))
        r = replay_of(ctx, w, res)
        assert r.status.cpu().numpy().tolist() == [0] * res.nlog
        assert r.nrec.cpu().numpy().tolist() == [len(lg) for lg in want.logs]
        assert np.array_equal(r.desc_numpy()[:res.nrec], desc)
    del keep
    return want, w, res


def sizes(want):
    return [len(lg) for lg in want.logs]


def extras(want):
    """(log, record index) of every (key, nil) record."""
    return [(s, r) for s, lg in enumerate(want.logs) for r, (_, v) in enumerate(lg) if v is None]


ALIGNS = [1, 16]
NODES = [(b"n", b"1"), (b"m", b"2")]
K16 = b"0123456789abcdef"
K40 = b"k" * 39


# ---- the fit boundary and log 0 ------------------------------------------------------

@pytest.mark.parametrize("align", ALIGNS)
def test_fit_boundary(ctx, align):
    ops = [P(b"k", b"abc")] * 6  # est 20 each
    assert sizes(run(ctx, ops, 0, 100, align=align)[0]) == [5, 1]  # 100 fits exactly
    assert sizes(run(ctx, ops, 0, 99, align=align)[0]) == [4, 2]   # one byte less rotates
    assert sizes(run(ctx, ops, 1, 100, align=align)[0]) == [4, 2]
    assert sizes(run(ctx, ops[:5], 0, 100, align=align)[0]) == [5]


@pytest.mark.parametrize("align", ALIGNS)
def test_log0(ctx, align):
    big, small = P(b"big", b"x" * 200), P(b"s")
    want, _, res = run(ctx, [big, small], 0, 50, align=align)   # an empty memtable is promoted too
    assert sizes(want) == [0, 1, 1] and res.log_start.tolist() == [0, 0, 1, 2]
    assert sizes(run(ctx, [small, small], 40, 50, align=align)[0]) == [0, 2]   # 40 + 17 > 50
    assert sizes(run(ctx, [small, small], 33, 50, align=align)[0]) == [1, 1]   # 33 + 17 = 50 fits
    want, _, res = run(ctx, [small], 70, 50, align=align)                      # mem_size0 > mem_max
    assert sizes(want) == [0, 1] and res.mem_size == 17
    want, _, res = run(ctx, [small], 70, 100, align=align)
    assert sizes(want) == [1] and res.mem_size == 87


@pytest.mark.parametrize("align", ALIGNS)
def test_oversized_op_mid_batch(ctx, align):
    big, small = P(b"big", b"x" * 200), P(b"s")
    want, _, _ = run(ctx, [small, big, small, small, big, big], 0, 50, align=align)
    assert sizes(want) == [1, 1, 2, 1, 1]


# ---- the Deletes ------------------------------------------------------------------------

@pytest.mark.parametrize("align", ALIGNS)
def test_deletes(ctx, align):
    assert extras(run(ctx, [D(b"a")], align=align)[0]) == []                       # absent
    assert extras(run(ctx, [P(b"a", b"v"), D(b"a")], align=align)[0]) == [(0, 1)]  # Put then Delete
    assert extras(run(ctx, [D(b"a"), D(b"a")], align=align)[0]) == [(0, 1)]        # the tombstone is a node
    assert extras(run(ctx, [P(b"b"), D(b"a"), P(b"a"), D(b"b"), D(b"a")], align=align)[0]) == [(0, 3), (0, 5)]


@pytest.mark.parametrize("align", ALIGNS)
def test_deletes_and_rotation(ctx, align):
    v = b"v" * 20
    # a is in log 0; the Delete is the second op of log 1: no extra
    want, _, _ = run(ctx, [P(b"a", v), P(b"b", v), D(b"a")], 0, 70, align=align)
    assert sizes(want) == [1, 2] and extras(want) == []
    # the Delete opens log 1 and its key is in log 0: the extra closes log 0
    want, _, _ = run(ctx, [P(b"k", b"v" * 10), D(b"k")], 0, 30, align=align)
    assert want.logs == [[(b"k", b"v" * 10), (b"k", None)], [(b"k", TOMB)]]
    # ... and with an absent key
    want, _, _ = run(ctx, [P(b"j", b"v" * 10), D(b"k")], 0, 30, align=align)
    assert sizes(want) == [1, 1] and extras(want) == []
    # every op rotates: each Delete looks into the one-op log before it
    want, _, _ = run(ctx, [D(b"a"), D(b"a"), D(b"b"), D(b"b"), D(b"a")], 0, 30, align=align)
    assert sizes(want) == [2, 1, 2, 1, 1] and extras(want) == [(0, 1), (2, 1)]


@pytest.mark.parametrize("align", ALIGNS)
def test_current_memtable(ctx, align):
    # a key only among the nodes
    want, _, _ = run(ctx, [D(b"n")], nodes=NODES, align=align)
    assert want.logs == [[(b"n", None), (b"n", TOMB)]]
    assert extras(run(ctx, [D(b"x"), P(b"m"), D(b"m")], nodes=NODES, align=align)[0]) == [(0, 2)]
    # the same key after a rotation: the nodes are log 0's alone
    ops = [D(b"n"), P(b"p", b"x" * 40), D(b"n"), D(b"m")]
    want, _, _ = run(ctx, ops, 0, 60, nodes=NODES, align=align)
    assert sizes(want) == [2, 1, 2] and extras(want) == [(0, 0)]
    # a Delete that opens log 1, its key only among the nodes: the extra goes to log 0
    want, _, _ = run(ctx, [P(b"p", b"x" * 40), D(b"n")], 0, 60, nodes=NODES, align=align)
    assert want.logs == [[(b"p", b"x" * 40), (b"n", None)], [(b"n", TOMB)]]
    # ... as op 0 of a memtable that is already full: log 0 holds the extra alone
    want, _, _ = run(ctx, [D(b"m"), D(b"q")], 100, 60, nodes=NODES, align=align)
    assert want.logs == [[(b"m", None)], [(b"m", TOMB), (b"q", TOMB)]]
    # NULL nodes with a count, and nodes with a count of zero: an empty skiplist
    cur, keep = current(ctx, NODES)
    assert extras(run(ctx, [D(b"n")], cur=(cur[0], cur[1], cur[2][:0]), align=align)[0]) == []


@pytest.mark.parametrize("align", ALIGNS)
def test_key_shapes(ctx, align):
    ops = [P(K16 + b"a", b"1"), D(K16 + b"b"), D(K16 + b"a"),      # 16 equal bytes, the tail differs
           P(K16), D(K16 + b"\x00"), D(K16[:15]), D(K16),          # a prefix at the 16-byte edge
           P(b""), D(b"\x00"), D(b""),                             # the empty key
           P(b"ab"), D(b"a"), D(b"abc"), D(b"ab"),                 # proper prefixes
           P(K40 + b"a"), D(K40 + b"b"), D(K40), D(K40 + b"a"),    # 40 bytes, the last differs
           D(b"\xff" * 17), D(b"\xff" * 17)]
    want, _, _ = run(ctx, ops, 0, 10000, align=align)
    assert sizes(want) == [len(ops) + 6]
    assert [want.logs[0][r][0] for _, r in extras(want)] == [K16 + b"a", K16, b"", b"ab", K40 + b"a", b"\xff" * 17]
    # the same keys among the nodes, and across a rotation
    nodes = [(K16 + b"a", b"1"), (b"", b"2"), (b"ab", b"3"), (K40 + b"a", b"4")]
    dels = [D(K16 + b"b"), D(K16), D(b"a"), D(b"abc"), D(K40 + b"b"), D(K40), D(b"\x00"),
            D(K40 + b"a"), D(b"ab"), D(b""), D(K16 + b"a")]
    want, _, _ = run(ctx, dels, nodes=nodes, align=align)
    assert [want.logs[0][r][0] for _, r in extras(want)] == [K40 + b"a", b"ab", b"", K16 + b"a"]
    run(ctx, ops + dels, 0, 120, nodes=nodes, align=align)


@pytest.mark.parametrize("align", ALIGNS)
def test_values(ctx, align):
    ops = [P(b"k", b""), P(b"k", TOMB), D(b"k", b"not written"), P(b"", b""), D(b"j", b"x" * 50),
           P(b"v", bytes(range(256)) * 3)]
    want, _, res = run(ctx, ops, align=align)
    assert extras(want) == [(0, 2)] and res.nrec == 7
    # a Delete's est counts the 13 tombstone bytes, not its CSR value: 30 + 30 fit 60
    assert sizes(run(ctx, [D(b"a", b"x" * 100), D(b"b", b"y" * 100)], 0, 60, align=align)[0]) == [2]


# ---- many ops ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,align", [(0, 1), (1, 16), (2, 16), (3, 7)])
def test_random_batches_rotate_many_times(ctx, seed, align):
    rng = random.Random(seed)
    keys = [b"", b"a", b"ab", b"abc", b"b", K16 + b"x", K16 + b"y"]
    ops = random_ops(rng, 400, keys=keys)
    nodes = [(b"a", b"1"), (K16 + b"y", TOMB)] if seed % 2 else []
    mem_max = [150, 400, 64, 1000][seed]
    want, _, _ = run(ctx, ops, rng.choice([0, 30, mem_max + 1]), mem_max, nodes=nodes, align=align)
    assert want.nlog > 10 and len(extras(want)) > 20


def test_a_log_past_one_sort_tile(ctx):
    """2,600 ops over up to 50 keys of 1-3 bytes, a third Deletes, mem_max 48 KiB:
    the first log holds more than 1,024 ops, so presence goes through a merge
    pass and the boundary Delete's bisection spans tiles."""
    rng = random.Random(5)
    keys = [bytes(rng.choice(b"abcd") for _ in range(rng.randrange(1, 4))) for _ in range(50)]
    ops = []
    for _ in range(2600):
        k = rng.choice(keys)
        ops.append(D(k) if rng.random() < 1 / 3 else P(k, b"v" * rng.randrange(0, 21)))
    want, _, _ = run(ctx, ops, 0, 48 << 10, nodes=[(keys[0], b"n"), (keys[1], b"n")])
    assert want.nlog >= 2 and want.log_start[1] > lsmgpu.MEMTABLE_TILE
    assert len(extras(want)) > 500


# ---- the call's edges ------------------------------------------------------------------------

def test_no_ops_writes_nothing(ctx):
    batch, kinds = to_device(ctx, [])
    w = lsmgpu.db_write(ctx, batch, kinds, fill=FILL)
    ops = torch.zeros(1, dtype=torch.uint8, device=ctx.torch_device)
    lsmgpu.db_write_into(ctx, batch, ops, w)  # the call itself, n == 0
    torch.cuda.synchronize()
    assert w.meta.cpu().numpy().tolist() == [0] * w.meta.numel()
    assert (w.wal.cpu().numpy() == FILL).all()


def test_overflow(ctx):
    ops = [P(b"k", b"abc")] * 12
    want = ref.write(ops, 0, 50)  # two ops a log
    assert want.nlog == 6
    batch, kinds = to_device(ctx, ops)
    w = lsmgpu.db_write(ctx, batch, kinds, mem_max=50, nlog_max=want.nlog - 1, fill=FILL)
    torch.cuda.synchronize()
    assert w.counts.cpu().numpy().tolist() == [0, 0, 0, 1, 0, 0]
    assert w.result().overflow
    run(ctx, ops, 0, 50, nlog_max=want.nlog)  # exactly enough


@pytest.mark.parametrize("align", ALIGNS)
def test_optional_outputs_null(ctx, align):
    rng = random.Random(11)
    ops = random_ops(rng, 150)
    run(ctx, ops, 0, 200, align=align, desc=False, main_slot=False)
    run(ctx, ops, 0, 200, align=align, desc=False)
    run(ctx, ops, 0, 200, align=align, main_slot=False)


# ---- chaining and the round trip ---------------------------------------------------------------

@pytest.mark.parametrize("seed,cut", [(0, 200), (1, 37), (2, 399)])
def test_two_calls_equal_one(ctx, seed, cut):
    rng = random.Random(20 + seed)
    ops = random_ops(rng, 400, keys=[b"", b"a", b"ab", b"b", K16 + b"x", K16 + b"y"])
    mem_max = [300, 5000, 120][seed]
    whole, _, _ = run(ctx, ops, 0, mem_max)
    _, w1, res1 = run(ctx, ops[:cut], 0, mem_max)
    # the open log's nodes: lsm_memtable_order over the first call's descriptors, no replay
    r, wal_off = w1.replay(res1.nlog)
    mo = lsmgpu.memtable_order(ctx, w1.wal, r, wal_off, res1.most_records, lsmgpu.MEMTABLE_ALL)
    torch.cuda.synchronize()
    per_log, _, over = mo.result()
    assert not over
    fs = np.concatenate([[0], np.cumsum([len(x) for x in per_log])])
    open_log = ref.write(ops[:cut], 0, mem_max).logs[-1]
    cur = (w1.wal, w1.desc, mo.idx[int(fs[-2]):int(fs[-1])])
    nodes = [(k, b"") for k in {k for k, _ in open_log}]
    assert len(nodes) == len(per_log[-1])
    first = ref.write(ops[:cut], 0, mem_max)
    second, _, _ = run(ctx, ops[cut:], res1.mem_size, mem_max, nodes=nodes, cur=cur)
    joined = first.log_bytes()[:-1] + [first.log_bytes()[-1] + second.log_bytes()[0]] + second.log_bytes()[1:]
    assert joined == whole.log_bytes()
    assert second.size == whole.size


def test_round_trip_into_memtable_search(ctx):
    """The produced descriptors go straight into lsm_memtable_order and
    lsm_memtable_search: Manager.Search answers what a dict of the ops holds."""
    rng = random.Random(31)
    keys = [b"", b"a", b"ab", b"abc", b"b", K16 + b"x", K16 + b"y", K40]
    ops = random_ops(rng, 500, keys=keys[:-1])
    _, w, res = run(ctx, ops, 0, 250)
    assert res.nlog > 10
    r, wal_off = w.replay(res.nlog)
    mo = lsmgpu.memtable_order(ctx, w.wal, r, wal_off, res.most_records, lsmgpu.MEMTABLE_ALL)
    kb, ko = csr(keys + [b"zz"])
    probes = lsmgpu.batch_to_device(ctx, kb, ko, np.zeros(1, np.uint8), np.zeros(len(ko), np.uint64))
    got, _, _, val = lsmgpu.memtable_search(ctx, w.wal, r, mo, probes)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    val = val.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
    raw = w.wal.cpu().numpy().tobytes()
    model = ref.dict_model(ops)
    for i, key in enumerate(keys + [b"zz"]):
        if key not in model:
            assert got[i] == MISS
        elif model[key] == TOMB:
            assert got[i] == DELETED
        else:
            o, n = int(val[i]["rec_off"]) + 4, int(val[i]["val_len"])
            assert got[i] == VALUE and raw[o:o + n] == model[key]
