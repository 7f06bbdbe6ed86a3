"""GPU parity of lsm_tree_scan: the batched range scan over a whole tree
against tests/tree_scan_ref.py (Manager.Search applied to every key the tree
holds in the range; pinned against the iterator walk in
tests/test_tree_scan_ref.py).  Bit-exact on count, more and, per entry, the
key's view, the answering table, the result code and the value's view -- with
the Seek tree and without it, in both modes.
"""
import dataclasses

import numpy as np
import pytest
import torch

import lsmgpu
import pyoracle as ora
import tree_scan_cases as cases
from search_ref import csr
from tree_scan_ref import LIVE, RAW

pytestmark = pytest.mark.gpu


class DeviceTree:
    def __init__(self, ctx, host):
        self.host = host
        self.d_img = lsmgpu.to_device_bytes(host.buf, ctx.torch_device)
        self.r = lsmgpu.decode_sst(ctx, self.d_img, host.offs, host.lens)
        self.index = lsmgpu.level_index(ctx, self.d_img, self.r) if self.r.nfile else None
        self.tree = lsmgpu.level_get_tree(ctx, self.d_img, self.r) if self.r.nfile else None


_trees = {}


def device_tree(ctx, host):
    if id(host) not in _trees:
        _trees[id(host)] = DeviceTree(ctx, host)
    return _trees[id(host)]


def to_ranges(ctx, ranges):
    lb, lo = csr([r[0] for r in ranges])
    hb, ho = csr([r[1] for r in ranges])
    batch = lsmgpu.batch_to_device(ctx, lb if lb.size else np.zeros(1, np.uint8), lo,
                                   hb if hb.size else np.zeros(1, np.uint8), ho)
    flags = np.array([lsmgpu.SCAN_NO_UPPER if r[2] else 0 for r in ranges], np.uint8)
    return batch, flags


def check(ctx, dt, ranges, limit, mode, batch=None):
    """lsm_tree_scan with and without the Seek tree against the reference."""
    ref = dt.host.ref
    assert ref.absent == 0
    wc, wm, widx = ref.scan_batch(ranges, limit, mode)
    if batch is None:
        batch = to_ranges(ctx, ranges)
    sel = widx >= 0
    at = widx[sel]
    for tr in ((None, dt.tree) if dt.tree is not None else (None,)):
        count, more, key, value, table, result = lsmgpu.tree_scan(
            ctx, dt.d_img, dt.r, dt.host.level_start, batch[0], batch[1], limit, mode, index=dt.index, tree=tr)
        torch.cuda.synchronize()
        count = count.cpu().numpy().view(np.uint32)
        more = more.cpu().numpy()
        assert (count == wc).all(), (tr is not None, np.flatnonzero(count != wc)[:8], count[:8], wc[:8])
        assert (more == wm).all(), (tr is not None, np.flatnonzero(more != wm)[:8])
        key = key.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(len(ranges), limit)[sel]
        value = value.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(len(ranges), limit)[sel]
        table = table.cpu().numpy().reshape(len(ranges), limit)[sel]
        result = result.cpu().numpy().reshape(len(ranges), limit)[sel]
        bad = np.flatnonzero((key["rec_off"] != ref.koff[at]) | (key["key_len"] != ref.klen[at]) |
                             (table != ref.table[at]) | (result != ref.res[at]) |
                             (value["rec_off"] != ref.voff[at]) | (value["val_len"] != ref.vlen[at]))
        assert bad.size == 0, (tr is not None, mode, limit, bad.size,
                               [(int(i), ref.keys[at[i]], key[i], table[i], ref.table[at[i]], result[i],
                                 ref.res[at[i]], value[i]) for i in bad[:4]])
        assert (key["val_len"] == 8).all() and (value["key_len"] == 0).all()
    return wc, wm, widx


def run_case(ctx, case):
    dt = device_tree(ctx, case.tree)
    batch = to_ranges(ctx, case.ranges)
    emitted = 0
    for mode in (RAW, LIVE):
        for limit in case.limits:
            wc, _, _ = check(ctx, dt, case.ranges, limit, mode, batch)
            emitted += int(wc.sum())
    return dt, emitted


def test_mixed_tree(ctx):
    case = cases.mixed()
    _, emitted = run_case(ctx, case)
    wc, wm, _ = case.tree.ref.scan_batch(case.ranges, 7, RAW)
    # what makes the comparison meaningful: full, partial and empty ranges, more set and clear
    assert emitted > 5000 and (wc == 7).any() and (wc == 0).sum() >= 3 and wm.any() and not wm.all()
    assert case.tree.ref.scan_batch(case.ranges, 4096, RAW)[0][0] == len(case.tree.ref.keys)


def test_shadowing(ctx):
    case = cases.shadowing()
    dt, _ = run_case(ctx, case)
    ref = case.tree.ref
    batch = to_ranges(ctx, [(b"s", b"u", False), (b"w", b"z", False)])
    out = {}
    for mode in (RAW, LIVE):
        count, more, key, value, table, _ = lsmgpu.tree_scan(ctx, dt.d_img, dt.r, case.tree.level_start,
                                                             batch[0], batch[1], 2, mode, index=dt.index)
        torch.cuda.synchronize()
        value = value.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(2, 2)
        vals = [[case.tree.buf[int(v["rec_off"]) + 4:int(v["rec_off"]) + 4 + int(v["val_len"])].tobytes()
                 for v in value[q][:int(count[q])]] for q in range(2)]
        out[mode] = (count.cpu().tolist(), more.cpu().tolist(), vals, table.cpu().numpy().reshape(2, 2))
    # "s" once, from level-0 table 0; RAW emits level 0's tombstone bytes for "t", LIVE nothing
    assert out[RAW][0][0] == 2 and out[RAW][2][0] == [b"zero-a", cases.TOMB] and (out[RAW][3][0] == 0).all()
    assert out[LIVE][0][0] == 1 and out[LIVE][2][0] == [b"zero-a"] and out[LIVE][1][0] == 0
    # past the limit only tombstones: more is 1 in RAW and 0 in LIVE
    assert out[RAW][0][1] == 2 and out[LIVE][0][1] == 2 and out[RAW][1][1] == 1 and out[LIVE][1][1] == 0
    assert ref.tomb.sum() == 4


def test_level_seams(ctx):
    case = cases.seams()
    run_case(ctx, case)
    ref = case.tree.ref
    idx, _ = ref.scan(b"m5", b"n0", False, 64, RAW)
    assert [ref.keys[i] for i in idx] == [b"m5", b"m9"]
    assert ref.table[idx[1]] == int(case.tree.level_start[2]) + 1   # the later table's entry, once


def test_keys(ctx):
    _, emitted = run_case(ctx, cases.keys_case())
    assert emitted > 50


def test_wide_level0(ctx):
    case = cases.wide_level0()
    assert int(case.tree.level_start[1]) == 70   # more sources than a wave has lanes
    _, emitted = run_case(ctx, case)
    assert emitted > 100


def test_value_errors(ctx):
    case = cases.value_errors()
    run_case(ctx, case)
    ref = case.tree.ref
    assert ref.res[3] == ora.GET_SEEK_FAILED and ref.res[7] == ora.GET_VALUE_LENGTH
    assert ref.voff[3] == 0 and ref.vlen[3] == 0 and ref.voff[7] == 0 and ref.vlen[7] == 0


def test_many_ranges(ctx):
    case = cases.many_ranges()
    dt = device_tree(ctx, case.tree)
    batch = to_ranges(ctx, case.ranges)
    for mode in (RAW, LIVE):
        wc, wm, _ = check(ctx, dt, case.ranges, 8, mode, batch)
    assert (wc == 8).sum() > 1000 and (wc == 0).sum() > 300 and wm.sum() > 1000


def test_edges(ctx):
    """An empty tree; nq == 0 leaves the outputs untouched; LSM_ESPACE for a
    short tree buffer; LSM_EINVAL for limit == 0 and for a bad mode."""
    case = cases.empty_tree()
    dt = device_tree(ctx, case.tree)
    batch, flags = to_ranges(ctx, case.ranges)
    for mode in (RAW, LIVE):
        count, more, *_ = lsmgpu.tree_scan(ctx, dt.d_img, dt.r, case.tree.level_start, batch, flags, 4, mode)
        torch.cuda.synchronize()
        assert count.cpu().tolist() == [0, 0] and more.cpu().tolist() == [0, 0]
    case = cases.mixed()
    dt = device_tree(ctx, case.tree)
    dev = ctx.torch_device
    batch, flags = to_ranges(ctx, case.ranges)
    flags = torch.from_numpy(flags).to(dev)
    nq = len(case.ranges)

    def outputs(limit):
        return [torch.full((nq,), 77, dtype=torch.int32, device=dev),
                torch.full((nq,), 77, dtype=torch.uint8, device=dev),
                torch.full((nq * limit, 4), 77, dtype=torch.int32, device=dev),
                torch.full((nq * limit, 4), 77, dtype=torch.int32, device=dev),
                torch.full((nq * limit,), 77, dtype=torch.int32, device=dev),
                torch.full((nq * limit,), 77, dtype=torch.int32, device=dev)]
    out = outputs(4)
    none = dataclasses.replace(batch, n=0)
    lsmgpu.tree_scan_into(ctx, dt.d_img, dt.r, case.tree.level_start, none, flags, 4, LIVE, dt.index, *out)
    torch.cuda.synchronize()
    assert all(bool((x == 77).all()) for x in out)
    short = lsmgpu.SeekTree(dt.tree.data[:dt.tree.data.numel() // 2], dt.tree.max_nidx)
    with pytest.raises(RuntimeError, match="code -4"):
        lsmgpu.tree_scan_into(ctx, dt.d_img, dt.r, case.tree.level_start, batch, flags, 4, LIVE, dt.index, *out,
                              tree=short)
    with pytest.raises(RuntimeError, match="code -1"):
        lsmgpu.tree_scan_into(ctx, dt.d_img, dt.r, case.tree.level_start, batch, flags, 0, LIVE, dt.index, *out)
    with pytest.raises(RuntimeError, match="code -1"):
        lsmgpu.tree_scan_into(ctx, dt.d_img, dt.r, case.tree.level_start, batch, flags, 4, 2, dt.index, *out)
    torch.cuda.synchronize()
    assert all(bool((x == 77).all()) for x in out)
