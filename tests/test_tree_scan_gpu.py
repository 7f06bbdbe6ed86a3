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


def check(ctx, dt, ranges, limit, mode, batch=None, want=None):
    """lsm_tree_scan with and without the Seek tree against the reference
    (want: its scan_batch answer for these ranges, where the caller has it)."""
    ref = dt.host.ref
    assert ref.absent == 0
    wc, wm, widx = want if want is not None else ref.scan_batch(ranges, limit, mode)
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


def test_width_16(ctx):
    """16 sources: the first row's four shifts are the whole minimum."""
    case = cases.width_16()
    assert int(case.tree.level_start[1]) + cases.LEVELS - 1 == 16
    _, emitted = run_case(ctx, case)
    assert emitted > 300


def test_width_17(ctx):
    """17 sources: the full 64-lane minimum, level 6 in lane 16."""
    case = cases.width_17()
    assert int(case.tree.level_start[1]) + cases.LEVELS - 1 == 17
    _, emitted = run_case(ctx, case)
    assert emitted > 300


def test_width_64(ctx):
    """64 sources: every lane of the register path holds a head; a key per
    16-lane row that one source of the row holds alone."""
    case = cases.width_64()
    assert int(case.tree.level_start[1]) + cases.LEVELS - 1 == 64
    _, emitted = run_case(ctx, case)
    assert emitted > 300
    ref = case.tree.ref
    idx, _ = ref.scan(b"row", b"rox", False, 64, RAW)
    assert [int(ref.table[i]) for i in idx] == list(cases.ROW_TABLES)


def test_width_65(ctx):
    """65 sources: the workspace path, level 6 alone in the second round; the
    patched value offsets are emitted with their codes."""
    case = cases.width_65()
    assert int(case.tree.level_start[1]) + cases.LEVELS - 1 == 65
    _, emitted = run_case(ctx, case)
    assert emitted > 300
    ref = case.tree.ref
    assert ref.res[ref.keys.index(b"verr-neg")] == ora.GET_SEEK_FAILED
    assert ref.res[ref.keys.index(b"verr-end")] == ora.GET_VALUE_LENGTH


def test_wide_3rounds(ctx):
    """129 sources: three rounds, one live lane in the last."""
    case = cases.wide_3rounds()
    assert int(case.tree.level_start[1]) + cases.LEVELS - 1 == 129
    _, emitted = run_case(ctx, case)
    assert emitted > 30


def test_damaged(ctx):
    """Tables with a damaged data block (stages 5 and 6) take part, as in
    lsm_search; tables whose index did not decode (stage 4) do not."""
    case = cases.damaged()
    dt, emitted = run_case(ctx, case)
    assert [(int(m["stage"]), int(m["nidx"])) for m in dt.r.meta_numpy()] == cases.DAMAGED_TABLES
    assert emitted > 150
    ref = case.tree.ref
    assert (ref.table[[ref.keys.index(k) for k in (b"d11", b"d12", b"d05", b"d60")]] == [0, 5, 8, 9]).all()


def test_strides(ctx):
    """Both grid-stride loops iterate: the walk's waves take three ranges each
    (the last pass ragged), the Seeks pass 16,384 x 256 (range, source) pairs.
    A pattern of distinct ranges -- full, partial, empty, lo >= hi -- tiled to
    nq; the reference is the pattern's, tiled."""
    for tiled in (cases.strides_walk(), cases.strides_seek()):
        dt = device_tree(ctx, tiled.tree)
        batch = to_ranges(ctx, tiled.ranges)
        for mode in (RAW, LIVE):
            wc, _, _ = check(ctx, dt, tiled.ranges, tiled.limit, mode, batch, want=tiled.want(mode))
            assert wc.size == tiled.nq and wc[-1] == wc[(tiled.nq - 1) % len(tiled.pattern)]


def test_many_ranges(ctx):
    case = cases.many_ranges()
    dt = device_tree(ctx, case.tree)
    batch = to_ranges(ctx, case.ranges)
    for mode in (RAW, LIVE):
        wc, wm, _ = check(ctx, dt, case.ranges, 8, mode, batch)
    assert (wc == 8).sum() > 1000 and (wc == 0).sum() > 300 and wm.sum() > 1000


def test_edges(ctx):
    """An empty tree; nq == 0 leaves the outputs untouched; LSM_ESPACE for a
    short tree buffer and for a workspace one byte short; LSM_EINVAL for
    limit == 0, a bad mode, nq * limit == 2^32 and a decreasing level_start."""
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
    ws = lsmgpu.tree_scan_workspace(ctx, case.tree.level_start, nq)
    assert ws.numel() == nq * (int(case.tree.level_start[1]) + cases.LEVELS - 1) * 32
    with pytest.raises(RuntimeError, match="code -4"):
        lsmgpu.tree_scan_into(ctx, dt.d_img, dt.r, case.tree.level_start, batch, flags, 4, LIVE, dt.index, *out,
                              ws=ws[:ws.numel() - 1])
    # nq * limit == 2^32: refused before anything is read, so the batch's claimed size is never used
    with pytest.raises(RuntimeError, match="code -1"):
        lsmgpu.tree_scan_into(ctx, dt.d_img, dt.r, case.tree.level_start, dataclasses.replace(batch, n=1 << 16),
                              flags, 1 << 16, LIVE, dt.index, *out, ws=ws)
    down = np.array(case.tree.level_start).copy()
    down[3] = down[2] - 1                       # level 2 ends before it starts; the list's end is unchanged
    assert down[-1] == dt.r.nfile
    with pytest.raises(RuntimeError, match="code -1"):
        lsmgpu.tree_scan_into(ctx, dt.d_img, dt.r, down, batch, flags, 4, LIVE, dt.index, *out, ws=ws)
    torch.cuda.synchronize()
    assert all(bool((x == 77).all()) for x in out)
