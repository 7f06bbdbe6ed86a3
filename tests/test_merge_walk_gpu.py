"""The merge file walk on the GPU, case by case (tests/walk_cases.py): steps
3-5 of lsm_merge_kvs -- merge_scan_apply, merge_walk_abs_kernel,
merge_walk_kernel and merge_emit_kernel -- against pyoracle.merge_kvs, in both
tie orders and both descriptor layouts.

Every case is small and built to reach one path of the walk (the census in
walk_cases.py and tests/test_walk_cases.py prove which).  The output buffers
are the caller's own, 64 entries longer than the walk may use and filled with
a sentinel, so a slot written past the last entry shows.
"""
import functools

import numpy as np
import pytest
import torch

import lsmgpu
import pyoracle as ora
import walk_cases as wc

pytestmark = pytest.mark.gpu

SLACK = 64
OUT_SENTINEL = 0x5A5A5A5A          # not an input index: n <= 20,000
START_SENTINEL = 0x5A5A5A5A5A5A5A5A
TIES = {"input": (lsmgpu.TIE_INPUT, ora.TIE_INPUT), "goheap": (lsmgpu.TIE_GOHEAP, ora.TIE_GOHEAP)}
NAMES = [c.name for c in wc.CASES]


@functools.lru_cache(maxsize=None)
def expected(name, tie):
    return wc.expected(wc.BY_NAME[name], TIES[tie][1])


@functools.lru_cache(maxsize=4)
def laid_out(name, kv):
    buf, kd, vd, _, _ = wc.lay_out(wc.BY_NAME[name].pairs, kv, seed=len(name))
    return buf, kd, vd


def upload(ctx, name, kv):
    return to_device(ctx, *laid_out(name, kv))


def to_device(ctx, buf, kd, vd):
    dev = ctx.torch_device
    d_buf = lsmgpu.to_device_bytes(buf, dev)
    d_kd = torch.from_numpy(kd.view(np.int32).reshape(-1, 4).copy()).to(dev)
    d_vd = None if vd is None else torch.from_numpy(vd.view(np.int32).reshape(-1, 4).copy()).to(dev)
    return d_buf, d_kd, d_vd


def workspace(ctx, n):
    """A workspace full of a fixed byte, so that a stale word read by mistake
    is the same word in every run."""
    ws = int(ctx.lib.lsm_merge_kvs_workspace_bytes(n))
    return torch.full((ws,), 0xA5, dtype=torch.uint8, device=ctx.torch_device)


def buffers(ctx, n, ws):
    dev = ctx.torch_device
    out = torch.full((n + SLACK,), OUT_SENTINEL, dtype=torch.int32, device=dev)
    file_start = torch.full((n + 1 + SLACK,), START_SENTINEL, dtype=torch.int64, device=dev)
    return lsmgpu.Merge(out=out, file_start=file_start, workspace=ws, n=n)


def check(name, tie, m, nout, nfiles, max_recs):
    check_output(*expected(name, tie), m, nout, nfiles, max_recs)


def check_output(want, wstarts, m, nout, nfiles, max_recs):
    """The outputs whole: what the oracle wrote, then the sentinels."""
    out = m.out.cpu().numpy().view(np.uint32)
    starts = m.file_start.cpu().numpy().view(np.uint64)
    assert nfiles == wstarts.size - 1 and nout == want.size, (nfiles, wstarts.size - 1, nout, want.size)
    assert np.array_equal(starts[:nfiles + 1], wstarts), (starts[:nfiles + 1][:12], wstarts[:12])
    bad = np.flatnonzero(out[:nout] != want)
    assert bad.size == 0, (bad[:8], out[bad[:8]], want[bad[:8]])
    assert max_recs == wc.most_pairs(wstarts)
    assert np.all(out[nout:] == OUT_SENTINEL), np.flatnonzero(out[nout:] != OUT_SENTINEL)[:8] + nout
    assert np.all(starts[nfiles + 1:] == START_SENTINEL)


@pytest.mark.parametrize("kv", [False, True], ids=["views", "kv"])
@pytest.mark.parametrize("tie", list(TIES))
@pytest.mark.parametrize("name", NAMES)
def test_case(ctx, name, tie, kv):
    case = wc.BY_NAME[name]
    d_buf, d_kd, d_vd = upload(ctx, name, kv)
    m = buffers(ctx, case.n, workspace(ctx, case.n))
    lsmgpu.merge_kvs_into(ctx, d_buf, d_kd, d_vd, m, level=case.level, threshold=case.threshold,
                          tie=TIES[tie][0])
    torch.cuda.synchronize()
    check(name, tie, m, m.nout, m.nfiles, m.max_recs)


def counts_buffer(ctx):
    return torch.full((3,), START_SENTINEL, dtype=torch.int64, device=ctx.torch_device)


@pytest.mark.parametrize("tie", list(TIES))
@pytest.mark.parametrize("name", wc.ASYNC_CASES)
def test_case_async(ctx, name, tie):
    """lsm_merge_kvs_async: the counts stay on the device (written by the emit)."""
    case = wc.BY_NAME[name]
    d_buf, d_kd, d_vd = upload(ctx, name, False)
    m = buffers(ctx, case.n, workspace(ctx, case.n))
    dc = counts_buffer(ctx)
    lsmgpu.merge_kvs_into(ctx, d_buf, d_kd, d_vd, m, level=case.level, threshold=case.threshold,
                          tie=TIES[tie][0], d_counts=dc)
    torch.cuda.synchronize()
    c = dc.cpu().numpy().view(np.uint64)
    check(name, tie, m, int(c[0]), int(c[1]), int(c[2]))


@pytest.mark.parametrize("tie", list(TIES))
def test_back_to_back_on_one_workspace(ctx, tie):
    """Two cases, each twice, through one workspace with no synchronize of
    ours between the calls: nothing a call leaves in the workspace (the
    plateau arrays, phase 1's maps and head, the files, the counts) may reach
    the next call's output."""
    a, b = (wc.BY_NAME[x] for x in wc.BACK_TO_BACK)
    ws = workspace(ctx, max(a.n, b.n))
    ins = {c.name: upload(ctx, c.name, False) for c in (a, b)}
    runs = []
    for case in (a, b, a, b):
        m = buffers(ctx, case.n, ws)
        dc = counts_buffer(ctx)
        d_buf, d_kd, d_vd = ins[case.name]
        lsmgpu.merge_kvs_into(ctx, d_buf, d_kd, d_vd, m, level=case.level, threshold=case.threshold,
                              tie=TIES[tie][0], d_counts=dc)
        runs.append((case.name, m, dc))
    torch.cuda.synchronize()
    for name, m, dc in runs:
        c = dc.cpu().numpy().view(np.uint64)
        check(name, tie, m, int(c[0]), int(c[1]), int(c[2]))
