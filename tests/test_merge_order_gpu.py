"""The merge's ordering stage on the GPU, case by case
(tests/merge_order_cases.py): steps 1-2 of lsm_merge_kvs -- merge_stats_kernel,
merge_long_stats_kernel, the host's plan, the extract, rank and k-way kernels
and the radix passes -- against pyoracle.merge_pairs, in both tie orders and
both descriptor layouts.

Every case is small and built to sit on one edge of the plan choice or of a
kernel (the census in merge_order_cases.py and tests/test_merge_order_cases.py
prove which).  After each call the plan the host reports (lsm_merge_plan) must
equal the census's, word for word: the output alone cannot say which path
ordered it.  The workspace is filled with 0xA5 and the outputs are the walk
suite's sentinel buffers, compared whole (tests/test_merge_walk_gpu.py).
"""
import functools

import numpy as np
import pytest
import torch

import lsmgpu
import pyoracle as ora
import merge_order_cases as mc
import test_merge_walk_gpu as walk_gpu

pytestmark = pytest.mark.gpu

TIES = walk_gpu.TIES
NAMES = [c.name for c in mc.CASES]
LSM_EINVAL = -1


@functools.lru_cache(maxsize=None)
def expected(name, tie):
    return mc.expected(mc.BY_NAME[name], TIES[tie][1])


@functools.lru_cache(maxsize=None)
def plan(name):
    return mc.census(mc.BY_NAME[name]).plan


@functools.lru_cache(maxsize=4)
def laid_out(name, kv):
    buf, kd, vd, _, _ = mc.lay_out(mc.BY_NAME[name].pairs, kv, seed=len(name))
    return buf, kd, vd


def reported_plan(ctx):
    words = np.full(8, 0xEEEEEEEE, np.uint32)
    assert ctx.lib.lsm_merge_plan(ctx.handle, words.ctypes.data) == 0
    return tuple(int(x) for x in words)


@pytest.mark.parametrize("kv", [False, True], ids=["views", "kv"])
@pytest.mark.parametrize("tie", list(TIES))
@pytest.mark.parametrize("name", NAMES)
def test_case(ctx, name, tie, kv):
    case = mc.BY_NAME[name]
    d_buf, d_kd, d_vd = walk_gpu.to_device(ctx, *laid_out(name, kv))
    m = walk_gpu.buffers(ctx, case.n, walk_gpu.workspace(ctx, case.n))
    lsmgpu.merge_kvs_into(ctx, d_buf, d_kd, d_vd, m, level=case.level, threshold=case.threshold,
                          tie=TIES[tie][0])
    torch.cuda.synchronize()
    got = reported_plan(ctx)
    walk_gpu.check_output(*expected(name, tie), m, m.nout, m.nfiles, m.max_recs)
    assert got == plan(name), (got, plan(name))


def test_tie_orders_differ_somewhere():
    """TIE_GOHEAP's expected files come from the oracle alone; the cases hold
    duplicate groups long enough for the heap to leave the input order."""
    assert sum(not np.array_equal(expected(n, "input")[0], expected(n, "goheap")[0])
               for n in ("n4096_path", "three_passes", "path_no_4097_stride_2")) >= 2


@pytest.mark.parametrize("tie", list(TIES))
def test_key_past_the_cap_is_refused(ctx, tie):
    """A key of 1 MiB + 9 bytes is one 8-byte chunk more than kMaxChunks:
    LSM_EINVAL, the outputs keep their sentinels and no plan is reported."""
    case = mc.KEY_PAST_CAP
    assert mc.census(case).plan is None
    buf, kd, vd, _, _ = mc.lay_out(case.pairs, False, seed=1)
    d_buf, d_kd, d_vd = walk_gpu.to_device(ctx, buf, kd, vd)
    m = walk_gpu.buffers(ctx, case.n, walk_gpu.workspace(ctx, case.n))
    with pytest.raises(RuntimeError, match="lsm_merge_kvs_tie failed with code %d$" % LSM_EINVAL):
        lsmgpu.merge_kvs_into(ctx, d_buf, d_kd, d_vd, m, level=case.level, threshold=case.threshold,
                              tie=TIES[tie][0])
    torch.cuda.synchronize()
    assert torch.all(m.out == walk_gpu.OUT_SENTINEL) and torch.all(m.file_start == walk_gpu.START_SENTINEL)
    assert reported_plan(ctx) == (0,) * 8


def test_plan_arguments(ctx):
    words = np.zeros(8, np.uint32)
    assert ctx.lib.lsm_merge_plan(None, words.ctypes.data) == LSM_EINVAL
    assert ctx.lib.lsm_merge_plan(ctx.handle, None) == LSM_EINVAL


@pytest.mark.parametrize("tie", list(TIES))
def test_back_to_back_on_one_workspace(ctx, tie):
    """A merge-path case and a three-pass case, each twice, through one
    workspace with no synchronize of ours between the calls: nothing a call
    leaves in the workspace (the packed keys, the others' indices, the k-way
    starts list in the sort's temporary storage, either perm buffer) may reach
    the next call's order, and each call reports its own plan."""
    a, b = (mc.BY_NAME[x] for x in mc.BACK_TO_BACK)
    assert plan(a.name)[0] == mc.ORDER_PATH and plan(b.name)[3] == 3
    ws = walk_gpu.workspace(ctx, max(a.n, b.n))
    ins = {c.name: walk_gpu.to_device(ctx, *laid_out(c.name, False)) for c in (a, b)}
    runs = []
    for case in (a, b, a, b):
        m = walk_gpu.buffers(ctx, case.n, ws)
        dc = walk_gpu.counts_buffer(ctx)
        d_buf, d_kd, d_vd = ins[case.name]
        lsmgpu.merge_kvs_into(ctx, d_buf, d_kd, d_vd, m, level=case.level, threshold=case.threshold,
                              tie=TIES[tie][0], d_counts=dc)
        runs.append((case.name, m, dc, reported_plan(ctx)))
    torch.cuda.synchronize()
    for name, m, dc, got in runs:
        c = dc.cpu().numpy().view(np.uint64)
        walk_gpu.check_output(*expected(name, tie), m, int(c[0]), int(c[1]), int(c[2]))
        assert got == plan(name), (name, got, plan(name))
