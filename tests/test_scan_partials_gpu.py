"""GPU test of scan.h's scan_partials_kernel<T>, the scan of the tile sums
that the planning scans (T = u64) and the merge / gather scans (T = a pair of
sums) share, against numpy.cumsum, exactly.

A tile is 512 values.  The kernel gives each of its 1,024 threads
per = ceil(ntiles / 1024) tiles, read 8 at a time, so the sizes are: nothing;
one value; one tile less one, exactly, plus one; per = 1 with every thread
busy (512 * 1024); per = 2 with idle trailing threads (one more value); and
per = 9, a second round of the 8-wide loop (512 * 8192 + 513)."""
import numpy as np
import pytest
import torch

import lsmgpu

pytestmark = pytest.mark.gpu

TILE = 512
SIZES = [0, 1, TILE - 1, TILE, TILE + 1, TILE * 1024, TILE * 1024 + 1, TILE * 8192 + TILE + 1]


@pytest.fixture(scope="module")
def values():
    """Random block lengths below 70,000, and indices into a 257-pair source
    batch, for the largest size; smaller sizes take a prefix."""
    rng = np.random.default_rng(20)
    return rng.integers(0, 70000, SIZES[-1], dtype=np.uint32), rng.integers(0, 257, SIZES[-1], dtype=np.int32)


def excl(v):
    return np.concatenate([[0], np.cumsum(v.astype(np.uint64), dtype=np.uint64)])


@pytest.mark.parametrize("n", SIZES)
def test_u64_sums_through_plan(ctx, values, n):
    blk_len = values[0][:n]
    d_len = torch.from_numpy(blk_len.view(np.int32).copy()).to(ctx.torch_device)
    p = lsmgpu.plan(ctx, lsmgpu.GRAMMAR_KV, d_len, arena=True)
    torch.cuda.synchronize()
    assert np.array_equal(p.rec_base.cpu().numpy().view(np.uint64), excl(blk_len // 8))
    assert np.array_equal(p.arena_base.cpu().numpy().view(np.uint64), excl(blk_len))


@pytest.mark.parametrize("n", SIZES)
def test_pair_sums_through_gather(ctx, values, n):
    """koff / voff of a gather whose idx repeats the pairs of a small batch."""
    rng = np.random.default_rng(21)
    nsrc = 257
    klen = rng.integers(0, 20, nsrc, dtype=np.uint32)
    vlen = rng.integers(0, 41, nsrc, dtype=np.uint32)
    # keys and values apart, each after 4 bytes of padding (bytes at rec_off + 4)
    kd = np.zeros(nsrc, lsmgpu.DESC_DTYPE)
    vd = np.zeros(nsrc, lsmgpu.DESC_DTYPE)
    parts, pos = [], 0
    for i in range(nsrc):
        kd[i] = (pos, klen[i], 0)
        pos += 4 + int(klen[i])
        vd[i] = (pos, 0, vlen[i])
        pos += 4 + int(vlen[i])
    buf = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    dev = ctx.torch_device
    d_buf = lsmgpu.to_device_bytes(buf, dev)
    d_kd = torch.from_numpy(kd.view(np.int32).reshape(-1, 4).copy()).to(dev)
    d_vd = torch.from_numpy(vd.view(np.int32).reshape(-1, 4).copy()).to(dev)
    idx = values[1][:n]
    koff, voff = excl(klen[idx]), excl(vlen[idx])
    d_idx = torch.from_numpy(idx.copy()).to(dev)
    out = lsmgpu.gather_kvs(ctx, d_buf, d_kd, d_vd, d_idx, n, int(koff[-1]), int(voff[-1]))
    torch.cuda.synchronize()
    assert np.array_equal(out.koff.cpu().numpy().view(np.uint64), koff)
    assert np.array_equal(out.voff.cpu().numpy().view(np.uint64), voff)
    if n:  # the last pair's bytes: the offsets were also the copy's
        j = int(idx[-1])
        ks = int(kd[j]["rec_off"]) + 4
        assert out.keys[int(koff[-2]):int(koff[-1])].cpu().numpy().tobytes() == buf[ks:ks + int(klen[j])].tobytes()
