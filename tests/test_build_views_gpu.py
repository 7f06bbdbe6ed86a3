"""lsm_build_sst_views against the oracle, byte for byte, at small shapes:
sst_vregion_runs_kernel (V descriptors) and sst_vregion_views_kernel (KV
descriptors) of encode.hip on the cases of tests/views_cases.py, whose
coverage tests/test_views_cases.py proves on the CPU.

Every build writes into a buffer filled with 0xA5, so besides the images
(each region against pyoracle.build_sst, the only source of expected bytes)
the bytes between and behind the images are checked: the wave-edge writers
exist because the neighbouring bytes belong to someone else.

Not reachable at small shapes, and so not covered here: descriptors at
offsets of 4 GiB or more, and 64 values that together exceed 4 GiB.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lsmgpu
import views_cases as vc

pytestmark = pytest.mark.gpu

FILL = 0xA5
BASE = (20_000, 5)       # one LDS slice, bloom_file_kernel forked, the V region beside it
SHAPES = [
    (1_600_000, 16),     # the split build: bloom_or_kernel, V region on the side stream
    (1_600_000, 17),     # two slices hashed once, not split
    (1_638_401, 7),      # three slices: bloom_slices_kernel, V region on the side stream
]


def _desc(d, dev):
    return torch.from_numpy(d.view(np.int32).reshape(-1, 4).copy()).to(dev)


def upload(ctx, c):
    dev = ctx.torch_device
    keys_only = lsmgpu.codec.RecordBatch(
        keys=lsmgpu.to_device_bytes(c.keys, dev), koff=torch.from_numpy(c.koff.view(np.int64)).to(dev),
        vals=None, voff=torch.from_numpy(c.voff.view(np.int64)).to(dev), n=c.n,
        koff_host=c.koff, voff_host=c.voff)
    return SimpleNamespace(
        buf=lsmgpu.to_device_bytes(c.buf, dev), kd=_desc(c.key_desc, dev),
        vd=None if c.val_desc is None else _desc(c.val_desc, dev),
        idx=torch.from_numpy(c.idx.view(np.int32)).to(dev), batch=keys_only,
        file_start=torch.from_numpy(c.file_start.view(np.int64)).to(dev))


def build_views(ctx, c, up, m, k):
    sb = lsmgpu.prepare_sst_device(ctx, up.batch, up.file_start, c.nfile, c.max_recs,
                                   val_bytes=int(c.voff[-1]), m=m, k=k, align=16)
    sb.out.fill_(FILL)
    lsmgpu.build_sst_views_into(ctx, up.batch, sb, up.buf, up.kd, up.vd, up.idx)
    return sb


def _region(foot, size, at):
    data_off, data_size, idx_off, idx_size = (int(x) for x in foot)
    if at >= size - 32:
        return "footer"
    if at >= idx_off:
        return "index"
    if at >= data_off:
        return "data"
    return "header or filter (the filter block ends at %d)" % data_off


def compare(c, out, file_off, file_size, total, m, k):
    """out (host bytes of the whole output buffer) against the oracle's
    images, and the fill everywhere else."""
    want_off, want_size, _ = c.layout(m, k)
    assert np.array_equal(file_size, want_size), (c.name, file_size, want_size)
    assert np.array_equal(file_off, want_off[:-1]) and total == int(want_off[-1]), (c.name, file_off)
    assert total <= out.size
    owned = np.zeros(out.size, bool)
    for f, (want, foot) in enumerate(c.expected(m, k)):
        o = int(file_off[f])
        owned[o:o + want.size] = True
        got = out[o:o + want.size]
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            at = int(bad[0])
            raise AssertionError(
                f"{c.name} m={m} k={k}: file {f} ({int(c.file_start[f + 1] - c.file_start[f])} records): "
                f"{bad.size} bytes differ, first at {at} of {want.size}, in the {_region(foot, want.size, at)} "
                f"region (data at {int(foot[0])} + {int(foot[1])}): got {got[at:at + 8].tobytes().hex()} "
                f"want {want[at:at + 8].tobytes().hex()}")
    stray = np.nonzero(~owned & (out != FILL))[0]
    assert stray.size == 0, (f"{c.name} m={m} k={k}: {stray.size} bytes outside the images were written, "
                             f"first at {int(stray[0])} (images start at {list(file_off)}, "
                             f"sizes {list(file_size)}, total {total})")


def check_case(ctx, name, m, k):
    c = vc.case(name)
    up = upload(ctx, c)
    sb = build_views(ctx, c, up, m, k)
    torch.cuda.synchronize()
    out = sb.out.cpu().numpy()
    total = int(sb.d_file_off[c.nfile].item())
    compare(c, out, sb.file_off, sb.file_size, total, m, k)
    # lsm_build_sst from a host-gathered copy of the values: the two entry
    # points agree file for file
    full = lsmgpu.batch_to_device(ctx, c.keys, c.koff, c.vals, c.voff)
    sb2 = lsmgpu.prepare_sst_device(ctx, full, up.file_start, c.nfile, c.max_recs, m=m, k=k, align=16)
    lsmgpu.build_sst_into(ctx, full, sb2)
    torch.cuda.synchronize()
    assert np.array_equal(sb2.file_off, sb.file_off) and np.array_equal(sb2.file_size, sb.file_size)
    out2 = sb2.out.cpu().numpy()
    for f in range(c.nfile):
        o, n = int(sb.file_off[f]), int(sb.file_size[f])
        assert np.array_equal(out[o:o + n], out2[o:o + n]), (name, f)


@pytest.mark.parametrize("name", vc.NAMES)
def test_views_build_matches_oracle(ctx, name):
    check_case(ctx, name, *BASE)


@pytest.mark.parametrize("m,k", SHAPES)
@pytest.mark.parametrize("name", vc.SHAPE_NAMES)
def test_views_build_matches_oracle_other_bloom_shapes(ctx, name, m, k):
    check_case(ctx, name, m, k)


@pytest.mark.parametrize("m,k", [BASE, SHAPES[0], SHAPES[2]])
@pytest.mark.parametrize("name", ["fix_mix", "long_kv"])
def test_two_builds_back_to_back(ctx, name, m, k):
    """The same case built twice on one context and one stream with no
    synchronize between the builds, and each output copied on that stream
    right behind its build: a V region still running on the side stream (a
    missing join) would be missing from the copy, or would meet the second
    build's fork."""
    c = vc.case(name)
    up = upload(ctx, c)
    sb1 = build_views(ctx, c, up, m, k)
    snap1 = sb1.out.clone()
    sb2 = build_views(ctx, c, up, m, k)
    snap2 = sb2.out.clone()
    torch.cuda.synchronize()
    for sb, snap in ((sb1, snap1), (sb2, snap2)):
        total = int(sb.d_file_off[c.nfile].item())
        compare(c, snap.cpu().numpy(), sb.file_off, sb.file_size, total, m, k)
        assert torch.equal(sb.out, snap)
