"""CPU tests of lsm_memtable_order's host side (no GPU compute): the symbols,
the argument checks and the workspace formula of include/lsm_gpu.h."""
import lsmgpu
from lsmgpu import _lib

EINVAL, ESPACE = -1, -4


def ws_bytes(nlog, nslot, maxrec):
    return int(_lib.load().lsm_memtable_order_workspace_bytes(nlog, nslot, maxrec))


def order_args(ctx=None, nlog=3, nslot=1000, maxrec=100, scan=0, ws=None, ws_bytes_=0):
    one = 16  # any non-NULL address: the checks under test return before a launch
    return [ctx, one, one, None, one, one, one, nlog, nslot, maxrec, scan, one, one, one, ws, ws_bytes_, None]


def test_symbols_declared_and_abi_stays_7():
    assert {"lsm_memtable_order", "lsm_memtable_order_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 7 and _lib.load().lsm_abi_version() == 7
    assert (lsmgpu.MEMTABLE_ALL, lsmgpu.MEMTABLE_RANGESCAN) == (0, 1)
    assert lsmgpu.MEMTABLE_TILE == 1024


def test_null_ctx_is_einval():
    assert _lib.load().lsm_memtable_order(*order_args(ctx=None)) == EINVAL


def test_unknown_scan_is_einval():
    # a non-NULL context is never dereferenced before the scan check
    for scan in (2, -1, 7):
        assert _lib.load().lsm_memtable_order(*order_args(ctx=16, scan=scan)) == EINVAL


def test_no_logs_is_ok():
    assert _lib.load().lsm_memtable_order(*order_args(ctx=16, nlog=0)) == 0


def test_short_workspace_is_espace():
    need = ws_bytes(3, 1000, 100)
    assert need > 0
    assert _lib.load().lsm_memtable_order(*order_args(ctx=16, ws=16, ws_bytes_=need - 1)) == ESPACE
    assert _lib.load().lsm_memtable_order(*order_args(ctx=16, ws=None, ws_bytes_=need)) == ESPACE


def test_workspace_zero_without_logs():
    assert ws_bytes(0, 0, 0) == 0 and ws_bytes(0, 1 << 20, 1 << 18) == 0


def test_workspace_does_not_decrease():
    prev = 0
    for nslot in (0, 1, 63, 64, 1000, 1 << 16, 1 << 20, 1 << 24):
        cur = ws_bytes(11, nslot, 1 << 18)
        assert cur >= prev and cur >= 24 * nslot
        prev = cur
    prev = 0
    for maxrec in (0, 1, 255, 256, 257, 1024, 1 << 18, 1 << 24):
        cur = ws_bytes(11, 1 << 20, maxrec)
        assert cur >= prev
        prev = cur
    assert ws_bytes(64, 1000, 100) >= ws_bytes(11, 1000, 100) > 0
