"""CPU tests of lsm_tree_scan's host side (no GPU compute): the symbols, the
workspace formula and the argument checks of include/lsm_gpu.h, in their
order.  The checks run before the context is used and before any launch, so a
dummy context and dummy device pointers reach every one of them."""
import ctypes

import numpy as np

from lsmgpu import _lib

LEVELS = 7
EINVAL, ESPACE = -1, -4


def starts(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def ws_bytes(counts, nq):
    ls = starts(counts)
    return int(_lib.load().lsm_tree_scan_workspace_bytes(ls.ctypes.data, nq))


DUMMY = (ctypes.c_uint8 * 256)()
P = ctypes.addressof(DUMMY)

# positions in lsm_tree_scan's argument list
CTX, LEVEL_START, D_TREE, TREE_NIDX, TREE_BYTES, NQ, LIMIT, MODE, WS, WS_BYTES = 0, 3, 10, 11, 12, 18, 19, 20, 27, 28


def call(counts=(2, 3, 5, 0, 2, 1, 0), **over):
    ls = starts(counts)
    args = [P] * 30
    args[LEVEL_START] = ls.ctypes.data
    args[7] = None                      # d_rec_base
    args[D_TREE], args[TREE_NIDX], args[TREE_BYTES] = None, 0, 0
    args[NQ], args[LIMIT], args[MODE] = 4, 16, 1
    args[WS_BYTES] = 1 << 20
    args[29] = None                     # stream
    for k, v in over.items():
        args[int(k[1:])] = v
    return _lib.load().lsm_tree_scan(*args)


def test_symbols_declared():
    assert {"lsm_tree_scan", "lsm_tree_scan_workspace_bytes"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert hasattr(lib, "lsm_tree_scan") and hasattr(lib, "lsm_tree_scan_workspace_bytes")
    assert len(_lib.SIGNATURES["lsm_tree_scan"][1]) == 30
    assert _lib.ABI_VERSION == 7 and lib.lsm_abi_version() == 7


def test_workspace_bytes():
    bad = np.array([0, 2, 1, 3, 3, 3, 3, 3], np.uint32)
    assert int(_lib.load().lsm_tree_scan_workspace_bytes(bad.ctypes.data, 10)) == 0
    bad = np.array([1, 2, 2, 3, 3, 3, 3, 3], np.uint32)
    assert int(_lib.load().lsm_tree_scan_workspace_bytes(bad.ctypes.data, 10)) == 0
    assert ws_bytes((0,) * LEVELS, 1000) == 0
    # a 32-byte head per range and source (level-0 tables + six levels), left by the Seeks for the walk
    assert ws_bytes((2, 3, 5, 0, 2, 1, 0), 1) == 8 * 32
    assert ws_bytes((2, 3, 5, 0, 2, 1, 0), 5000) == 5000 * 8 * 32
    assert ws_bytes((58, 0, 0, 0, 0, 0, 9), 10 ** 6) == 10 ** 6 * 64 * 32
    assert ws_bytes((70, 1, 0, 0, 0, 0, 0), 4) == 4 * 76 * 32
    assert ws_bytes((0, 0, 0, 0, 0, 0, 1), 1 << 60) == 2 ** 64 - 1   # no buffer has it


def test_check_order():
    assert call(a0=None) == EINVAL                       # ctx == NULL
    assert call(a0=None, a18=0) == EINVAL                # ... before nq == 0
    assert call(a18=0, a19=0, a20=9) == 0                # nq == 0: 0, before every other check
    bad = np.array([0, 2, 1, 3, 3, 3, 3, 3], np.uint32)
    assert call(a3=bad.ctypes.data) == EINVAL
    assert call(a19=0) == EINVAL                         # limit == 0
    assert call(a18=1 << 16, a19=1 << 16) == EINVAL      # nq * limit >= 2^32
    assert call(a18=1 << 33, a19=1) == EINVAL
    assert call(a20=2) == EINVAL and call(a20=-1) == EINVAL   # an unknown mode
    for i in (13, 14, 15, 16, 17, 21, 22, 23, 24, 25, 26):    # lo, hi, flags and the outputs
        assert call(**{"a%d" % i: None}) == EINVAL, i
    for i in (1, 2, 4, 5, 6, 8, 9):                           # a tree input of a non-empty tree
        assert call(**{"a%d" % i: None}) == EINVAL, i
    # EINVAL before ESPACE
    assert call(a19=0, a28=0) == EINVAL
    # a tree buffer built for fewer tables, a short or missing workspace
    lib = _lib.load()
    need = int(lib.lsm_level_get_tree_bytes(13, 300))
    assert need > 0
    assert call(a10=P, a11=300, a12=need - 1) == ESPACE
    assert call(a28=4 * 8 * 32 - 1) == ESPACE
    assert call(a27=None) == ESPACE
    assert call(counts=(70, 1, 0, 0, 0, 0, 0), a28=4 * 76 * 32 - 1) == ESPACE
