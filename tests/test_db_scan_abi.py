"""CPU tests of lsm_db_scan's host side (no GPU compute): the symbols, the
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


def ws_bytes(nlog, counts, nq):
    ls = starts(counts)
    return int(_lib.load().lsm_db_scan_workspace_bytes(nlog, ls.ctypes.data, nq))


DUMMY = (ctypes.c_uint8 * 256)()
P = ctypes.addressof(DUMMY)

# positions in lsm_db_scan's argument list
MEM = (1, 2, 3, 4)                                   # d_bytes, d_desc, d_idx, d_file_start
NLOG, MEM_INDEX, MEM_INDEX_BYTES = 5, 6, 7
TREE = (8, 9, 11, 12, 13, 15, 16)                    # the tree's inputs but d_rec_base / d_tree
LEVEL_START, REC_BASE, D_TREE, TREE_NIDX, TREE_BYTES = 10, 14, 17, 18, 19
RANGES = (20, 21, 22, 23, 24)                        # lo, lo_off, hi, hi_off, flags
NQ, LIMIT, MODE = 25, 26, 27
OUTPUTS = (28, 29, 30, 31, 32, 33, 34)               # count, more, key, value, src, table, result
WS, WS_BYTES, STREAM = 35, 36, 37


def call(counts=(2, 3, 5, 0, 2, 1, 0), **over):
    ls = starts(counts)
    args = [P] * 38
    args[LEVEL_START] = ls.ctypes.data
    args[NLOG], args[MEM_INDEX], args[MEM_INDEX_BYTES] = 3, None, 0
    args[REC_BASE] = None
    args[D_TREE], args[TREE_NIDX], args[TREE_BYTES] = None, 0, 0
    args[NQ], args[LIMIT], args[MODE] = 4, 16, 1
    args[WS_BYTES] = 1 << 20
    args[STREAM] = None
    for k, v in over.items():
        args[int(k[1:])] = v
    return _lib.load().lsm_db_scan(*args)


def test_symbols_declared():
    assert {"lsm_db_scan", "lsm_db_scan_workspace_bytes"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert hasattr(lib, "lsm_db_scan") and hasattr(lib, "lsm_db_scan_workspace_bytes")
    assert len(_lib.SIGNATURES["lsm_db_scan"][1]) == 38
    assert len(_lib.SIGNATURES["lsm_db_scan_workspace_bytes"][1]) == 3
    assert _lib.ABI_VERSION == 7 and lib.lsm_abi_version() == 7


def test_workspace_bytes():
    lib = _lib.load()
    bad = np.array([0, 2, 1, 3, 3, 3, 3, 3], np.uint32)
    assert int(lib.lsm_db_scan_workspace_bytes(4, bad.ctypes.data, 10)) == 0
    bad = np.array([1, 2, 2, 3, 3, 3, 3, 3], np.uint32)
    assert int(lib.lsm_db_scan_workspace_bytes(4, bad.ctypes.data, 10)) == 0
    # both empty: nothing to keep
    assert ws_bytes(0, (0,) * LEVELS, 1000) == 0
    # 32 * nq * (nlog + level_start[1] + 6): a head per range and source
    assert ws_bytes(0, (2, 3, 5, 0, 2, 1, 0), 5000) == 5000 * 8 * 32            # lsm_tree_scan's
    assert ws_bytes(3, (2, 3, 5, 0, 2, 1, 0), 1) == 11 * 32
    assert ws_bytes(3, (2, 3, 5, 0, 2, 1, 0), 5000) == 5000 * 11 * 32
    assert ws_bytes(3, (0,) * LEVELS, 7) == 7 * 9 * 32                           # an empty tree: its six levels stay
    assert ws_bytes(11, (47, 0, 0, 0, 0, 0, 9), 10 ** 6) == 10 ** 6 * 64 * 32
    assert ws_bytes(70, (58, 1, 0, 0, 0, 0, 0), 4) == 4 * 134 * 32
    assert ws_bytes(65535, (0, 0, 0, 0, 0, 0, 1), 0) == 0
    assert ws_bytes(1, (0, 0, 0, 0, 0, 0, 1), 1 << 60) == 2 ** 64 - 1            # no buffer has it
    assert ws_bytes(1, (0,) * LEVELS, 1 << 60) == 2 ** 64 - 1


def test_check_order():
    assert call(a0=None) == EINVAL                       # ctx == NULL
    assert call(a0=None, a25=0) == EINVAL                # ... before nq == 0
    assert call(a25=0, a26=0, a27=9, a5=1 << 20) == 0    # nq == 0: 0, before every other check
    bad = np.array([0, 2, 1, 3, 3, 3, 3, 3], np.uint32)
    assert call(a10=bad.ctypes.data) == EINVAL
    bad = np.array([1, 2, 2, 3, 3, 3, 3, 3], np.uint32)
    assert call(a10=bad.ctypes.data) == EINVAL
    assert call(a26=0) == EINVAL                         # limit == 0
    assert call(a25=1 << 16, a26=1 << 16) == EINVAL      # nq * limit >= 2^32
    assert call(a25=1 << 32, a26=1) == EINVAL            # nq >= 2^32
    assert call(a27=2) == EINVAL and call(a27=-1) == EINVAL   # an unknown mode
    assert call(a5=65536) == EINVAL                      # nlog > 65535
    for i in RANGES + OUTPUTS:                           # d_src included
        assert call(**{"a%d" % i: None}) == EINVAL, i
    for i in MEM:                                        # a memtable input with nlog > 0
        assert call(**{"a%d" % i: None}) == EINVAL, i
    for i in TREE:                                       # a tree input of a non-empty tree
        assert call(**{"a%d" % i: None}) == EINVAL, i
    # EINVAL before ESPACE
    assert call(a26=0, a36=0) == EINVAL
    assert call(a1=None, a6=P, a7=1) == EINVAL
    # an index no node fits, a tree buffer built for fewer tables, a short or missing workspace
    lib = _lib.load()
    assert call(a6=P, a7=int(lib.lsm_memtable_search_index_bytes(1)) - 1) == ESPACE
    need = int(lib.lsm_level_get_tree_bytes(13, 300))
    assert need > 0
    assert call(a17=P, a18=300, a19=need - 1) == ESPACE
    assert call(a36=4 * 11 * 32 - 1) == ESPACE
    assert call(a35=None) == ESPACE
    assert call(counts=(58, 1, 0, 0, 0, 0, 0), a5=70, a36=4 * 134 * 32 - 1) == ESPACE
    # the memtable inputs may be NULL with nlog == 0, the tree's with an empty tree: the checks pass them
    # (the workspace, checked last, is what stops these calls before any launch)
    assert call(a5=0, a1=None, a2=None, a3=None, a4=None, a36=4 * 8 * 32 - 1) == ESPACE
    none_tree = {"a%d" % i: None for i in TREE}
    assert call(counts=(0,) * LEVELS, a36=4 * 9 * 32 - 1, **none_tree) == ESPACE
