"""CPU tests of lsm_search's host side (no GPU compute): argument checks and
the workspace formula of include/lsm_gpu.h."""
import ctypes

import numpy as np

from lsmgpu import _lib

LEVELS = 7
EINVAL = -1


def starts(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def ws_bytes(counts, nkeys):
    ls = starts(counts)
    return int(_lib.load().lsm_search_workspace_bytes(ls.ctypes.data, nkeys))


def test_symbols_declared():
    assert {"lsm_search", "lsm_search_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 7 and _lib.load().lsm_abi_version() == 7


def test_null_ctx_is_einval():
    ls = starts((2, 4, 8, 0, 0, 0, 0))
    args = [None] * 23
    args[3] = ls.ctypes.data
    args[12] = 5       # nkeys
    args[18] = 0       # tree_nidx
    args[19] = 0       # tree_bytes
    args[21] = 0       # ws_bytes
    assert _lib.load().lsm_search(*args) == EINVAL


def test_workspace_positive_for_a_tree_and_zero_for_none():
    assert ws_bytes((2, 4, 8, 16, 32, 0, 0), 1000) > 0
    assert ws_bytes((0, 0, 0, 0, 0, 0, 1), 1) > 0
    assert ws_bytes((0,) * LEVELS, 1000) == 0


def test_workspace_does_not_depend_on_nkeys():
    """One launch takes every key (one pass, whatever nkeys): the size for the
    launch's 8,192 x 256 threads and for ten times as many keys is the same,
    and the header's 256 bytes."""
    one_pass = 8192 * 256
    for counts in [(2, 4, 8, 16, 32, 0, 0), (2, 3, 5, 0, 2, 1, 0), (0, 1, 0, 0, 0, 0, 0), (9, 0, 0, 0, 0, 0, 0),
                   (0, 2100, 0, 0, 0, 0, 0)]:
        assert ws_bytes(counts, 1) == ws_bytes(counts, one_pass) == ws_bytes(counts, 10 * one_pass) == 256


def test_level_start_must_not_decrease():
    ls = np.array([0, 2, 1, 3, 3, 3, 3, 3], np.uint32)
    assert int(_lib.load().lsm_search_workspace_bytes(ls.ctypes.data, 10)) == 0
