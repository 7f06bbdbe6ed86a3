"""CPU tests of the host side of lsm_memtable_search, its index and lsm_db_get
(no GPU compute): the symbols, the enum values, every argument check of
include/lsm_gpu.h in its stated order, and the size functions."""
import numpy as np

import lsmgpu
from lsmgpu import _lib

EINVAL, ESPACE = -1, -4
ONE = 16  # any non-NULL address: the checks under test return before a launch
NEW = ["lsm_memtable_search", "lsm_memtable_search_index_bytes", "lsm_memtable_search_index_build",
       "lsm_db_get", "lsm_db_get_workspace_bytes"]


def lib():
    return _lib.load()


def index_bytes(n):
    return int(lib().lsm_memtable_search_index_bytes(n))


def search_args(ctx=ONE, nlog=3, index=None, index_bytes_=0, nkeys=5, **null):
    """lsm_memtable_search's arguments; name=None in `null` passes that pointer as NULL."""
    p = dict(bytes=ONE, desc=ONE, idx=ONE, file_start=ONE, keys=ONE, koff=ONE, mem_result=ONE, log=ONE,
             slot=ONE, value=ONE)
    p.update(null)
    return [ctx, p["bytes"], p["desc"], p["idx"], p["file_start"], nlog, index, index_bytes_, p["keys"],
            p["koff"], nkeys, p["mem_result"], p["log"], p["slot"], p["value"], None]


def build_args(ctx=ONE, nlog=3, nnode_max=100, index=ONE, index_bytes_=None, **null):
    p = dict(bytes=ONE, desc=ONE, idx=ONE, file_start=ONE)
    p.update(null)
    if index_bytes_ is None:
        index_bytes_ = index_bytes(nnode_max)
    return [ctx, p["bytes"], p["desc"], p["idx"], p["file_start"], nlog, nnode_max, index, index_bytes_, None]


LEVEL_START = np.array([0, 2, 5, 10, 10, 12, 13, 13], np.uint32)
EMPTY_TREE = np.zeros(8, np.uint32)


def db_args(ctx=ONE, nlog=3, mem_index=None, mem_index_bytes=0, level_start=LEVEL_START, nkeys=5, mode=0,
            ws=ONE, ws_bytes=None, tree=None, tree_nidx=0, tree_bytes=0, **null):
    p = dict(bytes=ONE, desc=ONE, idx=ONE, file_start=ONE, img=ONE, index=ONE, file_off=ONE, file_len=ONE,
             meta=ONE, idx_desc=ONE, idx_value=ONE, keys=ONE, koff=ONE, mem_result=ONE, log=ONE, slot=ONE,
             level=ONE, table=ONE, result=ONE, value=ONE, src=ONE)
    p.update(null)
    ls = None if level_start is None else level_start.ctypes.data
    if ws_bytes is None:
        ws_bytes = int(lib().lsm_db_get_workspace_bytes(ls, nkeys)) if ls else 0
    return [ctx, p["bytes"], p["desc"], p["idx"], p["file_start"], nlog, mem_index, mem_index_bytes,
            p["img"], p["index"], ls, p["file_off"], p["file_len"], p["meta"], None, p["idx_desc"],
            p["idx_value"], tree, tree_nidx, tree_bytes, p["keys"], p["koff"], nkeys, mode,
            p["mem_result"], p["log"], p["slot"], p["level"], p["table"], p["result"], p["value"], p["src"],
            ws, ws_bytes, None]


def test_symbols_declared_and_abi_stays_7():
    assert set(NEW) <= set(_lib.SIGNATURES)
    for name in NEW:
        assert hasattr(lib(), name)
    assert _lib.ABI_VERSION == 7 and lib().lsm_abi_version() == 7


def test_enum_values():
    assert (lsmgpu.MEM_MISS, lsmgpu.MEM_VALUE, lsmgpu.MEM_DELETED) == (0, 1, 2)
    assert (lsmgpu.DBGET_EXACT, lsmgpu.DBGET_TOMBSTONE_HIDES) == (0, 1)
    assert (lsmgpu.SRC_NONE, lsmgpu.SRC_MEMTABLE, lsmgpu.SRC_SSTABLE) == (-1, 0, 1)
    header = open(_lib.LIB_PATH.replace("go-lsm_amd/liblsm_gpu.so", "include/lsm_gpu.h")).read()
    for text in ("LSM_MEM_MISS = 0, LSM_MEM_VALUE = 1, LSM_MEM_DELETED = 2",
                 "LSM_DBGET_EXACT = 0, LSM_DBGET_TOMBSTONE_HIDES = 1",
                 "LSM_SRC_NONE = -1, LSM_SRC_MEMTABLE = 0, LSM_SRC_SSTABLE = 1", "#define LSM_ABI_VERSION 7"):
        assert text in header


# ---- lsm_memtable_search: the checks in their stated order ----------------------

def test_search_null_ctx_comes_first():
    # ... before nkeys == 0, before the pointers, before the index size
    assert lib().lsm_memtable_search(*search_args(ctx=None)) == EINVAL
    assert lib().lsm_memtable_search(*search_args(ctx=None, nkeys=0)) == EINVAL
    assert lib().lsm_memtable_search(*search_args(ctx=None, nkeys=0, nlog=70000, keys=None, index=ONE)) == EINVAL


def test_search_no_keys_is_ok_before_the_other_checks():
    assert lib().lsm_memtable_search(*search_args(nkeys=0)) == 0
    assert lib().lsm_memtable_search(*search_args(nkeys=0, nlog=70000)) == 0
    assert lib().lsm_memtable_search(*search_args(nkeys=0, keys=None, value=None)) == 0
    assert lib().lsm_memtable_search(*search_args(nkeys=0, index=ONE, index_bytes_=1)) == 0


def test_search_too_many_logs_or_a_null_pointer_is_einval():
    assert lib().lsm_memtable_search(*search_args(nlog=65536)) == EINVAL
    for name in ("bytes", "desc", "idx", "file_start", "keys", "koff", "mem_result", "log", "slot", "value"):
        assert lib().lsm_memtable_search(*search_args(**{name: None})) == EINVAL, name
    # ... before the index size: both wrong gives LSM_EINVAL
    assert lib().lsm_memtable_search(*search_args(nlog=65536, index=ONE, index_bytes_=1)) == EINVAL
    assert lib().lsm_memtable_search(*search_args(keys=None, index=ONE, index_bytes_=1)) == EINVAL


def test_search_short_index_is_espace():
    need = index_bytes(1)
    assert need > 0
    for n in (0, 1, need - 1):
        assert lib().lsm_memtable_search(*search_args(index=ONE, index_bytes_=n)) == ESPACE
        assert lib().lsm_memtable_search(*search_args(nlog=0, index=ONE, index_bytes_=n)) == ESPACE


# ---- the index -------------------------------------------------------------------

def test_index_bytes_zero_for_nothing_and_non_decreasing():
    assert index_bytes(0) == 0
    prev = 0
    for n in (1, 2, 63, 64, 1000, 1 << 16, 1 << 20, 1 << 24, (1 << 32) - 2):
        cur = index_bytes(n)
        assert cur >= prev and cur >= 16 * n  # 16 key bytes per node
        prev = cur


def test_index_build_checks():
    assert lib().lsm_memtable_search_index_build(*build_args(ctx=None)) == EINVAL
    assert lib().lsm_memtable_search_index_build(*build_args(ctx=None, nlog=0)) == EINVAL
    assert lib().lsm_memtable_search_index_build(*build_args(nlog=0, index=None)) == 0
    assert lib().lsm_memtable_search_index_build(*build_args(nnode_max=0, index=None)) == 0
    assert lib().lsm_memtable_search_index_build(*build_args(nlog=65536)) == EINVAL
    for name in ("bytes", "desc", "idx", "file_start"):
        assert lib().lsm_memtable_search_index_build(*build_args(**{name: None})) == EINVAL, name
    need = index_bytes(100)
    assert lib().lsm_memtable_search_index_build(*build_args(index_bytes_=need - 1)) == ESPACE
    assert lib().lsm_memtable_search_index_build(*build_args(index=None, index_bytes_=need)) == ESPACE
    assert lib().lsm_memtable_search_index_build(*build_args(idx=None, index_bytes_=need - 1)) == EINVAL


# ---- lsm_db_get ----------------------------------------------------------------------

def test_db_get_workspace_is_lsm_searchs():
    for ls in (LEVEL_START, EMPTY_TREE):
        for nkeys in (0, 1, 1000, 1 << 20):
            assert lib().lsm_db_get_workspace_bytes(ls.ctypes.data, nkeys) == \
                lib().lsm_search_workspace_bytes(ls.ctypes.data, nkeys)
    assert lib().lsm_db_get_workspace_bytes(EMPTY_TREE.ctypes.data, 1000) == 0
    assert lib().lsm_db_get_workspace_bytes(None, 1000) == 0
    prev = 0
    for nkeys in (0, 1, 255, 256, 1 << 20, 1 << 30):
        cur = int(lib().lsm_db_get_workspace_bytes(LEVEL_START.ctypes.data, nkeys))
        assert cur >= prev
        prev = cur
    assert prev > 0


def test_db_get_null_ctx_and_unknown_mode_are_einval():
    assert lib().lsm_db_get(*db_args(ctx=None)) == EINVAL
    assert lib().lsm_db_get(*db_args(ctx=None, nkeys=0)) == EINVAL
    for mode in (2, -1, 7):
        assert lib().lsm_db_get(*db_args(mode=mode)) == EINVAL
        assert lib().lsm_db_get(*db_args(mode=mode, nkeys=0)) == EINVAL


def test_db_get_no_keys_is_ok():
    for mode in (0, 1):
        assert lib().lsm_db_get(*db_args(nkeys=0, mode=mode)) == 0
        assert lib().lsm_db_get(*db_args(nkeys=0, mode=mode, nlog=70000, keys=None, level_start=None)) == 0


def test_db_get_pointer_and_shape_checks():
    assert lib().lsm_db_get(*db_args(level_start=None)) == EINVAL
    bad = LEVEL_START.copy()
    bad[2] = 1
    assert lib().lsm_db_get(*db_args(level_start=bad)) == EINVAL
    assert lib().lsm_db_get(*db_args(nlog=65536)) == EINVAL
    for name in ("bytes", "desc", "idx", "file_start", "img", "index", "file_off", "file_len", "meta",
                 "idx_desc", "idx_value", "keys", "koff", "mem_result", "log", "slot", "level", "table",
                 "result", "value", "src"):
        assert lib().lsm_db_get(*db_args(**{name: None})) == EINVAL, name
    assert lib().lsm_db_get(*db_args(ws=None)) == EINVAL


def test_db_get_short_buffers_are_espace():
    need = int(lib().lsm_db_get_workspace_bytes(LEVEL_START.ctypes.data, 5))
    assert need > 0
    assert lib().lsm_db_get(*db_args(ws_bytes=need - 1)) == ESPACE
    assert lib().lsm_db_get(*db_args(mem_index=ONE, mem_index_bytes=index_bytes(1) - 1)) == ESPACE
    # a Seek tree built for fewer tables
    nfile = int(LEVEL_START[-1])
    tb = int(lib().lsm_level_get_tree_bytes(nfile, 64))
    assert lib().lsm_db_get(*db_args(tree=ONE, tree_nidx=64, tree_bytes=tb - 1)) == ESPACE
    # an empty tree needs neither the tree's buffers nor a workspace: the memtable's checks remain
    none = dict(img=None, index=None, file_off=None, file_len=None, meta=None, idx_desc=None, idx_value=None)
    assert lib().lsm_db_get(*db_args(level_start=EMPTY_TREE, ws=None, ws_bytes=0, mem_index=ONE,
                                     mem_index_bytes=1, **none)) == ESPACE
    assert lib().lsm_db_get(*db_args(level_start=EMPTY_TREE, ws=None, ws_bytes=0, slot=None, **none)) == EINVAL
