"""CPU tests of the host side of lsm_db_write (no GPU compute): the symbols,
the enum values, every argument check of include/lsm_gpu.h in its stated
order, and the size functions."""
import random

import lsmgpu
from lsmgpu import _lib

import db_write_ref as ref
from test_db_write_ref import random_ops, sums

EINVAL, ESPACE = -1, -4
ONE = 16  # any non-NULL address: the checks under test return before a launch
NEW = ["lsm_db_write", "lsm_db_write_max_logs", "lsm_db_write_out_bytes", "lsm_db_write_workspace_bytes"]
REQUIRED = ("keys", "koff", "vals", "voff", "op", "wal", "log_start", "wal_off", "wal_len", "rec_base", "counts")


def lib():
    return _lib.load()


def ws_bytes(n, nlog_max=4, mem_max=1000):
    return int(lib().lsm_db_write_workspace_bytes(n, nlog_max, mem_max))


def args(ctx=ONE, n=5, mem_size0=0, mem_max=1000, cur_nnode=0, nlog_max=4, align=16, ws=ONE, ws_bytes_=None,
         **null):
    """lsm_db_write's arguments; name=None in `null` passes that pointer as NULL."""
    p = dict(keys=ONE, koff=ONE, vals=ONE, voff=ONE, op=ONE, cur_bytes=None, cur_desc=None, cur_idx=None,
             wal=ONE, log_start=ONE, wal_off=ONE, wal_len=ONE, desc=ONE, rec_base=ONE, main_slot=ONE, counts=ONE)
    p.update(null)
    if ws_bytes_ is None:
        ws_bytes_ = ws_bytes(n, min(max(nlog_max, 1), 65535), mem_max)
    return [ctx, p["keys"], p["koff"], p["vals"], p["voff"], p["op"], n, mem_size0, mem_max, p["cur_bytes"],
            p["cur_desc"], p["cur_idx"], cur_nnode, nlog_max, align, p["wal"], p["log_start"], p["wal_off"],
            p["wal_len"], p["desc"], p["rec_base"], p["main_slot"], p["counts"], ws, ws_bytes_, None]


def write(**kw):
    return lib().lsm_db_write(*args(**kw))


def test_symbols_declared_and_abi_stays_7():
    assert set(NEW) <= set(_lib.SIGNATURES)
    for name in NEW:
        assert hasattr(lib(), name)
    assert _lib.ABI_VERSION == 7 and lib().lsm_abi_version() == 7


def test_enum_values():
    assert (lsmgpu.OP_PUT, lsmgpu.OP_DELETE) == (0, 1) == (ref.PUT, ref.DELETE)
    assert lsmgpu.MAX_MEMTABLE_SIZE == 2 * 1024 * 1024
    header = open(_lib.LIB_PATH.replace("go-lsm_amd/liblsm_gpu.so", "include/lsm_gpu.h")).read()
    assert "LSM_OP_PUT = 0, LSM_OP_DELETE = 1" in header and "#define LSM_ABI_VERSION 7" in header


def test_null_ctx_comes_first():
    assert write(ctx=None) == EINVAL
    assert write(ctx=None, n=0) == EINVAL
    assert write(ctx=None, n=0, keys=None, mem_max=0, ws=None, ws_bytes_=0) == EINVAL


def test_no_ops_is_ok_before_the_other_checks():
    assert write(n=0) == 0
    assert write(n=0, keys=None, counts=None, wal=None) == 0
    assert write(n=0, mem_max=0, align=0, nlog_max=0) == 0
    assert write(n=0, cur_idx=ONE) == 0
    assert write(n=0, ws=None, ws_bytes_=0) == 0


def test_null_pointers_and_bad_sizes_are_einval():
    for name in REQUIRED:
        assert write(**{name: None}) == EINVAL, name
    assert write(mem_max=0) == EINVAL
    assert write(mem_max=(1 << 30) + 1) == EINVAL
    assert write(align=0) == EINVAL
    assert write(n=1 << 31, ws_bytes_=1 << 62) == EINVAL
    assert write(nlog_max=0) == EINVAL
    assert write(nlog_max=65536) == EINVAL
    # the current memtable: an index needs its bytes and descriptors, whatever the count
    for cur_nnode in (0, 3):
        assert write(cur_idx=ONE, cur_nnode=cur_nnode) == EINVAL
        assert write(cur_idx=ONE, cur_bytes=ONE, cur_nnode=cur_nnode) == EINVAL
        assert write(cur_idx=ONE, cur_desc=ONE, cur_nnode=cur_nnode) == EINVAL


def test_einval_comes_before_espace():
    assert write(keys=None, ws_bytes_=0) == EINVAL
    assert write(mem_max=0, ws=None) == EINVAL
    assert write(nlog_max=65536, ws_bytes_=1) == EINVAL
    assert write(cur_idx=ONE, ws_bytes_=1) == EINVAL


def test_short_workspace_is_espace():
    need = ws_bytes(5)
    assert need > 0
    for short in (0, 1, need - 1):
        assert write(ws_bytes_=short) == ESPACE
    assert write(ws=None) == ESPACE
    # the optional outputs and an absent memtable are not errors: the workspace check is reached
    assert write(desc=None, main_slot=None, ws_bytes_=need - 1) == ESPACE
    assert write(cur_bytes=ONE, cur_desc=ONE, cur_nnode=9, ws_bytes_=need - 1) == ESPACE
    # the largest accepted values reach it too
    assert write(mem_max=1 << 30, nlog_max=65535, n=(1 << 31) - 1, ws_bytes_=1) == ESPACE


def test_size_functions_are_monotone():
    L = lib()
    assert L.lsm_db_write_workspace_bytes(0, 4, 1000) == 0 and L.lsm_db_write_out_bytes(0, 0, 0, 4, 16) == 0
    prev_ws = prev_out = 0
    for n in (1, 2, 255, 256, 513, 1 << 16, 1 << 20, (1 << 31) - 1):
        cur_ws = int(L.lsm_db_write_workspace_bytes(n, 64, 2 << 20))
        cur_out = int(L.lsm_db_write_out_bytes(n, 16 * n, 100 * n, 64, 16))
        assert cur_ws >= prev_ws and cur_out >= prev_out and cur_ws > 0
        assert cur_out >= 8 * n + 16 * n + 100 * n  # at least the Puts' bytes
        prev_ws, prev_out = cur_ws, cur_out
    prev_ws = prev_out = 0
    for nlog_max in (1, 2, 64, 65535):
        cur_ws = int(L.lsm_db_write_workspace_bytes(1000, nlog_max, 2 << 20))
        cur_out = int(L.lsm_db_write_out_bytes(1000, 16000, 100000, nlog_max, 4096))
        assert cur_ws >= prev_ws and cur_out >= prev_out
        prev_ws, prev_out = cur_ws, cur_out
    for a, b in ((1, 16), (16, 4096)):
        assert L.lsm_db_write_out_bytes(1000, 16000, 100000, 8, a) <= L.lsm_db_write_out_bytes(1000, 16000, 100000, 8, b)
    # more bytes or a fuller memtable never need fewer logs; a larger memtable never more
    assert L.lsm_db_write_max_logs(0, 0, 0, 0, 100) == 1
    for n in (1, 10, 1000, 1 << 20):
        base = L.lsm_db_write_max_logs(n, 16 * n, 100 * n, 0, 2 << 20)
        assert base <= L.lsm_db_write_max_logs(n, 17 * n, 100 * n, 0, 2 << 20)
        assert base <= L.lsm_db_write_max_logs(n, 16 * n, 101 * n, 0, 2 << 20)
        assert base <= L.lsm_db_write_max_logs(n, 16 * n, 100 * n, 5 << 20, 2 << 20)
        assert base >= L.lsm_db_write_max_logs(n, 16 * n, 100 * n, 0, 4 << 20)
        assert base <= n + 1


def test_max_logs_and_out_bytes_bound_the_rule_on_random_batches():
    L = lib()
    rng = random.Random(7)
    for _ in range(600):
        n = rng.randrange(1, 80)
        ops = random_ops(rng, n, p_delete=rng.choice([0, 0.4, 1]))
        mem_max = rng.choice([1, 16, 29, 40, 100, 1000])
        mem_size0 = rng.choice([0, 1, mem_max, mem_max + 7])
        nodes = [b"a", b"ab"] if rng.random() < 0.5 else []
        kb, vb = sums(ops)
        w = ref.write(ops, mem_size0, mem_max, nodes)
        bound = L.lsm_db_write_max_logs(n, kb, vb, mem_size0, mem_max)
        assert bound == ref.max_logs(n, kb, vb, mem_size0, mem_max)
        assert w.nlog <= bound
        for align in (1, 16, 100):
            total = sum((len(b) + align - 1) // align * align for b in w.log_bytes())
            assert total <= L.lsm_db_write_out_bytes(n, kb, vb, bound, align)
