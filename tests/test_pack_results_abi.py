"""CPU tests of lsm_pack_results's host side (no GPU compute): the symbols, the
workspace formula and the argument checks of include/lsm_gpu.h, in their
order.  The checks run before the context is used and before any launch, so a
dummy context and dummy device pointers reach every one of them."""
import ctypes

from lsmgpu import _lib

EINVAL, ESPACE = -1, -4

DUMMY = (ctypes.c_uint8 * 256)()
P = ctypes.addressof(DUMMY)

# positions in lsm_pack_results's argument list
CTX, D_BYTES, D_IMG, D_SRC, D_KEY, D_VALUE, D_COUNT, NROW, LIMIT = range(9)
D_KEYS, KEY_CAP, D_VALS, VAL_CAP, ROW_START, ENTRY_SLOT, D_KOFF, D_VOFF, D_COUNTS = range(9, 18)
WS, WS_BYTES, STREAM = 18, 19, 20


def r256(x):
    return (x + 255) // 256 * 256


def formula(n):
    t = (n + 511) // 512 + 1
    return r256(16 * t) + r256(8 * t) + 2 * r256(8 * n)


def ws_bytes(nrow, limit):
    return int(_lib.load().lsm_pack_results_workspace_bytes(nrow, limit))


def call(**over):
    args = [P] * 21
    args[NROW], args[LIMIT] = 4, 16
    args[KEY_CAP], args[VAL_CAP] = 1 << 20, 1 << 20
    args[WS_BYTES] = 1 << 20
    args[STREAM] = None
    for k, v in over.items():
        args[int(k[1:])] = v
    return _lib.load().lsm_pack_results(*args)


def test_symbols_declared():
    assert {"lsm_pack_results", "lsm_pack_results_workspace_bytes"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert hasattr(lib, "lsm_pack_results") and hasattr(lib, "lsm_pack_results_workspace_bytes")
    assert len(_lib.SIGNATURES["lsm_pack_results"][1]) == 21
    assert len(_lib.SIGNATURES["lsm_pack_results_workspace_bytes"][1]) == 2
    assert _lib.ABI_VERSION == 7 and lib.lsm_abi_version() == 7


def test_workspace_bytes():
    # r(16 * t) + r(8 * t) + 2 * r(8 * n), t = ceil(n / 512) + 1, r = round up to 256
    assert ws_bytes(0, 16) == 0 and ws_bytes(16, 0) == 0 and ws_bytes(0, 0) == 0
    assert ws_bytes(1, 1) == 256 + 256 + 2 * 256
    assert ws_bytes(512, 1) == 256 + 256 + 2 * 4096
    assert ws_bytes(513, 1) == 256 + 256 + 2 * 4352
    assert ws_bytes(65536, 16) == 33024 + 16640 + 2 * 8388608          # 2,049 tile sums
    assert ws_bytes(65536, 100) == 205056 + 102656 + 2 * 52428800       # 12,801 tile sums
    assert ws_bytes(1000000, 1) == 31488 + 15872 + 2 * 8000000
    # a function of the product alone
    assert ws_bytes(700, 3) == ws_bytes(3, 700) == ws_bytes(2100, 1) == formula(2100)
    for n in (1, 63, 64, 65, 511, 512, 513, 1025, 4096, (1 << 32) - 1):
        assert ws_bytes(n, 1) == formula(n), n
    # the product leaves 64 bits, or the formula does: no buffer has it
    assert ws_bytes(1 << 60, 16) == 2 ** 64 - 1
    assert ws_bytes(1 << 63, 2) == 2 ** 64 - 1
    assert ws_bytes((1 << 64) - 1, (1 << 32) - 1) == 2 ** 64 - 1
    assert ws_bytes(1 << 62, 1) == 2 ** 64 - 1


def test_check_order():
    assert call(a0=None) == EINVAL                          # ctx == NULL
    assert call(a0=None, a7=0) == EINVAL                    # ... before nrow == 0
    # nrow == 0: 0, before every other check
    assert call(a7=0, a8=0, a5=None, a13=None, a16=None, a17=None, a18=None, a19=0) == 0
    assert call(a8=0) == EINVAL                             # limit == 0
    assert call(a7=1 << 16, a8=1 << 16) == EINVAL           # nrow * limit >= 2^32
    assert call(a7=1 << 32, a8=1) == EINVAL
    assert call(a7=1 << 62, a8=4) == EINVAL                 # ... a product that leaves 64 bits too
    for i in (D_VALUE, ROW_START, D_VOFF, D_COUNTS):        # the required pointers
        assert call(**{"a%d" % i: None}) == EINVAL, i
    assert call(a15=None) == EINVAL                         # d_key without d_koff
    assert call(a4=None) == EINVAL                          # d_keys without d_key
    assert call(a3=None, a2=None) == EINVAL                 # every slot LSM_SRC_SSTABLE and no images
    # EINVAL before ESPACE
    assert call(a8=0, a19=0) == EINVAL
    assert call(a5=None, a18=None) == EINVAL
    assert call(a3=None, a2=None, a19=0) == EINVAL
    # a short or missing workspace
    need = formula(4 * 16)
    assert call(a19=need - 1) == ESPACE
    assert call(a18=None) == ESPACE
    assert call(a7=700, a8=3, a19=formula(2100) - 1) == ESPACE
    # what may be NULL: the checks pass it (the workspace, checked last, is what stops these calls
    # before any launch)
    assert call(a1=None, a19=need - 1) == ESPACE            # d_bytes
    assert call(a2=None, a19=need - 1) == ESPACE            # d_img, with a d_src
    assert call(a3=None, a19=need - 1) == ESPACE            # d_src, with d_img
    assert call(a6=None, a19=need - 1) == ESPACE            # d_count
    assert call(a14=None, a19=need - 1) == ESPACE           # d_entry_slot
    assert call(a4=None, a9=None, a15=None, a19=need - 1) == ESPACE   # no keys: d_key, d_keys, d_koff
    assert call(a9=None, a11=None, a19=need - 1) == ESPACE  # the sizing call
    assert call(a7=(1 << 32) - 1, a8=1, a19=formula((1 << 32) - 1) - 1) == ESPACE
