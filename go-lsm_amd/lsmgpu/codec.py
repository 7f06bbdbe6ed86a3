"""Python driver of the gfx950 block codec (tests and bench).

Device memory and streams come from PyTorch (plumbing); every computation
runs in liblsm_gpu.so through the C ABI (include/lsm_gpu.h).  Unsigned C
types are carried in signed torch dtypes of the same width (uint64 -> int64,
uint32 -> int32); the bits are what matter.
"""
from dataclasses import dataclass
from typing import Optional

import ctypes
import numpy as np
import torch

from . import _lib

GRAMMAR_V, GRAMMAR_KV, GRAMMAR_IDX = 0, 1, 2

STATUS_NAMES = {
    0: "ok",
    1: "truncated length prefix",
    2: "truncated key",
    3: "key too long",
    4: "truncated value length",
    5: "value too long",
    6: "truncated value",
    7: "index overrun",
    8: "capacity",
}

DESC_DTYPE = np.dtype([("rec_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")])

# go-lsm defaults: bloom.go:79-82, sstable.go:21
DEFAULT_BLOOM_M = 1_600_000
DEFAULT_BLOOM_K = 16
MAX_SSTABLE_SIZE = 2 * 1024 * 1024


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream_handle(stream: Optional[torch.cuda.Stream]):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


INPUT_SLACK = _lib.INPUT_SLACK  # LSM_INPUT_SLACK, include/lsm_gpu.h (checked at load)


def pad16(n: int) -> int:
    """Device inputs must be readable to roundup16(n) + LSM_INPUT_SLACK."""
    return ((n + 15) // 16) * 16 + INPUT_SLACK


def _writable(a: np.ndarray) -> np.ndarray:
    """A contiguous array torch.from_numpy may wrap: read-only inputs (e.g.
    np.frombuffer over bytes) are copied first, since torch cannot mark the
    tensor read-only and warns of undefined behaviour."""
    a = np.ascontiguousarray(a)
    return a if a.flags.writeable else a.copy()


def _dev_i64(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(_writable(a).view(np.int64)).to(dev)


def to_device_bytes(buf: np.ndarray, device) -> torch.Tensor:
    """Copy a host byte array into a 16-byte padded device buffer."""
    n = int(buf.nbytes)
    t = torch.zeros(pad16(n), dtype=torch.uint8, device=device)
    if n:
        t[:n].copy_(torch.from_numpy(_writable(buf).view(np.uint8).reshape(-1)))
    return t


class Context:
    """One lsm_ctx per device (and per host thread in concurrent use)."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        self.device = device
        h = ctypes.c_void_p()
        _lib.check(self.lib.lsm_ctx_create(device, ctypes.byref(h)), "lsm_ctx_create")
        self.handle = h
        self.torch_device = torch.device("cuda", device)

    def close(self):
        if self.handle:
            self.lib.lsm_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_cus(self) -> int:
        return self.lib.lsm_ctx_num_cus(self.handle)


@dataclass
class DecodePlan:
    """Device-side output placement of one batch (lsm_plan_*)."""

    rec_base: torch.Tensor            # int64[nblk+1]
    arena_base: Optional[torch.Tensor]
    workspace: torch.Tensor
    total_records: int                # capacity (rec_base[nblk])


MIN_RECORD = {GRAMMAR_V: 4, GRAMMAR_KV: 8, GRAMMAR_IDX: 12}


@dataclass
class DecodeResult:
    desc: torch.Tensor                # int32[cap, 4] = lsm_rec_desc
    nrec: torch.Tensor                # int32[nblk]
    status: torch.Tensor              # int32[nblk]
    rec_base: Optional[torch.Tensor]  # int64[nblk+1], or None = offset-addressed
    idx_value: Optional[torch.Tensor] = None
    key_arena: Optional[torch.Tensor] = None
    val_arena: Optional[torch.Tensor] = None
    arena_base: Optional[torch.Tensor] = None
    key_arena_off: Optional[torch.Tensor] = None
    val_arena_off: Optional[torch.Tensor] = None

    grammar: int = GRAMMAR_KV

    def desc_numpy(self) -> np.ndarray:
        return self.desc.cpu().numpy().view(np.uint8).view(DESC_DTYPE).reshape(-1)

    def bases(self, blk_off: np.ndarray) -> np.ndarray:
        """Slot of each block's first record (host copy)."""
        if self.rec_base is not None:
            return self.rec_base.cpu().numpy().view(np.uint64)[:-1]
        return np.asarray(blk_off, dtype=np.uint64) // np.uint64(MIN_RECORD[self.grammar])

    def arena_bases(self, blk_off: np.ndarray) -> np.ndarray:
        if self.arena_base is not None:
            return self.arena_base.cpu().numpy().view(np.uint64)[:-1]
        return np.asarray(blk_off, dtype=np.uint64)


def plan(ctx: Context, grammar: int, blk_len: torch.Tensor, arena: bool = False,
         stream=None) -> DecodePlan:
    nblk = int(blk_len.numel())
    dev = ctx.torch_device
    ws = torch.empty(max(int(ctx.lib.lsm_plan_workspace_bytes(nblk)), 16), dtype=torch.uint8,
                     device=dev)
    rec_base = torch.empty(nblk + 1, dtype=torch.int64, device=dev)
    sh = _stream_handle(stream)
    _lib.check(ctx.lib.lsm_plan_rec_base(ctx.handle, grammar, _ptr(blk_len), nblk,
                                         _ptr(rec_base), _ptr(ws), ws.numel(), sh),
               "lsm_plan_rec_base")
    arena_base = None
    if arena:
        arena_base = torch.empty(nblk + 1, dtype=torch.int64, device=dev)
        _lib.check(ctx.lib.lsm_plan_arena_base(ctx.handle, _ptr(blk_len), nblk,
                                               _ptr(arena_base), _ptr(ws), ws.numel(), sh),
                   "lsm_plan_arena_base")
    total = int(rec_base[nblk].item()) if nblk else 0
    return DecodePlan(rec_base, arena_base, ws, total)


def replan(ctx: Context, grammar: int, blk_len: torch.Tensor, p: DecodePlan, stream=None):
    """Recompute rec_base in place (no host sync): the plan step of a timed loop."""
    nblk = int(blk_len.numel())
    _lib.check(ctx.lib.lsm_plan_rec_base(ctx.handle, grammar, _ptr(blk_len), nblk,
                                         _ptr(p.rec_base), _ptr(p.workspace),
                                         p.workspace.numel(), _stream_handle(stream)),
               "lsm_plan_rec_base")
    if p.arena_base is not None:
        _lib.check(ctx.lib.lsm_plan_arena_base(ctx.handle, _ptr(blk_len), nblk, _ptr(p.arena_base),
                                               _ptr(p.workspace), p.workspace.numel(),
                                               _stream_handle(stream)), "lsm_plan_arena_base")


def alloc_decode(ctx: Context, grammar: int, nblk: int, p: DecodePlan,
                 arena: bool = False, arena_offsets: bool = False) -> DecodeResult:
    dev = ctx.torch_device
    cap = max(p.total_records, 1)
    r = DecodeResult(
        desc=torch.empty((cap, 4), dtype=torch.int32, device=dev),
        nrec=torch.empty(max(nblk, 1), dtype=torch.int32, device=dev),
        status=torch.empty(max(nblk, 1), dtype=torch.int32, device=dev),
        rec_base=p.rec_base, grammar=grammar,
    )
    if grammar == GRAMMAR_IDX:
        r.idx_value = torch.empty(cap, dtype=torch.int64, device=dev)
    if arena:
        nbytes = int(p.arena_base[nblk].item()) if nblk else 0
        r.arena_base = p.arena_base
        if grammar != GRAMMAR_V:
            r.key_arena = torch.zeros(pad16(nbytes), dtype=torch.uint8, device=dev)
        if grammar != GRAMMAR_IDX:
            r.val_arena = torch.zeros(pad16(nbytes), dtype=torch.uint8, device=dev)
        if arena_offsets:
            if grammar != GRAMMAR_V:
                r.key_arena_off = torch.empty(cap, dtype=torch.int64, device=dev)
            if grammar != GRAMMAR_IDX:
                r.val_arena_off = torch.empty(cap, dtype=torch.int64, device=dev)
    return r


def alloc_decode_offset(ctx: Context, grammar: int, nblk: int, in_bytes: int,
                        arena: bool = False, arena_offsets: bool = False) -> DecodeResult:
    """Outputs for offset-addressed placement (rec_base = arena_base = NULL):
    block b's records at slots blk_off[b]/R.., its arena bytes at blk_off[b]."""
    dev = ctx.torch_device
    cap = in_bytes // MIN_RECORD[grammar] + 1
    r = DecodeResult(
        desc=torch.empty((cap, 4), dtype=torch.int32, device=dev),
        nrec=torch.empty(max(nblk, 1), dtype=torch.int32, device=dev),
        status=torch.empty(max(nblk, 1), dtype=torch.int32, device=dev),
        rec_base=None, grammar=grammar)
    if grammar == GRAMMAR_IDX:
        r.idx_value = torch.empty(cap, dtype=torch.int64, device=dev)
    if arena:
        if grammar != GRAMMAR_V:
            r.key_arena = torch.zeros(pad16(in_bytes), dtype=torch.uint8, device=dev)
        if grammar != GRAMMAR_IDX:
            r.val_arena = torch.zeros(pad16(in_bytes), dtype=torch.uint8, device=dev)
        if arena_offsets:
            if grammar != GRAMMAR_V:
                r.key_arena_off = torch.empty(cap, dtype=torch.int64, device=dev)
            if grammar != GRAMMAR_IDX:
                r.val_arena_off = torch.empty(cap, dtype=torch.int64, device=dev)
    return r


def _decode_out(r: DecodeResult):
    return _lib.DecodeOut(
        desc=r.desc.data_ptr(),
        rec_base=r.rec_base.data_ptr() if r.rec_base is not None else None,
        nrec=r.nrec.data_ptr(),
        status=r.status.data_ptr(),
        idx_value=r.idx_value.data_ptr() if r.idx_value is not None else None,
        key_arena=r.key_arena.data_ptr() if r.key_arena is not None else None,
        val_arena=r.val_arena.data_ptr() if r.val_arena is not None else None,
        arena_base=r.arena_base.data_ptr() if r.arena_base is not None else None,
        key_arena_off=r.key_arena_off.data_ptr() if r.key_arena_off is not None else None,
        val_arena_off=r.val_arena_off.data_ptr() if r.val_arena_off is not None else None,
    )


def decode_into(ctx: Context, grammar: int, d_in: torch.Tensor, blk_off: torch.Tensor,
                blk_len: torch.Tensor, r: DecodeResult, stream=None,
                schedule: Optional[torch.Tensor] = None, max_blk_len: Optional[int] = None) -> None:
    """lsm_decode_blocks into preallocated outputs (asynchronous).  With a
    `schedule` workspace (schedule_workspace()): lsm_decode_blocks_scheduled,
    the blocks launched largest first (for batches whose sizes vary).  With
    `max_blk_len`: lsm_decode_blocks_hinted (the ring chosen for that bound).
    The two are exclusive: the scheduled path picks its own (2 KiB) ring."""
    if max_blk_len is not None and schedule is not None:
        raise ValueError("decode_into: pass either schedule or max_blk_len, not both")
    out = _decode_out(r)
    if max_blk_len is not None:
        _lib.check(ctx.lib.lsm_decode_blocks_hinted(
            ctx.handle, grammar, _ptr(d_in), _ptr(blk_off), _ptr(blk_len), int(blk_off.numel()),
            int(max_blk_len), ctypes.byref(out), _stream_handle(stream)), "lsm_decode_blocks_hinted")
        return
    if schedule is not None:
        _lib.check(ctx.lib.lsm_decode_blocks_scheduled(
            ctx.handle, grammar, _ptr(d_in), _ptr(blk_off), _ptr(blk_len), int(blk_off.numel()),
            ctypes.byref(out), _ptr(schedule), schedule.numel(), _stream_handle(stream)),
            "lsm_decode_blocks_scheduled")
        return
    _lib.check(ctx.lib.lsm_decode_blocks(ctx.handle, grammar, _ptr(d_in), _ptr(blk_off),
                                         _ptr(blk_len), int(blk_off.numel()), ctypes.byref(out),
                                         _stream_handle(stream)), "lsm_decode_blocks")


def schedule_workspace(ctx: Context, nblk: int) -> torch.Tensor:
    n = int(ctx.lib.lsm_decode_schedule_workspace_bytes(nblk))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def decode_blocks(ctx: Context, grammar: int, d_in: torch.Tensor, blk_off: torch.Tensor,
                  blk_len: torch.Tensor, arena: bool = False, arena_offsets: bool = False,
                  placement: str = "plan", stream=None) -> DecodeResult:
    """placement: "plan" (dense CSR capacity via lsm_plan_*) or "offset"
    (offset-addressed, no plan; blocks must not overlap)."""
    nblk = int(blk_off.numel())
    if placement == "offset":
        r = alloc_decode_offset(ctx, grammar, nblk, int(d_in.numel()), arena=arena,
                                arena_offsets=arena_offsets)
    else:
        p = plan(ctx, grammar, blk_len, arena=arena, stream=stream)
        r = alloc_decode(ctx, grammar, nblk, p, arena=arena, arena_offsets=arena_offsets)
    if nblk:
        decode_into(ctx, grammar, d_in, blk_off, blk_len, r, stream=stream)
    return r


@dataclass
class DenseRecords:
    """lsm_compact_records output: block b's records at desc[base[b]:base[b+1]]."""
    desc: torch.Tensor                # int32[cap, 4]
    base: torch.Tensor                # int64[nblk+1]
    idx_value: Optional[torch.Tensor]
    workspace: torch.Tensor


def alloc_dense(ctx: Context, grammar: int, nblk: int, cap: int) -> DenseRecords:
    dev = ctx.torch_device
    return DenseRecords(
        desc=torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev),
        base=torch.empty(nblk + 1, dtype=torch.int64, device=dev),
        idx_value=torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        if grammar == GRAMMAR_IDX else None,
        workspace=torch.empty(max(int(ctx.lib.lsm_plan_workspace_bytes(nblk)), 16),
                              dtype=torch.uint8, device=dev))


def compact_into(ctx: Context, grammar: int, blk_off: torch.Tensor, r: DecodeResult,
                 d: DenseRecords, stream=None) -> None:
    """lsm_compact_records (asynchronous): the decode's records, dense."""
    out = _decode_out(r)
    _lib.check(ctx.lib.lsm_compact_records(
        ctx.handle, grammar, _ptr(blk_off), int(blk_off.numel()), ctypes.byref(out),
        _ptr(d.desc), _ptr(d.idx_value), _ptr(d.base), _ptr(d.workspace), d.workspace.numel(),
        _stream_handle(stream)), "lsm_compact_records")


def wal_workspace(ctx: Context, nwal: int, max_len: int) -> torch.Tensor:
    n = int(ctx.lib.lsm_wal_replay_workspace_bytes(nwal, max_len))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def wal_replay_into(ctx: Context, d_wal: torch.Tensor, wal_off: torch.Tensor,
                    wal_len: torch.Tensor, max_len: int, r: DecodeResult, ws: torch.Tensor,
                    stream=None) -> None:
    """lsm_wal_replay (wal.Recover, wal/wal.go:95-121) into preallocated outputs."""
    out = _decode_out(r)
    _lib.check(ctx.lib.lsm_wal_replay(ctx.handle, _ptr(d_wal), _ptr(wal_off), _ptr(wal_len),
                                      int(wal_off.numel()), max_len, ctypes.byref(out), _ptr(ws),
                                      ws.numel(), _stream_handle(stream)), "lsm_wal_replay")


def wal_replay(ctx: Context, d_wal: torch.Tensor, wal_off: torch.Tensor, wal_len: torch.Tensor,
               max_len: Optional[int] = None, stream=None) -> DecodeResult:
    """Replay nwal logs; offset-addressed outputs (record slots wal_off/8..)."""
    nwal = int(wal_off.numel())
    if max_len is None:
        max_len = int(wal_len.max().item()) if nwal else 0
    r = alloc_decode_offset(ctx, GRAMMAR_KV, nwal, int(d_wal.numel()))
    if nwal:
        wal_replay_into(ctx, d_wal, wal_off, wal_len, max_len, r,
                        wal_workspace(ctx, nwal, max_len), stream=stream)
    return r


# ---- whole .sst files (lsm_decode_sst) ----------------------------------------

SST_META_DTYPE = np.dtype([
    ("min_key_off", "<u8"), ("min_key_len", "<u8"), ("max_key_off", "<u8"), ("max_key_len", "<u8"),
    ("filter_m", "<u8"), ("filter_k", "<u8"), ("filter_nbits", "<u8"), ("filter_words_off", "<u8"),
    ("data_off", "<i8"), ("data_size", "<i8"), ("idx_off", "<i8"), ("idx_size", "<i8"),
    ("stage", "<i4"), ("status", "<i4"), ("nidx", "<u4"), ("ndata", "<u4")])
assert SST_META_DTYPE.itemsize == 112

SST_STAGE_NAMES = {0: "ok", 1: "header", 2: "filter", 3: "footer", 4: "index", 5: "data",
                   6: "mismatch"}


@dataclass
class SstDecode:
    """lsm_decode_sst outputs: file f's entries at slots base(f).. of the
    per-record arrays (offset addressing: base(f) = file_off[f] // 4)."""
    meta: torch.Tensor        # uint8[nfile * 112] = lsm_sst_meta
    idx_desc: torch.Tensor    # int32[cap, 4]
    idx_value: torch.Tensor   # int64[cap]
    data_desc: torch.Tensor   # int32[cap, 4]
    workspace: torch.Tensor
    d_file_off: torch.Tensor
    d_file_len: torch.Tensor
    file_off: np.ndarray
    nfile: int

    def meta_numpy(self) -> np.ndarray:
        return self.meta.cpu().numpy().view(SST_META_DTYPE).reshape(-1)

    def bases(self) -> np.ndarray:
        return self.file_off // 4


def alloc_sst_decode(ctx: Context, file_off: np.ndarray, file_len: np.ndarray,
                     img_bytes: int) -> SstDecode:
    dev = ctx.torch_device
    file_off = np.ascontiguousarray(file_off, dtype=np.uint64)
    file_len = np.ascontiguousarray(file_len, dtype=np.uint64)
    nf = file_off.size
    cap = img_bytes // 4 + 1
    ws = int(ctx.lib.lsm_decode_sst_workspace_bytes(nf))
    return SstDecode(
        meta=torch.zeros(max(nf, 1) * SST_META_DTYPE.itemsize, dtype=torch.uint8, device=dev),
        idx_desc=torch.zeros((cap, 4), dtype=torch.int32, device=dev),
        idx_value=torch.zeros(cap, dtype=torch.int64, device=dev),
        data_desc=torch.zeros((cap, 4), dtype=torch.int32, device=dev),
        workspace=torch.empty(max(ws, 16), dtype=torch.uint8, device=dev),
        d_file_off=_dev_i64(file_off, dev),
        d_file_len=_dev_i64(file_len, dev),
        file_off=file_off, nfile=nf)


def decode_sst_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, stream=None) -> None:
    _lib.check(ctx.lib.lsm_decode_sst(
        ctx.handle, _ptr(d_img), _ptr(r.d_file_off), _ptr(r.d_file_len), r.nfile, None,
        _ptr(r.meta), _ptr(r.idx_desc), _ptr(r.idx_value), _ptr(r.data_desc), _ptr(r.workspace),
        r.workspace.numel(), _stream_handle(stream)), "lsm_decode_sst")


def decode_sst(ctx: Context, d_img: torch.Tensor, file_off: np.ndarray, file_len: np.ndarray,
               stream=None) -> SstDecode:
    """Decode whole .sst images (SSTable.DecodeFrom + DecodeDataBlock +
    GetKeyValuePairs) held in d_img at file_off[f], file_len[f] bytes each."""
    r = alloc_sst_decode(ctx, file_off, file_len, int(d_img.numel()))
    if r.nfile:
        decode_sst_into(ctx, d_img, r, stream=stream)
    return r


def may_contain_workspace(ctx: Context, nfile: int, nkeys: int) -> torch.Tensor:
    n = int(ctx.lib.lsm_may_contain_workspace_bytes(nfile, nkeys))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def may_contain_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                     hit: torch.Tensor, ws: Optional[torch.Tensor] = None, stream=None) -> None:
    """lsm_may_contain: SSTable.MayContain of every key of `batch` against
    every file decoded into r; hit viewed as uint8[nkeys, nfile]."""
    if ws is None:
        ws = may_contain_workspace(ctx, r.nfile, batch.n)
    _lib.check(ctx.lib.lsm_may_contain(ctx.handle, _ptr(d_img), _ptr(r.d_file_off), _ptr(r.meta),
                                       r.nfile, _ptr(batch.keys), _ptr(batch.koff), batch.n,
                                       _ptr(hit), _ptr(ws), ws.numel(), _stream_handle(stream)),
               "lsm_may_contain")


def may_contain(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                stream=None) -> torch.Tensor:
    hit = torch.zeros((max(batch.n, 1), max(r.nfile, 1)), dtype=torch.uint8,
                      device=ctx.torch_device)
    if batch.n and r.nfile:
        may_contain_into(ctx, d_img, r, batch, hit, stream=stream)
    return hit


def level_may_contain_workspace(ctx: Context, nfile: int, nkeys: int) -> torch.Tensor:
    n = int(ctx.lib.lsm_level_may_contain_workspace_bytes(nfile, nkeys))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def level_index(ctx: Context, d_img: torch.Tensor, r: SstDecode, stream=None) -> torch.Tensor:
    """lsm_level_index_build: the level's sparse index (Manager.sparseIndexes),
    parsed once from the decoded tables' headers; valid with this d_img."""
    idx = torch.empty(max(int(ctx.lib.lsm_level_index_bytes(r.nfile)), 16), dtype=torch.uint8,
                      device=ctx.torch_device)
    if r.nfile:
        _lib.check(ctx.lib.lsm_level_index_build(
            ctx.handle, _ptr(d_img), _ptr(r.d_file_off), _ptr(r.meta), r.nfile, _ptr(idx),
            _stream_handle(stream)), "lsm_level_index_build")
    return idx


def level_may_contain_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                           table: torch.Tensor, may: torch.Tensor,
                           ws: Optional[torch.Tensor] = None, stream=None,
                           index: Optional[torch.Tensor] = None) -> None:
    """lsm_level_may_contain: searchFromLevelWithSparseIndex's candidate table
    (int32 per key, -1 for an empty level) and its MayContain (uint8 per key)
    for a level >= 1 whose tables were decoded into r in sparse-index order.
    index (level_index): lsm_level_may_contain_indexed, the headers not parsed
    again."""
    if ws is None:
        ws = level_may_contain_workspace(ctx, r.nfile, batch.n)
    if index is not None:
        _lib.check(ctx.lib.lsm_level_may_contain_indexed(
            ctx.handle, _ptr(d_img) if r.nfile else None, _ptr(index) if r.nfile else None,
            r.nfile, _ptr(batch.keys), _ptr(batch.koff), batch.n, _ptr(table), _ptr(may), _ptr(ws),
            ws.numel(), _stream_handle(stream)), "lsm_level_may_contain_indexed")
        return
    _lib.check(ctx.lib.lsm_level_may_contain(
        ctx.handle, _ptr(d_img) if r.nfile else None, _ptr(r.d_file_off) if r.nfile else None,
        _ptr(r.meta) if r.nfile else None, r.nfile, _ptr(batch.keys), _ptr(batch.koff), batch.n,
        _ptr(table), _ptr(may), _ptr(ws), ws.numel(), _stream_handle(stream)),
        "lsm_level_may_contain")


def level_may_contain(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                      stream=None):
    """-> (table int32[nkeys], may uint8[nkeys]) on the device."""
    table = torch.empty(max(batch.n, 1), dtype=torch.int32, device=ctx.torch_device)
    may = torch.empty(max(batch.n, 1), dtype=torch.uint8, device=ctx.torch_device)
    if batch.n:
        level_may_contain_into(ctx, d_img, r, batch, table, may, stream=stream)
    return table[:batch.n], may[:batch.n]


GET_ABSENT, GET_FOUND, GET_SEEK_FAILED, GET_VALUE_LENGTH, GET_VALUE_TOO_LONG, GET_VALUE_SHORT = range(6)


@dataclass
class SeekTree:
    """lsm_level_get_tree_build's output for one level: the tree bytes and the
    max_nidx it was built for (tables above it walk the index)."""
    data: torch.Tensor
    max_nidx: int


def level_get_tree(ctx: Context, d_img: torch.Tensor, r: SstDecode, max_nidx: Optional[int] = None,
                   stream=None) -> SeekTree:
    """The level's Seek tree (lsm_level_get_tree_build), built once per level
    load.  max_nidx None = the largest decoded nidx (read back once)."""
    if max_nidx is None:
        max_nidx = int(r.meta_numpy()[:r.nfile]["nidx"].max()) if r.nfile else 0
    nb = int(ctx.lib.lsm_level_get_tree_bytes(r.nfile, max_nidx))
    data = torch.empty(max(nb, 16), dtype=torch.uint8, device=ctx.torch_device)
    if r.nfile and nb:
        _lib.check(ctx.lib.lsm_level_get_tree_build(
            ctx.handle, _ptr(d_img), _ptr(r.d_file_off), _ptr(r.meta), r.nfile, None,
            _ptr(r.idx_desc), max_nidx, _ptr(data), nb, _stream_handle(stream)),
            "lsm_level_get_tree_build")
    return SeekTree(data, max_nidx)


def level_get_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                   table: torch.Tensor, may: torch.Tensor, result: torch.Tensor,
                   value: torch.Tensor, tree: Optional[SeekTree] = None, stream=None) -> None:
    """lsm_level_get: searchFromTable past MayContain for each key with
    may = 1 -- Iterator.Seek over its table's decoded index, then the value
    (GetValueByOffset).  result int32 per key (GET_*), value int32[nkeys, 4]
    (a lsm_rec_desc view of the value in d_img on GET_FOUND).  tree
    (level_get_tree) walks the bisection through the Seek tree; None walks
    the index (the same answers)."""
    _lib.check(ctx.lib.lsm_level_get(
        ctx.handle, _ptr(d_img) if r.nfile else None, _ptr(r.d_file_off) if r.nfile else None,
        _ptr(r.d_file_len) if r.nfile else None, _ptr(r.meta) if r.nfile else None, r.nfile, None,
        _ptr(r.idx_desc) if r.nfile else None, _ptr(r.idx_value) if r.nfile else None,
        _ptr(batch.keys), _ptr(batch.koff), batch.n, _ptr(table), _ptr(may), _ptr(result),
        _ptr(value), _ptr(tree.data) if tree is not None else None,
        tree.max_nidx if tree is not None else 0, tree.data.numel() if tree is not None else 0,
        _stream_handle(stream)), "lsm_level_get")


def level_get(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
              table: torch.Tensor, may: torch.Tensor, tree: Optional[SeekTree] = None,
              stream=None):
    """-> (result int32[nkeys], value int32[nkeys, 4]) on the device."""
    result = torch.empty(max(batch.n, 1), dtype=torch.int32, device=ctx.torch_device)
    value = torch.empty((max(batch.n, 1), 4), dtype=torch.int32, device=ctx.torch_device)
    if batch.n:
        level_get_into(ctx, d_img, r, batch, table, may, result, value, tree=tree, stream=stream)
    return result[:batch.n], value[:batch.n]


def level_search_get_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                          index: torch.Tensor, table: torch.Tensor, may: torch.Tensor,
                          result: torch.Tensor, value: torch.Tensor, tree: Optional[SeekTree] = None,
                          ws: Optional[torch.Tensor] = None, stream=None) -> None:
    """lsm_level_search_get: a level's whole batched Get in one call --
    searchFromLevelWithSparseIndex then searchFromTable -- the outputs of
    level_may_contain_into (table, may) and level_get_into (result, value)."""
    if ws is None:
        ws = level_may_contain_workspace(ctx, r.nfile, batch.n)
    nf = r.nfile
    _lib.check(ctx.lib.lsm_level_search_get(
        ctx.handle, _ptr(d_img) if nf else None, _ptr(index) if nf else None, nf,
        _ptr(r.d_file_off) if nf else None, _ptr(r.d_file_len) if nf else None, _ptr(r.meta) if nf else None,
        None, _ptr(r.idx_desc) if nf else None, _ptr(r.idx_value) if nf else None,
        _ptr(batch.keys), _ptr(batch.koff), batch.n, _ptr(table), _ptr(may), _ptr(result), _ptr(value),
        _ptr(tree.data) if tree is not None else None, tree.max_nidx if tree is not None else 0,
        tree.data.numel() if tree is not None else 0, _ptr(ws), ws.numel(), _stream_handle(stream)),
        "lsm_level_search_get")


def level_search_get(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                     tree: Optional[SeekTree] = None, index: Optional[torch.Tensor] = None, stream=None):
    """-> (table, may, result, value) on the device."""
    dev = ctx.torch_device
    n = max(batch.n, 1)
    table = torch.empty(n, dtype=torch.int32, device=dev)
    may = torch.empty(n, dtype=torch.uint8, device=dev)
    result = torch.empty(n, dtype=torch.int32, device=dev)
    value = torch.empty((n, 4), dtype=torch.int32, device=dev)
    if index is None:
        index = level_index(ctx, d_img, r, stream=stream)
    if batch.n:
        level_search_get_into(ctx, d_img, r, batch, index, table, may, result, value, tree=tree, stream=stream)
    return table[:batch.n], may[:batch.n], result[:batch.n], value[:batch.n]


def level0_get_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
                    table: torch.Tensor, result: torch.Tensor, value: torch.Tensor,
                    tree: Optional[SeekTree] = None, stream=None) -> None:
    """lsm_level0_get: searchFromLevel0 (manager.go:160-176) over r's tables in
    order (newest first): MayContain, Seek and the value per table until the
    first value or error.  table int32 per key (the answering table or -1),
    result / value as level_get_into."""
    _lib.check(ctx.lib.lsm_level0_get(
        ctx.handle, _ptr(d_img) if r.nfile else None, _ptr(r.d_file_off) if r.nfile else None,
        _ptr(r.d_file_len) if r.nfile else None, _ptr(r.meta) if r.nfile else None, r.nfile, None,
        _ptr(r.idx_desc) if r.nfile else None, _ptr(r.idx_value) if r.nfile else None,
        _ptr(batch.keys), _ptr(batch.koff), batch.n, _ptr(table), _ptr(result), _ptr(value),
        _ptr(tree.data) if tree is not None else None, tree.max_nidx if tree is not None else 0,
        tree.data.numel() if tree is not None else 0, _stream_handle(stream)), "lsm_level0_get")


def level0_get(ctx: Context, d_img: torch.Tensor, r: SstDecode, batch: "RecordBatch",
               tree: Optional[SeekTree] = None, stream=None):
    """-> (table int32[nkeys], result int32[nkeys], value int32[nkeys, 4]) on the device."""
    dev = ctx.torch_device
    table = torch.empty(max(batch.n, 1), dtype=torch.int32, device=dev)
    result = torch.empty(max(batch.n, 1), dtype=torch.int32, device=dev)
    value = torch.empty((max(batch.n, 1), 4), dtype=torch.int32, device=dev)
    if batch.n:
        level0_get_into(ctx, d_img, r, batch, table, result, value, tree=tree, stream=stream)
    return table[:batch.n], result[:batch.n], value[:batch.n]


SEARCH_LEVELS = 7  # LSM_SEARCH_LEVELS


def _level_start(level_start) -> np.ndarray:
    ls = np.ascontiguousarray(level_start, dtype=np.uint32)
    if ls.shape != (SEARCH_LEVELS + 1,):
        raise ValueError(f"level_start needs {SEARCH_LEVELS + 1} entries")
    return ls


def search_workspace(ctx: Context, level_start, nkeys: int) -> torch.Tensor:
    ls = _level_start(level_start)
    n = int(ctx.lib.lsm_search_workspace_bytes(ls.ctypes.data, nkeys))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def search_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, level_start, batch: "RecordBatch",
                index: torch.Tensor, level: torch.Tensor, table: torch.Tensor, result: torch.Tensor,
                value: torch.Tensor, tree: Optional[SeekTree] = None,
                ws: Optional[torch.Tensor] = None, stream=None) -> None:
    """lsm_search: Manager.Search (manager.go:99-133) of every key of `batch`
    over the whole tree decoded into r -- tables [level_start[L],
    level_start[L + 1]) are level L, level 0 newest first, the deeper levels in
    sparse-index order.  index = level_index over r, tree = level_get_tree
    over r (or None).  level / table int32 per key (the answering table's level
    and its index in r, -1 when absent), result / value as level_get_into."""
    ls = _level_start(level_start)
    if int(ls[-1]) != r.nfile:
        raise ValueError(f"level_start ends at {int(ls[-1])}, the tree holds {r.nfile} tables")
    if ws is None:
        ws = search_workspace(ctx, ls, batch.n)
    nf = r.nfile
    _lib.check(ctx.lib.lsm_search(
        ctx.handle, _ptr(d_img) if nf else None, _ptr(index) if nf else None, ls.ctypes.data,
        _ptr(r.d_file_off) if nf else None, _ptr(r.d_file_len) if nf else None, _ptr(r.meta) if nf else None,
        None, _ptr(r.idx_desc) if nf else None, _ptr(r.idx_value) if nf else None,
        _ptr(batch.keys), _ptr(batch.koff), batch.n, _ptr(level), _ptr(table), _ptr(result), _ptr(value),
        _ptr(tree.data) if tree is not None else None, tree.max_nidx if tree is not None else 0,
        tree.data.numel() if tree is not None else 0, _ptr(ws), ws.numel(), _stream_handle(stream)),
        "lsm_search")


def search(ctx: Context, d_img: torch.Tensor, r: SstDecode, level_start, batch: "RecordBatch",
           index: Optional[torch.Tensor] = None, tree: Optional[SeekTree] = None, stream=None):
    """-> (level int32[nkeys], table int32[nkeys], result int32[nkeys],
    value int32[nkeys, 4]) on the device."""
    dev = ctx.torch_device
    n = max(batch.n, 1)
    level = torch.empty(n, dtype=torch.int32, device=dev)
    table = torch.empty(n, dtype=torch.int32, device=dev)
    result = torch.empty(n, dtype=torch.int32, device=dev)
    value = torch.empty((n, 4), dtype=torch.int32, device=dev)
    if index is None:
        index = level_index(ctx, d_img, r, stream=stream)
    if batch.n:
        search_into(ctx, d_img, r, level_start, batch, index, level, table, result, value, tree=tree,
                    stream=stream)
    return level[:batch.n], table[:batch.n], result[:batch.n], value[:batch.n]


SCAN_RAW, SCAN_LIVE = 0, 1  # enum lsm_scan_mode
SCAN_NO_UPPER = 1           # LSM_SCAN_NO_UPPER, bit 0 of a range's flags


def _scan_flags(dev, flags, nq: int) -> torch.Tensor:
    """A scan's flags on the device: a uint8 tensor as it is, host values uploaded."""
    if isinstance(flags, torch.Tensor):
        return flags
    f = np.zeros(max(nq, 1), np.uint8)
    f[:nq] = np.asarray(flags, dtype=np.uint8)
    return torch.from_numpy(f).to(dev)


def _scan_outputs(dev, nq: int, limit: int):
    """-> (count, more, key, value, table, result): a scan's output tensors
    (tree_scan_into), none of them empty."""
    n = max(nq * max(limit, 0), 1)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
    return (i32(max(nq, 1)), torch.empty(max(nq, 1), dtype=torch.uint8, device=dev), i32((n, 4)), i32((n, 4)),
            i32(n), i32(n))


def tree_scan_workspace(ctx: Context, level_start, nq: int) -> torch.Tensor:
    ls = _level_start(level_start)
    n = int(ctx.lib.lsm_tree_scan_workspace_bytes(ls.ctypes.data, nq))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def tree_scan_into(ctx: Context, d_img: torch.Tensor, r: SstDecode, level_start, ranges: "RecordBatch",
                   flags: torch.Tensor, limit: int, mode: int, index: torch.Tensor, count: torch.Tensor,
                   more: torch.Tensor, key: torch.Tensor, value: torch.Tensor, table: torch.Tensor,
                   result: torch.Tensor, tree: Optional[SeekTree] = None,
                   ws: Optional[torch.Tensor] = None, stream=None) -> None:
    """lsm_tree_scan: up to `limit` entries of every range over the whole tree
    decoded into r (search_into's tree arguments), in key order, each key
    answered by the table Manager.Search answers it from.  `ranges` is a pair
    of CSRs in one RecordBatch: range q is [keys q, vals q) -- lo in
    ranges.keys / koff, hi in ranges.vals / voff; flags uint8 per range
    (SCAN_NO_UPPER: hi is ignored).  count int32[nq] (uint32 values), more
    uint8[nq]; key / value int32[nq * limit, 4] (lsm_rec_desc), table / result
    int32[nq * limit]: range q's entries at [q * limit, q * limit + count[q])."""
    ls = _level_start(level_start)
    if int(ls[-1]) != r.nfile:
        raise ValueError(f"level_start ends at {int(ls[-1])}, the tree holds {r.nfile} tables")
    if ws is None:
        ws = tree_scan_workspace(ctx, ls, ranges.n)
    nf = r.nfile
    _lib.check(ctx.lib.lsm_tree_scan(
        ctx.handle, _ptr(d_img) if nf else None, _ptr(index) if nf else None, ls.ctypes.data,
        _ptr(r.d_file_off) if nf else None, _ptr(r.d_file_len) if nf else None, _ptr(r.meta) if nf else None,
        None, _ptr(r.idx_desc) if nf else None, _ptr(r.idx_value) if nf else None,
        _ptr(tree.data) if tree is not None else None, tree.max_nidx if tree is not None else 0,
        tree.data.numel() if tree is not None else 0,
        _ptr(ranges.keys), _ptr(ranges.koff), _ptr(ranges.vals), _ptr(ranges.voff), _ptr(flags), ranges.n,
        limit, mode, _ptr(count), _ptr(more), _ptr(key), _ptr(value), _ptr(table), _ptr(result),
        _ptr(ws), ws.numel(), _stream_handle(stream)), "lsm_tree_scan")


def tree_scan(ctx: Context, d_img: torch.Tensor, r: SstDecode, level_start, ranges: "RecordBatch",
              flags, limit: int, mode: int = SCAN_LIVE, index: Optional[torch.Tensor] = None,
              tree: Optional[SeekTree] = None, stream=None):
    """-> (count int32[nq], more uint8[nq], key int32[nq * limit, 4], value
    int32[nq * limit, 4], table int32[nq * limit], result int32[nq * limit])
    on the device.  flags: a uint8 device tensor, or host values to upload."""
    dev = ctx.torch_device
    nq = ranges.n
    count, more, key, value, table, result = _scan_outputs(dev, nq, limit)
    flags = _scan_flags(dev, flags, nq)
    if index is None:
        index = level_index(ctx, d_img, r, stream=stream)
    if nq:
        tree_scan_into(ctx, d_img, r, level_start, ranges, flags, limit, mode, index, count, more, key,
                       value, table, result, tree=tree, stream=stream)
    return count[:nq], more[:nq], key[:nq * limit], value[:nq * limit], table[:nq * limit], result[:nq * limit]


# ---- encode -----------------------------------------------------------------

@dataclass
class RecordBatch:
    """Columnar (CSR) record batch on the device."""

    keys: torch.Tensor   # uint8, 16-byte padded
    koff: torch.Tensor   # int64[n+1]
    vals: torch.Tensor
    voff: torch.Tensor
    n: int
    koff_host: np.ndarray
    voff_host: np.ndarray


def batch_to_device(ctx: Context, keys: np.ndarray, koff: np.ndarray, vals: np.ndarray,
                    voff: np.ndarray) -> RecordBatch:
    dev = ctx.torch_device
    koff = np.ascontiguousarray(koff, dtype=np.uint64)
    voff = np.ascontiguousarray(voff, dtype=np.uint64)
    return RecordBatch(
        keys=to_device_bytes(keys, dev),
        koff=_dev_i64(koff, dev),
        vals=to_device_bytes(vals, dev),
        voff=_dev_i64(voff, dev),
        n=len(koff) - 1, koff_host=koff, voff_host=voff)


def encoded_size(grammar: int, koff: np.ndarray, voff: np.ndarray, r0: int, r1: int) -> int:
    n = r1 - r0
    if grammar == GRAMMAR_V:
        return 4 * n + int(voff[r1] - voff[r0])
    if grammar == GRAMMAR_KV:
        return 8 * n + int(koff[r1] - koff[r0]) + int(voff[r1] - voff[r0])
    return 12 * n + int(koff[r1] - koff[r0])


def encode_blocks(ctx: Context, grammar: int, batch: RecordBatch, rec_start: np.ndarray,
                  out_off: Optional[np.ndarray] = None, out_bytes: Optional[int] = None,
                  idx_off: Optional[np.ndarray] = None, stream=None):
    """Encode block b = records [rec_start[b], rec_start[b+1]) at out_off[b].
    Returns (d_out, out_off)."""
    dev = ctx.torch_device
    rec_start = np.ascontiguousarray(rec_start, dtype=np.uint64)
    nblk = len(rec_start) - 1
    sizes = np.array([encoded_size(grammar, batch.koff_host, batch.voff_host,
                                   int(rec_start[b]), int(rec_start[b + 1]))
                      for b in range(nblk)], dtype=np.uint64)
    if out_off is None:
        out_off = np.zeros(nblk, dtype=np.uint64)
        if nblk:
            out_off[1:] = np.cumsum(sizes)[:-1]
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    if out_bytes is None:
        out_bytes = int((out_off + sizes).max()) if nblk else 0
    d_out = torch.zeros(pad16(out_bytes), dtype=torch.uint8, device=dev)
    d_rs = _dev_i64(rec_start, dev)
    d_oo = _dev_i64(out_off, dev)
    d_io = None
    if grammar == GRAMMAR_IDX:
        d_io = torch.from_numpy(np.ascontiguousarray(idx_off, dtype=np.int64)).to(dev)
    _lib.check(ctx.lib.lsm_encode_blocks(
        ctx.handle, grammar, _ptr(batch.keys), _ptr(batch.koff), _ptr(batch.vals),
        _ptr(batch.voff), _ptr(d_io), _ptr(d_rs), nblk, _ptr(d_out), _ptr(d_oo),
        _stream_handle(stream)), "lsm_encode_blocks")
    return d_out, out_off


# ---- .sst build ---------------------------------------------------------------

def segment_files(ctx: Context, koff: np.ndarray, voff: np.ndarray,
                  threshold: int = MAX_SSTABLE_SIZE) -> np.ndarray:
    koff = np.ascontiguousarray(koff, dtype=np.uint64)
    voff = np.ascontiguousarray(voff, dtype=np.uint64)
    n = len(koff) - 1
    starts = np.zeros(n + 2, dtype=np.uint64)
    nf = ctx.lib.lsm_segment_files_host(koff.ctypes.data, voff.ctypes.data, n, threshold,
                                        starts.ctypes.data)
    return starts[: nf + 1].copy()


class SstBuild:
    """Inputs / outputs of lsm_build_sst for nfile images.  The layout
    (file_start, file_off, file_size) lives on the device; the host copies
    are made on first use (prepare_sst_device computes the layout on the
    device, so nothing is read back before the build)."""

    def __init__(self, out, footer, workspace, d_file_start, d_file_off, max_recs, m, k, nfile,
                 file_start=None, file_off=None, file_size=None, d_file_size=None, stream=None):
        self.out, self.footer, self.workspace = out, footer, workspace
        self.d_file_start, self.d_file_off, self.d_file_size = d_file_start, d_file_off, d_file_size
        self.max_recs, self.m, self.k, self.nfile = max_recs, m, k, nfile
        self._file_start, self._file_off, self._file_size = file_start, file_off, file_size
        self.stream = stream  # the stream the device layout (and the build) run on

    def _host(self, t, n):
        # the layout kernel ran on self.stream, which need not be torch's
        # current stream: wait for it before the first host copy
        if self.stream is not None:
            self.stream.synchronize()
        return t[:n].cpu().numpy().view(np.uint64).copy()

    @property
    def file_start(self) -> np.ndarray:
        if self._file_start is None:
            self._file_start = self._host(self.d_file_start, self.nfile + 1)
        return self._file_start

    @property
    def file_off(self) -> np.ndarray:
        if self._file_off is None:
            self._file_off = self._host(self.d_file_off, self.nfile)
        return self._file_off

    @property
    def file_size(self) -> np.ndarray:
        if self._file_size is None:
            self._file_size = self._host(self.d_file_size, self.nfile)
        return self._file_size


def prepare_sst(ctx: Context, batch: RecordBatch, file_start: np.ndarray,
                m: int = DEFAULT_BLOOM_M, k: int = DEFAULT_BLOOM_K, align: int = 16) -> SstBuild:
    dev = ctx.torch_device
    file_start = np.ascontiguousarray(file_start, dtype=np.uint64)
    nf = len(file_start) - 1
    koff, voff = batch.koff_host, batch.voff_host
    sizes = np.array([ctx.lib.lsm_sst_image_size_host(koff.ctypes.data, voff.ctypes.data,
                                                      int(file_start[f]), int(file_start[f + 1]),
                                                      m) for f in range(nf)], dtype=np.uint64)
    padded = (sizes + (align - 1)) // align * align
    file_off = np.zeros(nf, dtype=np.uint64)
    if nf:
        file_off[1:] = np.cumsum(padded)[:-1]
    total = int(padded.sum())
    max_recs = int(np.diff(file_start.astype(np.int64)).max()) if nf else 0
    ws_bytes = int(ctx.lib.lsm_build_sst_workspace_bytes(nf, max_recs, m, k))
    return SstBuild(
        out=torch.zeros(pad16(total), dtype=torch.uint8, device=dev),
        file_start=file_start, file_off=file_off, file_size=sizes,
        footer=torch.zeros(max(nf, 1) * 4, dtype=torch.int64, device=dev),
        workspace=torch.empty(ws_bytes, dtype=torch.uint8, device=dev),
        d_file_start=_dev_i64(file_start, dev),
        d_file_off=_dev_i64(file_off, dev),
        max_recs=max_recs, m=m, k=k, nfile=nf)


def build_sst_into(ctx: Context, batch: RecordBatch, sb: SstBuild, stream=None) -> None:
    nf = sb.nfile
    _lib.check(ctx.lib.lsm_build_sst(
        ctx.handle, _ptr(batch.keys), _ptr(batch.koff), _ptr(batch.vals), _ptr(batch.voff),
        _ptr(sb.d_file_start), nf, sb.max_recs, sb.m, sb.k, _ptr(sb.out), _ptr(sb.d_file_off),
        _ptr(sb.footer), _ptr(sb.workspace), sb.workspace.numel(), _stream_handle(stream)),
        "lsm_build_sst")


def build_sst(ctx: Context, batch: RecordBatch, file_start: np.ndarray,
              m: int = DEFAULT_BLOOM_M, k: int = DEFAULT_BLOOM_K, stream=None) -> SstBuild:
    sb = prepare_sst(ctx, batch, file_start, m=m, k=k)
    build_sst_into(ctx, batch, sb, stream=stream)
    return sb


class SstStream:
    """lsm_build_sst_stream's buffers for one sorted stream: the rule, the
    layout and the images in one call, sized on lsm_stream_max_files' bound.
    The counts stay on the device ({nfile, most records in a file, image
    bytes, overflow}); result() reads them back after the build."""

    def __init__(self, ctx, batch, threshold, m, k, align):
        dev = ctx.torch_device
        lib = ctx.lib
        n = batch.n
        kb, vb = int(batch.keys.numel()), int(batch.vals.numel())
        self.threshold, self.m, self.k, self.align, self.n = threshold, m, k, align, n
        self.nfile_max = int(lib.lsm_stream_max_files(n, kb, vb, threshold))
        out_bytes = int(lib.lsm_build_sst_stream_out_bytes(n, kb, vb, self.nfile_max, m, align))
        ws = int(lib.lsm_build_sst_stream_workspace_bytes(n, threshold, self.nfile_max, m, k))
        self.out = torch.empty(pad16(max(out_bytes, 1)), dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(max(ws, 16), dtype=torch.uint8, device=dev)
        self.d_file_start = torch.empty(self.nfile_max + 1, dtype=torch.int64, device=dev)
        self.d_file_off = torch.empty(self.nfile_max + 1, dtype=torch.int64, device=dev)
        self.footer = torch.empty(max(self.nfile_max, 1) * 4, dtype=torch.int64, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        self._koff, self._voff = batch.koff, batch.voff
        self._filter = int(lib.lsm_filter_block_size(m))

    def result(self) -> "SstBuild":
        """The build as an SstBuild with host copies of its layout (reads
        back; raises on overflow)."""
        torch.cuda.synchronize(self.out.device)
        c = self.counts.cpu().numpy().view(np.uint64)
        if int(c[3]):
            raise RuntimeError("lsm_build_sst_stream: the stream needs more than nfile_max files")
        nf = int(c[0])
        fs = self.d_file_start[:nf + 1].cpu().numpy().view(np.uint64).copy()
        fo = self.d_file_off[:nf + 1].cpu().numpy().view(np.uint64).copy()
        # image sizes (sstable.go:131-193) from the device offsets
        ko, vo = self._koff, self._voff
        r0, r1 = self.d_file_start[:nf], self.d_file_start[1:nf + 1]
        sz = (8 + (ko[r0 + 1] - ko[r0]) + (ko[r1] - ko[r1 - 1]) + self._filter + 16 * (r1 - r0) +
              (ko[r1] - ko[r0]) + (vo[r1] - vo[r0]) + 32) if nf else torch.zeros(0, dtype=torch.int64)
        return SstBuild(out=self.out, footer=self.footer, workspace=self.workspace,
                        d_file_start=self.d_file_start[:nf + 1], d_file_off=self.d_file_off[:nf + 1],
                        max_recs=int(c[1]), m=self.m, k=self.k, nfile=nf, file_start=fs,
                        file_off=fo[:nf], file_size=sz.cpu().numpy().view(np.uint64).copy(),
                        d_file_size=None)


def prepare_sst_stream(ctx: Context, batch: RecordBatch, threshold: int = MAX_SSTABLE_SIZE,
                       m: int = DEFAULT_BLOOM_M, k: int = DEFAULT_BLOOM_K, align: int = 16) -> SstStream:
    return SstStream(ctx, batch, threshold, m, k, align)


def build_sst_stream_into(ctx: Context, batch: RecordBatch, ss: SstStream, stream=None) -> None:
    """lsm_build_sst_stream: Builder.Add / ShouldFlush / Build over the sorted
    stream (merge.go:106-128) with SSTable.EncodeTo and Filter.Add per file."""
    _lib.check(ctx.lib.lsm_build_sst_stream(
        ctx.handle, _ptr(batch.keys), _ptr(batch.koff), _ptr(batch.vals), _ptr(batch.voff), batch.n,
        ss.threshold, ss.nfile_max, ss.m, ss.k, ss.align, _ptr(ss.out), _ptr(ss.d_file_start),
        _ptr(ss.d_file_off), _ptr(ss.footer), _ptr(ss.counts), _ptr(ss.workspace),
        ss.workspace.numel(), _stream_handle(stream)), "lsm_build_sst_stream")


def build_sst_stream(ctx: Context, batch: RecordBatch, threshold: int = MAX_SSTABLE_SIZE,
                     m: int = DEFAULT_BLOOM_M, k: int = DEFAULT_BLOOM_K, align: int = 16,
                     stream=None) -> SstStream:
    ss = prepare_sst_stream(ctx, batch, threshold, m, k, align)
    build_sst_stream_into(ctx, batch, ss, stream=stream)
    return ss


def segment_files_device(ctx: Context, batch: RecordBatch, threshold: int = MAX_SSTABLE_SIZE,
                         nfile_max: Optional[int] = None, stream=None):
    """lsm_segment_files (the builder rule on the device) -> (file starts as a
    host array, counts {nfile, most records in a file, 0, overflow})."""
    dev = ctx.torch_device
    if nfile_max is None:
        nfile_max = int(ctx.lib.lsm_stream_max_files(batch.n, int(batch.keys.numel()),
                                                     int(batch.vals.numel()), threshold))
    fs = torch.full((nfile_max + 1,), -1, dtype=torch.int64, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    _lib.check(ctx.lib.lsm_segment_files(ctx.handle, _ptr(batch.koff), _ptr(batch.voff), batch.n,
                                         threshold, nfile_max, _ptr(fs), _ptr(counts),
                                         _stream_handle(stream)), "lsm_segment_files")
    torch.cuda.synchronize(dev)
    c = counts.cpu().numpy().view(np.uint64).copy()
    return fs[:int(c[0]) + 1].cpu().numpy().view(np.uint64).copy(), c


def sum256(ctx: Context, batch: RecordBatch, stream=None) -> torch.Tensor:
    out = torch.empty((max(batch.n, 1), 4), dtype=torch.int64, device=ctx.torch_device)
    _lib.check(ctx.lib.lsm_sum256(ctx.handle, _ptr(batch.keys), _ptr(batch.koff), batch.n,
                                  _ptr(out), _stream_handle(stream)), "lsm_sum256")
    return out


def bloom_probe(ctx: Context, words: torch.Tensor, m: int, k: int, batch: RecordBatch,
                stream=None) -> torch.Tensor:
    hit = torch.empty(max(batch.n, 1), dtype=torch.uint8, device=ctx.torch_device)
    _lib.check(ctx.lib.lsm_bloom_probe(ctx.handle, _ptr(words), m, k, _ptr(batch.keys),
                                       _ptr(batch.koff), batch.n, _ptr(hit),
                                       _stream_handle(stream)), "lsm_bloom_probe")
    return hit


# ---- compaction merge ------------------------------------

TOMBSTONE = "～DELETED～".encode()  # kv.DeletedValue (kv/kv.go:29)


@dataclass
class Merge:
    """lsm_merge_kvs outputs: out[:nout] = input indices of the written pairs,
    file_start[:nfiles + 1] = each file's first position in out."""
    out: torch.Tensor         # int32[n] (u32 indices)
    file_start: torch.Tensor  # int64[n + 1]
    workspace: torch.Tensor
    n: int
    nout: int = 0
    nfiles: int = 0
    max_recs: int = 0  # the most pairs in one output file


def alloc_merge(ctx: Context, n: int) -> Merge:
    dev = ctx.torch_device
    ws = int(ctx.lib.lsm_merge_kvs_workspace_bytes(n))
    return Merge(out=torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                 file_start=torch.empty(n + 1, dtype=torch.int64, device=dev),
                 workspace=torch.empty(ws, dtype=torch.uint8, device=dev), n=n)


TIE_INPUT, TIE_GOHEAP = 0, 1  # enum lsm_tie


def merge_kvs_into(ctx: Context, d_bytes: torch.Tensor, key_desc: torch.Tensor,
                   val_desc: Optional[torch.Tensor], r: Merge, level: int = 1,
                   threshold: int = MAX_SSTABLE_SIZE, stream=None, tie: int = TIE_INPUT,
                   d_counts: Optional[torch.Tensor] = None) -> Merge:
    """CompactAndMergeKVs (merge.go:42-94) over pairs given as descriptors
    (key: IDX/KV descriptor, value: V descriptor or None for KV records).
    tie=TIE_GOHEAP: equal keys in container/heap's pop order (exact).
    d_counts (device int64[3]): lsm_merge_kvs_async -- the counts are left
    there, not read back (r.nout / nfiles / max_recs are not set)."""
    if d_counts is not None:
        _lib.check(ctx.lib.lsm_merge_kvs_async(
            ctx.handle, _ptr(d_bytes), _ptr(key_desc), _ptr(val_desc), r.n, level, threshold, tie,
            _ptr(r.out), _ptr(r.file_start), _ptr(d_counts), _ptr(r.workspace),
            r.workspace.numel(), _stream_handle(stream)), "lsm_merge_kvs_async")
        return r
    counts = np.zeros(3, np.uint64)
    _lib.check(ctx.lib.lsm_merge_kvs_tie(
        ctx.handle, _ptr(d_bytes), _ptr(key_desc), _ptr(val_desc), r.n, level, threshold, tie,
        _ptr(r.out), _ptr(r.file_start), counts.ctypes.data, _ptr(r.workspace),
        r.workspace.numel(), _stream_handle(stream)), "lsm_merge_kvs_tie")
    r.nout, r.nfiles, r.max_recs = int(counts[0]), int(counts[1]), int(counts[2])
    return r


def merge_kvs(ctx: Context, d_bytes: torch.Tensor, key_desc: torch.Tensor,
              val_desc: Optional[torch.Tensor], level: int = 1,
              threshold: int = MAX_SSTABLE_SIZE, stream=None, tie: int = TIE_INPUT) -> Merge:
    r = alloc_merge(ctx, int(key_desc.shape[0]))
    return merge_kvs_into(ctx, d_bytes, key_desc, val_desc, r, level, threshold, stream, tie)


def goheap_pop_order(ctx_or_lib, rank: np.ndarray, phases: bool = False):
    """lsm_goheap_pop_order_host: container/heap's pop order over key ranks.
    phases=True -> (order, push_ms, pop_ms)."""
    lib = ctx_or_lib.lib if isinstance(ctx_or_lib, Context) else ctx_or_lib
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    order = np.zeros(max(rank.size, 1), np.uint32)
    ns = np.zeros(2, np.uint64)
    _lib.check(lib.lsm_goheap_pop_order_host(rank.ctypes.data, rank.size, order.ctypes.data, ns.ctypes.data),
               "lsm_goheap_pop_order_host")
    if phases:
        return order[:rank.size], float(ns[0]) / 1e6, float(ns[1]) / 1e6
    return order[:rank.size]


def gather_kvs(ctx: Context, d_bytes: torch.Tensor, key_desc: torch.Tensor,
               val_desc: Optional[torch.Tensor], idx: torch.Tensor, nout: int,
               key_bytes: int, val_bytes: int, stream=None,
               reuse: Optional[RecordBatch] = None, d_nout: Optional[torch.Tensor] = None) -> RecordBatch:
    """The selected pairs as a device CSR batch (lsm_build_sst's input);
    key_bytes / val_bytes bound the selected bytes.  koff_host / voff_host
    are left None (use sst_layout for the image sizes).  reuse: an earlier
    result whose buffers are large enough is written again (a compaction
    loop allocates once)."""
    dev = ctx.torch_device
    kb, vb = pad16(max(key_bytes, 1)), (pad16(max(val_bytes, 1)) if val_bytes is not None else None)
    wsb = int(ctx.lib.lsm_gather_kvs_workspace_bytes(nout))
    if (reuse is not None and reuse.koff.numel() >= nout + 1 and reuse.keys.numel() >= kb and
            (vb is None) == (reuse.vals is None) and (vb is None or reuse.vals.numel() >= vb) and
            getattr(reuse, "_ws", None) is not None and reuse._ws.numel() >= wsb):
        keys, vals, koff, voff, ws = reuse.keys, reuse.vals, reuse.koff, reuse.voff, reuse._ws
    else:
        keys = torch.empty(kb, dtype=torch.uint8, device=dev)
        vals = torch.empty(vb, dtype=torch.uint8, device=dev) if vb is not None else None
        koff = torch.empty(nout + 1, dtype=torch.int64, device=dev)  # vals None: keys only
        voff = torch.empty(nout + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    if d_nout is not None:  # lsm_gather_kvs_dev: the count on the device, nout its bound
        _lib.check(ctx.lib.lsm_gather_kvs_dev(
            ctx.handle, _ptr(d_bytes), _ptr(key_desc), _ptr(val_desc), _ptr(idx), _ptr(d_nout), nout,
            _ptr(keys), _ptr(koff), _ptr(vals), _ptr(voff), _ptr(ws), ws.numel(),
            _stream_handle(stream)), "lsm_gather_kvs_dev")
    else:
        _lib.check(ctx.lib.lsm_gather_kvs(
            ctx.handle, _ptr(d_bytes), _ptr(key_desc), _ptr(val_desc), _ptr(idx), nout, _ptr(keys),
            _ptr(koff), _ptr(vals), _ptr(voff), _ptr(ws), ws.numel(), _stream_handle(stream)),
            "lsm_gather_kvs")
    out = RecordBatch(keys=keys, koff=koff, vals=vals, voff=voff, n=nout, koff_host=None,
                      voff_host=None)
    out._ws = ws
    return out


def prepare_sst_device(ctx: Context, batch: RecordBatch, d_file_start: torch.Tensor, nfile: int,
                       max_recs: int, val_bytes: Optional[int] = None,
                       m: int = DEFAULT_BLOOM_M, k: int = DEFAULT_BLOOM_K,
                       align: int = 16, stream=None, reuse: Optional["SstBuild"] = None) -> "SstBuild":
    """prepare_sst for a device-resident batch (a merge's output): the layout
    by lsm_sst_layout on the device, nothing read back.  max_recs = the merge's
    most pairs per file (Merge.max_recs); the image buffer is sized from the
    header's bound (batch.keys bounds the key bytes, val_bytes -- or
    batch.vals -- the value bytes)."""
    dev = ctx.torch_device
    if val_bytes is None:
        if batch.vals is None:
            raise ValueError("prepare_sst_device: val_bytes is required for a keys-only batch")
        val_bytes = int(batch.vals.numel())
    fbytes = int(ctx.lib.lsm_filter_block_size(m))
    bound = (nfile * (fbytes + 40 + align - 1) + 16 * batch.n + 3 * int(batch.keys.numel()) +
             int(val_bytes))
    if reuse is not None and reuse.nfile == nfile:
        d_size, d_off = reuse.d_file_size, reuse.d_file_off
    else:
        d_size = torch.empty(max(nfile, 1), dtype=torch.int64, device=dev)
        d_off = torch.empty(nfile + 1, dtype=torch.int64, device=dev)
    _lib.check(ctx.lib.lsm_sst_layout(
        ctx.handle, _ptr(batch.koff), _ptr(batch.voff), _ptr(d_file_start), nfile, m, align,
        _ptr(d_size), _ptr(d_off), _stream_handle(stream)), "lsm_sst_layout")
    ws_bytes = int(ctx.lib.lsm_build_sst_workspace_bytes(nfile, max_recs, m, k))
    if (reuse is not None and reuse.out.numel() >= pad16(bound) and reuse.footer.numel() >= nfile * 4
            and reuse.workspace.numel() >= ws_bytes):  # reuse: an earlier build's buffers
        out, footer, workspace = reuse.out, reuse.footer, reuse.workspace
    else:  # every image byte and every footer word is written by the build: no fill
        out = torch.empty(pad16(bound), dtype=torch.uint8, device=dev)
        footer = torch.empty(max(nfile, 1) * 4, dtype=torch.int64, device=dev)
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    return SstBuild(
        out=out, footer=footer, workspace=workspace,
        d_file_start=d_file_start[:nfile + 1], d_file_off=d_off, d_file_size=d_size,
        max_recs=max_recs, m=m, k=k, nfile=nfile,
        stream=stream if stream is not None else torch.cuda.current_stream(dev))


def sst_pairs_into(ctx: Context, r: "SstDecode", key_out: torch.Tensor, val_out: torch.Tensor,
                   prefix: torch.Tensor, stream=None) -> None:
    """lsm_sst_pairs: the positional join of every decoded file, file after
    file (loadLevelData's allPairs), into dense descriptor arrays."""
    _lib.check(ctx.lib.lsm_sst_pairs(
        ctx.handle, _ptr(r.meta), _ptr(r.d_file_off), r.nfile, _ptr(r.idx_desc), _ptr(r.data_desc),
        _ptr(key_out), _ptr(val_out), _ptr(prefix), _stream_handle(stream)), "lsm_sst_pairs")


def sst_pairs(ctx: Context, r: "SstDecode", stream=None) -> tuple:
    """(key descriptors, value descriptors, prefix) of every file's pairs in
    file order; sized from the decoded metadata."""
    dev = r.idx_desc.device
    cap = int(r.idx_desc.shape[0])
    kd = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    vd = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    prefix = torch.zeros(r.nfile + 1, dtype=torch.int64, device=dev)
    sst_pairs_into(ctx, r, kd, vd, prefix, stream=stream)
    n = int(prefix[r.nfile].item())
    return kd[:n], vd[:n], prefix


def compact_merge_into(ctx: Context, d_img: torch.Tensor, r: "SstDecode", key_out: torch.Tensor,
                       val_out: torch.Tensor, prefix: torch.Tensor, mg: Merge, d_counts: torch.Tensor,
                       level: int = 1, threshold: int = MAX_SSTABLE_SIZE, tie: int = TIE_INPUT,
                       stream=None) -> Merge:
    """lsm_compact_merge_async: sst_pairs_into + merge_kvs_into(d_counts=...)
    in one call (the join, then CompactAndMergeKVs, on one stream).  mg.n
    must be the join's pair count; the counts stay on the device in
    d_counts (int64[3])."""
    _lib.check(ctx.lib.lsm_compact_merge_async(
        ctx.handle, _ptr(d_img), _ptr(r.meta), _ptr(r.d_file_off), r.nfile, _ptr(r.idx_desc),
        _ptr(r.data_desc), mg.n, _ptr(key_out), _ptr(val_out), _ptr(prefix), level, threshold, tie,
        _ptr(mg.out), _ptr(mg.file_start), _ptr(d_counts), _ptr(mg.workspace), mg.workspace.numel(),
        _stream_handle(stream)), "lsm_compact_merge_async")
    return mg


def build_sst_views_into(ctx: Context, batch: RecordBatch, sb: "SstBuild", d_bytes: torch.Tensor,
                         key_desc: torch.Tensor, val_desc: Optional[torch.Tensor],
                         idx: torch.Tensor, stream=None) -> None:
    """lsm_build_sst_views: the images of a keys-only gathered batch, values
    read in place from their views (value i = view of pair idx[i])."""
    nf = sb.nfile
    _lib.check(ctx.lib.lsm_build_sst_views(
        ctx.handle, _ptr(batch.keys), _ptr(batch.koff), _ptr(d_bytes), _ptr(key_desc),
        _ptr(val_desc), _ptr(idx), _ptr(batch.voff), _ptr(sb.d_file_start), nf, sb.max_recs, sb.m,
        sb.k, _ptr(sb.out), _ptr(sb.d_file_off), _ptr(sb.footer), _ptr(sb.workspace),
        sb.workspace.numel(), _stream_handle(stream)), "lsm_build_sst_views")


# ---- memtable flush (lsm_memtable_order) ---------------------------------------

MEMTABLE_ALL, MEMTABLE_RANGESCAN = 0, 1  # enum lsm_memtable_scan
MEMTABLE_TILE = 1024                     # LSM_MEMTABLE_TILE
MEMTABLE_OVERFLOW = 1 << 63              # LSM_MEMTABLE_OVERFLOW, in counts[2]


def memtable_order_workspace(ctx: Context, nlog: int, nslot: int, max_log_records: int) -> torch.Tensor:
    n = int(ctx.lib.lsm_memtable_order_workspace_bytes(nlog, nslot, max_log_records))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


class MemtableOrder:
    """lsm_memtable_order's buffers: idx[file_start[w]:file_start[w + 1]] = the
    slots of log w's memtable nodes in key order.  file_start (nlog + 1) and
    the three counts share one device tensor, so one copy reads both back."""

    def __init__(self, ctx: Context, nlog: int, nslot: int, max_log_records: int):
        dev = ctx.torch_device
        self.nlog, self.nslot, self.max_log_records = nlog, nslot, max_log_records
        self.idx = torch.empty(max(nslot, 1), dtype=torch.int32, device=dev)
        self.fsc = torch.zeros(nlog + 1 + 3, dtype=torch.int64, device=dev)
        self.file_start, self.counts = self.fsc[:nlog + 1], self.fsc[nlog + 1:]
        self.workspace = memtable_order_workspace(ctx, nlog, nslot, max_log_records)

    def result(self):
        """(per-log slot arrays, counts {pairs, non-empty logs, most pairs in a
        log}, overflow) on the host (reads back)."""
        h = self.fsc.cpu().numpy().view(np.uint64)
        fs, c = h[:self.nlog + 1].astype(np.int64), h[self.nlog + 1:]
        idx = self.idx[:int(c[0])].cpu().numpy().view(np.uint32)
        per_log = [idx[fs[w]:fs[w + 1]].copy() for w in range(self.nlog)]
        over = bool(int(c[2]) & MEMTABLE_OVERFLOW)
        return per_log, [int(c[0]), int(c[1]), int(c[2]) & (MEMTABLE_OVERFLOW - 1)], over


def memtable_order_into(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, wal_off: torch.Tensor,
                        scan: int, mo: MemtableOrder, stream=None) -> None:
    """lsm_memtable_order over a WAL replay's outputs r (either placement)."""
    _lib.check(ctx.lib.lsm_memtable_order(
        ctx.handle, _ptr(d_wal), _ptr(r.desc), _ptr(r.rec_base), _ptr(wal_off), _ptr(r.nrec),
        _ptr(r.status), mo.nlog, mo.nslot, mo.max_log_records, scan, _ptr(mo.idx),
        _ptr(mo.file_start), _ptr(mo.counts), _ptr(mo.workspace), mo.workspace.numel(),
        _stream_handle(stream)), "lsm_memtable_order")


def memtable_order(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, wal_off: torch.Tensor,
                   max_log_records: int, scan: int = MEMTABLE_ALL, stream=None) -> MemtableOrder:
    """The memtables of the replayed logs: each log's last record per key, in
    key order (MEMTABLE_ALL), or IMemTable.RangeScan's exact delivery
    (MEMTABLE_RANGESCAN).  max_log_records: lsm_max_records(KV, max_wal_len)."""
    mo = MemtableOrder(ctx, int(wal_off.numel()), int(r.desc.shape[0]), int(max_log_records))
    if mo.nlog:
        memtable_order_into(ctx, d_wal, r, wal_off, scan, mo, stream=stream)
    return mo


# ---- memtable search and database.Get (lsm_memtable_search, lsm_db_get) -----------

MEM_MISS, MEM_VALUE, MEM_DELETED = 0, 1, 2        # enum lsm_mem_result
DBGET_EXACT, DBGET_TOMBSTONE_HIDES = 0, 1         # enum lsm_db_get_mode
SRC_NONE, SRC_MEMTABLE, SRC_SSTABLE = -1, 0, 1    # enum lsm_get_source


def memtable_search_index(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, mo: MemtableOrder,
                          index: Optional[torch.Tensor] = None, stream=None) -> Optional[torch.Tensor]:
    """lsm_memtable_search_index_build over the MEMTABLE_ALL order mo of the
    replay r: each node's first 16 key bytes in mo.idx order.  Valid while
    mo.idx is; pass `index` to rebuild into the same buffer.  None when there
    is nothing to index (no logs or no slots): the search takes None."""
    if mo.nlog == 0 or mo.nslot == 0:
        return None
    if index is None:
        n = int(ctx.lib.lsm_memtable_search_index_bytes(mo.nslot))
        index = torch.empty(n, dtype=torch.uint8, device=ctx.torch_device)
    _lib.check(ctx.lib.lsm_memtable_search_index_build(
        ctx.handle, _ptr(d_wal), _ptr(r.desc), _ptr(mo.idx), _ptr(mo.file_start), mo.nlog, mo.nslot,
        _ptr(index), index.numel(), _stream_handle(stream)), "lsm_memtable_search_index_build")
    return index


def memtable_search_into(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, mo: MemtableOrder,
                         batch: "RecordBatch", mem_result: torch.Tensor, log: torch.Tensor,
                         slot: torch.Tensor, value: torch.Tensor, index: Optional[torch.Tensor] = None,
                         stream=None) -> None:
    """lsm_memtable_search: memtable.Manager.Search (memtable/manager.go:61-74)
    of every key of `batch` over the memtables of mo (logs oldest first, the
    newest searched first).  mem_result / log int32 and slot int32 (0xFFFFFFFF
    reads as -1) per key, value int32[nkeys, 4] (a view into d_wal)."""
    _lib.check(ctx.lib.lsm_memtable_search(
        ctx.handle, _ptr(d_wal), _ptr(r.desc), _ptr(mo.idx), _ptr(mo.file_start), mo.nlog,
        _ptr(index) if index is not None else None, index.numel() if index is not None else 0,
        _ptr(batch.keys), _ptr(batch.koff), batch.n, _ptr(mem_result), _ptr(log), _ptr(slot), _ptr(value),
        _stream_handle(stream)), "lsm_memtable_search")


def memtable_search(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, mo: MemtableOrder,
                    batch: "RecordBatch", index: Optional[torch.Tensor] = None, stream=None):
    """-> (mem_result int32[nkeys], log int32[nkeys], slot int32[nkeys],
    value int32[nkeys, 4]) on the device."""
    dev = ctx.torch_device
    n = max(batch.n, 1)
    mem_result = torch.empty(n, dtype=torch.int32, device=dev)
    log = torch.empty(n, dtype=torch.int32, device=dev)
    slot = torch.empty(n, dtype=torch.int32, device=dev)
    value = torch.empty((n, 4), dtype=torch.int32, device=dev)
    if batch.n:
        memtable_search_into(ctx, d_wal, r, mo, batch, mem_result, log, slot, value, index=index,
                             stream=stream)
    return mem_result[:batch.n], log[:batch.n], slot[:batch.n], value[:batch.n]


@dataclass
class DbGet:
    """lsm_db_get's per-key outputs on the device."""
    mem_result: torch.Tensor  # int32: MEM_*
    log: torch.Tensor         # int32
    slot: torch.Tensor        # int32 (0xFFFFFFFF reads as -1)
    level: torch.Tensor       # int32
    table: torch.Tensor       # int32
    result: torch.Tensor      # int32: GET_*
    value: torch.Tensor       # int32[nkeys, 4]: the returned value's view
    src: torch.Tensor         # int32: SRC_*


def alloc_db_get(ctx: Context, nkeys: int) -> DbGet:
    dev = ctx.torch_device
    n = max(nkeys, 1)
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    return DbGet(i32(), i32(), i32(), i32(), i32(), i32(),
                 torch.empty((n, 4), dtype=torch.int32, device=dev), i32())


def db_get_into(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, mo: MemtableOrder,
                d_img: torch.Tensor, sd: SstDecode, level_start, batch: "RecordBatch",
                index: torch.Tensor, out: DbGet, mode: int = DBGET_TOMBSTONE_HIDES,
                mem_index: Optional[torch.Tensor] = None, tree: Optional[SeekTree] = None,
                ws: Optional[torch.Tensor] = None, stream=None) -> None:
    """lsm_db_get: database.Get (database/database.go:24-40) of every key of
    `batch` -- the memtables of mo (memtable_search_into's arguments), then the
    tree decoded into sd (search_into's arguments) for the keys they did not
    answer.  index = level_index over sd; mem_index = memtable_search_index."""
    ls = _level_start(level_start)
    if int(ls[-1]) != sd.nfile:
        raise ValueError(f"level_start ends at {int(ls[-1])}, the tree holds {sd.nfile} tables")
    if ws is None:
        ws = search_workspace(ctx, ls, batch.n)
    nf = sd.nfile
    _lib.check(ctx.lib.lsm_db_get(
        ctx.handle, _ptr(d_wal), _ptr(r.desc), _ptr(mo.idx), _ptr(mo.file_start), mo.nlog,
        _ptr(mem_index) if mem_index is not None else None,
        mem_index.numel() if mem_index is not None else 0,
        _ptr(d_img) if nf else None, _ptr(index) if nf else None, ls.ctypes.data,
        _ptr(sd.d_file_off) if nf else None, _ptr(sd.d_file_len) if nf else None,
        _ptr(sd.meta) if nf else None, None, _ptr(sd.idx_desc) if nf else None,
        _ptr(sd.idx_value) if nf else None,
        _ptr(tree.data) if tree is not None else None, tree.max_nidx if tree is not None else 0,
        tree.data.numel() if tree is not None else 0,
        _ptr(batch.keys), _ptr(batch.koff), batch.n, mode,
        _ptr(out.mem_result), _ptr(out.log), _ptr(out.slot), _ptr(out.level), _ptr(out.table),
        _ptr(out.result), _ptr(out.value), _ptr(out.src), _ptr(ws), ws.numel(), _stream_handle(stream)),
        "lsm_db_get")


def db_get(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, mo: MemtableOrder, d_img: torch.Tensor,
           sd: SstDecode, level_start, batch: "RecordBatch", mode: int = DBGET_TOMBSTONE_HIDES,
           index: Optional[torch.Tensor] = None, mem_index: Optional[torch.Tensor] = None,
           tree: Optional[SeekTree] = None, stream=None) -> DbGet:
    """-> DbGet of device tensors, each cut to nkeys entries."""
    out = alloc_db_get(ctx, batch.n)
    if index is None and sd.nfile:
        index = level_index(ctx, d_img, sd, stream=stream)
    if batch.n:
        db_get_into(ctx, d_wal, r, mo, d_img, sd, level_start, batch, index, out, mode=mode,
                    mem_index=mem_index, tree=tree, stream=stream)
    n = batch.n
    return DbGet(out.mem_result[:n], out.log[:n], out.slot[:n], out.level[:n], out.table[:n],
                 out.result[:n], out.value[:n], out.src[:n])


# ---- the database scan (lsm_db_scan) ------------------------------------------

@dataclass
class DbScan:
    """lsm_db_scan's outputs on the device: range q's entries at
    [q * limit, q * limit + count[q])."""
    count: torch.Tensor   # int32[nq] (uint32 values)
    more: torch.Tensor    # uint8[nq]
    key: torch.Tensor     # int32[nq * limit, 4]: lsm_rec_desc into d_wal (memtable) or d_img (table)
    value: torch.Tensor   # int32[nq * limit, 4]: the value's view, in the same buffer
    src: torch.Tensor     # int32[nq * limit]: SRC_MEMTABLE or SRC_SSTABLE
    table: torch.Tensor   # int32[nq * limit]: the log, or the table's index in the tree
    result: torch.Tensor  # int32[nq * limit]: GET_*


def db_scan_workspace(ctx: Context, nlog: int, level_start, nq: int) -> torch.Tensor:
    ls = _level_start(level_start)
    n = int(ctx.lib.lsm_db_scan_workspace_bytes(nlog, ls.ctypes.data, nq))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def db_scan_into(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, mo: MemtableOrder,
                 d_img: torch.Tensor, sd: SstDecode, level_start, ranges: "RecordBatch",
                 flags: torch.Tensor, limit: int, mode: int, index: torch.Tensor, out: DbScan,
                 mem_index: Optional[torch.Tensor] = None, tree: Optional[SeekTree] = None,
                 ws: Optional[torch.Tensor] = None, stream=None) -> None:
    """lsm_db_scan: up to `limit` entries of every range over the memtables of
    mo (db_get_into's memtable arguments; the newest log answers first) and
    then the tree decoded into sd (tree_scan_into's tree arguments), in key
    order, each key once.  `ranges` / flags / limit / mode as tree_scan_into.
    index = level_index over sd; mem_index = memtable_search_index."""
    ls = _level_start(level_start)
    if int(ls[-1]) != sd.nfile:
        raise ValueError(f"level_start ends at {int(ls[-1])}, the tree holds {sd.nfile} tables")
    if ws is None:
        ws = db_scan_workspace(ctx, mo.nlog, ls, ranges.n)
    nf, nl = sd.nfile, mo.nlog
    _lib.check(ctx.lib.lsm_db_scan(
        ctx.handle, _ptr(d_wal) if nl else None, _ptr(r.desc) if nl else None, _ptr(mo.idx) if nl else None,
        _ptr(mo.file_start) if nl else None, nl,
        _ptr(mem_index) if mem_index is not None else None,
        mem_index.numel() if mem_index is not None else 0,
        _ptr(d_img) if nf else None, _ptr(index) if nf else None, ls.ctypes.data,
        _ptr(sd.d_file_off) if nf else None, _ptr(sd.d_file_len) if nf else None,
        _ptr(sd.meta) if nf else None, None, _ptr(sd.idx_desc) if nf else None,
        _ptr(sd.idx_value) if nf else None,
        _ptr(tree.data) if tree is not None else None, tree.max_nidx if tree is not None else 0,
        tree.data.numel() if tree is not None else 0,
        _ptr(ranges.keys), _ptr(ranges.koff), _ptr(ranges.vals), _ptr(ranges.voff), _ptr(flags), ranges.n,
        limit, mode, _ptr(out.count), _ptr(out.more), _ptr(out.key), _ptr(out.value), _ptr(out.src),
        _ptr(out.table), _ptr(out.result), _ptr(ws), ws.numel(), _stream_handle(stream)), "lsm_db_scan")


def db_scan(ctx: Context, d_wal: torch.Tensor, r: DecodeResult, mo: MemtableOrder, d_img: torch.Tensor,
            sd: SstDecode, level_start, ranges: "RecordBatch", flags, limit: int, mode: int = SCAN_LIVE,
            index: Optional[torch.Tensor] = None, mem_index: Optional[torch.Tensor] = None,
            tree: Optional[SeekTree] = None, stream=None) -> DbScan:
    """-> DbScan of device tensors, cut to nq ranges and nq * limit entries.
    flags: a uint8 device tensor, or host values to upload."""
    dev = ctx.torch_device
    nq = ranges.n
    count, more, key, value, table, result = _scan_outputs(dev, nq, limit)
    out = DbScan(count, more, key, value, torch.empty_like(table), table, result)
    flags = _scan_flags(dev, flags, nq)
    if index is None and sd.nfile:
        index = level_index(ctx, d_img, sd, stream=stream)
    if nq:
        db_scan_into(ctx, d_wal, r, mo, d_img, sd, level_start, ranges, flags, limit, mode, index, out,
                     mem_index=mem_index, tree=tree, stream=stream)
    e = nq * limit
    return DbScan(out.count[:nq], out.more[:nq], out.key[:e], out.value[:e], out.src[:e], out.table[:e],
                  out.result[:e])


# ---- the answered bytes as CSR arenas (lsm_pack_results) -----------------------

@dataclass
class Packed:
    """lsm_pack_results's outputs on the device: row q's entries are
    [row_start[q], row_start[q + 1]); key e is keys[koff[e] : koff[e + 1]],
    value e is vals[voff[e] : voff[e + 1]]."""
    row_start: torch.Tensor             # int64[nrow + 1]
    entry_slot: Optional[torch.Tensor]  # int32[nrow * limit] (uint32 values): entry e's slot
    koff: Optional[torch.Tensor]        # int64[nrow * limit + 1]; None when no keys are packed
    voff: torch.Tensor                  # int64[nrow * limit + 1]
    keys: Optional[torch.Tensor]        # uint8
    vals: Optional[torch.Tensor]        # uint8
    counts: torch.Tensor                # int64[4]: {E, K, V, overflow}


def pack_results_workspace(ctx: Context, nrow: int, limit: int) -> torch.Tensor:
    n = int(ctx.lib.lsm_pack_results_workspace_bytes(nrow, limit))
    return torch.empty(max(n, 16), dtype=torch.uint8, device=ctx.torch_device)


def alloc_packed(ctx: Context, nrow: int, limit: int, key_cap: Optional[int], val_cap: Optional[int],
                 with_keys: bool = True, entry_slot: bool = True) -> Packed:
    """Output tensors for pack_results_into.  key_cap / val_cap None: no arena
    (both None: the sizing call).  with_keys False: no koff either."""
    dev = ctx.torch_device
    n = max(nrow * limit, 1)
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda k: torch.empty(max(k, 1), dtype=torch.uint8, device=dev)  # noqa: E731
    return Packed(row_start=i64(max(nrow, 0) + 1),
                  entry_slot=torch.empty(n, dtype=torch.int32, device=dev) if entry_slot else None,
                  koff=i64(n + 1) if with_keys else None, voff=i64(n + 1),
                  keys=u8(key_cap) if (with_keys and key_cap is not None) else None,
                  vals=u8(val_cap) if val_cap is not None else None, counts=i64(4))


def pack_results_into(ctx: Context, d_wal: Optional[torch.Tensor], d_img: Optional[torch.Tensor],
                      value: torch.Tensor, out: Packed, key: Optional[torch.Tensor] = None,
                      src: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None, *,
                      nrow: int, limit: int, key_cap: int = 0, val_cap: int = 0,
                      ws: Optional[torch.Tensor] = None, stream=None) -> None:
    """lsm_pack_results: the live slots of nrow rows of `limit` slots (slot q *
    limit + j is live when j < count[q]; count None: all) as dense entries, and
    their keys (key None: not packed) and values packed into out.keys /
    out.vals, at most key_cap / val_cap bytes (out.counts[3] = 1 and no byte
    written when they do not fit).  src int32 per slot picks d_wal
    (SRC_MEMTABLE) or d_img (SRC_SSTABLE; src None: every slot).  Never
    synchronises: the counts stay on the device."""
    if ws is None:
        ws = pack_results_workspace(ctx, nrow, limit)
    _lib.check(ctx.lib.lsm_pack_results(
        ctx.handle, _ptr(d_wal), _ptr(d_img), _ptr(src), _ptr(key), _ptr(value), _ptr(count), nrow, limit,
        _ptr(out.keys), key_cap, _ptr(out.vals), val_cap, _ptr(out.row_start), _ptr(out.entry_slot),
        _ptr(out.koff), _ptr(out.voff), _ptr(out.counts), _ptr(ws), ws.numel(), _stream_handle(stream)),
        "lsm_pack_results")


def pack_results(ctx: Context, d_wal: Optional[torch.Tensor], d_img: Optional[torch.Tensor],
                 value: torch.Tensor, key: Optional[torch.Tensor] = None,
                 src: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None, *,
                 nrow: int, limit: int, stream=None) -> Packed:
    """-> Packed with arenas of exactly K and V bytes.  Two calls: the sizing
    call, a read-back of its counts, then the packing call.  SYNCHRONISES the
    stream for that read-back (pack_results_into with caps of the caller's
    does not).  The offset arrays are cut to E + 1 entries."""
    dev = ctx.torch_device
    with_keys = key is not None
    out = alloc_packed(ctx, nrow, limit, None, None, with_keys=with_keys)
    if nrow == 0:
        out.row_start.zero_()
        out.voff.zero_()
        out.counts.zero_()
        if out.koff is not None:
            out.koff.zero_()
        E = K = V = 0
    else:
        ws = pack_results_workspace(ctx, nrow, limit)
        pack_results_into(ctx, d_wal, d_img, value, out, key=key, src=src, count=count, nrow=nrow,
                          limit=limit, ws=ws, stream=stream)
        if stream is not None:
            stream.synchronize()
        E, K, V, _ = (int(x) for x in out.counts.cpu().numpy())  # the read-back (synchronises)
        out.keys = torch.empty(max(K, 1), dtype=torch.uint8, device=dev) if with_keys else None
        out.vals = torch.empty(max(V, 1), dtype=torch.uint8, device=dev)
        pack_results_into(ctx, d_wal, d_img, value, out, key=key, src=src, count=count, nrow=nrow,
                          limit=limit, key_cap=K, val_cap=V, ws=ws, stream=stream)
    return Packed(row_start=out.row_start[:nrow + 1], entry_slot=out.entry_slot[:E],
                  koff=out.koff[:E + 1] if with_keys else None, voff=out.voff[:E + 1],
                  keys=out.keys[:K] if with_keys and out.keys is not None else None,
                  vals=out.vals[:V] if out.vals is not None else None, counts=out.counts)


def pack_db_scan(ctx: Context, d_wal: Optional[torch.Tensor], d_img: Optional[torch.Tensor], scan: DbScan,
                 limit: int, stream=None) -> Packed:
    """pack_results over what db_scan returned (synchronises)."""
    return pack_results(ctx, d_wal, d_img, scan.value, key=scan.key, src=scan.src, count=scan.count,
                        nrow=int(scan.count.numel()), limit=limit, stream=stream)


def pack_db_get(ctx: Context, d_wal: Optional[torch.Tensor], d_img: Optional[torch.Tensor], get: DbGet,
                stream=None) -> Packed:
    """pack_results over what db_get returned: entry e is key e, values only
    (synchronises)."""
    return pack_results(ctx, d_wal, d_img, get.value, src=get.src, nrow=int(get.src.numel()), limit=1,
                        stream=stream)


def pack_tree_scan(ctx: Context, d_img: torch.Tensor, scan, limit: int, stream=None) -> Packed:
    """pack_results over the tuple tree_scan returned (synchronises)."""
    count, _more, key, value = scan[:4]
    return pack_results(ctx, None, d_img, value, key=key, count=count, nrow=int(count.numel()), limit=limit,
                        stream=stream)


def pack_search(ctx: Context, d_img: torch.Tensor, found, stream=None) -> Packed:
    """pack_results over the tuple search returned: entry e is key e, values
    only (synchronises)."""
    value = found[3]
    return pack_results(ctx, None, d_img, value, nrow=int(value.shape[0]), limit=1, stream=stream)


@dataclass
class MemtableFlush:
    """memtable_flush's result: image f is out[file_off[f]:file_off[f] +
    file_len[f]] and holds the memtable of log `log[f]`; status[w] is log w's
    replay status (a failed log has no image)."""
    out: torch.Tensor
    file_off: np.ndarray
    file_len: np.ndarray
    log: np.ndarray
    status: np.ndarray
    overflow: bool
    order: MemtableOrder
    replay: DecodeResult


def memtable_flush(ctx: Context, d_wal: torch.Tensor, wal_off: torch.Tensor, wal_len: torch.Tensor,
                   scan: int, m: int = DEFAULT_BLOOM_M, k: int = DEFAULT_BLOOM_K,
                   max_len: Optional[int] = None, stream=None) -> MemtableFlush:
    """CreateNewSSTable's image (sstable/manager.go:74-95) for every log at
    once: lsm_wal_replay -> lsm_memtable_order -> lsm_gather_kvs_dev (keys) ->
    lsm_sst_layout -> lsm_build_sst_views, the values read in place from the
    WAL bytes.  One level-0 image per non-empty memtable; one read-back (the
    order's file starts and counts) between the order and the build."""
    dev = ctx.torch_device
    nlog = int(wal_off.numel())
    if max_len is None:
        max_len = int(wal_len.max().item()) if nlog else 0
    r = wal_replay(ctx, d_wal, wal_off, wal_len, max_len=max_len, stream=stream)
    mo = memtable_order(ctx, d_wal, r, wal_off, int(ctx.lib.lsm_max_records(GRAMMAR_KV, max_len)),
                        scan, stream=stream)
    nbytes = int(d_wal.numel())
    empty = np.zeros(0, np.uint64)
    if nlog == 0:
        return MemtableFlush(torch.zeros(pad16(0), dtype=torch.uint8, device=dev), empty, empty,
                             np.zeros(0, np.int64), np.zeros(0, np.int32), False, mo, r)
    batch = gather_kvs(ctx, d_wal, r.desc, None, mo.idx, min(mo.nslot, nbytes // 8), nbytes, None,
                       stream=stream, d_nout=mo.counts[:1])
    if stream is not None:
        stream.synchronize()
    h = mo.fsc.cpu().numpy().view(np.uint64)  # the one read-back
    fs, c = h[:nlog + 1], h[nlog + 1:]
    status = r.status[:nlog].cpu().numpy().copy()
    logs = np.nonzero(np.diff(fs.astype(np.int64)) > 0)[0]
    nfile, total = len(logs), int(c[0])
    over = bool(int(c[2]) & MEMTABLE_OVERFLOW)
    if nfile == 0:  # an empty memtable has no image (Go would reach EncodeTo with a nil Header)
        return MemtableFlush(torch.zeros(pad16(0), dtype=torch.uint8, device=dev), empty, empty, logs,
                             status, over, mo, r)
    # the file list without the empty memtables: their starts repeat the next one's
    d_fs = _dev_i64(np.concatenate([fs[logs], [np.uint64(total)]]).astype(np.uint64), dev)
    batch.n = total
    sb = prepare_sst_device(ctx, batch, d_fs, nfile, int(c[2]) & (MEMTABLE_OVERFLOW - 1),
                            val_bytes=nbytes, m=m, k=k, stream=stream)
    build_sst_views_into(ctx, batch, sb, d_wal, r.desc, None, mo.idx, stream=stream)
    return MemtableFlush(sb.out, sb.file_off, sb.file_size, logs, status, over, mo, r)


# ---- database.Put / Delete (lsm_db_write) ----------------------------------------

OP_PUT, OP_DELETE = 0, 1        # enum lsm_write_op
MAX_MEMTABLE_SIZE = 2 << 20     # maxMemoryTableSize (memtable/memtable.go)


@dataclass
class DbWriteResult:
    """lsm_db_write's counts and per-log arrays on the host."""
    nlog: int
    nrec: int
    nbytes: int
    overflow: bool
    most_records: int
    mem_size: int           # sizeInBytes of the last log: the next call's mem_size0
    log_start: np.ndarray   # int64[nlog + 1], op index
    wal_off: np.ndarray     # int64[nlog + 1]
    wal_len: np.ndarray     # int64[nlog]
    rec_base: np.ndarray    # int64[nlog + 1]


class DbWrite:
    """lsm_db_write's device buffers: log s is wal[wal_off[s]:wal_off[s] +
    wal_len[s]].  log_start, wal_off, rec_base (nlog_max + 1 each) and the six
    counts share one device tensor, so one copy reads them back."""

    def __init__(self, ctx: Context, n: int, key_bytes: int, val_bytes: int, mem_size0: int, mem_max: int,
                 nlog_max: Optional[int] = None, align: int = 16, desc: bool = True, main_slot: bool = True,
                 fill: int = 0):
        dev = ctx.torch_device
        if nlog_max is None:
            nlog_max = int(ctx.lib.lsm_db_write_max_logs(n, key_bytes, val_bytes, mem_size0, mem_max))
        self.n, self.mem_size0, self.mem_max, self.nlog_max, self.align = n, mem_size0, mem_max, nlog_max, align
        self.out_bytes = int(ctx.lib.lsm_db_write_out_bytes(n, key_bytes, val_bytes, nlog_max, align))
        self.wal = torch.full((pad16(self.out_bytes),), fill, dtype=torch.uint8, device=dev)
        m = nlog_max + 1
        self.meta = torch.zeros(3 * m + 6, dtype=torch.int64, device=dev)
        self.log_start, self.wal_off, self.rec_base = self.meta[:m], self.meta[m:2 * m], self.meta[2 * m:3 * m]
        self.counts = self.meta[3 * m:]
        self.wal_len = torch.zeros(max(nlog_max, 1), dtype=torch.int32, device=dev)
        self.desc = torch.zeros((max(2 * n, 1), 4), dtype=torch.int32, device=dev) if desc else None
        self.main_slot = torch.zeros(max(n, 1), dtype=torch.int32, device=dev) if main_slot else None
        nws = int(ctx.lib.lsm_db_write_workspace_bytes(n, nlog_max, mem_max))
        self.workspace = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)

    def result(self) -> DbWriteResult:
        """Reads the counts and the per-log arrays back."""
        m = self.nlog_max + 1
        h = self.meta.cpu().numpy()
        c = h[3 * m:]
        nlog = int(c[0])
        return DbWriteResult(nlog, int(c[1]), int(c[2]), bool(c[3]), int(c[4]), int(c[5]),
                             h[:nlog + 1].copy(), h[m:m + nlog + 1].copy(),
                             self.wal_len[:nlog].cpu().numpy().view(np.uint32).astype(np.int64),
                             h[2 * m:2 * m + nlog + 1].copy())

    def replay(self, nlog: int):
        """(DecodeResult, wal_off) as lsm_wal_replay would leave them for the
        first nlog logs (rec_base placement, every status 0): what
        memtable_order, memtable_search and db_get take.  No read-back."""
        nrec = (self.rec_base[1:nlog + 1] - self.rec_base[:nlog]).to(torch.int32)
        status = torch.zeros(max(nlog, 1), dtype=torch.int32, device=self.wal.device)
        return DecodeResult(self.desc, nrec, status, self.rec_base[:nlog + 1]), self.wal_off[:nlog]


def db_write_into(ctx: Context, batch: "RecordBatch", ops: torch.Tensor, w: DbWrite, cur=None,
                  stream=None) -> None:
    """lsm_db_write into preallocated buffers.  cur = (d_bytes, d_desc, d_idx):
    the current memtable's nodes, d_idx being memtable_order(MEMTABLE_ALL)'s
    idx slice of that one log over d_bytes / d_desc; None = an empty skiplist."""
    cb, cd, ci = cur if cur is not None else (None, None, None)
    _lib.check(ctx.lib.lsm_db_write(
        ctx.handle, _ptr(batch.keys), _ptr(batch.koff), _ptr(batch.vals), _ptr(batch.voff), _ptr(ops),
        batch.n, w.mem_size0, w.mem_max, _ptr(cb), _ptr(cd), _ptr(ci), int(ci.numel()) if ci is not None else 0,
        w.nlog_max, w.align, _ptr(w.wal), _ptr(w.log_start), _ptr(w.wal_off), _ptr(w.wal_len), _ptr(w.desc),
        _ptr(w.rec_base), _ptr(w.main_slot), _ptr(w.counts), _ptr(w.workspace), w.workspace.numel(),
        _stream_handle(stream)), "lsm_db_write")


def db_write(ctx: Context, batch: "RecordBatch", ops, mem_size0: int = 0, mem_max: int = MAX_MEMTABLE_SIZE,
             cur=None, nlog_max: Optional[int] = None, align: int = 16, desc: bool = True,
             main_slot: bool = True, fill: int = 0, stream=None) -> DbWrite:
    """database.Put / database.Delete (database/database.go:42-59) of a batch:
    ops[i] = OP_PUT / OP_DELETE for record i of `batch` (a Delete's value is
    ignored).  Returns the device buffers; .result() reads the counts back,
    .replay(nlog) hands the logs to memtable_order / memtable_search / db_get
    without a replay."""
    if not isinstance(ops, torch.Tensor):
        ops = torch.from_numpy(_writable(np.asarray(ops, dtype=np.uint8))).to(ctx.torch_device)
    w = DbWrite(ctx, batch.n, int(batch.koff_host[-1]), int(batch.voff_host[-1]), mem_size0, mem_max,
                nlog_max=nlog_max, align=align, desc=desc, main_slot=main_slot, fill=fill)
    if batch.n:
        db_write_into(ctx, batch, ops, w, cur=cur, stream=stream)
    return w
