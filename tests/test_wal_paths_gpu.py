"""lsm_wal_replay on the GPU, case by case (tests/wal_cases.py): every stitch
path of wal.hip against the oracle's serial chase, in both placements and at
three start misalignments.

Every case is a small log built to reach one path (the census in wal_cases.py
and tests/test_wal_cases.py prove which).  It is replayed between two
neighbour logs in one call, so that a store into another log's slots shows.
The outputs are the caller's own, 64 slots longer than needed and filled with
a sentinel, nrec and status are prefilled, and the whole arrays are compared:
a log's slots hold exactly the oracle's descriptors, every other slot is
still the sentinel.  The bytes around each log are hostile (a continuation of
valid records, or 0xFF), the start is shifted by h in {0, 1, 15} bytes off a
16-byte boundary, and the workspace is full of 0xA5.  All comparisons are
exact.
"""
import functools

import numpy as np
import pytest
import torch

import lsmgpu
import pyoracle as ora
import wal_cases as wc

pytestmark = pytest.mark.gpu

SLACK = 64
SENTINEL = 0x5A5A5A5A            # desc, nrec: no record offset or count of these calls
STATUS_SENTINEL = -77
GAP = 96                         # hostile bytes in front of and after each log, at least
NAMES = [c.name for c in wc.CASES]
LEFT = b"".join(wc.rec(b"left%d" % i, b"neighbour") for i in range(3))
RIGHT = b"".join(wc.rec(b"r%d" % i, b"the log after" * i) for i in range(5))
FILLER = b"".join(wc.rec(b"beyond%d" % i, b"not this log's") for i in range(8))


def gap_bytes(n, hostile):
    """n bytes for a gap between logs.  "records": whole records that end
    where the next log starts, and whole records from where a log ends."""
    if hostile == "ff":
        return b"\xff" * n
    head = FILLER[:29 * min((n - 13) // 29, 2)]    # whole records right after the log before
    return head + wc.rec(b"front", b"." * (n - len(head) - 13))


def lay_out(logs, h, hostile):
    """-> (buffer, wal_off, wal_len): each log starts h bytes off a 16-byte
    boundary, hostile bytes between and around the logs."""
    parts, pos, offs = [], 0, []
    for lg in logs:
        off = (pos + GAP + 15) // 16 * 16 + h
        parts.append(gap_bytes(off - pos, hostile))
        parts.append(lg)
        offs.append(off)
        pos = off + len(lg)
    parts.append(gap_bytes(GAP + (-(pos + GAP)) % 16, hostile))
    buf = np.frombuffer(b"".join(parts), np.uint8)
    return buf, np.array(offs, np.uint64), np.array([len(x) for x in logs], np.uint32)


class Call:
    """One lsm_wal_replay over `logs` with sentinel-guarded outputs; caps[w]
    slots for log w under rec_base placement (None: its record count + 3)."""

    def __init__(self, ctx, logs, h, hostile, placement, max_len=None, caps=None, ws=None):
        dev = ctx.torch_device
        self.buf, self.off, self.len = lay_out(logs, h, hostile)
        n = len(logs)
        caps = caps or [None] * n
        if placement == "rec_base":
            full = [len(ora.decode_block(ora.GRAMMAR_KV, self.buf, int(o), int(l))[1])
                    for o, l in zip(self.off, self.len)]
            self.cap = [f + 3 if c is None else c for f, c in zip(full, caps)]
            self.base = np.concatenate([[0], np.cumsum(self.cap)]).astype(np.int64)
            nslot = int(self.base[-1]) + SLACK
            rec_base = torch.from_numpy(self.base.copy()).to(dev)
        else:
            self.base = (self.off // np.uint64(8)).astype(np.int64)
            self.cap = [int((o + l) // 8 - o // 8) for o, l in zip(self.off.astype(np.int64), self.len)]
            nslot = self.buf.size // 8 + 1 + SLACK
            rec_base = None
        self.r = lsmgpu.codec.DecodeResult(
            desc=torch.full((nslot, 4), SENTINEL, dtype=torch.int32, device=dev),
            nrec=torch.full((n + 2,), SENTINEL, dtype=torch.int32, device=dev),
            status=torch.full((n + 2,), STATUS_SENTINEL, dtype=torch.int32, device=dev),
            rec_base=rec_base)
        max_len = int(self.len.max()) if max_len is None else max_len
        if ws is None:
            ws = workspace(ctx, n, max_len)
        self.d_buf = lsmgpu.to_device_bytes(self.buf, dev)
        self.d_off = torch.from_numpy(self.off.view(np.int64).copy()).to(dev)
        self.d_len = torch.from_numpy(self.len.view(np.int32).copy()).to(dev)
        lsmgpu.wal_replay_into(ctx, self.d_buf, self.d_off, self.d_len, max_len, self.r, ws)

    def check(self):
        n = len(self.off)
        nrec = self.r.nrec.cpu().numpy()
        status = self.r.status.cpu().numpy()
        desc = self.r.desc_numpy()
        want = np.frombuffer(np.full(desc.size * 4, SENTINEL, np.uint32).tobytes(), ora.DESC_DTYPE).copy()
        for w in range(n):
            st, d, _ = ora.decode_block(ora.GRAMMAR_KV, self.buf, int(self.off[w]), int(self.len[w]),
                                        cap=self.cap[w])
            print("log", w, "status", status[w], st, "nrec", nrec[w], len(d), "cap", self.cap[w])
            assert (status[w], nrec[w]) == (st, len(d)), (w, status[w], st, nrec[w], len(d))
            want[self.base[w]:self.base[w] + len(d)] = d
        bad = np.flatnonzero(desc != want)
        assert bad.size == 0, (bad[:8], desc[bad[:8]], want[bad[:8]])
        assert np.all(nrec[n:] == SENTINEL) and np.all(status[n:] == STATUS_SENTINEL)
        return status, nrec


def workspace(ctx, nwal, max_len):
    """A workspace full of a fixed byte, so that a stale word read by mistake
    is the same word in every run."""
    n = int(ctx.lib.lsm_wal_replay_workspace_bytes(nwal, max_len))
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=ctx.torch_device)


def call_of(ctx, case, h, hostile, placement, last=False, ws=None):
    logs = [LEFT, RIGHT, case.log] if last else [LEFT, case.log, RIGHT]
    caps = None
    if placement == "rec_base" and case.cap is not None:
        caps = [None, None, case.cap] if last else [None, case.cap, None]
    max_len = max(len(LEFT), len(RIGHT), len(case.log)) if case.max_len is None else case.max_len
    return Call(ctx, logs, h, hostile, placement, max_len=max_len, caps=caps, ws=ws)


@pytest.mark.parametrize("hostile", ["records", "ff"])
@pytest.mark.parametrize("h", [0, 1, 15])
@pytest.mark.parametrize("placement", ["offset", "rec_base"])
@pytest.mark.parametrize("name", NAMES)
def test_case(ctx, name, placement, h, hostile):
    c = call_of(ctx, wc.BY_NAME[name], h, hostile, placement)
    torch.cuda.synchronize()
    c.check()


CAPACITY = [c.name for c in wc.CASES if c.cap is not None]


@functools.lru_cache(maxsize=None)
def records_of(name):
    return wc.expected(wc.BY_NAME[name])


@pytest.mark.parametrize("h", [0, 1, 15])
@pytest.mark.parametrize("name", CAPACITY)
def test_capacity(ctx, name, h):
    """A caller's rec_base with fewer slots than records: LSM_ST_CAPACITY,
    nrec = the slots, the first of them exact and the slot after them
    untouched (the log is the call's last, the slot is the sentinel's); with
    exactly enough slots, the log's own status.  A log with more records than
    slots that also ends in an error is LSM_ST_CAPACITY (include/lsm_gpu.h)."""
    case = wc.BY_NAME[name]
    full_st, full = records_of(name)
    c = call_of(ctx, case, h, "records", "rec_base", last=True)
    torch.cuda.synchronize()
    status, nrec = c.check()
    if len(full) > case.cap:
        assert (status[2], nrec[2]) == (wc.ST_CAPACITY, case.cap)
    else:
        assert (status[2], nrec[2]) == (full_st, len(full))
    past = c.r.desc_numpy()[c.base[2] + case.cap:c.base[2] + case.cap + 1]
    assert past.tobytes() == np.full(4, SENTINEL, np.uint32).tobytes()


def test_back_to_back_on_one_workspace(ctx):
    """Two cases, each twice, through one workspace with no synchronize of
    ours between the calls: nothing a call leaves in the workspace (packed
    entries, full descriptors, WalSeg and fin words) may reach the next
    call's output."""
    a, b = (wc.BY_NAME[x] for x in wc.BACK_TO_BACK)
    ws = workspace(ctx, 3, max(len(a.log), len(b.log)))
    calls = [call_of(ctx, case, h, "ff", "offset", ws=ws) for case, h in ((a, 0), (b, 15), (a, 1), (b, 0))]
    torch.cuda.synchronize()
    for c in calls:
        c.check()
