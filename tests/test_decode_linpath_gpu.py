"""GPU parity of the straight-line DESC path for blocks that fit the LDS ring
(decode_block_lin in go-lsm_amd/csrc/decode_core.h) and of its hand-over to the
general chase: every case against pyoracle.decode_block (descriptors, nrec,
status, idx_value), with the descriptor buffers pre-filled with a sentinel so
that a store past a block's verified records shows.
"""
import struct

import numpy as np
import pytest
import torch

import lsmgpu
import pyoracle as ora
from lsmgpu import synth
from test_decode_gpu import check_against_oracle, rand_records

pytestmark = pytest.mark.gpu

V, KV, IDX = lsmgpu.GRAMMAR_V, lsmgpu.GRAMMAR_KV, lsmgpu.GRAMMAR_IDX
GRAMMARS = [V, KV, IDX]
PLACEMENTS = ["offset", "plan"]
MIN_REC = {V: 4, KV: 8, IDX: 12}
ST_CAPACITY = 8


def rec(grammar, k, v, tag=0):
    """One record with a key of k bytes and a value of v bytes (V: no key;
    IDX: the value is the i64 offset)."""
    kb = bytes((tag + 7 + i) & 255 for i in range(k))
    vb = bytes((tag * 3 + i * 37) & 255 for i in range(v))
    if grammar == V:
        return struct.pack("<I", v) + vb
    if grammar == KV:
        return struct.pack("<I", k) + kb + struct.pack("<I", v) + vb
    return struct.pack("<I", k) + kb + struct.pack("<q", 1000 * tag - 7)


def exact_len_block(grammar, length, k=16, v=100):
    """A valid block of exactly `length` bytes: equal records, the last one
    stretched (or one short record added) to end at `length`."""
    size = len(rec(grammar, k, v))
    n = length // size
    out = [rec(grammar, k, v, i) for i in range(n)]
    left = length - n * size
    if left:
        if left < MIN_REC[grammar]:  # take the room from the last full record
            out.pop()
            left += size
        if grammar == IDX:
            out.append(rec(grammar, left - 12, 8, 99))
        else:
            out.append(rec(grammar, 0, left - MIN_REC[grammar], 99))
    b = b"".join(out)
    assert len(b) == length
    return b


def pack(blocks, starts=None, seed=0):
    """The blocks in one buffer; block i starts at an offset with
    (off & 15) == starts[i] (random when not given).  The gaps hold non-zero
    bytes: a block's first and last LDS lines carry its neighbours' bytes."""
    rng = np.random.default_rng(seed)
    parts, offs, lens, pos = [], [], [], 0
    for i, b in enumerate(blocks):
        b = np.frombuffer(bytes(b), np.uint8)
        res = starts[i] if starts is not None else int(rng.integers(0, 16))
        gap = (res - pos) % 16
        parts.append(np.full(gap, 0xA5, np.uint8))
        pos += gap
        offs.append(pos)
        lens.append(b.size)
        parts.append(b)
        pos += b.size
    return np.concatenate(parts), np.array(offs, np.uint64), np.array(lens, np.uint32)


def decode(ctx, grammar, buf, offs, lens, placement, entry="plain", caps=None):
    dev = ctx.torch_device
    d_in = lsmgpu.to_device_bytes(buf, dev)
    d_off = torch.tensor(offs.view(np.int64), device=dev)
    d_len = torch.tensor(lens.view(np.int32), device=dev)
    nblk = offs.size
    if placement == "offset":
        r = lsmgpu.alloc_decode_offset(ctx, grammar, nblk, int(d_in.numel()))
    else:
        p = lsmgpu.plan(ctx, grammar, d_len)
        if caps is not None:
            rb = np.zeros(nblk + 1, np.int64)
            rb[1:] = np.cumsum(caps)
            p.rec_base.copy_(torch.tensor(rb, device=dev))
            p.total_records = int(rb[-1])
        r = lsmgpu.alloc_decode(ctx, grammar, nblk, p)
    r.desc.fill_(-1)  # the sentinel
    if r.idx_value is not None:
        r.idx_value.fill_(-1)
    kw = {}
    if entry == "fit":         # a bound that fits the 8 KiB ring: its padded instantiation
        kw["max_blk_len"] = 8192 - 15
    elif entry == "fit4k":     # the same, the bound go-lsm's own block size
        kw["max_blk_len"] = 4096
    elif entry == "hinted8":   # a bound within 32 KiB that does not fit: the plain 8 KiB ring
        kw["max_blk_len"] = 8192
    elif entry == "hinted16":  # a large-block bound: the 16 KiB ring
        kw["max_blk_len"] = 40000
    elif entry == "sched":     # largest first, the 2 KiB ring
        kw["schedule"] = lsmgpu.schedule_workspace(ctx, nblk)
    lsmgpu.decode_into(ctx, grammar, d_in, d_off, d_len, r, **kw)
    torch.cuda.synchronize()
    return r


def check(grammar, buf, offs, lens, r, caps=None):
    """The comparison of tests/test_decode_gpu.py, then the whole descriptor
    (and idx_value) buffers: the oracle's records at each block's slots, the
    sentinel everywhere else."""
    if caps is None:
        check_against_oracle(grammar, buf, offs, lens, r)
    nblk = offs.size
    nrec = r.nrec.cpu().numpy()[:nblk]
    status = r.status.cpu().numpy()[:nblk]
    base = r.bases(offs).astype(np.int64)
    desc = r.desc_numpy()
    exp = np.frombuffer(np.full(desc.nbytes, 0xFF, np.uint8), lsmgpu.DESC_DTYPE).copy()
    iv = r.idx_value.cpu().numpy() if r.idx_value is not None else None
    eiv = np.full_like(iv, -1) if iv is not None else None
    for b in range(nblk):
        cap = None if caps is None else int(caps[b])
        st, d, oiv = ora.decode_block(grammar, buf, int(offs[b]), int(lens[b]), cap=cap)
        assert status[b] == st, (b, status[b], st)
        assert nrec[b] == len(d), (b, nrec[b], len(d))
        exp[base[b]:base[b] + len(d)] = d
        if eiv is not None:
            eiv[base[b]:base[b] + len(d)] = oiv
    bad = np.nonzero(desc != exp)[0]
    assert bad.size == 0, ("descriptor slots differ (a store past nrec, or a wrong record)", bad[:8])
    if iv is not None:
        bad = np.nonzero(iv != eiv)[0]
        assert bad.size == 0, ("idx_value slots differ", bad[:8])


def run(ctx, grammar, blocks, placement, entry="plain", starts=None, caps=None, seed=0):
    buf, offs, lens = pack(blocks, starts=starts, seed=seed)
    r = decode(ctx, grammar, buf, offs, lens, placement, entry=entry, caps=caps)
    check(grammar, buf, offs, lens, r, caps=caps)
    return r


# ---- uniform blocks -------------------------------------------------------------

@pytest.mark.parametrize("grammar", GRAMMARS)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("entry", ["plain", "hinted8", "fit"])
def test_uniform_blocks(ctx, grammar, placement, entry):
    """Equal records: 1, 2, 33, 64, 65 and 130 of them (one run, exactly one
    wave, one more, two waves plus two); 130 of the largest shape fit 8 KiB."""
    blocks = []
    for k, v in [(5, 20), (0, 0), (16, 30), (3, 1)]:
        for n in (1, 2, 33, 64, 65, 130):
            blocks.append(b"".join(rec(grammar, k, v, i) for i in range(n)))
    assert max(len(b) for b in blocks) + 15 <= 8192
    r = run(ctx, grammar, blocks, placement, entry=entry, seed=grammar)
    assert int((r.status[:len(blocks)] != 0).sum()) == 0
    assert r.nrec.cpu().tolist()[:6] == [1, 2, 33, 64, 65, 130]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("entry", ["plain", "fit4k"])
def test_config2_shape(ctx, placement, entry):
    """The default benchmark line's blocks: 33 x (16 B key, 100 B value),
    4,092 bytes in a 4,096-byte slot, 256 blocks; through the plain entry and
    with the benchmark's bound of 4,096."""
    buf, offs, lens = synth.uniform_kv_blocks(np.arange(256))
    assert int(lens[0]) == 4092 and int(offs[1]) == 4096
    r = decode(ctx, KV, buf, offs, lens, placement, entry=entry)
    check(KV, buf, offs, lens, r)
    assert bool((r.nrec[:256] == 33).all()) and int((r.status[:256] != 0).sum()) == 0


# ---- the hand-over to the general chase -------------------------------------------

@pytest.mark.parametrize("grammar", GRAMMARS)
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_run_broken_at_one_point(ctx, grammar, placement):
    """Equal records except one (another key length, another value length,
    both) at record 1, a middle record, the last record, and around the end of
    a 64-record run: the straight-line run stops there and the general chase
    goes on from that record."""
    k, v = 6, 22
    breaks = {V: [(0, 9)], KV: [(11, 22), (6, 9), (11, 9)], IDX: [(11, 8)]}[grammar]
    blocks = []
    for n, places in ((40, (1, 20, 39)), (100, (1, 63, 64, 65, 99))):
        for at in places:
            for bk, bv in breaks:
                recs = [rec(grammar, k, v, i) for i in range(n)]
                recs[at] = rec(grammar, bk, bv, at)
                blocks.append(b"".join(recs))
    r = run(ctx, grammar, blocks, placement, seed=3 + grammar)
    assert int((r.status[:len(blocks)] != 0).sum()) == 0


def failing_tails(grammar):
    """Byte strings that fail one check each when they stand where a record
    should start (the reference's order: kv.go:77-115, data.go:58-76,
    index.go:70-98)."""
    big_key, big_val = 2**20 + 1, 2**30 + 1
    if grammar == V:
        return [b"\x07", b"\x07\x00\x00",                     # length prefix cut
                struct.pack("<I", 50) + bytes(49),             # value truncated
                struct.pack("<I", 2**32 - 1) + bytes(20)]
    if grammar == KV:
        key = bytes(range(6))
        return [b"\x06", b"\x06\x00\x00",                      # length prefix cut
                struct.pack("<I", big_key) + bytes(40),        # key too long
                struct.pack("<I", 6) + key[:5],                # key truncated
                struct.pack("<I", 30) + bytes(12),
                struct.pack("<I", 6) + key,                    # value length cut: none left
                struct.pack("<I", 6) + key + b"\x16\x00\x00",  # ... three bytes of it
                struct.pack("<I", 6) + key + struct.pack("<I", big_val) + bytes(40),  # value too long
                struct.pack("<I", 6) + key + struct.pack("<I", 22) + bytes(21),       # value truncated
                struct.pack("<I", 6) + key + struct.pack("<I", 2**32 - 1) + bytes(8)]
    key = bytes(range(6))
    return [b"\x06", b"\x06\x00\x00",                          # overrun inside the key length
            struct.pack("<I", 6) + key[:3],                    # ... inside the key
            struct.pack("<I", 6) + key,                        # ... before the offset
            struct.pack("<I", 6) + key + bytes(7),             # ... inside the offset
            struct.pack("<I", 2**32 - 1) + bytes(30)]


@pytest.mark.parametrize("grammar", GRAMMARS)
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_record_failing_each_check(ctx, grammar, placement):
    """Record 0 failing each check in turn, and the same failures on the last
    record after a verified run of 10, 64 and 70 equal records."""
    tails = failing_tails(grammar)
    blocks = []
    for m in (0, 10, 64, 70):
        head = b"".join(rec(grammar, 6, 22, i) for i in range(m))
        blocks += [head + t for t in tails]
    r = run(ctx, grammar, blocks, placement, seed=11 + grammar)
    assert int((r.status[:len(blocks)] == 0).sum()) == 0  # each one fails
    assert sorted(set(r.nrec.cpu().tolist()[:len(blocks)])) == [0, 10, 64, 70]


@pytest.mark.parametrize("grammar", GRAMMARS)
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_block_start_and_empty_blocks(ctx, grammar, placement):
    """blk_off & 15 in {0, 1, 4, 8, 15} and blk_len = 0."""
    blocks, starts = [], []
    for s in (0, 1, 4, 8, 15):
        for n in (1, 33, 70):
            blocks.append(b"".join(rec(grammar, 16, 100, i) for i in range(n)))
            starts.append(s)
        blocks.append(b"")
        starts.append(s)
    r = run(ctx, grammar, blocks, placement, starts=starts)
    assert r.nrec.cpu().tolist()[:4] == [1, 33, 70, 0]
    assert int((r.status[:len(blocks)] != 0).sum()) == 0


# ---- the ring boundary ----------------------------------------------------------------

@pytest.mark.parametrize("grammar", GRAMMARS)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("entry,ring", [("plain", 8192), ("fit4k", 8192), ("hinted16", 16384),
                                        ("sched", 2048)])
def test_ring_boundary(ctx, grammar, placement, entry, ring):
    """Blocks whose (off & 15) + len rounded up to 16 equals the ring (the
    straight-line path) and blocks one 16-byte line longer (the streamed
    chase), at several block starts; valid blocks, and blocks with the last
    record cut.  `fit4k`: the padded instantiation, with blocks longer than
    the declared bound (the bound only picks the kernel)."""
    blocks, starts = [], []
    for h in (0, 1, 8, 15):
        for total in (ring - 16, ring, ring + 16):
            for length in (total - h, total - h - 15):  # both ends of the 16-byte line
                b = exact_len_block(grammar, length)
                blocks += [b, b[:-3]]
                starts += [h, h]
    r = run(ctx, grammar, blocks, placement, entry=entry, starts=starts)
    st = r.status.cpu().numpy()[:len(blocks)]
    assert (st[0::2] == 0).all() and (st[1::2] != 0).all()


# ---- capacity -----------------------------------------------------------------------------

@pytest.mark.parametrize("grammar", GRAMMARS)
def test_capacity(ctx, grammar):
    """rec_base leaving fewer slots than records: LSM_ST_CAPACITY at the
    oracle's record, nothing stored past the block's slots."""
    blocks, caps = [], []
    for n, cs in ((33, (0, 1, 10, 32, 33, 40)), (100, (63, 64, 65, 99, 100))):
        for c in cs:
            blocks.append(b"".join(rec(grammar, 6, 22, i) for i in range(n)))
            caps.append(c)
    # a failing record exactly at the capacity, and one past it
    blocks += [b"".join(rec(grammar, 6, 22, i) for i in range(10)) + b"\x06\x00"] * 2
    caps += [10, 9]
    r = run(ctx, grammar, blocks, "plan", caps=caps, seed=5)
    st = r.status.cpu().tolist()
    assert st[:6] == [ST_CAPACITY] * 4 + [0, 0]
    assert st[6:11] == [ST_CAPACITY] * 4 + [0]
    assert r.nrec.cpu().tolist()[:11] == [0, 1, 10, 32, 33, 33, 63, 64, 65, 99, 100]


# ---- scheduled against plain ------------------------------------------------------------

@pytest.mark.parametrize("grammar", GRAMMARS)
def test_scheduled_matches_plain(ctx, grammar):
    """The scheduled entry (launch order, 2 KiB ring) and the plain entry
    (8 KiB ring) give identical outputs on a small mixed batch."""
    rng = np.random.default_rng(60 + grammar)
    blocks = []
    for i in range(200):
        kind = i % 4
        if kind == 0:    # equal records, some blocks past either ring
            blocks.append(b"".join(rec(grammar, 16, 100, j) for j in range(int(rng.integers(0, 90)))))
        elif kind == 1:  # equal records, then a cut
            b = b"".join(rec(grammar, 4, 12, j) for j in range(int(rng.integers(1, 80))))
            blocks.append(b[:int(rng.integers(0, len(b)))])
        else:            # records of varying shape
            blocks.append(rand_records(rng, grammar, int(rng.integers(0, 50)), kmax=24, vmax=120))
    buf, offs, lens = pack(blocks, seed=grammar)
    a = decode(ctx, grammar, buf, offs, lens, "offset")
    b = decode(ctx, grammar, buf, offs, lens, "offset", entry="sched")
    assert torch.equal(a.status, b.status) and torch.equal(a.nrec, b.nrec)
    assert torch.equal(a.desc, b.desc)
    if grammar == IDX:
        assert torch.equal(a.idx_value, b.idx_value)
    check(grammar, buf, offs, lens, b)


# ---- the large-launch instantiation ---------------------------------------------------

@pytest.mark.parametrize("entry", ["plain", "fit4k"])
def test_large_launch_small_blocks(ctx, entry):
    """More than 400k blocks in one launch take the large-launch
    instantiation (the general chase on a linear ring), with or without a
    bound that fits the ring.  410k blocks of 3 equal records (and every 1,000th
    block with its last record cut) in 96-byte slots: counts and statuses in
    closed form, the descriptors of sampled blocks against the oracle."""
    nblk, slot = 410_000, 96
    body = np.frombuffer(b"".join(rec(KV, 4, 20, i) for i in range(3)), np.uint8)
    assert body.size == 96
    buf = np.tile(body, nblk)
    offs = np.arange(nblk, dtype=np.uint64) * np.uint64(slot)
    lens = np.full(nblk, slot, np.uint32)
    lens[::1000] = slot - 5
    r = decode(ctx, KV, buf, offs, lens, "offset", entry=entry)
    nrec = r.nrec.cpu().numpy()[:nblk]
    status = r.status.cpu().numpy()[:nblk]
    cut = np.zeros(nblk, bool)
    cut[::1000] = True
    assert (nrec[~cut] == 3).all() and (status[~cut] == 0).all()
    assert (nrec[cut] == 2).all() and (status[cut] != 0).all()
    desc = r.desc_numpy()
    base = r.bases(offs).astype(np.int64)
    for b in np.concatenate([[0, 1000, nblk - 1], np.random.default_rng(9).choice(nblk, 61)]):
        st, d, _ = ora.decode_block(KV, buf, int(offs[b]), int(lens[b]))
        assert status[b] == st and np.array_equal(desc[base[b]:base[b] + len(d)], d), b
        tail = desc[base[b] + len(d):base[b] + slot // 8]
        assert (tail["key_len"] == 0xFFFFFFFF).all(), b  # the sentinel past nrec
