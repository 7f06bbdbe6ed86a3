"""GPU parity of lsm_pack_results against tests/pack_ref.py on hand-made
descriptors over two random buffers: bit-exact on row_start, entry_slot, koff,
voff, counts and both arenas.  The arenas are 64 bytes longer than needed and
pre-filled with a sentinel that must be intact past K and V (and everywhere on
overflow)."""
import numpy as np
import pytest
import torch

import lsmgpu
import pack_ref
from pack_ref import DESC, SRC_MEMTABLE, SRC_NONE, SRC_SSTABLE

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 64
LENGTHS = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 48, 100)
TILE = 512  # kScanTile: the slots of one scan workgroup


def buffers(seed, n=4096):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)


_dev = {}


def on_device(ctx, buf):
    """The device copy of a source buffer (padded to the input-slack contract), made once."""
    k = id(buf)
    if k not in _dev:
        _dev[k] = (buf, lsmgpu.to_device_bytes(buf, ctx.torch_device))
    return _dev[k][1]


def descs(rng, n, buf_len, lengths=LENGTHS):
    """n (key, value) descriptor pairs with lengths drawn from `lengths`, inside a buffer of buf_len."""
    key, value = np.zeros(n, DESC), np.zeros(n, DESC)
    key["key_len"] = rng.choice(lengths, n)
    key["val_len"] = 8
    value["val_len"] = rng.choice(lengths, n)
    key["rec_off"] = rng.integers(0, buf_len - 4 - max(lengths), n)
    value["rec_off"] = rng.integers(0, buf_len - 4 - max(lengths), n)
    return key, value


def run(ctx, wal, img, src, key, value, count, nrow, limit, key_cap="exact", val_cap="exact", entry_slot=True):
    """One lsm_pack_results call checked against pack_ref.  wal / img: host
    arrays or None (a NULL pointer).  key_cap / val_cap: "exact" (K / V), an
    int, or None (a NULL arena).  -> the reference."""
    dev = ctx.torch_device
    sizing = pack_ref.pack(wal, img, src, key, value, count, nrow, limit)
    E, K, V, _ = (int(x) for x in sizing.counts)
    kc = K if key_cap == "exact" else key_cap
    vc = V if val_cap == "exact" else val_cap
    if key is None:
        kc = None
    want = pack_ref.pack(wal, img, src, key, value, count, nrow, limit, key_cap=kc, val_cap=vc)
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    d_key = up(key, np.int32)
    d_value = up(value, np.int32)
    d_src, d_count = up(src, np.int32), up(count, np.int32)
    n = nrow * limit
    fill = lambda k, dt: torch.full((k,), -7, dtype=dt, device=dev)  # noqa: E731
    out = lsmgpu.Packed(
        row_start=fill(nrow + 1, torch.int64), entry_slot=fill(n, torch.int32) if entry_slot else None,
        koff=fill(n + 1, torch.int64) if key is not None else None, voff=fill(n + 1, torch.int64),
        keys=torch.full((K + PAD,), SENTINEL, dtype=torch.uint8, device=dev) if kc is not None else None,
        vals=torch.full((V + PAD,), SENTINEL, dtype=torch.uint8, device=dev) if vc is not None else None,
        counts=fill(4, torch.int64))
    lsmgpu.pack_results_into(
        ctx, on_device(ctx, wal) if wal is not None else None, on_device(ctx, img) if img is not None else None,
        d_value, out, key=d_key, src=d_src, count=d_count, nrow=nrow, limit=limit,
        key_cap=kc or 0, val_cap=vc or 0)
    torch.cuda.synchronize()
    assert out.counts.cpu().numpy().view(np.uint64).tolist() == want.counts.tolist()
    assert np.array_equal(out.row_start.cpu().numpy().view(np.uint64), want.row_start)
    if entry_slot:
        got = out.entry_slot.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:E], want.entry_slot)
        assert (out.entry_slot.cpu().numpy()[E:] == -7).all()
    assert np.array_equal(out.voff.cpu().numpy().view(np.uint64)[:E + 1], want.voff)
    assert (out.voff.cpu().numpy()[E + 1:] == -7).all()
    if key is not None:
        assert np.array_equal(out.koff.cpu().numpy().view(np.uint64)[:E + 1], want.koff)
    for arena, ref, total in ((out.keys, want.keys, K), (out.vals, want.vals, V)):
        if arena is None:
            continue
        got = arena.cpu().numpy()
        if ref is None:   # overflow: no byte of either arena
            assert (got == SENTINEL).all()
        else:
            assert len(ref) == total
            bad = np.flatnonzero(got[:total] != np.frombuffer(ref, np.uint8))
            assert bad.size == 0, (bad[:8], total)
            assert (got[total:] == SENTINEL).all()
    return want


def test_alignment(ctx):
    """One row of 64 slots: every length of LENGTHS for keys and values, source
    offsets over every residue mod 16 (the funnel shift's every case)."""
    wal, img = buffers(1)
    rng = np.random.default_rng(11)
    for rep in range(4):
        key, value = descs(rng, 64, img.size)
        key["rec_off"] = key["rec_off"].astype(np.int64) // 16 * 16 + (np.arange(64) + rep) % 16
        value["rec_off"] = value["rec_off"].astype(np.int64) // 16 * 16 + (np.arange(64) * 5 + rep) % 16
        key["key_len"][:12] = LENGTHS
        value["val_len"][:12] = LENGTHS[::-1]
        residues = lambda d: set(((d["rec_off"].astype(np.int64) + 4) % 16).tolist())  # noqa: E731
        assert residues(key) == set(range(16)) == residues(value)
        want = run(ctx, None, img, None, key, value, np.array([64], np.uint32), 1, 64)
        assert int(want.counts[0]) == 64
    # every length at every source residue and every destination residue: values of one length, keys of 1
    # byte shift the destination
    for n in LENGTHS:
        key, value = descs(rng, 64, img.size, lengths=(1,))
        value["val_len"] = n
        value["rec_off"] = 100 + 37 * np.arange(64)
        run(ctx, None, img, None, key, value, None, 1, 64)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 1025])
def test_wave_and_tile_edges(ctx, E):
    """The Get shape (limit 1, d_count NULL) around a wave's 64 entries, a copy
    workgroup's 256 and a scan tile's 512."""
    wal, img = buffers(2)
    rng = np.random.default_rng(E)
    key, value = descs(rng, E, img.size, lengths=(0, 5, 16, 24))
    want = run(ctx, None, img, None, key, value, None, E, 1)
    assert want.row_start.tolist() == list(range(E + 1))
    src = rng.choice([SRC_MEMTABLE, SRC_SSTABLE], E).astype(np.int32)
    run(ctx, wal, img, src, None, value, None, E, 1, entry_slot=False)


def test_ragged_rows(ctx):
    """700 rows of 3 slots, counts 0..3, more than 600 consecutive empty rows
    (whole tiles with nothing live), one count of limit + 5 (clamped), decoys
    in every slot that is not live."""
    wal, img = buffers(3)
    rng = np.random.default_rng(33)
    nrow, limit = 700, 3
    count = rng.integers(0, 4, nrow).astype(np.uint32)
    count[40:650] = 0
    count[20] = limit + 5
    count[699] = 3
    key, value = descs(rng, nrow * limit, img.size, lengths=(7, 16, 24, 33))  # the decoys too: non-zero
    src = rng.choice([SRC_MEMTABLE, SRC_SSTABLE], nrow * limit).astype(np.int32)
    want = run(ctx, wal, img, src, key, value, count, nrow, limit)
    assert int(want.counts[0]) == int(np.minimum(count, limit).sum()) and 0 < int(want.counts[0]) < 200
    assert want.row_start[21] - want.row_start[20] == 3
    assert (want.row_start[41:651] == want.row_start[40]).all()


def test_long_strings(ctx):
    """A 40,000-byte value and a 5,000-byte key between short entries: longer
    than a wave's chunk window (1,024 chunks of 16 bytes)."""
    wal, img = buffers(4, n=48 * 1024)
    rng = np.random.default_rng(44)
    n = 70
    key, value = descs(rng, n, img.size, lengths=(1, 16, 24))
    value[9] = (1003, 0, 40000)
    key[9] = (3, 16, 8)
    key[37] = (2001, 5000, 8)
    value[66] = (12345, 0, 17000)
    want = run(ctx, None, img, None, key, value, None, n, 1)
    assert int(want.counts[2]) > 57000 and int(want.counts[1]) > 5000


def test_two_sources(ctx):
    """Neighbouring entries of one wave alternate between the two buffers at
    the same offsets (the wrong base gives wrong bytes); LSM_SRC_NONE entries
    in between are entries of no bytes; so is a memtable entry when d_bytes is
    NULL."""
    wal, img = buffers(5)
    assert not np.array_equal(wal, img)
    rng = np.random.default_rng(55)
    n = 200
    key, value = descs(rng, n, img.size, lengths=(3, 16, 24, 40))
    src = np.where(np.arange(n) % 2 == 0, SRC_MEMTABLE, SRC_SSTABLE).astype(np.int32)
    src[5::7] = SRC_NONE
    src[10] = 7   # any other value reads as LSM_SRC_NONE
    want = run(ctx, wal, img, src, key, value, None, 4, 50)
    sizes = np.diff(want.voff.astype(np.int64))
    assert int(want.counts[0]) == n and (sizes[src == SRC_NONE] == 0).all() and sizes[10] == 0
    assert (sizes[(src == SRC_MEMTABLE) | (src == SRC_SSTABLE)] > 0).all()
    none = run(ctx, None, img, src, key, value, None, 4, 50)
    sizes = np.diff(none.voff.astype(np.int64))
    assert (sizes[src == SRC_MEMTABLE] == 0).all() and (sizes[src == SRC_SSTABLE] > 0).all()
    assert (np.diff(none.koff.astype(np.int64))[src == SRC_MEMTABLE] == 0).all()


def test_keys_omitted(ctx):
    """d_key, d_keys and d_koff NULL: values only."""
    wal, img = buffers(6)
    rng = np.random.default_rng(66)
    _, value = descs(rng, 300, img.size)
    count = rng.integers(0, 4, 100).astype(np.uint32)
    want = run(ctx, None, img, None, None, value, count, 100, 3)
    assert want.koff is None and int(want.counts[1]) == 0 and int(want.counts[2]) > 0


def test_nothing_live(ctx):
    wal, img = buffers(7)
    rng = np.random.default_rng(77)
    key, value = descs(rng, 600 * 2, img.size, lengths=(16, 24))
    want = run(ctx, None, img, None, key, value, np.zeros(600, np.uint32), 600, 2)
    assert want.counts.tolist() == [0, 0, 0, 0] and not want.row_start.any()
    assert want.koff.tolist() == [0] and want.voff.tolist() == [0]


def test_capacity(ctx):
    """One byte short in either arena: the flag, both arenas untouched, the
    offsets and counts in full; exact caps pack; the sizing call returns the
    same offsets and counts."""
    wal, img = buffers(8)
    rng = np.random.default_rng(88)
    key, value = descs(rng, 150, img.size, lengths=(16, 24, 5))
    count = rng.integers(1, 4, 50).astype(np.uint32)
    src = rng.choice([SRC_MEMTABLE, SRC_SSTABLE], 150).astype(np.int32)
    exact = run(ctx, wal, img, src, key, value, count, 50, 3)
    E, K, V, over = (int(x) for x in exact.counts)
    assert over == 0 and K > 0 and V > 0
    for kc, vc in ((K - 1, V), (K, V - 1), (0, 0)):
        short = run(ctx, wal, img, src, key, value, count, 50, 3, key_cap=kc, val_cap=vc)
        assert short.counts.tolist() == [E, K, V, 1] and short.keys is None and short.vals is None
    sizing = run(ctx, wal, img, src, key, value, count, 50, 3, key_cap=None, val_cap=None)
    assert sizing.counts.tolist() == [E, K, V, 0]
    assert np.array_equal(sizing.koff, exact.koff) and np.array_equal(sizing.voff, exact.voff)
    # one arena NULL: it is skipped and its cap ignored
    only_vals = run(ctx, wal, img, src, key, value, count, 50, 3, key_cap=None, val_cap=V)
    assert only_vals.counts.tolist() == [E, K, V, 0] and only_vals.vals == exact.vals


def test_wrapper_sizes_and_packs(ctx):
    """pack_results: the sizing call, exact arenas, the offsets cut to E + 1."""
    wal, img = buffers(9)
    rng = np.random.default_rng(99)
    key, value = descs(rng, 90, img.size, lengths=(16, 24, 0))
    count = rng.integers(0, 4, 30).astype(np.uint32)
    src = rng.choice([SRC_MEMTABLE, SRC_SSTABLE, SRC_NONE], 90).astype(np.int32)
    want = pack_ref.pack(wal, img, src, key, value, count, 30, 3, key_cap=1 << 30, val_cap=1 << 30)
    dev = ctx.torch_device
    up = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)  # noqa: E731
    p = lsmgpu.pack_results(ctx, on_device(ctx, wal), on_device(ctx, img), up(value), key=up(key), src=up(src),
                            count=up(count), nrow=30, limit=3)
    torch.cuda.synchronize()
    assert p.counts.cpu().numpy().view(np.uint64).tolist() == want.counts.tolist()
    assert p.keys.cpu().numpy().tobytes() == want.keys and p.vals.cpu().numpy().tobytes() == want.vals
    assert np.array_equal(p.koff.cpu().numpy().view(np.uint64), want.koff)
    assert np.array_equal(p.voff.cpu().numpy().view(np.uint64), want.voff)
    assert np.array_equal(p.row_start.cpu().numpy().view(np.uint64), want.row_start)
    assert np.array_equal(p.entry_slot.cpu().numpy().view(np.uint32), want.entry_slot)
