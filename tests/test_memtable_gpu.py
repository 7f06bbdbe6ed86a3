"""GPU parity of lsm_memtable_order and the composed flush (memtable_flush):
a WAL's records -> its memtable's contents -> its level-0 SSTable image.

The order is checked against memtable_ref.order (pinned to the restated
skiplist in tests/test_memtable_ref.py) over the oracle's decode of each log;
the images against ora.build_sst of those pairs, byte for byte.  Every
comparison is exact.  T = lsmgpu.MEMTABLE_TILE, the records one workgroup
sorts in LDS: the record counts sit around its multiples, where the tile sort
hands over to the merge passes.
"""
import struct

import numpy as np
import pytest
import torch

import lsmgpu
import memtable_ref as ref
import pyoracle as ora

pytestmark = pytest.mark.gpu

T = lsmgpu.MEMTABLE_TILE
TOMB = ref.TOMBSTONE
SCANS = [lsmgpu.MEMTABLE_ALL, lsmgpu.MEMTABLE_RANGESCAN]


def pack(logs):
    """The logs in one buffer, each at a multiple of 16 -> (buf, offsets)."""
    offs, pos, parts = [], 0, []
    for lg in logs:
        offs.append(pos)
        pad = (16 - len(lg) % 16) % 16 + 16
        parts += [np.frombuffer(lg, np.uint8), np.zeros(pad, np.uint8)]
        pos += len(lg) + pad
    return np.concatenate(parts + [np.zeros(16, np.uint8)]), np.array(offs, np.uint64)


def records_of(buf, off, length):
    """The oracle's decode of one log -> (status, [(key, value)])."""
    st, desc, _ = ora.decode_block(ora.GRAMMAR_KV, buf, int(off), int(length))
    raw, recs = buf.tobytes(), []
    for o, kl, vl in zip(desc["rec_off"].tolist(), desc["key_len"].tolist(), desc["val_len"].tolist()):
        recs.append((raw[o + 4:o + 4 + kl], raw[o + 8 + kl:o + 8 + kl + vl]))
    return st, recs


class Case:
    """Logs on the device, replayed in one placement, with the oracle's records."""

    def __init__(self, ctx, logs, placement="offset"):
        self.ctx, self.logs = ctx, logs
        dev = ctx.torch_device
        self.buf, self.offs = pack(logs)
        self.lens = np.array([len(x) for x in logs], np.uint32)
        self.d = lsmgpu.to_device_bytes(self.buf, dev)
        self.off = torch.tensor(self.offs.view(np.int64), device=dev)
        self.len = torch.tensor(self.lens.view(np.int32), device=dev)
        self.max_len = int(self.lens.max()) if len(logs) else 0
        if placement == "offset":
            self.r = lsmgpu.wal_replay(ctx, self.d, self.off, self.len, max_len=self.max_len)
        else:
            p = lsmgpu.plan(ctx, lsmgpu.GRAMMAR_KV, self.len)
            self.r = lsmgpu.alloc_decode(ctx, lsmgpu.GRAMMAR_KV, len(logs), p)
            lsmgpu.wal_replay_into(ctx, self.d, self.off, self.len, self.max_len, self.r,
                                   lsmgpu.wal_workspace(ctx, len(logs), self.max_len))
        self.bases = self.r.bases(self.offs).astype(np.int64)
        self.decoded = [records_of(self.buf, o, n) for o, n in zip(self.offs, self.lens)]
        self.maxrec = int(ctx.lib.lsm_max_records(lsmgpu.GRAMMAR_KV, self.max_len))

    def want(self, scan, skip=()):
        out = []
        for w, (st, recs) in enumerate(self.decoded):
            pos = [] if st != 0 or w in skip else ref.order(recs, scan)
            out.append((self.bases[w] + np.array(pos, np.int64)).astype(np.uint32))
        return out

    def order(self, scan, maxrec=None):
        mo = lsmgpu.memtable_order(self.ctx, self.d, self.r, self.off,
                                   self.maxrec if maxrec is None else maxrec, scan)
        torch.cuda.synchronize()
        return mo.result()

    def check(self, scan, maxrec=None, skip=()):
        got, counts, over = self.order(scan, maxrec)
        want = self.want(scan, skip)
        for w, (g, x) in enumerate(zip(got, want)):
            assert np.array_equal(g, x), (w, scan, len(g), len(x), g[:8], x[:8])
        sizes = [len(x) for x in want]
        assert counts == [sum(sizes), sum(1 for s in sizes if s), max(sizes, default=0)]
        assert over == bool(skip)
        return want


def rec(k, v):
    return struct.pack("<I", len(k)) + k + struct.pack("<I", len(v)) + v


def random_log(rng, n, nkeys=None, p_tomb=0.1):
    """n records over a key pool small enough that about a third overwrite."""
    nkeys = nkeys or max(1, (2 * n) // 3)
    out = []
    for i in range(n):
        k = b"k_%d" % int(rng.integers(0, nkeys))
        v = TOMB if rng.random() < p_tomb else b"v%d" % i
        out.append(rec(k, v))
    return b"".join(out)


COUNTS = [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1, 4 * T + 1]  # the last needs three merge passes


@pytest.fixture(scope="module")
def count_logs():
    rng = np.random.default_rng(71)
    return [random_log(rng, n) for n in COUNTS]


@pytest.mark.parametrize("placement", ["offset", "plan"])
def test_record_counts_around_the_tile_both_scans_both_placements(ctx, count_logs, placement):
    c = Case(ctx, count_logs, placement)
    assert [len(r) for _, r in c.decoded] == COUNTS
    for scan in SCANS:
        want = c.check(scan)
    every = c.want(lsmgpu.MEMTABLE_ALL)
    assert any(len(a) > len(b) for a, b in zip(every, want))  # RangeScan really loses pairs


def test_mixed_logs_empty_failed_and_shared_keys(ctx):
    rng = np.random.default_rng(72)
    a = random_log(rng, 700, nkeys=300)
    b = random_log(rng, 2 * T + 7, nkeys=300)  # the same keys as a: both keep theirs
    cut = random_log(rng, 500)[:-3]            # a record cut short: wal.Recover fails
    c = Case(ctx, [a, b"", b, cut, rec(b"k_1", b"x")])
    assert [st for st, _ in c.decoded] == [0, 0, 0, 6, 0]  # 6 = LSM_ST_TRUNC_VAL
    for scan in SCANS:
        want = c.check(scan)
        assert len(want[1]) == 0 and len(want[3]) == 0
    keys = [set(c.decoded[w][1][s - c.bases[w]][0] for s in c.want(0)[w]) for w in (0, 2)]
    assert len(keys[0] & keys[1]) > 100


def comparator_keys():
    long4k = bytes(range(256)) * 16
    long64k = bytes(reversed(range(256))) * 256
    keys = [b"", b"\x00", b"\x00\x00",
            b"samefirst8-A", b"samefirst8-B", b"samefirst8", b"samefirs",
            b"sixteen-bytes-eq-then-X", b"sixteen-bytes-eq-then-Y", b"sixteen-bytes-eq-",
            b"prefix7", b"prefix78", b"prefix789", b"prefix7\x00", b"prefix78\x00", b"prefix789\x00",
            b"t", b"t\x00", b"t\x00\x00", b"tttttttt", b"tttttttt\x00", b"tttttttt\x00\x00",
            b"\x7f", b"\x80", b"\xff", b"\x7fzzzzzzz\x7f", b"\x7fzzzzzzz\x80", b"\x7fzzzzzzz\xff",
            b"\x80zzzzzzz\x7f", b"\xffzzzzzzz\x80",
            # around the 16 bytes the sort keeps per record
            b"0123456789abcde", b"0123456789abcdef", b"0123456789abcdefg", b"0123456789abcde\x00",
            b"0123456789abcdef\x00", b"0123456789abcdef\x00\x00", b"0123456789abcdef\x7f",
            b"0123456789abcdef\x80", b"0123456789abcdef\xff", b"0123456789abcdefgh-24-bytes-A",
            b"0123456789abcdefgh-24-bytes-B", b"0123456789abcdefgh-24-bytes-",
            long4k, long4k[:-1], long4k[:-1] + b"\xfe", long64k, long64k[:-1] + b"\x01"]
    assert len(set(keys)) == len(keys)
    return keys


def test_comparator_go_string_order_and_survivor(ctx):
    """Every key written twice (three times for a few), shuffled: the order is
    bytes order and the survivor the last write, whatever the key's length."""
    rng = np.random.default_rng(73)
    keys = comparator_keys()
    writes = [(k, b"first") for k in keys] + [(k, b"second") for k in keys] + [(k, b"3") for k in keys[::3]]
    order = rng.permutation(len(writes))
    log = b"".join(rec(*writes[i]) for i in order)
    c = Case(ctx, [log, rec(b"b", b"1") + rec(b"a", b"2")])
    for scan in SCANS:
        want = c.check(scan)
    recs = c.decoded[0][1]
    got_keys = [recs[s - c.bases[0]][0] for s in want[0]]
    assert got_keys == sorted(keys)


def test_last_writer_wins_across_tile_boundaries(ctx):
    rng = np.random.default_rng(74)
    hot = []  # one key written in every tile of a 3T-record log
    for i in range(3 * T):
        hot.append(rec(b"hot" if i % 97 == 5 else b"cold%05d" % int(rng.integers(0, 10 ** 5)), b"%d" % i))
    same = [rec(b"only", b"%d" % i) for i in range(2 * T + 5)]  # every record the same key
    edge = [rec(b"f%05d" % i, b"x") for i in range(T + 50)]
    edge[T - 1] = rec(b"edge", b"older")
    edge[T] = rec(b"edge", b"newer")
    c = Case(ctx, [b"".join(hot), b"".join(same), b"".join(edge)])
    want = c.check(lsmgpu.MEMTABLE_ALL)
    c.check(lsmgpu.MEMTABLE_RANGESCAN)
    assert want[1].tolist() == [c.bases[1] + 2 * T + 4]
    assert c.bases[2] + T in want[2] and c.bases[2] + T - 1 not in want[2]
    last_hot = max(i for i in range(3 * T) if i % 97 == 5)
    assert c.bases[0] + last_hot in want[0]


TOMBSTONE_LOGS = {
    "leading": [(b"a", TOMB), (b"b", TOMB), (b"c", b"1"), (b"d", b"2")],
    "middle": [(b"a", b"1"), (b"b", b"2"), (b"c", b"x"), (b"c", b""), (b"c", TOMB), (b"d", b"4"), (b"e", b"5")],
    "leading+middle": [(b"a", TOMB), (b"b", b"1"), (b"c", TOMB), (b"d", b"2")],
    "only": [(b"a", TOMB), (b"b", b""), (b"b", TOMB)],
    "overwritten": [(b"a", b"1"), (b"b", TOMB), (b"b", b"back"), (b"c", b"3")],
    "ordinary": [(b"a", b""), (b"b", TOMB + b"!"), (b"c", TOMB[:-1]), (b"d", b"x")],
}


def test_scan_modes_on_the_tombstone_cases(ctx):
    names = list(TOMBSTONE_LOGS)
    c = Case(ctx, [b"".join(rec(k, v) for k, v in TOMBSTONE_LOGS[n]) for n in names])
    every = dict(zip(names, c.check(lsmgpu.MEMTABLE_ALL)))
    scan = dict(zip(names, c.check(lsmgpu.MEMTABLE_RANGESCAN)))

    def keys(name, slots):
        w = names.index(name)
        return [c.decoded[w][1][s - c.bases[w]][0] for s in slots]
    assert keys("leading", scan["leading"]) == [b"c", b"d"]
    assert keys("middle", scan["middle"]) == [b"a", b"b"]            # d and e are lost
    assert keys("middle", every["middle"]) == [b"a", b"b", b"c", b"d", b"e"]
    assert keys("leading+middle", scan["leading+middle"]) == [b"b"]
    assert len(scan["only"]) == 0 and keys("only", every["only"]) == [b"a", b"b"]
    assert keys("overwritten", scan["overwritten"]) == [b"a", b"b", b"c"]
    assert keys("ordinary", scan["ordinary"]) == [b"a", b"b", b"c", b"d"]


def test_max_log_records_below_a_logs_count(ctx):
    """The documented overflow answer: the log gets no pairs, bit 63 of
    counts[2] is set, the other logs are unaffected."""
    rng = np.random.default_rng(75)
    c = Case(ctx, [random_log(rng, 300), random_log(rng, 1500), random_log(rng, 299)])
    for scan in SCANS:
        c.check(scan, maxrec=300, skip={1})
        c.check(scan, maxrec=1500)


def test_equals_merge_kvs_over_the_reversed_log(ctx):
    """The composition the library already had: per log, merge_kvs (level 0, one
    file, TIE_INPUT keeps the first of equal keys) over the descriptors in
    reversed order gives MEMTABLE_ALL's pairs."""
    rng = np.random.default_rng(76)
    c = Case(ctx, [random_log(rng, 2 * T + 100), random_log(rng, 900)])
    got, _, _ = c.order(lsmgpu.MEMTABLE_ALL)
    for w in range(2):
        n, base = len(c.decoded[w][1]), int(c.bases[w])
        rev = torch.flip(c.r.desc[base:base + n], dims=[0]).contiguous()
        mg = lsmgpu.merge_kvs(ctx, c.d, rev, None, level=0, threshold=1 << 40)
        torch.cuda.synchronize()
        idx = mg.out[:mg.nout].cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(base + n - 1 - idx, got[w].astype(np.int64))


def expected_images(c, scan, m, k, skip=()):
    """[(log, image)] of ora.build_sst over each non-empty memtable's pairs."""
    out = []
    for w, slots in enumerate(c.want(scan, skip)):
        if len(slots) == 0:
            continue
        recs = c.decoded[w][1]
        pairs = [recs[s - c.bases[w]] for s in slots]
        kb, ko = csr([p[0] for p in pairs])
        vb, vo = csr([p[1] for p in pairs])
        img, _ = ora.build_sst(kb, ko, vb, vo, 0, len(pairs), m=m, k=k)
        out.append((w, img, pairs))
    return out


def csr(items):
    data = b"".join(items)
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return (np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)), off


def flush_and_check(c, scan, m, k):
    fl = lsmgpu.memtable_flush(c.ctx, c.d, c.off, c.len, scan, m=m, k=k)
    torch.cuda.synchronize()
    want = expected_images(c, scan, m, k)
    assert fl.log.tolist() == [w for w, _, _ in want]
    assert fl.status.tolist() == [st for st, _ in c.decoded]
    out = fl.out.cpu().numpy()
    for f, (w, img, _) in enumerate(want):
        o, n = int(fl.file_off[f]), int(fl.file_len[f])
        assert n == img.size and out[o:o + n].tobytes() == img.tobytes(), (f, w)
    return fl, out, want


@pytest.mark.parametrize("m,k", [(lsmgpu.DEFAULT_BLOOM_M, lsmgpu.DEFAULT_BLOOM_K), (256, 3)])
def test_flush_images_byte_identical(ctx, m, k):
    rng = np.random.default_rng(77)
    cut = random_log(rng, 400)[:-1]
    c = Case(ctx, [random_log(rng, 1200), b"", random_log(rng, T + 3), cut, rec(b"z", TOMB),
                   random_log(rng, 5)])
    for scan in SCANS:
        fl, out, want = flush_and_check(c, scan, m, k)
        assert 3 not in fl.log and 1 not in fl.log  # no image for a failed or an empty log
        for f, (w, img, pairs) in enumerate(want):  # decode_sst gives back the pairs
            o, n = int(fl.file_off[f]), int(fl.file_len[f])
            rc, meta, idesc, _, ddesc = ora.sst_decode(out[o:o + n])
            assert rc == 0 and meta.nidx == meta.ndata == len(pairs)
            image = out[o:o + n]
            for (key, val), di, dd in zip(pairs, idesc, ddesc):
                assert image[int(di["rec_off"]) + 4:][:int(di["key_len"])].tobytes() == key
                assert image[int(dd["rec_off"]) + 4:][:int(dd["val_len"])].tobytes() == val


def test_flushed_tables_answer_every_key_with_its_last_value(ctx):
    """lsm_level0_get over the flushed tables, newest first: every key ever
    written is found with the value of its last write."""
    rng = np.random.default_rng(78)
    logs = [random_log(rng, 900, nkeys=500, p_tomb=0.05) for _ in range(4)]  # oldest first
    c = Case(ctx, logs)
    fl = lsmgpu.memtable_flush(ctx, c.d, c.off, c.len, lsmgpu.MEMTABLE_ALL, m=1 << 14, k=4)
    torch.cuda.synchronize()
    assert fl.log.tolist() == [0, 1, 2, 3]
    last = {}
    for _, recs in c.decoded:
        for key, val in recs:
            last[key] = val
    newest_first = np.arange(3, -1, -1)
    r = lsmgpu.decode_sst(ctx, fl.out, fl.file_off[newest_first], fl.file_len[newest_first])
    probes = sorted(last)
    kb, ko = csr(probes)
    batch = lsmgpu.batch_to_device(ctx, kb, ko, np.zeros(1, np.uint8), np.zeros(len(probes) + 1, np.uint64))
    table, res, val = lsmgpu.level0_get(ctx, fl.out, r, batch)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == lsmgpu.GET_FOUND).all()
    out = fl.out.cpu().numpy()
    v = val.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
    for i, key in enumerate(probes):
        o = int(v["rec_off"][i]) + 4
        assert out[o:o + int(v["val_len"][i])].tobytes() == last[key], key


def test_flush_skips_the_overflowing_log(ctx):
    """max_len below one log: its memtable is not indexed and gets no image."""
    rng = np.random.default_rng(79)
    small, big = random_log(rng, 40), rec(b"a", b"1") * 2000
    c = Case(ctx, [small, big, small])
    fl = lsmgpu.memtable_flush(ctx, c.d, c.off, c.len, lsmgpu.MEMTABLE_ALL, m=256, k=3, max_len=len(small))
    torch.cuda.synchronize()
    assert fl.overflow and fl.log.tolist() == [0, 2]
    want = expected_images(c, lsmgpu.MEMTABLE_ALL, 256, 3, skip={1})
    out = fl.out.cpu().numpy()
    for f, (w, img, _) in enumerate(want):
        o = int(fl.file_off[f])
        assert out[o:o + img.size].tobytes() == img.tobytes()


def test_full_size_recovery_eleven_memtables(ctx):
    """go-lsm's recovery maximum: 11 logs of 2 MiB with overwrites and deletes."""
    rng = np.random.default_rng(80)
    logs = []
    for w in range(11):
        n = 2 * 1024 * 1024 // 38
        ids = rng.integers(0, (2 * n) // 3, n)
        tomb = rng.random(n) < 0.02
        logs.append(b"".join(rec(b"k_%07d" % i, TOMB if t else b"value_%09d" % j)
                             for j, (i, t) in enumerate(zip(ids.tolist(), tomb.tolist()))))
    c = Case(ctx, logs)
    c.check(lsmgpu.MEMTABLE_RANGESCAN)
    c.check(lsmgpu.MEMTABLE_ALL)
    flush_and_check(c, lsmgpu.MEMTABLE_ALL, lsmgpu.DEFAULT_BLOOM_M, lsmgpu.DEFAULT_BLOOM_K)


def test_order_is_capturable_in_a_graph(ctx):
    """No host synchronisation, read-back or allocation inside the call: it is
    captured once and replayed over new logs written into the same buffers."""
    rng = np.random.default_rng(81)
    first = [random_log(rng, T + 200), random_log(rng, 300)]
    c = Case(ctx, first)
    mo = lsmgpu.MemtableOrder(ctx, 2, int(c.r.desc.shape[0]), c.maxrec)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up outside the capture
        lsmgpu.memtable_order_into(ctx, c.d, c.r, c.off, lsmgpu.MEMTABLE_ALL, mo)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lsmgpu.memtable_order_into(ctx, c.d, c.r, c.off, lsmgpu.MEMTABLE_ALL, mo)
    second = [random_log(rng, T // 2 + 7), random_log(rng, 120)]  # other counts, same buffers
    for logs in (first, second):
        assert all(len(a) <= len(b) for a, b in zip(logs, first))
        buf = c.buf.copy()
        lens = np.array([len(x) for x in logs], np.uint32)
        for o, lg in zip(c.offs, logs):
            buf[int(o):int(o) + len(lg)] = np.frombuffer(lg, np.uint8)
        c.d[:buf.size].copy_(torch.from_numpy(buf))
        c.len.copy_(torch.from_numpy(lens.view(np.int32)))
        lsmgpu.wal_replay_into(ctx, c.d, c.off, c.len, c.max_len, c.r,
                               lsmgpu.wal_workspace(ctx, 2, c.max_len))
        graph.replay()
        torch.cuda.synchronize()
        got, counts, over = mo.result()
        for w, (o, n) in enumerate(zip(c.offs, lens)):
            st, recs = records_of(buf, o, n)
            assert st == 0
            want = (c.bases[w] + np.array(ref.order(recs, ref.ALL), np.int64)).astype(np.uint32)
            assert np.array_equal(got[w], want), w
        assert not over and counts[0] == sum(len(g) for g in got)
