"""GPU parity of lsm_search: Manager.Search (sstable/manager.go:99-133) for a
batch of keys over a whole tree in one call, against the per-level
composition of the oracle (tests/search_ref.py, pinned against a restatement
of the Go text in tests/test_search_ref.py).  Bit-exact: the answering level
and table, the result code and the value view of every probe, with the Seek
tree and without it.
"""
import numpy as np
import pytest
import torch

import lsmgpu
import pyoracle as ora
import search_ref
from search_ref import csr

pytestmark = pytest.mark.gpu

LEVELS = search_ref.LEVELS
L0_CAP = 8          # the issue's wide level 0: one table more than this
MAX_TABLES = 2048   # tables the level search's LDS index holds (kLvMaxFiles)
MAX_GRID = 8192     # workgroups of one launch (kSrMaxGrid)


def build(keys, vals, m=4096, k=4):
    kb, ko = csr(keys)
    vb, vo = csr(vals)
    img, _ = ora.build_sst(kb if kb.size else np.zeros(1, np.uint8), ko,
                           vb if vb.size else np.zeros(1, np.uint8), vo, 0, len(keys), m=m, k=k)
    return img.copy()


def place(rng, images):
    offs, pos, parts = [], 0, []
    for im in images:
        gap = int(rng.integers(0, 23))
        parts += [np.zeros(gap, np.uint8), im]
        pos += gap
        offs.append(pos)
        pos += im.size
    buf = np.concatenate(parts + [np.zeros(16, np.uint8)])
    return buf, np.array(offs, np.uint64)


class Tree:
    """levels: LEVELS lists of images.  The device copy, its decode, index and
    Seek tree, and what the oracle needs."""

    def __init__(self, ctx, rng, levels):
        assert len(levels) == LEVELS
        self.images = [im for lv in levels for im in lv]
        self.level_start = search_ref.level_starts([len(lv) for lv in levels])
        self.buf, self.offs = place(rng, self.images)
        self.lens = np.array([im.size for im in self.images], np.uint64)
        self.dec = [ora.sst_decode(im) for im in self.images]
        self.d_img = lsmgpu.to_device_bytes(self.buf, ctx.torch_device)
        self.r = lsmgpu.decode_sst(ctx, self.d_img, self.offs, self.lens)
        self.index = lsmgpu.level_index(ctx, self.d_img, self.r)
        self.tree = lsmgpu.level_get_tree(ctx, self.d_img, self.r)

    def reference(self, probes):
        kb, ko = csr(probes)
        return search_ref.search(self.buf, self.offs, self.lens, self.dec, self.level_start, kb, ko,
                                 len(probes))


def to_batch(ctx, kb, ko):
    return lsmgpu.batch_to_device(ctx, kb if kb.size else np.zeros(1, np.uint8), ko,
                                  np.zeros(1, np.uint8), np.zeros(len(ko), np.uint64))


def check(ctx, tree, probes, want, pick=None):
    """lsm_search with and without the Seek tree against `want` (the
    reference of the distinct probes; pick: the batch is probes[pick]).
    -> (level, table, res, val) of the run with the tree."""
    kb, ko = csr(probes)
    if pick is not None:  # the batch's CSR gathered from the distinct probes'
        start = ko.astype(np.int64)
        ln = (start[1:] - start[:-1])[pick]
        off = np.zeros(len(pick) + 1, np.int64)
        off[1:] = np.cumsum(ln)
        src = np.repeat(start[:-1][pick] - off[:-1], ln) + np.arange(int(off[-1]), dtype=np.int64)
        kb, ko = kb[src], off.astype(np.uint64)
    batch = to_batch(ctx, kb, ko)
    wl, wt, wr, wo, wn = [x if pick is None else x[pick] for x in want[:5]]
    out = None
    for tr in (None, tree.tree):
        level, table, res, val = lsmgpu.search(ctx, tree.d_img, tree.r, tree.level_start, batch,
                                               index=tree.index, tree=tr)
        torch.cuda.synchronize()
        level, table, res = level.cpu().numpy(), table.cpu().numpy(), res.cpu().numpy()
        val = val.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        bad = np.flatnonzero((level != wl) | (table != wt) | (res != wr) | (val["rec_off"] != wo) |
                             (val["val_len"] != wn))
        assert bad.size == 0, (tr is not None, bad.size,
                               [(int(i), level[i], wl[i], table[i], wt[i], res[i], wr[i], val[i], wo[i], wn[i])
                                for i in bad[:6]])
        assert (val["key_len"] == 0).all()
        out = (level, table, res, val)
    return out


def run(ctx, rng, levels, probes):
    tree = Tree(ctx, rng, levels)
    return tree, check(ctx, tree, probes, tree.reference(probes))


ALL_KEYS = [b"key%05d" % i for i in range(4000)]
MIXED_PROBES = ALL_KEYS + [b"", b"zzz", b"key", b"key00000\x00"]
MIXED_COUNTS = (2, 3, 5, 0, 2, 1, 0)


def mixed_levels(rng, counts=MIXED_COUNTS, per=300):
    """`per` random ids of the 4,000 per table; a level >= 1 is one sorted draw
    cut into disjoint tables; filters alternate between one that passes most
    keys (m=256, k=2) and a sharp one (m=16384, k=6)."""
    levels, t = [], 0
    for L, c in enumerate(counts):
        if L == 0:
            sets = [sorted(rng.choice(4000, per, replace=False).tolist()) for _ in range(c)]
        else:
            ids = sorted(rng.choice(4000, per * c, replace=False).tolist())
            sets = [ids[j * per:(j + 1) * per] for j in range(c)]
        lv = []
        for s in sets:
            m, k = (256, 2) if t % 2 == 0 else (16384, 6)
            lv.append(build([ALL_KEYS[i] for i in s], [b"L%d.t%d.%d" % (L, t, i) for i in s], m=m, k=k))
            t += 1
        levels.append(lv)
    return levels


@pytest.fixture(scope="module")
def mixed(ctx):
    """The mixed tree and the reference of its probes, computed once."""
    tree = Tree(ctx, np.random.default_rng(401), mixed_levels(np.random.default_rng(401)))
    return tree, tree.reference(MIXED_PROBES)


def test_mixed_tree(ctx, mixed):
    tree, want = mixed
    stats = want[5]
    print("per level (answered, false positives):", stats, "absent:", int((want[2] == ora.GET_ABSENT).sum()))
    for L, c in enumerate(MIXED_COUNTS):
        if c:  # what makes the comparison meaningful, on the oracle's answer
            assert stats[L][0] >= 50, (L, stats)
            assert L == 0 or stats[L][1] >= 100, (L, stats)
    assert (want[2] == ora.GET_ABSENT).sum() >= 1000
    check(ctx, tree, MIXED_PROBES, want)


def test_shadowing(ctx):
    """The shallowest level answers: level 0 over levels 2 and 4; a tombstone
    at level 1 over a live value at level 3 is FOUND at level 1 (Search does
    not interpret it); an empty value ends the search."""
    rng = np.random.default_rng(402)
    tomb = lsmgpu.TOMBSTONE
    levels = [[] for _ in range(LEVELS)]
    levels[0] = [build([b"a", b"e"], [b"zero", b""])]
    levels[1] = [build([b"d", b"x"], [tomb, b"x1"])]
    levels[2] = [build([b"a", b"b"], [b"two", b"b2"])]
    levels[3] = [build([b"d", b"e"], [b"live", b"e3"])]
    levels[4] = [build([b"a", b"c"], [b"four", b"c4"])]
    probes = [b"a", b"b", b"c", b"d", b"e", b"x", b"y"]
    tree, (level, table, res, val) = run(ctx, rng, levels, probes)
    assert level.tolist() == [0, 2, 4, 1, 0, 1, -1]
    assert table.tolist() == [0, 2, 4, 1, 0, 1, -1]
    assert res.tolist() == [ora.GET_FOUND] * 6 + [ora.GET_ABSENT]
    got = [tree.buf[int(v["rec_off"]) + 4:int(v["rec_off"]) + 4 + int(v["val_len"])].tobytes() for v in val[:6]]
    assert got == [b"zero", b"b2", b"c4", tomb, b"", b"x1"]


def test_error_ends_the_search(ctx):
    """Corrupted value offsets in a level-1 table (negative, at the file end,
    2 bytes before it, into the index), the same keys live at level 2: the
    answers are level 1's error codes, never level 2's values."""
    rng = np.random.default_rng(403)
    keys = [b"e%04d" % i for i in range(0, 400, 2)]
    im1 = build(keys, [b"one%d" % i for i in range(len(keys))], m=1 << 14, k=5)
    im2 = build(keys, [b"two%d" % i for i in range(len(keys))], m=1 << 14, k=5)
    _, meta, idesc, _, _ = ora.sst_decode(im1)
    n = im1.size
    for j, off in {0: -5, 1: n, 2: n - 2, 3: int(meta.idx_off)}.items():
        at = int(idesc["rec_off"][j]) + 4 + int(idesc["key_len"][j])
        im1[at:at + 8] = np.frombuffer(int(off).to_bytes(8, "little", signed=True), np.uint8)
    levels = [[], [im1], [im2], [], [], [], []]
    probes = keys + [b"e%04d" % i for i in range(1, 400, 2)]
    _, (level, table, res, val) = run(ctx, rng, levels, probes)
    assert res[0] == ora.GET_SEEK_FAILED
    assert set(res[:4].tolist()) >= {ora.GET_SEEK_FAILED, ora.GET_VALUE_LENGTH}
    # an offset into the index decodes whatever bytes lie there: level 1's answer all the same
    assert (res[:3] > ora.GET_FOUND).all() and (val["val_len"][:3] == 0).all()
    assert (level[:4] == 1).all() and (table[:4] == 0).all()
    assert (res[4:len(keys)] == ora.GET_FOUND).all() and (level[4:len(keys)] == 1).all()
    assert (level[len(keys):] == -1).all()


def test_edges(ctx):
    """An empty tree; only level 0; only level 6; an empty table inside a
    level; keys below a level's first MinKey and above its last MaxKey; a
    level_start that decreases."""
    rng = np.random.default_rng(404)
    probes = [b"", b"a0", b"a1", b"a2", b"a3", b"a5", b"a9", b"b", b"m1", b"m5", b"zz"]
    a = build([b"a1", b"a3", b"a5"], [b"x", b"", b"z"])
    e = build([], [])
    b = build([b"a2", b"a3", b"a9"], [b"q", b"w", b"e"])
    c = build([b"m1", b"m3"], [b"1", b"3"])
    d = build([b"m5", b"m7"], [b"5", b"7"])
    empty = [[] for _ in range(LEVELS)]
    _, (level, table, res, _) = run(ctx, rng, empty, probes)
    assert (level == -1).all() and (table == -1).all() and (res == ora.GET_ABSENT).all()
    _, (level, table, _, _) = run(ctx, rng, [[a, e, b]] + empty[1:], probes)
    assert table.tolist() == [-1, -1, 0, 2, 0, 0, 2, -1, -1, -1, -1]
    assert (level[table >= 0] == 0).all()
    _, (level, table, _, _) = run(ctx, rng, empty[:6] + [[c, d]], probes)
    assert table.tolist() == [-1] * 8 + [0, 1, -1] and (level[8:10] == 6).all()
    # an empty table first in a level (MinKey ""), and between two others at level 0
    tree, (level, table, _, _) = run(ctx, rng, [[a, e, b], [], [e, c, d]] + empty[3:], probes)
    assert table.tolist() == [-1, -1, 0, 2, 0, 0, 2, -1, 4, 5, -1]
    bad = tree.level_start.copy()
    bad[2] = 1
    kb, ko = csr(probes)
    batch = to_batch(ctx, kb, ko)
    with pytest.raises(RuntimeError, match="code -1"):
        lsmgpu.search(ctx, tree.d_img, tree.r, bad, batch, index=tree.index)
    # a workspace below lsm_search_workspace_bytes, a Seek tree built for fewer tables: LSM_ESPACE
    out = [torch.empty(len(probes), dtype=torch.int32, device=ctx.torch_device) for _ in range(3)]
    val = torch.empty((len(probes), 4), dtype=torch.int32, device=ctx.torch_device)
    with pytest.raises(RuntimeError, match="code -4"):
        lsmgpu.search_into(ctx, tree.d_img, tree.r, tree.level_start, batch, tree.index, *out, val,
                           ws=torch.empty(16, dtype=torch.uint8, device=ctx.torch_device))
    short = lsmgpu.SeekTree(tree.tree.data[:tree.tree.data.numel() // 2], tree.tree.max_nidx)
    with pytest.raises(RuntimeError, match="code -4"):
        lsmgpu.search(ctx, tree.d_img, tree.r, tree.level_start, batch, index=tree.index, tree=short)


def test_wide_level0_and_many_tables(ctx):
    """Nine tiny level-0 tables over two deeper levels, and a tree of more
    tables (2,100 two-key tables over levels 1 to 3) than the level search's
    LDS index holds."""
    rng = np.random.default_rng(405)
    space = [b"p%04d" % i for i in range(600)]
    l0 = []
    for t in range(L0_CAP + 1):
        s = sorted(rng.choice(600, 40, replace=False).tolist())
        l0.append(build([space[i] for i in s], [b"0.%d.%d" % (t, i) for i in s], m=128, k=2))
    deep = []
    for L in (1, 2):
        ids = sorted(rng.choice(600, 150, replace=False).tolist())
        deep.append([build([space[i] for i in ids[j:j + 50]], [b"%d.%d" % (L, i) for i in ids[j:j + 50]],
                           m=128, k=2) for j in (0, 50, 100)])
    probes = space + [b"", b"zzz"]
    _, (level, _, _, _) = run(ctx, rng, [l0, deep[0], deep[1], [], [], [], []], probes)
    assert {0, 1, 2, -1} <= set(level.tolist())
    # 2,100 two-key tables over levels 1 to 3
    n = MAX_TABLES + 52
    per = n // 3
    keys = [b"w%05d" % i for i in range(12 * per)]
    levels = [[] for _ in range(LEVELS)]
    for L in (1, 2, 3):
        # every level spans the key space: its table j holds keys 12j + 4(L-1) and + 2
        levels[L] = [build([keys[12 * j + 4 * (L - 1)], keys[12 * j + 4 * (L - 1) + 2]], [b"v%d" % L, b"hi"],
                           m=64, k=1) for j in range(per)]
    assert sum(len(lv) for lv in levels) == n > MAX_TABLES
    probes = keys[::5] + [b"", b"w", b"x"]
    _, (level, _, _, _) = run(ctx, rng, levels, probes)
    assert {1, 2, 3, -1} <= set(level.tolist())


def test_passes(ctx, mixed):
    """More probes than the launch has threads (8,192 workgroups of 256: one
    pass over the keys; the threads stride over the rest): just above one
    pass.  The batch indexes the mixed tree's distinct probes, so the
    oracle's answer is the one computed once."""
    tree, want = mixed
    one_pass = MAX_GRID * 256
    rng = np.random.default_rng(406)
    pick = rng.integers(0, len(MIXED_PROBES), one_pass + 12345)
    check(ctx, tree, MIXED_PROBES, want, pick=pick)


def test_production_filters(ctx):
    """go-lsm's filter shape (m = 1,600,000, k = 16: 200 KB of words, past the
    144 KiB the filter test stages in LDS), 6,000 16-byte keys per table."""
    from lsmgpu import synth
    rng = np.random.default_rng(407)
    n = 6000
    levels, t = [[] for _ in range(LEVELS)], 0
    for L, c in enumerate((2, 2, 3)):
        for j in range(c):
            # level 0: overlapping strides; deeper levels: disjoint slices, every other id
            ids = np.arange(j, 3 * n, 3)[:n] if L == 0 else np.arange(j * 2 * n, (j + 1) * 2 * n, 2) + L
            kk = synth.keys_for(ids)
            levels[L].append(build([kk[i].tobytes() for i in range(n)], [bytes([t]) * 100] * n,
                                   m=1_600_000, k=16))
            t += 1
    pk = synth.keys_for(rng.integers(0, 7 * n, 20_000))
    probes = [pk[i].tobytes() for i in range(len(pk))]
    _, (level, _, res, _) = run(ctx, rng, levels, probes)
    assert (res == ora.GET_FOUND).sum() > 5000 and {0, 1, 2, -1} <= set(level.tolist())


def test_equals_the_composition_of_the_level_calls(ctx, mixed):
    """lsm_level0_get, then lsm_level_search_get per non-empty level, the first
    answer per key selected with torch: the outputs are lsm_search's."""
    tree, want = mixed
    kb, ko = csr(MIXED_PROBES)
    batch = to_batch(ctx, kb, ko)
    n = batch.n
    dev = ctx.torch_device
    level = torch.full((n,), -1, dtype=torch.int32, device=dev)
    table = torch.full((n,), -1, dtype=torch.int32, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    val = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    for L in range(LEVELS):
        a, b = int(tree.level_start[L]), int(tree.level_start[L + 1])
        if a == b:
            continue
        r = lsmgpu.decode_sst(ctx, tree.d_img, tree.offs[a:b], tree.lens[a:b])
        if L == 0:
            t, rr, vv = lsmgpu.level0_get(ctx, tree.d_img, r, batch)
        else:
            t, _, rr, vv = lsmgpu.level_search_get(ctx, tree.d_img, r, batch)
        take = (res == lsmgpu.GET_ABSENT) & (rr != lsmgpu.GET_ABSENT)
        level = torch.where(take, torch.full_like(level, L), level)
        table = torch.where(take, t + a, table)
        res = torch.where(take, rr, res)
        val = torch.where(take[:, None], vv, val)
    for tr in (None, tree.tree):
        got = lsmgpu.search(ctx, tree.d_img, tree.r, tree.level_start, batch, index=tree.index, tree=tr)
        torch.cuda.synchronize()
        for x, y in zip(got, (level, table, res, val)):
            assert torch.equal(x, y)
