"""GPU parity of lsm_memtable_search (with its index and without) and of
lsm_db_get: memtable.Manager.Search and database.Get for a batch of keys over
the memtables lsm_memtable_order delivers and a tree of SSTables.

Every comparison is exact, against the short form of memtable_search_ref.py
(pinned to the restated skiplist in test_memtable_search_ref.py) over the
oracle's decode of each log, and against search_ref.search for the tables.
The helpers that put logs and trees on the device are those of
test_memtable_gpu.py and test_search_gpu.py.  T = lsmgpu.MEMTABLE_TILE.
"""
import numpy as np
import pytest
import torch

import lsmgpu
import memtable_search_ref as ref
import pyoracle as ora
import search_ref
from search_ref import csr
from test_memtable_gpu import TOMBSTONE_LOGS, Case, random_log, rec
from test_search_gpu import ALL_KEYS, Tree, mixed_levels, to_batch

pytestmark = pytest.mark.gpu

T = lsmgpu.MEMTABLE_TILE
TOMB = lsmgpu.TOMBSTONE
MAX_GRID = 2048  # workgroups of one lsm_memtable_search launch (kMsMaxGrid)
NONE = 0xFFFFFFFF


class Mem:
    """Logs (oldest first) replayed and ordered on the device, the search index,
    and the reference's view of them: per log its records and descriptors from
    the oracle, None for a log without nodes (failed, or in `skip`)."""

    def __init__(self, ctx, logs, placement="offset", maxrec=None, skip=()):
        self.ctx = ctx
        self.c = c = Case(ctx, logs, placement)
        self.mo = lsmgpu.memtable_order(ctx, c.d, c.r, c.off, c.maxrec if maxrec is None else maxrec,
                                        lsmgpu.MEMTABLE_ALL)
        self.index = lsmgpu.memtable_search_index(ctx, c.d, c.r, self.mo)
        self.desc = [ora.decode_block(ora.GRAMMAR_KV, c.buf, int(o), int(n))[1] for o, n in zip(c.offs, c.lens)]
        self.logs = [None if st != 0 or w in skip else recs for w, (st, recs) in enumerate(c.decoded)]
        self.tables = [None if lg is None else ref.last_positions(lg) for lg in self.logs]

    def want(self, probes):
        """-> (result, log, slot, value offset, value length) per probe."""
        n = len(probes)
        res, log = np.zeros(n, np.int32), np.full(n, -1, np.int32)
        slot, voff, vlen = np.full(n, NONE, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        for i, key in enumerate(probes):
            r, w, pos, _ = ref.search(self.logs, key, self.tables)
            res[i], log[i] = r, w
            if r != ref.MISS:
                slot[i] = self.c.bases[w] + pos
            if r == ref.VALUE:
                d = self.desc[w][pos]
                voff[i] = int(d["rec_off"]) + 4 + int(d["key_len"])
                vlen[i] = d["val_len"]
        return res, log, slot, voff, vlen

    def value_bytes(self, voff, vlen):
        return self.c.buf[int(voff) + 4:int(voff) + 4 + int(vlen)].tobytes()


def gather(kb, ko, pick):
    """The CSR batch probes[pick] from the distinct probes' CSR."""
    start = ko.astype(np.int64)
    ln = (start[1:] - start[:-1])[pick]
    off = np.zeros(len(pick) + 1, np.int64)
    off[1:] = np.cumsum(ln)
    src = np.repeat(start[:-1][pick] - off[:-1], ln) + np.arange(int(off[-1]), dtype=np.int64)
    return kb[src], off.astype(np.uint64)


def check(mem, probes, want=None, pick=None):
    """lsm_memtable_search with the index and without it against the
    reference of the distinct probes (pick: the batch is probes[pick])."""
    want = mem.want(probes) if want is None else want
    kb, ko = csr(probes)
    if pick is not None:
        kb, ko = gather(kb, ko, pick)
        want = [x[pick] for x in want]
    batch = to_batch(mem.ctx, kb, ko)
    c = mem.c
    for index in (mem.index, None):
        res, log, slot, val = lsmgpu.memtable_search(mem.ctx, c.d, c.r, mem.mo, batch, index=index)
        torch.cuda.synchronize()
        res, log = res.cpu().numpy(), log.cpu().numpy()
        slot = slot.cpu().numpy().view(np.uint32)
        val = val.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        bad = np.flatnonzero((res != want[0]) | (log != want[1]) | (slot != want[2]) |
                             (val["rec_off"] != want[3]) | (val["val_len"] != want[4]) | (val["key_len"] != 0))
        assert bad.size == 0, (index is not None, bad.size,
                               [(int(i), res[i], want[0][i], log[i], want[1][i], slot[i], want[2][i], val[i])
                                for i in bad[:6]])
    return want


def neighbours(keys):
    out = []
    for k in keys:
        out += [k, k + b"\x00", k[:-1]]
    return out


# ---- node counts per log ---------------------------------------------------------

COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, T - 1, T, T + 1, 2 * T + 1]


def log_with_nodes(rng, n, pool):
    """A log whose memtable holds exactly n nodes: n distinct keys of the pool,
    a third of them written twice, one write in ten a tombstone, shuffled."""
    ids = rng.choice(pool, n, replace=False)
    ids = np.concatenate([ids, ids[:n // 3]])
    rng.shuffle(ids)
    return b"".join(rec(b"k_%05d" % i, TOMB if rng.random() < 0.1 else b"v%d.%d" % (i, j))
                    for j, i in enumerate(ids.tolist()))


@pytest.mark.parametrize("placement", ["offset", "plan"])
def test_node_counts_around_the_tile_both_placements(ctx, placement):
    rng = np.random.default_rng(501)
    counts = COUNTS[::-1]  # the large memtables oldest: the small ones over them answer their keys
    mem = Mem(ctx, [log_with_nodes(rng, n, 3 * T) for n in counts], placement)
    torch.cuda.synchronize()
    assert [len(x) for x in mem.mo.result()[0]] == counts
    keys = sorted({k for lg in mem.logs for k, _ in lg})
    # every key present, its two near misses, one key below the smallest, one above the largest, the empty key
    probes = neighbours(keys) + [b"a", b"zzz", b""]
    assert b"a" < keys[0] and keys[-1] < b"zzz"
    want = check(mem, probes)
    assert set(want[0].tolist()) == {ref.MISS, ref.VALUE, ref.DELETED}
    assert set(want[1].tolist()) == set(range(len(COUNTS) - 1)) | {-1}  # every log with nodes answers some key


# ---- comparator ----------------------------------------------------------------------

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


def test_comparator_go_string_order_any_key_length(ctx):
    """The comparator keys are the nodes of one log; they and their near
    neighbours (one byte more, one byte less, the last byte one up or down)
    are the probes: a probe is found exactly when it is a node."""
    rng = np.random.default_rng(502)
    keys = comparator_keys()
    order = rng.permutation(len(keys))
    log = b"".join(rec(keys[i], b"v%d" % i) for i in order)
    mem = Mem(ctx, [log])
    probes = set(neighbours(keys))
    for k in keys:
        if k:
            probes.add(k[:-1] + bytes([(k[-1] + 1) & 0xFF]))
            probes.add(k[:-1] + bytes([(k[-1] - 1) & 0xFF]))
    probes = sorted(probes)
    want = check(mem, probes)
    found = [p for p, r in zip(probes, want[0]) if r == ref.VALUE]
    assert found == sorted(keys) and len(probes) > 2 * len(keys)
    for p, o, n in zip(probes, want[3], want[4]):
        if p in keys:
            assert mem.value_bytes(o, n) == b"v%d" % keys.index(p)


# ---- precedence ------------------------------------------------------------------------

def test_newest_log_wins_and_a_tombstone_hides_the_older_value(ctx):
    rng = np.random.default_rng(503)
    logs = [random_log(rng, 500, nkeys=300, p_tomb=0.2) for _ in range(4)]  # oldest first, shared keys
    logs[0] += rec(b"hidden", b"old value") + rec(b"empty", b"x") + rec(b"kept", b"oldest")
    logs[2] += rec(b"hidden", TOMB) + rec(b"empty", b"") + b"".join(rec(k, v) for k, v in TOMBSTONE_LOGS["ordinary"])
    logs[3] += rec(b"reborn", TOMB) + rec(b"reborn", b"again")
    mem = Mem(ctx, logs)
    probes = [b"k_%d" % i for i in range(305)] + [b"hidden", b"empty", b"kept", b"reborn", b"a", b"b", b"c", b"d",
                                                  b"", b"nothing"]
    want = check(mem, probes)
    at = {p: i for i, p in enumerate(probes)}
    res, log, _, voff, vlen = want
    assert (res[at[b"hidden"]], log[at[b"hidden"]]) == (ref.DELETED, 2)  # not log 0's value
    assert (res[at[b"empty"]], log[at[b"empty"]], vlen[at[b"empty"]]) == (ref.VALUE, 2, 0)
    assert (res[at[b"kept"]], log[at[b"kept"]]) == (ref.VALUE, 0)
    assert (res[at[b"reborn"]], log[at[b"reborn"]]) == (ref.VALUE, 3)
    # the look-alikes of the tombstone are ordinary values
    for k, v in TOMBSTONE_LOGS["ordinary"]:
        i = at[k]
        assert res[i] == ref.VALUE and log[i] == 2 and mem.value_bytes(voff[i], vlen[i]) == v
    # every log answers, and some tombstone sits over an older value
    assert set(log.tolist()) == {-1, 0, 1, 2, 3}
    older = [p for p in probes[:300] if res[at[p]] == ref.DELETED and
             any(p in mem.tables[w] for w in range(log[at[p]]))]
    assert len(older) > 10


# ---- logs without nodes -------------------------------------------------------------------

def test_failed_empty_and_overflowed_logs_answer_nothing(ctx):
    rng = np.random.default_rng(504)
    good0, good1 = random_log(rng, 250, nkeys=200), random_log(rng, 290, nkeys=200)
    cut = random_log(rng, 200, nkeys=200)[:-3]       # a record cut short: wal.Recover fails
    big = random_log(rng, 1500, nkeys=200)           # more records than max_log_records
    newest_cut = random_log(rng, 100, nkeys=200)[:-1]
    mem = Mem(ctx, [good0, cut, b"", big, good1, newest_cut], maxrec=300, skip={3})
    torch.cuda.synchronize()
    per_log, _, over = mem.mo.result()
    assert over and [len(x) > 0 for x in per_log] == [True, False, False, False, True, False]
    assert [st for st, _ in mem.c.decoded] == [0, 6, 0, 0, 0, 6]
    probes = [b"k_%d" % i for i in range(205)] + [b""]
    want = check(mem, probes)
    assert set(want[1].tolist()) == {-1, 0, 4}
    # keys only the node-less logs hold are misses
    lost = [p for p in probes[:200] if want[0][probes.index(p)] == ref.MISS and
            any(p == k for w in (1, 3, 5) for k, _ in mem.c.decoded[w][1])]
    assert lost


# ---- batch sizes -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shared(ctx):
    """Three logs and the reference of their distinct probes, computed once."""
    rng = np.random.default_rng(505)
    mem = Mem(ctx, [random_log(rng, T + 100, nkeys=600), random_log(rng, 700, nkeys=600),
                    random_log(rng, 300, nkeys=600)])
    probes = [b"k_%d" % i for i in range(640)] + [b"", b"zzz"]
    return mem, probes, mem.want(probes)


@pytest.mark.parametrize("nkeys", [1, 255, 256, 257])
def test_batch_sizes_around_a_workgroup(ctx, shared, nkeys):
    mem, probes, want = shared
    pick = np.random.default_rng(nkeys).integers(0, len(probes), nkeys)
    check(mem, probes, want, pick=pick)


def test_more_keys_than_one_pass_of_the_grid(ctx, shared):
    """2,048 workgroups of 256 threads: the threads stride over the rest."""
    mem, probes, want = shared
    pick = np.random.default_rng(506).integers(0, len(probes), MAX_GRID * 256 + 257)
    check(mem, probes, want, pick=pick)


def test_index_built_for_fewer_nodes_gives_the_same_answers(ctx, shared):
    """An index with room for the first log only: the other logs are searched
    through d_idx.  No logs at all: every key misses."""
    mem, probes, want = shared
    c = mem.c
    per_log = [len(x) for x in mem.mo.result()[0]]
    small = lsmgpu.MemtableOrder(ctx, mem.mo.nlog, per_log[0] + 5, mem.mo.max_log_records)
    small.idx, small.fsc, small.file_start = mem.mo.idx, mem.mo.fsc, mem.mo.file_start
    full = mem.index
    mem.index = lsmgpu.memtable_search_index(ctx, c.d, c.r, small)
    assert mem.index.numel() < full.numel()
    try:
        check(mem, probes, want)
    finally:
        mem.index = full
    kb, ko = csr(probes)
    none = lsmgpu.MemtableOrder(ctx, 0, mem.mo.nslot, mem.mo.max_log_records)
    res, log, slot, val = lsmgpu.memtable_search(ctx, c.d, c.r, none, to_batch(ctx, kb, ko))
    torch.cuda.synchronize()
    assert (res == 0).all() and (log == -1).all() and (slot == -1).all() and (val == 0).all()


# ---- lsm_db_get -------------------------------------------------------------------------------------

ERROR_TEXT = {ora.GET_SEEK_FAILED: "seek", ora.GET_VALUE_LENGTH: "length", ora.GET_VALUE_TOO_LONG: "too long",
              ora.GET_VALUE_SHORT: "short"}


def db_levels(rng):
    """test_search_gpu's mixed tree with four value offsets of its first
    level-1 table corrupted: those keys answer with error codes."""
    levels = mixed_levels(rng)
    im = levels[1][0]
    _, meta, idesc, _, _ = ora.sst_decode(im)
    for j, off in {0: -5, 1: im.size, 2: im.size - 2, 3: -1}.items():
        at = int(idesc["rec_off"][j]) + 4 + int(idesc["key_len"][j])
        im[at:at + 8] = np.frombuffer(int(off).to_bytes(8, "little", signed=True), np.uint8)
    return levels


def db_logs(rng, tree_want, probes):
    """Three logs over the tree's key space and the keys the cases need: a
    tombstone over a table's value, a value over a table's value, a tombstone
    over an older memtable value, keys only the memtables hold."""
    _, _, tres, _, _, _ = tree_want
    in_tables = [p for p, r in zip(probes, tres) if r == ora.GET_FOUND]
    absent = [p for p, r in zip(probes, tres) if r == ora.GET_ABSENT]
    errors = [p for p, r in zip(probes, tres) if r > ora.GET_FOUND]
    assert len(in_tables) > 1000 and len(absent) > 1000 and len(errors) >= 2
    pick = lambda pool, n: [pool[2 + i] for i in rng.choice(len(pool) - 2, n, replace=False)]  # noqa: E731
    logs = []
    for w in range(3):
        recs = [(k, b"m%d." % w + k) for k in pick(in_tables, 150) + pick(absent, 150)]
        recs += [(k, TOMB) for k in pick(in_tables, 60) + pick(absent, 40)]
        recs += [(k, b"") for k in pick(in_tables, 10)]
        rng.shuffle(recs)
        logs.append(recs)
    logs[0].append((errors[0], b"a value over the table's error"))
    logs[2].append((in_tables[0], TOMB))          # uncovers / hides the table's value
    logs[1].append((in_tables[1], b"both"))       # present in both
    return [b"".join(rec(k, v) for k, v in lg) for lg in logs], in_tables, errors


@pytest.fixture(scope="module")
def db(ctx):
    rng = np.random.default_rng(507)
    tree = Tree(ctx, rng, db_levels(np.random.default_rng(507)))
    probes = ALL_KEYS + [b"", b"zzz", b"key", b"key00000\x00"]
    tree_want = tree.reference(probes)
    logs, in_tables, errors = db_logs(rng, tree_want, probes)
    mem = Mem(ctx, logs)
    return tree, mem, probes, tree_want, mem.want(probes), in_tables, errors


def db_expected(tree, mem_want, tree_want, probes, mode):
    """lsm_db_get's outputs: the memtable's for every key, the tree's
    (search_ref.search over the keys that went on) for those, and the view."""
    res, log, slot, voff, vlen = mem_want
    n = len(probes)
    on = np.array([ref.goes_on(r, mode) for r in res])
    level, table, tres = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    off, ln = np.where(on, 0, voff).astype(np.uint64), np.where(on, 0, vlen).astype(np.uint32)
    src = np.where(on, ref.SRC_NONE, ref.SRC_MEMTABLE).astype(np.int32)
    if on.any() and tree_want is not None:
        # Search answers a key whatever the batch around it: the reference of the keys that went on
        kb, ko = csr([p for p, g in zip(probes, on) if g])
        sub = search_ref.search(tree.buf, tree.offs, tree.lens, tree.dec, tree.level_start, kb, ko, int(on.sum()))
        for x, full in zip(sub[:5], tree_want[:5]):
            assert np.array_equal(x, full[on])
        level[on], table[on], tres[on], off[on], ln[on] = sub[:5]
        src[on] = np.where(sub[2] == ora.GET_ABSENT, ref.SRC_NONE, ref.SRC_SSTABLE)
    return on, (res, log, slot, level, table, tres, off, ln, src)


def run_db_get(ctx, tree, mem, probes, mode, mem_index, seek_tree):
    kb, ko = csr(probes)
    c = mem.c
    out = lsmgpu.db_get(ctx, c.d, c.r, mem.mo, tree.d_img, tree.r, tree.level_start, to_batch(ctx, kb, ko),
                        mode=mode, index=tree.index if tree.r.nfile else None, mem_index=mem_index,
                        tree=seek_tree)
    torch.cuda.synchronize()
    val = out.value.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
    assert (val["key_len"] == 0).all()
    return (out.mem_result.cpu().numpy(), out.log.cpu().numpy(), out.slot.cpu().numpy().view(np.uint32),
            out.level.cpu().numpy(), out.table.cpu().numpy(), out.result.cpu().numpy(), val["rec_off"],
            val["val_len"], out.src.cpu().numpy())


NAMES = ("mem_result", "log", "slot", "level", "table", "result", "value offset", "value length", "src")


def compare(got, want):
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, bad.size, [(int(i), g[i], w[i]) for i in bad[:6]])


@pytest.mark.parametrize("mode", [lsmgpu.DBGET_EXACT, lsmgpu.DBGET_TOMBSTONE_HIDES])
def test_db_get_both_modes_with_and_without_the_index_and_the_seek_tree(ctx, db, mode):
    tree, mem, probes, tree_want, mem_want, in_tables, errors = db
    on, want = db_expected(tree, mem_want, tree_want, probes, mode)
    for mem_index, seek_tree in ((mem.index, tree.tree), (None, None), (mem.index, None)):
        got = run_db_get(ctx, tree, mem, probes, mode, mem_index, seek_tree)
        compare(got, want)
    at = {p: i for i, p in enumerate(probes)}
    res, src, tres = want[0], want[8], want[5]
    # the tombstone over a table's value: uncovered as written, hidden in the recommended mode
    i = at[in_tables[0]]
    assert res[i] == ref.DELETED and want[1][i] == 2
    if mode == lsmgpu.DBGET_EXACT:
        assert (src[i], tres[i]) == (ref.SRC_SSTABLE, ora.GET_FOUND) and want[7][i] > 0
    else:
        assert (src[i], tres[i], want[6][i], want[7][i]) == (ref.SRC_MEMTABLE, ora.GET_ABSENT, 0, 0)
    # present in both: the memtable's value, no table output
    i = at[in_tables[1]]
    assert (res[i], src[i], want[3][i], want[4][i], tres[i]) == (ref.VALUE, ref.SRC_MEMTABLE, -1, -1, 0)
    assert mem.value_bytes(want[6][i], want[7][i]) == b"both"
    # a table's error code passes through with SRC_SSTABLE; one is answered by the memtable first
    err = [at[k] for k in errors]
    assert src[err[0]] == ref.SRC_MEMTABLE
    passed = [i for i in err[1:] if on[i]]
    assert passed and all(tres[i] > ora.GET_FOUND and src[i] == ref.SRC_SSTABLE and want[7][i] == 0 for i in passed)
    assert {ref.SRC_NONE, ref.SRC_MEMTABLE, ref.SRC_SSTABLE} == set(src.tolist())
    # the table outputs of the keys that went on are lsm_search's of those same keys
    kb, ko = csr([p for p, g in zip(probes, on) if g])
    lv, tb, rs, vv = lsmgpu.search(ctx, tree.d_img, tree.r, tree.level_start, to_batch(ctx, kb, ko),
                                   index=tree.index, tree=tree.tree)
    torch.cuda.synchronize()
    vv = vv.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
    compare((lv.cpu().numpy(), tb.cpu().numpy(), rs.cpu().numpy(), vv["rec_off"], vv["val_len"]),
            [x[on] for x in want[3:8]])
    # database.Get, restated, over the recovered memtables and the reference's Search
    mgr = ref.Manager.recover([lg for lg in mem.logs])
    _, _, wres, woff, wlen, _ = tree_want

    def sst(key):
        j = at[key]
        if wres[j] > ora.GET_FOUND:
            return None, ERROR_TEXT[int(wres[j])]
        if wres[j] == ora.GET_ABSENT:
            return None, None
        return tree.buf[int(woff[j]) + 4:int(woff[j]) + 4 + int(wlen[j])].tobytes(), None
    differ = 0
    for i, key in enumerate(probes):
        s, o, n, r = int(src[i]), want[6][i], want[7][i], int(tres[i])
        value = None if s == ref.SRC_NONE or r > ora.GET_FOUND else \
            (mem.value_bytes(o, n) if s == ref.SRC_MEMTABLE else tree.buf[int(o) + 4:int(o) + 4 + int(n)].tobytes())
        if s == ref.SRC_MEMTABLE and res[i] == ref.DELETED:
            value = None
        got = (value, ERROR_TEXT.get(r))
        exact = ref.database_get(mgr.search, sst, key)
        if mode == lsmgpu.DBGET_EXACT:
            assert got == exact, key
        else:
            assert got == ref.get(mem.logs, sst, key, mode, mem.tables)[1:], key
            differ += got != exact
    assert mode == lsmgpu.DBGET_EXACT or differ > 20  # the modes differ where a tombstone covers a table's answer


def test_db_get_without_logs_and_with_an_empty_tree(ctx, db):
    tree, mem, probes, tree_want, mem_want, _, _ = db
    # nlog == 0: lsm_search's answers
    no_logs = Mem.__new__(Mem)
    no_logs.c, no_logs.mo = mem.c, lsmgpu.MemtableOrder(ctx, 0, mem.mo.nslot, mem.mo.max_log_records)
    n = len(probes)
    miss = (np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full(n, NONE, np.uint32), np.zeros(n, np.uint64),
            np.zeros(n, np.uint32))
    for mode in (lsmgpu.DBGET_EXACT, lsmgpu.DBGET_TOMBSTONE_HIDES):
        on, want = db_expected(tree, miss, tree_want, probes, mode)
        assert on.all()
        compare(run_db_get(ctx, tree, no_logs, probes, mode, None, tree.tree), want)
        compare(want[3:8], tree_want[:5])
    # an empty tree: the memtables' answers, nothing from the tables
    empty = Tree(ctx, np.random.default_rng(508), [[] for _ in range(search_ref.LEVELS)])
    for mode in (lsmgpu.DBGET_EXACT, lsmgpu.DBGET_TOMBSTONE_HIDES):
        on, want = db_expected(empty, mem_want, None, probes, mode)
        got = run_db_get(ctx, empty, mem, probes, mode, mem.index, None)
        compare(got, want)
        assert (got[3] == -1).all() and (got[5] == ora.GET_ABSENT).all()
        deleted = want[0] == ref.DELETED
        assert deleted.any()
        assert (got[8][deleted] == (ref.SRC_NONE if mode == lsmgpu.DBGET_EXACT else ref.SRC_MEMTABLE)).all()


# ---- graph capture ---------------------------------------------------------------------------------------

def test_index_build_and_db_get_are_capturable_in_a_graph(ctx, db):
    """Captured once, replayed over new logs written into the same buffers."""
    tree, _, probes, tree_want, _, in_tables, _ = db
    rng = np.random.default_rng(509)

    def make(n0, n1):
        return [b"".join(rec(k, TOMB if rng.random() < 0.2 else b"g." + k)
                         for k in (probes[i] for i in rng.integers(0, 4000, n))) for n in (n0, n1)]
    first, second = make(T + 200, 300), make(T // 2 + 7, 120)
    mem = Mem(ctx, first)
    c = mem.c
    kb, ko = csr(probes)
    batch = to_batch(ctx, kb, ko)
    out = lsmgpu.alloc_db_get(ctx, batch.n)
    ws = lsmgpu.search_workspace(ctx, tree.level_start, batch.n)
    mode = lsmgpu.DBGET_TOMBSTONE_HIDES

    def step():
        lsmgpu.memtable_search_index(ctx, c.d, c.r, mem.mo, index=mem.index)
        lsmgpu.db_get_into(ctx, c.d, c.r, mem.mo, tree.d_img, tree.r, tree.level_start, batch, tree.index, out,
                           mode=mode, mem_index=mem.index, tree=tree.tree, ws=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for logs in (first, second):
        assert all(len(a) <= len(b) for a, b in zip(logs, first))
        buf = c.buf.copy()
        lens = np.array([len(x) for x in logs], np.uint32)
        for o, lg in zip(c.offs, logs):
            buf[int(o):int(o) + len(lg)] = np.frombuffer(lg, np.uint8)
        c.d[:buf.size].copy_(torch.from_numpy(buf))
        c.len.copy_(torch.from_numpy(lens.view(np.int32)))
        lsmgpu.wal_replay_into(ctx, c.d, c.off, c.len, c.max_len, c.r, lsmgpu.wal_workspace(ctx, 2, c.max_len))
        lsmgpu.memtable_order_into(ctx, c.d, c.r, c.off, lsmgpu.MEMTABLE_ALL, mem.mo)
        for t in (out.mem_result, out.log, out.slot, out.level, out.table, out.result, out.value, out.src):
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        now = Mem.__new__(Mem)  # the reference's view of the logs now in the buffers
        now.c = Case.__new__(Case)
        now.c.buf, now.c.bases = buf, c.bases
        dec = [ora.decode_block(ora.GRAMMAR_KV, buf, int(o), int(n)) for o, n in zip(c.offs, lens)]
        assert all(st == 0 for st, _, _ in dec)
        now.desc = [d for _, d, _ in dec]
        raw = buf.tobytes()
        now.logs = [[(raw[o + 4:o + 4 + kl], raw[o + 8 + kl:o + 8 + kl + vl])
                     for o, kl, vl in zip(d["rec_off"].tolist(), d["key_len"].tolist(), d["val_len"].tolist())]
                    for d in now.desc]
        now.tables = [ref.last_positions(lg) for lg in now.logs]
        _, want = db_expected(tree, now.want(probes), tree_want, probes, mode)
        val = out.value.cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        compare((out.mem_result.cpu().numpy(), out.log.cpu().numpy(), out.slot.cpu().numpy().view(np.uint32),
                 out.level.cpu().numpy(), out.table.cpu().numpy(), out.result.cpu().numpy(), val["rec_off"],
                 val["val_len"], out.src.cpu().numpy()), want)


# ---- one full-size case --------------------------------------------------------------------------------------

def test_full_size_eleven_memtables_200k_probes(ctx):
    """go-lsm's recovery maximum, 11 logs of 2 MiB, checked in closed form
    from the generator's ids (bench_get.expected_memtable)."""
    import bench_get
    import bench_memtable
    logs = [bench_memtable.gen_log(2 * 1024 * 1024, 1000 + w) for w in range(11)]
    offs, pos = [], 0
    for buf, _, _ in logs:
        offs.append(pos)
        pos += (buf.size + 15) // 16 * 16 + 16
    whole = np.zeros(pos, np.uint8)
    for (buf, _, _), o in zip(logs, offs):
        whole[o:o + buf.size] = buf
    lens = np.array([b.size for b, _, _ in logs], np.uint32)
    dev = ctx.torch_device
    d_wal = lsmgpu.to_device_bytes(whole, dev)
    d_off = torch.tensor(np.array(offs, np.uint64).view(np.int64), device=dev)
    d_len = torch.tensor(lens.view(np.int32), device=dev)
    r = lsmgpu.wal_replay(ctx, d_wal, d_off, d_len, max_len=int(lens.max()))
    mo = lsmgpu.memtable_order(ctx, d_wal, r, d_off, int(ctx.lib.lsm_max_records(lsmgpu.GRAMMAR_KV, int(lens.max()))))
    index = lsmgpu.memtable_search_index(ctx, d_wal, r, mo)
    rng = np.random.default_rng(510)
    nid = 4 * max(ids.size for _, ids, _ in logs)
    probe_ids = rng.integers(0, nid + nid // 8, 200_000)  # an eighth above every log's ids
    kb = np.frombuffer(b"".join(b"k%015d" % i for i in probe_ids.tolist()), np.uint8)
    ko = np.arange(probe_ids.size + 1, dtype=np.uint64) * 16
    batch = to_batch(ctx, kb, ko)
    want = bench_get.expected_memtable([(ids, tomb) for _, ids, tomb in logs], offs, probe_ids)
    assert {0, 1, 2} == set(want[0].tolist()) and set(want[1].tolist()) == set(range(-1, 11))
    for ix in (index, None):
        got = lsmgpu.memtable_search(ctx, d_wal, r, mo, batch, index=ix)
        torch.cuda.synchronize()
        bench_get.check_memtable(got, want)
