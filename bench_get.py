#!/usr/bin/env python3
"""database.Get for a batch of keys on the device (database/database.go:24-40):
memtable.Manager.Search over bench_memtable's 11 memtable-sized logs
(lsm_memtable_search over lsm_memtable_order's output), then Manager.Search
over bench_search's five-level tree for the keys the memtables did not answer
(lsm_db_get, LSM_DBGET_TOMBSTONE_HIDES).

2^20 probes: a third written in some log (a value or a tombstone there), a
third held only by the tables, a third absent from both.  Timed:

  mem_indexed   lsm_memtable_search with the search index
  mem_plain     lsm_memtable_search without it (three dependent loads per step)
  db_get        lsm_db_get: both halves, answered keys skip the tables
  search_all    lsm_search over every key, no memtable step: all the parent
                library offers, and the lower bound for the table half

Every answer of the first three is checked in closed form from the generators'
ids: the newest log holding the key, its last record there, value or
tombstone, the value's view; for db_get also the first table holding a key that
went on, and the source.

  python bench_get.py [--probes N] [--steps K] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "go-lsm_amd"))

import bench_memtable  # noqa: E402
import bench_search  # noqa: E402

KEY_LEN, VAL_LEN, TOMB_LEN = bench_memtable.KEY_LEN, bench_memtable.VAL_LEN, len(bench_memtable.TOMBSTONE)
MISS, VALUE, DELETED = 0, 1, 2
SRC_NONE, SRC_MEMTABLE, SRC_SSTABLE = -1, 0, 1
ABSENT_ID0 = 10 ** 12  # ids no log and no table holds
NLOG, LOG_BYTES = 11, 2 * 1024 * 1024


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--probes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    return ap.parse_args(argv)


def expected_memtable(logs, offs, probe_ids):
    """Manager.Search in closed form.  logs: (ids, tomb) per log, oldest first
    (bench_memtable.gen_log's arrays); offs: each log's byte offset in the WAL
    buffer (offset placement: its first slot is offs / 8).
    -> (result, log, slot, value offset, value length) per probe."""
    probe_ids = np.asarray(probe_ids, np.int64)
    n = probe_ids.size
    res, log = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    slot = np.full(n, 0xFFFFFFFF, np.uint32)
    voff, vlen = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    for w in range(len(logs) - 1, -1, -1):  # newest first; an answered key stays answered
        ids, tomb = logs[w]
        last = np.full(int(ids.max()) + 1 if ids.size else 1, -1, np.int64)
        np.maximum.at(last, ids, np.arange(ids.size))
        inside = probe_ids < last.size
        pos = np.where(inside, last[np.minimum(probe_ids, last.size - 1)], -1)
        hit = (res == MISS) & (pos >= 0)
        p = pos[hit]
        rec_off = np.zeros(ids.size + 1, np.int64)
        rec_off[1:] = np.cumsum(8 + KEY_LEN + np.where(tomb, TOMB_LEN, VAL_LEN))
        dead = tomb[p]
        res[hit] = np.where(dead, DELETED, VALUE)
        log[hit] = w
        slot[hit] = int(offs[w]) // 8 + p
        voff[hit] = np.where(dead, 0, int(offs[w]) + rec_off[p] + 4 + KEY_LEN)
        vlen[hit] = np.where(dead, 0, VAL_LEN)
    return res, log, slot, voff, vlen


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def check_memtable(got, want):
    """got: lsm_memtable_search's (mem_result, log, slot, value[n, 4]).
    Raises AssertionError naming the property that fails."""
    res, log, slot, val = (_host(x) for x in got)
    val = np.ascontiguousarray(val).view(np.dtype([("rec_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")]))
    val = val.reshape(-1)
    assert np.array_equal(log, want[1]), "the answering log (the newest holding the key)"
    tomb = want[0] == DELETED
    assert (res[tomb] == DELETED).all(), "a tombstone answered as something else"
    assert np.array_equal(res, want[0]), "miss / value / deleted"
    assert np.array_equal(slot.view(np.uint32), want[2]), "the node (the key's last record in that log)"
    assert np.array_equal(val["rec_off"], want[3]) and np.array_equal(val["val_len"], want[4]), "the value's view"
    assert (val["key_len"] == 0).all(), "key_len of a value view"


def expected_tables(tabs, offs, level_start, probe_ids, data_off, val_len):
    """Manager.Search in closed form: the first level, in level 0 the newest
    table, holding the id (bench_search's check).  tabs: sorted ids per table.
    -> (level, table, found, value offset)."""
    n = probe_ids.size
    t_of, off = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for t in range(len(tabs) - 1, -1, -1):
        tid = tabs[t]
        j = np.searchsorted(tid, probe_ids)
        inn = (j < tid.size) & (tid[np.minimum(j, tid.size - 1)] == probe_ids)
        t_of[inn] = t
        off[inn] = int(offs[t]) + data_off + j[inn] * (4 + val_len)
    found = t_of >= 0
    lev = np.where(found, np.searchsorted(np.asarray(level_start[1:], np.int64), t_of, side="right"), -1)
    return lev, t_of, found, off


def expected_get(mem, tables, hides, table_val_len):
    """lsm_db_get's outputs from the two closed forms.
    -> (level, table, result, value offset, value length, src, went on)."""
    res, _, _, voff, vlen = mem
    lev, t_of, found, off = tables
    on = (res == MISS) | ((res == DELETED) & (not hides))
    hit = on & found
    level = np.where(hit, lev, -1).astype(np.int32)
    table = np.where(hit, t_of, -1).astype(np.int32)
    result = hit.astype(np.int32)  # LSM_GET_FOUND = 1, LSM_GET_ABSENT = 0
    o = np.where(on, np.where(hit, off, 0), voff).astype(np.uint64)
    ln = np.where(on, np.where(hit, table_val_len, 0), vlen).astype(np.uint32)
    src = np.where(on, np.where(hit, SRC_SSTABLE, SRC_NONE), SRC_MEMTABLE).astype(np.int32)
    return level, table, result, o, ln, src, on


def check_get(got, mem, want):
    """got: lsm_db_get's (mem_result, log, slot, level, table, result,
    value[n, 4], src).  Raises AssertionError naming the property that fails."""
    level, table, result, val, src = (_host(got[i]) for i in (3, 4, 5, 6, 7))
    assert np.array_equal(_host(got[0])[want[5] == SRC_MEMTABLE], mem[0][want[5] == SRC_MEMTABLE]), \
        "a tombstone or a value of the memtables answered as something else"
    assert np.array_equal(src, want[5]), "the source of the returned value"
    check_memtable((got[0], got[1], got[2], _memtable_view(got, mem)), mem)
    val = np.ascontiguousarray(val).view(np.dtype([("rec_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")]))
    val = val.reshape(-1)
    assert np.array_equal(table, want[1]) and np.array_equal(level, want[0]), "the answering table and level"
    assert np.array_equal(result, want[2]), "the table result"
    assert np.array_equal(val["rec_off"], want[3]) and np.array_equal(val["val_len"], want[4]), "the value's view"


def _memtable_view(got, mem):
    """lsm_db_get overwrites the view of a key that went on: the memtable's
    own view is checked where it is still there (the answered keys)."""
    val = _host(got[6]).copy()
    flat = np.ascontiguousarray(val).view(np.dtype([("rec_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")]))
    flat = flat.reshape(-1)
    away = _host(got[7]) != SRC_MEMTABLE
    flat["rec_off"][away] = mem[3][away]
    flat["val_len"][away] = mem[4][away]
    flat["key_len"][away] = 0
    return val


def gen_probes(nprobe, mem_ids, table_ids, seed):
    """A third written in some log, a third held only by the tables, the rest
    absent from both, shuffled -> (ids, kind): kind 0 / 1 / 2."""
    rng = np.random.default_rng(seed)
    only = np.setdiff1d(table_ids, mem_ids)
    a, b = nprobe // 3, nprobe // 3
    ids = np.concatenate([rng.choice(mem_ids, a), rng.choice(only, b),
                          rng.integers(ABSENT_ID0, 10 * ABSENT_ID0, nprobe - a - b)])
    kind = np.concatenate([np.zeros(a, np.int8), np.ones(b, np.int8), np.full(nprobe - a - b, 2, np.int8)])
    order = rng.permutation(nprobe)
    return ids[order], kind[order]


def main(argv=None):
    args = parse(argv)
    import torch
    import lsmgpu
    from lsmgpu import synth
    from bench_sstdec import level0_tables

    assert torch.cuda.is_available(), "bench_get.py needs the GPU"
    ctx = lsmgpu.Context(0)
    dev = ctx.torch_device
    # the memtables: bench_memtable's logs, replayed and ordered
    logs = [bench_memtable.gen_log(LOG_BYTES, 1000 + w) for w in range(NLOG)]
    woffs, pos = [], 0
    for buf, _, _ in logs:
        woffs.append(pos)
        pos += (buf.size + 15) // 16 * 16 + 16
    whole = np.zeros(pos, np.uint8)
    for (buf, _, _), o in zip(logs, woffs):
        whole[o:o + buf.size] = buf
    lens = np.array([b.size for b, _, _ in logs], np.uint32)
    d_wal = lsmgpu.to_device_bytes(whole, dev)
    d_off = torch.tensor(np.array(woffs, np.uint64).view(np.int64), device=dev)
    d_len = torch.tensor(lens.view(np.int32), device=dev)
    max_len = int(lens.max())
    rp = lsmgpu.wal_replay(ctx, d_wal, d_off, d_len, max_len=max_len)
    mo = lsmgpu.memtable_order(ctx, d_wal, rp, d_off, int(ctx.lib.lsm_max_records(lsmgpu.GRAMMAR_KV, max_len)))
    mem_index = lsmgpu.memtable_search_index(ctx, d_wal, rp, mo)
    torch.cuda.synchronize()
    nnode = int(mo.result()[1][0])

    # the tree: bench_search's
    tabs = [ids for ids, _ in level0_tables(0)]
    vals0 = [v for _, v in level0_tables(0)]
    vals = list(vals0)
    for L, c in enumerate(bench_search.LEVEL_TABLES, start=1):
        for ids in bench_search.level_ids(L, c):
            vals.append(synth.value_bytes(ids + (len(tabs) + 1) * 10 ** 9, synth.VAL_LEN))
            tabs.append(ids)
    counts = [3] + list(bench_search.LEVEL_TABLES) + [0, 0]
    level_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    imgs, offs, ilen, pos = [], [], [], 0
    for ids, v in zip(tabs, vals):
        n = ids.size
        batch = lsmgpu.batch_to_device(ctx, synth.keys_for(ids).reshape(-1),
                                       np.arange(n + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN),
                                       v.reshape(-1).copy(),
                                       np.arange(n + 1, dtype=np.uint64) * np.uint64(synth.VAL_LEN))
        sb = lsmgpu.build_sst(ctx, batch, np.array([0, n], np.uint64))
        torch.cuda.synchronize()
        size = int(sb.file_size[0])
        imgs.append(sb.out[:size].clone())
        offs.append(pos)
        ilen.append(size)
        pos += (size + 15) // 16 * 16
    d_img = torch.zeros(pos + 64, dtype=torch.uint8, device=dev)
    for im, o in zip(imgs, offs):
        d_img[o:o + im.numel()] = im
    del imgs
    offs, ilen = np.array(offs, np.uint64), np.array(ilen, np.uint64)
    sd = lsmgpu.decode_sst(ctx, d_img, offs, ilen)
    index = lsmgpu.level_index(ctx, d_img, sd)
    tree = lsmgpu.level_get_tree(ctx, d_img, sd)

    nprobe = args.probes
    mem_ids = np.unique(np.concatenate([ids for _, ids, _ in logs]))
    ids, kind = gen_probes(nprobe, mem_ids, np.unique(np.concatenate(tabs)), synth.SEED + 11)
    pk = synth.keys_for(ids).reshape(-1)
    pko = np.arange(nprobe + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN)
    probes = lsmgpu.batch_to_device(ctx, pk, pko, np.zeros(1, np.uint8), np.zeros(nprobe + 1, np.uint64))
    stream = torch.cuda.current_stream()

    i32 = lambda: torch.empty(nprobe, dtype=torch.int32, device=dev)  # noqa: E731
    m_out = {k: (i32(), i32(), i32(), torch.empty((nprobe, 4), dtype=torch.int32, device=dev))
             for k in ("indexed", "plain")}
    g_out = lsmgpu.alloc_db_get(ctx, nprobe)
    s_out = (i32(), i32(), i32(), torch.empty((nprobe, 4), dtype=torch.int32, device=dev))
    ws = lsmgpu.search_workspace(ctx, level_start, nprobe)
    mode = lsmgpu.DBGET_TOMBSTONE_HIDES

    def mem_indexed():
        lsmgpu.memtable_search_into(ctx, d_wal, rp, mo, probes, *m_out["indexed"], index=mem_index, stream=stream)

    def mem_plain():
        lsmgpu.memtable_search_into(ctx, d_wal, rp, mo, probes, *m_out["plain"], index=None, stream=stream)

    def db_get():
        lsmgpu.db_get_into(ctx, d_wal, rp, mo, d_img, sd, level_start, probes, index, g_out, mode=mode,
                           mem_index=mem_index, tree=tree, ws=ws, stream=stream)

    def search_all():
        lsmgpu.search_into(ctx, d_img, sd, level_start, probes, index, *s_out, tree=tree, ws=ws, stream=stream)

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            step()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    steps = [("mem_indexed", mem_indexed), ("mem_plain", mem_plain), ("db_get", db_get), ("search_all", search_all)]
    for _, step in steps:
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in steps}
    for _ in range(args.repeats):  # alternating
        for name, step in steps:
            ms[name].append(timed(step))

    # closed-form checks of the timed outputs
    mem = expected_memtable([(i, t) for _, i, t in logs], woffs, ids)
    check_memtable(m_out["indexed"], mem)
    check_memtable(m_out["plain"], mem)
    data_off = 8 + 2 * synth.KEY_LEN + 32 + 8 * ((lsmgpu.DEFAULT_BLOOM_M + 63) // 64)
    tables = expected_tables(tabs, offs, level_start, ids, data_off, synth.VAL_LEN)
    want = expected_get(mem, tables, True, synth.VAL_LEN)
    check_get((g_out.mem_result, g_out.log, g_out.slot, g_out.level, g_out.table, g_out.result, g_out.value,
               g_out.src), mem, want)
    assert (mem[0][kind == 0] != MISS).all() and (mem[0][kind != 0] == MISS).all(), "the probe mix"
    assert tables[2][kind == 1].all() and not tables[2][kind == 2].any(), "the probe mix"

    def span(x):
        return {"us_per_call": round(float(np.mean(x)) * 1e3, 2), "min": round(float(min(x)) * 1e3, 2),
                "max": round(float(max(x)) * 1e3, 2), "repeats": [round(float(v) * 1e3, 2) for v in x],
                "M_keys_per_s": round(nprobe / (float(np.mean(x)) * 1e-3) / 1e6, 1)}

    mean = {k: float(np.mean(v)) for k, v in ms.items()}
    went_on = int(want[6].sum())
    steps_per_key = float(np.log2(max(nnode / NLOG, 2)))
    out = {
        "metric": "M keys/s through database.Get on the device (lsm_db_get: memtables, then the tree)",
        "unit": "M keys/s", "value": round(nprobe / (mean["db_get"] * 1e-3) / 1e6, 2), "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True,
        "dtype": "u8", "timing": "device events around K calls on one stream",
        "data": f"synthetic: bench_memtable's {NLOG} logs of {LOG_BYTES} bytes over bench_search's tree "
                f"({len(tabs)} tables, 5 levels); probes a third written in some log, a third only in the "
                "tables, a third absent",
        "verified": "every probe of mem_indexed, mem_plain and db_get in closed form from the generators' ids: "
                    "the newest log holding the key, its last record, value or tombstone, the view; the first "
                    "table holding a key that went on; the source",
        "config": {"logs": NLOG, "memtable_nodes": nnode, "tables": len(tabs), "probes": nprobe,
                   "mode": "LSM_DBGET_TOMBSTONE_HIDES", "memtable_value": int((mem[0] == VALUE).sum()),
                   "memtable_deleted": int((mem[0] == DELETED).sum()), "went_on_to_the_tables": went_on,
                   "found_in_tables": int(want[2].sum()), "search_index_bytes": int(mem_index.numel())},
        "mem_indexed": span(ms["mem_indexed"]), "mem_plain": span(ms["mem_plain"]),
        "db_get": span(ms["db_get"]), "search_all": span(ms["search_all"]),
        "index_speedup": round(mean["mem_plain"] / mean["mem_indexed"], 2),
        "expectation": "db_get < search_all + mem_indexed (answered keys skip the tables)",
        "db_get_vs_sum": round(mean["db_get"] / (mean["search_all"] + mean["mem_indexed"]), 3),
        "expectation_holds": bool(mean["db_get"] < mean["search_all"] + mean["mem_indexed"]),
        # computed, not measured: whether the bisection's gathers are served from L2 is not known
        "computed": {"bisection_steps_per_log": round(steps_per_key, 1),
                     "index_bytes_gathered_per_key_at_most": int(16 * steps_per_key * NLOG),
                     "note": "upper bound: every log bisected to the end; a hit ends the walk"},
    }
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
