#!/usr/bin/env python3
"""Batched short range scans (YCSB E) over the whole database: lsm_db_scan over
bench_get.py's 11 memtable-sized logs in front of bench_search.py's five-level
tree, against lsm_db_get (LSM_DBGET_TOMBSTONE_HIDES, memtable index and Seek
tree) told exactly the keys the scan returned -- the only way to read those
entries without the scan, and it has to be told the keys.  lsm_tree_scan over
the same ranges is timed beside them for context: it does different work (no
memtable source, other entries), so it sets no bar.

Ranges: lo drawn uniformly from the tree's id space, no upper bound, limit 16
and 100, LSM_SCAN_RAW and LSM_SCAN_LIVE (about one memtable node in ten is a
tombstone).  The timed output of every configuration is checked in closed
form: the keys are the next `limit` ids of the union of the logs' and the
tables' ids (LIVE: those whose answering entry is no tombstone), each answered
by the newest log that holds it, else by the first table that does.

  python bench_db_scan.py [--steps K] [--warmup W] [--repeats R] [--ranges N] [--out FILE]

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "go-lsm_amd"))

import bench_get  # noqa: E402  (the logs)
import bench_memtable  # noqa: E402
import bench_search  # noqa: E402  (the tree recipe)
import bench_tree_scan  # noqa: E402  (the tree's closed form)

LIMITS = (16, 100)
MODES = (("raw", 0), ("live", 1))
KEY_LEN, VAL_LEN, TOMB_LEN = bench_get.KEY_LEN, bench_get.VAL_LEN, bench_get.TOMB_LEN
SRC_MEMTABLE, SRC_SSTABLE = 0, 1


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ranges", type=int, default=1 << 16)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    return ap.parse_args(argv)


def memtable_nodes(logs, offs):
    """The memtables' answer for every id some log holds.  logs: (ids, tomb) per
    log, oldest first (bench_memtable.gen_log's arrays); offs: each log's byte
    offset in the WAL buffer.  -> (ids sorted, log: the newest log holding the
    id, rec_off: its last record there as a byte offset in the buffer, tomb)."""
    space = max(int(ids.max()) + 1 if ids.size else 1 for ids, _ in logs)
    log_of = np.full(space, -1, np.int64)
    off_of = np.zeros(space, np.int64)
    tomb_of = np.zeros(space, bool)
    for w, (ids, tomb) in enumerate(logs):  # oldest first: a newer log overwrites
        last = np.full(space, -1, np.int64)
        np.maximum.at(last, ids, np.arange(ids.size))
        held = np.flatnonzero(last >= 0)
        p = last[held]
        rec_off = np.zeros(ids.size + 1, np.int64)
        rec_off[1:] = np.cumsum(8 + KEY_LEN + np.where(tomb, TOMB_LEN, VAL_LEN))
        log_of[held] = w
        off_of[held] = int(offs[w]) + rec_off[p]
        tomb_of[held] = tomb[p]
    ids = np.flatnonzero(log_of >= 0)
    return ids, log_of[ids], off_of[ids], tomb_of[ids]


def database(mem_ids, tree_ids):
    """-> (union: every id the database holds, sorted; mem_at: the id's position
    in mem_ids or -1; tree_at: its position in tree_ids, -1 where a memtable
    answers)."""
    union = np.union1d(mem_ids, tree_ids)
    j = np.searchsorted(mem_ids, union)
    in_mem = (j < mem_ids.size) & (mem_ids[np.minimum(j, mem_ids.size - 1)] == union)
    mem_at = np.where(in_mem, j, -1)
    tree_at = np.where(in_mem, -1, np.searchsorted(tree_ids, union))
    return union, mem_at, tree_at


def expected(union, dead, lo, limit):
    """The scan of [lo, no upper) with `limit` over the entries of union that
    are not dead (RAW: none is).  -> (count, more, at: int64[nq, limit], the
    positions in union of each range's entries, -1 past count)."""
    alive = np.flatnonzero(~dead)
    first = np.searchsorted(union[alive], lo, side="left")
    left = alive.size - first
    count = np.minimum(left, limit)
    j = np.arange(limit, dtype=np.int64)[None, :]
    pick = np.minimum(first[:, None] + j, max(alive.size - 1, 0))
    at = np.where(j < count[:, None], alive[pick] if alive.size else -1, -1)
    return count.astype(np.uint32), (left > limit).astype(np.uint8), at


def main(argv=None):
    args = parse(argv)
    import torch
    import lsmgpu
    from lsmgpu import synth
    from bench_sstdec import level0_tables

    assert torch.cuda.is_available(), "bench_db_scan.py needs the GPU"
    ctx = lsmgpu.Context(0)
    dev = ctx.torch_device
    # the memtables: bench_get.py's logs, replayed and ordered
    logs = [bench_memtable.gen_log(bench_get.LOG_BYTES, 1000 + w) for w in range(bench_get.NLOG)]
    woffs, pos = [], 0
    for buf, _, _ in logs:
        woffs.append(pos)
        pos += (buf.size + 15) // 16 * 16 + 16
    whole = np.zeros(pos, np.uint8)
    for (buf, _, _), o in zip(logs, woffs):
        whole[o:o + buf.size] = buf
    wlens = np.array([b.size for b, _, _ in logs], np.uint32)
    d_wal = lsmgpu.to_device_bytes(whole, dev)
    d_off = torch.tensor(np.array(woffs, np.uint64).view(np.int64), device=dev)
    d_len = torch.tensor(wlens.view(np.int32), device=dev)
    max_len = int(wlens.max())
    rp = lsmgpu.wal_replay(ctx, d_wal, d_off, d_len, max_len=max_len)
    mo = lsmgpu.memtable_order(ctx, d_wal, rp, d_off, int(ctx.lib.lsm_max_records(lsmgpu.GRAMMAR_KV, max_len)))
    mem_index = lsmgpu.memtable_search_index(ctx, d_wal, rp, mo)
    torch.cuda.synchronize()

    # the tree: bench_search.py's, as bench_tree_scan.py builds it
    l0 = level0_tables(0)
    tabs = bench_tree_scan.tree_tables([ids for ids, _ in l0])
    counts = [3] + list(bench_search.LEVEL_TABLES) + [0, 0]
    level_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    nfile = len(tabs)
    imgs, offs, lens, pos = [], [], [], 0
    for t, (_, ids) in enumerate(tabs):
        n = ids.size
        vals = l0[t][1] if t < len(l0) else synth.value_bytes(ids + (t + 1) * 10 ** 9, synth.VAL_LEN)
        batch = lsmgpu.batch_to_device(ctx, synth.keys_for(ids).reshape(-1),
                                       np.arange(n + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN),
                                       vals.reshape(-1).copy(),
                                       np.arange(n + 1, dtype=np.uint64) * np.uint64(synth.VAL_LEN))
        sb = lsmgpu.build_sst(ctx, batch, np.array([0, n], np.uint64))
        torch.cuda.synchronize()
        size = int(sb.file_size[0])
        imgs.append(sb.out[:size].clone())
        offs.append(pos)
        lens.append(size)
        pos += (size + 15) // 16 * 16
    d_img = torch.zeros(pos + 64, dtype=torch.uint8, device=dev)
    for im, o in zip(imgs, offs):
        d_img[o:o + im.numel()] = im
    del imgs
    offs, lens = np.array(offs, np.uint64), np.array(lens, np.uint64)
    sd = lsmgpu.decode_sst(ctx, d_img, offs, lens)
    index = lsmgpu.level_index(ctx, d_img, sd)
    tree = lsmgpu.level_get_tree(ctx, d_img, sd)
    stream = torch.cuda.current_stream()

    # the closed form
    mem_ids, mem_log, mem_off, mem_tomb = memtable_nodes([(ids, tomb) for _, ids, tomb in logs], woffs)
    tree_ids, ans_table, ans_slot = bench_tree_scan.answers(tabs)
    union, mem_at, tree_at = database(mem_ids, tree_ids)
    is_mem = mem_at >= 0
    tomb = np.where(is_mem, mem_tomb[np.maximum(mem_at, 0)], False)
    data_off = 8 + 2 * synth.KEY_LEN + 32 + 8 * ((lsmgpu.DEFAULT_BLOOM_M + 63) // 64)
    bases = torch.from_numpy((offs // 4).astype(np.int64)).to(dev)

    nq = args.ranges
    lo_ids = bench_tree_scan.draw_lo(nq, bench_search.SPACE, synth.SEED + 11)
    ranges = lsmgpu.batch_to_device(ctx, synth.keys_for(lo_ids).reshape(-1),
                                    np.arange(nq + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN),
                                    np.zeros(1, np.uint8), np.zeros(nq + 1, np.uint64))
    flags = torch.full((nq,), lsmgpu.SCAN_NO_UPPER, dtype=torch.uint8, device=dev)
    ws = lsmgpu.db_scan_workspace(ctx, mo.nlog, level_start, nq)
    tws = lsmgpu.tree_scan_workspace(ctx, level_start, nq)

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            step()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def span(x):
        return {"us_per_call": round(float(np.mean(x)) * 1e3, 2), "min": round(float(min(x)) * 1e3, 2),
                "max": round(float(max(x)) * 1e3, 2), "repeats": [round(float(v) * 1e3, 2) for v in x]}

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)

    results = []
    for limit in LIMITS:
        n = nq * limit
        out = {name: lsmgpu.DbScan(i32(nq), torch.empty(nq, dtype=torch.uint8, device=dev), i32(n, 4), i32(n, 4),
                                   i32(n), i32(n), i32(n)) for name, _ in MODES}
        t_out = (i32(nq), torch.empty(nq, dtype=torch.uint8, device=dev), i32(n, 4), i32(n, 4), i32(n), i32(n))
        want = {name: expected(union, tomb if mode == 1 else np.zeros(union.size, bool), lo_ids, limit)
                for name, mode in MODES}
        # the baseline of each mode: lsm_db_get told exactly the keys that scan returned
        probes, g_out, gws, total = {}, {}, {}, {}
        for name, _ in MODES:
            at = want[name][2]
            at = at[at >= 0]
            total[name] = int(at.size)
            probes[name] = lsmgpu.batch_to_device(
                ctx, synth.keys_for(union[at]).reshape(-1),
                np.arange(at.size + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN),
                np.zeros(1, np.uint8), np.zeros(at.size + 1, np.uint64))
            g_out[name] = lsmgpu.alloc_db_get(ctx, at.size)
            gws[name] = lsmgpu.search_workspace(ctx, level_start, at.size)

        def scan_step(name, mode):
            def step():
                lsmgpu.db_scan_into(ctx, d_wal, rp, mo, d_img, sd, level_start, ranges, flags, limit, mode, index,
                                    out[name], mem_index=mem_index, tree=tree, ws=ws, stream=stream)
            return step

        def get_step(name):
            def step():
                lsmgpu.db_get_into(ctx, d_wal, rp, mo, d_img, sd, level_start, probes[name], index, g_out[name],
                                   mode=lsmgpu.DBGET_TOMBSTONE_HIDES, mem_index=mem_index, tree=tree,
                                   ws=gws[name], stream=stream)
            return step

        def tree_step():
            lsmgpu.tree_scan_into(ctx, d_img, sd, level_start, ranges, flags, limit, 1, index, *t_out, tree=tree,
                                  ws=tws, stream=stream)

        which = []
        for name, mode in MODES:
            which += [("scan_" + name, scan_step(name, mode)), ("get_" + name, get_step(name))]
        which.append(("tree_scan_live", tree_step))
        for _, step in which:
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in which}
        for _ in range(args.repeats):  # alternating
            for name, step in which:
                ms[name].append(timed(step))

        # closed form
        row = {"limit": limit, "ranges": nq}
        for name, _ in MODES:
            want_count, want_more, at2 = want[name]
            sel = at2 >= 0
            at = at2[sel]
            o = out[name]
            assert np.array_equal(o.count.cpu().numpy().view(np.uint32), want_count), name + ": count"
            assert np.array_equal(o.more.cpu().numpy(), want_more), name + ": more"
            d_sel = torch.from_numpy(sel.reshape(-1)).to(dev)
            mem = is_mem[at]
            src = o.src[d_sel].cpu().numpy()
            assert np.array_equal(src, np.where(mem, SRC_MEMTABLE, SRC_SSTABLE)), name + ": source"
            ma, ta = mem_at[at][mem], tree_at[at][~mem]
            want_t = np.where(mem, 0, 0).astype(np.int64)
            want_t[mem] = mem_log[ma]
            want_t[~mem] = ans_table[ta]
            assert np.array_equal(o.table[d_sel].cpu().numpy().astype(np.int64), want_t), name + ": log / table"
            assert bool((o.result[d_sel] == lsmgpu.GET_FOUND).all()), name + ": result"
            want_k = np.zeros(at.size, np.int64)
            want_v = np.zeros(at.size, np.int64)
            want_vl = np.zeros(at.size, np.int64)
            want_k[mem] = mem_off[ma]
            want_v[mem] = mem_off[ma] + 4 + KEY_LEN
            want_vl[mem] = np.where(mem_tomb[ma], TOMB_LEN, VAL_LEN)
            t_of = ans_table[ta]
            d_slot = bases[torch.from_numpy(t_of).to(dev)] + torch.from_numpy(ans_slot[ta]).to(dev)
            want_k[~mem] = sd.idx_desc[d_slot].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)["rec_off"]
            want_v[~mem] = offs[t_of].astype(np.int64) + data_off + ans_slot[ta] * (4 + synth.VAL_LEN)
            want_vl[~mem] = synth.VAL_LEN
            k = o.key[d_sel].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
            v = o.value[d_sel].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
            assert np.array_equal(k["rec_off"].astype(np.int64), want_k) and (k["key_len"] == KEY_LEN).all(), \
                name + ": key view"
            assert np.array_equal(v["rec_off"].astype(np.int64), want_v), name + ": value view"
            assert np.array_equal(v["val_len"].astype(np.int64), want_vl), name + ": value length"
            # the baseline read the same entries: the same source, and the same view where it returns one
            g = g_out[name]
            gsrc = g.src[:at.size].cpu().numpy()
            assert np.array_equal(gsrc, np.where(mem, SRC_MEMTABLE, SRC_SSTABLE)), name + ": lsm_db_get's source"
            gv = g.value[:at.size].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
            live = ~tomb[at]
            assert np.array_equal(gv["rec_off"].astype(np.int64)[live], want_v[live]), name + ": lsm_db_get's view"
            base, kk = float(np.mean(ms["get_" + name])), float(np.mean(ms["scan_" + name]))
            row["entries_" + name] = total[name]
            row["from_memtables_" + name] = int(mem.sum())
            row["db_get_over_the_returned_keys_" + name] = dict(
                span(ms["get_" + name]), M_entries_per_s=round(total[name] / (base * 1e-3) / 1e6, 2))
            row["scan_" + name] = dict(span(ms["scan_" + name]),
                                       M_entries_per_s=round(total[name] / (kk * 1e-3) / 1e6, 2),
                                       ratio_to_db_get=round(base / kk, 3))
        row["tree_scan_live_same_ranges"] = span(ms["tree_scan_live"])
        results.append(row)
        del out, probes, g_out, t_out

    head = results[0]["scan_live"]
    line = json.dumps({
        "metric": "M entries/s returned by short range scans over the memtables and the tree (limit 16, LIVE)",
        "unit": "M entries/s", "value": head["M_entries_per_s"], "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "u8",
        "data": f"synthetic: bench_get.py's {mo.nlog} logs of {bench_get.LOG_BYTES} bytes ({int(mem_ids.size)} "
                f"distinct keys, {int(mem_tomb.sum())} answered by a tombstone) over bench_search.py's tree "
                f"({nfile} tables of 2 MiB, level_start {level_start.tolist()}); {nq} ranges, lo uniform over the "
                f"{bench_search.SPACE}-id space, no upper bound",
        "verified": "every configuration: count, more, and per entry the source, the log or table (closed form: "
                    "the newest log holding the id, else the first table), GET_FOUND, the key's and the value's "
                    "view; the baseline's source and value view likewise",
        "baseline": "lsm_db_get (TOMBSTONE_HIDES, memtable index, Seek tree) over exactly the keys the scan "
                    "returned (it has to be told them)",
        "context": "tree_scan_live_same_ranges: lsm_tree_scan over the same ranges -- no memtable source, other "
                   "entries; reported, not a bar",
        "timing": "device events around `steps` calls, `repeats` windows alternating scan / db_get per mode, "
                  "then tree_scan",
        "database_keys": int(union.size), "workspace_bytes": int(ws.numel()),
        "results": results})
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
