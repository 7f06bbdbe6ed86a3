#!/usr/bin/env python3
"""lsm_pack_results over bench_db_scan.py's database (bench_get.py's 11 logs in
front of bench_search.py's five-level tree, 65,536 ranges, limits 16 and 100):

  (a) lsm_tree_scan RAW results packed with exact caps, timed beside
      lsm_gather_kvs (existing code) over the same entries in the same process,
      alternating.  lsm_gather_kvs is handed a dense d_idx (the pack's
      entry_slot, built outside the timed window): it moves the same bytes and
      is spared the pass over the nrow * limit slots.  The bar: the ratio pack /
      gather against 1 + (lsm_gather_kvs's spread over the repeats) + 0.10.
  (b) lsm_db_scan LIVE results (two source buffers, which lsm_gather_kvs cannot
      do) packed, beside a flat device copy of K + V bytes: context, no bar.
  (c) lsm_db_get results of 1M keys: limit 1, values only.

Every packed output is checked in closed form: entry e's key is its id's key,
its value the generator's value for the answering source (the log's bytes at
the newest record, or the answering table's value).

  python bench_pack.py [--steps K] [--warmup W] [--repeats R] [--ranges N] [--keys N] [--out FILE]

Prints one JSON line (default --out: profiles/bench_pack.json).
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "go-lsm_amd"))

import bench_db_scan  # noqa: E402  (the database's closed form)
import bench_get  # noqa: E402  (the logs, the probes)
import bench_memtable  # noqa: E402
import bench_search  # noqa: E402  (the tree recipe)
import bench_tree_scan  # noqa: E402  (the tree's closed form)
from lsmgpu import synth  # noqa: E402

LIMITS = bench_db_scan.LIMITS
KEY_LEN, MEM_VAL_LEN, TABLE_VAL_LEN = bench_db_scan.KEY_LEN, bench_db_scan.VAL_LEN, synth.VAL_LEN
HBM_PEAK_GBS = bench_search.HBM_PEAK_GBS
EXTRA_PASS_MARGIN = 0.10  # the pass over the slots: a count load per row and a flag per slot
CHUNK = 1 << 18


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ranges", type=int, default=1 << 16)
    ap.add_argument("--keys", type=int, default=1 << 20, help="the keys of (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pack.json"))
    return ap.parse_args(argv)


def table_values(ids, table):
    """The generator's value of id in table t of the tree (bench_db_scan.py's
    recipe, level 0 included): (n, TABLE_VAL_LEN) uint8."""
    return synth.value_bytes(np.asarray(ids, np.int64) + (np.asarray(table, np.int64) + 1) * 10 ** 9, TABLE_VAL_LEN)


def expected_packed(ids, is_mem, mem_off, mem_live, table, wal, with_keys=True):
    """The arenas of entries e = 0 .. E-1 in closed form.  ids[e]: the entry's
    id (its key is synth.keys_for(id)); is_mem[e]: a memtable answers, with its
    record at byte mem_off[e] of wal and mem_live[e] False where the entry packs
    no value (a tombstone the Get hides); else table[e] answers; a table < 0 is
    a miss (no value).  -> (keys uint8, koff uint64[E + 1], vals uint8, voff
    uint64[E + 1]); keys / koff None without keys."""
    ids = np.asarray(ids, np.int64)
    E = ids.size
    is_mem = np.asarray(is_mem, bool)
    table = np.asarray(table, np.int64)
    from_table = ~is_mem & (table >= 0)
    from_mem = is_mem & np.asarray(mem_live, bool)
    vlen = np.where(from_table, TABLE_VAL_LEN, np.where(from_mem, MEM_VAL_LEN, 0)).astype(np.uint64)
    voff = np.zeros(E + 1, np.uint64)
    voff[1:] = np.cumsum(vlen)
    vals = np.zeros(int(voff[-1]), np.uint8)
    width = max(TABLE_VAL_LEN, MEM_VAL_LEN)
    for c in range(0, E, CHUNK):  # a chunk's values as rows of `width` bytes, then cut to their lengths
        e = slice(c, min(c + CHUNK, E))
        rows = np.zeros((e.stop - c, width), np.uint8)
        t, m = from_table[e], from_mem[e]
        if t.any():
            rows[t, :TABLE_VAL_LEN] = table_values(ids[e][t], table[e][t])
        if m.any():
            src = np.asarray(mem_off, np.int64)[e][m] + 8 + KEY_LEN
            rows[m, :MEM_VAL_LEN] = wal[src[:, None] + np.arange(MEM_VAL_LEN)]
        keep = np.arange(width)[None, :] < vlen[e].astype(np.int64)[:, None]
        vals[int(voff[c]):int(voff[e.stop])] = rows[keep]
    if not with_keys:
        return None, None, vals, voff
    keys = synth.keys_for(ids).reshape(-1)
    koff = np.arange(E + 1, dtype=np.uint64) * np.uint64(KEY_LEN)
    return keys, koff, vals, voff


def roofline_bytes(nrow, limit, E, K, V, with_keys, with_src, with_count):
    """The bytes lsm_pack_results has to move: K + V read and written; per slot
    the descriptors (two with keys, one without) and the source word; per row
    the count; the offset arrays (koff with keys, voff), row_start and
    entry_slot written."""
    nslot = nrow * limit
    per_slot = 16 * (2 if with_keys else 1) + (4 if with_src else 0)
    offsets = 8 * (E + 1) * (2 if with_keys else 1) + 8 * (nrow + 1) + 4 * E
    return 2 * (K + V) + nslot * per_slot + (4 * nrow if with_count else 0) + offsets


def verdict(pack_ms, gather_ms):
    """(a)'s bar from the repeats: ratio = mean pack / mean gather; the margin is
    lsm_gather_kvs's own spread (max - min) / min plus EXTRA_PASS_MARGIN."""
    ratio = float(np.mean(pack_ms)) / float(np.mean(gather_ms))
    spread = (float(max(gather_ms)) - float(min(gather_ms))) / float(min(gather_ms))
    margin = spread + EXTRA_PASS_MARGIN
    return {"ratio_pack_over_gather": round(ratio, 4), "gather_spread": round(spread, 4),
            "margin": round(margin, 4), "inside_margin": bool(ratio <= 1.0 + margin)}


def log(msg):
    print("bench_pack: " + msg, file=sys.stderr, flush=True)


def span(x, nbytes=None):
    out = {"us_per_call": round(float(np.mean(x)) * 1e3, 2), "min": round(float(min(x)) * 1e3, 2),
           "max": round(float(max(x)) * 1e3, 2), "repeats": [round(float(v) * 1e3, 2) for v in x]}
    if nbytes is not None:
        gbs = nbytes / (float(np.mean(x)) * 1e-3) / 1e9
        out.update(roofline_bytes=int(nbytes), GB_per_s=round(gbs, 1),
                   fraction_of_hbm_roofline=round(gbs / HBM_PEAK_GBS, 4))
    return out


def build_database(ctx):
    """bench_db_scan.py's database on the device and its closed form."""
    import torch
    import lsmgpu
    from bench_sstdec import level0_tables

    dev = ctx.torch_device
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

    l0 = level0_tables(0)
    tabs = bench_tree_scan.tree_tables([ids for ids, _ in l0])
    counts = [3] + list(bench_search.LEVEL_TABLES) + [0, 0]
    level_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    imgs, offs, lens, pos = [], [], [], 0
    for t, (_, ids) in enumerate(tabs):
        n = ids.size
        batch = lsmgpu.batch_to_device(ctx, synth.keys_for(ids).reshape(-1),
                                       np.arange(n + 1, dtype=np.uint64) * np.uint64(KEY_LEN),
                                       table_values(ids, np.full(n, t)).reshape(-1).copy(),
                                       np.arange(n + 1, dtype=np.uint64) * np.uint64(TABLE_VAL_LEN))
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

    mem_ids, mem_log, mem_off, mem_tomb = bench_db_scan.memtable_nodes([(ids, tomb) for _, ids, tomb in logs], woffs)
    tree_ids, ans_table, _ = bench_tree_scan.answers(tabs)
    union, mem_at, tree_at = bench_db_scan.database(mem_ids, tree_ids)
    return types.SimpleNamespace(
        whole=whole, d_wal=d_wal, rp=rp, mo=mo, mem_index=mem_index, level_start=level_start, d_img=d_img, sd=sd,
        index=index, tree=tree, nfile=len(tabs), mem_ids=mem_ids, mem_off=mem_off, mem_tomb=mem_tomb,
        tree_ids=tree_ids, ans_table=ans_table, union=union, mem_at=mem_at, tree_at=tree_at)


def main(argv=None):
    args = parse(argv)
    import torch
    import lsmgpu

    assert torch.cuda.is_available(), "bench_pack.py needs the GPU"
    ctx = lsmgpu.Context(0)
    dev = ctx.torch_device
    db = build_database(ctx)
    log("the database is on the device")
    stream = torch.cuda.current_stream()
    nq = args.ranges
    lo_ids = bench_tree_scan.draw_lo(nq, bench_search.SPACE, synth.SEED + 11)
    ranges = lsmgpu.batch_to_device(ctx, synth.keys_for(lo_ids).reshape(-1),
                                    np.arange(nq + 1, dtype=np.uint64) * np.uint64(KEY_LEN),
                                    np.zeros(1, np.uint8), np.zeros(nq + 1, np.uint64))
    flags = torch.full((nq,), lsmgpu.SCAN_NO_UPPER, dtype=torch.uint8, device=dev)
    is_mem_u = db.mem_at >= 0
    tomb_u = np.where(is_mem_u, db.mem_tomb[np.maximum(db.mem_at, 0)], False)

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            step()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def run(which):
        """Warm every step up, then `repeats` windows, alternating."""
        for _, step in which:
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in which}
        for _ in range(args.repeats):
            for name, step in which:
                ms[name].append(timed(step))
        return ms

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)

    def sized(nrow, limit, value, key=None, src=None, count=None):
        """The sizing call and its read-back -> (a Packed with exact arenas, its workspace, E, K, V)."""
        ws = lsmgpu.pack_results_workspace(ctx, nrow, limit)
        p = lsmgpu.alloc_packed(ctx, nrow, limit, None, None, with_keys=key is not None)
        lsmgpu.pack_results_into(ctx, db.d_wal, db.d_img, value, p, key=key, src=src, count=count, nrow=nrow,
                                 limit=limit, ws=ws, stream=stream)
        E, K, V, over = (int(x) for x in p.counts.cpu().numpy())
        assert over == 0
        if key is not None:
            p.keys = torch.empty(max(K, 1), dtype=torch.uint8, device=dev)
        p.vals = torch.empty(max(V, 1), dtype=torch.uint8, device=dev)
        return p, ws, E, K, V

    def check(p, E, K, V, want, row_counts, slots, tag):
        """The packed output against the closed form (device-side compares of the arenas)."""
        keys, koff, vals, voff = want
        got = p.counts.cpu().numpy().view(np.uint64).tolist()
        assert got == [E, K if keys is not None else 0, V, 0], (tag, got)
        assert V == int(voff[-1]) and E == voff.size - 1, tag + ": totals"
        row_start = np.concatenate([[0], np.cumsum(row_counts.astype(np.int64))])
        assert np.array_equal(p.row_start.cpu().numpy(), row_start), tag + ": row_start"
        assert np.array_equal(p.entry_slot[:E].cpu().numpy().view(np.uint32), slots), tag + ": entry_slot"
        up = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)  # noqa: E731
        assert torch.equal(p.voff[:E + 1], up(voff, np.int64)), tag + ": voff"
        assert torch.equal(p.vals[:V], up(vals, np.uint8)), tag + ": values"
        if keys is not None:
            assert K == keys.size
            assert torch.equal(p.koff[:E + 1], up(koff, np.int64)), tag + ": koff"
            assert torch.equal(p.keys[:K], up(keys, np.uint8)), tag + ": keys"

    results = {"a_tree_scan_raw": [], "b_db_scan_live": []}
    for limit in LIMITS:
        n = nq * limit
        slot_of = lambda count: (np.arange(nq, dtype=np.int64)[:, None] * limit +  # noqa: E731
                                 np.arange(limit)[None, :])[np.arange(limit)[None, :] < count[:, None]]
        # ---- (a) lsm_tree_scan RAW, pack beside lsm_gather_kvs ---------------------------------
        t_out = (i32(nq), torch.empty(nq, dtype=torch.uint8, device=dev), i32(n, 4), i32(n, 4), i32(n), i32(n))
        lsmgpu.tree_scan_into(ctx, db.d_img, db.sd, db.level_start, ranges, flags, limit, lsmgpu.SCAN_RAW, db.index,
                              *t_out, tree=db.tree, stream=stream)
        count, _, key, value = t_out[:4]
        p, ws, E, K, V = sized(nq, limit, value, key=key, count=count)

        def pack_a():
            lsmgpu.pack_results_into(ctx, None, db.d_img, value, p, key=key, count=count, nrow=nq, limit=limit,
                                     key_cap=K, val_cap=V, ws=ws, stream=stream)

        pack_a()
        d_idx = p.entry_slot[:E].clone()  # the dense index list lsm_gather_kvs wants, outside the timed window
        g = lsmgpu.gather_kvs(ctx, db.d_img, key, value, d_idx, E, K, V, stream=stream)
        state = {"g": g}

        def gather_a():
            state["g"] = lsmgpu.gather_kvs(ctx, db.d_img, key, value, d_idx, E, K, V, stream=stream,
                                           reuse=state["g"])

        ms = run([("pack", pack_a), ("gather", gather_a)])
        want_count, _, first = bench_tree_scan.expected(db.tree_ids, lo_ids, limit)
        at = (first[:, None] + np.arange(limit)[None, :])[np.arange(limit)[None, :] < want_count[:, None]]
        want = expected_packed(db.tree_ids[at], np.zeros(at.size, bool), None, None, db.ans_table[at], None)
        check(p, E, K, V, want, want_count, slot_of(want_count), "(a) limit %d" % limit)
        g = state["g"]
        assert torch.equal(g.keys[:K], p.keys[:K]) and torch.equal(g.vals[:V], p.vals[:V]), "(a): lsm_gather_kvs"
        assert torch.equal(g.koff[:E + 1], p.koff[:E + 1]) and torch.equal(g.voff[:E + 1], p.voff[:E + 1])
        nbytes = roofline_bytes(nq, limit, E, K, V, True, False, True)
        row = {"limit": limit, "ranges": nq, "entries": E, "key_bytes": K, "value_bytes": V,
               "pack_results": span(ms["pack"], nbytes), "gather_kvs_dense_idx": span(ms["gather"])}
        row.update(verdict(ms["pack"], ms["gather"]))
        results["a_tree_scan_raw"].append(row)
        log("(a) limit %d: %s" % (limit, json.dumps(row)))
        del t_out, p, ws, g, state, d_idx, want

        # ---- (b) lsm_db_scan LIVE (two sources), pack beside a flat copy of K + V bytes -------
        out = lsmgpu.DbScan(i32(nq), torch.empty(nq, dtype=torch.uint8, device=dev), i32(n, 4), i32(n, 4), i32(n),
                            i32(n), i32(n))
        lsmgpu.db_scan_into(ctx, db.d_wal, db.rp, db.mo, db.d_img, db.sd, db.level_start, ranges, flags, limit,
                            lsmgpu.SCAN_LIVE, db.index, out, mem_index=db.mem_index, tree=db.tree, stream=stream)
        p, ws, E, K, V = sized(nq, limit, out.value, key=out.key, src=out.src, count=out.count)

        def pack_b():
            lsmgpu.pack_results_into(ctx, db.d_wal, db.d_img, out.value, p, key=out.key, src=out.src,
                                     count=out.count, nrow=nq, limit=limit, key_cap=K, val_cap=V, ws=ws,
                                     stream=stream)

        flat_src = torch.empty(K + V, dtype=torch.uint8, device=dev)
        flat_dst = torch.empty(K + V, dtype=torch.uint8, device=dev)
        ms = run([("pack", pack_b), ("flat_copy", lambda: flat_dst.copy_(flat_src))])
        want_count, _, at2 = bench_db_scan.expected(db.union, tomb_u, lo_ids, limit)
        at = at2[at2 >= 0]
        mem = is_mem_u[at]
        ma = np.maximum(db.mem_at[at], 0)
        table = np.where(mem, -1, db.ans_table[np.maximum(db.tree_at[at], 0)])
        want = expected_packed(db.union[at], mem, db.mem_off[ma], ~db.mem_tomb[ma], table, db.whole)
        check(p, E, K, V, want, want_count, slot_of(want_count), "(b) limit %d" % limit)
        nbytes = roofline_bytes(nq, limit, E, K, V, True, True, True)
        results["b_db_scan_live"].append({
            "limit": limit, "ranges": nq, "entries": E, "from_memtables": int(mem.sum()), "key_bytes": K,
            "value_bytes": V, "pack_results": span(ms["pack"], nbytes),
            "flat_copy_of_K_plus_V_bytes_context_only": span(ms["flat_copy"], 2 * (K + V))})
        log("(b) limit %d: %s" % (limit, json.dumps(results["b_db_scan_live"][-1])))
        del out, p, ws, flat_src, flat_dst, want

    # ---- (c) lsm_db_get of --keys keys: limit 1, values only ---------------------------------------
    nk = args.keys
    probe_ids, kind = bench_get.gen_probes(nk, db.mem_ids, db.tree_ids, synth.SEED + 5)
    probes = lsmgpu.batch_to_device(ctx, synth.keys_for(probe_ids).reshape(-1),
                                    np.arange(nk + 1, dtype=np.uint64) * np.uint64(KEY_LEN),
                                    np.zeros(1, np.uint8), np.zeros(nk + 1, np.uint64))
    got = lsmgpu.db_get(ctx, db.d_wal, db.rp, db.mo, db.d_img, db.sd, db.level_start, probes,
                        mode=lsmgpu.DBGET_TOMBSTONE_HIDES, index=db.index, mem_index=db.mem_index, tree=db.tree,
                        stream=stream)
    p, ws, E, K, V = sized(nk, 1, got.value, src=got.src)

    def pack_c():
        lsmgpu.pack_results_into(ctx, db.d_wal, db.d_img, got.value, p, src=got.src, nrow=nk, limit=1, val_cap=V,
                                 ws=ws, stream=stream)

    ms = run([("pack", pack_c)])
    j = np.searchsorted(db.mem_ids, probe_ids)
    in_mem = (j < db.mem_ids.size) & (db.mem_ids[np.minimum(j, db.mem_ids.size - 1)] == probe_ids)
    j = np.minimum(j, db.mem_ids.size - 1)
    t = np.searchsorted(db.tree_ids, probe_ids)
    in_tree = (t < db.tree_ids.size) & (db.tree_ids[np.minimum(t, db.tree_ids.size - 1)] == probe_ids)
    table = np.where(~in_mem & in_tree, db.ans_table[np.minimum(t, db.tree_ids.size - 1)], -1)
    assert np.array_equal(in_mem, kind == 0) and np.array_equal(table >= 0, kind == 1)
    want = expected_packed(probe_ids, in_mem, db.mem_off[j], ~db.mem_tomb[j], table, db.whole, with_keys=False)
    check(p, E, K, V, want, np.ones(nk, np.int64), np.arange(nk, dtype=np.uint32), "(c)")
    nbytes = roofline_bytes(nk, 1, E, 0, V, False, True, False)
    results["c_db_get"] = {"keys": nk, "answered_by_a_memtable": int(in_mem.sum()),
                           "answered_by_a_table": int((table >= 0).sum()), "value_bytes": V,
                           "pack_results": span(ms["pack"], nbytes)}

    head = results["a_tree_scan_raw"][0]
    line = json.dumps({
        "metric": "lsm_pack_results over lsm_tree_scan RAW results (limit 16): time relative to lsm_gather_kvs "
                  "over the same entries with a ready-made dense index",
        "unit": "ratio pack / gather", "value": head["ratio_pack_over_gather"], "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": False, "dtype": "u8",
        "data": f"synthetic: bench_db_scan.py's database -- bench_get.py's {db.mo.nlog} logs of "
                f"{bench_get.LOG_BYTES} bytes over bench_search.py's tree ({db.nfile} tables of 2 MiB, level_start "
                f"{db.level_start.tolist()}); {nq} ranges, lo uniform over the {bench_search.SPACE}-id space, no "
                f"upper bound; (c): {nk} probes, a third in a log, a third in the tables alone, a third absent",
        "verified": "every configuration: counts, row_start, entry_slot, koff, voff and both arenas in closed form "
                    "(entry e's key is its id's key, its value the generator's for the answering log or table); "
                    "(a) also byte-identical to lsm_gather_kvs",
        "bar": "(a): ratio_pack_over_gather <= 1 + gather_spread + %.2f (inside_margin)" % EXTRA_PASS_MARGIN,
        "context": "(b)'s flat copy and every fraction_of_hbm_roofline (roofline_bytes / time against "
                   f"{HBM_PEAK_GBS:.0f} GB/s) are context, not bars",
        "timing": "device events around `steps` calls, `repeats` windows, alternating between the two of a pair",
        "results": results})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
