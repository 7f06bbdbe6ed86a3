#!/usr/bin/env python3
"""Batched short range scans (YCSB E) over a whole tree: lsm_tree_scan against
lsm_search over exactly the keys the scan returned -- the only way to read
those entries without lsm_tree_scan, and it has to be told the keys.

The tree is bench_search.py's: level 0 of 3 overlapping 2 MiB tables, levels
1-4 full at go-lsm's caps (4, 8, 16, 32 tables), 16-byte keys, 100-byte
values, every image built on the device.  Ranges: lo drawn uniformly from the
tree's id space, no upper bound, limit 16 and 100, LSM_SCAN_RAW and
LSM_SCAN_LIVE (the tree holds no tombstone: the same output, LIVE reads every
answering value to know).  The timed output of every configuration is checked
in closed form: the keys are the next `limit` ids of the union of the tables'
ids, each answered by the first table that holds it.

  python bench_tree_scan.py [--steps K] [--warmup W] [--repeats R] [--ranges N] [--out FILE]

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "go-lsm_amd"))

import bench_search  # noqa: E402  (the tree recipe)

LIMITS = (16, 100)
MODES = (("raw", 0), ("live", 1))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ranges", type=int, default=1 << 16)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    return ap.parse_args(argv)


def tree_tables(level0):
    """(level, sorted ids) per table in the tree's order: level0's tables
    (newest first), then bench_search.py's levels 1-4."""
    tabs = [(0, ids) for ids in level0]
    for L, c in enumerate(bench_search.LEVEL_TABLES, start=1):
        tabs += [(L, ids) for ids in bench_search.level_ids(L, c)]
    return tabs


def answers(tabs):
    """-> (union: the tree's distinct ids, sorted; table: the first table of
    the tree's order that holds each; slot: its entry there)."""
    union = np.unique(np.concatenate([ids for _, ids in tabs]))
    table = np.full(union.size, -1, np.int64)
    slot = np.zeros(union.size, np.int64)
    for t in range(len(tabs) - 1, -1, -1):  # deeper / older first, shallower / newer overwrite
        ids = tabs[t][1]
        at = np.searchsorted(union, ids)
        table[at] = t
        slot[at] = np.arange(ids.size)
    return union, table, slot


def draw_lo(nq, space, seed):
    """lo ids drawn uniformly from [0, space)."""
    return np.random.default_rng(seed).integers(0, space, nq).astype(np.int64)


def expected(union, lo, limit):
    """The scan of [lo, no upper) with `limit`: -> (count, more, first: the
    position in union of each range's first entry)."""
    first = np.searchsorted(union, lo, side="left")
    left = union.size - first
    return np.minimum(left, limit).astype(np.uint32), (left > limit).astype(np.uint8), first


def main(argv=None):
    args = parse(argv)
    import torch
    import lsmgpu
    from lsmgpu import synth
    from bench_sstdec import level0_tables

    assert torch.cuda.is_available(), "bench_tree_scan.py needs the GPU"
    ctx = lsmgpu.Context(0)
    dev = ctx.torch_device
    l0 = level0_tables(0)
    tabs = tree_tables([ids for ids, _ in l0])
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
    r = lsmgpu.decode_sst(ctx, d_img, offs, lens)
    index = lsmgpu.level_index(ctx, d_img, r)
    tree = lsmgpu.level_get_tree(ctx, d_img, r)
    stream = torch.cuda.current_stream()

    nq = args.ranges
    union, ans_table, ans_slot = answers(tabs)
    lo_ids = draw_lo(nq, bench_search.SPACE, synth.SEED + 11)
    ranges = lsmgpu.batch_to_device(ctx, synth.keys_for(lo_ids).reshape(-1),
                                    np.arange(nq + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN),
                                    np.zeros(1, np.uint8), np.zeros(nq + 1, np.uint64))
    flags = torch.full((nq,), lsmgpu.SCAN_NO_UPPER, dtype=torch.uint8, device=dev)
    ws = lsmgpu.tree_scan_workspace(ctx, level_start, nq)
    data_off = 8 + 2 * synth.KEY_LEN + 32 + 8 * ((lsmgpu.DEFAULT_BLOOM_M + 63) // 64)
    bases = torch.from_numpy((offs // 4).astype(np.int64)).to(dev)

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

    results = []
    for limit in LIMITS:
        n = nq * limit
        out = {name: (torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.uint8, device=dev),
                      torch.empty((n, 4), dtype=torch.int32, device=dev),
                      torch.empty((n, 4), dtype=torch.int32, device=dev),
                      torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
               for name, _ in MODES}
        want_count, want_more, first = expected(union, lo_ids, limit)
        # the emitted entries, range by range: positions in union
        j = np.arange(limit, dtype=np.int64)[None, :]
        sel = j < want_count[:, None]
        at = (first[:, None] + j)[sel]
        total = int(at.size)
        # the baseline: lsm_search told exactly those keys
        probes = lsmgpu.batch_to_device(ctx, synth.keys_for(union[at]).reshape(-1),
                                        np.arange(total + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN),
                                        np.zeros(1, np.uint8), np.zeros(total + 1, np.uint64))
        s_out = (torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev),
                 torch.empty(total, dtype=torch.int32, device=dev),
                 torch.empty((total, 4), dtype=torch.int32, device=dev))
        sws = lsmgpu.search_workspace(ctx, level_start, total)

        def scan_step(mode):
            def step():
                lsmgpu.tree_scan_into(ctx, d_img, r, level_start, ranges, flags, limit, mode, index,
                                      *out["raw" if mode == 0 else "live"], tree=tree, ws=ws, stream=stream)
            return step

        def search_step():
            lsmgpu.search_into(ctx, d_img, r, level_start, probes, index, *s_out, tree=tree, ws=sws, stream=stream)

        which = [(name, scan_step(mode)) for name, mode in MODES] + [("search", search_step)]
        for _, step in which:
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in which}
        for _ in range(args.repeats):  # alternating
            for name, step in which:
                ms[name].append(timed(step))

        # closed form
        want_t = ans_table[at]
        want_v = offs[want_t].astype(np.int64) + data_off + ans_slot[at] * (4 + synth.VAL_LEN)
        d_sel = torch.from_numpy(sel.reshape(-1)).to(dev)
        d_slot = bases[torch.from_numpy(want_t).to(dev)] + torch.from_numpy(ans_slot[at]).to(dev)
        want_key = r.idx_desc[d_slot].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        for name, _ in MODES:
            count, more, key, value, table, result = out[name]
            assert np.array_equal(count.cpu().numpy().view(np.uint32), want_count), name + ": count"
            assert np.array_equal(more.cpu().numpy(), want_more), name + ": more"
            assert np.array_equal(table[d_sel].cpu().numpy().astype(np.int64), want_t), name + ": answering table"
            assert bool((result[d_sel] == lsmgpu.GET_FOUND).all()), name + ": result"
            val = value[d_sel].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
            assert np.array_equal(val["rec_off"].astype(np.int64), want_v), name + ": value view"
            assert (val["val_len"] == synth.VAL_LEN).all(), name + ": value length"
            k = key[d_sel].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
            assert np.array_equal(k["rec_off"], want_key["rec_off"]) and (k["key_len"] == synth.KEY_LEN).all(), \
                name + ": key view"
        assert np.array_equal(s_out[1].cpu().numpy().astype(np.int64), want_t), "lsm_search: answering table"
        sval = s_out[3].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        assert np.array_equal(sval["rec_off"].astype(np.int64), want_v), "lsm_search: value view"

        base = float(np.mean(ms["search"]))
        row = {"limit": limit, "ranges": nq, "entries": total,
               "search_over_the_returned_keys": dict(span(ms["search"]),
                                                     M_entries_per_s=round(total / (base * 1e-3) / 1e6, 2))}
        for name, _ in MODES:
            k = float(np.mean(ms[name]))
            row["scan_" + name] = dict(span(ms[name]), M_entries_per_s=round(total / (k * 1e-3) / 1e6, 2),
                                       ratio_to_search=round(base / k, 3))
        results.append(row)
        del out, probes, s_out

    head = results[0]["scan_live"]
    line = json.dumps({
        "metric": "M entries/s returned by short range scans over the whole tree (limit 16, LIVE)",
        "unit": "M entries/s", "value": head["M_entries_per_s"], "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "u8",
        "data": f"synthetic: bench_search.py's tree ({nfile} tables of 2 MiB, level_start {level_start.tolist()}); "
                f"{nq} ranges, lo uniform over the {bench_search.SPACE}-id space, no upper bound",
        "verified": "every configuration: count, more, and per entry the key's view, the answering table "
                    "(closed form: the first table holding the id), GET_FOUND and the value's view; the "
                    "baseline's table and value view likewise",
        "baseline": "lsm_search over exactly the keys the scan returned (it has to be told them)",
        "timing": "device events around `steps` calls, `repeats` windows alternating scan RAW / scan LIVE / search",
        "tree_keys": int(union.size), "workspace_bytes": int(ws.numel()), "seek_tree_bytes": int(tree.data.numel()),
        "results": results})
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
