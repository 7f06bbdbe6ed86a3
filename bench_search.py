#!/usr/bin/env python3
"""Batched Manager.Search (sstable/manager.go:99-133) over a whole tree:
lsm_search against the composition of the per-level entry points
(lsm_level0_get, then lsm_level_search_get per level, then the first answer
per key selected with torch) -- what a binding can do without lsm_search and
without a host round trip.

The tree: level 0 as `bench.py --config get0` builds it (3 overlapping 2 MiB
tables of one 40,000-key space, newest first), levels 1-4 full at go-lsm's
caps (4, 8, 16, 32 tables of 2 MiB: 15,888 16-byte keys, 100-byte values),
ranges disjoint inside a level and overlapping across levels, every image
built on the device (lsmgpu.build_sst).  2^20 probes: half held somewhere in
the tree, a quarter absent inside the ranges, a quarter above them.  The timed
outputs of both are checked in closed form against the tables' contents.

  python bench_search.py [--steps K] [--warmup W] [--repeats R] [--out FILE]
  python bench_search.py --kstats kernel_stats.csv --only search|compose --steps K --into FILE
      (no GPU: adds the per-kernel times of a `rocprofv3 --kernel-trace
       --stats -- python bench_search.py --only ...` run of K steps, warm-up
       included, to a report)

Prints one JSON line.
"""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "go-lsm_amd"))

LEVEL_TABLES = (4, 8, 16, 32)  # levels 1-4 at go-lsm's 2^(L+1) caps
PER = 15_888                   # keys per 2 MiB table
SPACE = 1_200_000              # ids the deeper levels spread over
HBM_PEAK_GBS = 8000.0


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--probes", type=int, default=1 << 20)
    ap.add_argument("--only", choices=["both", "search", "compose"], default="both")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    ap.add_argument("--kstats", default=None, help="rocprofv3 kernel_stats.csv to add to --into")
    ap.add_argument("--into", default=None)
    return ap.parse_args(argv)


def merge_kstats(args):
    rows = list(csv.DictReader(open(args.kstats)))
    kernels = []
    for r in rows:
        # the timed step's own kernels (the trace also holds the tree's build and torch's)
        m = re.search(r"\b(search_kernel|level0_get_kernel|lv_classify_kernel|lv_test_kernel|level_get_kernel)"
                      r"(<[^(]*>)?", r["Name"])
        if not m:
            continue
        kernels.append({"kernel": m.group(1) + (m.group(2) or ""), "calls_per_step": int(r["Calls"]) / args.steps,
                        "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                        "us_per_step": round(float(r["TotalDurationNs"]) / args.steps / 1e3, 2)})
    rep = json.load(open(args.into))
    rep["kernels_" + args.only] = {
        "source": f"rocprofv3 --kernel-trace --stats of `bench_search.py --only {args.only}`, a run of its own",
        "steps": args.steps, "per_kernel": kernels}
    line = json.dumps(rep)
    with open(args.into, "w") as f:
        f.write(line + "\n")
    print(line)


def level_ids(L, c):
    """Level L's c tables: table j holds PER ids of its own slice of SPACE,
    evenly strided from an offset that differs per level."""
    span = SPACE // c
    stride = span // PER
    return [j * span + (L % stride) + np.arange(PER, dtype=np.int64) * stride for j in range(c)]


def main(argv=None):
    args = parse(argv)
    if args.kstats:
        return merge_kstats(args)
    import torch
    import lsmgpu
    from lsmgpu import synth
    from bench_sstdec import level0_tables

    assert torch.cuda.is_available(), "bench_search.py needs the GPU"
    ctx = lsmgpu.Context(0)
    dev = ctx.torch_device
    # (level, sorted ids, values) per table in the tree's order
    tabs = [(0, ids, vals) for ids, vals in level0_tables(0)]
    for L, c in enumerate(LEVEL_TABLES, start=1):
        for ids in level_ids(L, c):
            tabs.append((L, ids, synth.value_bytes(ids + (len(tabs) + 1) * 10 ** 9, synth.VAL_LEN)))
    counts = [3] + list(LEVEL_TABLES) + [0, 0]
    level_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    nfile = len(tabs)
    imgs, offs, lens, pos = [], [], [], 0
    for _, ids, vals in tabs:
        n = ids.size
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

    nprobe = args.probes
    rng = np.random.default_rng(synth.SEED + 9)
    union = np.unique(np.concatenate([t[1] for t in tabs]))
    missing = np.setdiff1d(np.arange(SPACE), union)
    held = rng.choice(union, nprobe // 2)
    inside = rng.choice(missing, nprobe // 4)
    above = rng.integers(10 ** 12, 10 ** 13, nprobe - nprobe // 2 - nprobe // 4)
    ids = rng.permutation(np.concatenate([held, inside, above]))
    pk = synth.keys_for(ids).reshape(-1)
    pko = np.arange(nprobe + 1, dtype=np.uint64) * np.uint64(synth.KEY_LEN)
    probes = lsmgpu.batch_to_device(ctx, pk, pko, np.zeros(1, np.uint8), np.zeros(nprobe + 1, np.uint64))
    stream = torch.cuda.current_stream()

    def outputs():
        return (torch.empty(nprobe, dtype=torch.int32, device=dev), torch.empty(nprobe, dtype=torch.int32, device=dev),
                torch.empty(nprobe, dtype=torch.int32, device=dev),
                torch.empty((nprobe, 4), dtype=torch.int32, device=dev))

    # lsm_search
    s_level, s_table, s_res, s_val = outputs()
    ws = lsmgpu.search_workspace(ctx, level_start, nprobe)
    ws_bytes = int(ctx.lib.lsm_search_workspace_bytes(level_start.ctypes.data, nprobe))

    def search_step():
        lsmgpu.search_into(ctx, d_img, r, level_start, probes, index, s_level, s_table, s_res, s_val,
                           tree=tree, ws=ws, stream=stream)

    # the composition: each level its own decode view, sparse index, Seek tree and workspace
    parts = []
    for L in range(lsmgpu.SEARCH_LEVELS):
        a, b = int(level_start[L]), int(level_start[L + 1])
        if a == b:
            continue
        rl = lsmgpu.decode_sst(ctx, d_img, offs[a:b], lens[a:b])
        parts.append({"L": L, "a": a, "r": rl, "index": lsmgpu.level_index(ctx, d_img, rl),
                      "tree": lsmgpu.level_get_tree(ctx, d_img, rl),
                      "ws": lsmgpu.level_may_contain_workspace(ctx, rl.nfile, nprobe),
                      "may": torch.empty(nprobe, dtype=torch.uint8, device=dev), "out": outputs()})
    c_out = {}

    def compose_calls():
        for p in parts:
            _, t, res, val = p["out"]
            if p["L"] == 0:
                lsmgpu.level0_get_into(ctx, d_img, p["r"], probes, t, res, val, tree=p["tree"], stream=stream)
            else:
                lsmgpu.level_search_get_into(ctx, d_img, p["r"], probes, p["index"], t, p["may"], res, val,
                                             tree=p["tree"], ws=p["ws"], stream=stream)

    def compose_select():
        # the first level whose result is not ABSENT, per key
        found = torch.stack([p["out"][2] != lsmgpu.GET_ABSENT for p in parts])
        any_found = found.any(0)
        first = found.to(torch.uint8).argmax(0)
        sel = first[None, :]
        res = torch.stack([p["out"][2] for p in parts]).gather(0, sel)[0]
        tab = torch.stack([p["out"][1] + p["a"] for p in parts]).gather(0, sel)[0]
        val = torch.stack([p["out"][3] for p in parts]).gather(0, sel[:, :, None].expand(1, nprobe, 4))[0]
        lev = torch.tensor([p["L"] for p in parts], dtype=torch.int32, device=dev)[first]
        neg = torch.full_like(tab, -1)
        c_out["v"] = (torch.where(any_found, lev, neg), torch.where(any_found, tab, neg), res, val)

    def compose_step():
        compose_calls()
        compose_select()

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            step()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    which = {"search": [("search", search_step)], "compose": [("compose", compose_step)],
             "both": [("compose", compose_step), ("compose_calls", compose_calls), ("search", search_step)]}[args.only]
    for _, step in which:
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in which}
    for _ in range(args.repeats):  # alternating
        for name, step in which:
            ms[name].append(timed(step))

    # closed form: the first level, and in level 0 the newest table, holding the key
    want_t = np.full(nprobe, -1, np.int64)
    want_off = np.zeros(nprobe, np.int64)
    data_off = 8 + 2 * synth.KEY_LEN + 32 + 8 * ((lsmgpu.DEFAULT_BLOOM_M + 63) // 64)
    for t in range(nfile - 1, -1, -1):  # deeper / older first, shallower / newer overwrite
        tid = tabs[t][1]
        j = np.searchsorted(tid, ids)
        inn = (j < tid.size) & (tid[np.minimum(j, tid.size - 1)] == ids)
        want_t[inn] = t
        want_off[inn] = int(offs[t]) + data_off + j[inn] * (4 + synth.VAL_LEN)
    found = want_t >= 0
    want_l = np.where(found, np.searchsorted(level_start[1:].astype(np.int64), want_t, side="right"), -1)

    def verify(out, what):
        lev, tab, res = (x.cpu().numpy() for x in out[:3])
        val = out[3].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        assert np.array_equal(tab.astype(np.int64), want_t), what + ": answering table"
        assert np.array_equal(lev.astype(np.int64), want_l), what + ": answering level"
        assert (res[found] == lsmgpu.GET_FOUND).all() and (res[~found] == lsmgpu.GET_ABSENT).all(), what
        assert np.array_equal(val["rec_off"][found].astype(np.int64), want_off[found]), what + ": value view"
        assert (val["val_len"][found] == synth.VAL_LEN).all() and (val["val_len"][~found] == 0).all(), what

    if "search" in ms:
        verify((s_level, s_table, s_res, s_val), "lsm_search")
    if "compose" in ms:
        verify(c_out["v"], "composition")

    def span(x):
        return {"ms_per_step": round(float(np.mean(x)), 5), "min": round(float(min(x)), 5),
                "max": round(float(max(x)), 5), "repeats": [round(float(v), 5) for v in x]}

    fbits = r.meta_numpy()["filter_nbits"].astype(np.float64)
    # algorithmic bytes per call: the probe keys and offsets read once, 28 B
    # out per probe (level, table, result, value view), every stored filter
    # word read once, and per found probe its index entry (4 + key + 8 B) and
    # the value's length prefix (4 B)
    alg = pk.size + 8.0 * (nprobe + 1) + 28.0 * nprobe + float((8 * np.ceil(fbits / 64)).sum()) + \
        float(found.sum()) * (4 + synth.KEY_LEN + 8 + 4)
    out = {
        "metric": "M keys/s looked up in the whole tree (Manager.Search: level 0, then levels 1-4)",
        "unit": "M keys/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "repeats": args.repeats, "higher_is_better": True, "dtype": "u8",
        "data": f"synthetic: level 0 of 3 overlapping 2 MiB tables (bench.py --config get0's), levels 1-4 of "
                f"{LEVEL_TABLES} disjoint 2 MiB tables over one {SPACE}-id space; probes half held, a quarter "
                "absent inside the ranges, a quarter above them",
        "verified": "every probe of both: the answering level and table = the first holding the key "
                    "(closed form from the tables' ids), its value's view; every other probe absent",
        "config": {"tables": nfile, "level_start": level_start.tolist(), "probes": nprobe,
                   "found": int(found.sum()),
                   "found_per_level": np.bincount(want_l[found], minlength=5).tolist()},
        "workspace_bytes": ws_bytes,
        "seek_tree_bytes": int(tree.data.numel()),
    }
    if "search" in ms:
        k = float(np.mean(ms["search"]))
        out["value"] = round(nprobe / (k * 1e-3) / 1e6, 2)
        out["search"] = span(ms["search"])
        out["roofline"] = {"bound": "hbm", "kernel": "lsm_search (search_kernel, one launch)",
                           "kernel_ms": round(k, 5), "achieved": round(alg / (k * 1e-3) / 1e9, 1),
                           "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(alg / (k * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "alg_bytes_per_call": int(alg)}
    if "compose" in ms:
        out["composition"] = span(ms["compose"])
        out["composition"]["what"] = ("lsm_level0_get + lsm_level_search_get x %d + the select (torch)"
                                      % (len(parts) - 1))
    if "compose_calls" in ms:
        out["composition_calls_only"] = span(ms["compose_calls"])
    if "search" in ms and "compose" in ms:
        out["speedup"] = round(float(np.mean(ms["compose"])) / float(np.mean(ms["search"])), 2)
        out["search_slowest_beats_composition_fastest"] = bool(
            max(ms["search"]) < min(ms["compose"]) and max(ms["search"]) < min(ms["compose_calls"]))
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
