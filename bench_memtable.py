#!/usr/bin/env python3
"""Memtable flush on the device: WAL records -> each memtable's contents
(lsm_memtable_order) -> its level-0 SSTable image (memtable_flush), for 11
memtable-sized logs at once -- go-lsm's recovery maximum (memtable/manager.go:
140-180: up to 10 IMemTables and 1 MemTable) -- or, with --logs 64, the WAL
bench's batch.

The logs are generated here: 16-byte keys, 24-byte values, about a third of
the records overwrite an earlier key of the same log, and one record in 25 is
a Delete's tombstone (synth.wal_logs has no repeated keys).  Timed:

  order       lsm_memtable_order alone, over the replayed logs (one call)
  flush       replay + order + gather + layout + build, with its one read-back
  per_log     the only way to order such logs on the device without the call:
              one lsm_merge_kvs per log over that log's descriptors in
              reversed order (it keeps the first pair of a key group), one
              host synchronisation per log

The order's output is checked in closed form from the generator's arrays:
sorted, unique, survivor = last position, counts; the per-log loop must give
the same pairs; the image sizes follow from the pairs.

  python bench_memtable.py [--logs N] [--log-bytes B] [--steps K] [--warmup W]
                           [--repeats R] [--scan all|rangescan] [--out FILE]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "go-lsm_amd"))

KEY_LEN, VAL_LEN = 16, 24
TOMBSTONE = "～DELETED～".encode()
OVERWRITE, DELETE = 1 / 3, 1 / 25
ALL, RANGESCAN = 0, 1


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--logs", type=int, default=11)
    ap.add_argument("--log-bytes", type=int, default=2 * 1024 * 1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scan", choices=["all", "rangescan"], default="all")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    return ap.parse_args(argv)


def gen_log(log_bytes, seed):
    """One log of at most log_bytes -> (bytes, ids, tomb): record i writes key
    b"k%015d" % ids[i]; tomb[i] marks a tombstone value.  A record overwrites
    an earlier fresh key of this log with probability OVERWRITE."""
    rng = np.random.default_rng(seed)
    n = log_bytes // (8 + KEY_LEN + VAL_LEN)
    fresh = rng.random(n) >= OVERWRITE
    fresh[0] = True
    nfresh_before = np.cumsum(fresh) - fresh  # fresh records before i
    fresh_ids = rng.permutation(4 * n)[:int(fresh.sum())]
    pick = (rng.random(n) * np.maximum(nfresh_before, 1)).astype(np.int64)
    ids = np.where(fresh, fresh_ids[np.minimum(nfresh_before, fresh_ids.size - 1)], fresh_ids[pick])
    tomb = rng.random(n) < DELETE
    vlen = np.where(tomb, len(TOMBSTONE), VAL_LEN)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(8 + KEY_LEN + vlen)
    buf = np.zeros(int(off[-1]), np.uint8)
    o = off[:-1]
    buf[o] = KEY_LEN
    keys = np.frombuffer(b"".join(b"k%015d" % i for i in ids.tolist()), np.uint8).reshape(n, KEY_LEN)
    buf[o[:, None] + 4 + np.arange(KEY_LEN)] = keys
    buf[o + 4 + KEY_LEN] = vlen
    vals = rng.integers(97, 123, (n, VAL_LEN), dtype=np.uint8)
    live = ~tomb
    buf[o[live, None] + 8 + KEY_LEN + np.arange(VAL_LEN)] = vals[live]
    buf[o[tomb, None] + 8 + KEY_LEN + np.arange(len(TOMBSTONE))] = np.frombuffer(TOMBSTONE, np.uint8)
    return buf, ids.astype(np.int64), tomb


def expected_window(ids, tomb, scan):
    """(distinct ids sorted, their last positions, lead, cut): the memtable's
    nodes and the window [lead, cut) of them the scan delivers."""
    last = np.full(int(ids.max()) + 1 if ids.size else 1, -1, np.int64)
    np.maximum.at(last, ids, np.arange(ids.size))
    uniq = np.unique(ids)
    pos = last[uniq]
    if scan == ALL:
        return uniq, pos, 0, uniq.size
    dead = tomb[pos]
    live = np.nonzero(~dead)[0]
    lead = int(live[0]) if live.size else uniq.size
    later = np.nonzero(dead[lead:])[0]
    cut = lead + int(later[0]) if later.size else uniq.size
    return uniq, pos, lead, cut


def check_order(ids, tomb, got, scan):
    """Closed-form check of one log's delivered positions `got` (relative to
    the log).  Raises AssertionError naming the property that fails."""
    got = np.asarray(got, np.int64)
    assert ((got >= 0) & (got < ids.size)).all(), "position out of the log"
    k = ids[got]
    assert (np.diff(k) > 0).all(), "not sorted by key, or a key delivered twice"
    uniq, pos, lead, cut = expected_window(ids, tomb, scan)
    last = dict(zip(uniq.tolist(), pos.tolist()))
    assert all(last[key] == p for key, p in zip(k.tolist(), got.tolist())), "survivor is not the key's last write"
    assert got.size == cut - lead, "count: %d delivered, %d expected" % (got.size, cut - lead)
    assert got.size == 0 or k[0] == uniq[lead], "the window starts at another key"
    return got.size


def check_counts(counts, sizes):
    want = [int(sum(sizes)), int(sum(1 for s in sizes if s)), int(max(sizes, default=0))]
    assert list(counts) == want, "counts %s, expected %s" % (list(counts), want)


def main(argv=None):
    args = parse(argv)
    import torch
    import lsmgpu

    assert torch.cuda.is_available(), "bench_memtable.py needs the GPU"
    scan = ALL if args.scan == "all" else RANGESCAN
    ctx = lsmgpu.Context(0)
    dev = ctx.torch_device
    logs = [gen_log(args.log_bytes, 1000 + w) for w in range(args.logs)]
    offs, pos = [], 0
    for buf, _, _ in logs:
        offs.append(pos)
        pos += (buf.size + 15) // 16 * 16 + 16
    whole = np.zeros(pos, np.uint8)
    for (buf, _, _), o in zip(logs, offs):
        whole[o:o + buf.size] = buf
    lens = np.array([b.size for b, _, _ in logs], np.uint32)
    d_wal = lsmgpu.to_device_bytes(whole, dev)
    d_off = torch.tensor(np.array(offs, np.uint64).view(np.int64), device=dev)
    d_len = torch.tensor(lens.view(np.int32), device=dev)
    max_len = int(lens.max())
    maxrec = int(ctx.lib.lsm_max_records(lsmgpu.GRAMMAR_KV, max_len))
    nrec = [ids.size for _, ids, _ in logs]

    r = lsmgpu.wal_replay(ctx, d_wal, d_off, d_len, max_len=max_len)
    mo = lsmgpu.MemtableOrder(ctx, args.logs, int(r.desc.shape[0]), maxrec)
    bases = [o // 8 for o in offs]

    def order_step():
        lsmgpu.memtable_order_into(ctx, d_wal, r, d_off, scan, mo)

    def flush_step():
        return lsmgpu.memtable_flush(ctx, d_wal, d_off, d_len, scan, max_len=max_len)

    # the per-log loop: reversed descriptors and buffers prepared outside the timing
    rev = [torch.flip(r.desc[b:b + n], dims=[0]).contiguous() for b, n in zip(bases, nrec)]
    merges = [lsmgpu.alloc_merge(ctx, n) for n in nrec]

    def per_log_step():
        for d, mg in zip(rev, merges):
            lsmgpu.merge_kvs_into(ctx, d_wal, d, None, mg, level=0, threshold=1 << 40)

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    steps = [("per_log", per_log_step), ("order", order_step), ("flush", flush_step)]
    for _, step in steps:
        for _ in range(args.warmup):
            step()
    ms = {name: [] for name, _ in steps}
    for _ in range(args.repeats):  # alternating
        for name, step in steps:
            ms[name].append(timed(step))

    # closed-form checks of the timed outputs
    order_step()
    torch.cuda.synchronize()
    got, counts, over = mo.result()
    assert not over
    sizes = [check_order(ids, tomb, g.astype(np.int64) - b, scan)
             for (_, ids, tomb), g, b in zip(logs, got, bases)]
    check_counts(counts, sizes)
    if scan == ALL:  # the per-log loop keeps the same pairs
        per_log_step()
        torch.cuda.synchronize()
        for mg, g, b, n in zip(merges, got, bases, nrec):
            idx = mg.out[:mg.nout].cpu().numpy().view(np.uint32).astype(np.int64)
            assert np.array_equal(b + n - 1 - idx, g.astype(np.int64)), "per-log loop differs"
    fl = flush_step()
    torch.cuda.synchronize()
    filt = int(ctx.lib.lsm_filter_block_size(lsmgpu.DEFAULT_BLOOM_M))
    want_len = []
    for (_, ids, tomb), g, b in zip(logs, got, bases):
        if g.size:
            vbytes = int(np.where(tomb[g.astype(np.int64) - b], len(TOMBSTONE), VAL_LEN).sum())
            want_len.append(8 + 2 * KEY_LEN + filt + 16 * g.size + KEY_LEN * g.size + vbytes + 32)
    assert fl.file_len.tolist() == want_len and fl.log.tolist() == [w for w, s in enumerate(sizes) if s]

    def span(x):
        return {"ms_per_step": round(float(np.mean(x)), 5), "min": round(float(min(x)), 5),
                "max": round(float(max(x)), 5), "repeats": [round(float(v), 5) for v in x]}

    total = int(sum(nrec))
    k = float(np.mean(ms["order"]))
    out = {
        "metric": "M WAL records/s ordered into their memtables' contents (lsm_memtable_order, one call)",
        "unit": "M records/s", "value": round(total / (k * 1e-3) / 1e6, 2), "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True,
        "dtype": "u8", "timing": "host wall clock around K steps and one device synchronisation",
        "data": f"synthetic: {args.logs} logs of {args.log_bytes} bytes, {KEY_LEN}-byte keys, {VAL_LEN}-byte "
                "values, a third of the records overwrite an earlier key, one in 25 is a tombstone",
        "verified": "closed form per log: sorted, unique, survivor = last write, counts; the per-log "
                    "merge loop keeps the same pairs (scan all); the flush's image sizes",
        "config": {"logs": args.logs, "records": total, "delivered": int(counts[0]), "scan": args.scan,
                   "max_log_records": maxrec, "tile": lsmgpu.MEMTABLE_TILE,
                   "workspace_bytes": int(mo.workspace.numel()), "wal_bytes": int(lens.sum()),
                   "image_bytes": int(sum(want_len))},
        "order": span(ms["order"]),
        "flush": span(ms["flush"]),
        "per_log_merge_loop": span(ms["per_log"]),
        "speedup_order_vs_per_log": round(float(np.mean(ms["per_log"])) / k, 2),
        "order_slowest_beats_per_log_fastest": bool(max(ms["order"]) < min(ms["per_log"])),
    }
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
