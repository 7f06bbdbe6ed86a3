#!/usr/bin/env python3
"""database.Put / database.Delete for a batch on the device (lsm_db_write):
the write-ahead logs with memtable rotation, and their descriptors.

1M ops by default: 16-byte keys drawn from a key space small enough that a key
repeats inside a 2 MiB log, 100-byte values, 10 % Deletes, mem_max 2 MiB.
Timed, alternating, in one process:

  db_write        lsm_db_write of the batch (descriptors and main slots written)
  copy            a device-to-device copy of as many bytes as the logs hold
  db_write_puts   the same batch with every op a Put (no presence to find)
  encode_blocks   lsm_encode_blocks(KV) over the same records with the logs'
                  rec_start / out_off computed on the host: the only way the
                  library made these bytes on the device before lsm_db_write

and, from a profiler window of the same process, the time of each kernel group
of lsm_db_write (rotation, presence, layout, emit).

The outputs are checked in closed form on the host: the log count, each log's
first op, bytes and records, the counts, every op's main slot, and the bytes of
a sample of records; the delete-free logs equal lsm_encode_blocks' bytes.

  python bench_write.py [--ops N] [--keyspace K] [--deletes P] [--mem-max B]
                        [--steps K] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "go-lsm_amd"))

KEY_LEN, VAL_LEN, TOMB_LEN = 16, 100, 13
GROUPS = {  # kernel name fragment -> group
    "wr_est": "rotation", "scan_partials": "scans_of_tile_sums", "wr_next": "rotation", "wr_chase": "rotation",
    "wr_seg": "rotation", "mt_tile_sort": "presence", "mt_merge_pass": "presence", "wr_presence": "presence",
    "wr_stream": "layout", "wr_logs": "layout", "wr_emit": "emit",
}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ops", type=int, default=1_000_000)
    ap.add_argument("--keyspace", type=int, default=4096)
    ap.add_argument("--deletes", type=float, default=0.10)
    ap.add_argument("--mem-max", type=int, default=2 * 1024 * 1024)
    ap.add_argument("--align", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    return ap.parse_args(argv)


def gen_ops(n, keyspace, p_delete, seed=0x5EED):
    """-> (key ids, is_delete) of n ops."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, keyspace, n).astype(np.int64), rng.random(n) < p_delete


def closed_form(ids, is_del, mem_size0, mem_max, align, key_len=KEY_LEN, val_len=VAL_LEN):
    """lsm_db_write's layout for fixed-length keys and values, vectorised: the
    rotation by running est sums, a Delete's extra record when the previous op
    of its key lies in the log current before it.
    -> dict(nlog, log_start, wal_len, wal_off, rec_base, main_slot, extra, nrec, nbytes, most, mem_size)."""
    ids, is_del = np.asarray(ids, np.int64), np.asarray(is_del, bool)
    n = ids.size
    e = 16 + key_len + np.where(is_del, TOMB_LEN, val_len).astype(np.int64)
    E = np.concatenate([[0], np.cumsum(e)])
    # log 0 holds the ops that fit beside mem_size0; every further log its first op, then what fits
    starts = [0]
    a = int(np.searchsorted(E[1:], mem_max - mem_size0, side="right")) if mem_size0 <= mem_max else 0
    while a < n:
        starts.append(a)
        a = max(a + 1, int(np.searchsorted(E[1:], E[a] + mem_max, side="right")))
    log_start = np.array(starts + [n], np.int64)
    nlog = len(starts)
    seg = np.searchsorted(log_start[:nlog], np.arange(n), side="right") - 1
    before = np.concatenate([[0], seg[:-1]])  # L(i)
    order = np.argsort(ids, kind="stable")
    prev = np.full(n, -1, np.int64)
    same = ids[order][1:] == ids[order][:-1]
    prev[order[1:][same]] = order[:-1][same]
    extra = is_del & (prev >= 0) & (prev >= log_start[before])
    main_bytes = 8 + key_len + np.where(is_del, TOMB_LEN, val_len).astype(np.int64)
    extra_bytes = np.where(extra, 8 + key_len, 0).astype(np.int64)
    wal_len = np.bincount(seg, main_bytes, nlog).astype(np.int64) + np.bincount(before, extra_bytes, nlog).astype(np.int64)
    nrec = np.bincount(seg, minlength=nlog).astype(np.int64) + np.bincount(before, extra, nlog).astype(np.int64)
    wal_off = np.concatenate([[0], np.cumsum((wal_len + align - 1) // align * align)])
    rec_base = np.concatenate([[0], np.cumsum(nrec)])
    # op i's main record follows every record of ops before it, and its own extra
    main_slot = np.arange(n) + np.cumsum(extra)
    last = starts[-1]
    return dict(nlog=nlog, log_start=log_start, wal_len=wal_len, wal_off=wal_off, rec_base=rec_base,
                main_slot=main_slot, extra=extra, nrec=int(rec_base[-1]), nbytes=int(wal_off[-1]),
                most=int(nrec.max()), mem_size=int(E[n] - E[last]) + (mem_size0 if nlog == 1 else 0))


def verify(got, want):
    """got: the fields of lsmgpu.DbWriteResult (any object with them) and,
    optionally, main_slot.  Raises AssertionError naming the property that fails."""
    assert not got.overflow, "overflow"
    assert got.nlog == want["nlog"], f"the log count: {got.nlog}, the rule gives {want['nlog']}"
    assert np.array_equal(got.log_start, want["log_start"]), "each log's first op"
    assert np.array_equal(got.wal_len, want["wal_len"]), "each log's bytes"
    assert np.array_equal(got.wal_off, want["wal_off"]), "each log's offset"
    assert np.array_equal(got.rec_base, want["rec_base"]), "each log's records"
    assert got.nrec == want["nrec"], "the record count"
    assert got.nbytes == want["nbytes"], "the byte count"
    assert got.most_records == want["most"], "the most records in one log"
    assert got.mem_size == want["mem_size"], "sizeInBytes of the last log"
    slots = getattr(got, "main_slot", None)
    if slots is not None:
        assert np.array_equal(slots, want["main_slot"]), "each op's main slot"


def verify_sample(wal, desc, keys, vals, is_del, want, sample):
    """The bytes of the sampled ops' records, through their descriptors."""
    from lsmgpu import synth
    for i in sample.tolist():
        slot = int(want["main_slot"][i])
        recs = [(slot, synth.TOMBSTONE if is_del[i] else vals[i].tobytes())]
        if want["extra"][i]:
            recs.append((slot - 1, b""))
        for s, value in recs:
            o, kl, vl = int(desc[s]["rec_off"]), int(desc[s]["key_len"]), int(desc[s]["val_len"])
            assert (kl, vl) == (KEY_LEN, len(value)), "a descriptor's lengths"
            raw = wal[o:o + 8 + kl + vl].tobytes()
            assert raw == (KEY_LEN.to_bytes(4, "little") + keys[i].tobytes() + len(value).to_bytes(4, "little") +
                           value), "a record's bytes"


def kernel_groups(torch, step, calls):
    """Device time per kernel group per call, from a profiler window over
    `calls` calls -> (groups in us, None) or (None, why not)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                step()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            total = getattr(ev, "device_time_total", None)
            if total is None:
                total = getattr(ev, "cuda_time_total", 0)
            for frag, group in GROUPS.items():
                if frag in ev.key:
                    out[group] = out.get(group, 0.0) + float(total) / calls
                    break
        if not out:
            return None, "the profiler recorded no kernel of lsm_db_write"
        return {k: round(v, 2) for k, v in out.items()}, None
    except Exception as exc:  # the profiler is optional; the call times are not
        return None, f"{type(exc).__name__}: {exc}"


def main(argv=None):
    args = parse(argv)
    import torch
    import lsmgpu
    from lsmgpu import synth

    assert torch.cuda.is_available(), "bench_write.py needs the GPU"
    ctx = lsmgpu.Context(0)
    dev = ctx.torch_device
    n = args.ops
    ids, is_del = gen_ops(n, args.keyspace, args.deletes)
    keys = synth.keys_for(ids)
    vals = synth.value_bytes(np.arange(n), VAL_LEN)
    koff = np.arange(n + 1, dtype=np.uint64) * np.uint64(KEY_LEN)
    voff = np.arange(n + 1, dtype=np.uint64) * np.uint64(VAL_LEN)
    batch = lsmgpu.batch_to_device(ctx, keys.reshape(-1), koff, vals.reshape(-1), voff)
    stream = torch.cuda.current_stream()
    puts = np.zeros(n, bool)

    def prepare(kinds):
        ops = torch.from_numpy(kinds.astype(np.uint8)).to(dev)
        return ops, lsmgpu.DbWrite(ctx, n, n * KEY_LEN, n * VAL_LEN, 0, args.mem_max, align=args.align)

    ops_d, w_d = prepare(is_del)
    ops_p, w_p = prepare(puts)
    want_d = closed_form(ids, is_del, 0, args.mem_max, args.align)
    want_p = closed_form(ids, puts, 0, args.mem_max, args.align)

    # lsm_encode_blocks over the delete-free logs: block = log, placed by the host
    enc_out = torch.zeros(lsmgpu.pad16(want_p["nbytes"]), dtype=torch.uint8, device=dev)
    enc_rs = torch.from_numpy(want_p["log_start"].astype(np.int64)).to(dev)
    enc_oo = torch.from_numpy(want_p["wal_off"][:-1].astype(np.int64)).to(dev)
    copy_src = torch.zeros(want_d["nbytes"], dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)

    def db_write():
        lsmgpu.db_write_into(ctx, batch, ops_d, w_d, stream=stream)

    def db_write_puts():
        lsmgpu.db_write_into(ctx, batch, ops_p, w_p, stream=stream)

    def encode_blocks():
        lsmgpu._lib.check(ctx.lib.lsm_encode_blocks(
            ctx.handle, lsmgpu.GRAMMAR_KV, batch.keys.data_ptr(), batch.koff.data_ptr(), batch.vals.data_ptr(),
            batch.voff.data_ptr(), None, enc_rs.data_ptr(), want_p["nlog"], enc_out.data_ptr(),
            enc_oo.data_ptr(), stream.cuda_stream), "lsm_encode_blocks")

    def copy():
        copy_dst.copy_(copy_src)

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            step()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    steps = [("db_write", db_write), ("copy", copy), ("db_write_puts", db_write_puts),
             ("encode_blocks", encode_blocks)]
    for _, step in steps:
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in steps}
    for _ in range(args.repeats):  # alternating
        for name, step in steps:
            ms[name].append(timed(step))
    groups, why_not = kernel_groups(torch, db_write, max(args.warmup, 3))

    # closed-form checks of the timed outputs
    for w, want, kinds in ((w_d, want_d, is_del), (w_p, want_p, puts)):
        got = w.result()
        got.main_slot = w.main_slot[:n].cpu().numpy().view(np.uint32).astype(np.int64)
        verify(got, want)
        wal = w.wal.cpu().numpy()
        desc = w.desc[:got.nrec].cpu().numpy().view(lsmgpu.DESC_DTYPE).reshape(-1)
        sample = np.unique(np.concatenate([np.arange(min(n, 64)), np.arange(max(n - 64, 0), n),
                                           want["log_start"][:-1], np.maximum(want["log_start"][1:] - 1, 0),
                                           np.random.default_rng(1).integers(0, n, 4096)]))
        verify_sample(wal, desc, keys, vals, kinds, want, sample)
    nb = want_p["nbytes"]
    assert torch.equal(w_p.wal[:nb], enc_out[:nb]), "the delete-free logs against lsm_encode_blocks' bytes"

    def span(x, nbytes):
        mean = float(np.mean(x))
        return {"us_per_call": round(mean * 1e3, 2), "min": round(float(min(x)) * 1e3, 2),
                "max": round(float(max(x)) * 1e3, 2), "repeats": [round(float(v) * 1e3, 2) for v in x],
                "out_GiB_per_s": round(nbytes / (mean * 1e-3) / 2 ** 30, 1)}

    mean = {k: float(np.mean(v)) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / float(np.mean(v)) for k, v in ms.items()}
    out = {
        "metric": "M ops/s through database.Put / Delete on the device (lsm_db_write)",
        "unit": "M ops/s", "value": round(n / (mean["db_write"] * 1e-3) / 1e6, 2), "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True,
        "dtype": "u8", "timing": "device events around K calls on one stream; kernel groups from a profiler "
                                 "window of the same process",
        "data": f"synthetic: {n} ops, {KEY_LEN}-byte keys over {args.keyspace} ids, {VAL_LEN}-byte values, "
                f"{args.deletes:.0%} Deletes, mem_max {args.mem_max}",
        "verified": "log count, each log's first op / bytes / offset / records, the counts and every op's main "
                    "slot in closed form; the bytes of a sample of records; the delete-free logs equal "
                    "lsm_encode_blocks' bytes",
        "config": {"ops": n, "keyspace": args.keyspace, "deletes": int(is_del.sum()),
                   "extra_records": int(want_d["extra"].sum()), "logs": want_d["nlog"],
                   "records": want_d["nrec"], "bytes": want_d["nbytes"], "most_records_in_a_log": want_d["most"],
                   "logs_delete_free": want_p["nlog"], "bytes_delete_free": want_p["nbytes"],
                   "nlog_max": w_d.nlog_max, "workspace_bytes": int(w_d.workspace.numel())},
        "db_write": span(ms["db_write"], want_d["nbytes"]), "copy": span(ms["copy"], want_d["nbytes"]),
        "db_write_puts": span(ms["db_write_puts"], want_p["nbytes"]),
        "encode_blocks": span(ms["encode_blocks"], want_p["nbytes"]),
        "db_write_vs_copy": round(mean["db_write"] / mean["copy"], 2),
        "db_write_puts_vs_encode_blocks": round(mean["db_write_puts"] / mean["encode_blocks"], 2),
        "spread": {k: round(v, 3) for k, v in spread.items()},
        "kernel_groups_us_per_call": groups if groups is not None else "not measured",
    }
    if why_not:
        out["kernel_groups_not_measured_because"] = why_not
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
