"""Small adversarial inputs for steps 1-2 of lsm_merge_kvs (the key statistics,
the host's choice of a sort plan, and the ordering kernels that build `perm`),
and a census of the paths they reach.  Plain numpy and the CPU oracle: no
torch, no GPU.  The companion of tests/walk_cases.py, which does the same for
steps 3-5; Case, lay_out and Unsafe are the ones defined there.

go-lsm_amd/csrc/merge.hip orders the pairs one of three ways: not at all (no
key bit varies), by LSD radix passes over packed groups of fields, or by the
merge path (one sorted run of the input holds at least half the pairs; the
others are ranked as a k-way merge of their sorted runs or radix-sorted, and
the two sequences are ranked against each other).  Which one runs depends on
the tile summaries of merge_stats_kernel, on the OR / AND words and on four
thresholds, so a case here is named after the edge it sits on, and the plan
the host reports (lsm_merge_plan, eight words) must equal the census's.

census() restates, in Python integers and for LSM_TIE_INPUT:
  * the stats tiling (sb = min(ceil(N / 256), 1024), chunk = ceil(N / sb)),
    each tile's first, last and count of descents and, for 2..64 descents,
    its longest run strictly inside the tile; the three-way descent compare
    (32-byte prefix, lengths, whole keys);
  * the host's run stitching, the fields / and_d / minlen rule, the plan
    choice and the cutting of the fields into groups;
  * pext64 and the packed keys, the extract kernels, the three rank kernels
    (merge_rank_run_kernel, merge_rank_others_kernel, the k-way rank);
  * merge_kway_runs_kernel and merge_kway_rank_kernel: the starts list, R,
    stride, the sample bounds, the lo / hi intervals and the interval search.
rocPRIM's radix sort is taken as what it is documented to be: a stable sort
on the key bits [0, bits).

The census returns the plan, the modelled perm and a Counter of tags for every
branch taken.  It never produces expected output: that comes only from
pyoracle.merge_pairs.  Every modelled load and store is checked against the
sizes of merge_ws_layout's buffers (and a load must hit a word the call has
written, a rank store an empty slot), and the modelled perm must be a
permutation of 0..N-1, or the census raises Unsafe.

Not reachable by cases this small, and left to the full-size tests of
tests/test_merge_gpu.py: chunk > 256 in the stats loop (a thread taking more
than one pair of its tile needs N > 262,144 -- the census asserts chunk <= 256)
and per > 1 in scan_partials_kernel.

census(case, mutant=...) applies one of MUTANTS, one-line value-only changes
of steps 1-2 that were also applied to a scratch copy of merge.hip to prove
that the GPU tests bite; see the table at the end.
"""
import random
import struct
from collections import Counter

import walk_cases as wc
from walk_cases import Case, Unsafe, lay_out, expected, most_pairs  # noqa: F401 (shared with the GPU test)

MAX_PAIRS = wc.MAX_PAIRS
MAX_BYTES = 1 << 20

# merge.hip
THREADS = 256            # kMergeThreads
WAVE = 64
STAT_BLOCKS = 1024       # kStatBlocks
FAST_CHUNKS = 4          # kFastChunks
KEY_CAP = 1 << 20        # kKeyCap
MAX_CHUNKS = KEY_CAP // 8 + 1
MERGE_PATH_MIN = 4096    # kMergePathMin
GROUP_FIELDS = 8         # kGroupFields
KWAY_MAX_RUNS = 12       # kKwayMaxRuns
KWAY_THREADS = 1024      # kKwayThreads
KWAY_SAMPLES = 4096      # kKwaySamples
LEN_FIELD = 0xFFFFFFFF   # kNone as a field: the key length
M64 = (1 << 64) - 1

ORDER_IOTA, ORDER_RADIX, ORDER_PATH = 0, 1, 2
OTHERS_NONE, OTHERS_KWAY, OTHERS_RADIX = 0, 1, 2

MUTANTS = ("path_min_4097", "no_junction", "hi_plus_1", "hi_minus_1", "later_le", "rank_run_le",
           "pass_ignores_perm", "extract_shift", "stitch_ge", "width_lt_32", "kway_bound_13")


class Buf:
    """A device array of `cap` elements: a store must be in bounds, a load in
    bounds and of an element this call has stored (the tests fill the
    workspace with 0xA5; a stale word is not an index)."""

    def __init__(self, name, cap):
        self.name, self.cap, self.a = name, cap, {}

    def st(self, i, v):
        if not 0 <= i < self.cap:
            raise Unsafe("store %s[%d], %d elements" % (self.name, i, self.cap))
        self.a[i] = v

    def st_once(self, i, v):
        if i in self.a:
            raise Unsafe("%s[%d] ranked twice: another slot stays stale" % (self.name, i))
        self.st(i, v)

    def ld(self, i):
        if not 0 <= i < self.cap:
            raise Unsafe("load %s[%d], %d elements" % (self.name, i, self.cap))
        if i not in self.a:
            raise Unsafe("load %s[%d]: never stored" % (self.name, i))
        return self.a[i]


def _segments(mask):
    """pext64's loop over the runs of set bits of mask -> [(lo, len)]."""
    segs = []
    while mask:
        lo = (mask & -mask).bit_length() - 1
        m = mask >> lo
        inv = ~m & M64
        ln = ((inv & -inv).bit_length() - 1) if inv else 64 - lo
        segs.append((lo, ln))
        mask = 0 if ln + lo >= 64 else mask & ~(((1 << ln) - 1) << lo)
    return segs


def _pext(v, segs):
    r = pos = 0
    for lo, ln in segs:
        r |= ((v >> lo) if ln >= 64 else (v >> lo) & ((1 << ln) - 1)) << pos
        pos += ln
    return r & M64


class Census:
    """What census() returns.  plan: lsm_merge_plan's eight words, or None
    when the call returns LSM_EINVAL (a key past the cap); perm: the modelled
    sorted order (input indices); tags: Counter of the branches taken; R: the
    k-way rank's run count (0 off that path)."""


def census(case, mutant=None):
    assert mutant is None or mutant in MUTANTS
    keys = [k for k, _ in case.pairs]
    N = len(keys)
    kl = [len(k) for k in keys]
    CH = []
    for k in keys:
        nch = (len(k) + 7) // 8
        CH.append(struct.unpack(">%dQ" % nch, k.ljust(8 * nch, b"\0")))
    tags = Counter()
    res = Census()
    res.tags, res.plan, res.perm, res.R = tags, None, None, 0

    def chunk_of(i, d):
        c = CH[i]
        return c[d] if d < len(c) else 0

    # ---- merge_stats_kernel: one tile a workgroup --------------------------
    sb = min((N + THREADS - 1) // THREADS, STAT_BLOCKS)
    chunk = (N + sb - 1) // sb
    assert chunk <= THREADS, "a thread with two pairs of a tile: not modelled (N > 262,144)"
    tags["stats:tiles"] = sb

    def descent_cmp(i):
        """key(i) against key(i - 1) as the kernel decides it."""
        a, b = CH[i], CH[i - 1]
        for d in range(FAST_CHUNKS):
            x, y = (a[d] if d < len(a) else 0), (b[d] if d < len(b) else 0)
            if x != y:
                tags["cmp:prefix"] += 1
                return -1 if x < y else 1
        if kl[i] <= 8 * FAST_CHUNKS and kl[i - 1] <= 8 * FAST_CHUNKS:
            tags["cmp:lengths" if kl[i] != kl[i - 1] else "cmp:equal"] += 1
            return -1 if kl[i] < kl[i - 1] else 1 if kl[i] > kl[i - 1] else 0
        # key_cmp: all chunks again, then the lengths
        if min(kl[i], kl[i - 1]) <= 8 * FAST_CHUNKS:
            tags["cmp:full_one_side_le32"] += 1
        for d in range((max(kl[i], kl[i - 1]) + 7) // 8):
            x, y = chunk_of(i, d), chunk_of(i - 1, d)
            if x != y:
                assert d >= FAST_CHUNKS
                tags["cmp:full_past32"] += 1
                return -1 if x < y else 1
        tags["cmp:full_lengths" if kl[i] != kl[i - 1] else "cmp:full_equal"] += 1
        return -1 if kl[i] < kl[i - 1] else 1 if kl[i] > kl[i - 1] else 0

    part = []  # per tile: (first, last, count, inner s, inner e)
    for t in range(sb):
        lo, hi = t * chunk, min(t * chunk + chunk, N)
        desc = []
        for i in range(lo, hi):
            if i == 0:
                continue
            tid = i - lo
            tags["pred:lane0_load" if tid % WAVE == 0 else "pred:shuffle"] += 1
            if descent_cmp(i) < 0:
                desc.append(i)
                if i == lo:
                    tags["descent:tile_first"] += 1
                elif tid % WAVE == 0:
                    tags["descent:wave_lane0"] += 1
                if i == hi - 1:
                    tags["descent:tile_last"] += 1
        cnt = len(desc)
        tags["tile:descents=%d" % cnt if cnt in (0, 1, 2, 64, 65) else "tile:descents=other"] += 1
        bs = be = 0
        if 2 <= cnt <= WAVE:
            # wave_max64 of len << 32 | x: the longest, the later one on ties
            best = max(((desc[a + 1] - desc[a]) << 32 | desc[a]) for a in range(cnt - 1))
            bs = best & 0xFFFFFFFF
            be = bs + (best >> 32)
            tags["tile:inner_run"] += 1
        elif cnt > WAVE:
            tags["tile:inner_run_skipped"] += 1
        part.append((desc[0] if cnt else LEN_FIELD, desc[-1] if cnt else 0, cnt, bs, be))

    # ---- the host: run stitching --------------------------------------------
    run = [0, 0, "none"]
    cur_s = 0
    descents = 0

    def take(a, b, src):
        longer = (b - a >= run[1] - run[0]) if mutant == "stitch_ge" else (b - a > run[1] - run[0])
        if longer:
            if b - a == run[1] - run[0]:
                tags["stitch:tie_replaced"] += 1
            run[:] = [a, b, src]
        elif b - a == run[1] - run[0] and b > a:
            tags["stitch:tie_first_wins"] += 1

    for first, last, cnt, bs, be in part:
        descents += cnt
        if cnt == 0:
            tags["stitch:tile_without_descent"] += 1
            continue
        take(cur_s, first, "open")
        if be > bs:
            take(bs, be, "inner")
        cur_s = last
    take(cur_s, N, "tail")
    rs, re, src = run
    tags["run:from_%s" % src] += 1
    if rs == 0:
        tags["run:starts_at_0"] += 1
    if re == N:
        tags["run:ends_at_N"] += 1

    # ---- the fields ----------------------------------------------------------
    maxlen, minlen = max(kl), min(kl)
    D = (maxlen + 7) // 8
    if D > MAX_CHUNKS:
        tags["einval:key_past_cap"] += 1
        return res
    len_or = len_and = None
    for x in kl:
        len_or = x if len_or is None else len_or | x
        len_and = x if len_and is None else len_and & x
    orand = {}
    for d in range(max(D, FAST_CHUNKS)):
        o, a = 0, M64
        for i in range(N):
            if kl[i] > 8 * d:
                c = CH[i][d]
                o |= c
                a &= c
        orand[d] = (o, a)
    if D > FAST_CHUNKS:
        # merge_long_stats_kernel: sb x 256 threads cover every pair; its words
        # sit at stats[2 + 2d], stats[2 + 2d + 1]
        tags["long_stats:chunks"] = D - FAST_CHUNKS
        if 2 + 2 * (D - 1) + 1 >= 2 + 2 * MAX_CHUNKS:
            raise Unsafe("long-key words past w.stats")
    fields = []  # least significant first
    if len_or & ~len_and:
        fields.append((LEN_FIELD, len_or & ~len_and))
    for d in range(D - 1, -1, -1):
        and_d = orand[d][1] if minlen > 8 * d else 0
        if minlen <= 8 * d:
            tags["fields:short_keys_hold_0"] += 1
        vary = orand[d][0] & ~and_d
        if vary:
            fields.append((d, vary))
            if d >= FAST_CHUNKS:
                tags["fields:from_long_stats"] += 1
    all_bits = sum(bin(m).count("1") for _, m in fields)
    tags["fields=%d" % len(fields)] += 1
    tags["all_bits=%d" % all_bits] += 1

    segs = {m: _segments(m) for _, m in fields}

    def packed(i, group, kmask, shift=0):
        key = 0
        for f, m in group:  # most significant first
            x = kl[i] if f == LEN_FIELD else chunk_of(i, f)
            bits = bin(m).count("1")
            key = ((0 if bits >= 64 else (key << (bits + shift)) & M64) | _pext(x, segs[m]))
        return key & kmask

    nn = N
    no = N - (re - rs)
    path_min = MERGE_PATH_MIN + 1 if mutant == "path_min_4097" else MERGE_PATH_MIN
    width = others = passes = 0
    perm = None
    if fields and len(fields) <= GROUP_FIELDS and all_bits <= 64 and no <= N // 2 and N >= path_min:
        # ---- the merge path ---------------------------------------------------
        if src == "inner":
            tags["path:run_from_inner"] += 1
        width = 32 if (all_bits < 32 if mutant == "width_lt_32" else all_bits <= 32) else 64
        kmask = (1 << width) - 1
        group = fields[::-1]
        cap = nn * 8 // (width // 8)
        run_keys, okb, oib, perm0 = Buf("keys[0]", cap), Buf("keys[1]", cap), Buf("perm[1]", nn), Buf("perm[0]", nn)
        bound = KWAY_MAX_RUNS + 1 if mutant == "kway_bound_13" else KWAY_MAX_RUNS
        kway = no > 0 and descents + 2 <= bound
        others = OTHERS_KWAY if kway else OTHERS_RADIX if no else OTHERS_NONE
        nrun = re - rs
        for j in range(N):  # merge_extract_split_kernel
            pk = packed(j, group, kmask)
            if rs <= j < re:
                run_keys.st(j - rs, pk)
            else:
                q = j if j < rs else j - nrun
                okb.st(q, pk)
                oib.st(q, j)
        if rs > 0 and re < N:
            tags["path:others_both_sides"] += 1
            tags["path:junction_descent" if okb.ld(rs) < okb.ld(rs - 1) else "path:junction_no_descent"] += 1
        elif rs > 0:
            tags["path:others_before_only"] += 1
        elif re < N:
            tags["path:others_after_only"] += 1
        if kway:
            _kway(res, tags, mutant, okb, oib, no, rs)
            tags["kway:keys_in_3_runs_and_the_long_run"] = len(
                res.keys_in_3_runs & {run_keys.ld(r) for r in range(nrun)})
        elif no:
            # rocPRIM: stable, on the key bits [0, all_bits)
            low = (1 << all_bits) - 1
            order = sorted(range(no), key=lambda q: okb.ld(q) & low)
            for p, q in enumerate(order):
                okb.st(no + p, okb.ld(q))
                oib.st(no + p, oib.ld(q))
            tags["path:others_radix"] += 1
        else:
            tags["path:no_others"] += 1
        tags["path:rank_others_workgroups"] = (no + THREADS - 1) // THREADS
        for q in range(no):  # merge_rank_others_kernel
            k, i = okb.ld(no + q), oib.ld(no + q)
            lo, hi = 0, nrun
            while lo < hi:
                mid = (lo + hi) >> 1
                x = run_keys.ld(mid)
                if x < k or (x == k and rs + mid < i):
                    lo = mid + 1
                else:
                    hi = mid
            if 0 < lo < nrun and run_keys.ld(lo - 1) == k:
                tags["rank:other_after_equal_run_key"] += 1
            elif lo < nrun and run_keys.ld(lo) == k:
                tags["rank:other_before_equal_run_key"] += 1
            perm0.st_once(q + lo, i)
        for r in range(nrun):  # merge_rank_run_kernel
            k, i = run_keys.ld(r), rs + r
            lo, hi = 0, no
            while lo < hi:
                mid = (lo + hi) >> 1
                x = okb.ld(no + mid)
                if mutant == "rank_run_le":
                    before = x <= k
                else:
                    before = x < k or (x == k and oib.ld(no + mid) < i)
                if before:
                    lo = mid + 1
                else:
                    hi = mid
            perm0.st_once(r + lo, i)
        perm = [perm0.ld(j) for j in range(N)]
        fields = []
    # ---- the LSD radix passes ------------------------------------------------
    f0 = 0
    widths = []
    while f0 < len(fields):
        f1, bits = f0, 0
        while f1 < len(fields) and f1 - f0 < GROUP_FIELDS and bits + bin(fields[f1][1]).count("1") <= 64:
            bits += bin(fields[f1][1]).count("1")
            f1 += 1
        if f1 < len(fields):
            tags["group:cut_by_fields" if f1 - f0 == GROUP_FIELDS else "group:cut_by_bits"] += 1
        group = fields[f0:f1][::-1]
        k32 = bits <= 32
        kmask = 0xFFFFFFFF if k32 else M64
        kb = Buf("keys[0]", nn * (2 if k32 else 1))
        for j in range(N):  # merge_extract_kernel
            i = perm[j] if perm is not None and not (mutant == "pass_ignores_perm") else j
            kb.st(j, packed(i, group, kmask, -1 if mutant == "extract_shift" else 0))
        if perm is None:
            perm = list(range(N))  # merge_iota_kernel
        low = (1 << bits) - 1
        order = sorted(range(N), key=lambda j: kb.ld(j) & low)
        perm = [perm[j] for j in order]
        widths.append(32 if k32 else 64)
        tags["pass:%d" % widths[-1]] += 1
        tags["pass:fields=%d" % len(group)] += 1
        passes += 1
        f0 = f1
    if widths:
        tags["passes:" + ",".join(map(str, widths))] += 1
    if perm is None:
        perm = list(range(N))  # merge_iota_kernel alone
        tags["iota_only"] += 1
    if sorted(perm) != list(range(N)):
        raise Unsafe("perm is not a permutation of 0..N-1")
    res.perm = perm
    res.plan = (ORDER_PATH if width else ORDER_RADIX if passes else ORDER_IOTA, width, others, passes, D, rs, re,
                min(descents, 0xFFFFFFFF))
    return res


def _kway(res, tags, mutant, okb, oib, no, junction):
    """merge_kway_runs_kernel and merge_kway_rank_kernel: ok1 / oi1 are
    okb / oib from element `no` on."""
    # the starts list in w.sort_tmp: the count, then 2 * kKwayMaxRuns entries
    # (the host checks the buffer holds them)
    starts = []
    for j in range(1, no):
        if (mutant != "no_junction" and j == junction) or okb.ld(j) < okb.ld(j - 1):
            starts.append(j)
            if j == junction:
                tags["kway:junction_start"] += 1
    if len(starts) > KWAY_MAX_RUNS - 1:
        # the kernel keeps the first 11 in the order the atomics landed
        raise Unsafe("%d run starts: which 11 the rank kernel keeps is not determined" % len(starts))
    n = len(starts)
    sbv = [0] + sorted(starts) + [no]
    R = n + 1
    stride = max((no + KWAY_SAMPLES - 1) // KWAY_SAMPLES, 1)
    sbase = [0]
    for b in range(R):
        sbase.append(sbase[-1] + (sbv[b + 1] - sbv[b] + stride - 1) // stride)
    res.R = R
    tags["kway:R=%d" % R] += 1
    tags["kway:stride=%d" % stride] += 1
    tags["kway:workgroups"] = (no + KWAY_THREADS - 1) // KWAY_THREADS
    if any((sbv[b + 1] - sbv[b]) % stride == 0 for b in range(R)) and stride > 1:
        tags["kway:run_length_multiple_of_stride"] += 1
    if any(sbv[b + 1] - sbv[b] == 1 for b in range(R)):
        tags["kway:run_of_length_1"] += 1
    smp = Buf("smp", KWAY_SAMPLES + KWAY_MAX_RUNS)
    for b in range(R):
        for t in range(sbase[b + 1] - sbase[b]):
            smp.st(sbase[b] + t, okb.ld(sbv[b] + t * stride))
    in3 = Counter()
    for b in range(R):
        for k in {okb.ld(j) for j in range(sbv[b], sbv[b + 1])}:
            in3[k] += 1
    res.keys_in_3_runs = {k for k, c in in3.items() if c >= 3}
    for j in range(no):
        k = okb.ld(j)
        a = 0
        while a + 1 < R and sbv[a + 1] <= j:
            a += 1
        pos = j - sbv[a]
        for b in range(R):
            if b == a:
                continue
            l, h = sbase[b], sbase[b + 1]
            eq = False
            while l < h:
                mid = (l + h) >> 1
                x = smp.ld(mid)
                eq |= x == k
                if (x <= k) if b < a else (x < k):
                    l = mid + 1
                else:
                    h = mid
            t = l - sbase[b]
            end = sbv[b + 1]
            if t == 0:
                tags["kway:probe_below_every_sample"] += 1
            elif t == sbase[b + 1] - sbase[b]:
                tags["kway:probe_above_every_sample"] += 1
            if eq:
                tags["kway:probe_equals_a_sample"] += 1
            lo = sbv[b] if t == 0 else sbv[b] + (t - 1) * stride + 1
            top = sbv[b] + t * stride + (1 if mutant == "hi_plus_1" else -1 if mutant == "hi_minus_1" else 0)
            hi = top if top < end else end
            if sbv[b] + t * stride > end:
                tags["kway:interval_clipped_by_run_end"] += 1
            if lo < hi:
                tags["kway:interval_searched"] += 1
            while lo < hi:
                mid = (lo + hi) >> 1
                if mid >= no:
                    raise Unsafe("k-way search reads ok0[%d], %d others" % (mid, no))
                x = okb.ld(mid)
                if b < a:
                    before = x <= k
                else:
                    before = x <= k if mutant == "later_le" else x < k
                if before:
                    lo = mid + 1
                else:
                    hi = mid
            pos += lo - sbv[b]
        if not 0 <= pos < no:
            raise Unsafe("k-way rank %d of %d others" % (pos, no))
        okb.st_once(no + pos, k)
        oib.st(no + pos, oib.ld(j))


def stable_order(case):
    """Go string order, equal keys in input order."""
    return sorted(range(case.n), key=lambda i: case.pairs[i][0])


# ---- the cases ---------------------------------------------------------------
#
# A merge-path case is a list of sorted sequences laid end to end: some
# others-runs, the long run, more others-runs; every boundary is a descent (the
# builder counts them), so the input's descents are the sequences less one.
# The others-runs draw a third of their keys from a small pool they share and
# a third from the long run's keys (duplicates that straddle the sequences: run
# against others, others-run against others-run) and the rest from keys nobody
# else holds (stretches of distinct keys).  Values are the input index, the
# level is 1 (every first pair of a key is written) and the threshold gives a
# handful of files, so a stability error and a misplaced pair both change the
# written indices.

T_ORDER = 30_000


def k8(v):
    return struct.pack(">Q", v)


def k16(v):  # 32 varying bits in each of two chunks
    return struct.pack(">QQ", 0x4100000000000000 | v >> 32, 0x4200000000000000 | v & 0xFFFFFFFF)


def k16x40(v):  # 40 varying bits in each of two chunks
    return struct.pack(">QQ", v >> 40, v & ((1 << 40) - 1))


def k24x40(v):  # 40 varying bits in each of three chunks
    return struct.pack(">QQQ", v >> 80, (v >> 40) & ((1 << 40) - 1), v & ((1 << 40) - 1))


def k64(v):  # 64-byte keys: 3 varying bits in each of eight chunks
    return b"".join(struct.pack(">Q", 0x4141414141414140 | (v >> 3 * (7 - d)) & 7) for d in range(8))


def universe(rng, bits, count, enc=k8):
    """`count` distinct keys over `bits` varying bits, the all-zero and
    all-one values among them (so that exactly those bits vary), sorted."""
    vals = {0, (1 << bits) - 1}
    while len(vals) < count:
        vals.add(rng.getrandbits(bits))
    return sorted(enc(v) for v in vals)


def count_descents(keys):
    return sum(1 for i in range(1, len(keys)) if keys[i] < keys[i - 1])


def sequences(seed, univ, nrun, before, after, ranges=None, common=0, run_dups=0):
    """-> keys in input order.  before / after: the others-runs' lengths;
    ranges[r] = (f0, f1): others-run r draws from that fraction of the
    universe; common: the long run's middle key is put into that many
    others-runs; run_dups: equal neighbours inside the long run."""
    for attempt in range(200):
        rng = random.Random(seed * 1000 + attempt)
        inner = univ[1:-1]
        base = sorted(rng.sample(inner, nrun - 2 - run_dups) + [univ[0], univ[-1]])
        run = sorted(base + rng.sample(base, run_dups))
        runset = set(base)
        free = [k for k in inner if k not in runset]
        pool = rng.sample(inner, min(len(inner), 96))
        mid = base[len(base) // 2]
        seqs = []
        for r, L in enumerate(list(before) + list(after)):
            f0, f1 = (ranges or {}).get(r, (0.0, 1.0))
            kmin, kmax = inner[int(f0 * (len(inner) - 1))], inner[int(f1 * (len(inner) - 1))]
            ok = lambda k: kmin <= k <= kmax
            ks = set()
            if L == 1:
                ks.add(rng.choice([k for k in free if ok(k)][len(free) // 3: 2 * len(free) // 3] or free))
            else:
                if r < common:
                    ks.add(mid)
                cand = [k for k in pool if ok(k)]
                ks |= set(rng.sample(cand, min(len(cand), L // 3)))
                cand = [k for k in base[1:-1] if ok(k)]
                ks |= set(rng.sample(cand, min(len(cand), L // 3)))
                ks = set(sorted(ks)[:L])
                cand = [k for k in free if ok(k) and k not in ks]
                ks |= set(rng.sample(cand, L - len(ks)))
            assert len(ks) == L
            seqs.append(sorted(ks))
        keys = [k for s in seqs[:len(before)] for k in s] + run + [k for s in seqs[len(before):] for k in s]
        if count_descents(keys) == len(seqs):
            return keys
    raise AssertionError("no seed gives a descent at every boundary")


def runs_at(seed, univ, N, cuts, dups=0):
    """N keys in sorted runs that break exactly at the positions `cuts`."""
    rng = random.Random(seed)
    edges = [0] + sorted(cuts) + [N]
    keys, prev = [], None
    for a, b in zip(edges, edges[1:]):
        L = b - a
        assert L > 0
        for attempt in range(1000):
            room = univ[: min(len(univ) * 3 // 4, len(univ) - L)]  # L - 1 larger keys remain
            first = rng.choice(room[4:] if prev is None else [k for k in room if k < prev])
            rest = rng.sample([k for k in univ if k > first], L - 1 - min(dups, L - 1)) if L > 1 else []
            s = sorted([first] + rest)
            s = sorted(s + rng.sample(s, min(dups, L - 1)))
            if len(s) == L and s[-1] > univ[len(univ) // 8]:
                break
        else:
            raise AssertionError("run of %d after %r" % (L, prev))
        keys += s
        prev = s[-1]
    assert count_descents(keys) == len(cuts)
    return keys


def with_values(keys):
    return [(k, b"%d" % i) for i, k in enumerate(keys)]


# CLAIM[name] = (order kind, packed width, others, radix passes): what the
# case's name says the host chooses.
CLAIM = {}
# the cases that may exceed MAX_BYTES (1 MiB keys)
KEY_CAP_CASES = ("keycap_two_keys_1mib",)


def _build():
    cs = []

    def add(name, keys, claim, level=1, T=T_ORDER):
        cs.append(Case(name, with_values(keys), level, T))
        CLAIM[name] = claim

    PATH32K, PATH64K, PATH32R = (2, 32, 1, 0), (2, 64, 1, 0), (2, 32, 2, 0)
    u20 = universe(random.Random(1), 20, 12_000)

    # plan boundaries
    k4096 = sequences(1, u20, 3000, [300, 200], [596])
    add("n4095_radix", k4096[:-1], (1, 0, 0, 1))
    add("n4096_path", k4096, PATH32K)
    add("no_half_path", sequences(2, u20, 2048, [700, 648], [700]), PATH32K)
    add("no_half_plus1_radix", sequences(2, u20, 2047, [700, 649], [700]), (1, 0, 0, 1))
    add("bits32_path32", sequences(3, universe(random.Random(3), 32, 9000), 3000, [400, 296], [400]), PATH32K)
    add("bits33_path64", sequences(4, universe(random.Random(4), 33, 9000), 3000, [400, 296], [400]), PATH64K)
    u64 = universe(random.Random(5), 64, 9000)
    assert u64[0] == bytes(8) and u64[-1] == b"\xff" * 8
    add("bits64_one_field_path64", sequences(5, u64, 3000, [400, 296], [400]), PATH64K)
    # a varying length bit on top: 8- and 9-byte keys, the ninth byte zero
    u65 = sorted(k + b"\0" if i % 3 == 1 else k for i, k in enumerate(u64))
    add("bits65_len_bit_pass32_then_pass64", sequences(6, u65, 3000, [400, 296], [400]), (1, 0, 0, 2))
    add("bits64_two_fields_path64", sequences(7, universe(random.Random(7), 64, 9000, k16), 3000, [400, 296], [400]),
        PATH64K)
    u8f = universe(random.Random(8), 24, 9000, k64)
    add("fields8_long_keys_path32", sequences(8, u8f, 3000, [400, 296], [400]), PATH32K)
    u9f = sorted({k[:56] if i % 4 == 2 else k for i, k in enumerate(u8f)})
    assert u9f[0] == u8f[0] and u9f[-1] == u8f[-1]
    add("fields9_long_keys_cut_by_fields", sequences(9, u9f, 3000, [400, 296], [400]), (1, 0, 0, 2))
    rng = random.Random(10)
    u80 = universe(rng, 80, 900, k16x40)
    add("groups_2x40_bits_cut_by_bits", [rng.choice(u80) for _ in range(1500)], (1, 0, 0, 2))
    u120 = universe(rng, 120, 900, k24x40)
    add("three_passes", [rng.choice(u120) for _ in range(1500)], (1, 0, 0, 3))

    # no or trivial fields
    add("all_keys_equal", [b"same-key"] * 300, (0, 0, 0, 0))
    add("all_keys_empty", [b""] * 300, (0, 0, 0, 0))
    add("only_length_varies", [bytes(rng.choice(range(41))) for _ in range(498)] + [bytes(0), bytes(40)], (1, 0, 0, 1))
    longer = [b"a" + bytes(8) + b"b%03d" % rng.randrange(200) for _ in range(300)]
    mix = longer + [b"a", b"a\0", b"a\0\0"] * 20
    rng.shuffle(mix)
    add("a_a0_a00_among_longer", mix, (1, 0, 0, 1))

    # stats and run detection: 1,000 pairs are 4 tiles of 250, 3,000 are 12
    u = universe(random.Random(11), 20, 3000)
    add("descent_at_tile_first", runs_at(12, u, 1000, [250, 620]), (1, 0, 0, 1))
    add("descent_at_tile_last", runs_at(13, u, 1000, [499, 620]), (1, 0, 0, 1))
    add("descent_at_wave_lane0", runs_at(14, u, 1000, [314, 620]), (1, 0, 0, 1))
    add("run_spans_ten_tiles_equal_neighbours", runs_at(15, u, 3000, [100, 2600], dups=40), (1, 0, 0, 1))
    add("run_starts_at_0", runs_at(16, u, 1000, [600, 700, 900]), (1, 0, 0, 1))
    add("run_ends_at_N", runs_at(17, u, 1000, [100, 200, 400]), (1, 0, 0, 1))
    add("two_equal_runs_first_wins", runs_at(18, u, 1000, [500]), (1, 0, 0, 1))
    add("tiles_with_1_64_65_descents",
        runs_at(19, u, 1000, [100] + [252 + 3 * k for k in range(64)] + [501 + 3 * k for k in range(65)]),
        (1, 0, 0, 1))
    fives = [c for c in range(5, 1000, 5) if not 250 <= c < 500]
    add("inner_run_is_the_longest", runs_at(20, u, 1000, fives + [260, 480]), (1, 0, 0, 1))
    fifties = [c for c in range(50, 1000, 50) if not 250 <= c < 500]
    add("inner_run_skipped_at_65_descents",
        runs_at(21, u, 1000, fifties + [251, 252, 253, 254, 260, 380] + list(range(382, 500, 2))), (1, 0, 0, 1))
    # the descent compare: equal 32-byte prefixes with both lengths <= 32 (the
    # keys differ in trailing zero bytes, or not at all), one length 33, and
    # a difference only past byte 32
    P = b"p" * 30
    Q = b"q" * 32
    special = [P, P + b"\0", P + b"\0\0", Q, Q + b"\0", Q + b"\1", Q + b"AAAAAAAB", Q + b"AAAAAAAC",
               Q + b"AAAAAAAB\0"]
    add("descent_compare_branches", [rng.choice(special) for _ in range(400)], (1, 0, 0, 1))

    # the merge path
    add("path_no_others", sequences(30, u20, 4096, [], [], run_dups=200), (2, 32, 0, 0))
    add("path_others_before_only", sequences(31, u20, 3000, [500, 596], []), PATH32K)
    add("path_others_after_only", sequences(32, u20, 3000, [], [500, 596]), PATH32K)
    add("path_junction_descent", sequences(33, u20, 3000, [548], [548], ranges={0: (0.5, 1.0), 1: (0.0, 0.5)}),
        PATH32K)
    add("path_junction_no_descent", sequences(34, u20, 3000, [548], [548], ranges={0: (0.0, 0.5), 1: (0.5, 1.0)}),
        PATH32K)
    add("path_others_run_of_length_1", sequences(35, u20, 3000, [1, 500], [594, 1]), PATH32K)
    add("path_descents_10_kway", sequences(36, u20, 3000, [110] * 5, [110, 110, 110, 110, 106]), PATH32K)
    add("path_descents_11_radix_others", sequences(37, u20, 3000, [100] * 6, [100, 100, 100, 100, 96]), PATH32R)
    add("path_no_1024", sequences(38, u20, 3072, [512], [512]), PATH32K)
    add("path_no_1025", sequences(38, u20, 3072, [512], [513]), PATH32K)
    u20b = universe(random.Random(2), 20, 45_000)
    add("path_no_4096_stride_1", sequences(39, u20b, 4204, [1365, 1366], [1365], common=3), PATH32K)
    add("path_no_4097_stride_2", sequences(40, u20b, 4204, [1367, 1365], [1365], common=3), PATH32K)
    add("path_no_8200_stride_3", sequences(41, u20b, 8300, [2734, 2735], [2731], common=3), PATH32K)

    # the key cap: D = 131,072 chunks, one varying byte in the last
    big = bytes(range(256)) * 4096
    assert len(big) == KEY_CAP
    add("keycap_two_keys_1mib", [big[:-1] + b"\x02", big[:-1] + b"\x01"], (1, 0, 0, 1))
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
# one pair whose key is 9 bytes past the cap: LSM_EINVAL, nothing written
KEY_PAST_CAP = Case("keycap_plus_9_einval", [(bytes(KEY_CAP + 9), b"v")], 1, T_ORDER)
# four calls on one workspace, alternating (tests/test_merge_order_gpu.py)
BACK_TO_BACK = ("n4096_path", "three_passes")

# ---- the mutants -------------------------------------------------------------
#
# One-line, value-only changes of steps 1-2, each mirrored in census(case,
# mutant).  A mutant is cleared for a GPU run only if the model keeps every
# load and store in the device's buffers and perm a permutation in every case.
#  path_min_4097      kMergePathMin = 4097
#  no_junction        merge_kway_runs_kernel without `j == junction ||`
#  hi_plus_1          the k-way rank's hi[b] = min(sb[b] + t * stride + 1, end)
#  hi_minus_1         ... = min(sb[b] + t * stride - 1, end)
#  later_le           the interval search's later-run side: x[b] <= k for x[b] < k
#  rank_run_le        merge_rank_run_kernel: `x <= k` for `x < k || (x == k && oi[mid] < i)`
#  pass_ignores_perm  merge_extract_kernel: i = j, not perm[j]
#  extract_shift      merge_extract_kernel: key << (bits - 1)
#  stitch_ge          the host's run(): b - a >= run_e - run_s
#  width_lt_32        merge_kvs: all_bits < 32 picks the 32-bit merge path
#  kway_bound_13      merge_path: descents + 2 <= kKwayMaxRuns + 1
# MUTANT_UNSAFE[m]: the cases in which the model raises Unsafe; a mutant with
# any is not run on a GPU.  MUTANT_RED[m]: the cases a cleared mutant must turn
# red (a wrong output or a wrong plan word); every other case stays green.
# MUTANT_GPU_RED[m]: the cases that failed when the mutant ran on an MI355X,
# once, through tests/test_merge_order_gpu.py::test_case.
_PATH_AT_4096 = {"n4096_path", "no_half_path", "bits32_path32", "bits33_path64", "bits64_one_field_path64",
                 "bits64_two_fields_path64", "fields8_long_keys_path32", "path_no_others",
                 "path_others_before_only", "path_others_after_only", "path_junction_descent",
                 "path_junction_no_descent", "path_others_run_of_length_1", "path_descents_10_kway",
                 "path_descents_11_radix_others", "path_no_1024"}
_KWAY_CASES = {"n4096_path", "no_half_path", "bits32_path32", "bits33_path64", "bits64_one_field_path64",
               "bits64_two_fields_path64", "fields8_long_keys_path32", "path_others_before_only",
               "path_others_after_only", "path_junction_descent", "path_junction_no_descent",
               "path_others_run_of_length_1", "path_descents_10_kway", "path_no_1024", "path_no_1025",
               "path_no_4096_stride_1", "path_no_4097_stride_2", "path_no_8200_stride_3"}
# A wrong rank on the merge path never gives a wrong permutation: two pairs
# land on one slot and another slot keeps a stale word, which steps 3-5 would
# use as an input index.  So hi_minus_1, later_le and rank_run_le are not
# cleared.  later_le and hi_minus_1 touch only the interval search, which runs
# when stride > 1.  rank_run_le is harmless only where no run key equals a key
# of the others, or every such other comes first in the input.
MUTANT_UNSAFE = {
    "hi_minus_1": {"path_no_4097_stride_2", "path_no_8200_stride_3"},
    "later_le": {"path_no_4097_stride_2", "path_no_8200_stride_3"},
    "rank_run_le": (_KWAY_CASES | {"path_descents_11_radix_others"}) - {"path_others_before_only"},
}
# no_junction and hi_plus_1 change nothing anywhere.  Without the junction
# start, the pairs before and after the long run form one others-run exactly
# when they ascend across the junction, and then they are one sorted run.  An
# interval that also holds sample t finds the same bound, because sample t is
# already known not to be before the probe.
MUTANT_RED = {
    "path_min_4097": _PATH_AT_4096,                       # the plan only: radix passes give the same order
    "no_junction": set(),
    "hi_plus_1": set(),
    "pass_ignores_perm": {"bits65_len_bit_pass32_then_pass64", "fields9_long_keys_cut_by_fields",
                          "groups_2x40_bits_cut_by_bits", "three_passes"},         # the output
    "extract_shift": {"fields9_long_keys_cut_by_fields", "a_a0_a00_among_longer",
                      "descent_compare_branches"},                                  # the output
    "stitch_ge": {"three_passes", "two_equal_runs_first_wins", "descent_compare_branches",
                  "keycap_two_keys_1mib"},                                          # run_s, run_e
    "width_lt_32": {"bits32_path32"},                                               # the width
    "kway_bound_13": {"path_descents_11_radix_others"},                             # others: k-way, R = 11
    "hi_minus_1": set(), "later_le": set(), "rank_run_le": set(),                   # in the cases they are safe in
}
CLEARED = tuple(m for m in MUTANTS if not MUTANT_UNSAFE.get(m))
MUTANT_GPU_RED = {
    "path_min_4097": _PATH_AT_4096,
    "no_junction": set(),
    "hi_plus_1": set(),
    "pass_ignores_perm": {"bits65_len_bit_pass32_then_pass64", "fields9_long_keys_cut_by_fields",
                          "groups_2x40_bits_cut_by_bits", "three_passes"},
    "extract_shift": {"a_a0_a00_among_longer", "descent_compare_branches", "fields9_long_keys_cut_by_fields"},
    "stitch_ge": {"descent_compare_branches", "keycap_two_keys_1mib", "three_passes", "two_equal_runs_first_wins"},
    "width_lt_32": {"bits32_path32"},
    "kway_bound_13": {"path_descents_11_radix_others"},
}  # each red case was red in both tie orders and both layouts


def output_of(case, perm):
    """What steps 3-5 write when handed `perm` as the sorted order (merge.go's
    loop; the cases here hold no tombstones) -> (written indices, file starts).
    Used only to say whether a mutant's order changes the output."""
    out, starts, last, size = [], [0], None, 0
    for i in perm:
        k, v = case.pairs[i]
        assert v != wc.TOMB
        if k and k == last:
            continue
        out.append(i)
        last = k
        size += 16 + len(k) + len(v)
        if size >= case.threshold:
            starts.append(len(out))
            last, size = None, 0
    if starts[-1] != len(out):
        starts.append(len(out))
    return out, starts


def agrees(r, case, reference_plan):
    """Would a device computing what Census r models pass the GPU test?"""
    return r.plan == reference_plan and output_of(case, r.perm) == output_of(case, stable_order(case))
