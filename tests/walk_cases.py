"""Small adversarial inputs for steps 3-5 of lsm_merge_kvs (groups and
candidates, the sums and the file walk, the emit), and a census of the paths
they reach.  Plain numpy and the CPU oracle: no torch, no GPU.

A file's end can be found three ways in go-lsm_amd/csrc/merge.hip: the
one-shot prediction (merge_walk_abs_kernel's maps, chained by phase 1 of
merge_walk_kernel), the rounds, and the general step.  Hand-offs between them
are single bytes.  A Case is a named list of (key, value) pairs in input order
with a level and a threshold; the expected output comes only from
pyoracle.merge_kvs.

census() restates, for TIE_INPUT, what merge_flags_kernel,
merge_candidate_kernel, merge_scan_apply, merge_walk_abs_kernel,
merge_walk_kernel and merge_emit_kernel do, over the stable-sorted pairs in
plain Python integers and doubles.  It exists so that tests can prove the case
list reaches what it claims to reach: which path wrote each file, and every
hand-off code met.  Its own file starts and written indices must equal the
oracle's (tests/test_walk_cases.py), or the census is wrong; it never produces
expected output.

census(case, mutant="a".."j") applies one of ten value-only changes to the
model and checks every modelled load and store against the device's buffer
sizes (Unsafe otherwise).  The mutants are the ones applied to a scratch copy
of merge.hip to prove the GPU tests bite; the model says which cases each must
turn red and that its stores stay in bounds there.
"""
import random
from collections import Counter

import numpy as np

import pyoracle as ora

TOMB = "～DELETED～".encode()  # kv.DeletedValue, 13 bytes
MAX_PAIRS = 20_000

# merge.hip / scan.h
SCAN_TILE = 512        # kScanTile
SCAN_PER = 2           # kScanPer: positions per thread of merge_scan_apply
EXT_SCAN = 254         # kExtScan
EMIT_BLOCK = 256       # kMergeThreads
WALK_THREADS = 1024    # kWalkThreads
WALK_ENTRIES = 4096    # kWalkEntries
WALK_MAX_R = 32        # kWalkMaxR
WAVE = 64
ABS_W = 248            # kAbsW
ABS_MAX_WIN = 352      # kAbsMaxWin
ABS_LAST, ABS_STOP, ABS_GENERAL, ABS_MISS = 252, 253, 254, 255
SUCC_MISS, SUCC_GENERAL, SUCC_STOP, SUCC_LAST = 0xFFFF, 0xFFFE, 0xFFFD, 0xFFFC
INF = (1 << 64) - 1
M64 = (1 << 64) - 1
ABS_NAME = {ABS_LAST: "kAbsLast", ABS_STOP: "kAbsStop", ABS_GENERAL: "kAbsGeneral", ABS_MISS: "kAbsMiss"}
SUCC_NAME = {SUCC_MISS: "kSuccMiss", SUCC_GENERAL: "kSuccGeneral", SUCC_STOP: "kSuccStop",
             SUCC_LAST: "kSuccLast"}
MARGIN = 1e-6
MUTANTS = "abcdefghij"


class Unsafe(Exception):
    """A modelled load or store outside the device's buffers, or a walk that
    does not end: such a mutant is not run on a GPU."""


class Case:
    def __init__(self, name, pairs, level, threshold):
        assert 0 < len(pairs) <= MAX_PAIRS and threshold > 0
        self.name, self.pairs, self.level, self.threshold = name, pairs, level, threshold

    @property
    def n(self):
        return len(self.pairs)

    def nbytes(self):
        return sum(len(k) + len(v) for k, v in self.pairs)

    def __repr__(self):
        return "Case(%s, n=%d, level=%d, T=%d)" % (self.name, self.n, self.level, self.threshold)


def lay_out(pairs, kv_layout, seed=0):
    """The pairs as descriptors over one byte buffer, stored in shuffled
    order (test_merge_gpu.lay_out's conventions).  kv_layout: KV records
    [klen][key][vlen][value], value descriptors None; else keys and values
    apart, each after 4 bytes of padding (bytes at rec_off + 4).
    -> (buf, key desc, value desc or None, kpos, vpos)."""
    rng = random.Random(seed)
    n = len(pairs)
    place = list(range(n))
    rng.shuffle(place)
    parts, pos = [], 0
    kpos, vpos = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    kd = np.zeros(n, ora.DESC_DTYPE)
    vd = np.zeros(n, ora.DESC_DTYPE)
    for i in place:
        k, v = pairs[i]
        gap = rng.randint(0, 3)
        parts.append(bytes(gap))
        pos += gap
        if kv_layout:
            kd[i] = (pos, len(k), len(v))
            kpos[i], vpos[i] = pos + 4, pos + 8 + len(k)
            parts += [len(k).to_bytes(4, "little"), k, len(v).to_bytes(4, "little"), v]
            pos += 8 + len(k) + len(v)
        else:
            kd[i] = (pos, len(k), 0)
            kpos[i] = pos + 4
            parts += [b"\xAA" * 4, k]
            pos += 4 + len(k)
            vd[i] = (pos, 0, len(v))
            vpos[i] = pos + 4
            parts += [b"\xBB" * 4, v]
            pos += 4 + len(v)
    parts.append(bytes(16))
    buf = np.frombuffer(b"".join(parts), np.uint8)
    return buf, kd, (None if kv_layout else vd), kpos, vpos


def expected(case, tie):
    """CompactAndMergeKVs by the oracle -> (written input indices, file starts)."""
    return ora.merge_pairs(case.pairs, case.level, case.threshold, tie)


# ---- the census -------------------------------------------------------------


def _walk_file(P, Q, X, first, n, T, tail_s, mutant):
    """walk_file -> (code, p, wpos, wperm, tg); Q = (position, continues),
    X = (perm value, delta, size)."""
    wpos, wperm, wsize, p, tg = None, 0, 0, 0, INF
    if not first:
        p = Q[0] + 1
        if p >= n:
            return SUCC_STOP, p, wpos, wperm, tg
        if Q[1]:
            if X is None:
                raise Unsafe("cand_ext of a candidate that continues no group")
            d = X[1]
            if d == 0xFF:
                return SUCC_GENERAL, p, wpos, wperm, tg
            if d:
                wpos, wperm, wsize = Q[0] + d, X[0], X[2]
                if (wsize > T) if mutant == "c" else (wsize >= T):
                    return SUCC_GENERAL, p, wpos, wperm, tg
    tg = (P + T - wsize) & M64
    return (SUCC_LAST if tail_s < tg else 0), p, wpos, wperm, tg


class Census:
    """What census() returns.
    paths[f]: "abs", "round(R)" or "general(reason)" for file f;
    codes: Counter of the hand-off codes met (phase 1's head and chain, the
    rounds' chain ends, cand_ext's delta classes at the plateaus used);
    counts: derived numbers the coverage test asserts;
    out, starts: the written input indices and file starts as modelled;
    most: counts[2]; margin: the least distance of a truncated floating-point
    quantity from an integer boundary."""


def census(case, mutant=None):
    assert mutant is None or mutant in MUTANTS
    pairs, level, T = case.pairs, case.level, case.threshold
    n = len(pairs)
    perm = sorted(range(n), key=lambda i: pairs[i][0])  # stable: equal keys in input order
    key = [pairs[i][0] for i in perm]
    val = [pairs[i][1] for i in perm]
    res = Census()
    codes, cnt = Counter(), Counter()
    res.codes, res.counts = codes, cnt
    margin = [1.0]

    # merge_flags_kernel, merge_candidate_kernel
    gs = [j == 0 or len(key[j]) == 0 or key[j] != key[j - 1] for j in range(n)]
    wr = [level < 6 or val[j] != TOMB for j in range(n)]
    size = [16 + len(key[j]) + len(val[j]) for j in range(n)]
    csize = [0] * n
    for j in range(n):
        c = wr[j]
        if c and not gs[j]:
            k = j
            while k > 0:
                k -= 1
                if wr[k]:
                    c = False
                    break
                if gs[k]:
                    break
        if c:
            csize[j] = size[j]
    cnt["groups"] = sum(gs)
    cnt["candidates"] = sum(1 for x in csize if x)
    cnt["empty_key_candidates"] = sum(1 for j in range(n) if csize[j] and not key[j])

    # merge_scan_tiles / merge_scan_apply: the sums and the plateau arrays
    S, C = [0] * (n + 1), [0] * (n + 1)
    for j in range(n):
        S[j + 1], C[j + 1] = S[j] + csize[j], C[j] + (csize[j] != 0)
    tail_s, tail_c = S[n], C[n]
    ncand = tail_c
    cand_pn, cand_pos, cand_ext = [], [], []
    for k in range(n):
        if not csize[k]:
            continue
        cont = k + 1 < n and not gs[k + 1]
        cand_pn.append(S[k] + csize[k])
        cand_pos.append((k, cont))
        X = None
        if cont:
            X = (0, 0xFF, 0)
            if wr[k + 1]:
                if size[k + 1] < 0xFFFFFF:
                    X = (perm[k + 1], 1, size[k + 1])
            else:
                for d in range(2, EXT_SCAN + 1):
                    q = k + d
                    if q >= n or gs[q]:
                        X = (0, 0, 0)
                        break
                    if wr[q]:
                        if size[q] < (1 << 24):
                            X = (perm[q], d, size[q])
                        break
            if mutant == "d" and X[1] == 0xFF:
                X = (0, 0, 0)
        cand_ext.append(X)

    def ld(e):  # plateau e's (P, Q, X): cand_*[e - 1]
        if not 1 <= e <= n:
            raise Unsafe("plateau %d outside the arrays" % e)
        if e > ncand:
            raise Unsafe("plateau %d past the last candidate (stale words)" % e)
        return cand_pn[e - 1], cand_pos[e - 1], cand_ext[e - 1]

    def wf(P, Q, X, first):
        return _walk_file(P, Q, X, first, n, T, tail_s, mutant)

    def note_ext(e):
        """The cand_ext class of plateau e, used as a file's start."""
        k, cont = cand_pos[e - 1]
        if not cont:
            return
        d = cand_ext[e - 1][1]
        codes["ext:" + ("0" if d == 0 else "255" if d == 0xFF else str(d))] += 1
        if d == 0xFF and k + 1 < n and wr[k + 1]:
            codes["ext:255:2^24"] += 1
        if k % SCAN_TILE == SCAN_TILE - 1:
            cnt["ext_tile_last"] += 1
        if k % SCAN_PER == SCAN_PER - 1:
            cnt["ext_other_thread"] += 1
        if d and d != 0xFF:
            sz = cand_ext[e - 1][2]
            codes["extra:" + ("T-1" if sz == T - 1 else "T" if sz == T else "T+1" if sz == T + 1 else
                              "<T" if sz < T else ">T")] += 1

    # device buffers: files[n + 2], out[n + 64] in the tests' own buffers
    files, out, paths = {}, {}, {}

    def st_file(f, p, extra, o, path=None):
        if not 0 <= f < n + 2:
            raise Unsafe("files[%d]" % f)
        files[f] = (p, extra, o)
        if path:
            paths[f] = path

    def st_out(o, v):
        if not 0 <= o < n + 64:
            raise Unsafe("out[%d]" % o)
        out[o] = v

    # merge_walk_abs_kernel
    def abs_base(f):
        span = (float(T) + 0.5 * float(tail_s) / float(tail_c)) * float(tail_c) / float(tail_s)
        x = float(f + 1) * span + 0.5
        margin[0] = min(margin[0], abs(x - round(x)))
        c = int(x)
        return c - ABS_W // 2 if c > 1 + ABS_W // 2 else 1

    nwin = 0 if tail_c == 0 else min(tail_s // T + 2, ABS_MAX_WIN)
    cnt["abs_windows"] = nwin
    bases = [(abs_base(f), abs_base(f + 1)) for f in range(nwin)]
    if nwin and abs_base(0) == 1 and (float(T) + 0.5 * tail_s / tail_c) * tail_c / tail_s < 1.0:
        cnt["abs_span_below_1"] = 1
        cnt["abs_b0_eq_b1"] = sum(1 for b0, b1 in bases if b0 == b1)

    def abs_succ(f, t):
        """succ[f][t]: plateau bases[f][0] + t as the end of file f -> file
        f + 1's end in window f + 1."""
        b0, b1 = bases[f]
        e = b0 + t
        if e > ncand:
            return ABS_MISS
        P, Q, X = ld(e)
        c, _, _, _, tg = wf(P, Q, X, False)
        if c == SUCC_LAST:
            return ABS_LAST
        if c == SUCC_STOP:
            return ABS_STOP
        if c == SUCC_GENERAL:
            return ABS_GENERAL
        npv = [cand_pn[b1 + i - 1] if b1 + i <= ncand else INF for i in range(ABS_W)]
        pos, s = 0, 128
        while s:
            if pos + s <= ABS_W and npv[pos + s - 1] < tg:
                pos += s
            s >>= 1
        if pos < ABS_W and (pos > 0 or b1 <= e + 1 or mutant == "a"):
            if pos == 0:
                cnt["abs_pos0_accepted"] += 1
            return pos
        cnt["abs_pos0_rejected" if pos == 0 else "abs_past_window"] += 1
        return ABS_MISS

    head1 = None
    if nwin:
        if tail_s < T:
            head1 = ABS_LAST
        else:
            b0 = bases[0][0]
            x = next((t for t in range(ABS_W) if (cand_pn[b0 + t - 1] if b0 + t <= ncand else INF) >= T), ABS_W)
            head1 = x if (x < ABS_W and (x > 0 or b0 <= 1)) else ABS_MISS

    # merge_walk_kernel
    est = float(T) * float(tail_c) / float(tail_s) if tail_s else 0.0
    if 1.0 <= est <= float(ncand):
        margin[0] = min(margin[0], abs(est - round(est)))
    span0 = 1 if est < 1.0 else ncand if est > float(ncand) else int(est)
    st = dict(p=0, e=0, nf=0, span=span0, R=WALK_MAX_R, stop=0, o=0, most=0, P=0)

    if nwin > 0:  # phase 1
        chosen, x, f = [], head1, 0
        codes["head:" + ABS_NAME.get(head1, "hit")] += 1
        while x < ABS_W:
            chosen.append(x)
            f += 1
            if f == nwin or bases[f - 1][1] != bases[f][0]:
                cnt["abs_window_limit"] += f == ABS_MAX_WIN
                x = ABS_MISS
                codes["abs:end of windows"] += 1
                break
            x = abs_succ(f - 1, x)
            if x >= ABS_LAST:
                codes["abs:" + ABS_NAME[x]] += 1
        nres, code = f, x
        cnt["abs_nres"] = nres
        if nres > WALK_THREADS:
            raise Unsafe("nres")
        nws, starts_ = [], []
        for t in range(nres + 1):
            es, Ps, pf, wposf, wpermf = 0, 0, 0, None, 0
            if t > 0:
                es = bases[t - 1][0] + chosen[t - 1]
                Ps, Q, X = ld(es)
                _, pf, wposf, wpermf, _ = wf(Ps, Q, X, False)
                note_ext(es)
            nw = 0
            if t < nres:
                nw = (wposf is not None) + (bases[t][0] + chosen[t] - es)
            elif code == ABS_LAST:
                nw = (wposf is not None) + (tail_c - es)
                if nw == 0:
                    cnt["abs_last_nothing"] += 1
            if nw < 0:
                raise Unsafe("a file of %d pairs" % nw)
            nws.append(nw)
            starts_.append((es, Ps, pf, wposf, wpermf))
        waves = [nws[w:w + WAVE] for w in range(0, len(nws), WAVE)]
        most = max(max(w) for w in (waves[:1] if mutant == "j" else waves))
        cnt["abs_waves"] = len(waves)
        if len(waves) > 1 and max(waves[0]) < max(nws):
            cnt["abs_most_past_wave0"] = 1
        o, tot = 0, sum(nws)
        for t, nw in enumerate(nws):
            es, Ps, pf, wposf, wpermf = starts_[t]
            ot = o - (sum(sum(w) for w in waves[:t // WAVE]) if mutant == "g" else 0)
            if nw:
                st_file(t, pf, wposf, ot, "abs")
                if wposf is not None:
                    st_out(ot, wpermf)
            o += nw
        if nres > 0:
            es, Ps, pf, wposf, wpermf = starts_[nres]
            st.update(p=pf, e=es, P=Ps, nf=nres + (1 if nws[nres] else 0), o=tot, most=most,
                      span=max((es + nres // 2) // nres, 1),
                      stop=1 if code in (ABS_LAST, ABS_STOP) else 2 if code == ABS_GENERAL else 0)
            if st["stop"] == 2:
                st["why"] = "unresolved" if cand_ext[es - 1][1] == 0xFF else "extra>=T"
            if pf >= n:
                st["stop"] = 1
            if st["stop"] == 0:
                cnt["abs_to_rounds_nres>0"] = 1
                cnt["abs_to_rounds_span"] = st["span"]
        elif code == ABS_LAST:
            st.update(nf=1 if nws[0] else 0, o=tot, most=most, stop=1)

    passes = 0
    while True:
        S0 = dict(st)
        if S0["stop"] == 1 or S0["nf"] > n:
            if S0["stop"] != 1:
                cnt["failsafe"] += 1
            break
        passes += 1
        if passes > 4 * n + 8:
            raise Unsafe("the walk does not end")
        why = S0.pop("why", None)
        st.pop("why", None)
        if S0["stop"] == 0 and S0["p"] != 0 and S0["e"] == 0:
            S0["stop"], why = 2, "no-plateau"
        if S0["stop"] == 0:
            R = S0["R"]
            W = WALK_ENTRIES // R
            e0, span = S0["e"], S0["span"]

            def base(r):
                c = e0 + (r + 1) * span
                return c - W // 2 if c > e0 + 1 + W // 2 else e0 + 1

            def win(x):  # the LDS window arrays
                r = x // W
                e = base(r) + (x - r * W)
                if e <= ncand:
                    return ld(e)
                return INF, (0, False), (0, 0, 0)

            def succ(x):
                r = x // W
                e = base(r) + (x - r * W)
                if not (r + 1 < R and e <= ncand):
                    return SUCC_MISS
                P, Q, X = win(x)
                c, _, _, _, tg = wf(P, Q, X, False)
                if c:
                    return c
                b1, pos, s = (r + 1) * W, 0, W // 2
                while s:
                    if win(b1 + pos + s - 1)[0] < tg:
                        pos += s
                    s >>= 1
                lo = pos + (1 if win(b1 + pos)[0] < tg else 0)
                ok = lo < W and (lo > 0 or base(r + 1) <= e + 1 or mutant == "b")
                if lo == 0:
                    cnt["round_lo0_accepted" if base(r + 1) <= e + 1 else "round_lo0_rejected"] += 1
                return lo if ok else SUCC_MISS

            Qs, Xs = (0, False), (0, 0, 0)
            if S0["p"]:
                _, Qs, Xs = ld(e0)
            code, p, _, _, tg = wf(S0["P"], Qs, Xs, S0["p"] == 0)
            if p != S0["p"] and mutant != "f":
                code = SUCC_GENERAL
                why = "not a plateau start"
            elif code == SUCC_GENERAL:
                why = "unresolved" if Xs[1] == 0xFF else "extra>=T"
            if code == 0:
                code = SUCC_MISS
                for x in range(W):
                    if win(x)[0] >= tg:
                        if x > 0 or base(0) <= e0 + 1:
                            code = x
                        break
            nres, my_x = 0, []
            while code < SUCC_LAST:
                my_x.append(code)
                nres += 1
                if nres == R:
                    break
                code = succ((nres - 1) * W + code)
            if nres < R:
                codes["succ:" + SUCC_NAME[code]] += 1
            else:
                cnt["round_all_resolved_R%d" % R] += 1
            lanes = []
            for lane in range(nres + 1):
                Ps, es, Qr, Xr = S0["P"], e0, Qs, Xs
                if lane > 0:
                    Ps, Qr, Xr = win((lane - 1) * W + my_x[lane - 1])
                    es = base(lane - 1) + my_x[lane - 1]
                    if es > ncand:
                        raise Unsafe("a file ends past the last plateau")
                    note_ext(es)
                _, pr, wposr, wpermr, _ = wf(Ps, Qr, Xr, lane == 0 and S0["p"] == 0)
                if lane == 0:
                    pr = S0["p"]
                nw = 0
                if lane < nres:
                    nw = (wposr is not None) + (base(lane) + my_x[lane] - es)
                elif nres < R and code == SUCC_LAST:
                    nw = (wposr is not None) + (tail_c - es)
                if nw < 0:
                    raise Unsafe("a file of %d pairs" % nw)
                lanes.append((pr, wposr, wpermr, nw, es, Ps))
            ox, most, nfn = S0["o"], S0["most"], S0["nf"]
            for lane, (pr, wposr, wpermr, nw, es, Ps) in enumerate(lanes):
                most = max(most, nw)
                if nw:
                    st_file(S0["nf"] + lane, pr, wposr, ox, "round(%d)" % R)
                    if wposr is not None:
                        st_out(ox, wpermr)
                    nfn += 1
                ox += nw
            np_, _, _, _, ne, nP = lanes[nres]
            stop, Rn = 0, R
            if nres == R:
                Rn = 2 * R if R < WALK_MAX_R else R
                if R < WALK_MAX_R:
                    cnt["round_doubling"] += 1
                stop = 1 if np_ >= n else 0
            elif code in (SUCC_STOP, SUCC_LAST):
                stop = 1
            elif code == SUCC_GENERAL:
                stop = 2
            else:
                Rn = 1
                while 2 * Rn <= nres:
                    Rn *= 2
                stop = 2 if nres == 0 else 0
                if nres:
                    cnt["round_miss_nres>0"] += 1
                    cnt["round_miss_R%d_to_R%d" % (R, Rn)] += 1
                else:
                    cnt["round_miss_nres0"] += 1
                    why = "missed its window"
            nspan = S0["span"]
            if nres > 0 and ne > e0:
                nspan = (ne - e0 + nres // 2) // nres
            st = dict(p=np_, e=ne, nf=nfn, span=max(nspan, 1), R=Rn, stop=stop, o=ox, most=most, P=nP)
            if stop == 2:
                if code == SUCC_GENERAL and nres > 0:
                    why = "unresolved" if cand_ext[ne - 1][1] == 0xFF else "extra>=T"
                st["why"] = why
            continue
        # the general step
        p = S0["p"]
        starts = p == 0 or gs[p]
        g, w, wsize = p, None, 0
        if not starts:
            q0, chunk = p, 0
            while True:
                ends = [q for q in range(q0, q0 + WALK_THREADS) if q >= n or (q > p and gs[q])]
                ge = min(min(ends), n) if ends else None
                ws = [q for q in range(q0, min(q0 + WALK_THREADS, n))
                      if not (q > p and gs[q]) and (ge is None or q < ge) and wr[q]]
                if w is None and ws and (mutant != "e" or q0 == p):
                    w = min(ws)
                    cnt["general_w_chunk%d" % chunk] += 1
                if ge is not None:
                    g = ge
                    break
                q0 += WALK_THREADS
                chunk += 1
            cnt["general_group_chunks_%d" % (chunk + 1)] += 1
            cnt["general_group_len_%d" % (g - p)] += 1
            if w is None:
                cnt["general_w_absent"] += 1
            if g == n:
                cnt["general_group_to_n"] += 1
            if w is not None:
                wsize = size[w]
        Sg, Cg = S[g], C[g]
        end = n
        if w is not None and wsize >= T:
            end = w + 1
            cnt["general_extra_fills"] += 1
        else:
            tg = (Sg + (T - wsize)) & M64
            if tail_s >= tg:
                lo, hi, first = g + 1, n, True
                while hi > lo:
                    sp = hi - lo
                    step = (sp + WALK_THREADS - 2) // (WALK_THREADS - 1) if sp >= WALK_THREADS - 1 else 1
                    if first:
                        cnt["general_search_span_max"] = max(cnt["general_search_span_max"], sp)
                        cnt["general_search_span_min"] = min(cnt["general_search_span_min"] or sp, sp)
                        if sp < WALK_THREADS - 1:
                            cnt["general_search_short"] += 1
                        if step > 1:
                            cnt["general_search_strided"] += 1
                        first = False

                    def pos_of(t):
                        k = lo + t * step
                        return hi if (k > hi or t == WALK_THREADS - 1) else k

                    f = next(t for t in range(WALK_THREADS) if S[min(pos_of(t), n)] >= tg)
                    if f == 0:
                        hi = lo
                        break
                    kf = pos_of(f)
                    lo, hi = lo + (f - 1) * step + 1, kf
                end = lo
            else:
                cnt["general_writes_last"] += 1
        nw = (w is not None) + (C[end] - Cg if end > g else 0)
        if nw == 0 and mutant != "i":
            st = dict(S0, stop=1)
            cnt["general_nothing_left"] += 1
        else:
            if nw == 0:
                cnt["general_nothing_left"] += 1
            st_file(S0["nf"], p, w, S0["o"], "general(%s)" % why)
            codes["general:%s" % why] += 1
            if w is not None:
                st_out(S0["o"], perm[w])
            st = dict(S0, o=S0["o"] + nw, most=max(S0["most"], nw), nf=S0["nf"] + 1, p=end, e=C[end],
                      P=S[end], stop=1 if end >= n else 0)
            if end > g and C[end] > Cg:
                st["span"] = C[end] - Cg
    nf = st["nf"]
    st_file(nf, n, None, st["o"])

    # merge_emit_kernel
    def last_le(lo, hi, x):
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if files[mid][0] <= x:
                lo = mid
            else:
                hi = mid
        return lo

    for f in range(nf + 1):
        if f not in files:
            raise Unsafe("files[%d] never written" % f)
    for j0 in range(0, n + 1, EMIT_BLOCK):
        s_lo = last_le(0, nf, j0) if nf else 0
        if nf and j0 < n and j0 > files[nf - 1][0]:
            cnt["emit_block_past_last_start"] += 1
        for j in range(j0, min(j0 + EMIT_BLOCK, n)):
            if not csize[j]:
                continue
            lo, step = s_lo, 0
            while lo + 1 < nf and files[lo + 1][0] <= j:
                if step == 4:
                    cnt["emit_research"] += 1
                    if mutant != "h":
                        lo = last_le(lo, nf, j)
                    break
                lo += 1
                step += 1
            if nf == 0 or files[lo][0] > j or j >= files[lo + 1][0]:
                continue
            Fp, Fx, Fo = files[lo]
            st_out(Fo + (Fx is not None) + (C[j] - C[Fp]), perm[j])
    res.nout, res.nfiles, res.most = st["o"], nf, st["most"]
    res.out = np.array([out.get(i, 0xFFFFFFFF) for i in range(res.nout)], np.uint32)
    res.out_past_nout = sorted(i for i in out if i >= res.nout)
    res.starts = np.array([files[f][2] for f in range(nf + 1)], np.uint64)
    res.paths = [paths.get(f, "?") for f in range(nf)]
    res.margin = margin[0]
    return res


# ---- the cases --------------------------------------------------------------
#
# Keys are 8 decimal digits, so a plain pair's EstimateSize is 24 + its value
# length.  A plain pair is 34 bytes and the usual threshold is 331: ten pairs
# a file (340 >= 331 > 306).  The sums are kept off the values at which
# (f + 1) * span + 0.5 or threshold * candidates / bytes is an integer.

SZ, T10 = 34, 331
BIG = 400  # >= T10: the file holding such a pair ends right after it


def K(i):
    return b"%08d" % i


def U(i, size=SZ):
    return (K(i), bytes([65 + i % 26]) * (size - 24))


def plain(i0, count, size=SZ):
    return [U(i, size) for i in range(i0, i0 + count)]


def group(i, t, v1=40, v0=BIG, more=0):
    """[V0, tombstone x t, V1, `more` further duplicates] under key i; v1 =
    V1's EstimateSize or None for a group with no second value."""
    g = [(K(i), b"0" * (v0 - 24))] + [(K(i), TOMB)] * t
    if v1 is not None:
        g.append((K(i), b"1" * (v1 - 24)))
    return g + [(K(i), b"m" * 6)] * more


def scramble(sorted_pairs, seed):
    """Input order: every pair at a random place, equal keys keeping their
    order (TIE_INPUT keeps input order inside a group, so the sorted order is
    the one given, and the sorted permutation is far from the identity)."""
    rng = random.Random(seed)
    n = len(sorted_pairs)
    slots = rng.sample(range(n), n)
    by_key = {}
    for i, (k, _) in enumerate(sorted_pairs):
        by_key.setdefault(k, []).append(i)
    out = [None] * n
    for idx in by_key.values():
        for i, s in zip(idx, sorted(slots[i] for i in idx)):
            out[s] = sorted_pairs[i]
    return out


def _random_pairs(rng, n, nkeys, tomb=0.25, empty=0.0):
    out = []
    for _ in range(n):
        k = b"" if rng.random() < empty else K(rng.randrange(nkeys))
        v = TOMB if rng.random() < tomb else bytes([rng.randrange(256)]) * rng.randrange(0, 40)
        out.append((k, v))
    return out


def _build():
    cs = []

    def add(name, sorted_pairs, level=6, T=T10, raw=False):
        pairs = sorted_pairs if raw else scramble(sorted_pairs, len(cs) + 1)
        cs.append(Case(name, pairs, level, T))

    # cand_ext: the file before ends right after V0 (V0 alone is >= T)
    def around(g, pre=10, post=25):
        return plain(0, pre) + g + plain(5000, post)

    add("ext_t0_level1", around(group(100, 0)), level=1)
    add("ext_t1", around(group(100, 1)))
    add("ext_t253", around(group(100, 253)))
    add("ext_t254", around(group(100, 254)))
    add("ext_none_inside", around(group(100, 5, v1=None)))
    add("ext_none_at_end", around(group(9000, 5, v1=None), post=0) )
    add("ext_tile_last", around(group(1000, 3), pre=511))
    add("ext_odd_position", around(group(100, 2), pre=11))
    # the extra against the threshold
    for d, nm in ((-1, "T-1"), (0, "T"), (1, "T+1")):
        add("extra_size_" + nm, around(group(100, 0, v1=T10 + d)), level=1)
    add("dups_each_fill_a_file", around([(K(100), bytes([48 + i]) * (BIG - 24)) for i in range(4)]), level=1)
    # one 2^24-byte extra under a threshold above it: 16,385 pairs of 1,024
    # bytes and V0 fill the first file
    big = 1 << 24
    add("extra_2p24", plain(0, 16385, 1024) + [(K(20000), b"0" * 1000), (K(20000), bytes(big))] +
        plain(30000, 7, 1024), level=1, T=big + 2047)
    # phase 1
    add("abs_one_file", plain(0, 7), T=10_001)
    for nres, tail in ((1, 5), (2, 5), (63, 5), (64, 5)):
        add("abs_nres%d" % nres, plain(0, 10 * nres + tail))
    # files past thread 63 hold 11 pairs of 31 bytes: the most pairs in a file
    # and the files' first slots come from the waves after wave 0
    add("abs_nres65", plain(0, 640) + plain(640, 11 + 6, 31))
    add("abs_nres131", plain(0, 640) + plain(640, 11 * 67 + 6, 31))
    add("abs_stop", plain(0, 70))
    add("abs_tail_of_dropped", plain(0, 70) + [(K(1000 + i), TOMB) for i in range(600)])
    add("abs_window_limit", plain(0, 4005))
    add("regime_small_to_large", plain(0, 3001) + plain(3001, 600, 340), T=3399)
    add("regime_large_to_small", plain(0, 600, 340) + plain(600, 3001), T=3399)
    add("file0_miss", plain(0, 2000, 24) + plain(2000, 200, 2424), T=23_999)
    add("file0_miss_wide", plain(0, 19699, 24) + plain(19699, 300, 2424), T=23_999)
    # a threshold below half the mean pair: every pair a file of its own
    add("tiny_T_41", plain(0, 41), T=11)
    add("tiny_T_400_stop", plain(0, 421), T=11)
    add("tiny_T_400_last", plain(0, 421) + [(K(1000 + i), TOMB) for i in range(3)], T=11)
    add("tiny_T_400_general", plain(0, 401) + group(500, 0, v0=SZ, v1=SZ) + plain(600, 19), T=11, level=1)
    # rounds: a plateau at window offset 0, accepted and refused.  The general
    # step's file (V1 and nine pairs) leaves span = 9 and R = 32 (windows of
    # 128); then come files of one pair.  File r + 1 of the round ends at
    # plateau e0 + r + 2, and window r + 1 starts at e0 + 9 (r + 2) - 64 once
    # that exceeds e0 + 1: at r + 2 = 8 exactly at the file's end (offset 0,
    # right after its start: accepted), at r + 2 = 9 past it (refused).
    add("round_offset0", plain(0, 10) + group(100, 254) + plain(200, 9) + plain(300, 12, BIG) + plain(400, 25))
    # the general step's group scan
    add("gen_len1023", around(group(100, 1022)))
    add("gen_len1024", around(group(100, 1023)))
    add("gen_len1025", around(group(100, 1024)))
    add("gen_len2102_w_chunk2", around(group(100, 2101)))
    add("gen_len2200_no_w", around(group(100, 2200, v1=None)))
    add("gen_w_chunk0_long_group", around(group(100, 300, more=2000)))
    add("gen_group_to_n", around(group(9000, 300, more=50), post=0))
    add("gen_nothing_left", around(group(9000, 300, v1=None), post=0))
    # emit
    rng = random.Random(77)
    add("emit_T1", sorted(_random_pairs(rng, 700, 500, tomb=0.1), key=lambda p: p[0]), T=1)
    # sizes
    for n in (1, 2, 511, 512, 513, 1024, 1025):
        rng = random.Random(n)
        add("size_n%d" % n, _random_pairs(rng, n, max(n // 2, 1)), T=197, raw=True)
    rng = random.Random(5)
    mix = _random_pairs(rng, 300, 60, tomb=0.3, empty=0.15)
    add("empty_keys_level6", mix, T=203, raw=True)
    add("empty_keys_level5", mix, T=203, level=5, raw=True)
    rng = random.Random(6)
    tb = _random_pairs(rng, 400, 150, tomb=0.5)
    add("tombstones_level5", tb, T=203, level=5, raw=True)
    add("tombstones_level6", tb, T=203, level=6, raw=True)
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _build()
BY_NAME = {c.name: c for c in CASES}

# The five cases also run through lsm_merge_kvs_async, and the two run back to
# back on one workspace (tests/test_merge_walk_gpu.py).
ASYNC_CASES = ("regime_small_to_large", "abs_window_limit", "ext_t254", "dups_each_fill_a_file", "abs_one_file")
BACK_TO_BACK = ("ext_t254", "regime_small_to_large")

# ---- the mutants ------------------------------------------------------------
#
# One-line, value-only changes of merge.hip (no loop exit, no barrier), each
# mirrored in census(case, mutant):
#  a  merge_walk_abs_kernel accepts pos == 0 unconditionally
#  b  the rounds' succession accepts lo == 0 unconditionally
#  c  walk_file: wsize >= T becomes wsize > T
#  d  merge_scan_apply stores X = 0 for an unresolved extra, not code 255
#  e  the general step takes w only from the first chunk (q0 == p)
#  f  `if (p != S0.p) code = kSuccGeneral` removed
#  g  phase 1 drops `pre` from a file's first slot
#  h  the emit stops at step == 4 without the re-search
#  i  the general step writes a file when nw == 0
#  j  phase 1 takes `most` from wave 0 only
# MUTANT_RED[m]: the cases whose output the model says m changes; every other
# case must stay green.  f changes nothing anywhere: a state whose p is not
# the position after plateau e comes only from a general step whose extra
# alone filled the file, and then cand_ext of plateau e either holds that same
# extra (size >= T) or is unresolved, so walk_file returns kSuccGeneral by
# itself.  MUTANT_UNSAFE[m]: cases in which the model says m reads a plateau
# past the last candidate; m is not run on them.
MUTANT_RED = {
    "a": {"regime_large_to_small"},
    "b": {"regime_small_to_large", "round_offset0"},
    "c": {"extra_size_T"},
    "d": {"ext_t254", "extra_2p24", "round_offset0", "gen_len1023", "gen_len1024", "gen_len1025",
          "gen_len2102_w_chunk2", "gen_w_chunk0_long_group", "gen_group_to_n"},
    "e": {"gen_len1025", "gen_len2102_w_chunk2"},
    "f": set(),
    "g": {"abs_nres64", "abs_nres65", "abs_nres131", "abs_window_limit", "tiny_T_400_stop", "tiny_T_400_last",
          "tiny_T_400_general", "size_n1024", "size_n1025"},
    "h": {"ext_tile_last", "extra_size_T-1", "extra_size_T", "extra_size_T+1", "dups_each_fill_a_file",
          "abs_nres63", "abs_nres64", "abs_nres65", "abs_nres131", "abs_stop", "abs_tail_of_dropped",
          "abs_window_limit", "regime_small_to_large", "regime_large_to_small", "file0_miss", "file0_miss_wide",
          "tiny_T_41", "tiny_T_400_stop", "tiny_T_400_last", "tiny_T_400_general", "round_offset0", "emit_T1",
          "size_n511", "size_n512", "size_n513", "size_n1024", "size_n1025", "empty_keys_level6",
          "empty_keys_level5", "tombstones_level5", "tombstones_level6"},
    "i": {"gen_nothing_left"},
    "j": {"abs_nres65", "abs_nres131"},
}
MUTANT_UNSAFE = {"b": {"file0_miss", "file0_miss_wide"}}


def most_pairs(starts):
    """The most pairs in one file, from the file starts."""
    return int(np.diff(np.asarray(starts).astype(np.int64)).max()) if len(starts) > 1 else 0


def agrees(r, want, wstarts):
    """Would a device computing what Census r models pass the GPU test?"""
    return (np.array_equal(r.out, want) and np.array_equal(r.starts, wstarts) and
            r.most == most_pairs(wstarts) and not r.out_past_nout)
