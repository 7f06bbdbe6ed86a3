// wal.hip — WAL replay: one long KV stream per log (SURVEY.md §8(f) f4;
// lsm_wal_replay), over decode_core.h's chase.
#include <string.h>

#include "decode_core.h"

namespace lsm {
namespace {

// wal.Recover chases a whole log (~1.7 MB, ~44k records for a 2 MiB
// memtable) as one serial chain; one wave per log would take milliseconds.
// The log is cut into 16 KiB segments, one wave each:
//   wal_seg_lanes_kernel: the segment guesses where its first record starts
//     (the first position from which two records in a row have plausible
//     lengths).  A record is two length-prefixed fields, so a chain started
//     at a value-length field looks just as plausible, one field out of
//     phase, and never meets the true chain: phase 0 starts at the guess g,
//     phase 1 at g + 4 + u32(g) (the record after the value if g was a
//     value length).  Each phase is chased to the first record starting in
//     the next segment, its records written to a scratch area of its own.
//   wal_stitch_kernel: one wave per log walks the segments in order with the
//     true chain position e (0 at the start).  A chain of the segment that
//     starts at e is the serial chase's (same start, same deterministic
//     chain); if neither does, the segment is chased again from e.  The
//     first error ends the log, as it ends Recover.
//   wal_compact_kernel: each segment's records move to their final slots.
// The result equals one serial chase for any input; guesses only decide how
// much is chased twice.
constexpr uint32_t kWalSeg = 16 * 1024;  // 12 and 8 KiB measured slower
constexpr uint32_t kWalSegSlots = kWalSeg / 8 + 1;  // records starting in a segment
// Scratch entry of a record of a segment's chain (wal_seg_lanes_kernel): its
// start less the segment's start (14 bits) and its key length (18 bits;
// kWalKlEsc: re-read from the log).  The value length is the distance to the
// next record's start (or to the chain's exit) less 8 + the key length: 4
// bytes per record and phase instead of a 16-byte descriptor (the scratch
// round trip was 1.9x the replay's algorithmic bytes).
constexpr uint32_t kWalPosBits = 14;
constexpr uint32_t kWalKlEsc = (1u << (32 - kWalPosBits)) - 1;
static_assert(kWalSeg <= (1u << kWalPosBits), "segment offsets fit the scratch entry");
// fin[2q + 1] flags: the chosen phase, and a segment the stitch chased again
// (its records in the scratch as full descriptors)
constexpr uint32_t kWalFinPhase1 = 0x80000000u, kWalFinFull = 0x40000000u, kWalFinCount = 0x3FFFFFFFu;

struct WalSeg {
    uint32_t entry, exit, nrec;
    int32_t status;
};

struct WalArgs {
    const uint8_t *wal;
    const uint64_t *wal_off;
    const uint32_t *wal_len;
    uint32_t nwal, segs, max_len;
    lsm_decode_out out;
    WalSeg *seg;      // nwal * segs * 2 (two phases)
    uint32_t *fin;    // nwal * segs * 2: prefix, count | phase << 31
    u32x4 *scratch;   // nwal * segs * 2 * kWalSegSlots
};

__device__ __forceinline__ void wal_slots(const WalArgs &a, uint32_t w, uint64_t &base,
                                          uint64_t &cap) {
    if (a.out.rec_base) {
        base = a.out.rec_base[w];
        cap = a.out.rec_base[w + 1] - base;
    } else {
        const uint64_t o = a.wal_off[w];
        base = o / 8;
        cap = (o + a.wal_len[w]) / 8 - base;
    }
}

// Lane-parallel segment chase.  WAL records are small
// (~40 B for go-lsm's benchmark) and vary in shape, so one wave chasing a
// 16 KiB segment spends its time in ~400 serial exact steps.  Here the
// segment [g, E) (g the segment's guess as above, E its end) is split into
// 64 shares, one per lane:
//   1. lane 0 starts at g; lane l > 0 guesses its first record start (the
//      first position of its share from which two plausible records follow)
//      and chases both field phases (the guess, and the guess read as a value
//      length), each to the first record starting past its share;
//   2. the wave stitches the shares in order from g: the chain that starts
//      where the previous share ended is the serial chase's; if neither
//      does, that share is chased again from the true position;
//   3. each lane writes the descriptors of its accepted chain.
// The result is the serial chase of [g, E) for any input (exact check order
// of kv.go:77-115); the segment is read from an LDS copy (plus 4 KiB past
// its end) and past that through a range-checked buffer resource.
// LDS copy of a segment plus a tail for the chains that cross its end.  The
// copy sets the occupancy (160 KiB LDS per CU): + 1 KiB admits 9 waves per CU
// and measured 603 GiB/s on the wal bench; + 3.5 KiB (8 waves) 552 and + 4 KiB
// (20,496 B: 7 waves) 542.  Reads past the tail go through the buffer resource.
constexpr uint32_t kWalStage = kWalSeg + 1024;

struct WalLog {
    rsrc_t r;       // the log's bytes, offsets relative to the aligned base
    uint32_t h;     // log start inside the base
    uint32_t len;
    uint32_t s0;    // LDS copy covers resource offsets [s0, s0 + sz)
    uint32_t sz;
    const uint32_t *lds;
    __device__ __forceinline__ uint32_t rd32(uint32_t x) const {  // bytes [x, x+4) of the log
        const uint32_t o = h + x;
        if (o >= s0 && o + 8 <= s0 + sz) {
            const uint32_t q = o - s0;
            return funnel(lds[q >> 2], lds[(q >> 2) + 1], q);
        }
        const uint32_t oa = o & ~3u;
        return funnel(ld_b32(r, oa), ld_b32(r, oa + 4), o);
    }
    // exact KV record at p < len (kv.go:77-115 / ora_decode_block order)
    __device__ __forceinline__ int32_t record(uint32_t p, uint32_t &kl, uint32_t &vl) const {
        const uint32_t rem = len - p;
        if (rem < 4) return LSM_ST_TRUNC_LEN_PREFIX;
        kl = rd32(p);
        if (kl > kKeyCap) return LSM_ST_KEY_TOO_LONG;
        if (rem - 4 < kl) return LSM_ST_TRUNC_KEY;
        const uint32_t rem2 = rem - 4 - kl;
        if (rem2 < 4) return LSM_ST_TRUNC_VLEN;
        vl = rd32(p + 4 + kl);
        if (vl > kValCap) return LSM_ST_VAL_TOO_LONG;
        if (rem2 - 4 < vl) return LSM_ST_TRUNC_VAL;
        return LSM_OK;
    }
    // bytes [x, x+4) and [y, y+4): both from LDS in one round trip when both
    // lie in the copy (the common case), else one at a time
    __device__ __forceinline__ void rd32x2(uint32_t x, uint32_t y, uint32_t &u, uint32_t &v) const {
        const uint32_t ox = h + x - s0, oy = h + y - s0;  // wraps above sz when below s0
        if (ox <= sz - 8 && oy <= sz - 8) {
            const uint32_t a0 = lds[ox >> 2], a1 = lds[(ox >> 2) + 1];
            const uint32_t b0 = lds[oy >> 2], b1 = lds[(oy >> 2) + 1];
            u = funnel(a0, a1, ox);
            v = funnel(b0, b1, oy);
        } else {
            u = rd32(x);
            v = rd32(y);
        }
    }
    // chase() of two chains at once (a lane's two guesses): each step reads
    // both chains' key lengths in one LDS round trip, then both value lengths
    // (the chains are independent; chased one after the other they were two
    // serial chains of dependent reads).  `park` is a position inside the copy
    // for a chain that has stopped.  Same results as two chase() calls.
    __device__ __forceinline__ void chase2(uint32_t pa, uint32_t pb, uint32_t end, uint32_t park,
                                           uint32_t &ca, uint32_t &xa, int32_t &sa, uint32_t &cb,
                                           uint32_t &xb, int32_t &sb) const {
        chase2(pa, pb, end, end, park, ca, xa, sa, cb, xb, sb);
    }
    // the same with an end per chain
    __device__ __forceinline__ void chase2(uint32_t pa, uint32_t pb, uint32_t enda, uint32_t endb,
                                           uint32_t park, uint32_t &ca, uint32_t &xa, int32_t &sa,
                                           uint32_t &cb, uint32_t &xb, int32_t &sb) const {
        ca = cb = 0;
        sa = sb = LSM_OK;
        bool ra = pa < enda && pa < len, rb = pb < endb && pb < len;
        while (ra || rb) {
            // kv.go:77-115 order, as record(): length prefix, key, value length, value
            const uint32_t rma = len - pa, rmb = len - pb;
            const bool ka_ok = ra && rma >= 4, kb_ok = rb && rmb >= 4;
            uint32_t ka, kb;
            rd32x2(ka_ok ? pa : park, kb_ok ? pb : park, ka, kb);
            const bool ka2 = ka_ok && ka <= kKeyCap && rma - 4 >= ka && rma - 4 - ka >= 4;
            const bool kb2 = kb_ok && kb <= kKeyCap && rmb - 4 >= kb && rmb - 4 - kb >= 4;
            uint32_t va, vb;
            rd32x2(ka2 ? pa + 4 + ka : park, kb2 ? pb + 4 + kb : park, va, vb);
            if (ra) {
                int32_t st = LSM_OK;
                if (!ka_ok) st = LSM_ST_TRUNC_LEN_PREFIX;
                else if (ka > kKeyCap) st = LSM_ST_KEY_TOO_LONG;
                else if (rma - 4 < ka) st = LSM_ST_TRUNC_KEY;
                else if (rma - 4 - ka < 4) st = LSM_ST_TRUNC_VLEN;
                else if (va > kValCap) st = LSM_ST_VAL_TOO_LONG;
                else if (rma - 8 - ka < va) st = LSM_ST_TRUNC_VAL;
                if (st != LSM_OK) {
                    sa = st;
                    ra = false;
                } else {
                    ca++;
                    pa += 8 + ka + va;
                    ra = pa < enda && pa < len;
                }
            }
            if (rb) {
                int32_t st = LSM_OK;
                if (!kb_ok) st = LSM_ST_TRUNC_LEN_PREFIX;
                else if (kb > kKeyCap) st = LSM_ST_KEY_TOO_LONG;
                else if (rmb - 4 < kb) st = LSM_ST_TRUNC_KEY;
                else if (rmb - 4 - kb < 4) st = LSM_ST_TRUNC_VLEN;
                else if (vb > kValCap) st = LSM_ST_VAL_TOO_LONG;
                else if (rmb - 8 - kb < vb) st = LSM_ST_TRUNC_VAL;
                if (st != LSM_OK) {
                    sb = st;
                    rb = false;
                } else {
                    cb++;
                    pb += 8 + kb + vb;
                    rb = pb < endb && pb < len;
                }
            }
        }
        xa = pa;
        xb = pb;
    }
    // chase from p while records start before `end`: count, stop position, status
    __device__ __forceinline__ void chase(uint32_t p, uint32_t end, uint32_t &cnt, uint32_t &exitp,
                                          int32_t &st) const {
        cnt = 0;
        st = LSM_OK;
        while (p < end && p < len) {
            uint32_t kl = 0, vl = 0;
            st = record(p, kl, vl);
            if (st != LSM_OK) break;
            cnt++;
            p += 8 + kl + vl;
        }
        exitp = p;
    }
    // The first plausible start in [ss, se), every position of which lies in
    // the LDS copy (a lane's share of its segment).  A plausible start holds a
    // key length <= 1024, so its u32 has two zero high bytes: positions are
    // screened 16 at a time from five LDS dwords read together, and only the
    // (few) that pass -- in KV logs the length fields -- are tested in full.
    // (Testing every position in full was a serial chain of ~40 dependent
    // LDS round trips per lane.)
    __device__ __forceinline__ uint32_t first_plausible(uint32_t ss, uint32_t se) const {
        const uint32_t ob = h - s0;  // LDS byte offset of log position 0 (mod 2^32)
        for (uint32_t w = (ob + ss) >> 2; 4 * w < ob + se; w += 4) {
            uint32_t d[5];
#pragma unroll
            for (uint32_t t = 0; t < 5; t++) d[t] = lds[w + t];
            uint32_t m = 0;
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) {
                const uint32_t x = funnel(d[j >> 2], d[(j >> 2) + 1], j);
                const uint32_t p = 4 * w + j - ob;
                m |= (uint32_t)(x <= 1024u && p >= ss && p < se) << j;
            }
            while (m) {
                const uint32_t p = 4 * w + (uint32_t)__builtin_ctz(m) - ob;
                if (plausible(p)) return p;
                m &= m - 1;
            }
        }
        return 0xFFFFFFFFu;
    }
    // plausible record start (as the segment guess: two records or the log's end)
    __device__ __forceinline__ bool plausible(uint32_t q) const {
        uint32_t seen = 0;
        for (int rec = 0; rec < 2; rec++) {
            if (q == len) return seen >= 1;
            if ((uint64_t)q + 8 > len) return false;
            const uint32_t k = rd32(q);
            if (k > 1024 || (uint64_t)q + 8 + k > len) return false;
            const uint32_t v = rd32(q + 4 + k);
            if (v > (1u << 20) || (uint64_t)q + 8 + k + v > len) return false;
            q += 8 + k + v;
            seen++;
        }
        return true;
    }
};

// One wave serves both phases of a segment: the shares' chains do not depend
// on the segment's entry, only lane 0's does, so they are chased once and
// stitched twice (from g and from g read as a value length).
__global__ __launch_bounds__(64) void wal_seg_lanes_kernel(WalArgs a) {
    constexpr uint32_t STAGE = kWalStage;
    __shared__ __attribute__((aligned(16))) uint32_t stage[STAGE / 4 + 4];
    const uint32_t s = blockIdx.x, w = blockIdx.y, lane = lane_id();
    const uint32_t len = uni(a.wal_len[w]);
    const uint64_t off = uni64(a.wal_off[w]);
    const uint64_t q0 = ((uint64_t)w * a.segs + s) * 2;
    const uint32_t start = s * kWalSeg;
    if (start >= len || len > a.max_len) {
        if (lane == 0) a.seg[q0] = a.seg[q0 + 1] = WalSeg{0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0};
        return;
    }
    WalLog L;
    const uint64_t base = off & ~(uint64_t)15;
    L.h = (uint32_t)(off - base);
    L.len = len;
    L.r = make_rsrc(a.wal + base, (L.h + len + 15) & ~15u);
    L.s0 = (L.h + start) & ~15u;
    L.sz = STAGE;
    L.lds = stage;
    {
        // the segment + a tail (the loads are already all in flight: staging
        // by buffer_load ... lds measured no faster)
        for (uint32_t c = 0; c < STAGE / 16; c += kWave) {
            const uint32_t o = L.s0 + 16 * (c + lane);
            if (c + lane < STAGE / 16)
                *reinterpret_cast<u32x4 *>(&stage[4 * (c + lane)]) = ld_b128(L.r, o);
        }
        __syncthreads();
    }
    uint32_t g = start, g1 = 0xFFFFFFFFu;  // entries of phase 0 and phase 1
    if (s > 0) {  // the segment's guess: the first plausible start in its first 2 KiB
        g = 0xFFFFFFFFu;
        const uint32_t span = len - start < 2048 ? len - start : 2048;
        for (uint32_t t0 = 0; t0 < span && g == 0xFFFFFFFFu; t0 += kWave) {
            const uint32_t p = start + t0 + lane;
            const uint64_t m = __ballot(t0 + lane < span && L.plausible(p));
            if (m) g = start + t0 + (uint32_t)__builtin_ctzll(m);
        }
        if (g == 0xFFFFFFFFu) g = start;
        g = uni(g);
        const uint32_t v = (uint64_t)g + 4 <= len ? L.rd32(g) : 0xFFFFFFFFu;
        g1 = uni((uint64_t)g + 4 + v <= len ? g + 4 + v : len);
    }
    const uint32_t E = start + kWalSeg < len ? start + kWalSeg : len;
    // 1. shares of [start, E): lane 0's chains are the two entries themselves.
    //    A share width of a multiple of 128 B would start every lane on the
    //    same LDS bank; widths of 4 mod 8 dwords spread them.
    uint32_t W = (E - start + kWave - 1) / kWave;
    W = (W + 3) & ~3u;
    if ((W / 4) % 8 != 4) W += 4 * ((12 - (W / 4) % 8) % 8);
    const uint32_t ss = start + lane * W < E ? start + lane * W : E;
    const uint32_t se = ss + W < E ? ss + W : E;
    uint32_t e0 = 0xFFFFFFFFu, e1 = 0xFFFFFFFFu, c0 = 0, c1 = 0, x0 = 0, x1 = 0;
    int32_t st0 = LSM_OK, st1 = LSM_OK;
    if (lane > 0 && ss < se) {
        e0 = L.first_plausible(ss, se);
        if (e0 != 0xFFFFFFFFu && (uint64_t)e0 + 4 <= len) {
            const uint32_t v = L.rd32(e0);
            if ((uint64_t)e0 + 4 + v <= len) e1 = e0 + 4 + v;
        }
    }
    // A guess at or past the share's end is a chain with no records that
    // passes its position through (exit = the guess); chase() returns exactly
    // that.  Leaving its exit unset once made a share holding only a value
    // field report exit 0 when the previous chain ended on that guess.
    {
        // both guesses' chains at once; a missing guess is a stopped chain
        // (its count, exit and status keep their initial values)
        uint32_t ca, xa, cb, xb;
        int32_t sa, sb;
        L.chase2(e0 != 0xFFFFFFFFu ? e0 : se, e1 != 0xFFFFFFFFu ? e1 : se, se, start, ca, xa, sa, cb,
                 xb, sb);
        if (e0 != 0xFFFFFFFFu) { c0 = ca; x0 = xa; st0 = sa; }
        if (e1 != 0xFFFFFFFFu) { c1 = cb; x1 = xb; st1 = sb; }
    }
    // The share holding each phase's entry is chased exactly from the entry
    // (the fast stitch below), both phases together.
    uint32_t kc[2], cc[2], xc[2];
    int32_t sc[2];
    {
        const uint32_t live1 = s > 0 && g1 < E;  // phase 1 exists (g < E always)
        kc[0] = (g - start) / W;
        kc[1] = live1 ? (g1 - start) / W : 0;
        const uint32_t se0 = uni(__builtin_amdgcn_readlane(se, kc[0]));
        const uint32_t se1 = uni(__builtin_amdgcn_readlane(se, kc[1]));
        L.chase2(g, live1 ? g1 : se1, se0, se1, start, cc[0], xc[0], sc[0], cc[1], xc[1], sc[1]);
#pragma unroll
        for (uint32_t i = 0; i < 2; i++) {
            cc[i] = uni(cc[i]);
            xc[i] = uni(xc[i]);
            sc[i] = (int32_t)uni((uint32_t)sc[i]);
        }
    }
    // 2. per phase: stitch from the entry (each lane's accepted chain)
    uint32_t wpre[2] = {0, 0}, wentry[2] = {0, 0}, wcnt[2] = {0, 0};
#pragma unroll
    for (uint32_t ph = 0; ph < 2; ph++) {
        const uint64_t q = q0 + ph;
        const uint32_t gp = ph ? g1 : g;
        if (ph == 1 && s == 0) {  // segment 0 starts at 0
            if (lane == 0) a.seg[q] = WalSeg{0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0};
            break;
        }
        if (gp >= E) {
            if (lane == 0) a.seg[q] = WalSeg{gp, gp, 0, 0};
            continue;
        }
        uint32_t e = gp, acc_entry = 0xFFFFFFFFu, acc_cnt = 0, total = 0;
        int32_t status = LSM_OK;
        bool dead = false;
        // fast stitch: the share k holding the entry is chased exactly; after
        // it, lane l's choice of chain (0: from e0, 1: from e1) is a function
        // of lane l-1's choice (its chain's exit matched against lane l's
        // entries); a 6-step scan composes these maps across the lanes.  Any
        // miss (a wrong guess, or a record longer than a share) falls back to
        // the serial stitch below.
        bool fast = false;
        {
            const uint32_t k = kc[ph];
            const uint32_t last = (E - 1 - start) / W < kWave - 1 ? (E - 1 - start) / W : kWave - 1;
            const uint32_t ck = cc[ph], xk = xc[ph];
            const int32_t stk = sc[ph];
            auto match = [&](uint32_t x) -> uint32_t {
                return (e0 != 0xFFFFFFFFu && x == e0) ? 0u : (e1 != 0xFFFFFFFFu && x == e1) ? 1u : 2u;
            };
            // map from lane l-1's choice to lane l's, as h0 | h1 << 4 (2 = miss)
            const uint32_t xp0 = __shfl_up(x0, 1), xp1 = __shfl_up(x1, 1);
            const uint32_t ep0 = __shfl_up(e0, 1), ep1 = __shfl_up(e1, 1);
            uint32_t h;
            if (lane <= k) {
                h = 0u | 1u << 4;  // identity (never used: lane k+1's map is constant)
            } else if (lane == k + 1) {
                const uint32_t c = match(xk);
                h = c | c << 4;
            } else {
                const uint32_t m0 = ep0 != 0xFFFFFFFFu ? match(xp0) : 2u;
                const uint32_t m1 = ep1 != 0xFFFFFFFFu ? match(xp1) : 2u;
                h = m0 | m1 << 4;
            }
#pragma unroll
            for (uint32_t d = 1; d < kWave; d <<= 1) {
                const uint32_t pv = __shfl_up(h, d);
                if (lane >= d) {  // h := h o pv
                    const uint32_t p0 = pv & 15, p1 = pv >> 4;
                    const uint32_t n0 = p0 == 2 ? 2u : p0 == 0 ? (h & 15) : (h >> 4);
                    const uint32_t n1 = p1 == 2 ? 2u : p1 == 0 ? (h & 15) : (h >> 4);
                    h = n0 | n1 << 4;
                }
            }
            const uint32_t ch = h & 15;  // lanes k+1 .. last: the chosen chain
            const bool live = lane > k && lane <= last;
            const int32_t cst = ch == 0 ? st0 : st1;
            const uint64_t errm = __ballot(live && ch < 2 && cst != LSM_OK);
            const uint32_t lim = stk != LSM_OK ? k : errm ? (uint32_t)__builtin_ctzll(errm) : last;
            const uint64_t below = lim >= kWave - 1 ? ~0ull : (2ull << lim) - 1;  // lanes <= lim
            const uint64_t missm = __ballot(live && ch == 2) & below;
            if (!missm) {
                fast = true;
                if (lane == k) {
                    acc_entry = gp;
                    acc_cnt = ck;
                } else if (live && lane <= lim) {
                    acc_entry = ch == 0 ? e0 : e1;
                    acc_cnt = ch == 0 ? c0 : c1;
                }
                const uint32_t xe = ch == 0 ? x0 : x1;
                if (lim == k) {
                    e = xk;
                    status = stk;
                } else {
                    e = uni(__builtin_amdgcn_readlane(xe, lim));
                    status = errm ? (int32_t)uni(__builtin_amdgcn_readlane((uint32_t)cst, lim)) : LSM_OK;
                }
                uint32_t t;
                wave_excl_scan(acc_cnt, &t);
                total = t;
            }
        }
        for (uint32_t l = 0; !fast && l < kWave; l++) {
            const uint32_t sl = uni(__builtin_amdgcn_readlane(ss, l));
            const uint32_t el = uni(__builtin_amdgcn_readlane(se, l));
            if (dead || sl >= el || e >= el) continue;
            uint32_t cnt, ex;
            int32_t st;
            if (l > 0 && uni(__builtin_amdgcn_readlane(e0, l)) == e) {
                cnt = uni(__builtin_amdgcn_readlane(c0, l));
                ex = uni(__builtin_amdgcn_readlane(x0, l));
                st = (int32_t)uni(__builtin_amdgcn_readlane((uint32_t)st0, l));
            } else if (l > 0 && uni(__builtin_amdgcn_readlane(e1, l)) == e) {
                cnt = uni(__builtin_amdgcn_readlane(c1, l));
                ex = uni(__builtin_amdgcn_readlane(x1, l));
                st = (int32_t)uni(__builtin_amdgcn_readlane((uint32_t)st1, l));
            } else {  // the entry share, or neither guess on the chain: chase from e
                L.chase(e, el, cnt, ex, st);
                cnt = uni(cnt);
                ex = uni(ex);
                st = (int32_t)uni((uint32_t)st);
            }
            if (lane == l) {
                acc_entry = e;
                acc_cnt = cnt;
            }
            total += cnt;
            e = ex;
            if (st != LSM_OK) {
                status = st;
                dead = true;
            }
        }
        uint32_t tot;
        wpre[ph] = wave_excl_scan(acc_cnt, &tot);
        wentry[ph] = acc_entry;
        wcnt[ph] = acc_cnt;
        if (lane == 0) a.seg[q] = WalSeg{gp, e, total, status};
    }
    // 3. both phases' accepted chains walked together, a 4-byte scratch entry
    //    per record: each step reads both key lengths in one LDS round trip,
    //    then both value lengths (walked one phase after the other they were
    //    two serial chains: 1,117 -> 1,167 GiB/s, A/B)
    {
        uint32_t *dst0 = reinterpret_cast<uint32_t *>(a.scratch + q0 * kWalSegSlots) + wpre[0];
        uint32_t *dst1 = reinterpret_cast<uint32_t *>(a.scratch + (q0 + 1) * kWalSegSlots) + wpre[1];
        uint32_t pa = wentry[0], pb = wentry[1];
        const uint32_t n = wcnt[0] > wcnt[1] ? wcnt[0] : wcnt[1];
        for (uint32_t i = 0; i < n; i++) {
            const bool ra = i < wcnt[0], rb = i < wcnt[1];
            uint32_t ka, kb, va, vb;
            L.rd32x2(ra ? pa : start, rb ? pb : start, ka, kb);
            L.rd32x2(ra ? pa + 4 + ka : start, rb ? pb + 4 + kb : start, va, vb);
            if (ra) {
                dst0[i] = (pa - start) | (ka < kWalKlEsc ? ka : kWalKlEsc) << kWalPosBits;
                pa += 8 + ka + va;
            }
            if (rb) {
                dst1[i] = (pb - start) | (kb < kWalKlEsc ? kb : kWalKlEsc) << kWalPosBits;
                pb += 8 + kb + vb;
            }
        }
    }
}

__global__ __launch_bounds__(64) void wal_stitch_kernel(WalArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t ring[8 * kChunk / 4 + 4];
    const uint32_t w = blockIdx.x, lane = lane_id();
    const uint32_t len = uni(a.wal_len[w]);
    const uint64_t off = uni64(a.wal_off[w]);
    uint64_t base, cap;
    wal_slots(a, w, base, cap);
    base = uni64(base);
    const uint32_t ocap = uni(cap < 0xFFFFFFFFull ? (uint32_t)cap : 0xFFFFFFFFu);
    if (len > a.max_len) {  // outside the segment grid: one exact chase, in place
        DecodeArgs d = {};
        d.in = a.wal;
        d.desc = a.out.desc ? reinterpret_cast<u32x4 *>(a.out.desc) : nullptr;
        uint32_t nr = 0;
        int32_t st = LSM_OK;
        decode_range_any<LSM_GRAMMAR_KV, 8>(d, ring, off, len, base, ocap, nr, st);
        for (uint32_t s = lane; s < a.segs; s += kWave) {
            a.fin[2 * ((uint64_t)w * a.segs + s)] = 0;
            a.fin[2 * ((uint64_t)w * a.segs + s) + 1] = 0;
        }
        if (lane == 0) {
            a.out.nrec[w] = nr;
            a.out.status[w] = st;
        }
        return;
    }
    const uint32_t nseg = (len + kWalSeg - 1) / kWalSeg;
    uint32_t e = 0, total = 0;
    int32_t status = LSM_OK;
    bool dead = false;
    for (uint32_t s0 = 0; s0 < a.segs; s0 += kWave) {
        const uint32_t sl = s0 + lane;
        const uint64_t q0 = ((uint64_t)w * a.segs + sl) * 2;
        const WalSeg T0 = sl < nseg ? a.seg[q0] : WalSeg{0, 0, 0, 0};
        const WalSeg T1 = sl < nseg ? a.seg[q0 + 1] : WalSeg{0, 0, 0, 0};
        uint32_t f_pre = 0, f_cnt = 0;
        // fast form: segment j's choice of chain (0, 1; 2 = neither, or the
        // previous chain runs past segment j's end) is a function of segment
        // j-1's choice; a 6-step scan composes these maps across the 64
        // segments of the group, as wal_seg_lanes_kernel does across shares.
        // Any miss before the first error falls back to the serial walk.
        bool fast = false;
        if (!dead && s0 < nseg) {
            const uint32_t gl = nseg - s0 < kWave ? nseg - s0 : kWave;  // live segments
            const bool live = lane < gl;
            const uint32_t send = (sl + 1) * kWalSeg;
            auto match = [&](uint32_t x) -> uint32_t {
                return x >= send ? 2u : x == T0.entry ? 0u : x == T1.entry ? 1u : 2u;
            };
            const uint32_t xp0 = __shfl_up(T0.exit, 1), xp1 = __shfl_up(T1.exit, 1);
            uint32_t h;
            if (lane == 0) {
                const uint32_t c = match(e);
                h = c | c << 4;
            } else {
                h = match(xp0) | match(xp1) << 4;
            }
#pragma unroll
            for (uint32_t d = 1; d < kWave; d <<= 1) {
                const uint32_t pv = __shfl_up(h, d);
                if (lane >= d) {  // h := h o pv
                    const uint32_t p0 = pv & 15, p1 = pv >> 4;
                    const uint32_t n0 = p0 == 2 ? 2u : p0 == 0 ? (h & 15) : (h >> 4);
                    const uint32_t n1 = p1 == 2 ? 2u : p1 == 0 ? (h & 15) : (h >> 4);
                    h = n0 | n1 << 4;
                }
            }
            const uint32_t ch = h & 15;
            const int32_t cst = ch == 0 ? T0.status : T1.status;
            const uint64_t errm = __ballot(live && ch < 2 && cst != LSM_OK);
            const uint32_t lim = errm ? (uint32_t)__builtin_ctzll(errm) : gl - 1;
            const uint64_t below = lim >= kWave - 1 ? ~0ull : (2ull << lim) - 1;  // lanes <= lim
            if (!(__ballot(live && ch == 2) & below)) {
                fast = true;
                const bool take = live && lane <= lim;
                const uint32_t nr = take ? (ch == 0 ? T0.nrec : T1.nrec) : 0u;
                const uint32_t xe = ch == 0 ? T0.exit : T1.exit;
                uint32_t sum;
                f_pre = total + wave_excl_scan(nr, &sum);
                f_cnt = nr | (take && ch == 1 ? kWalFinPhase1 : 0u);
                total += uni(sum);
                e = uni(__builtin_amdgcn_readlane(xe, lim));
                if (errm) {
                    status = (int32_t)uni(__builtin_amdgcn_readlane((uint32_t)cst, lim));
                    dead = true;
                }
            }
        }
        for (uint32_t j = 0; !fast && j < kWave && s0 + j < nseg; j++) {
            const uint32_t s = s0 + j;
            uint32_t pre = total, cnt = 0;
            if (!dead && e < len && e < (s + 1) * kWalSeg) {
                const uint32_t e0 = uni(__builtin_amdgcn_readlane(T0.entry, j));
                const uint32_t e1 = uni(__builtin_amdgcn_readlane(T1.entry, j));
                const uint32_t ph = e0 == e ? 0u : e1 == e ? 1u : 2u;
                uint32_t ex, nr;
                int32_t st;
                if (ph == 0) {
                    ex = uni(__builtin_amdgcn_readlane(T0.exit, j));
                    nr = uni(__builtin_amdgcn_readlane(T0.nrec, j));
                    st = (int32_t)uni(__builtin_amdgcn_readlane((uint32_t)T0.status, j));
                } else if (ph == 1) {
                    ex = uni(__builtin_amdgcn_readlane(T1.exit, j));
                    nr = uni(__builtin_amdgcn_readlane(T1.nrec, j));
                    st = (int32_t)uni(__builtin_amdgcn_readlane((uint32_t)T1.status, j));
                } else {  // both guesses missed: chase from the true position
                    DecodeArgs d = {};
                    d.in = a.wal;
                    d.desc = a.scratch;
                    const uint32_t stop = ((s + 1) * kWalSeg < len ? (s + 1) * kWalSeg : len) - e;
                    uint32_t endp = 0;
                    nr = 0;
                    st = LSM_OK;
                    decode_range_any<LSM_GRAMMAR_KV, 8>(
                        d, ring, off + e, len - e, ((uint64_t)w * a.segs + s) * 2 * kWalSegSlots,
                        kWalSegSlots, nr, st, stop, &endp);
                    ex = e + endp;
                }
                cnt = nr | (ph == 1 ? kWalFinPhase1 : ph == 2 ? kWalFinFull : 0u);
                total += nr;
                e = ex;
                if (st != LSM_OK) {
                    status = st;
                    dead = true;
                }
            } else if (e >= len) {
                dead = true;
            }
            if (lane == j) {
                f_pre = pre;
                f_cnt = cnt;
            }
        }
        if (sl < a.segs) {
            a.fin[2 * ((uint64_t)w * a.segs + sl)] = f_pre;
            a.fin[2 * ((uint64_t)w * a.segs + sl) + 1] = f_cnt;
        }
    }
    if (lane == 0) {
        if (total > ocap) {  // caller's record capacity (not a reference error)
            total = ocap;
            status = LSM_ST_CAPACITY;
        }
        a.out.nrec[w] = total;
        a.out.status[w] = status;
    }
}

__global__ __launch_bounds__(256) void wal_compact_kernel(WalArgs a) {
    const uint32_t s = blockIdx.x, w = blockIdx.y;
    const uint64_t q = (uint64_t)w * a.segs + s;
    const uint32_t pre = a.fin[2 * q], cf = a.fin[2 * q + 1];
    const uint32_t cnt = cf & kWalFinCount;
    if (cnt == 0) return;
    uint64_t base, cap;
    wal_slots(a, w, base, cap);
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.out.desc);
    const uint32_t ph = cf >> 31;
    if (cf & kWalFinFull) {  // chased again by the stitch: full descriptors
        const u32x4 *src = a.scratch + q * 2 * kWalSegSlots;
        for (uint32_t j = threadIdx.x; j < cnt; j += blockDim.x)
            if ((uint64_t)pre + j < cap)  // nt: written once (A/B: 997 -> 1,017 GiB/s)
                __builtin_nontemporal_store(src[j], &dst[base + pre + j]);
        return;
    }
    // packed entries: record j ends where record j + 1 starts (the chain's
    // exit after the last), so its value length is that distance less 8 +
    // its key length
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.scratch + (q * 2 + ph) * kWalSegSlots);
    const uint64_t start = (uint64_t)a.wal_off[w] + (uint64_t)s * kWalSeg;
    const uint32_t rel_exit = a.seg[q * 2 + ph].exit - s * kWalSeg;
    for (uint32_t j = threadIdx.x; j < cnt; j += blockDim.x) {
        if ((uint64_t)pre + j >= cap) continue;
        const uint32_t e = src[j];
        const uint32_t p = e & ((1u << kWalPosBits) - 1);
        const uint32_t pn = j + 1 < cnt ? (src[j + 1] & ((1u << kWalPosBits) - 1)) : rel_exit;
        uint32_t kl = e >> kWalPosBits;
        if (kl == kWalKlEsc) {  // a key of 2^18 bytes or more: its length from the log
            const uint8_t *kp = a.wal + start + p;
            kl = (uint32_t)kp[0] | (uint32_t)kp[1] << 8 | (uint32_t)kp[2] << 16 | (uint32_t)kp[3] << 24;
        }
        const uint64_t ro = start + p;
        __builtin_nontemporal_store(u32x4{(uint32_t)ro, (uint32_t)(ro >> 32), kl, pn - p - 8 - kl},
                                    &dst[base + pre + j]);
    }
}

// The workspace: per segment and phase the scratch records (16-byte aligned
// first), then the WalSeg, then two `fin` words per segment.  Returns the
// bytes needed; with `a`, sets a->segs and carves `base`.
size_t wal_ws_layout(uint8_t *base, uint32_t nwal, uint32_t max_wal_len, WalArgs *a) {
    const uint32_t segs = max_wal_len ? (uint32_t)(((uint64_t)max_wal_len + kWalSeg - 1) / kWalSeg) : 1;
    const uint64_t n = (uint64_t)nwal * segs;
    const uint64_t scratch = n * 2 * kWalSegSlots * 16, seg = n * 2 * sizeof(WalSeg), fin = n * 8;
    if (a) {
        a->segs = segs;
        a->scratch = reinterpret_cast<u32x4 *>(base);
        a->seg = reinterpret_cast<WalSeg *>(base + scratch);
        a->fin = reinterpret_cast<uint32_t *>(base + scratch + seg);
    }
    return (size_t)(scratch + seg + fin + 64);
}

}  // namespace
}  // namespace lsm

using namespace lsm;

extern "C" size_t lsm_wal_replay_workspace_bytes(uint32_t nwal, uint32_t max_wal_len) {
    return wal_ws_layout(nullptr, nwal, max_wal_len, nullptr);
}

extern "C" int lsm_wal_replay(lsm_ctx *ctx, const uint8_t *d_wal, const uint64_t *d_wal_off,
                              const uint32_t *d_wal_len, uint32_t nwal, uint32_t max_wal_len,
                              const lsm_decode_out *out, void *d_workspace, size_t ws_bytes,
                              void *stream) {
    if (!ctx || !out) return LSM_EINVAL;
    if (nwal == 0) return 0;
    if (!d_wal || !d_wal_off || !d_wal_len || !out->desc || !out->nrec || !out->status ||
        !d_workspace || out->key_arena || out->val_arena || nwal > 65535)
        return LSM_EINVAL;
    WalArgs a;
    if (ws_bytes < wal_ws_layout(static_cast<uint8_t *>(d_workspace), nwal, max_wal_len, &a))
        return LSM_ESPACE;
    a.wal = d_wal;
    a.wal_off = d_wal_off;
    a.wal_len = d_wal_len;
    a.nwal = nwal;
    a.max_len = max_wal_len;
    a.out = *out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(wal_seg_lanes_kernel, dim3(a.segs, nwal), dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(wal_stitch_kernel, dim3(nwal), dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(wal_compact_kernel, dim3(a.segs, nwal), dim3(256), 0, s, a);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}
