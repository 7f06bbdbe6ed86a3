// decode_core.h — the block chase as device templates (no kernel, no host
// code): shared by decode.hip, sstdec.hip and wal.hip.
//
// One wavefront owns one block or range.  It streams through a per-wave LDS
// ring of 1 KiB chunks, loaded by LDS-DMA (buffer_load_dwordx4 ... lds,
// range-checked so a block never reads past its padded end).  Record
// boundaries are a dependent chain (each position depends on every earlier
// length, data.go:58-76): the wave verifies 64 records at a time by
// speculative runs and chases the rest exactly on the VALU (decode_range_v2);
// a DESC block that fits the ring is landed in one burst and starts with one
// run from record 0 (decode_block_lin).  Descriptors leave as coalesced
// 16-byte stores; in ARENA mode the key and value bytes are gathered from the
// LDS ring into packed arenas with 16-byte stores (the bytes Go's
// make()+ReadFull produce).
#pragma once

#include "common.h"

namespace lsm {
namespace {

constexpr uint32_t kChunk = 1024;  // one b128 wave-load
constexpr uint32_t kRingChunks = 8;  // 8 KiB ring: 4 KiB blocks fit whole, 64 KiB stream
// Cache policy of the block loads: nt (streaming).  Each block byte is read
// once; keeping the stream out of the L2/MALL's normal replacement measured
// 80.5 -> 71.7 us for decode4k's memory pattern (tools/block_probe.py).
constexpr int kBlockLoadAux = 2;
// Per ring size (A/B on one box, wall GiB/s: resident / rotated copies / one
// 1M-block launch): the 8 KiB ring (4 KiB blocks) stores its descriptors nt
// too: 4,800 / 4,045 / 4,100 with plain stores, 4,836 / 4,800 / 4,650 with nt
// stores.  ARENA on the 8 KiB ring also loads the blocks with the default
// policy (2,150 -> 2,290 GiB/s).  The 16 KiB ring (64 KiB blocks) and the
// 2 KiB ring (mixed, scheduled) keep plain stores: nt stores measured 4,530
// -> 4,140 and 5,030 -> 4,850 GiB/s there.
// A launch of more than kBigLaunch blocks on the 8 KiB ring (gigabytes of
// input, far past the 256 MB MALL) loads its blocks with the default policy:
// 1M blocks 4,610 -> 5,030 GiB/s, 500k 4,835 -> 4,945; at 250k and below nt
// loads stay ahead (250k: 4,880 against 4,776; 100k, resident: 4,850 against
// 4,600).
constexpr uint32_t kBigLaunch = 400000;
template <uint32_t NCH, bool ARENA, bool BIG = false>
struct RingPolicy {
    static constexpr int load_aux = ((ARENA || BIG) && NCH == 8) ? 0 : kBlockLoadAux;
    static constexpr bool nt_desc = NCH == 8;
};
// LDS held beside the 8 KiB ring by the DESC kernel of a launch whose caller
// declared blocks of 3 KiB to the ring's size (lsm_decode_blocks_hinted): 12
// KiB per one-wave workgroup, 13 waves per CU instead of 19.  Measured, on one
// box (boxes differ by +-4%), config 2 with the straight-line path
// (decode_block_lin), resident / cold kernel us: 19 waves 83.3 / 83.9, 17:
// 81.0 / 81.9, 15: 76.6 / 78.3, 14: 75.9 / 78.2, 13: 75.0 / 74.3, 11: 79.8 /
// 78.8, 9: 83.6 / 84.4, 7: 102.0 / 102.7; the parent's general chase 78.1 /
// 79.1 at 19 waves, 90.3 / 88.5 at 13.  Inferred from these sweeps, not from a
// counter: a wave of the straight-line path waits for its block for nearly
// all its life, and 19 x 4 KiB streams per CU are more than HBM serves well.
// The pad is fitted to that block size: it loses on blocks of 1-3 KiB (1 KiB:
// 151.6 against 109.4 us), on streamed blocks (mixed sizes 130.4 against
// 114.5) and on IDX blocks (120.4 against 117.9), so only a declared bound
// selects it, and never for IDX.
constexpr uint32_t kFitPad = 4096;
constexpr uint32_t kFitMin = 3072;  // a bound above this (3 KiB blocks lose: 85.6 against 78.5 us)

template <uint32_t NCH, bool ARENA>
__device__ __forceinline__ void store_desc(u32x4 *p, const u32x4 &d) {
    if (RingPolicy<NCH, ARENA>::nt_desc)
        __builtin_nontemporal_store(d, p);
    else
        *p = d;
}


struct DecodeArgs {
    const uint8_t *in;
    const uint64_t *blk_off;
    const uint32_t *blk_len;
    uint32_t nblk;
    u32x4 *desc;
    const uint64_t *rec_base;
    uint32_t *nrec;
    int32_t *status;
    int64_t *idx_value;
    uint8_t *key_arena;
    uint8_t *val_arena;
    const uint64_t *arena_base;
    uint64_t *key_arena_off;
    uint64_t *val_arena_off;
    const uint32_t *order;  // launch order of the blocks (null: 0, 1, ..)
};

// Streams one block through this wave's LDS ring and serves u32 length
// fields at wave-uniform block positions.
//
// Ring: NCH x 1 KiB chunks, filled by LDS-DMA (buffer_load_dwordx4 ... lds:
// no VGPR staging), read by the chase with ds_read at block positions.
template <int N>
__device__ __forceinline__ void wait_vmcnt_le(uint32_t k) {
    // s_waitcnt takes an immediate: one arm per count (N <= 16).
#define LSM_VMW(i) case i: __asm__ __volatile__("s_waitcnt vmcnt(" #i ")" ::: "memory"); break;
    switch (k < N ? k : N - 1) {
    LSM_VMW(0) LSM_VMW(1) LSM_VMW(2) LSM_VMW(3) LSM_VMW(4) LSM_VMW(5) LSM_VMW(6) LSM_VMW(7)
    LSM_VMW(8) LSM_VMW(9) LSM_VMW(10) LSM_VMW(11) LSM_VMW(12) LSM_VMW(13) LSM_VMW(14)
    default: __asm__ __volatile__("s_waitcnt vmcnt(15)" ::: "memory"); break;
    }
#undef LSM_VMW
}

template <uint32_t NCH, int AUX = kBlockLoadAux>
struct BlockReaderT {
    uint32_t *ring;
    rsrc_t rsrc;
    uint32_t h;        // block start inside its first 16-byte line
    uint32_t total;    // loadable stream bytes: round_up16(h + n)
    uint32_t nchunks;  // chunks covering [0, total)
    uint32_t hi_c;     // chunks [.., hi_c) have been issued into the ring
    uint32_t landed;   // chunks [.., landed) are known to be in LDS

    __device__ void init(uint32_t *ring_, const uint8_t *in, uint64_t off, uint32_t n) {
        ring = ring_;
        uint64_t a0 = off & ~(uint64_t)15;
        h = (uint32_t)(off - a0);
        uint64_t tot = ((uint64_t)h + n + 15) & ~(uint64_t)15;
        total = (uint32_t)(tot > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : tot);
        nchunks = (total + kChunk - 1) / kChunk;
        rsrc = make_rsrc(in + a0, total);
        hi_c = 0;
        landed = 0;
    }

    // Make stream bytes [s0, s0 + want) resident (clamped to the block and
    // to the ring's reach from s0's chunk).  Every free ring slot is refilled,
    // but the wait is counted: only the chunks asked for must have landed, the
    // younger ones stay in flight while the chase runs.  vmcnt retires in
    // issue order across loads, stores and LDS-DMA, so descriptor stores
    // issued after a prefetch only make the count conservative.  (A plain
    // vmcnt(0) here streams a block larger than the ring at one HBM round
    // trip per refill.)
    __device__ __forceinline__ void ensure(uint32_t s0, uint32_t want = kChunk) {
        const uint32_t c0 = s0 / kChunk;
        // Top up: every slot whose chunk lies behind s0 is free; refill it now
        // (even when the bytes asked for are already resident), so a chunk is
        // issued NCH - 1 chunks before the chase reaches it.
        uint32_t last = c0 + NCH;
        if (last > nchunks) last = nchunks;
        if (last > hi_c) {
            const uint32_t voff = lane_id() * 16;
            for (uint32_t c = hi_c > c0 ? hi_c : c0; c < last; c++)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsrc, (__attribute__((address_space(3))) void *)&ring[(c % NCH) * (kChunk / 4)],
                    16, voff + c * kChunk, 0, 0, AUX);
            hi_c = last;
        }
        uint64_t need_end = (uint64_t)s0 + want;
        if (need_end > total) need_end = total;
        if (need_end > (uint64_t)last * kChunk) need_end = (uint64_t)last * kChunk;
        const uint32_t need_hi = (uint32_t)((need_end + kChunk - 1) / kChunk);
        if (need_hi <= landed) return;
        // The DMA writes are invisible to the compiler's waitcnt tracking of
        // ds_read; wait for them explicitly before any LDS read of them.
        wait_vmcnt_le<NCH>(hi_c - need_hi);
        landed = need_hi;
    }

};
template <int G>
struct MinRecord { static constexpr uint32_t R = G == LSM_GRAMMAR_V ? 4 : G == LSM_GRAMMAR_KV ? 8 : 12; };

// Record slots: CSR rec_base, or offset-addressed (rec_base == NULL): block b
// owns slots [off/R, (off+n)/R) with R the grammar's minimum record size,
// disjoint for non-overlapping blocks -- no scan needed.
template <int G>
__device__ __forceinline__ void record_slots(const DecodeArgs &a, uint32_t b, uint64_t off,
                                             uint32_t n, uint64_t &base, uint64_t &cap) {
    constexpr uint32_t R = MinRecord<G>::R;
    if (a.rec_base) {
        base = a.rec_base[b];
        cap = a.rec_base[b + 1] - base;
    } else {
        base = off / R;
        cap = (off + n) / R - base;
    }
}

// ---- v2: the chase with the fewest scalar instructions -------------------
//
// The exact step is a serial chain, and a wave-uniform chain runs on the CU's
// one scalar unit, shared by all resident waves: PMC on config 5 (record
// shapes vary, so speculative runs rarely verify) counted 107 SALU
// instructions per record for the round-0 wave-uniform step, 74% of the
// kernel time at one SALU issue per cycle.  v2 keeps the same semantics with
// a leaner step:
//  * one compare decides whether the bytes are landed (`lim`), the ring
//    bookkeeping only runs when a step crosses it;
//  * blocks that fit the ring are read without modulo arithmetic (LIN);
//  * the value length is read at the previous key length in the same LDS
//    round trip as the key length;
//  * descriptors are staged branch-free (v_cndmask) and stored 64 at a time;
//  * error statuses are only computed on the (one) failing record.
// Speculative runs: after an exact step of size S (key length K, value
// length V) all 64 lanes test "the next 64 records have the same K and V"
// straight from LDS; the ballot's count of leading successes is the verified
// run (each check reads the record's own fields, so the verified records are
// exactly the chase's), stored coalesced.
// A wave-uniform value moved into a VGPR, so the arithmetic that depends on
// it stays on the vector ALU (the compiler would otherwise keep a uniform
// chain on the CU's single scalar unit).
__device__ __forceinline__ uint32_t to_vgpr(uint32_t s) {
    uint32_t v;
    __asm__ __volatile__("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
    return v;
}

// ---- ARENA: key and value bytes gathered from the LDS ring -----------------
//
// kv.go:88-111 / data.go:68-75 hand back freshly allocated key and value
// slices; ARENA mode packs them per block, in record order, into a key arena
// and a value arena.  A batch of records (a verified run, or the <= 64 staged
// records of exact steps) occupies one contiguous range of each arena, so the
// copy is output-driven: each lane assembles one 16-byte output chunk from
// the record fields it covers (four funnel-shifted dwords, bytewise only
// where a record boundary falls inside a dword) and stores it whole.  Only a
// batch's first and last chunks, shared with the neighbouring batch or
// block, are written byte by byte.
template <uint32_t NCH, bool LIN>
struct RingBytes {
    const uint32_t *ring;
    rsrc_t rs;          // the block in global memory (stream byte = rsrc offset)
    uint32_t res_lo;    // stream bytes [res_lo, res_hi) are landed in the ring
    uint32_t res_hi;
    __device__ __forceinline__ uint32_t word(uint32_t w) const {
        return LIN ? ring[w] : ring[w % (NCH * kChunk / 4)];
    }
    // the ring dword at dword-aligned stream byte sb
    __device__ __forceinline__ uint32_t word_at(uint32_t sb) const {
        constexpr uint32_t kB = NCH * kChunk;
        return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(ring) +
                                                   (LIN ? sb : sb & (kB - 1)));
    }
    __device__ __forceinline__ uint32_t u32(uint32_t sb) const {
        return funnel(word(sb >> 2), word((sb >> 2) + 1), sb);
    }
    __device__ __forceinline__ uint32_t u8(uint32_t sb) const {
        return (word(sb >> 2) >> (8 * (sb & 3))) & 0xFFu;
    }
    // stream bytes [sb, sb + 16) from two aligned 16-byte LDS lines: two
    // ds_read_b128 (conflict-free when lanes take consecutive chunks; five
    // ds_read_b32 at a 16-byte lane stride are 4-way bank conflicts)
    __device__ __forceinline__ u32x4 u128(uint32_t sb) const {
        constexpr uint32_t kB = NCH * kChunk;
        const uint32_t a = sb & ~15u;
        const uint32_t i0 = (LIN ? a : a % kB) >> 2, i1 = (LIN ? a + 16 : (a + 16) % kB) >> 2;
        const u32x4 x = *reinterpret_cast<const u32x4 *>(&ring[i0]);
        const u32x4 y = *reinterpret_cast<const u32x4 *>(&ring[i1]);
        const uint32_t d = (sb >> 2) & 3;
        const uint32_t d0 = d == 0 ? x.x : d == 1 ? x.y : d == 2 ? x.z : x.w;
        const uint32_t d1 = d == 0 ? x.y : d == 1 ? x.z : d == 2 ? x.w : y.x;
        const uint32_t d2 = d == 0 ? x.z : d == 1 ? x.w : d == 2 ? y.x : y.y;
        const uint32_t d3 = d == 0 ? x.w : d == 1 ? y.x : d == 2 ? y.y : y.z;
        const uint32_t d4 = d == 0 ? y.x : d == 1 ? y.y : d == 2 ? y.z : y.w;
        return u32x4{funnel(d0, d1, sb), funnel(d1, d2, sb), funnel(d2, d3, sb),
                     funnel(d3, d4, sb)};
    }
    // a field not (wholly) in the ring: read through the caches
    __device__ __forceinline__ uint32_t g32(uint32_t sb) const {
        const uint32_t a = sb & ~3u;
        return funnel(ld_b32(rs, a), ld_b32(rs, a + 4), sb);
    }
    __device__ __forceinline__ uint32_t g8(uint32_t sb) const {
        return (ld_b32(rs, sb & ~3u) >> (8 * (sb & 3))) & 0xFFu;
    }
};

// Store 16 bytes at the 16-aligned dst; only bytes [lo, hi) are this batch's
// (a batch's first and last chunk share 16 bytes with its neighbours).  The
// arena streams are written once: every arena store is nt (A/B, config 2
// ARENA: 160-168 -> 145-146 us per launch).
__device__ __forceinline__ void store_chunk(uint8_t *dst, u32x4 v, int lo, int hi) {
    if (lo <= 0 && hi >= 16) {
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(dst));
        return;
    }
#pragma unroll 1
    for (int t = lo < 0 ? 0 : lo; t < (hi < 16 ? hi : 16); t++) {
        const uint32_t d = t < 4 ? v.x : t < 8 ? v.y : t < 12 ? v.z : v.w;
        dst[t] = (uint8_t)(d >> (8 * (t & 3)));
    }
}

__device__ __forceinline__ void set_dword(u32x4 &v, uint32_t j, uint32_t w) {
    v.x = j == 0 ? w : v.x;
    v.y = j == 1 ? w : v.y;
    v.z = j == 2 ? w : v.z;
    v.w = j == 3 ? w : v.w;
}

// A verified run: cnt records of stride S whose field of L bytes starts at
// ring stream byte src0 + i*S (all landed), packed to out[0, cnt*L).  One
// output dword per lane per step (consecutive lanes read consecutive ring
// dwords: no bank conflicts; 256-byte coalesced stores), with as few VALU
// operations per dword
// as the shape allows: the field index by one FMA (q / L rounded from
// q + 1/2, exact for q < 2^16), the second ring dword only where some lane's
// source is unaligned, the next field's bytes only where a field boundary
// falls inside some lane's dword (k < 4), bytes singly only in the run's
// first and last dword.  Ring reads are indexed modulo the ring, so lanes
// past the end read harmless bytes.
// a*b + c for a, b < 2^24 (full-rate v_mad_u32_u24; b wave-uniform)
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t d;
    __asm__("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(b), "v"(c));
    return d;
}

template <uint32_t NCH, bool LIN>
__device__ __forceinline__ void arena_emit_run(const RingBytes<NCH, LIN> &rb, uint8_t *out,
                                               uint32_t src0, uint32_t S, uint32_t L,
                                               uint32_t cnt) {
    const uint32_t T = cnt * L;  // <= the ring: a run lies inside the landed bytes
    if (T == 0) return;
    const uint32_t lane = lane_id();
    // full-rate 24-bit products (v_mul_u32_u24): every operand here is < 2^24
    auto mul24 = [](uint32_t x, uint32_t y) { return (x & 0xFFFFFFu) * (y & 0xFFFFFFu); };
    if (((src0 | S | L | (uint32_t)(uintptr_t)out) & 3) == 0) {
        // dword-aligned run: output dword j is ring byte src0 + 4j + r*(S-L)
        // with r = floor(j / (L/4)) -- one ring read and one store per dword.
        // The stores go through a buffer resource spanning exactly the run:
        // lanes past its end are dropped by the range check (no exec masks,
        // no 64-bit address arithmetic; the whole offset is in the VGPR).
        const uint32_t L4 = L >> 2, GB = S - L;
        // floor((j + 1/2) * rcp(L4)) is exact for j < 2^16: the quotient is at
        // least 1/(2 L4) from an integer, the error below 2^-6 / L4
        const float inv4 = __builtin_amdgcn_rcpf((float)L4), hinv4 = 0.5f * inv4;
        const rsrc_t os = make_rsrc(out, T);
        constexpr uint32_t V = 4;  // ring reads in flight per lane
#pragma unroll 1
        for (uint32_t b = 0; b < T; b += 4 * V * kWave) {  // wave-uniform output byte
            uint32_t v[V], o[V];
#pragma unroll
            for (uint32_t t = 0; t < V; t++) {  // past the run: harmless ring bytes
                const uint32_t j = (b >> 2) + t * kWave + lane;
                const uint32_t r = (uint32_t)__builtin_fmaf((float)j, inv4, hinv4);
                o[t] = 4 * j;
                v[t] = rb.word_at(mad_u24(r, GB, src0 + o[t]));
            }
#pragma unroll
            for (uint32_t t = 0; t < V; t++) __builtin_amdgcn_raw_buffer_store_b32(v[t], os, o[t], 0, 2);
        }
        return;
    }
    const uint32_t lead = (uint32_t)((uintptr_t)out & 3);
    uint32_t *a0 = reinterpret_cast<uint32_t *>(out - lead);
    const uint32_t nd = (lead + T + 3) >> 2;
    const float inv = 1.0f / (float)L, hinv = 0.5f * inv;  // once per run
    auto rec = [&](uint32_t q) -> uint32_t {  // floor(q / L), q < 2^16
        return (uint32_t)__builtin_fmaf((float)q, inv, hinv);
    };
    constexpr uint32_t U = 1;  // dwords per lane per step (2 and 4 measured no faster)
#pragma unroll 1
    for (uint32_t w0 = 0; w0 < nd; w0 += U * kWave) {
        uint32_t W[U], sb[U], kk[U], rr[U];
        int qv[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const int q = (int)(4 * (w0 + u * kWave + lane)) - (int)lead;
            const uint32_t qc = q < 0 ? 0u : (uint32_t)q;
            const uint32_t r = rec(qc), o = qc - mul24(r, L);
            qv[u] = q;
            rr[u] = r;
            kk[u] = L - o;
            sb[u] = src0 + mul24(r, S) + o;
            W[u] = rb.word(sb[u] >> 2);
        }
        bool unal = false, cross = false;
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            unal |= (sb[u] & 3) != 0;
            cross |= kk[u] < 4;
        }
        if (__ballot(unal)) {
#pragma unroll
            for (uint32_t u = 0; u < U; u++) W[u] = funnel(W[u], rb.word((sb[u] >> 2) + 1), sb[u]);
        }
        if (L < 4) {  // fields of 0-3 bytes: byte by byte
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t qc = qv[u] < 0 ? 0u : (uint32_t)qv[u];
                uint32_t x = 0;
                for (uint32_t t = 0; t < 4; t++) {
                    const uint32_t qq = qc + t;
                    if (qq < T) {
                        const uint32_t r = rec(qq);
                        x |= rb.u8(src0 + mul24(r, S) + (qq - mul24(r, L))) << (8 * t);
                    }
                }
                W[u] = x;
            }
        } else if (__ballot(cross)) {  // a field boundary inside some lane's dword
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t B = rb.u32(src0 + mul24(rr[u] + 1, S)), k = kk[u];
                W[u] = k < 4 ? (W[u] & ((1u << (8 * k)) - 1)) | (B << (8 * k)) : W[u];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t w = w0 + u * kWave + lane;
            const int q = qv[u];
            if (q >= 0 && (uint32_t)q + 4 <= T) {
                __builtin_nontemporal_store(W[u], &a0[w]);
            } else if (w < nd) {  // the run's first or last dword, shared with its neighbours
                const uint32_t sh = q < 0 ? (uint32_t)(-q) : 0u;  // bytes before the run
                uint8_t *b = reinterpret_cast<uint8_t *>(a0 + w);
                for (uint32_t t = sh; t < 4 && (uint32_t)(q + (int)t) < T; t++)
                    b[t] = (uint8_t)(W[u] >> (8 * (t - sh)));
            }
        }
    }
}

// A staged batch: lane l < cnt holds a record field of len bytes at ring
// stream byte src; the fields are packed in lane order to out[0, T).  A field
// wholly landed in the ring is read from LDS, any other (a value longer than
// the ring) through the caches.  tab: 129 dwords of LDS.  Returns T.
template <uint32_t NCH, bool LIN>
__device__ __forceinline__ uint32_t arena_emit_batch(const RingBytes<NCH, LIN> &rb, uint32_t *tab,
                                                     uint8_t *out, uint32_t cnt, uint32_t src,
                                                     uint32_t len, uint64_t *out_off,
                                                     uint64_t cur) {
    const uint32_t lane = lane_id();
    const uint32_t l = lane < cnt ? len : 0u;
    uint32_t T;
    const uint32_t start = wave_excl_scan(l, &T);
    if (out_off && lane < cnt) out_off[lane] = cur + start;
    if (T == 0) return 0;
    uint32_t *tstart = tab, *tsrc = tab + 65;
    if (lane < cnt) {
        tstart[lane] = start;
        tsrc[lane] = src;
    }
    if (lane == 0) tstart[cnt] = T;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t lead = (uint32_t)((uintptr_t)out & 15);
    uint8_t *a0 = out - lead;
    const uint32_t nch = (lead + T + 15) >> 4;
#pragma unroll 1
    for (uint32_t c = lane; c < nch; c += kWave) {
        const int q0 = (int)(16 * c) - (int)lead;
        const uint32_t qf = q0 < 0 ? 0u : (uint32_t)q0;
        // the last record whose packed range starts at or before qf
        uint32_t lo = 0, hi = cnt;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tstart[mid] <= qf) lo = mid;
            else hi = mid;
        }
        uint32_t r = lo, rs0 = tstart[r], rs1 = tstart[r + 1], rsrc = tsrc[r];
        auto in_ring = [&]() { return rsrc >= rb.res_lo && rsrc + (rs1 - rs0) <= rb.res_hi; };
        auto seek = [&](uint32_t q) {  // advance r to the record holding byte q
            while (rs1 <= q) {
                r++;
                rs0 = rs1;
                rs1 = tstart[r + 1];
                rsrc = tsrc[r];
            }
        };
        auto byte_at = [&](uint32_t q) -> uint32_t {
            seek(q);
            const uint32_t sb = rsrc + (q - rs0);
            return in_ring() ? rb.u8(sb) : rb.g8(sb);
        };
        u32x4 v{0, 0, 0, 0};
        if (q0 >= 0 && q0 + 16 <= (int)T && (uint32_t)q0 + 16 <= rs1) {
            // the chunk lies in one field
            const uint32_t sb = rsrc + ((uint32_t)q0 - rs0);
            if (in_ring())
                v = rb.u128(sb);
            else
                v = u32x4{rb.g32(sb), rb.g32(sb + 4), rb.g32(sb + 8), rb.g32(sb + 12)};
        } else {
#pragma unroll 1
            for (int t = 0; t < 16; t++) {
                const int q = q0 + t;
                if (q >= 0 && q < (int)T) {
                    const uint32_t b = byte_at((uint32_t)q) << (8 * (t & 3));
                    set_dword(v, (uint32_t)t >> 2, (t < 4 ? v.x : t < 8 ? v.y : t < 12 ? v.z : v.w) | b);
                }
            }
        }
        store_chunk(a0 + 16 * c, v, -q0, (int)T - q0);
    }
    // the table is rewritten by the next batch: all reads done first
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return T;
}

typedef __attribute__((address_space(3))) uint32_t lds_u32_t;

// arena_emit_batch as one out-of-line call per batch: a staged flush has
// several call sites in the chase, and inlining each multiplies the live
// registers of the whole kernel.  The LDS pointers keep their address space
// (ds_read, not flat loads).
template <uint32_t NCH, bool LIN>
__device__ __forceinline__ uint32_t arena_emit_batch_call(lds_u32_t *ring, rsrc_t rs, uint32_t res_lo,
                                                       uint32_t res_hi, lds_u32_t *tab,
                                                       uint8_t *out, uint32_t cnt, uint32_t src,
                                                       uint32_t len, uint64_t *out_off,
                                                       uint64_t cur) {
    RingBytes<NCH, LIN> rb{(const uint32_t *)ring, rs, res_lo, res_hi};
    return arena_emit_batch(rb, (uint32_t *)tab, out, cnt, src, len, out_off, cur);
}

// Arena cursors of one block (ARENA mode): the next free byte of each arena.
struct ArenaCur {
    uint64_t k, v;
};

// Decode the byte range [off, off + n) of a.in as one block whose records
// go to slots base.. (capacity ncap); returns the record count, the status
// and the position where the chase stopped.  Records that start at or past
// `stop` are not decoded (a clean stop; stop = n decodes the whole range).
// ARENA: keys and values are also packed into a.key_arena / a.val_arena from
// the cursors `ac` (tab: the 129-dword LDS table of arena_emit_batch).
// Where a chase goes on after records verified elsewhere: record nr at block
// position pos, kprev the last key length (none: 0xFFFFFFFF).
struct ChaseResume {
    uint32_t pos = 0, nr = 0, kprev = 0xFFFFFFFFu;
};
// PRE: the caller (decode_block_lin) has landed the whole block in the ring
// and verified the records before rs0.pos: the chase goes on there and loads
// nothing (the reader only supplies the block's descriptor and start).
template <int G, uint32_t NCH, bool LIN, bool ARENA = false, bool BIG = false, bool PRE = false>
__device__ void decode_range_v2(const DecodeArgs &a, uint32_t *ring, uint64_t off, uint32_t n,
                                uint64_t base, uint32_t ncap, uint32_t &nr_out, int32_t &st_out,
                                uint32_t stop, uint32_t &pos_out, ArenaCur ac = {},
                                uint32_t *tab = nullptr, bool lin_rt = LIN,
                                const ChaseResume rs0 = {}) {
    static_assert(!PRE || (LIN && !ARENA), "a pre-landed ring is a DESC block that fits it");
    // the block fits the ring (read linearly, landed whole at the first
    // step): a template constant, or for ARENA a runtime flag (the ring is
    // then always indexed modulo its size, which is the same for such blocks)
    const bool lin = ARENA ? lin_rt : LIN;
    const uint32_t lane = lane_id();
    BlockReaderT<NCH, RingPolicy<NCH, ARENA, BIG>::load_aux> rd;
    rd.init(ring, a.in, off, n);
    RingBytes<NCH, LIN> rb{ring, rd.rsrc, 0, 0};

    auto word = [&](uint32_t w) -> uint32_t { return rb.word(w); };
    auto fld = [&](uint32_t p) -> uint32_t {  // wave-uniform u32 at block position p
        return uni(rb.u32(rd.h + p));
    };
    auto lds_u32 = [&](uint32_t p) -> uint32_t {  // per-lane u32 at block position p
        return rb.u32(rd.h + p);
    };

    uint32_t s_pos = 0, s_k = 0, s_v = 0, s_xlo = 0, s_xhi = 0, ns = 0, s_first = 0;
    // (a resumed chase starts its back-off afresh, miss = skip = 0, where the
    // chase from record 0 would carry skip = 1 after a failed first run: the
    // heuristic only picks which step verifies a record, never the result)
    uint32_t pos = rs0.pos, nr = rs0.nr, kprev = rs0.kprev, miss = 0, skip = 0;
    // ARENA: the exact step's record (the last staged one) leaves its arena
    // bytes together with the run that follows it (same K, V, stride)
    uint32_t pend = 0, pend_pos = 0, pend_k = 0, pend_v = 0;
    auto emit_run_arena = [&](uint32_t p0, uint32_t K, uint32_t V, uint32_t S, uint32_t cnt,
                              uint64_t slot0) {
        // keys, then values: one emitter body serves both arenas
#pragma unroll 1
        for (uint32_t f = G == LSM_GRAMMAR_V ? 1u : 0u; f < (G == LSM_GRAMMAR_IDX ? 1u : 2u);
             f++) {
            uint8_t *ar = f ? a.val_arena : a.key_arena;
            if (!ar) continue;
            uint64_t *ao = f ? a.val_arena_off : a.key_arena_off;
            const uint64_t cur = f ? ac.v : ac.k;
            const uint32_t L = f ? V : K;
            arena_emit_run(rb, ar + cur, rd.h + p0 + (f == 0 ? 4u : G == LSM_GRAMMAR_KV ? 8 + K : 4u),
                           S, L, cnt);
            if (ao)  // cnt <= 65: the pending record + a full run
                for (uint32_t i = lane; i < cnt; i += kWave) ao[slot0 + i] = cur + (uint64_t)i * L;
            if (f) ac.v += (uint64_t)cnt * L;
            else ac.k += (uint64_t)cnt * L;
        }
    };
    auto flush = [&]() {
        if (ns) {
            if (lane < ns) {
                const uint64_t ro = off + s_pos;
                u32x4 d;
                d.x = (uint32_t)ro;
                d.y = (uint32_t)(ro >> 32);
                d.z = s_k;
                d.w = s_v;
                store_desc<NCH, ARENA>(&a.desc[base + s_first + lane], d);
                if (G == LSM_GRAMMAR_IDX && a.idx_value)
                    a.idx_value[base + s_first + lane] = (int64_t)((uint64_t)s_xhi << 32 | s_xlo);
            }
            if (ARENA && ns > pend) {  // (the pending record leaves with its run)
                lds_u32_t *lring = (lds_u32_t *)ring, *ltab = (lds_u32_t *)tab;
                // keys, then values: one emitter body serves both arenas
#pragma unroll 1
                for (uint32_t f = G == LSM_GRAMMAR_V ? 1u : 0u;
                     f < (G == LSM_GRAMMAR_IDX ? 1u : 2u); f++) {
                    uint8_t *ar = f ? a.val_arena : a.key_arena;
                    if (!ar) continue;
                    uint64_t *ao = f ? a.val_arena_off : a.key_arena_off;
                    const uint64_t cur = f ? ac.v : ac.k;
                    const uint32_t src =
                        rd.h + s_pos + (f == 0 ? 4u : G == LSM_GRAMMAR_KV ? 8 + s_k : 4u);
                    const uint32_t t = arena_emit_batch_call<NCH, LIN>(
                        lring, rb.rs, rb.res_lo, rb.res_hi, ltab, ar + cur, ns - pend, src,
                        f ? s_v : s_k, ao ? ao + base + s_first : nullptr, cur);
                    if (f) ac.v += t;
                    else ac.k += t;
                }
            }
            ns = 0;
        }
    };
    // Block bytes below `lim` (and at or above the last anchor) are landed.
    uint32_t lim = PRE ? n : 0;
    auto need = [&](uint32_t p, uint32_t len) {
        if (PRE || (uint64_t)p + len <= lim) return;
        // a streamed block recycles ring chunks: the staged records' arena
        // bytes leave first
        if (ARENA && !lin) {
            flush();
            if (pend) {
                emit_run_arena(pend_pos, pend_k, pend_v, 0, 1, base + nr - 1);
                pend = 0;
            }
        }
        rd.ensure(rd.h + p, lin ? rd.total : len);
        lim = rd.landed >= rd.nchunks ? n : rd.landed * kChunk - rd.h;
        if (ARENA) {
            rb.res_lo = (rd.hi_c > NCH ? rd.hi_c - NCH : 0u) * kChunk;
            rb.res_hi = rd.landed * kChunk;
        }
    };

    int32_t status = LSM_OK;
    for (;;) {
        // ---- exact step at pos (same checks and order as the reference) ----
        const uint32_t rem = n - pos;
        if (rem == 0 || pos >= stop) break;
        if (rem < 4) {
            status = G == LSM_GRAMMAR_IDX ? LSM_ST_IDX_OVERRUN : LSM_ST_TRUNC_LEN_PREFIX;
            break;
        }
        need(pos, rem < kChunk ? rem : kChunk);
        uint32_t K = 0, V, S;
        uint64_t x = 0;
        if (G == LSM_GRAMMAR_V) {
            V = fld(pos);  // data.go:58-76
            if (rem - 4 < V) { status = LSM_ST_TRUNC_VAL; break; }
            S = 4 + V;
        } else if (G == LSM_GRAMMAR_KV) {
            // kv.go:77-115; the guess at kprev lies inside the landed KiB
            const bool sv = kprev <= kChunk - 8;
            K = fld(pos);
            const uint32_t vg = sv ? fld(pos + 4 + kprev) : 0u;
            if (K > kKeyCap) { status = LSM_ST_KEY_TOO_LONG; break; }
            if (rem - 4 < K) { status = LSM_ST_TRUNC_KEY; break; }
            const uint32_t vp = pos + 4 + K;
            const uint32_t rem2 = n - vp;
            if (rem2 < 4) { status = LSM_ST_TRUNC_VLEN; break; }
            if (sv && K == kprev) {
                V = vg;
            } else {
                need(vp, rem2 < kChunk ? rem2 : kChunk);
                V = fld(vp);
            }
            if (V > kValCap) { status = LSM_ST_VAL_TOO_LONG; break; }
            if (rem2 - 4 < V) { status = LSM_ST_TRUNC_VAL; break; }
            kprev = K;
            S = 8 + K + V;
        } else {
            K = fld(pos);  // index.go:70-98
            if ((uint64_t)rem < 12ull + K) { status = LSM_ST_IDX_OVERRUN; break; }
            const uint32_t vp = pos + 4 + K;
            need(vp, 8);
            x = (uint64_t)fld(vp + 4) << 32 | fld(vp);
            V = 8;
            S = 12 + K;
        }
        if (nr >= ncap) { status = LSM_ST_CAPACITY; break; }
        if (ns == 0) s_first = nr;
        {
            const bool me = lane == ns;
            s_pos = me ? pos : s_pos;
            s_k = me ? K : s_k;
            s_v = me ? V : s_v;
            if (G == LSM_GRAMMAR_IDX) {
                s_xlo = me ? (uint32_t)x : s_xlo;
                s_xhi = me ? (uint32_t)(x >> 32) : s_xhi;
            }
        }
        if (++ns == kWave) flush();
        nr++;
        pos += S;

        // ---- records of varying shape: the VALU chain ----
        // After a failed run (skip > 0) the following records are chased with
        // the cursor in a VGPR: all lanes compute the same step, the checks
        // combine into one ballot and the scalar unit only counts.  The step
        // guesses the previous record's key length and reads the value length
        // there in the same LDS round trip (re-read when the key length
        // differs); any record it cannot vouch for (a key over 1 KiB, bytes
        // not yet landed, an error, the block end, capacity) drops back to the
        // exact step above.
        if (skip) {
            skip--;
            if (G == LSM_GRAMMAR_KV && kprev <= kChunk - 8) {
                uint32_t vpos = to_vgpr(pos), kp = to_vgpr(kprev);
                while (nr < ncap) {
                    const uint32_t sb = rd.h + vpos, sv = sb + 4 + kp;
                    const uint32_t k = funnel(word(sb >> 2), word((sb >> 2) + 1), sb);
                    uint32_t v = funnel(word(sv >> 2), word((sv >> 2) + 1), sv);
                    // a key of another length: the value length is elsewhere
                    // (one more LDS round trip, still on the vector ALU)
                    if (!__ballot(k == kp) && __ballot(k <= kChunk - 8)) {
                        const uint32_t sw = sb + 4 + k;
                        v = funnel(word(sw >> 2), word((sw >> 2) + 1), sw);
                    }
                    const uint32_t rem = n - vpos;
                    const bool ok = (k <= kChunk - 8) & (vpos <= lim) & (lim - vpos >= 8 + k) &
                                    (v <= kValCap) & (rem - 8 - k >= v) & (vpos < stop);
                    if (!__ballot(ok)) break;
                    if (ns == 0) s_first = nr;
                    const bool me = lane == ns;
                    s_pos = me ? vpos : s_pos;
                    s_k = me ? k : s_k;
                    s_v = me ? v : s_v;
                    if (++ns == kWave) flush();
                    nr++;
                    vpos += 8 + k + v;
                    kp = k;
                }
                pos = uni(vpos);
                kprev = uni(kp);
            } else if (G == LSM_GRAMMAR_V) {
                uint32_t vpos = to_vgpr(pos);
                while (nr < ncap) {
                    const uint32_t sb = rd.h + vpos;
                    const uint32_t v = funnel(word(sb >> 2), word((sb >> 2) + 1), sb);
                    const uint32_t rem = n - vpos;
                    const bool ok = (vpos <= lim) & (lim - vpos >= 4u) & (rem - 4 >= v) &
                                    (vpos < stop);
                    if (!__ballot(ok)) break;
                    if (ns == 0) s_first = nr;
                    const bool me = lane == ns;
                    s_pos = me ? vpos : s_pos;
                    s_k = me ? 0u : s_k;
                    s_v = me ? v : s_v;
                    if (++ns == kWave) flush();
                    nr++;
                    vpos += 4 + v;
                }
                pos = uni(vpos);
            }
            continue;
        }
        // the exact record is still staged (not flushed as a 64th) and wholly
        // in the ring (landed, and its start not recycled by the value-length
        // refill of a streamed block)
        if (ARENA && ns > 0 && pos <= lim && rd.h + pos - S >= rb.res_lo) {
            pend = 1;
            pend_pos = pos - S;
            pend_k = K;
            pend_v = V;
        }
        flush();
        for (bool first = true;; first = false) {
            if (pos >= n) break;
            // wait for the span the run can verify (64 records): all of a
            // block that fits the ring, half the ring otherwise (the other
            // half stays in flight while the run is checked)
            const uint32_t span_max = (lin ? NCH : NCH / 2) * kChunk;
            const uint64_t span = (uint64_t)S * kWave + 8;
            const uint32_t want = span < span_max ? (uint32_t)span : span_max;
            need(pos, n - pos < want ? n - pos : want);
            const uint64_t pe = (uint64_t)pos + (uint64_t)(lane + 1) * S;  // record end
            const uint32_t p = pos + lane * S;
            bool ok = pe <= lim && nr + lane < ncap && p < stop;
            uint64_t xx = 0;
            if (ok) {
                if (G == LSM_GRAMMAR_V) {
                    ok = lds_u32(p) == V;
                } else if (G == LSM_GRAMMAR_KV) {
                    ok = (int)(lds_u32(p) == K) & (int)(lds_u32(p + 4 + K) == V);
                } else {
                    ok = lds_u32(p) == K;
                    xx = (uint64_t)lds_u32(p + 8 + K) << 32 | lds_u32(p + 4 + K);
                }
            }
            const uint64_t m = __ballot(ok);
            const uint32_t j = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
            if (lane < j) {
                const uint64_t ro = off + p;
                u32x4 d;
                d.x = (uint32_t)ro;
                d.y = (uint32_t)(ro >> 32);
                d.z = K;
                d.w = V;
                store_desc<NCH, ARENA>(&a.desc[base + nr + lane], d);
                if (G == LSM_GRAMMAR_IDX && a.idx_value) a.idx_value[base + nr + lane] = (int64_t)xx;
            }
            if (ARENA && j + pend) {
                // the run's fields (and the pending exact record's, S bytes
                // before it) are landed: straight from the ring
                emit_run_arena(pos - pend * S, K, V, S, j + pend, base + nr - pend);
                pend = 0;
            }
            // the run ended at the landed limit, not at a mismatch
            const bool at_lim = j == 64 || (uint64_t)pos + (uint64_t)(j + 1) * S > lim;
            nr += j;
            pos += j * S;
            if (first) {
                if (j == 0) {
                    miss = miss < 4 ? miss + 1 : 4;
                    skip = (1u << miss) - 1;
                } else {
                    miss = 0;
                }
            }
            // a run cut short by the landed limit goes on once more bytes
            // have landed (no exact step in between); a mismatch ends it
            if (j < 64 && !(at_lim && j > 0)) break;
        }
        if (ARENA && pend) {  // no run followed (the block ended)
            emit_run_arena(pend_pos, pend_k, pend_v, 0, 1, base + nr - 1);
            pend = 0;
        }
    }
    flush();
    nr_out = nr;
    st_out = status;
    pos_out = pos;
}

template <int G, uint32_t NCH, bool LIN, bool ARENA, bool BIG = false>
__device__ void decode_block_v2(const DecodeArgs &a, uint32_t b, uint32_t *ring, uint32_t *tab,
                                uint64_t off, uint32_t n, bool lin_rt = LIN) {
    uint64_t base, cap;
    record_slots<G>(a, b, off, n, base, cap);
    uint32_t nr, end;
    int32_t st;
    ArenaCur ac{};
    if (ARENA) {  // A(b): arena_base[b], or offset-addressed arenas
        ac.k = a.arena_base ? uni64(a.arena_base[b]) : off;
        ac.v = ac.k;
    }
    decode_range_v2<G, NCH, LIN, ARENA, BIG>(a, ring, off, n, uni64(base),
                                        uni(cap < 0xFFFFFFFFull ? (uint32_t)cap : 0xFFFFFFFFu), nr,
                                        st, n, end, ac, tab, lin_rt);
    if (lane_id() == 0) {
        a.nrec[b] = nr;
        a.status[b] = st;
    }
}

// ---- DESC blocks that fit the ring: the straight-line path -----------------
//
// A block with round_up16(h + n) <= ring needs none of the ring's
// bookkeeping: every chunk's LDS-DMA is issued in one unrolled burst, one
// vmcnt(0) lands the block, and record 0's fields are read once.  Lane i then
// tests the record at i * S against record 0's (K, V) straight from LDS (lane
// 0 is record 0 itself); one ballot gives the verified count j, one store
// covers the descriptors of records 0..j-1 (config 2: one 528-byte nt store
// per block, the block's first 128-byte descriptor line written whole).  A
// run that ends at n finishes the block there.  Anything else (a record 0
// that fails a check, a mismatch, a run of 64, a truncated tail, capacity)
// goes on in the general chase at the first unverified record with the ring
// as landed (PRE): the statuses and the records are the exact step's.
//
// Record 0 passes the reference's checks (kv.go:77-115, data.go:58-76,
// index.go:70-98) exactly when its fields end inside the block: n is at most
// the ring, far below kKeyCap and kValCap, so the two cap checks cannot fail
// on a record that fits.

template <int G, uint32_t NCH, bool BIG>
__device__ __forceinline__ void decode_block_lin(const DecodeArgs &a, uint32_t b, uint32_t *ring,
                                                 uint64_t off, uint32_t n) {
    static_assert(NCH * kChunk <= kKeyCap && NCH * kChunk <= kValCap, "caps hold for a block that fits");
    constexpr int AUX = RingPolicy<NCH, false, BIG>::load_aux;
    constexpr uint32_t R = MinRecord<G>::R;
    const uint32_t lane = lane_id();
    const uint32_t h = (uint32_t)off & 15;
    const uint32_t total = (h + n + 15) & ~15u;  // <= NCH * kChunk
    const uint32_t nchunks = (total + kChunk - 1) / kChunk;
    const rsrc_t rsrc = make_rsrc(a.in + (off - h), total);
    const uint32_t voff = lane * 16;
#pragma unroll
    for (uint32_t c = 0; c < NCH; c++)
        if (c < nchunks)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsrc, (__attribute__((address_space(3))) void *)&ring[c * (kChunk / 4)], 16,
                voff + c * kChunk, 0, 0, AUX);
    uint64_t base64, cap64;
    record_slots<G>(a, b, off, n, base64, cap64);
    const uint64_t base = uni64(base64);
    const uint32_t ncap = uni(cap64 < 0xFFFFFFFFull ? (uint32_t)cap64 : 0xFFFFFFFFu);
    // The DMA writes are invisible to the compiler's waitcnt tracking of
    // ds_read; wait for them explicitly before any LDS read of them.
    __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");
    const RingBytes<NCH, true> rb{ring, rsrc, 0, 0};
    uint32_t pos = 0, nr = 0, K = 0, V = 8;
    if (n >= R) {
        bool ok0;
        if (G == LSM_GRAMMAR_V) {
            V = uni(rb.u32(h));
            ok0 = V <= n - 4;
        } else if (G == LSM_GRAMMAR_KV) {
            K = uni(rb.u32(h));
            ok0 = K <= n - 8;
            if (ok0) {
                V = uni(rb.u32(h + 4 + K));
                ok0 = V <= n - 8 - K;
            }
        } else {
            K = uni(rb.u32(h));
            ok0 = K <= n - 12;
        }
        if (ok0) {
            const uint32_t S = G == LSM_GRAMMAR_V ? 4 + V : G == LSM_GRAMMAR_KV ? 8 + K + V : 12 + K;
            const uint32_t p = lane * S;  // S <= n <= 16 KiB: no overflow
            bool ok = p + S <= n && lane < ncap;
            uint64_t xx = 0;
            if (ok) {
                if (G == LSM_GRAMMAR_V) {
                    ok = rb.u32(h + p) == V;
                } else if (G == LSM_GRAMMAR_KV) {
                    ok = (int)(rb.u32(h + p) == K) & (int)(rb.u32(h + p + 4 + K) == V);
                } else {
                    ok = rb.u32(h + p) == K;
                    xx = (uint64_t)rb.u32(h + p + 8 + K) << 32 | rb.u32(h + p + 4 + K);
                }
            }
            const uint64_t m = __ballot(ok);
            const uint32_t j = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
            if (lane < j) {
                const uint64_t ro = off + p;
                u32x4 d;
                d.x = (uint32_t)ro;
                d.y = (uint32_t)(ro >> 32);
                d.z = K;
                d.w = V;
                store_desc<NCH, false>(&a.desc[base + lane], d);
                if (G == LSM_GRAMMAR_IDX && a.idx_value) a.idx_value[base + lane] = (int64_t)xx;
            }
            nr = j;
            pos = j * S;
        }
    }
    int32_t st = LSM_OK;
    if (pos != n) {
        uint32_t end;
        decode_range_v2<G, NCH, true, false, BIG, true>(
            a, ring, off, n, base, ncap, nr, st, n, end, {}, nullptr, true,
            ChaseResume{pos, nr, G == LSM_GRAMMAR_KV && nr ? K : 0xFFFFFFFFu});
    }
    if (lane == 0) {
        a.nrec[b] = nr;
        a.status[b] = st;
    }
}

// Either form of the range decoder: linear when the range fits the ring.
template <int G, uint32_t NCH>
__device__ void decode_range_any(const DecodeArgs &a, uint32_t *ring, uint64_t off, uint32_t n,
                                 uint64_t base, uint32_t ncap, uint32_t &nr, int32_t &st,
                                 uint32_t stop = 0xFFFFFFFFu, uint32_t *end = nullptr) {
    uint32_t e;
    if (((off & 15) + (uint64_t)n + 15) / 16 * 16 <= NCH * kChunk)
        decode_range_v2<G, NCH, true>(a, ring, off, n, base, ncap, nr, st, stop, e);
    else
        decode_range_v2<G, NCH, false>(a, ring, off, n, base, ncap, nr, st, stop, e);
    if (end) *end = e;
}

}  // namespace
}  // namespace lsm
