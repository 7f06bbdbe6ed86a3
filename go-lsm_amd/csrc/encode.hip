// encode.hip — batched record encode, fused-bloom .sst build and bloom probe (gfx950).
//
// Encoding is output-centric.  With a CSR record batch every record's output
// position is closed-form (KV: 8*i + K(i) + V(i), V: 4*i + V(i), IDX:
// 12*i + K(i), relative to the region's first record), which is exactly
// SSTable.EncodeTo's exclusive prefix sum of 4+len (sstable.go:164-175)
// without a scan.  A wave takes a chunk of up to 64 records (one per lane,
// positions by a wave prefix sum), then every lane assembles whole aligned
// output dwords: the common dword lies inside one key/value and is two
// aligned source loads + v_alignbyte; dwords that straddle a length field
// are assembled byte by byte.  Chunk-edge dwords shared with a neighbour
// chunk are written with byte stores, everything else with dword stores.
//
// The bloom filter (1.6 Mbit in go-lsm) does not fit one CU's LDS, so each
// .sst's bitmap is built in LDS slices: one workgroup per (file, slice)
// hashes every key of the file (sum256 + 16 locations + Barrett modulo) and
// ds_or's the bits that fall in its slice; the slice is then stored once.
// No global atomics.
#include <stdlib.h>

#include "common.h"
#include "murmur.h"

namespace lsm {
namespace {

struct RegionSrc {
    const uint8_t *keys;
    const uint64_t *koff;
    const uint8_t *vals;
    const uint64_t *voff;
    const int64_t *idx_off;  // IDX: per-record offsets (encode_blocks) or null
    int64_t idx_base;        // IDX (.sst): offset(i) = idx_base + 4*(i-rs) + V(i)-V(rs)
    uint64_t rs, vrs;
};

template <int G>
struct GrammarTraits;
template <>
struct GrammarTraits<LSM_GRAMMAR_V> { static constexpr uint32_t pre = 4; static constexpr bool K = false, V = true; };
template <>
struct GrammarTraits<LSM_GRAMMAR_KV> { static constexpr uint32_t pre = 8; static constexpr bool K = true, V = true; };
template <>
struct GrammarTraits<LSM_GRAMMAR_IDX> { static constexpr uint32_t pre = 12; static constexpr bool K = true, V = false; };

// Byte w of a record (w < record size).
template <int G>
__device__ __forceinline__ uint32_t rec_byte(const RegionSrc &S, uint64_t K0, uint32_t kl,
                                             uint64_t V0, uint32_t vl, int64_t xo, uint64_t w) {
    if (G == LSM_GRAMMAR_V) {
        if (w < 4) return (vl >> (8 * w)) & 0xff;
        return S.vals[V0 + w - 4];
    }
    if (w < 4) return (kl >> (8 * w)) & 0xff;
    if (w < 4 + (uint64_t)kl) return S.keys[K0 + w - 4];
    uint64_t w2 = w - 4 - kl;
    if (G == LSM_GRAMMAR_IDX) return (uint32_t)((uint64_t)xo >> (8 * w2)) & 0xff;
    if (w2 < 4) return (vl >> (8 * w2)) & 0xff;
    return S.vals[V0 + w2 - 4];
}

// Per-wave record table of one chunk (LDS).
struct ChunkTable {
    uint64_t P[kWave + 1];  // chunk-relative record starts; P[cnt] = chunk bytes
    uint64_t K0[kWave], V0[kWave];
    int64_t xo[kWave];
    uint32_t kl[kWave], vl[kWave];
};

// Encode records [c0, c0+cnt) (cnt <= 64) whose first byte goes to dst.
template <int G>
__device__ void encode_chunk(const RegionSrc &S, uint64_t c0, uint32_t cnt, uint8_t *dst,
                             ChunkTable *tb) {
    using T = GrammarTraits<G>;
    const uint32_t lane = lane_id();
    uint64_t K0 = 0, V0 = 0;
    uint32_t kl = 0, vl = 0;
    int64_t xo = 0;
    uint64_t sz = 0;
    if (lane < cnt) {
        uint64_t i = c0 + lane;
        if (T::K) { K0 = S.koff[i]; kl = (uint32_t)(S.koff[i + 1] - K0); }
        if (T::V || (G == LSM_GRAMMAR_IDX && !S.idx_off)) {
            V0 = S.voff[i];
            vl = (uint32_t)(S.voff[i + 1] - V0);
        }
        if (G == LSM_GRAMMAR_IDX)
            xo = S.idx_off ? S.idx_off[i]
                           : S.idx_base + (int64_t)(4 * (i - S.rs) + (V0 - S.vrs));
        sz = T::pre + (T::K ? kl : 0) + (T::V ? vl : 0);
    }
    uint64_t tot;
    const uint64_t P = wave_excl_scan64(sz, &tot);
    // Publish the table; a previous chunk's readers in this wave are done
    // (LDS ops of one wave execute in order).
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    if (lane < cnt) {
        tb->P[lane] = P;
        tb->K0[lane] = K0;
        tb->V0[lane] = V0;
        tb->xo[lane] = xo;
        tb->kl[lane] = kl;
        tb->vl[lane] = vl;
    }
    if (lane == 0) tb->P[cnt] = tot;
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");

    const uintptr_t Ob = reinterpret_cast<uintptr_t>(dst);
    const uint32_t head = (uint32_t)(Ob & 3);
    gptr_t<uint32_t> dA = gbl_at<uint32_t>(Ob - head);
    const uint64_t ndw = (head + tot + 3) >> 2;

    uint32_t r = 0;             // this lane's record cursor
    uint64_t Pn = tb->P[1 <= cnt ? 1 : 0];  // start of record r+1
    for (uint64_t d = lane; d < ndw; d += kWave) {
        const int64_t u0 = (int64_t)(4 * d) - head;
        const uint64_t uf = u0 < 0 ? 0 : (uint64_t)u0;
        while (r + 1 < cnt && Pn <= uf) {
            r++;
            Pn = tb->P[r + 1];
        }
        const bool full = u0 >= 0 && (uint64_t)u0 + 4 <= tot;
        const uint64_t Pr = tb->P[r];
        const uint32_t rkl = T::K ? tb->kl[r] : 0;
        uint32_t v = 0;
        bool fast = false;
        if (full) {
            const uint64_t w0 = (uint64_t)u0 - Pr;
            if (T::K && w0 >= 4 && w0 + 4 <= 4 + (uint64_t)rkl) {
                v = ldg_u32_unaligned(S.keys + tb->K0[r] + (w0 - 4));
                fast = true;
            } else if (G == LSM_GRAMMAR_KV && w0 >= 8 + (uint64_t)rkl &&
                       w0 + 4 <= 8 + (uint64_t)rkl + tb->vl[r]) {
                v = ldg_u32_unaligned(S.vals + tb->V0[r] + (w0 - 8 - rkl));
                fast = true;
            } else if (G == LSM_GRAMMAR_V && w0 >= 4 && w0 + 4 <= 4 + (uint64_t)tb->vl[r]) {
                v = ldg_u32_unaligned(S.vals + tb->V0[r] + (w0 - 4));
                fast = true;
            }
        }
        if (fast) {
            dA[d] = v;
            continue;
        }
        // Slow path (length fields, record boundaries, chunk edges): byte by byte.
        uint32_t rr = r;
        gptr_t<uint8_t> db = (gptr_t<uint8_t>)(dA + d);
        for (uint32_t t = 0; t < 4; t++) {
            const int64_t u = u0 + t;
            if (u < 0 || (uint64_t)u >= tot) continue;
            while (rr + 1 < cnt && tb->P[rr + 1] <= (uint64_t)u) rr++;
            const uint32_t byte = rec_byte<G>(S, tb->K0[rr], tb->kl[rr], tb->V0[rr], tb->vl[rr],
                                              tb->xo[rr], (uint64_t)u - tb->P[rr]);
            if (full) v |= byte << (8 * t);
            else db[t] = (uint8_t)byte;
        }
        if (full) dA[d] = v;
    }
}


// ---- LDS-staged chunk encoder (the fast path) -----------------------------
//
// The chunk's source bytes (its keys span and/or values span, each contiguous
// in the CSR batch) are staged into LDS with coalesced 16 B loads, all issued
// before the first use, so the chunk costs one memory latency.  Output is
// then assembled in aligned 16 B segments: a segment inside one key or value
// is five LDS dwords and four v_alignbyte, a segment across a length field or
// record boundary is built per dword, and the two chunk-edge segments (bytes
// shared with neighbour chunks) are stored byte by byte.
constexpr uint32_t kStageBytes = 8192;  // per wave

struct StagedTable {
    uint32_t P[kWave + 1];  // chunk-relative record start; P[cnt] = chunk bytes
    uint32_t ks[kWave], vs[kWave];  // stage offsets of the key / value bytes
    uint32_t kl[kWave], vl[kWave];
    uint32_t xlo[kWave], xhi[kWave];  // IDX offset
};

struct StageLds {
    StagedTable tb;
    uint32_t w[kStageBytes / 4 + 8];
};

__device__ __forceinline__ uint32_t stage_byte(const uint32_t *w, uint32_t q) {
    return (w[q >> 2] >> (8 * (q & 3))) & 0xff;
}

template <int G>
__device__ __forceinline__ uint32_t staged_byte(const StageLds &L, uint32_t r, uint32_t w) {
    const StagedTable &t = L.tb;
    if (G == LSM_GRAMMAR_V) {
        if (w < 4) return (t.vl[r] >> (8 * w)) & 0xff;
        return stage_byte(L.w, t.vs[r] + w - 4);
    }
    const uint32_t kl = t.kl[r];
    if (w < 4) return (kl >> (8 * w)) & 0xff;
    if (w < 4 + kl) return stage_byte(L.w, t.ks[r] + w - 4);
    const uint32_t w2 = w - 4 - kl;
    if (G == LSM_GRAMMAR_IDX) return ((w2 < 4 ? t.xlo[r] : t.xhi[r]) >> (8 * (w2 & 3))) & 0xff;
    if (w2 < 4) return (t.vl[r] >> (8 * w2)) & 0xff;
    return stage_byte(L.w, t.vs[r] + w2 - 4);
}

// Stage offset of record-relative bytes [w, w+len) if they lie inside one
// key or value of record r, else ~0u.
template <int G>
__device__ __forceinline__ uint32_t staged_src(const StagedTable &t, uint32_t r, uint32_t w,
                                               uint32_t len) {
    if (G == LSM_GRAMMAR_V) {
        return (w >= 4 && w + len <= 4 + t.vl[r]) ? t.vs[r] + w - 4 : ~0u;
    }
    const uint32_t kl = t.kl[r];
    if (w >= 4 && w + len <= 4 + kl) return t.ks[r] + w - 4;
    if (G == LSM_GRAMMAR_KV && w >= 8 + kl && w + len <= 8 + kl + t.vl[r]) return t.vs[r] + w - 8 - kl;
    return ~0u;
}

// Stage two byte spans [srcA, srcA+nA) and [srcB, srcB+nB) (either may be
// empty) by LDS-DMA (buffer_load_dwordx4 ... lds: 1 KiB per wave
// instruction, no VGPR staging): span A's 16-byte lines at stage offset 0,
// span B's at the next 1 KiB boundary.  All loads are in flight together and
// one s_waitcnt releases them.  Returns the stage offsets of srcA and srcB.
__device__ __forceinline__ uint32_t span_lines(uint64_t src, uint32_t n) {
    return n ? (uint32_t)(((src & 15) + n + 15) >> 4) : 0;
}
__device__ __forceinline__ uint32_t span_stage_bytes(uint32_t lines) {
    return (lines * 16 + 1023) & ~1023u;
}

__device__ __forceinline__ void dma_span(uint32_t *w, uint32_t at, const uint8_t *base, uint64_t src,
                                         uint32_t lines) {
    const uint64_t a0 = src & ~(uint64_t)15;
    const rsrc_t r = make_rsrc(base + a0, lines * 16);
    const uint32_t v = lane_id() * 16;
    for (uint32_t c = 0; c * kWave < lines; c++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            r, (__attribute__((address_space(3))) void *)&w[(at + 1024 * c) / 4], 16, 1024 * c + v, 0,
            0, 0);
}

__device__ __forceinline__ void stage_spans(uint32_t *w, const uint8_t *baseA, uint64_t srcA,
                                            uint32_t nA, const uint8_t *baseB, uint64_t srcB,
                                            uint32_t nB, uint32_t &offA, uint32_t &offB) {
    const uint32_t lA = span_lines(srcA, nA), lB = span_lines(srcB, nB);
    const uint32_t atB = span_stage_bytes(lA);
    if (lA) dma_span(w, 0, baseA, srcA, lA);
    if (lB) dma_span(w, atB, baseB, srcB, lB);
    // The DMA writes are invisible to the compiler's LDS tracking.
    __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");
    offA = (uint32_t)(srcA & 15);
    offB = atB + (uint32_t)(srcB & 15);
}

// Encode records [c0, c0+cnt) (cnt <= 64) to dst through LDS.  Returns false
// (nothing written) when the chunk's source bytes exceed the stage.
template <int G>
__device__ bool encode_chunk_staged(const RegionSrc &S, uint64_t c0, uint32_t cnt, uint8_t *dst,
                                    StageLds *L) {
    using T = GrammarTraits<G>;
    const uint32_t lane = lane_id();
    const bool useK = T::K;
    const bool useV = T::V;
    const uint64_t Kc = useK ? uni64(S.koff[c0]) : 0, Ke = useK ? uni64(S.koff[c0 + cnt]) : 0;
    const uint64_t Vc = (useV || (G == LSM_GRAMMAR_IDX && !S.idx_off)) ? uni64(S.voff[c0]) : 0;
    const uint64_t Ve = useV ? uni64(S.voff[c0 + cnt]) : 0;
    const uint64_t nK = Ke - Kc, nV = Ve - Vc;
    if (nK > kStageBytes || nV > kStageBytes) return false;
    const uint32_t need = span_stage_bytes(useK ? span_lines(Kc, (uint32_t)nK) : 0) +
                          span_stage_bytes(useV ? span_lines(Vc, (uint32_t)nV) : 0);
    if (need > kStageBytes) return false;

    uint32_t kbase = 0, vbase = 0;
    stage_spans(L->w, S.keys, Kc, useK ? (uint32_t)nK : 0, S.vals, Vc, useV ? (uint32_t)nV : 0,
                kbase, vbase);

    uint32_t kl = 0, vl = 0, ks = 0, vs = 0, sz = 0;
    uint64_t xo = 0;
    if (lane < cnt) {
        const uint64_t i = c0 + lane;
        uint64_t K0 = 0, V0 = 0;
        if (useK) { K0 = S.koff[i]; kl = (uint32_t)(S.koff[i + 1] - K0); ks = kbase + (uint32_t)(K0 - Kc); }
        if (useV || (G == LSM_GRAMMAR_IDX && !S.idx_off)) V0 = S.voff[i];
        if (useV) { vl = (uint32_t)(S.voff[i + 1] - V0); vs = vbase + (uint32_t)(V0 - Vc); }
        if (G == LSM_GRAMMAR_IDX)
            xo = S.idx_off ? (uint64_t)S.idx_off[i]
                           : (uint64_t)(S.idx_base + (int64_t)(4 * (i - S.rs) + (V0 - S.vrs)));
        sz = T::pre + (useK ? kl : 0) + (useV ? vl : 0);
    }
    uint32_t tot;
    const uint32_t P = wave_excl_scan(sz, &tot);
    tot = uni(tot);
    if (lane < cnt) {
        L->tb.P[lane] = P;
        L->tb.ks[lane] = ks;
        L->tb.vs[lane] = vs;
        L->tb.kl[lane] = kl;
        L->tb.vl[lane] = vl;
        L->tb.xlo[lane] = (uint32_t)xo;
        L->tb.xhi[lane] = (uint32_t)(xo >> 32);
    }
    if (lane == 0) L->tb.P[cnt] = tot;
    // LDS ops of one wave complete in order: the stage and table are visible
    // to every lane's later reads.
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");

    const StagedTable &t = L->tb;
    const uintptr_t Ob = reinterpret_cast<uintptr_t>(dst);
    const uint32_t head = (uint32_t)(Ob & 15);
    gptr_t<u32x4> dA = gbl_at<u32x4>(Ob - head);
    const uint32_t nseg = (head + tot + 15) >> 4;
    uint32_t r = 0;
    for (uint32_t e = lane; e < nseg; e += kWave) {
        const int32_t u0 = (int32_t)(16 * e) - (int32_t)head;
        const uint32_t uf = u0 < 0 ? 0 : (uint32_t)u0;
        while (r + 1 < cnt && t.P[r + 1] <= uf) r++;
        if (u0 >= 0 && (uint32_t)u0 + 16 <= tot) {
            u32x4 out;
            const uint32_t q = staged_src<G>(t, r, (uint32_t)u0 - t.P[r], 16);
            if (q != ~0u) {
                const uint32_t a = q >> 2;
                const uint32_t s0 = L->w[a], s1 = L->w[a + 1], s2 = L->w[a + 2], s3 = L->w[a + 3],
                               s4 = L->w[a + 4];
                out.x = funnel(s0, s1, q);
                out.y = funnel(s1, s2, q);
                out.z = funnel(s2, s3, q);
                out.w = funnel(s3, s4, q);
            } else {
                uint32_t dw[4];
                uint32_t rr = r;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t u = (uint32_t)u0 + 4 * i;
                    while (rr + 1 < cnt && t.P[rr + 1] <= u) rr++;
                    const uint32_t w = u - t.P[rr];
                    const uint32_t q4 = (u + 4 <= t.P[rr + 1]) ? staged_src<G>(t, rr, w, 4) : ~0u;
                    if (q4 != ~0u) {
                        dw[i] = funnel(L->w[q4 >> 2], L->w[(q4 >> 2) + 1], q4);
                    } else {
                        uint32_t v = 0, rb = rr;
                        for (uint32_t b = 0; b < 4; b++) {
                            while (rb + 1 < cnt && t.P[rb + 1] <= u + b) rb++;
                            v |= staged_byte<G>(*L, rb, u + b - t.P[rb]) << (8 * b);
                        }
                        dw[i] = v;
                    }
                }
                out.x = dw[0]; out.y = dw[1]; out.z = dw[2]; out.w = dw[3];
            }
            dA[e] = out;
        } else {
            // chunk-edge segment: only this chunk's bytes, one at a time
            gptr_t<uint8_t> db = (gptr_t<uint8_t>)(dA + e);
            uint32_t rb = r;
            for (uint32_t b = 0; b < 16; b++) {
                const int32_t u = u0 + (int32_t)b;
                if (u < 0 || (uint32_t)u >= tot) continue;
                while (rb + 1 < cnt && t.P[rb + 1] <= (uint32_t)u) rb++;
                db[b] = (uint8_t)staged_byte<G>(*L, rb, (uint32_t)u - t.P[rb]);
            }
        }
    }
    // The next chunk overwrites the stage: every lane's reads must be done.
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    return true;
}

// ---- DMA-gather chunk encoder (V and IDX: the .sst regions) ----------------
//
// A V record is [u32 vlen][value] and an IDX record [u32 klen][key][i64 off]:
// one payload (value / key) plus fixed-size fields.  With chunk-relative
// record starts P[r] = pre*r + (payload bytes before r) (pre = 4 / 12), the
// payload byte at chunk position x of record r sits at source position
// x - pre*r - 4 (relative to the chunk's first payload byte): a per-record
// shift that is a multiple of 4.  So if the chunk image is laid out in LDS
// with the source's dword phase, every LDS dword of the image is exactly one
// aligned source dword, and the image is gathered by LDS-DMA (64 dwords per
// wave instruction, each lane's source from a 6-step ds_bpermute binary
// search for its record) -- no per-byte work and no divergence, whatever the
// record sizes.  Bytes of the fixed fields receive neighbouring payload bytes
// from the gather and are then overwritten by each record's lane (ds_write_b8;
// a dword never reaches from one payload into the next one's payload, since
// the 4-byte prefix sits between).  The image is stored with aligned 16-byte
// stores (ds_read_b128 + funnel shift), chunk-edge bytes singly.
constexpr uint32_t kGatherDwords = 1856;  // 7.25 KiB per wave
constexpr uint32_t kGatherMaskWords = kWave;  // one per lane; >= 2 * ceil(kGatherDwords / 64)

template <int G, uint32_t GD = kGatherDwords>
__device__ bool encode_chunk_gather(const RegionSrc &S, uint64_t c0, uint32_t cnt, uint8_t *dst,
                                    uint32_t *lds) {
    static_assert(kGatherMaskWords >= 2 * ((GD + 63) / 64), "one mask bit per image dword");
    static_assert(G != LSM_GRAMMAR_KV, "one payload per record");
    constexpr uint32_t pre = G == LSM_GRAMMAR_V ? 4 : 12;
    const uint32_t lane = lane_id();
    const uint8_t *sbase = G == LSM_GRAMMAR_V ? S.vals : S.keys;
    const uint64_t *soff = G == LSM_GRAMMAR_V ? S.voff : S.koff;
    const uint64_t Sc = uni64(soff[c0]);
    uint64_t len = 0, xo = 0;
    if (lane < cnt) {
        const uint64_t i = c0 + lane;
        len = soff[i + 1] - soff[i];
        if (G == LSM_GRAMMAR_IDX)
            xo = S.idx_off ? (uint64_t)S.idx_off[i]
                           : (uint64_t)(S.idx_base + (int64_t)(4 * (i - S.rs) + (S.voff[i] - S.vrs)));
    }
    uint64_t tot64;
    const uint64_t P64 = wave_excl_scan64(lane < cnt ? pre + len : 0, &tot64);
    tot64 = uni64(tot64);  // wave-uniform: keeps the loops below scalar
    const uint32_t ph = (uint32_t)(Sc & 3);
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
    if (tot64 + 64 > 4ull * GD) return false;
    const uint32_t tot = (uint32_t)tot64, P = (uint32_t)P64;
    const uint32_t nD = (tot + ph + 3) >> 2;
    const int32_t T = (int32_t)ph - (int32_t)head;
    const uint32_t sh = (uint32_t)T & 3;
    const uint32_t OD = 8 + (((uint32_t)(-(T - (int32_t)sh)) >> 2) & 3);
    if (OD + ((nD + 63) & ~63u) + 8 > GD) return false;

    // gather: image dword D covers chunk bytes [4D - ph, 4D - ph + 4)
    const uint32_t sbytes = (uint32_t)(soff[c0 + cnt] - Sc);  // wave-uniform load below
    const rsrc_t rs = make_rsrc(sbase + (Sc - ph), uni((sbytes + ph + 3) & ~3u));
    // Record of image dword D (its first byte x0 = 4D - ph): the number of
    // record starts t >= 1 with P[t] <= x0, i.e. with e_t = ceil((P[t]+ph)/4)
    // <= D.  Records are >= 4 bytes, so the e_t are distinct: one bit each
    // in an LDS mask, and window i (dwords [64i, 64i+64)) reads its 64-bit
    // word once -- a lane's record is the running count plus a masked
    // popcount (mbcnt), no search.
    uint32_t *mask = lds + GD;  // kGatherMaskWords after the image
    for (uint32_t w = lane; w < kGatherMaskWords; w += kWave) mask[w] = 0;
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    if (lane >= 1 && lane < cnt) {
        const uint32_t et = (P + ph + 3) >> 2;
        atomicOr(&mask[et >> 5], 1u << (et & 31));
    }
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    uint32_t rb = 0;
    const uint32_t mv = mask[lane];  // lane w holds mask word w (64 words)
    for (uint32_t i = 0; i * kWave < nD; i++) {
        const int32_t x0 = 256 * (int32_t)i + 4 * (int32_t)lane - (int32_t)ph;
        // (readlane returns int: cast to u32 before widening, no sign extension)
        const uint64_t M = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(mv, 2 * i + 1) << 32 |
                           (uint32_t)__builtin_amdgcn_readlane(mv, 2 * i);
        const uint32_t r = rb + mbcnt(M) + (uint32_t)((M >> lane) & 1);
        rb += (uint32_t)__builtin_popcountll(M);
        const uint32_t voff = (uint32_t)(x0 - (int32_t)(pre * r) - 4 + (int32_t)ph);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void *)&lds[OD + i * kWave], 4, voff, 0, 0, 2);
    }
    __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");

    // fixed fields of this lane's record
    uint8_t *ob = reinterpret_cast<uint8_t *>(lds) + 4 * OD + ph;
    if (lane < cnt) {
        const uint32_t l32 = (uint32_t)len;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) ob[P + b] = (uint8_t)(l32 >> (8 * b));
        if (G == LSM_GRAMMAR_IDX) {
#pragma unroll
            for (uint32_t b = 0; b < 8; b++) ob[P + 4 + l32 + b] = (uint8_t)(xo >> (8 * b));
        }
    }
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");

    // store: segment e = global bytes [dA + 16e, +16) = chunk bytes [16e - head, +16)
    gptr_t<u32x4> dA = gbl_at<u32x4>(reinterpret_cast<uintptr_t>(dst) - head);
    const uint32_t nseg = (head + tot + 15) >> 4;
    const uint32_t q0 = OD + (uint32_t)((T - (int32_t)sh) >> 2);  // dword of segment 0
    for (uint32_t e = lane; e < nseg; e += kWave) {
        const int32_t u0 = 16 * (int32_t)e - (int32_t)head;
        if (u0 >= 0 && (uint32_t)u0 + 16 <= tot) {
            const uint32_t q = q0 + 4 * e;
            const u32x4 a = *reinterpret_cast<const u32x4 *>(&lds[q]);
            const uint32_t a4 = lds[q + 4];
            u32x4 o;
            o.x = funnel(a.x, a.y, sh);
            o.y = funnel(a.y, a.z, sh);
            o.z = funnel(a.z, a.w, sh);
            o.w = funnel(a.w, a4, sh);
            __builtin_nontemporal_store(o, &dA[e]);
        } else {
            gptr_t<uint8_t> db = (gptr_t<uint8_t>)(dA + e);
            for (uint32_t b = 0; b < 16; b++) {
                const int32_t u = u0 + (int32_t)b;
                if (u >= 0 && (uint32_t)u < tot) db[b] = ob[u];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    return true;
}

// Per-wave LDS: the staged encoder, or the global-source fallback's table.
union EncodeLds {
    StageLds st;
    ChunkTable ct;
    uint32_t gather[kGatherDwords + kGatherMaskWords];
};
// Chunk encoder dispatch: DMA gather (V / IDX), LDS-staged (KV), then the
// global-source fallback for chunks too large for LDS.  The three LDS views
// alias one per-wave buffer.
template <int G, uint32_t GD = kGatherDwords>
__device__ __forceinline__ void encode_chunk_any(const RegionSrc &S, uint64_t c0, uint32_t cnt,
                                                 uint8_t *dst, uint32_t *gather, StageLds *st,
                                                 ChunkTable *ct) {
    if (G == LSM_GRAMMAR_KV) {
        if (encode_chunk_staged<LSM_GRAMMAR_KV>(S, c0, cnt, dst, st)) return;
    } else {
        if (encode_chunk_gather<G == LSM_GRAMMAR_KV ? LSM_GRAMMAR_V : G, GD>(S, c0, cnt, dst,
                                                                             gather))
            return;
    }
    encode_chunk<G>(S, c0, cnt, dst, ct);
}

// ---- lsm_encode_blocks ----------------------------------------------------

struct EncodeBlocksArgs {
    RegionSrc S;
    const uint64_t *rec_start;
    uint32_t nblk;
    uint8_t *out;
    const uint64_t *out_off;
};

constexpr int kEncWaves = 4;

template <int G>
__global__ __launch_bounds__(256) void encode_blocks_kernel(EncodeBlocksArgs a) {
    using T = GrammarTraits<G>;
    __shared__ EncodeLds lds[kEncWaves];
    const uint32_t b = blockIdx.x;
    const uint32_t wave = uni(threadIdx.x / kWave);
    const uint64_t rs = uni64(a.rec_start[b]);
    const uint64_t re = uni64(a.rec_start[b + 1]);
    uint8_t *out = a.out + uni64(a.out_off[b]);
    const uint64_t Krs = T::K ? uni64(a.S.koff[rs]) : 0;
    const uint64_t Vrs = T::V ? uni64(a.S.voff[rs]) : 0;
    for (uint64_t c0 = rs + (uint64_t)wave * kWave; c0 < re; c0 += kEncWaves * kWave) {
        uint32_t cnt = (uint32_t)((re - c0) < (uint64_t)kWave ? (re - c0) : kWave);
        uint64_t rel = T::pre * (c0 - rs);
        if (T::K) rel += uni64(a.S.koff[c0]) - Krs;
        if (T::V) rel += uni64(a.S.voff[c0]) - Vrs;
        encode_chunk_any<G>(a.S, c0, cnt, out + rel, lds[wave].gather, &lds[wave].st, &lds[wave].ct);
    }
}

// ---- fused bloom build (LDS slices) --------------------------------------

// Header bytes of the .sst holding records [s, e): u32 kl | min key | u32 kl |
// max key (header.go:25-37; Builder.Finalize sets min/max = first/last key).
__device__ __forceinline__ uint64_t sst_header_bytes(const uint64_t *koff, uint64_t s, uint64_t e) {
    if (e <= s) return 8;
    return 8 + (uni64(koff[s + 1]) - uni64(koff[s])) + (uni64(koff[e]) - uni64(koff[e - 1]));
}

// Big-endian stream dword q of the filter words held in LDS as native u32
// pairs (word w = bits[2w] | bits[2w+1] << 32; bitset.WriteTo writes words
// big-endian, so stream dword 2w is bswap(hi), 2w+1 is bswap(lo)).
__device__ __forceinline__ uint32_t be_dword(const uint32_t *bits, uint64_t q) {
    return bswap32(bits[(q & ~1ull) + ((q & 1) ^ 1)]);
}

// Store an LDS slice holding native filter words [wlo, whi) (bits[0] = word
// wlo's low half).  Image mode (img_words != null, pointing at filter word 0
// inside the .sst): big-endian bytes, whole dwords inside the slice's byte
// range and single bytes at its edges (the neighbouring bytes belong to the
// other slice or to the filter prefix).  Native mode: u64 words to native.
// The thread group a filter body runs on (the whole workgroup).
struct WgGroup {
    __device__ uint32_t tid() const { return threadIdx.x; }
    __device__ uint32_t size() const { return blockDim.x; }
    __device__ void sync() { __syncthreads(); }
};

template <class Grp>
__device__ void store_filter_slice(const Grp &g, const uint32_t *bits, uint64_t wlo, uint64_t whi,
                                   uint8_t *img_words, uint64_t *native) {
    const uint32_t nthr = g.size();
    if (!img_words) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(native + wlo);
        for (uint64_t i = g.tid(); i < 2 * (whi - wlo); i += nthr) dst[i] = bits[i];
        return;
    }
    const uint64_t len = 8 * (whi - wlo);
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(img_words + 8 * wlo);
    const uint32_t head = (uint32_t)(p0 & 3);
    gptr_t<uint32_t> dA = gbl_at<uint32_t>(p0 - head);
    const uint64_t ndw = (head + len + 3) / 4;
    for (uint64_t d = g.tid(); d < ndw; d += nthr) {
        const int64_t u0 = (int64_t)(4 * d) - head;
        if (u0 >= 0 && (uint64_t)u0 + 4 <= len) {
            const uint64_t q = (uint64_t)u0 >> 2;
            const uint32_t sh = (uint32_t)u0 & 3;
            const uint32_t lo = be_dword(bits, q);
            const uint32_t hi = sh ? be_dword(bits, q + 1) : 0;
            __builtin_nontemporal_store(funnel(lo, hi, sh), &dA[d]);
        } else {
            gptr_t<uint8_t> db = (gptr_t<uint8_t>)(dA + d);
            for (uint32_t b = 0; b < 4; b++) {
                const int64_t u = u0 + b;
                if (u < 0 || (uint64_t)u >= len) continue;
                db[b] = (uint8_t)(be_dword(bits, (uint64_t)u >> 2) >> (8 * ((uint32_t)u & 3)));
            }
        }
    }
}

struct BloomArgs {
    const uint8_t *keys;
    const uint64_t *koff;
    const uint64_t *file_start;
    uint64_t m, mrecip;
    uint32_t k;
    uint64_t slice_bits;   // multiple of 64
    uint64_t nwords;       // ceil(m/64)
    uint64_t *bitmap;      // native mode: nfile * nwords u64 words
    uint64_t nkeys;        // keys of the single filter when file_start == null
    uint8_t *out;          // image mode (bitmap == null): .sst images
    const uint64_t *file_off;
};

// One workgroup per (filter, slice): hashes every key of the filter (sum256 +
// k locations + Barrett modulo) and ds_or's the bits inside its slice.  Used
// for single filters (lsm_bloom_build) and for filters whose slice count the
// binned path below does not cover.
__global__ __launch_bounds__(1024) void bloom_slices_kernel(BloomArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_bits[];
    const uint32_t f = blockIdx.x;
    const uint64_t lo = (uint64_t)blockIdx.y * a.slice_bits;
    if (lo >= a.m) return;
    const uint64_t hi = lo + a.slice_bits < a.m ? lo + a.slice_bits : a.m;
    const uint32_t nw32 = (uint32_t)((hi - lo + 63) / 64) * 2;
    for (uint32_t i = threadIdx.x; i < nw32; i += blockDim.x) lds_bits[i] = 0;
    __syncthreads();
    const uint64_t s = a.file_start ? a.file_start[f] : 0;
    const uint64_t e = a.file_start ? a.file_start[f + 1] : a.nkeys;
    for (uint64_t i = s + threadIdx.x; i < e; i += blockDim.x) {
        uint64_t k0 = a.koff[i];
        uint64_t h[4];
        sum256(a.keys + k0, a.koff[i + 1] - k0, h);
        for (uint32_t j = 0; j < a.k; j++) {
            uint64_t p = mod_barrett(location(h[0], h[1], h[2], h[3], j), a.m, a.mrecip);
            if (p >= lo && p < hi) {
                uint32_t q = (uint32_t)(p - lo);
                atomicOr(&lds_bits[q >> 5], 1u << (q & 31));
            }
        }
    }
    __syncthreads();
    const uint64_t wlo = lo / 64, whi = (hi + 63) / 64;
    if (a.bitmap) {
        store_filter_slice(WgGroup{}, lds_bits, wlo, whi, nullptr, a.bitmap + (uint64_t)f * a.nwords);
    } else {
        const uint64_t hdr = sst_header_bytes(a.koff, s, e);
        store_filter_slice(WgGroup{}, lds_bits, wlo, whi, a.out + uni64(a.file_off[f]) + hdr + 32,
                           nullptr);
    }
}

constexpr uint32_t kBinBatch = 8;  // locations per staging round

// ---- per-file bloom build, hash once (one or two slices, m < 2^32) -----------
//
// One 1024-thread workgroup per filter holds slice 0 (the first <= 100 KiB of
// bits) in LDS.  It hashes each key of its filter exactly once: bits in slice
// 0 are ds_or'ed at once, bits in slice 1 are appended to the filter's own
// workspace list (wave-aggregated: one LDS counter add per location index
// and a coalesced store).  Slice 0 is then stored, the LDS re-zeroed, and
// the list -- just written by this workgroup, read back through L2 with nt
// loads -- OR'ed in as slice 1.  No cross-workgroup dependency, no global
// atomics, and the hash (the VALU-bound part) is done once per key.
struct BloomFileArgs {
    const uint8_t *keys;
    const uint64_t *koff;
    const uint64_t *file_start;  // null: one filter over keys [0, nkeys)
    uint64_t nkeys;
    uint64_t m, mrecip;
    uint32_t k;
    uint32_t split;   // slice 0 = bits [0, split); split >= m: one slice
    uint32_t c64;     // 2^64 mod m (m <= 2^30)
    uint32_t *pos;    // slice-1 list of filter f at f * k * maxr (two slices only)
    uint32_t maxr;
    uint64_t nwords;
    uint8_t *out;     // image mode
    const uint64_t *file_off;
    uint64_t *bitmap; // native mode (out == null)
};

// The filter of file f by thread group g (lds_bits: the slice-0 LDS, n1: a
// shared counter): the whole workgroup in bloom_file_kernel, the filter waves
// in sst_build_kernel.
template <class Grp>
__device__ void bloom_file_body(Grp &g, const BloomFileArgs &a, uint32_t f, uint32_t *lds_bits,
                                uint32_t &n1) {
    const uint32_t lane = lane_id();
    const uint64_t s = a.file_start ? uni64(a.file_start[f]) : 0;
    const uint64_t e = a.file_start ? uni64(a.file_start[f + 1]) : a.nkeys;
    const bool two = a.split < a.m;
    const uint64_t lo1 = two ? a.split : a.m;  // end of slice 0
    const uint32_t nw0 = (uint32_t)((lo1 + 63) / 64) * 2;
    for (uint32_t i = g.tid(); i < nw0; i += g.size()) lds_bits[i] = 0;
    if (g.tid() == 0) n1 = 0;
    g.sync();
    uint32_t *list = two ? a.pos + (uint64_t)f * a.k * a.maxr : nullptr;
    // Two-stage load pipeline across rounds (a wave takes 64 keys per round,
    // rounds 1024 keys apart): while round r hashes, the first 16 key bytes
    // of round r+1 and the offsets of round r+2 are in flight.  Indices past
    // the filter are clamped to its last key (unconditional loads).
    const uint32_t stride = g.size();
    auto clampi = [&](uint64_t i) { return i < e ? i : e - 1; };
    uint64_t i0 = s + (g.tid() & ~63u);
    uint64_t ka = 0, la = 0, fa0 = 0, fa1 = 0, kb = 0, lb = 0;
    if (i0 < e) {
        const uint64_t ii = clampi(i0 + lane);
        ka = a.koff[ii];
        la = a.koff[ii + 1] - ka;
        fa0 = ldg_u64_unaligned(a.keys + ka);
        fa1 = ldg_u64_unaligned(a.keys + ka + 8);
        const uint64_t jn = clampi(i0 + stride + lane);
        kb = a.koff[jn];
        lb = a.koff[jn + 1] - kb;
    }
    for (; i0 < e; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool act = i < e;
        // prefetch: key bytes of the next round, offsets of the one after
        const uint64_t fb0 = ldg_u64_unaligned(a.keys + kb);
        const uint64_t fb1 = ldg_u64_unaligned(a.keys + kb + 8);
        const uint64_t jc = clampi(i0 + 2 * stride + lane);
        const uint64_t kc = a.koff[jc];
        const uint64_t lc = a.koff[jc + 1] - kc;
        uint64_t h[4];
        sum256_pre(a.keys + ka, la, fa0, fa1, h);
        ka = kb; la = lb; fa0 = fb0; fa1 = fb1;
        kb = kc; lb = lc;
        // 16 locations per round; a lane keeps its slice-1 positions in
        // registers and the wave reserves list space once per round.
        // location(j) = h[j%2] + j*h[2 + ((j + j%2) % 4)/2] (bloom.go:133-136):
        // by class c = j%4 the multiplier is h2, h3, h3, h2, so each class is
        // an arithmetic progression with step 4*h2 or 4*h3 -- additions only
        // (64-bit multiplies are quarter-rate).
        // The residues mod m follow the progressions too: r += (step mod m),
        // less (2^64 mod m) when the 64-bit addition wraps -- 32-bit adds and
        // v_min instead of a Barrett reduction per location (m <= 2^30).
        uint64_t loc[4] = {h[0], h[1] + h[3], h[0] + (h[3] << 1), h[1] + h[2] + (h[2] << 1)};
        const uint64_t st2 = h[2] << 2, st3 = h[3] << 2;
        const uint32_t m32 = (uint32_t)a.m, rl = (uint32_t)a.mrecip, rh = (uint32_t)(a.mrecip >> 32);
        uint32_t res[4];
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) res[c] = mod_small(loc[c], m32, rl, rh);
        const uint32_t d2 = mod_small(st2, m32, rl, rh), d3 = mod_small(st3, m32, rl, rh);
        // the steps less 2^64 mod m, for a step whose 64-bit add wraps
        const uint32_t w2 = d2 >= a.c64 ? d2 - a.c64 : d2 + m32 - a.c64;
        const uint32_t w3 = d3 >= a.c64 ? d3 - a.c64 : d3 + m32 - a.c64;
        for (uint32_t j0 = 0; j0 < a.k; j0 += kBinBatch) {
            uint32_t pp[kBinBatch];
            uint32_t c1 = 0;
#pragma unroll
            for (uint32_t jj = 0; jj < kBinBatch; jj++) {
                const uint32_t j = j0 + jj;
                const bool valid = act && j < a.k;
                const uint32_t c = jj & 3;  // j0 is a multiple of 4
                const uint32_t p = res[c];
                if (j + 4 < a.k) {  // wave-uniform: the class's next location
                    const bool a2 = c == 0 || c == 3;
                    uint64_t nl;
                    const bool carry = __builtin_add_overflow(loc[c], a2 ? st2 : st3, &nl);
                    loc[c] = nl;
                    const uint32_t t = res[c] + (carry ? (a2 ? w2 : w3) : (a2 ? d2 : d3));
                    res[c] = min(t, t - m32);
                }
                const bool in1 = p >= (uint32_t)lo1;  // lo1 <= m <= 2^30
                if (valid && !in1) atomicOr(&lds_bits[p >> 5], 1u << (p & 31));
                pp[jj] = valid && in1 ? p : 0xFFFFFFFFu;
                c1 += (uint32_t)(valid && in1);
            }
            if (two) {
                uint32_t tot1;
                const uint32_t ex = wave_excl_scan(c1, &tot1);
                tot1 = uni(tot1);
                if (tot1) {
                    uint32_t o = 0;
                    if (lane == 0) o = atomicAdd(&n1, tot1);
                    uint32_t w = uni(o) + ex;
#pragma unroll
                    for (uint32_t jj = 0; jj < kBinBatch; jj++)
                        if (pp[jj] != 0xFFFFFFFFu) list[w++] = pp[jj];
                }
            }
        }
    }
    g.sync();
    if (a.out) {
        const uint64_t hdr = sst_header_bytes(a.koff, s, e);
        store_filter_slice(g, lds_bits, 0, (lo1 + 63) / 64, a.out + uni64(a.file_off[f]) + hdr + 32,
                           nullptr);
    } else {
        store_filter_slice(g, lds_bits, 0, (lo1 + 63) / 64, nullptr, a.bitmap + (uint64_t)f * a.nwords);
    }
    if (!two) {
        g.sync();  // the LDS slice is reused by the caller
        return;
    }
    // slice 1 from this group's own list
    __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");
    g.sync();
    const uint32_t nw1 = (uint32_t)((a.m - lo1 + 63) / 64) * 2;
    for (uint32_t i = g.tid(); i < nw1; i += g.size()) lds_bits[i] = 0;
    g.sync();
    const uint32_t n = n1;
    constexpr uint32_t kU = 16;
    for (uint32_t t0 = g.tid(); t0 < n; t0 += kU * g.size()) {
        uint32_t q[kU];
#pragma unroll
        for (uint32_t j = 0; j < kU; j++) {
            const uint32_t t = t0 + j * g.size();
            q[j] = __builtin_nontemporal_load(&list[t < n ? t : n - 1]) - (uint32_t)lo1;
        }
#pragma unroll
        for (uint32_t j = 0; j < kU; j++) atomicOr(&lds_bits[q[j] >> 5], 1u << (q[j] & 31));
    }
    g.sync();
    if (a.out) {
        const uint64_t hdr = sst_header_bytes(a.koff, s, e);
        store_filter_slice(g, lds_bits, lo1 / 64, a.nwords, a.out + uni64(a.file_off[f]) + hdr + 32,
                           nullptr);
    } else {
        store_filter_slice(g, lds_bits, lo1 / 64, a.nwords, nullptr, a.bitmap + (uint64_t)f * a.nwords);
    }
    g.sync();  // the LDS slice is reused by the caller
}

__global__ __launch_bounds__(1024) void bloom_file_kernel(BloomFileArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_bits[];
    __shared__ uint32_t n1;
    WgGroup g;
    bloom_file_body(g, a, blockIdx.x, lds_bits, n1);
}

// ---- split bloom build: hash in the region writer, then OR per slice -------
//
// bloom_file_kernel pins one 1024-thread workgroup and 100 KiB of LDS per
// filter to a CU for the whole hash, so beside the region writers it runs on
// 208 CUs with LDS to spare for only a few region waves.  For two-slice
// filters with k <= 16 the build is split: the region writer (which gathers
// every key into LDS for the index region anyway) hashes each key once and
// leaves per key the residues mod m of the four location classes' bases and
// of the class step of classes 0 and 3 (location(j) = h[j%2] + j*h[2 + ((j + j%2) % 4)/2],
// bloom.go:133-136: class c = j%4 is an arithmetic progression) plus the carry
// bit of each 64-bit step and the two carries that rebuild the other class
// step from the class bases: 16 bytes; bloom_or_kernel then rebuilds the k
// locations of every key of its filter from them (additions only) and ORs
// those of its slice into LDS.
//
// Record (m <= 2^21: a two-slice filter is at most 2 * 819,200 bits), dword c
// of 4: bits 0-20 the residue of class c's base, bits 21-23 the carries of
// its three steps, bits 24-31 byte c of X = res(4 h2) | a << 21 | b << 22,
// where T = 2 h3 mod 2^64, a = carry of h0 + T (class 2's base) and b = the
// top bit of T: res(T) = res(base2) - res(base0) + a (2^64 mod m), and
// res(4 h3) = 2 res(T) - b (2^64 mod m), all mod m.  (24 bytes per key, the
// round-4 record, were read twice and written once: 1.28x the algorithmic
// traffic of config 3.)
constexpr uint32_t kHashRecDwords = 4;
constexpr uint32_t kHashRecBits = 21;  // residue bits: m <= 2^21
constexpr uint32_t kOrSlices = 2;  // bloom_or_kernel workgroups per filter
constexpr uint32_t kSplitMaxK = 16;  // three carries per class fit the record

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// The 16-byte hash record of a key from its sum256 digest (layout above).
__device__ __forceinline__ void store_hash_rec(const uint64_t h[4], uint32_t m, uint32_t rl,
                                               uint32_t rh, uint32_t *rec) {
    const uint64_t T = h[3] << 1;
    const uint64_t loc[4] = {h[0], h[1] + h[3], h[0] + T, h[1] + h[2] + (h[2] << 1)};
    const uint64_t st2 = h[2] << 2, st3 = h[3] << 2;
    uint32_t r[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        uint32_t cy = 0;  // bit n: the step to location 4(n + 1) + c carries
        const uint64_t st = (c == 0 || c == 3) ? st2 : st3;
        uint64_t l = loc[c];
#pragma unroll
        for (uint32_t n = 0; n < 3; n++) {
            uint64_t nl;
            cy |= (uint32_t)__builtin_add_overflow(l, st, &nl) << n;
            l = nl;
        }
        r[c] = mod_small(loc[c], m, rl, rh) | cy << kHashRecBits;
    }
    const uint32_t a = loc[2] < h[0];  // h0 + T wrapped
    const uint32_t x = mod_small(st2, m, rl, rh) | a << 21 | (uint32_t)(T >> 63) << 22;
#pragma unroll
    for (uint32_t c = 0; c < 3; c++) r[c] |= ((x >> (8 * c)) & 0xFFu) << 24;
    *(gptr_t<u32x4>)gbl(rec) = u32x4{r[0], r[1], r[2], r[3]};
}

struct BloomOrArgs {
    const uint64_t *file_start;  // rec[0] is key file_start[0]
    const uint32_t *rec;
    uint32_t m, k, c64;
    uint32_t split;     // slice 0 = bits [0, split), slice 1 = [split, m)
    uint32_t nfiles;
    uint64_t nwords;
    const uint64_t *koff;
    uint8_t *out;
    const uint64_t *file_off;
    const uint64_t *dnf;  // the stream build: the file count on the device (nfiles bounds it)
};

// ---- .sst image writer ------------------------------------------------------

struct SstArgs {
    const uint8_t *keys;
    const uint64_t *koff;
    const uint8_t *vals;
    const uint64_t *voff;
    const uint64_t *file_start;
    uint8_t *out;
    const uint64_t *file_off;
    int64_t *footer;
    uint64_t m, nwords;
    uint32_t k;
    uint32_t skip_v;  // the V region is written from value views (lsm_build_sst_views)
    // the filter's key hashes fused into the region writer: a hash record per
    // key (store_hash_rec, key file_start[0] first), or null
    uint32_t *hrec;
    uint32_t hm, hrl, hrh;
    // the stream build (lsm_build_sst_stream): the region writer's grid is one
    // dimension of 128-record spans, span j of file span_file[j], whose
    // layout is desc[span_file[j]] (written by sst_stream_plan_kernel); null
    // for the file-major grid of lsm_build_sst
    const uint32_t *span_file;
    const struct FileDesc *desc;
    const uint32_t *plan;  // {nfile, spans, common span count, 0}
};

// One file of a stream build, as the plan kernel lays it out: records
// [s, e), the image at out + img, its V / IDX regions at data_off / idx_off
// inside it, Ks = koff[s], Vs = voff[s], and its first span in the region
// writer's grid.  64 bytes: one scalar load of 16 dwords.
struct FileDesc {
    uint64_t s, e, img, data_off, idx_off, Ks, Vs;
    uint32_t span0, pad;
};

struct SstLayout {
    uint64_t s, e;
    uint32_t kl0, kl1;
    uint64_t hdr, filter_bytes, data_off, data_size, idx_off, idx_size, img;
};

__device__ __forceinline__ SstLayout sst_layout(const SstArgs &a, uint32_t f) {
    SstLayout L;
    L.s = uni64(a.file_start[f]);
    L.e = uni64(a.file_start[f + 1]);
    L.kl0 = L.kl1 = 0;
    if (L.e > L.s) {
        L.kl0 = (uint32_t)(uni64(a.koff[L.s + 1]) - uni64(a.koff[L.s]));
        L.kl1 = (uint32_t)(uni64(a.koff[L.e]) - uni64(a.koff[L.e - 1]));
    }
    L.hdr = 8 + (uint64_t)L.kl0 + L.kl1;
    L.filter_bytes = 32 + 8 * a.nwords;
    L.data_off = L.hdr + L.filter_bytes;
    const uint64_t n = L.e - L.s;
    L.data_size = 4 * n + (uni64(a.voff[L.e]) - uni64(a.voff[L.s]));
    L.idx_off = L.data_off + L.data_size;
    L.idx_size = 12 * n + (uni64(a.koff[L.e]) - uni64(a.koff[L.s]));
    L.img = L.idx_off + L.idx_size + 32;
    return L;
}

constexpr int kSstWaves = 4;
constexpr uint32_t kSstChunkRecs = kSstWaves * kWave;  // records per workgroup

// ---- .sst regions: pipelined two-region gather ------------------------------
//
// Data region (V grammar, [u32 vlen][value], sstable.go:159-175) and index
// region (IDX grammar, [u32 klen][key][i64 off], index.go:30-58) of file
// blockIdx.x.  One wave writes kRegWaveChunks consecutive 64-record chunks.
// Both region images of a chunk are DMA-gathered into the wave's LDS buffer
// together (encode_chunk_gather's dword-phase layout, one memory round trip
// for both), the next chunk's record offsets are loaded while they land, and
// the chunk's stores are still in flight when the next chunk's gathers are
// issued.  A chunk whose images do not fit the buffer takes the one-region
// encoders.
constexpr uint32_t kRegWaves = 2;         // waves per workgroup
constexpr uint32_t kRegWaveChunks = 1;    // 64-record chunks per wave (4: config 3 0.2573 ms, 2: 0.2500, 8: 0.2650; 1: 0.2488 vs 0.2531, round 5; A/B)
constexpr uint32_t kRegBufDwords = 2432;  // both images of a chunk (9.5 KiB)
constexpr uint32_t kRegIdxDwords = 1024;  // the IDX image alone (values from views: 4 KiB)
constexpr uint32_t kRegSpanRecs = kRegWaves * kRegWaveChunks * kWave;  // records per workgroup
constexpr uint32_t kRegMaxImage = 32 * kGatherMaskWords;  // dwords one mask covers

// Per-lane record offsets of a chunk (record c0 + lane): value bounds (V
// payload, and the IDX offset) and key bounds (IDX payload).
struct ChunkOffs {
    uint64_t v0, v1, k0, k1;
};

__device__ __forceinline__ ChunkOffs load_offs(const SstArgs &a, uint64_t c0, uint32_t cnt) {
    ChunkOffs o{0, 0, 0, 0};
    if (lane_id() < cnt) {
        const uint64_t i = c0 + lane_id();
        o.v0 = a.voff[i];
        o.v1 = a.voff[i + 1];
        o.k0 = a.koff[i];
        o.k1 = a.koff[i + 1];
    }
    return o;
}

__device__ __forceinline__ uint64_t lane64(uint64_t v, uint32_t l) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l) << 32 |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
}

// One region image of a chunk in the LDS buffer: image dword D (at buffer
// dword base + OD + D) covers chunk bytes [4D - ph, 4D - ph + 4).
struct RegionPlan {
    uint32_t P, len;  // per lane: chunk-relative record start, payload length
    uint64_t xo;      // per lane: IDX offset
    uint32_t cnt, tot, ph, head, sh, OD, nD, base, sbytes;  // wave-uniform
    uint32_t ulen;    // wave-uniform: the records' common payload length, or ~0u
    uint64_t Sc;      // wave-uniform: source offset of the first payload byte
    uint8_t *dst;
};

// Lays out region G of the chunk at buffer dword `base`; false if it does not
// fit below `cap` (or one mask word set does not cover it).
template <int G>
__device__ __forceinline__ bool region_plan(RegionPlan &R, const ChunkOffs &o, uint32_t cnt,
                                            uint8_t *dst, uint32_t base, uint32_t cap,
                                            int64_t xo_base) {
    constexpr uint32_t pre = G == LSM_GRAMMAR_V ? 4 : 12;
    const uint32_t lane = lane_id();
    const uint64_t p0 = G == LSM_GRAMMAR_V ? o.v0 : o.k0, p1 = G == LSM_GRAMMAR_V ? o.v1 : o.k1;
    const uint64_t len = lane < cnt ? p1 - p0 : 0;
    R.cnt = cnt;
    R.dst = dst;
    R.base = base;
    R.Sc = lane64(p0, 0);
    R.sbytes = 0;
    // records of one payload length (fixed-size keys or values): the record
    // starts are lane * (pre + len), no 64-bit scan
    const uint64_t l0 = lane64(len, 0);
    const bool uniform = !__ballot(lane < cnt && len != l0);
    uint64_t P64, tot64;
    if (uniform) {
        P64 = (uint64_t)lane * (pre + l0);
        tot64 = (uint64_t)cnt * (pre + l0);
    } else {
        P64 = wave_excl_scan64(lane < cnt ? pre + len : 0, &tot64);
        tot64 = uni64(tot64);
    }
    if (tot64 + 64 > 4ull * cap) return false;
    R.len = (uint32_t)len;
    R.ulen = uniform && l0 < 0xFFFFFFFFull ? (uint32_t)l0 : ~0u;
    R.P = (uint32_t)P64;
    R.tot = (uint32_t)tot64;
    R.xo = G == LSM_GRAMMAR_IDX ? (uint64_t)(xo_base + (int64_t)(4 * lane) + (int64_t)o.v0) : 0;
    R.sbytes = uni((uint32_t)(lane64(p1, cnt - 1) - R.Sc));
    R.ph = (uint32_t)(R.Sc & 3);
    R.head = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
    R.nD = (R.tot + R.ph + 3) >> 2;
    const int32_t T = (int32_t)R.ph - (int32_t)R.head;
    R.sh = (uint32_t)T & 3;
    R.OD = 8 + (((uint32_t)(-(T - (int32_t)R.sh)) >> 2) & 3);
    return R.nD <= kRegMaxImage && base + R.OD + ((R.nD + 63) & ~63u) + 8 <= cap;
}

// Issues the DMA gather of a planned region (see encode_chunk_gather).
template <int G>
__device__ __forceinline__ void region_issue(const RegionPlan &R, uint32_t *buf, uint32_t *mask,
                                             const uint8_t *sbase) {
    constexpr uint32_t pre = G == LSM_GRAMMAR_V ? 4 : 12;
    const uint32_t lane = lane_id();
    const rsrc_t rs = make_rsrc(sbase + (R.Sc - R.ph), uni((R.sbytes + R.ph + 3) & ~3u));
    if (R.ulen != ~0u) {
        // records of one size S: the record of image dword D (first byte
        // x0 = 4D - ph) is floor(x0 / S) (< cnt inside the image; dwords past
        // it are never read back).  floor((x + 1/2) * rcp(S)) is exact for
        // x < 2^16 (the quotient is at least 1/(2S) from an integer); it
        // seeds the first two rounds, and each later round (x0 + 256) steps
        // the record by q = floor(256 / S) or q + 1 and the source offset
        // with it: a remainder test instead of the float division per round.
        const uint32_t S = pre + R.ulen;
        const float inv = __builtin_amdgcn_rcpf((float)S), hinv = 0.5f * inv;
        const int32_t x00 = 4 * (int32_t)lane - (int32_t)R.ph;
        {
            const uint32_t xq = x00 < 0 ? 0u : (uint32_t)x00;
            const uint32_t r = min((uint32_t)__builtin_fmaf((float)xq, inv, hinv), R.cnt - 1);
            const uint32_t voff = (uint32_t)(x00 - (int32_t)(pre * r) - 4 + (int32_t)R.ph);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rs, (__attribute__((address_space(3))) void *)&buf[R.base + R.OD], 4, voff, 0, 0, 2);
        }
        if (R.nD <= kWave) return;
        const uint32_t x1 = (uint32_t)(x00 + 256);  // > 0
        uint32_t r = (uint32_t)__builtin_fmaf((float)x1, inv, hinv);
        int32_t rem = (int32_t)(x1 - r * S);  // in [0, S)
        uint32_t voff = x1 - pre * r - 4 + R.ph;
        const uint32_t q = 256 / S;
        const int32_t dq = 256 - (int32_t)(q * S);      // in [0, S)
        const uint32_t dv = 256 - pre * q;              // source step when the record steps by q
        for (uint32_t i = 1; i * kWave < R.nD; i++) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rs, (__attribute__((address_space(3))) void *)&buf[R.base + R.OD + i * kWave], 4,
                voff, 0, 0, 2);
            rem += dq;
            const bool c = rem >= (int32_t)S;
            rem = c ? rem - (int32_t)S : rem;
            voff += c ? dv - pre : dv;
        }
        return;
    }
    mask[lane] = 0;  // kGatherMaskWords == kWave
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    if (lane >= 1 && lane < R.cnt) {
        const uint32_t et = (R.P + R.ph + 3) >> 2;
        atomicOr(&mask[et >> 5], 1u << (et & 31));
    }
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    const uint32_t mv = mask[lane];
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    uint32_t rb = 0;
    for (uint32_t i = 0; i * kWave < R.nD; i++) {
        const int32_t x0 = 256 * (int32_t)i + 4 * (int32_t)lane - (int32_t)R.ph;
        const uint64_t M = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(mv, 2 * i + 1) << 32 |
                           (uint32_t)__builtin_amdgcn_readlane(mv, 2 * i);
        const uint32_t r = rb + mbcnt(M) + (uint32_t)((M >> lane) & 1);
        rb += (uint32_t)__builtin_popcountll(M);
        const uint32_t voff = (uint32_t)(x0 - (int32_t)(pre * r) - 4 + (int32_t)R.ph);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void *)&buf[R.base + R.OD + i * kWave], 4, voff,
            0, 0, 2);
    }
}

// After the gather landed: the fixed fields, then the aligned 16-byte stores
// (chunk-edge segments by dwords where whole and bytes at the ends).  Image
// bytes are written once and not read back by this call: nt stores (config
// 3: 288 -> 275 us per call, as the filter words and the views' data regions).
template <int G>
__device__ __forceinline__ void region_finish(const RegionPlan &R, uint32_t *buf) {
    const uint32_t lane = lane_id();
    uint8_t *ob = reinterpret_cast<uint8_t *>(buf + R.base + R.OD) + R.ph;
    if (lane < R.cnt) {
        // dword stores where the field is dword-aligned in LDS (fixed-size
        // records of a multiple of 4 bytes: every record), bytes otherwise
        const uint32_t A = R.ph + R.P;
        if ((A & 3) == 0) *reinterpret_cast<uint32_t *>(ob + R.P) = R.len;
        else {
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) ob[R.P + b] = (uint8_t)(R.len >> (8 * b));
        }
        if (G == LSM_GRAMMAR_IDX) {
            if (((A + R.len) & 3) == 0) {
                uint32_t *o = reinterpret_cast<uint32_t *>(ob + R.P + 4 + R.len);
                o[0] = (uint32_t)R.xo;
                o[1] = (uint32_t)(R.xo >> 32);
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 8; b++) ob[R.P + 4 + R.len + b] = (uint8_t)(R.xo >> (8 * b));
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
    gptr_t<u32x4> dA = gbl_at<u32x4>(reinterpret_cast<uintptr_t>(R.dst) - R.head);
    const uint32_t nseg = (R.head + R.tot + 15) >> 4;
    const uint32_t *img = buf + R.base;
    const uint32_t q0 = R.OD + (uint32_t)(((int32_t)R.ph - (int32_t)R.head - (int32_t)R.sh) >> 2);
    const int32_t tot = (int32_t)R.tot;
    for (uint32_t e = lane; e < nseg; e += kWave) {
        const int32_t u0 = 16 * (int32_t)e - (int32_t)R.head;
        if (u0 >= 0 && u0 + 16 <= tot) {
            const uint32_t q = q0 + 4 * e;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(&img[q]);
            u32x4 o = v;
            if (R.sh) {  // wave-uniform: source and image share their dword phase otherwise
                const uint32_t v4 = img[q + 4];
                o.x = funnel(v.x, v.y, R.sh);
                o.y = funnel(v.y, v.z, R.sh);
                o.z = funnel(v.z, v.w, R.sh);
                o.w = funnel(v.w, v4, R.sh);
            }
            __builtin_nontemporal_store(o, &dA[e]);
        } else {
            gptr_t<uint8_t> db = (gptr_t<uint8_t>)(dA + e);
            for (uint32_t k = 0; k < 4; k++) {
                const int32_t u = u0 + 4 * (int32_t)k;
                if (u >= 0 && u + 4 <= tot) {
                    const uint32_t q = q0 + 4 * e + k;
                    *(gptr_t<uint32_t>)(db + 4 * k) = funnel(img[q], img[q + 1], R.sh);
                } else {
                    for (uint32_t b = 0; b < 4; b++)
                        if (u + (int32_t)b >= 0 && u + (int32_t)b < tot) db[4 * k + b] = ob[u + b];
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __asm__ __volatile__("" ::: "memory");
}

// WithV = false (lsm_build_sst_views: the data region comes from the value
// views' kernel): the buffer holds only the IDX image, 4 instead of 9.5 KiB
// per wave, so a CU holds twice the waves (compaction 1.031-1.037 -> 1.018 ms
// per call, A/B; the data region straight from the values arena without the
// LDS image measured 0.250 -> 0.332 ms per config-3 build and is not used).
// Desc (the stream build): the grid is one dimension of spans and each file's
// layout comes precomputed in one 64-byte FileDesc (two dependent scalar
// loads per wave instead of sst_layout's eight loads and its 64-bit
// arithmetic: a wave writes one chunk, so this setup is paid per chunk).
template <bool WithV, bool Desc>
__global__ __launch_bounds__(kRegWaves *kWave) void sst_regions_kernel(SstArgs a) {
    constexpr uint32_t BD = WithV ? kRegBufDwords : kRegIdxDwords;
    __shared__ __attribute__((aligned(16))) uint32_t lds[kRegWaves][BD + kGatherMaskWords];
    const uint32_t wave = uni(threadIdx.x / kWave);
    SstLayout L;
    uint64_t c0, imgo, Ks, Vs, K0;
    if (Desc) {
        // span j's file: j / the common span count when every file but the
        // last has it (files of one record size: no table), else the table
        const uint32_t j = blockIdx.x, nf = a.plan[0], nsp = a.plan[2];
        if (j >= a.plan[1]) return;
        const uint32_t f = nsp ? min(j / nsp, nf - 1) : a.span_file[j];
        const FileDesc D = a.desc[f];
        L.s = D.s;
        L.e = D.e;
        L.data_off = D.data_off;
        L.idx_off = D.idx_off;
        c0 = D.s + (uint64_t)(blockIdx.x - D.span0) * kRegSpanRecs + (uint64_t)wave * kRegWaveChunks * kWave;
        imgo = D.img;
        Ks = D.Ks;
        Vs = D.Vs;
        K0 = 0;  // the stream starts at record 0
    } else {
        const uint32_t f = blockIdx.x;
        L = sst_layout(a, f);
        c0 = L.s + (uint64_t)blockIdx.y * kRegSpanRecs + (uint64_t)wave * kRegWaveChunks * kWave;
        imgo = uni64(a.file_off[f]);
        Ks = uni64(a.koff[L.s]);
        Vs = uni64(a.voff[L.s]);
        K0 = a.hrec ? uni64(a.file_start[0]) : 0;
    }
    if (c0 >= L.e) return;
    const uint64_t cend = L.e - c0 < (uint64_t)kRegWaveChunks * kWave ? L.e : c0 + kRegWaveChunks * kWave;
    uint32_t *buf = lds[wave];
    uint32_t *mask = buf + BD;
    uint8_t *img = a.out + imgo;
    auto count = [&](uint64_t c) { return (uint32_t)(cend - c < (uint64_t)kWave ? cend - c : kWave); };
    ChunkOffs off = load_offs(a, c0, count(c0));
    for (;;) {
        const uint32_t cnt = count(c0);
        const uint64_t rel = c0 - L.s;
        const uint64_t Vc = lane64(off.v0, 0), Kc = lane64(off.k0, 0);
        uint8_t *dV = img + L.data_off + 4 * rel + (Vc - Vs);
        uint8_t *dI = img + L.idx_off + 12 * rel + (Kc - Ks);
        // IDX offset of record i: data_off + 4 (i - s) + V(i) - V(s) (sstable.go:164-175)
        const int64_t xo_base = (int64_t)L.data_off + (int64_t)(4 * rel) - (int64_t)Vs;
        RegionPlan pv, pi;
        bool ok = true;
        uint32_t ibase = 0;
        if (WithV) {
            ok = region_plan<LSM_GRAMMAR_V>(pv, off, cnt, dV, 0, BD, 0);
            ibase = (pv.OD + pv.nD + 8 + 63) & ~63u;
        }
        ok = ok && region_plan<LSM_GRAMMAR_IDX>(pi, off, cnt, dI, ibase, BD, xo_base);
        const uint64_t cn = c0 + kWave;
        const bool more = cn < cend;
        if (ok) {
            if (WithV) region_issue<LSM_GRAMMAR_V>(pv, buf, mask, a.vals);
            region_issue<LSM_GRAMMAR_IDX>(pi, buf, mask, a.keys);
            const ChunkOffs nxt = more ? load_offs(a, cn, count(cn)) : off;
            // The DMA writes are invisible to the compiler's LDS tracking.
            __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");
            if (WithV) region_finish<LSM_GRAMMAR_V>(pv, buf);
            region_finish<LSM_GRAMMAR_IDX>(pi, buf);
            if (a.hrec && lane_id() < cnt) {
                // Filter.Add's key hash (bloom.go:175-181) from the key
                // already gathered into the IDX image, while its stores drain
                const uint32_t A = 4 * (pi.base + pi.OD) + pi.ph + pi.P + 4;
                const uint32_t q = A >> 2;
                const uint32_t x0 = buf[q], x1 = buf[q + 1], x2 = buf[q + 2], x3 = buf[q + 3],
                               x4 = buf[q + 4];
                const uint64_t f0 = (uint64_t)funnel(x1, x2, A) << 32 | funnel(x0, x1, A);
                const uint64_t f1 = (uint64_t)funnel(x3, x4, A) << 32 | funnel(x2, x3, A);
                uint64_t h[4];
                sum256_pre(a.keys + off.k0, pi.len, f0, f1, h);
                store_hash_rec(h, a.hm, a.hrl, a.hrh, a.hrec + kHashRecDwords * (c0 + lane_id() - K0));
            }
            off = nxt;
        } else {
            // a chunk with records too large for one buffer: region by region
            RegionSrc S;
            S.keys = a.keys; S.koff = a.koff; S.vals = a.vals; S.voff = a.voff;
            S.idx_off = nullptr;
            S.idx_base = (int64_t)L.data_off;
            S.rs = L.s;
            S.vrs = Vs;
            ChunkTable *ct = reinterpret_cast<ChunkTable *>(buf);
            if (WithV) encode_chunk_any<LSM_GRAMMAR_V, kRegMaxImage>(S, c0, cnt, dV, buf, nullptr, ct);
            encode_chunk_any<LSM_GRAMMAR_IDX, (WithV ? kRegMaxImage : kRegIdxDwords)>(S, c0, cnt, dI, buf, nullptr, ct);
            if (a.hrec && lane_id() < cnt) {
                uint64_t h[4];
                sum256(a.keys + off.k0, off.k1 - off.k0, h);
                store_hash_rec(h, a.hm, a.hrl, a.hrh, a.hrec + kHashRecDwords * (c0 + lane_id() - K0));
            }
            if (more) off = load_offs(a, cn, count(cn));
        }
        if (!more) break;
        c0 = cn;
    }
}

// ---- builder rule on the device (lsm_segment_files / lsm_build_sst_stream) --
//
// Builder.Add sums EstimateSize = 16 + key + value bytes (kv.go:118-121) and
// the driver flushes once the sum reaches the threshold (builder.go:40-42,
// merge.go:118-121); the leftovers make a last file (merge.go:125-128).
// With S(t) = 16 t + koff[t] + voff[t] (strictly increasing), the file after
// a file starting at s starts at next(s) = the smallest t in (s, n] with
// S(t) - S(s) >= T, or n when no t reaches it.  The starts are the orbit of 0
// under next(), a serial chain; one workgroup resolves it in rounds:
//  * from the exact start `cur`, slot i of the round predicts file i's start
//    at cur + i G (G = the records per file seen so far) and computes next()
//    there exactly (a galloping search seeded at the prediction + G: one
//    round trip when the prediction holds);
//  * W = 1 (1,024 slots): slot i is verified when every earlier slot's next()
//    equals the following slot's prediction (a min-reduction finds the first
//    break; for records of one size every prediction holds and one round
//    resolves every file);
//  * W = 32 (32 slots of 32 window positions): after a break, positions
//    around each prediction, and one thread walks the chain through the
//    windows; a full walk returns to W = 1.
// Every file start written is exact: a slot's next() is only used once the
// slot's own position is known to be a start.  Then, in the same launch, the
// image layout (sizes, 16-byte aligned offsets, lsm_sst_layout's) and, for
// the build, each file's FileDesc and the span table of the region writer.
constexpr uint32_t kSegThreads = 1024;
constexpr uint32_t kSegWin = 32;
constexpr uint32_t kSegLdsFiles = 4096;  // file starts kept in LDS for the layout
constexpr uint64_t kSegNone = ~0ull;

struct StreamPlanArgs {
    const uint64_t *koff, *voff;
    uint64_t n, T;
    uint32_t nfile_max, span_max;
    uint64_t filter_bytes, align;
    uint64_t *file_start;  // nfile_max + 1
    uint64_t *file_off;    // nfile_max + 1, or null (the rule alone)
    FileDesc *desc;        // nfile_max, or null
    uint32_t *span_file;   // span_max, or null
    uint32_t *plan;        // 4: {nfile, spans, the common span count or 0, 0}
    uint64_t *counts;      // {nfile, most records in a file, image bytes, overflow}
};

// The plan kernel's barrier: LDS only.  A __syncthreads() also waits for
// the workgroup's global stores to complete (its release fence): after the
// file starts, descriptors and span table were stored that cost ~3.5 us per
// launch.  Global data one thread wrote and another reads back (file starts
// past kSegLdsFiles) takes a __syncthreads() of its own.
__device__ __forceinline__ void seg_barrier() {
    __asm__ __volatile__("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

struct SegPair {
    uint64_t s, c;
};

// Exclusive sums of two values over the plan kernel's 1,024 threads.
__device__ __forceinline__ SegPair seg_block_scan2(uint64_t s, uint64_t c, SegPair *total) {
    constexpr uint32_t NW = kSegThreads / kWave;
    __shared__ uint64_t ws_[NW], wc_[NW];
    uint64_t ts, tc;
    const uint64_t xs = wave_excl_scan64(s, &ts), xc = wave_excl_scan64(c, &tc);
    const uint32_t w = threadIdx.x / kWave;
    if (lane_id() == 0) {
        ws_[w] = ts;
        wc_[w] = tc;
    }
    seg_barrier();
    uint64_t ps = 0, pc = 0, as = 0, ac = 0;
    for (uint32_t i = 0; i < NW; i++) {
        if (i < w) {
            ps += ws_[i];
            pc += wc_[i];
        }
        as += ws_[i];
        ac += wc_[i];
    }
    seg_barrier();
    *total = SegPair{as, ac};
    return SegPair{ps + xs, pc + xc};
}

// The largest value over the wave (lane 0 holds it, as every lane).
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t o = (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d) << 32 |
                           (uint32_t)__shfl_xor((int)(uint32_t)v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t est_at(const uint64_t *koff, const uint64_t *voff, uint64_t t) {
    return 16 * t + koff[t] + voff[t];
}

// next(p) for p < n with S(n) >= S(p) + T known: the smallest t in (p, n]
// with S(t) >= target, searched from `guess` by galloping, then bisection.
__device__ uint64_t seg_next(const uint64_t *koff, const uint64_t *voff, uint64_t p, uint64_t n,
                             uint64_t target, uint64_t guess) {
    uint64_t lo = p + 1, hi = n;  // the answer is in [lo, hi]; S(hi) >= target
    const uint64_t g = guess < lo ? lo : (guess > hi ? hi : guess);
    {
        // S(g - 1) and S(g) in one round trip: the prediction holds when
        // they bracket the target
        const uint64_t a = g > lo ? est_at(koff, voff, g - 1) : 0;
        const uint64_t b = est_at(koff, voff, g);
        if (b >= target) {
            if (g == lo || a < target) return g;
            hi = g - 1;  // S(g - 1) >= target
            uint64_t d = 1;
            for (;;) {  // gallop down
                const uint64_t x = hi - lo > d ? hi - d : lo;
                if (est_at(koff, voff, x) >= target) {
                    hi = x;
                    if (x == lo) return lo;
                    d <<= 1;
                } else {
                    lo = x + 1;
                    break;
                }
            }
        } else {
            lo = g + 1;
            uint64_t d = 1;
            while (lo < hi) {  // gallop up
                const uint64_t x = hi - lo > d ? lo + d - 1 : hi;
                if (est_at(koff, voff, x) >= target) {
                    hi = x;
                    break;
                }
                lo = x + 1;
                d <<= 1;
            }
        }
    }
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (est_at(koff, voff, mid) >= target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kSegThreads) void sst_stream_plan_kernel(StreamPlanArgs a) {
    __shared__ uint64_t s_pos[kSegThreads], s_nxt[kSegThreads];
    __shared__ uint64_t s_fs[kSegLdsFiles + 1];  // the first file starts, for the layout
    __shared__ uint64_t s_cur, s_G;
    __shared__ uint32_t s_nf, s_W, s_brk, s_over;
    __shared__ uint64_t s_carry, s_scarry, s_maxr;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.n, T = a.T;
    // every thread reads the stream's ends itself (the same lines: no round
    // trip through thread 0 and a barrier); koff[n - 1] for the last file's
    // layout
    const uint64_t kn = n ? a.koff[n] : 0, vn = n ? a.voff[n] : 0, knm = n ? a.koff[n - 1] : 0;
    const uint64_t Sn = 16 * n + kn + vn;
    const uint64_t S0 = n ? est_at(a.koff, a.voff, 0) : 0;
    // Round 1 (W = 1) leaves slot tid's file layout inputs in registers --
    // koff at the file's first two and last two records, voff at its ends --
    // so that when that round resolves every file (records of one size) the
    // layout below reads nothing: thread tid is file tid's slot and its
    // layout thread.
    uint64_t rk0 = 0, rk01 = 0, rk1m = 0, rk1 = 0, rv0 = 0, rv1 = 0;
    bool rhave = false;
    uint32_t rounds = 0;
    if (tid == 0) {
        s_cur = 0;
        s_nf = 0;
        s_W = 1;
        s_over = 0;
        // records per file if every record had the mean size
        const uint64_t tot = Sn - S0;
        const double g = tot ? ceil((double)T * (double)n / (double)tot) : 1.0;
        s_G = g < 1.0 ? 1 : (g > 4.0e18 ? (uint64_t)4e18 : (uint64_t)g);
    }
    seg_barrier();
    if (n && T == 0) {  // never flush (BuildSSTableFromIMemTable): one file
        if (tid == 0) {
            if (a.nfile_max >= 1) {
                a.file_start[0] = 0;
                s_fs[0] = 0;
                s_nf = 1;
            } else {
                s_over = 1;
            }
            s_cur = n;
        }
        seg_barrier();
    }
    for (;;) {
        const uint64_t cur = s_cur;
        const uint32_t nf = s_nf;
        if (cur >= n || s_over) break;
        const uint32_t W = s_W, R = kSegThreads / W;
        const uint64_t G = s_G;
        const uint32_t i = tid / W, w = tid % W;
        uint64_t P = kSegNone;
        if (i == 0) {
            if (w == 0) P = cur;
        } else {
            const uint64_t c = cur + (uint64_t)i * G;  // may exceed n: no slot
            const uint64_t h = W / 2;
            if (c >= h && c - h + w > cur && c - h + w < n) P = c - h + w;
        }
        uint64_t nx = kSegNone;
        if (P != kSegNone) {
            // S(P) and the predicted end's bracket S(g - 1), S(g) in one
            // round trip (T > 0 here, so S(P) < target: g = P + 1 is covered)
            const uint64_t g = P + G < n ? P + G : n;
            const uint64_t kp = a.koff[P], vp = a.voff[P], kp1 = a.koff[P + 1];
            const uint64_t kg1 = a.koff[g - 1], vg1 = a.voff[g - 1], kg = a.koff[g], vg = a.voff[g];
            const uint64_t sp = 16 * P + kp + vp;
            const uint64_t sa = 16 * (g - 1) + kg1 + vg1, sb = 16 * g + kg + vg;
            const uint64_t target = sp + T;
            const bool bracket = sb >= target && sa < target;
            nx = Sn < target ? n : (bracket ? g : seg_next(a.koff, a.voff, P, n, target, g));
            if (rounds == 0 && W == 1) {
                rk0 = kp;
                rk01 = kp1;
                rv0 = vp;
                // the file's end: the bracket's g, or the stream's end
                rhave = Sn < target || bracket;
                rk1m = Sn < target ? knm : kg1;
                rk1 = Sn < target ? kn : kg;
                rv1 = Sn < target ? vn : vg;
            }
        }
        s_pos[tid] = P;
        s_nxt[tid] = nx;
        if (tid == 0) s_brk = R - 1;
        seg_barrier();
        uint32_t adv = 0;  // files whose start this round resolved
        uint64_t ncur = cur;
        if (W == 1) {
            // slot tid is the chain's last of this round if its next() is
            // not slot tid + 1's prediction (or ends the stream, or the slot
            // has no position); the first such slot by a ballot per wave and
            // one LDS atomic per wave (an atomic per thread serialized ~800
            // of them on one address: 3 us)
            const bool brk = tid < R - 1 && (s_nxt[tid] == kSegNone || s_nxt[tid] >= n ||
                                             s_nxt[tid] != s_pos[tid + 1]);
            const uint64_t bb = __ballot(brk);
            if (bb && lane_id() == 0) atomicMin(&s_brk, (tid & ~(kWave - 1)) + (uint32_t)__builtin_ctzll(bb));
            seg_barrier();
            const uint32_t J = s_brk;  // slots 0 .. J are starts; slot J's next() is exact
            adv = J + 1;
            ncur = s_nxt[J];
            if (nf + adv > a.nfile_max) {
                if (tid == 0) s_over = 1;
            } else if (tid <= J) {
                a.file_start[nf + tid] = s_pos[tid];
                if (nf + tid <= kSegLdsFiles) s_fs[nf + tid] = s_pos[tid];
            }
        } else {
            if (tid == 0) {
                uint64_t c = cur;
                uint32_t k = nf;
                for (uint32_t j = 0; j < R && c < n; j++) {
                    uint64_t x = kSegNone;
                    if (j == 0) {
                        x = s_nxt[0];
                    } else {
                        const uint64_t lo = cur + (uint64_t)j * G - W / 2;
                        if (cur + (uint64_t)j * G >= W / 2 && c >= lo && c - lo < W) x = s_nxt[j * W + (c - lo)];
                    }
                    if (x == kSegNone) break;  // c is a start, next(c) not in the window
                    if (k >= a.nfile_max) {
                        s_over = 1;
                        break;
                    }
                    if (k <= kSegLdsFiles) s_fs[k] = c;
                    a.file_start[k++] = c;
                    c = x;
                }
                s_brk = k - nf;
                s_pos[0] = c;
            }
            seg_barrier();
            adv = s_brk;
            ncur = s_pos[0];
        }
        seg_barrier();
        if (tid == 0) {
            if (adv) {
                const uint64_t g = (ncur - cur + adv / 2) / adv;  // mean records per file
                s_G = g ? g : 1;
            }
            s_W = (W == 1 && adv < R && ncur < n) ? kSegWin : (W > 1 && adv == R ? 1 : W);
            s_cur = ncur;
            s_nf = nf + adv;
        }
        rounds++;
        seg_barrier();
    }
    // the registers hold file tid's inputs when round 1 resolved every file
    rhave = rhave && rounds == 1 && s_cur >= n && !s_over;
    const uint32_t nfile = s_over ? 0 : s_nf;
    if (!a.file_off && nfile > kSegLdsFiles) __syncthreads();  // as below, for the rule alone
    if (tid == 0) {
        a.file_start[nfile] = n;
        if (nfile <= kSegLdsFiles) s_fs[nfile] = n;
        a.counts[0] = nfile;
        a.counts[3] = s_over;
        s_carry = 0;
        s_scarry = 0;
        s_maxr = 0;
    }
    seg_barrier();
    if (!a.file_off) {
        // the rule alone: the most records in one file
        uint64_t mr = 0;
        for (uint32_t f = tid; f < nfile; f += kSegThreads) {
            const uint64_t r = (f + 1 <= kSegLdsFiles ? s_fs[f + 1] : a.file_start[f + 1]) -
                               (f <= kSegLdsFiles ? s_fs[f] : a.file_start[f]);
            mr = r > mr ? r : mr;
        }
        mr = wave_max64(mr);  // one LDS atomic per wave, not per thread
        if (lane_id() == 0 && mr) atomicMax((unsigned long long *)&s_maxr, (unsigned long long)mr);
        seg_barrier();
        if (tid == 0) {
            a.counts[1] = s_maxr;
            a.counts[2] = 0;
        }
        return;
    }
    seg_barrier();
    if (nfile > kSegLdsFiles) __syncthreads();  // the later file starts are read back from global memory
    // layout: sizes, aligned offsets, FileDesc, span starts (tile after tile)
    __shared__ uint32_t s_nsp0, s_nonuni;
    if (tid == 0) s_nonuni = 0;
    for (uint32_t f0 = 0; f0 < nfile; f0 += kSegThreads) {
        const uint32_t f = f0 + tid;
        uint64_t sz = 0, nr = 0, r0 = 0, r1 = 0, k0 = 0, k1 = 0, v0 = 0, v1 = 0, hdr = 8;
        if (f < nfile) {
            r0 = f <= kSegLdsFiles ? s_fs[f] : a.file_start[f];
            r1 = f + 1 <= kSegLdsFiles ? s_fs[f + 1] : a.file_start[f + 1];
            nr = r1 - r0;
            uint64_t k01, k1m;
            if (f0 == 0 && rhave) {  // round 1's registers (thread tid = file tid)
                k0 = rk0;
                k01 = rk01;
                k1m = rk1m;
                k1 = rk1;
                v0 = rv0;
                v1 = rv1;
            } else {
                k0 = a.koff[r0];
                k01 = a.koff[r0 + 1];
                k1m = a.koff[r1 - 1];
                k1 = a.koff[r1];
                v0 = a.voff[r0];
                v1 = a.voff[r1];
            }
            hdr += (k01 - k0) + (k1 - k1m);  // nr >= 1
            // Header | Filter | V region (4 + vlen) | IDX region (4 + klen + 8) | Footer
            sz = hdr + a.filter_bytes + 4 * nr + (v1 - v0) + 12 * nr + (k1 - k0) + 32;
        }
        const uint64_t nsp = (nr + kRegSpanRecs - 1) / kRegSpanRecs;
        if (f == 0) s_nsp0 = (uint32_t)nsp;
        SegPair tot;
        const SegPair x = seg_block_scan2((sz + a.align - 1) / a.align * a.align, nsp, &tot);
        if (f < nfile) {
            const uint64_t off = s_carry + x.s;
            a.file_off[f] = off;
            FileDesc D;
            D.s = r0;
            D.e = r1;
            D.img = off;
            D.data_off = hdr + a.filter_bytes;
            D.idx_off = D.data_off + 4 * nr + (v1 - v0);
            D.Ks = k0;
            D.Vs = v0;
            D.span0 = (uint32_t)(s_scarry + x.c);
            D.pad = 0;
            a.desc[f] = D;
        }
        const uint64_t wm = wave_max64(nr);  // one LDS atomic per wave
        if (lane_id() == 0 && wm) atomicMax((unsigned long long *)&s_maxr, (unsigned long long)wm);
        // every file but the last of one span count: the region writer's span
        // j is then file j / that count, no table (s_nsp0 was set before the
        // scan's barriers)
        const uint64_t nu = __ballot(f + 1 < nfile && nsp != s_nsp0);
        if (nu && lane_id() == 0) s_nonuni = 1;
        seg_barrier();
        if (tid == 0) {
            s_carry += tot.s;
            s_scarry += tot.c;
        }
        seg_barrier();
    }
    if (s_nonuni) {
        // files of several span counts: the span table, one wave per file
        // (lane-strided stores), from the descriptors just written
        __syncthreads();
        const uint32_t wv = tid / kWave, nw = kSegThreads / kWave;
        for (uint32_t g = wv; g < nfile; g += nw) {
            const uint32_t b0 = a.desc[g].span0;
            const uint32_t b1 = g + 1 < nfile ? a.desc[g + 1].span0 : (uint32_t)s_scarry;
            for (uint32_t j = b0 + lane_id(); j < b1; j += kWave) a.span_file[j] = g;
        }
    }
    if (tid == 0) {
        a.file_off[nfile] = s_carry;
        a.counts[1] = s_maxr;
        a.counts[2] = s_carry;
        // the region writer's grid header: files, spans, the span count of
        // every file but the last (0: look spans up in the table)
        a.plan[0] = nfile;
        a.plan[1] = (uint32_t)s_scarry;
        a.plan[2] = s_nonuni ? 0u : s_nsp0;
        a.plan[3] = 0;
    }
}

// Data region (V grammar, sstable.go:159-175) of file blockIdx.x straight
// from value views: record j of the batch is [u32 vlen][value], its value at
// bytes + view(idx[j]) (a V descriptor, or the value of a KV descriptor).
// One wave per 64 records: their records form one contiguous output range
// [A, B), written a dword per lane per step (256 coalesced bytes per store
// instruction).  An LDS map gives each output dword the record holding its
// first byte; the dword is assembled from that record's prefix and value
// bytes and, where the record ends inside it, the next record's prefix (a
// record is at least its 4-byte prefix, so no dword spans three records).
// Only the two dwords cut by A and B are written a byte at a time (the
// neighbouring waves own their other bytes).  kVvMap dwords per pass.
struct VViewArgs {
    const uint8_t *bytes;
    const u32x4 *kd, *vd;  // vd == null: KV descriptors (value after the key)
    const uint32_t *idx;
};
constexpr uint32_t kVvMap = 2048;
constexpr uint32_t kVvUnroll = 8;

__device__ __forceinline__ void vv_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void sst_vregion_views_kernel(SstArgs a, VViewArgs v) {
    constexpr uint32_t W = kSstWaves;
    __shared__ uint64_t s_dst[W][kWave + 1];  // output offset of record r's length prefix
    __shared__ uint64_t s_src[W][kWave];      // source offset of its value bytes
    __shared__ uint32_t s_vl[W][kWave];
    __shared__ uint8_t s_map[W][kVvMap];
    const uint32_t f = blockIdx.x, w = threadIdx.x / kWave, lane = lane_id();
    const SstLayout L = sst_layout(a, f);
    const uint64_t c0 = L.s + (uint64_t)blockIdx.y * kSstChunkRecs + (uint64_t)w * kWave;
    if (c0 >= L.e) return;
    const uint32_t cnt = (uint32_t)((L.e - c0) < (uint64_t)kWave ? (L.e - c0) : kWave);
    const uint64_t Vs = uni64(a.voff[L.s]);
    // record j's prefix at out + rbase + 4 j + voff[j]
    const uint64_t rbase = uni64(a.file_off[f]) + L.data_off - 4 * L.s - Vs;
    uint64_t d0 = 0, d1 = 0;
    if (lane < cnt) {
        const uint64_t j = c0 + lane;
        const uint32_t i = v.idx[j];
        const u32x4 k = v.kd[i];
        uint64_t src;
        uint32_t vl;
        if (v.vd) {
            const u32x4 d = v.vd[i];
            src = ((uint64_t)d.y << 32 | d.x) + 4;
            vl = d.w;
        } else {
            src = ((uint64_t)k.y << 32 | k.x) + 8 + k.z;
            vl = k.w;
        }
        d0 = rbase + 4 * j + a.voff[j];
        d1 = d0 + 4 + vl;
        s_dst[w][lane] = d0;
        s_src[w][lane] = src;
        s_vl[w][lane] = vl;
    }
    if (lane == 0) s_dst[w][cnt] = rbase + 4 * (c0 + cnt) + a.voff[c0 + cnt];
    vv_sync();
    const uint64_t A = s_dst[w][0], B = s_dst[w][cnt], X = A & ~(uint64_t)3;
    const uint64_t ndw = (B - X + 3) / 4;
    const gptr_t<uint8_t> out = gbl(a.out);
    const gptr_t<const uint8_t> vb = gbl(v.bytes);
    for (uint64_t P = 0; P < ndw; P += kVvMap) {
        const uint32_t np = (uint32_t)(ndw - P < kVvMap ? ndw - P : kVvMap);
        // 1. dwords whose first byte lies in my record
        if (lane < cnt) {
            const uint64_t lo = (d0 - X + 3) / 4, hi = (d1 - 1 - X) / 4;
            const uint64_t c_lo = lo > P ? lo : P;
            const uint64_t c_hi = hi < P + np - 1 ? hi : P + np - 1;
            for (uint64_t c = c_lo; c <= c_hi; c++) s_map[w][c - P] = (uint8_t)lane;
        }
        vv_sync();
        // 2. kVvUnroll dwords per lane per step, every load issued before
        //    the first is used (the step is one load latency, not kVvUnroll)
        for (uint32_t cb = 0; cb < np; cb += kWave * kVvUnroll) {
            uint32_t q0[kVvUnroll], q1[kVvUnroll], o_[kVvUnroll], r_[kVvUnroll];
            bool ok[kVvUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kVvUnroll; u++) {
                const uint32_t c = cb + u * kWave + lane;
                const uint64_t x = X + 4 * (P + c);
                ok[u] = c < np && x >= A && x + 4 <= B;
                const uint32_t r = ok[u] ? s_map[w][c] : 0;
                const uint32_t o = ok[u] ? (uint32_t)(x - s_dst[w][r]) : 4;  // byte o of record r
                const uintptr_t sa = reinterpret_cast<uintptr_t>(v.bytes + s_src[w][r] + (o >= 4 ? o - 4 : 0));
                const gptr_t<const uint32_t> q = gbl_at<const uint32_t>(sa & ~(uintptr_t)3);
                q0[u] = q[0];
                q1[u] = q[1];
                o_[u] = o;
                r_[u] = r;
            }
#pragma unroll
            for (uint32_t u = 0; u < kVvUnroll; u++) {
                if (!ok[u]) continue;
                const uint32_t c = cb + u * kWave + lane, r = r_[u], o = o_[u];
                const uint64_t x = X + 4 * (P + c);
                const uintptr_t sa = reinterpret_cast<uintptr_t>(v.bytes + s_src[w][r] + (o >= 4 ? o - 4 : 0));
                uint32_t val = funnel(q0[u], q1[u], (uint32_t)sa);
                if (o < 4) val = (s_vl[w][r] >> (8 * o)) | (o ? val << (32 - 8 * o) : 0);
                const uint32_t k = (uint32_t)(s_dst[w][r + 1] - x);  // bytes left in record r
                if (k < 4) val = (val & ((1u << (8 * k)) - 1)) | (s_vl[w][r + 1] << (8 * k));
                *(gptr_t<uint32_t>)(out + x) = val;
            }
        }
        // 3. the dwords cut by A and B, a byte at a time
        if (lane < 2) {
            const uint64_t c = lane == 0 ? 0 : ndw - 1;
            const uint64_t x = X + 4 * c;
            if (c >= P && c < P + np && (x < A || x + 4 > B)) {
                uint32_t r = x >= A ? cnt - 1 : 0;
                for (uint32_t u = 0; u < 4; u++) {
                    const uint64_t b = x + u;
                    if (b < A || b >= B) continue;
                    while (b >= s_dst[w][r + 1]) r++;
                    const uint64_t t = b - s_dst[w][r];  // byte t of record r
                    out[b] = t < 4 ? (uint8_t)(s_vl[w][r] >> (8 * t))
                                   : vb[s_src[w][r] + (t - 4)];
                }
            }
        }
        vv_sync();
    }
}

// The same data region when the values are V descriptors of decoded data
// regions (lsm_decode_sst's data_desc): a V record [u32 vlen][value] is
// byte-identical to the source record its descriptor points at (rec_off is
// the record's own length prefix, the grammar is the same), so the output is
// a segmented copy of source records (a descriptor whose source prefix does
// not hold its length -- any caller-made view -- gets its prefix from the
// descriptor instead, as a run of its own).  Consecutive records that were
// consecutive in their source (a run: every stretch of pairs taken from one
// input file) are one shifted memcpy.  One wave per 64 records: lanes mark
// where their record does not continue the previous lane's source, the runs
// (output start, source start) go to LDS, and each lane then writes whole
// 16-byte output segments: the segment's run by a binary search over the
// runs, a dword-aligned 16-byte source load and the dword after it
// funnel-shifted into one 16-byte store (multi-dword global loads need only
// dword alignment; two 16-byte-aligned loads and a dword select by the shift:
// 1.148 -> 1.113 ms per compaction, A/B).  Segments that straddle a run boundary are assembled byte by byte;
// the two segments cut by the wave's range [A, B) are written a byte at a
// time (the neighbouring waves own their other bytes).
constexpr uint32_t kVrUnroll = 4;  // segments per lane in flight
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned

__global__ __launch_bounds__(256) void sst_vregion_runs_kernel(SstArgs a, VViewArgs v) {
    constexpr uint32_t W = kSstWaves;
    __shared__ uint64_t s_d[W][kWave + 1];  // run q's first output byte - A; [nrun] = B - A
    __shared__ uint64_t s_in[W][kWave];     // run q's first source byte
    __shared__ uint32_t s_fix[W][kWave];    // run q's prefix from the descriptor: vlen + 1, or 0
    __shared__ uint32_t s_slow[W][2 * kWave + 4];  // segments not inside one run
    const uint32_t f = blockIdx.x, w = threadIdx.x / kWave, lane = lane_id();
    const SstLayout L = sst_layout(a, f);
    const uint64_t c0 = L.s + (uint64_t)blockIdx.y * kSstChunkRecs + (uint64_t)w * kWave;
    if (c0 >= L.e) return;
    const uint32_t cnt = (uint32_t)((L.e - c0) < (uint64_t)kWave ? (L.e - c0) : kWave);
    const uint64_t Vs = uni64(a.voff[L.s]);
    // record j's prefix at out + rbase + 4 j + voff[j]
    const uint64_t rbase = uni64(a.file_off[f]) + L.data_off - 4 * L.s - Vs;
    uint64_t d0 = 0, in0 = 0, in1 = 0;
    uint32_t vl = 0;
    bool bad = false;
    if (lane < cnt) {
        const uint64_t j = c0 + lane;
        const u32x4 d = v.vd[v.idx[j]];
        in0 = (uint64_t)d.y << 32 | d.x;  // the record's length prefix
        vl = d.w;
        in1 = in0 + 4 + vl;
        d0 = rbase + 4 * j + a.voff[j];
        const gptr_t<const uint8_t> pb = gbl(v.bytes) + in0;
        bad = ((uint32_t)pb[0] | (uint32_t)pb[1] << 8 | (uint32_t)pb[2] << 16 |
               (uint32_t)pb[3] << 24) != vl;
    }
    const uint64_t A = lane64(d0, 0);
    const uint64_t B = uni64(rbase + 4 * (c0 + cnt) + a.voff[c0 + cnt]);
    const uint64_t prev = __shfl_up(in1, 1);
    const bool prev_bad = __shfl_up((uint32_t)bad, 1) != 0;
    const bool brk = lane < cnt && (lane == 0 || prev != in0 || bad || prev_bad);
    const uint64_t bm = __ballot(brk);
    const uint32_t nrun = (uint32_t)__builtin_popcountll(bm);
    if (brk) {
        const uint32_t q = mbcnt(bm);
        s_d[w][q] = d0 - A;
        s_in[w][q] = in0;
        s_fix[w][q] = bad ? vl + 1 : 0;
    }
    if (lane == 0) s_d[w][nrun] = B - A;
    vv_sync();
    const uint64_t X = A & ~(uint64_t)15;
    const uint32_t nseg = (uint32_t)((B - X + 15) >> 4);
    const uint32_t head = (uint32_t)(A - X);  // segment 0 starts head bytes before A
    const uint64_t tot = B - A;  // 64 values may exceed 4 GB
    const gptr_t<uint8_t> out = gbl(a.out);
    const gptr_t<const uint8_t> vb = gbl(v.bytes);
    // the run holding output byte r (relative to A): the last q with s_d[q] <= r
    auto run_of = [&](uint64_t r) {
        uint32_t lo = 0, hi = nrun;  // s_d[lo] <= r < s_d[hi]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_d[w][mid] <= r) lo = mid; else hi = mid;
        }
        return lo;
    };
    // 1. whole segments inside one run: one 16-byte store each; the others
    //    (a run boundary or an end of [A, B) inside) are listed
    uint32_t nslow = 0;
    for (uint32_t eb = 0; eb < nseg; eb += kWave * kVrUnroll) {
        u32x4 x0[kVrUnroll], x1[kVrUnroll];
        uint32_t sh[kVrUnroll];
        bool fast[kVrUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kVrUnroll; u++) {
            const uint32_t e = eb + u * kWave + lane;
            const int64_t r0 = 16 * (int64_t)e - (int64_t)head;  // segment's first byte - A
            fast[u] = false;
            sh[u] = 0;
            x0[u] = x1[u] = u32x4{0, 0, 0, 0};
            if (e < nseg && r0 >= 0 && r0 + 16 <= (int64_t)tot) {
                const uint32_t q = run_of((uint64_t)r0);
                if ((uint64_t)r0 + 16 <= s_d[w][q + 1] && (!s_fix[w][q] || (uint64_t)r0 >= s_d[w][q] + 4)) {
                    const uint64_t src = s_in[w][q] + ((uint64_t)r0 - s_d[w][q]);
                    const uintptr_t sa = reinterpret_cast<uintptr_t>(v.bytes) + (src & ~(uint64_t)3);
                    x0[u] = *gbl_at<const u32x4a>(sa);
                    x1[u].x = *gbl_at<const uint32_t>(sa + 16);
                    sh[u] = (uint32_t)src & 3;
                    fast[u] = true;
                }
            }
            const uint64_t sm = __ballot(e < nseg && !fast[u]);
            if (e < nseg && !fast[u]) s_slow[w][nslow + mbcnt(sm)] = e;
            nslow += (uint32_t)__builtin_popcountll(sm);
        }
#pragma unroll
        for (uint32_t u = 0; u < kVrUnroll; u++) {
            if (!fast[u]) continue;
            const uint32_t e = eb + u * kWave + lane;
            const uint32_t w0 = x0[u].x, w1 = x0[u].y, w2 = x0[u].z, w3 = x0[u].w, w4 = x1[u].x;
            __builtin_nontemporal_store(
                u32x4{funnel(w0, w1, sh[u]), funnel(w1, w2, sh[u]), funnel(w2, w3, sh[u]),
                      funnel(w3, w4, sh[u])}, (gptr_t<u32x4>)(out + X + 16 * (uint64_t)e));
        }
    }
    vv_sync();
    // 2. the listed segments, a lane each: every byte's source first, then
    //    all 16 loads in flight at once; whole segments by one store, the two
    //    cut by A and B a byte at a time
    for (uint32_t i = lane; i < nslow; i += kWave) {
        const uint32_t e = s_slow[w][i];
        const int64_t r0 = 16 * (int64_t)e - (int64_t)head;
        const bool whole = r0 >= 0 && r0 + 16 <= (int64_t)tot;
        uint64_t src[16];
        uint32_t fixb = 0, inr = 0;  // bit b: byte b from a descriptor / inside [A, B)
        uint32_t pre[4] = {0, 0, 0, 0};
        uint32_t q = run_of(r0 > 0 ? (uint64_t)r0 : 0);
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            const int64_t r = r0 + b;
            src[b] = s_in[w][q];  // harmless when unused
            if (r < 0 || r >= (int64_t)tot) continue;
            inr |= 1u << b;
            while ((uint64_t)r >= s_d[w][q + 1]) q++;
            const uint64_t t = (uint64_t)r - s_d[w][q];
            const uint32_t fx = s_fix[w][q];
            src[b] = s_in[w][q] + t;
            if (fx && t < 4) {
                fixb |= 1u << b;
                pre[b >> 2] |= (((fx - 1) >> (8 * t)) & 0xFFu) << (8 * (b & 3));
            }
        }
        uint32_t by[16];
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) by[b] = vb[src[b]];
        uint32_t wd[4] = {pre[0], pre[1], pre[2], pre[3]};
#pragma unroll
        for (uint32_t b = 0; b < 16; b++)
            if (!((fixb >> b) & 1)) wd[b >> 2] |= by[b] << (8 * (b & 3));
        if (whole) {
            *(gptr_t<u32x4>)(out + X + 16 * (uint64_t)e) = u32x4{wd[0], wd[1], wd[2], wd[3]};
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 16; b++)
                if ((inr >> b) & 1) out[X + 16 * (uint64_t)e + b] = (uint8_t)(wd[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// Header, filter-block prefix and footer of file f (one wave; byte stores,
// since the neighbouring bytes belong to other kernels).  The filter words
// themselves are stored by the bloom kernels.
__device__ void sst_meta_body(const SstArgs &a, uint32_t f) {
    const SstLayout L = sst_layout(a, f);
    uint8_t *img = a.out + uni64(a.file_off[f]);
    const uint32_t lane = lane_id();
    // Header (header.go:25-37): u32 kl0 | key[s] | u32 kl1 | key[e-1]
    const uint64_t k0 = L.e > L.s ? uni64(a.koff[L.s]) : 0;
    const uint64_t k1 = L.e > L.s ? uni64(a.koff[L.e - 1]) : 0;
    for (uint64_t q = lane; q < L.hdr; q += kWave) {
        uint32_t b;
        if (q < 4) b = (L.kl0 >> (8 * q)) & 0xff;
        else if (q < 4 + (uint64_t)L.kl0) b = a.keys[k0 + q - 4];
        else if (q < 8 + (uint64_t)L.kl0) b = (L.kl1 >> (8 * (q - 4 - L.kl0))) & 0xff;
        else b = a.keys[k1 + q - 8 - L.kl0];
        img[q] = (uint8_t)b;
    }
    // Filter prefix (bloom.go:472-491): u64le 24+8*nwords | u64be m | u64be k | u64be nbits
    if (lane < 32) {
        const uint32_t fi = lane / 8, fb = lane % 8;
        uint32_t b;
        if (fi == 0) b = (uint32_t)((24 + 8 * a.nwords) >> (8 * fb)) & 0xff;
        else {
            const uint64_t v = fi == 2 ? (uint64_t)a.k : a.m;
            b = (uint32_t)(v >> (8 * (7 - fb))) & 0xff;
        }
        img[L.hdr + lane] = (uint8_t)b;
        // Footer (footer.go:43-55): dataOff, dataSize, idxOff, idxSize (i64le)
        const uint64_t vals[4] = {L.data_off, L.data_size, L.idx_off, L.idx_size};
        img[L.img - 32 + lane] = (uint8_t)(vals[lane / 8] >> (8 * (lane % 8)));
        if (a.footer && lane < 4) a.footer[4 * (uint64_t)f + lane] = (int64_t)vals[lane];
    }
}

__global__ __launch_bounds__(64) void sst_meta_kernel(SstArgs a) { sst_meta_body(a, blockIdx.x); }

// ORs one key's k locations (its hash record, store_hash_rec) into the LDS
// slice.  The ORs are bound by VALU issue, not by the LDS (PMC,
// profiles/r04_pmc_sst_lds.txt: LDS array busy 21 % of the kernel, 256 VALU
// per key in the round-3 form), so per location the work is three VALU to
// place the bit and three to step the class's residue, and nothing else:
//  * no slice test: the word's LDS address ((p >> 5) << 2) - lo / 8 of a
//    location outside the slice lies outside the workgroup's LDS allocation
//    (above it, or wrapped below zero), and the LDS drops out-of-range
//    accesses (tools/lds_or_probe.py modes 7, 8, 10: bitmaps identical to
//    the exec-masked form) -- no compare, no exec-mask branch per location;
//  * the class steps are chosen once per key (a step whose 64-bit add wraps
//    loses 2^64: its residue less 2^64 mod m), by bitfield insert.
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// A hash record (store_hash_rec) unpacked: the residues of the four class
// bases (location c of class c) and each class's three steps, the carried
// ones already less 2^64 mod m: location 4(n + 1) + c = r[c] + st[c][n] mod m.
struct HashRecSteps {
    uint32_t r[4];
    uint32_t st[4][3];
};

__device__ __forceinline__ HashRecSteps unpack_hash_rec(const u32x4 x, uint32_t m, uint32_t c64) {
    constexpr uint32_t kRes = (1u << kHashRecBits) - 1;
    const uint32_t raw[4] = {x.x, x.y, x.z, x.w};
    HashRecSteps H;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) H.r[c] = raw[c] & kRes;
    // X = res(4 h2) | a << 21 | b << 22 from the top bytes of dwords 0-2
    const uint32_t X = __builtin_amdgcn_perm(raw[1], raw[0], 0x0c0c0703u) |
                       (raw[2] >> 24) << 16;
    const uint32_t d2 = X & kRes;
    // res(T) = res(base2) - res(base0) + a c64, res(4 h3) = 2 res(T) - b c64 (mod m)
    uint32_t rt = H.r[2] - H.r[0];
    rt = min(rt, rt + m);
    rt = (X >> 21) & 1 ? rt + c64 : rt;
    rt = min(rt, rt - m);
    uint32_t d3 = rt << 1;
    d3 = min(d3, d3 - m);
    d3 = (X >> 22) & 1 ? d3 - c64 : d3;
    d3 = min(d3, d3 + m);
    // the steps less 2^64 mod m, for a step whose 64-bit add wraps
    const uint32_t t2 = d2 - c64, t3 = d3 - c64;
    const uint32_t w2 = min(t2, t2 + m), w3 = min(t3, t3 + m);
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        const bool a2 = c == 0 || c == 3;
#pragma unroll
        for (uint32_t n = 0; n < 3; n++) {
            // all-ones where the step from location 4n + c carries (bit
            // 21 + n of dword c), then one bitfield insert (the compiler's
            // and / compare / cndmask form is three VALU)
            const uint32_t msk = (uint32_t)__builtin_amdgcn_sbfe((int)raw[c], kHashRecBits + n, 1);
            uint32_t v;
            __asm__("v_bfi_b32 %0, %1, %2, %3" : "=v"(v) : "v"(msk), "v"(a2 ? w2 : w3), "v"(a2 ? d2 : d3));
            H.st[c][n] = v;
        }
    }
    return H;
}

template <uint32_t K, bool Masked>
__device__ __forceinline__ void or_key_locations(const u32x4 x, uint32_t k, uint32_t m, uint32_t c64,
                                                 uint32_t base, uint32_t lo, uint32_t span) {
    HashRecSteps H = unpack_hash_rec(x, m, c64);
    uint32_t *r = H.r;
    auto &st = H.st;
#pragma unroll
    for (uint32_t j = 0; j < kSplitMaxK; j++) {
        const uint32_t c = j & 3, n = j >> 2;  // compile-time: r[] stays in registers
        if (K == 0 && j >= k) break;           // wave-uniform
        if (K != 0 && j >= K) break;
        const uint32_t p = r[c];
        // LDS byte address of the bit's word, out of range outside the slice
        // (shift + shift-add: the compiler's shift / and / add form is three)
        uint32_t a;
        __asm__("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(a) : "v"(p >> 5), "v"(base));
        if (!Masked || p - lo < span)
            __hip_atomic_fetch_or((lds_u32 *)(size_t)a, 1u << (p & 31), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WORKGROUP);
        if (n < 3) {
            const uint32_t t = p + st[c][n];
            r[c] = min(t, t - m);
        }
    }
}

// Filter blockIdx.x, slice blockIdx.y: every key's k locations rebuilt from
// its record, the slice's bits ORed in LDS, then stored big-endian into the
// image; the first slice's workgroup also writes the file's framing.
template <uint32_t K, bool Masked>
__device__ __forceinline__ void bloom_or_body(const BloomOrArgs &a, uint64_t s, uint64_t e,
                                              uint32_t base, uint32_t lo, uint32_t span) {
    const uint32_t m = a.m, c64 = a.c64;
    const uint64_t k0 = uni64(a.file_start[0]);
    // the file's records through one buffer resource: the record offset is
    // a 32-bit register stepping by 16 KiB per round, and the loads two
    // rounds ahead past the last key return zeros (never used)
    constexpr uint32_t kRec = 4 * kHashRecDwords;
    const rsrc_t rs = make_rsrc(a.rec + kHashRecDwords * (s - k0), (uint32_t)(kRec * (e - s)));
    uint32_t vo = kRec * threadIdx.x;
    constexpr uint32_t kStep = kRec * 1024;
    u32x4 xa = ld_b128(rs, vo), xb = ld_b128(rs, vo + kStep);
    for (uint64_t i = s + threadIdx.x; i < e; i += 1024) {
        const u32x4 x = xa;
        xa = xb;
        vo += kStep;
        xb = ld_b128(rs, vo + kStep);
        or_key_locations<K, Masked>(x, a.k, m, c64, base, lo, span);
    }
}

__global__ __launch_bounds__(1024) void bloom_or_kernel(BloomOrArgs a, SstArgs sa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_bits[];
    // workgroups b and b + 8 share an XCD (blocks are dealt round-robin over
    // the 8 XCDs, the guide's observed placement; speed only): the two
    // slices of filter f are blocks 16 (f / 8) + f % 8 and that + 8, so they
    // run side by side on one XCD and the second read of the filter's hash
    // records is served by that XCD's L2
    const uint32_t b = blockIdx.x, f = (b / 16) * 8 + b % 8, sl = (b / 8) % 2;
    if (f >= a.nfiles || (a.dnf && f >= uni64(*a.dnf))) return;
    // the image's header, filter prefix and footer (disjoint from the words)
    if (sl == 0 && threadIdx.x < kWave) sst_meta_body(sa, f);
    const uint32_t lo = sl * a.split, hi = lo + a.split < a.m ? lo + a.split : a.m;
    const uint32_t nw = (hi - lo + 63) / 64 * 2;
    for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) lds_bits[i] = 0;
    __syncthreads();
    const uint64_t s = uni64(a.file_start[f]), e = uni64(a.file_start[f + 1]);
    // lo is a multiple of 64: the slice's bit p sits in LDS word (p - lo) >> 5,
    // bit p & 31; base = -lo / 8 bytes, plus the array's own LDS address.
    // The unmasked ORs rely on lds_bits being the workgroup's only LDS, at
    // address 0: a location below the slice then wraps below zero and one
    // above it lies past the allocation, and the LDS drops both.  This
    // kernel and everything it calls (sst_meta_body, store_filter_slice)
    // declare no static __shared__ (tests/test_source_invariants.py); should
    // the array ever not start at 0, the slice test is made per location
    // instead (a wave-uniform choice, never taken in this build).
    const uint32_t lds0 = (uint32_t)(size_t)(lds_u32 *)lds_bits;
    const uint32_t base = lds0 - lo / 8, span = hi - lo;
    if (lds0 == 0) {
        if (a.k == kSplitMaxK) bloom_or_body<kSplitMaxK, false>(a, s, e, base, lo, span);
        else bloom_or_body<0, false>(a, s, e, base, lo, span);
    } else {
        bloom_or_body<0, true>(a, s, e, base, lo, span);
    }
    __syncthreads();
    const uint64_t hdr = sst_header_bytes(a.koff, s, e);
    store_filter_slice(WgGroup{}, lds_bits, lo / 64, hi == a.m ? a.nwords : (uint64_t)(hi + 63) / 64,
                       a.out + uni64(a.file_off[f]) + hdr + 32, nullptr);
}



// ---- probe / hash ----------------------------------------------------------

__global__ __launch_bounds__(256) void sum256_kernel(const uint8_t *keys, const uint64_t *koff,
                                                     uint64_t n, uint64_t *out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t h[4];
    uint64_t k0 = koff[i];
    sum256(keys + k0, koff[i + 1] - k0, h);
    for (int j = 0; j < 4; j++) out[4 * i + j] = h[j];
}

__global__ __launch_bounds__(256) void bloom_probe_kernel(const uint64_t *words, uint64_t m,
                                                          uint64_t mrecip, uint32_t k,
                                                          const uint8_t *keys,
                                                          const uint64_t *koff, uint64_t n,
                                                          uint8_t *hit) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t h[4];
    uint64_t k0 = koff[i];
    sum256(keys + k0, koff[i + 1] - k0, h);
    uint8_t ok = 1;
    for (uint32_t j = 0; j < k && ok; j++) {
        uint64_t p = mod_barrett(location(h[0], h[1], h[2], h[3], j), m, mrecip);
        if (!((words[p >> 6] >> (p & 63)) & 1)) ok = 0;
    }
    hit[i] = ok;
}

// ---- batched SSTable.MayContain ------------------------
//
// d_hit[i * nfile + f] = SSTable.MayContain(key i) on file f (sstable.go:300-
// 305): the key range check against the header's min / max key in Go string
// order, then Filter.Test (bloom.go:371-379) on the filter block as stored in
// the image (u64 big-endian words, bitset v1.22.0 WriteTo; bit p -> word p>>6
// bit p&63; bitset.Test is false past its length).  One thread per key
// hashes it once (sum256) and walks the files.  Per tile of kMcTile files the
// block stages each file's bounds (16-byte big-endian prefixes), pointers
// and filter parameters in LDS, packs its results four files to a dword in
// an LDS out tile, and then writes the block's rows x tile sub-block of the
// hit matrix coalesced (dwords when nfile is a multiple of 4).
constexpr uint32_t kMcTile = 64;
constexpr uint32_t kMcThreads = 256;
constexpr uint32_t kMcProbeGrid = 1024;  // per-probe path: workgroups (grid-stride)
constexpr uint32_t kMcRow = kMcTile / 4 + 1;  // dwords per out-tile row (+1: LDS banks)

// Filter.Test tests hashNum locations and stops at the first clear bit; a
// stored k beyond this (only a corrupted file) is capped so a probe of a
// saturated filter ends (deviations).
constexpr uint32_t kMcMaxK = 1u << 24;

struct McFile {
    uint32_t lo[4], hi[4];  // first 16 bytes of min / max key, big-endian, zero padded
    uint32_t lo_len, hi_len;
    uint32_t ok;            // header and filter decoded (lsm_sst_meta.stage not 1 or 2)
    uint32_t k;             // filter k, capped so a probe always ends
    uint64_t lo_at, hi_at;  // image offsets of the min / max key bytes
    uint64_t words_at;      // image offset of the first filter word
    uint64_t m, mr, nbits;  // filter m, its Barrett reciprocal, stored bit count
};

__device__ __forceinline__ uint32_t be_word_at(const uint8_t *p, uint64_t len, uint32_t j) {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; b++) {
        const uint64_t at = 4ull * j + b;
        w = (w << 8) | (at < len ? p[at] : 0u);
    }
    return w;
}

// Go string comparison of a and b (bytewise, then length): <0, 0, >0.
__device__ __forceinline__ int go_cmp(const uint8_t *a, uint64_t la, const uint8_t *b,
                                      uint64_t lb) {
    const uint64_t n = la < lb ? la : lb;
    for (uint64_t i = 0; i < n; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return la < lb ? -1 : la > lb ? 1 : 0;
}

// Compare the 16-byte big-endian prefixes, then (when both go on) the bytes.
__device__ __forceinline__ int bound_cmp(const uint32_t bw[4], uint64_t blen, const uint8_t *bp,
                                         const uint32_t kw[4], uint64_t klen, const uint8_t *kp) {
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (bw[j] != kw[j]) return bw[j] < kw[j] ? -1 : 1;
    // equal over min(16, len) bytes with zero padding: decide by the rest
    if (blen <= 16 || klen <= 16) {
        // zero padding hides a real 0x00 byte only when one side ends first
        return go_cmp(bp, blen, kp, klen);
    }
    return go_cmp(bp + 16, blen - 16, kp + 16, klen - 16);
}

// Lexicographic compare of two 16-byte big-endian prefixes: -1, 0, 1 (branch-free).
__device__ __forceinline__ int prefix_cmp(const uint32_t a[4], const uint32_t b[4]) {
    const uint64_t a0 = (uint64_t)a[0] << 32 | a[1], a1 = (uint64_t)a[2] << 32 | a[3];
    const uint64_t b0 = (uint64_t)b[0] << 32 | b[1], b1 = (uint64_t)b[2] << 32 | b[3];
    const int lt = (a0 < b0) | ((a0 == b0) & (a1 < b1));
    const int gt = (a0 > b0) | ((a0 == b0) & (a1 > b1));
    return gt - lt;
}

// bound_cmp with the common case (prefixes differ) branch-free
__device__ __forceinline__ int bound_cmp_fast(const uint32_t bw[4], uint64_t blen, const uint8_t *bp,
                                              const uint32_t kw[4], uint64_t klen, const uint8_t *kp) {
    const int c = prefix_cmp(bw, kw);
    if (c != 0) return c;
    return bound_cmp(bw, blen, bp, kw, klen, kp);
}

__global__ __launch_bounds__(kMcThreads) void may_contain_kernel(const uint8_t *img,
                                                                 const uint64_t *file_off,
                                                                 const lsm_sst_meta *meta,
                                                                 uint32_t nfile, const uint8_t *keys,
                                                                 const uint64_t *koff, uint64_t nkeys,
                                                                 uint8_t *hit,
                                                                 const uint32_t *grouped) {
    __shared__ McFile tile[kMcTile];
    if (*grouped) return;  // the files are sorted and disjoint: mc_* kernels answer
    __shared__ uint32_t sout[kMcThreads * kMcRow];
    // a capped grid strides over the probes (when the grouped path answers,
    // fewer workgroups have to start only to see the flag)
    for (uint64_t i0 = (uint64_t)blockIdx.x * kMcThreads; i0 < nkeys;
         i0 += (uint64_t)gridDim.x * kMcThreads) {
        __syncthreads();  // sout and tile of the previous rows are consumed
        const uint64_t i = i0 + threadIdx.x;
        const bool act = i < nkeys;
        const uint32_t rows = nkeys - i0 < kMcThreads ? (uint32_t)(nkeys - i0) : kMcThreads;
        uint64_t k0 = 0, kl = 0;
        uint64_t h[4] = {0, 0, 0, 0};
        uint32_t kw[4] = {0, 0, 0, 0};
        if (act) {
            k0 = koff[i];
            kl = koff[i + 1] - k0;
            sum256(keys + k0, kl, h);
    #pragma unroll
            for (uint32_t j = 0; j < 4; j++) kw[j] = be_word_at(keys + k0, kl, j);
        }
        const uint8_t *kp = keys + k0;
        for (uint32_t f0 = 0; f0 < nfile; f0 += kMcTile) {
            const uint32_t nt = nfile - f0 < kMcTile ? nfile - f0 : kMcTile;
            __syncthreads();
            for (uint32_t t = threadIdx.x; t < nt; t += kMcThreads) {
                const lsm_sst_meta &M = meta[f0 + t];
                const uint64_t fo = file_off[f0 + t];
                const uint8_t *base = img + fo;
                McFile F;
                F.ok = M.stage != 1 && M.stage != 2;
                F.lo_len = (uint32_t)M.min_key_len;
                F.hi_len = (uint32_t)M.max_key_len;
                for (uint32_t j = 0; j < 4; j++) {
                    F.lo[j] = F.ok ? be_word_at(base + M.min_key_off, M.min_key_len, j) : 0;
                    F.hi[j] = F.ok ? be_word_at(base + M.max_key_off, M.max_key_len, j) : 0;
                }
                F.lo_at = fo + M.min_key_off;
                F.hi_at = fo + M.max_key_off;
                F.words_at = fo + M.filter_words_off;
                // k from the file (no max(1, k) on a decoded filter); Test's
                // early exit ends a probe at its first clear bit, a corrupted k
                // beyond kMcMaxK is capped (deviations)
                F.k = M.filter_k < kMcMaxK ? (uint32_t)M.filter_k : kMcMaxK;
                F.m = M.filter_m;
                F.mr = M.filter_m ? ~0ull / M.filter_m : 0;
                F.nbits = M.filter_nbits;
                tile[t] = F;
            }
            // a tile of decoded files in key order with disjoint ranges (level >= 1
            // files) holds a key in at most one file: the last whose MinKey <= key
            bool sorted = true;
            if (threadIdx.x < nt) {
                const McFile &A = tile[threadIdx.x];
                // MinKey <= MaxKey too: a corrupted header with min > max breaks
                // the order the binary search relies on
                sorted = A.ok != 0 &&
                         bound_cmp_fast(A.lo, A.lo_len, img + A.lo_at, A.hi, A.hi_len, img + A.hi_at) <= 0;
                if (sorted && threadIdx.x + 1 < nt) {
                    const McFile &B = tile[threadIdx.x + 1];
                    sorted = B.ok && bound_cmp_fast(A.hi, A.hi_len, img + A.hi_at, B.lo, B.lo_len,
                                                    img + B.lo_at) < 0;
                }
            }
            sorted = __syncthreads_and(sorted);
            uint32_t cand_lo = 0, cand_hi = nt;  // files to test: [cand_lo, cand_hi)
            if (sorted && act) {
                uint32_t lo = 0, hi = nt;  // first t with MinKey > key
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) / 2;
                    const McFile &F = tile[mid];
                    if (bound_cmp_fast(F.lo, F.lo_len, img + F.lo_at, kw, kl, kp) <= 0) lo = mid + 1;
                    else hi = mid;
                }
                cand_lo = lo ? lo - 1 : 0;
                cand_hi = lo;
            }
            uint32_t pack = 0;
            for (uint32_t t = 0; t < nt; t++) {
                uint32_t r = 0;
                if (act && t >= cand_lo && t < cand_hi && tile[t].ok) {
                    const McFile &F = tile[t];
                    // sstable.go:301: MinKey > key || MaxKey < key -> false
                    if (bound_cmp_fast(F.lo, F.lo_len, img + F.lo_at, kw, kl, kp) <= 0 &&
                        bound_cmp_fast(F.hi, F.hi_len, img + F.hi_at, kw, kl, kp) >= 0) {
                        const uint64_t m = F.m;
                        // hashNum 0: Test is true (bloom.go:373 loop never runs);
                        // m == 0 with k > 0: Go's location() divides by zero and
                        // panics, answered false here
                        r = F.k == 0 || m != 0;
                        // Test's answer is the AND of all k bits (its early exit
                        // changes nothing): sixteen loads in flight at a time
                        for (uint32_t j0 = 0; j0 < F.k && r; j0 += 16) {
                            uint32_t bits = 1;
    #pragma unroll
                            for (uint32_t u = 0; u < 16; u++) {
                                const uint32_t j = j0 + u;
                                if (j < F.k && r) {
                                    const uint64_t x = location(h[0], h[1], h[2], h[3], j);
                                    const uint64_t p = m < (1ull << 63) ? mod_barrett(x, m, F.mr) : x % m;
                                    bits &= p < F.nbits
                                                ? (uint32_t)(img[F.words_at + 8 * (p >> 6) + 7 - ((p & 63) >> 3)] >> (p & 7)) & 1
                                                : 0u;
                                }
                            }
                            r &= bits;
                        }
                    }
                }
                pack |= r << (8 * (t & 3));
                if ((t & 3) == 3 || t + 1 == nt) {
                    sout[threadIdx.x * kMcRow + t / 4] = pack;
                    pack = 0;
                }
            }
            __syncthreads();
            // the rows x nt sub-block of hit, coalesced
            if ((nfile & 3) == 0) {  // every row segment starts 4-aligned (nt is a multiple of 4)
                const uint32_t nd = nt / 4;
                for (uint32_t x = threadIdx.x; x < rows * nd; x += kMcThreads) {
                    const uint32_t rr = x / nd, c = x % nd;
                    *reinterpret_cast<uint32_t *>(hit + (i0 + rr) * nfile + f0 + 4 * c) =
                        sout[rr * kMcRow + c];
                }
            } else {
                for (uint32_t x = threadIdx.x; x < rows * nt; x += kMcThreads) {
                    const uint32_t rr = x / nt, c = x % nt;
                    hit[(i0 + rr) * nfile + f0 + c] = (uint8_t)(sout[rr * kMcRow + c / 4] >> (8 * (c & 3)));
                }
            }
        }
    }
}

// Grouped path for the level >= 1 shape (every file decoded, files in key
// order with disjoint ranges, at most kMcMaxFiles files): each probe has at
// most one candidate file.  mc_classify_kernel hashes the candidates once and
// groups each workgroup's by file into its slots (the level search's layout,
// LvWs), and lv_test_kernel<true> (one workgroup per file) stages the filter
// in LDS and tests its probes' bits there: the filter bits are read once from
// HBM instead of once per probe bit.
constexpr uint32_t kMcLdsBytes = 144 * 1024;  // filter words staged in LDS per file
constexpr uint32_t kMcNone = 0xFFFFFFFFu;
constexpr uint32_t kMcGroupThreads = 1024;
constexpr uint32_t kMcGroupPer = 2;  // probes per thread
constexpr uint32_t kMcGroupProbes = kMcGroupThreads * kMcGroupPer;
constexpr uint32_t kMcMaxFiles = 2048;  // LDS bounds + counters; more files: per-probe path

// A table whose filter takes the 16-byte hash record of the encode path
// (store_hash_rec: m <= 2^21, k <= 16; go-lsm's 1.6 Mbit, k = 16): classify
// stores the record for the table's m, and the test rebuilds the locations
// from it by additions -- 16 bytes per probe through the workspace instead
// of the 32-byte sum256, and no modulo in the test.
__device__ __forceinline__ bool lv_compact(const McFile &F) {
    return F.m != 0 && F.m <= (1ull << kHashRecBits) && F.k <= kSplitMaxK;
}

constexpr uint32_t kLvThreads = 1024;
constexpr uint32_t kLvPer = 2;  // probes per thread
constexpr uint32_t kLvProbes = kLvThreads * kLvPer;
constexpr uint32_t kLvMaxFiles = 2048;
constexpr uint32_t kLvMaxWgs = 1024;  // classify workgroups per pass (2M probes)

struct LvWs {
    McFile *files;
    uint32_t *grid;   // [nfile][nwg]: the table's first slot in the workgroup
    uint32_t *cnt;    // [nfile][nwg]: the table's probes in the workgroup
    uint32_t *ids;    // [nwg * 2048] probe of each slot
    u32x4 *rec;       // [nwg * 2048] its 16-byte hash record (lv_compact tables),
                      // else h0, h1 of its sum256
    u32x4 *ext;       // [nwg * 2048] h2, h3 (tables that are not lv_compact)
};


LvWs lv_ws_layout(uint8_t *base, uint32_t nfile, uint64_t nkeys, size_t *total) {
    LvWs w{};
    size_t at = 0;
    auto take = [&](size_t bytes) -> uint8_t * {
        uint8_t *p = base ? base + at : nullptr;
        at += (bytes + 255) & ~(size_t)255;
        return p;
    };
    const uint64_t pass = nkeys < (uint64_t)kLvMaxWgs * kLvProbes ? nkeys : (uint64_t)kLvMaxWgs * kLvProbes;
    const uint64_t nwg = (pass + kLvProbes - 1) / kLvProbes;
    const size_t nf = nfile ? nfile : 1;
    w.files = reinterpret_cast<McFile *>(take(sizeof(McFile) * nf));
    w.grid = reinterpret_cast<uint32_t *>(take(4 * nf * (nwg ? nwg : 1)));
    w.cnt = reinterpret_cast<uint32_t *>(take(4 * nf * (nwg ? nwg : 1)));
    w.ids = reinterpret_cast<uint32_t *>(take(4 * (nwg ? nwg : 1) * kLvProbes));
    w.rec = reinterpret_cast<u32x4 *>(take(16 * (nwg ? nwg : 1) * kLvProbes));
    w.ext = reinterpret_cast<u32x4 *>(take(16 * (nwg ? nwg : 1) * kLvProbes));
    if (total) *total = at;
    return w;
}

static_assert(kMcGroupProbes == kLvProbes && kMcGroupThreads == kLvThreads && kMcMaxFiles == kLvMaxFiles,
              "the all-tables classify fills the level search's slot layout");

struct McWs {
    uint32_t *flag;     // [0] = 1: grouped path
    McFile *files;
    LvWs lv;            // the probes grouped by candidate file, as the level search's
};

// key bytes [p, p + len) as four big-endian words, zero padded past len
// (reads 16 bytes at p: the input slack covers a key that ends a buffer)
__device__ __forceinline__ void key_prefix(const uint8_t *p, uint64_t len, uint32_t kw[4]) {
    uint64_t f0 = ldg_u64_unaligned(p), f1 = ldg_u64_unaligned(p + 8);
    if (len < 8) { f0 &= len ? (~0ull >> (64 - 8 * len)) : 0; f1 = 0; }
    else if (len < 16) f1 &= len > 8 ? (~0ull >> (128 - 8 * len)) : 0;
    kw[0] = __builtin_bswap32((uint32_t)f0);
    kw[1] = __builtin_bswap32((uint32_t)(f0 >> 32));
    kw[2] = __builtin_bswap32((uint32_t)f1);
    kw[3] = __builtin_bswap32((uint32_t)(f1 >> 32));
}

__device__ __forceinline__ McFile mc_file(const uint8_t *img, const uint64_t *file_off,
                                          const lsm_sst_meta &M, uint32_t f) {
    const uint64_t fo = file_off[f];
    const uint8_t *base = img + fo;
    McFile F;
    F.ok = M.stage != 1 && M.stage != 2;
    F.lo_len = (uint32_t)M.min_key_len;
    F.hi_len = (uint32_t)M.max_key_len;
    // the key prefixes by unaligned 8-byte loads, all in flight (byte loads
    // under a per-byte condition were 32 serialized round trips per file)
    for (uint32_t j = 0; j < 4; j++) F.lo[j] = F.hi[j] = 0;
    if (F.ok) {
        key_prefix(base + M.min_key_off, M.min_key_len, F.lo);
        key_prefix(base + M.max_key_off, M.max_key_len, F.hi);
    }
    F.lo_at = fo + M.min_key_off;
    F.hi_at = fo + M.max_key_off;
    F.words_at = fo + M.filter_words_off;
    F.k = M.filter_k < kMcMaxK ? (uint32_t)M.filter_k : kMcMaxK;
    F.m = M.filter_m;
    F.mr = M.filter_m ? ~0ull / M.filter_m : 0;
    F.nbits = M.filter_nbits;
    return F;
}

__global__ __launch_bounds__(256) void mc_prep_kernel(const uint8_t *img, const uint64_t *file_off,
                                                      const lsm_sst_meta *meta, uint32_t nfile,
                                                      McWs w) {
    bool ok = true;
    for (uint32_t f = threadIdx.x; f < nfile; f += blockDim.x) {
        const McFile F = mc_file(img, file_off, meta[f], f);
        w.files[f] = F;
        // m < 2^63 for the Barrett reduction; MinKey <= MaxKey (a corrupted
        // header with min > max would break the order of the bound search)
        ok = ok && F.ok && F.m < (1ull << 63) &&
             bound_cmp_fast(F.lo, F.lo_len, img + F.lo_at, F.hi, F.hi_len, img + F.hi_at) <= 0;
    }
    if (nfile > kMcMaxFiles) ok = false;
    __syncthreads();
    for (uint32_t f = threadIdx.x; f + 1 < nfile; f += blockDim.x) {
        const McFile &A = w.files[f], &B = w.files[f + 1];
        ok = ok && bound_cmp_fast(A.hi, A.hi_len, img + A.hi_at, B.lo, B.lo_len, img + B.lo_at) < 0;
    }
    ok = __syncthreads_and(ok);
    if (threadIdx.x == 0) w.flag[0] = ok ? 1u : 0u;
}

// Probes are grouped block-locally first (LDS counters), so each workgroup
// adds to a file's global counter once: 1M probes over 208 files serialised
// on 208 global atomics took 350 us, the block-local counts take a few.
// The files' bound prefixes sit in LDS for the candidate search.
__global__ __launch_bounds__(kMcGroupThreads) void mc_classify_kernel(const uint8_t *img, uint32_t nfile,
                                                                      const uint8_t *keys,
                                                                      const uint64_t *koff,
                                                                      uint64_t k_begin, uint64_t nkeys,
                                                                      McWs w, uint32_t nwg,
                                                                      uint8_t *hit) {
    __shared__ uint4 slo[kMcMaxFiles], shi[kMcMaxFiles];
    __shared__ uint32_t lh[kMcMaxFiles];
    __shared__ uint32_t part[kMcGroupThreads];
    if (!w.flag[0]) return;
    const uint32_t t = threadIdx.x;
    for (uint32_t f = threadIdx.x; f < nfile; f += kMcGroupThreads) {
        const McFile &F = w.files[f];
        slo[f] = make_uint4(F.lo[0], F.lo[1], F.lo[2], F.lo[3]);
        shi[f] = make_uint4(F.hi[0], F.hi[1], F.hi[2], F.hi[3]);
        lh[f] = 0;
    }
    // every probe's first 16 key bytes (dword loads; batches are 16-byte
    // padded), all loads in flight before the search
    uint64_t k0[kMcGroupPer], kl[kMcGroupPer], f0[kMcGroupPer], f1[kMcGroupPer];
#pragma unroll
    for (uint32_t p = 0; p < kMcGroupPer; p++) {
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kMcGroupProbes + p * kMcGroupThreads + t;
        k0[p] = i < nkeys ? koff[i] : 0;
        kl[p] = i < nkeys ? koff[i + 1] - k0[p] : 0;
    }
#pragma unroll
    for (uint32_t p = 0; p < kMcGroupPer; p++) {
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kMcGroupProbes + p * kMcGroupThreads + t;
        f0[p] = i < nkeys ? ldg_u64_unaligned(keys + k0[p]) : 0;
        f1[p] = i < nkeys ? ldg_u64_unaligned(keys + k0[p] + 8) : 0;
    }
    uint32_t kw[kMcGroupPer][4];
#pragma unroll
    for (uint32_t p = 0; p < kMcGroupPer; p++) {
        // zero the bytes past the key, then the big-endian prefix words
        const uint64_t l = kl[p];
        if (l < 8) { f0[p] &= l ? (~0ull >> (64 - 8 * l)) : 0; f1[p] = 0; }
        else if (l < 16) f1[p] &= l > 8 ? (~0ull >> (128 - 8 * l)) : 0;
        kw[p][0] = __builtin_bswap32((uint32_t)f0[p]);
        kw[p][1] = __builtin_bswap32((uint32_t)(f0[p] >> 32));
        kw[p][2] = __builtin_bswap32((uint32_t)f1[p]);
        kw[p][3] = __builtin_bswap32((uint32_t)(f1[p] >> 32));
    }
    __syncthreads();
    uint32_t cand[kMcGroupPer], rank[kMcGroupPer];
    uint64_t hh[kMcGroupPer][4];
#pragma unroll
    for (uint32_t p = 0; p < kMcGroupPer; p++) cand[p] = kMcNone;
#pragma unroll
    for (uint32_t p = 0; p < kMcGroupPer; p++) {
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kMcGroupProbes + p * kMcGroupThreads + t;
        if (i >= nkeys) break;
        const uint8_t *kp = keys + k0[p];
        uint32_t lo = 0, hi = nfile;  // first file with MinKey > key
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            const uint4 v = slo[mid];
            const uint32_t bw[4] = {v.x, v.y, v.z, v.w};
            int c = prefix_cmp(bw, kw[p]);
            if (c == 0) {
                const McFile &F = w.files[mid];
                c = bound_cmp(bw, F.lo_len, img + F.lo_at, kw[p], kl[p], kp);
            }
            if (c <= 0) lo = mid + 1;
            else hi = mid;
        }
        if (lo > 0) {
            const uint4 v = shi[lo - 1];
            const uint32_t bw[4] = {v.x, v.y, v.z, v.w};
            int r = prefix_cmp(bw, kw[p]);
            if (r == 0) {
                const McFile &F = w.files[lo - 1];
                r = bound_cmp(bw, F.hi_len, img + F.hi_at, kw[p], kl[p], kp);
            }
            if (r >= 0) {  // only candidates are ever tested
                cand[p] = lo - 1;
                rank[p] = atomicAdd(&lh[lo - 1], 1u);
                sum256_pre(kp, kl[p], f0[p], f1[p], hh[p]);
            }
        }
    }
    {   // the workgroup's rows of the hit matrix, written once: 0 except the
        // candidate's 1 (the test clears it when a bit is 0), 16-byte stores;
        // the candidates through LDS (the scan's row, free until the scan)
        uint16_t *scand = reinterpret_cast<uint16_t *>(part);
#pragma unroll
        for (uint32_t p = 0; p < kMcGroupPer; p++)
            scand[p * kMcGroupThreads + t] = cand[p] == kMcNone ? (uint16_t)0xFFFFu : (uint16_t)cand[p];
        __syncthreads();
        const uint64_t r0 = k_begin + (uint64_t)blockIdx.x * kMcGroupProbes;
        const uint64_t r1 = r0 + kMcGroupProbes < nkeys ? r0 + kMcGroupProbes : nkeys;
        uint8_t *z = hit + r0 * nfile;
        const uint32_t nz = (uint32_t)((r1 - r0) * nfile);  // <= 2,048 rows x 2,048 files
        const uint32_t mis = (uint32_t)((uintptr_t)z & 15);
        const uint32_t head = ((16 - mis) & 15) < nz ? ((16 - mis) & 15) : nz;
        const uint32_t n16 = (nz - head) / 16, tail = head + 16 * n16;
        auto one_at = [&](uint32_t o) -> uint32_t {  // byte o of the rows: the candidate's 1
            const uint32_t row = o / nfile;
            const uint32_t c = scand[row];
            return c != 0xFFFFu && row * nfile + c == o ? 1u : 0u;
        };
        if (t < head) z[t] = (uint8_t)one_at(t);
        u32x4 *z16 = reinterpret_cast<u32x4 *>(z + head);
        for (uint32_t x = t; x < n16; x += kMcGroupThreads) {
            const uint32_t o = head + 16 * x;
            uint32_t wd[4] = {0, 0, 0, 0};
            for (uint32_t row = o / nfile; row * nfile < o + 16; row++) {
                const uint32_t c = scand[row];
                const uint32_t at = row * nfile + c;
                if (c != 0xFFFFu && at >= o && at < o + 16) wd[(at - o) >> 2] |= 1u << (8 * ((at - o) & 3));
            }
            z16[x] = u32x4{wd[0], wd[1], wd[2], wd[3]};
        }
        if (tail + t < nz) z[tail + t] = (uint8_t)one_at(tail + t);
    }
    __syncthreads();
    // the workgroup's candidates grouped by file into its slots, as the level
    // search's classify does: exclusive scan of the per-file counts (<= 2,048
    // files, 2 per thread), the file-major grid, then the ids and records
    const uint32_t c0 = 2 * t < nfile ? lh[2 * t] : 0u, c1 = 2 * t + 1 < nfile ? lh[2 * t + 1] : 0u;
    part[t] = c0 + c1;
    __syncthreads();
    for (uint32_t d = 1; d < kMcGroupThreads; d <<= 1) {
        const uint32_t x = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    const uint32_t ex = part[t] - c0 - c1;
    __syncthreads();  // every lh read before it is overwritten with offsets
    if (2 * t < nfile) {
        lh[2 * t] = ex;
        w.lv.grid[(uint64_t)(2 * t) * nwg + blockIdx.x] = ex;
        w.lv.cnt[(uint64_t)(2 * t) * nwg + blockIdx.x] = c0;
    }
    if (2 * t + 1 < nfile) {
        lh[2 * t + 1] = ex + c0;
        w.lv.grid[(uint64_t)(2 * t + 1) * nwg + blockIdx.x] = ex + c0;
        w.lv.cnt[(uint64_t)(2 * t + 1) * nwg + blockIdx.x] = c1;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t p = 0; p < kMcGroupPer; p++) {
        if (cand[p] == kMcNone) continue;
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kMcGroupProbes + p * kMcGroupThreads + t;
        const uint64_t slot = (uint64_t)blockIdx.x * kMcGroupProbes + lh[cand[p]] + rank[p];
        w.lv.ids[slot] = (uint32_t)(i - k_begin);
        const McFile &F = w.files[cand[p]];
        if (lv_compact(F)) {  // 16 bytes, and no modulo in the test
            store_hash_rec(hh[p], (uint32_t)F.m, (uint32_t)F.mr, (uint32_t)(F.mr >> 32),
                           reinterpret_cast<uint32_t *>(w.lv.rec + slot));
        } else {
            *(gptr_t<u64x2>)gbl(w.lv.rec + slot) = u64x2{hh[p][0], hh[p][1]};
            *(gptr_t<u64x2>)gbl(w.lv.ext + slot) = u64x2{hh[p][2], hh[p][3]};
        }
    }
}

// Filter.Test (bloom.go:371-379) of one probe against F, the bytes below
// in_lds from LDS (lb), the rest from the image through L2.  Sixteen
// locations at a time, every read of a round issued before any is waited for:
// the LDS read at a clamped address, the tail read under a predicate into its
// own register (a read per branch whose join waits for it is sixteen
// serialized round trips).  Lds = false: no LDS copy, every bit from src.
template <bool Lds = true>
__device__ __forceinline__ uint32_t filter_test(const McFile &F, const uint64_t h[4], const uint8_t *lb,
                                                uint64_t in_lds, const uint8_t *src) {
    // k == 0: true; m == 0 < k: Go panics, answered false
    uint32_t r = F.k == 0 || F.m != 0;
    const bool small = F.m <= (1ull << 30);
    const uint32_t m32 = (uint32_t)F.m, rl = (uint32_t)F.mr, rh = (uint32_t)(F.mr >> 32);
    for (uint32_t j0 = 0; j0 < F.k && r; j0 += 16) {
        uint64_t p[16];
        uint32_t lv[16], gv[16];
#pragma unroll
        for (uint32_t u = 0; u < 16; u++) {
            const uint64_t x = location(h[0], h[1], h[2], h[3], j0 + u);
            p[u] = small ? mod_small(x, m32, rl, rh) : mod_barrett(x, F.m, F.mr);
            const uint64_t q = 8 * (p[u] >> 6) + 7 - ((p[u] & 63) >> 3);
            const bool inl = Lds && q < in_lds;
            lv[u] = Lds ? lb[inl ? q : 0] : 0u;
            gv[u] = 0xFFu;
            if (j0 + u < F.k && !inl && p[u] < F.nbits) gv[u] = gbl(src)[q];
        }
        uint32_t bits = 1;
#pragma unroll
        for (uint32_t u = 0; u < 16; u++) {
            const uint64_t q = 8 * (p[u] >> 6) + 7 - ((p[u] & 63) >> 3);
            const uint32_t byte = Lds && q < in_lds ? lv[u] : gv[u];
            // bitset.Test is false past its length
            const uint32_t bit = p[u] < F.nbits ? (byte >> (p[u] & 7)) & 1u : 0u;
            bits &= j0 + u < F.k ? bit : 1u;
        }
        r = bits;
    }
    return r;
}

// filter_test from a probe's hash record (lv_compact tables): the k <= 16
// locations by additions (unpack_hash_rec), the bits read as filter_test does
// (all reads in flight, then combined).
__device__ __forceinline__ uint32_t filter_test_rec(const McFile &F, const HashRecSteps &H0,
                                                    uint32_t m, const uint8_t *lb, uint64_t in_lds,
                                                    const uint8_t *src) {
    uint32_t r[4] = {H0.r[0], H0.r[1], H0.r[2], H0.r[3]};
    uint32_t pos[kSplitMaxK];
#pragma unroll
    for (uint32_t j = 0; j < kSplitMaxK; j++) {
        const uint32_t c = j & 3, n = j >> 2;
        pos[j] = r[c];
        if (n < 3) {
            const uint32_t t = r[c] + H0.st[c][n];
            r[c] = min(t, t - m);
        }
    }
    uint32_t lv[kSplitMaxK], gv[kSplitMaxK];
#pragma unroll
    for (uint32_t j = 0; j < kSplitMaxK; j++) {
        const uint32_t p = pos[j];
        const uint32_t q = 8 * (p >> 6) + 7 - ((p & 63) >> 3);
        const bool inl = q < in_lds;
        lv[j] = lb[inl ? q : 0u];
        gv[j] = 0xFFu;
        if (j < F.k && !inl && p < F.nbits) gv[j] = gbl(src)[q];
    }
    uint32_t bits = 1;
#pragma unroll
    for (uint32_t j = 0; j < kSplitMaxK; j++) {
        const uint32_t p = pos[j];
        const uint32_t q = 8 * (p >> 6) + 7 - ((p & 63) >> 3);
        const uint32_t byte = q < in_lds ? lv[j] : gv[j];
        // bitset.Test is false past its length
        const uint32_t bit = p < F.nbits ? (byte >> (p & 7)) & 1u : 0u;
        bits &= j < F.k ? bit : 1u;
    }
    return bits;
}

McWs mc_ws_layout(uint8_t *base, uint32_t nfile, uint64_t nkeys, size_t *total) {
    McWs w{};
    size_t at = 0;
    auto take = [&](size_t bytes) -> uint8_t * {
        uint8_t *p = base ? base + at : nullptr;
        at += (bytes + 255) & ~(size_t)255;
        return p;
    };
    w.flag = reinterpret_cast<uint32_t *>(take(16));
    w.files = reinterpret_cast<McFile *>(take(sizeof(McFile) * (size_t)(nfile ? nfile : 1)));
    size_t lt = 0;
    w.lv = lv_ws_layout(base ? base + at : nullptr, nfile, nkeys, &lt);
    at += lt;
    w.lv.files = w.files;
    if (total) *total = at;
    return w;
}

// ---- batched level search: Manager.searchFromLevelWithSparseIndex ---------
//
// For a level >= 1 (sstable/manager.go:178-207): sort.Search over the
// level's tables in sparse-index order (sorted by MinKey, :290-303) for the
// first whose MinKey > key, index-- when > 0, then searchFromTable's
// SSTable.MayContain (:209-212, sstable.go:300-305) of that one table.  Per
// probe the answer is 5 bytes (candidate table, may bit) instead of a row of
// the nkeys x nfile matrix lsm_may_contain writes.
//
//  lv_classify_kernel: each workgroup takes 2,048 probes: Go's sort.Search
//    (h = (i + j) >> 1) over the tables' 16-byte MinKey prefixes in LDS (the
//    full keys only on a prefix tie), the candidate stored coalesced; a probe
//    the range check rejects gets its 0 here; the others are hashed once
//    (sum256) and counting-sorted by table in LDS into the workgroup's slots,
//    and the workgroup's (start, count) per table goes to a table-major grid.
//  lv_test_kernel: one workgroup per table: its row of the grid (scanned in
//    LDS) locates its probes in every classify workgroup's slots, the
//    filter's first 144 KiB are staged in LDS (the tail read through L2) and
//    each probe's k bits tested there.
// Tables beyond kLvMaxFiles take lv_probe_kernel (search over the table
// list in global memory, bits read from the image).

// The search view of table f: MinKey / MaxKey prefixes whenever the header
// decoded (stage != 1); a table whose header did not decode searches as the
// zero Header (MinKey "", what the oracle restates).  ok: header and filter
// decoded (MayContain is answered only then).
__device__ __forceinline__ McFile lv_file(const uint8_t *img, const uint64_t *file_off,
                                          const lsm_sst_meta &M, uint32_t f) {
    McFile F = mc_file(img, file_off, M, f);
    if (M.stage == 2) {  // header decoded, filter not: search by its MinKey
        const uint8_t *base = img + file_off[f];
        key_prefix(base + M.min_key_off, M.min_key_len, F.lo);
        key_prefix(base + M.max_key_off, M.max_key_len, F.hi);
    } else if (M.stage == 1) {
        F.lo_len = F.hi_len = 0;
    }
    return F;
}

__global__ __launch_bounds__(256) void lv_prep_kernel(const uint8_t *img, const uint64_t *file_off,
                                                      const lsm_sst_meta *meta, uint32_t nfile,
                                                      LvWs w) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f < nfile) w.files[f] = lv_file(img, file_off, meta[f], f);
}

// sort.Search(n, MinKey_h > key) exactly as Go's sort.go runs it.
template <typename LoAt>
__device__ __forceinline__ uint32_t lv_search(uint32_t nfile, LoAt lo_prefix, const McFile *files,
                                              const uint8_t *img, const uint32_t kw[4], uint64_t kl,
                                              const uint8_t *kp) {
    uint32_t i = 0, j = nfile;
    while (i < j) {
        const uint32_t h = (uint32_t)(((uint64_t)i + j) >> 1);
        uint32_t bw[4];
        lo_prefix(h, bw);
        int c = prefix_cmp(bw, kw);
        if (c == 0) {
            const McFile &F = files[h];
            c = bound_cmp(bw, F.lo_len, img + F.lo_at, kw, kl, kp);
        }
        if (c <= 0) i = h + 1;  // !f(h)
        else j = h;
    }
    return i;
}

__global__ __launch_bounds__(kLvThreads) void lv_classify_kernel(const uint8_t *img, uint32_t nfile,
                                                                 const uint8_t *keys, const uint64_t *koff,
                                                                 uint64_t k_begin, uint64_t nkeys, LvWs w,
                                                                 uint32_t nwg, int32_t *table,
                                                                 uint8_t *may) {
    __shared__ uint4 slo[kLvMaxFiles];
    __shared__ uint32_t lh[kLvMaxFiles];
    __shared__ uint32_t part[kLvThreads];
    const uint32_t t = threadIdx.x;
    for (uint32_t f = t; f < nfile; f += kLvThreads) {
        const McFile &F = w.files[f];
        slo[f] = make_uint4(F.lo[0], F.lo[1], F.lo[2], F.lo[3]);
        lh[f] = 0;
    }
    uint64_t k0[kLvPer], kl[kLvPer], f0[kLvPer], f1[kLvPer];
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kLvProbes + p * kLvThreads + t;
        k0[p] = i < nkeys ? koff[i] : 0;
        kl[p] = i < nkeys ? koff[i + 1] - k0[p] : 0;
    }
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kLvProbes + p * kLvThreads + t;
        f0[p] = i < nkeys ? ldg_u64_unaligned(keys + k0[p]) : 0;
        f1[p] = i < nkeys ? ldg_u64_unaligned(keys + k0[p] + 8) : 0;
    }
    uint32_t kw[kLvPer][4];
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        const uint64_t l = kl[p];
        if (l < 8) { f0[p] &= l ? (~0ull >> (64 - 8 * l)) : 0; f1[p] = 0; }
        else if (l < 16) f1[p] &= l > 8 ? (~0ull >> (128 - 8 * l)) : 0;
        kw[p][0] = __builtin_bswap32((uint32_t)f0[p]);
        kw[p][1] = __builtin_bswap32((uint32_t)(f0[p] >> 32));
        kw[p][2] = __builtin_bswap32((uint32_t)f1[p]);
        kw[p][3] = __builtin_bswap32((uint32_t)(f1[p] >> 32));
    }
    __syncthreads();
    auto lo_lds = [&](uint32_t h, uint32_t bw[4]) {
        const uint4 v = slo[h];
        bw[0] = v.x; bw[1] = v.y; bw[2] = v.z; bw[3] = v.w;
    };
    uint32_t cand[kLvPer], rank[kLvPer];
    uint64_t hh[kLvPer][4];
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kLvProbes + p * kLvThreads + t;
        cand[p] = kMcNone;
        if (i >= nkeys) continue;
        const uint8_t *kp = keys + k0[p];
        const uint32_t lo = lv_search(nfile, lo_lds, w.files, img, kw[p], kl[p], kp);
        const uint32_t idx = lo ? lo - 1 : 0;  // manager.go:189-191
        table[i] = (int32_t)idx;
        // MayContain (sstable.go:301): lo > 0 means f(lo - 1) was evaluated
        // false, i.e. MinKey <= key; then MaxKey >= key and a decoded filter
        bool test = false;
        if (lo > 0) {
            const McFile &F = w.files[idx];
            if (F.ok) {
                int r = prefix_cmp(F.hi, kw[p]);
                if (r == 0) r = bound_cmp(F.hi, F.hi_len, img + F.hi_at, kw[p], kl[p], kp);
                test = r >= 0;
            }
        }
        may[i] = test ? 1 : 0;  // the test clears a candidate whose bit is 0
        if (!test) continue;
        cand[p] = idx;
        rank[p] = atomicAdd(&lh[idx], 1u);
        sum256_pre(kp, kl[p], f0[p], f1[p], hh[p]);
    }
    __syncthreads();
    // exclusive scan of the per-table counts (<= 2,048 tables, 2 per thread)
    const uint32_t c0 = 2 * t < nfile ? lh[2 * t] : 0u, c1 = 2 * t + 1 < nfile ? lh[2 * t + 1] : 0u;
    part[t] = c0 + c1;
    __syncthreads();
    for (uint32_t d = 1; d < kLvThreads; d <<= 1) {
        const uint32_t x = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    const uint32_t ex = part[t] - c0 - c1;
    __syncthreads();  // every lh read before it is overwritten with offsets
    if (2 * t < nfile) {
        lh[2 * t] = ex;
        w.grid[(uint64_t)(2 * t) * nwg + blockIdx.x] = ex;
        w.cnt[(uint64_t)(2 * t) * nwg + blockIdx.x] = c0;
    }
    if (2 * t + 1 < nfile) {
        lh[2 * t + 1] = ex + c0;
        w.grid[(uint64_t)(2 * t + 1) * nwg + blockIdx.x] = ex + c0;
        w.cnt[(uint64_t)(2 * t + 1) * nwg + blockIdx.x] = c1;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        if (cand[p] == kMcNone) continue;
        const uint64_t i = k_begin + (uint64_t)blockIdx.x * kLvProbes + p * kLvThreads + t;
        const uint64_t slot = (uint64_t)blockIdx.x * kLvProbes + lh[cand[p]] + rank[p];
        w.ids[slot] = (uint32_t)(i - k_begin);
        const McFile &F = w.files[cand[p]];
        if (lv_compact(F)) {
            store_hash_rec(hh[p], (uint32_t)F.m, (uint32_t)F.mr, (uint32_t)(F.mr >> 32),
                           reinterpret_cast<uint32_t *>(w.rec + slot));
        } else {
            *(gptr_t<u64x2>)gbl(w.rec + slot) = u64x2{hh[p][0], hh[p][1]};
            *(gptr_t<u64x2>)gbl(w.ext + slot) = u64x2{hh[p][2], hh[p][3]};
        }
    }
}

// The filter words of F: the first `cap` bytes into LDS from the 16-byte
// boundary below them (aligned 16-byte global->LDS loads, all in flight, the
// wave chunks rotated per file so the fills of files at equal offsets
// spread over the channels).  -> bytes staged.
__device__ __forceinline__ uint64_t stage_filter(const uint8_t *src, uint64_t nbits, uint8_t *lds,
                                                 uint32_t cap, uint32_t rot_seed, uint32_t &delta) {
    const uint64_t nb = 8 * (nbits / 64 + ((nbits & 63) != 0));
    delta = (uint32_t)((uintptr_t)src & 15);
    const uint64_t in_lds = nb < cap - 16 ? nb : cap - 16;
    const uint4 *src16 = reinterpret_cast<const uint4 *>(src - delta);
    const uint32_t n16 = (uint32_t)((delta + in_lds + 15) / 16);
    const uint32_t nwc = (n16 + kWave - 1) / kWave, wave = threadIdx.x / kWave;
    const uint32_t rot = nwc ? (rot_seed * 37u) % nwc : 0;
    const uint32_t nwaves = blockDim.x / kWave;
    for (uint32_t cl = wave; cl < nwc; cl += nwaves) {
        const uint32_t c = cl + rot < nwc ? cl + rot : cl + rot - nwc;
        const uint32_t xw = c * kWave, x = xw + (threadIdx.x & (kWave - 1));
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void *)(src16 + (x < n16 ? x : n16 - 1)),
            (__attribute__((address_space(3))) void *)(lds + 16 * xw), 16, 0, 0);
    }
    return n16 ? in_lds : 0;
}


// Matrix = false: the level search's may-bit per probe (may[k]); true: the
// all-tables form's hit matrix (may[k * nfile + f]), run only when the grouped
// path holds (*flag).  Either way classify wrote each candidate's 1 and the
// test clears the candidates whose bit is 0.
template <bool Matrix>
__global__ __launch_bounds__(kLvThreads) void lv_test_kernel(const uint8_t *img, uint32_t nfile,
                                                             uint32_t nwg, LvWs w, uint64_t k_begin,
                                                             uint8_t *may, const uint32_t *flag) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fbytes[];
    __shared__ uint32_t sb[kLvMaxWgs + 1];  // first probe of each workgroup's segment
    __shared__ uint32_t sg[kLvMaxWgs];      // its first slot in that workgroup
    __shared__ uint32_t part[kLvThreads];
    if (Matrix && !flag[0]) return;
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    // the table's segments: counts scanned (nwg <= 1,024: one per thread)
    const uint32_t c = t < nwg ? w.cnt[(uint64_t)f * nwg + t] : 0u;
    if (t < nwg) sg[t] = w.grid[(uint64_t)f * nwg + t];
    part[t] = c;
    __syncthreads();
    for (uint32_t d = 1; d < kLvThreads; d <<= 1) {
        const uint32_t x = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    if (t < nwg) sb[t] = part[t] - c;
    if (t == 0) sb[nwg] = part[kLvThreads - 1];
    __syncthreads();
    const uint32_t total = sb[nwg];
    if (total == 0) return;
    const McFile F = w.files[f];
    // the slot of the table's probe q: binary search of its segment
    auto slot_of = [&](uint32_t q) -> uint64_t {
        uint32_t a = 0, b = nwg;  // last segment with sb <= q
        while (b - a > 1) {
            const uint32_t mid = (a + b) >> 1;
            if (sb[mid] <= q) a = mid;
            else b = mid;
        }
        return (uint64_t)a * kLvProbes + sg[a] + (q - sb[a]);
    };
    const bool compact = lv_compact(F);
    const uint32_t m32 = (uint32_t)F.m;
    // 2^64 mod m for the record's carried steps
    const uint32_t c64 = compact ? (mod_small(~0ull, m32, (uint32_t)F.mr, (uint32_t)(F.mr >> 32)) + 1) % m32 : 0u;
    uint32_t q = t, id = 0;
    u32x4 x = {0, 0, 0, 0}, y = {0, 0, 0, 0};
    if (q < total) {  // the first probe's hash in flight during the fill
        const uint64_t sl = slot_of(q);
        id = w.ids[sl];
        x = w.rec[sl];
        if (!compact) y = w.ext[sl];
    }
    const uint8_t *src = img + F.words_at;
    uint32_t delta;
    const uint64_t in_lds = stage_filter(src, F.nbits, fbytes, kMcLdsBytes, f, delta);
    __asm__ __volatile__("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint8_t *lb = fbytes + delta;
    while (q < total) {
        const uint32_t qn = q + kLvThreads;
        uint32_t idn = 0;
        u32x4 xn = {0, 0, 0, 0}, yn = {0, 0, 0, 0};
        if (qn < total) {
            const uint64_t sl = slot_of(qn);
            idn = w.ids[sl];
            xn = w.rec[sl];
            if (!compact) yn = w.ext[sl];
        }
        uint32_t r;
        if (compact) {
            r = filter_test_rec(F, unpack_hash_rec(x, m32, c64), m32, lb, in_lds, src);
        } else {
            const uint64_t h[4] = {(uint64_t)x.y << 32 | x.x, (uint64_t)x.w << 32 | x.z,
                                   (uint64_t)y.y << 32 | y.x, (uint64_t)y.w << 32 | y.z};
            r = filter_test(F, h, lb, in_lds, src);
        }
        if (Matrix) {
            if (!r) may[(k_begin + id) * nfile + f] = 0;  // classify wrote the 1
        }
        else if (!r) may[k_begin + id] = 0;
        q = qn;
        id = idn;
        x = xn;
        y = yn;
    }
}

// More tables than the LDS search holds: per probe, the search over the
// table list in global memory and the bits read from the image.
__global__ __launch_bounds__(256) void lv_probe_kernel(const uint8_t *img, uint32_t nfile,
                                                       const uint8_t *keys, const uint64_t *koff,
                                                       uint64_t nkeys, LvWs w, int32_t *table,
                                                       uint8_t *may) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nkeys;
         i += (uint64_t)gridDim.x * 256) {
        const uint64_t k0 = koff[i], kl = koff[i + 1] - k0;
        const uint8_t *kp = keys + k0;
        uint32_t kw[4];
        for (uint32_t j = 0; j < 4; j++) kw[j] = be_word_at(kp, kl, j);
        auto lo_g = [&](uint32_t h, uint32_t bw[4]) {
            for (int j = 0; j < 4; j++) bw[j] = w.files[h].lo[j];
        };
        const uint32_t lo = lv_search(nfile, lo_g, w.files, img, kw, kl, kp);
        const uint32_t idx = lo ? lo - 1 : 0;
        table[i] = (int32_t)idx;
        uint8_t r = 0;
        if (lo > 0 && w.files[idx].ok) {
            const McFile &F = w.files[idx];
            if (bound_cmp_fast(F.hi, F.hi_len, img + F.hi_at, kw, kl, kp) >= 0) {
                uint64_t h[4];
                sum256(kp, kl, h);
                const uint8_t *src = img + F.words_at;
                r = (uint8_t)filter_test<false>(F, h, nullptr, 0, src);
            }
        }
        may[i] = r;
    }
}

// ---- batched Get past MayContain: Iterator.Seek + GetValueByOffset ---------
//
// searchFromTable (sstable/manager.go:209-223) after its MayContain: Seek
// (sstable/block/index.go:157-181: left, right := 0, n; mid := left +
// (right-left)/2; Indexes[mid].Key < target -> left = mid + 1, else right =
// mid; valid only if Indexes[left].Key == target) over the table's decoded
// IndexBlock, then Iterator.Value -> GetValueByOffset (sstable.go:271-296:
// Seek to the entry's offset, Value.DecodeFrom, kv.go:181-200).  One thread
// per probe; the bisection compares 16-byte big-endian prefixes loaded from
// the index entries in the image (the bytes past them only on a prefix tie).
struct GetArgs {
    const uint8_t *img;
    const uint64_t *file_off, *file_len;
    const lsm_sst_meta *meta;
    uint32_t nfile;
    const uint64_t *rec_base;
    const lsm_rec_desc *idx_desc;
    const int64_t *idx_value;
    const uint8_t *keys;
    const uint64_t *koff;
    uint64_t nkeys;
    const int32_t *table;
    const uint8_t *may;
    int32_t *result;
    lsm_rec_desc *value;
    const uint8_t *tree;  // the Seek tree (lsm_level_get_tree_build), or null
    uint32_t tree_nidx;   // the tree's max_nidx: larger tables walk the index
    uint32_t tree_top;    // levels in the tree's top block (1-3)
    uint64_t tree_stride; // bytes per table
};

// The Seek tree.  Go's bisection over a table's n index entries visits a
// fixed binary tree of midpoints (the midpoint of [l, r) is l + (r - l)/2
// whatever the keys hold), so it is laid down once per level -- as the
// decoded IndexBlocks are, when the level is loaded -- in 128-byte blocks of
// three tree levels: seven nodes of the key's 16-byte big-endian prefix
// (bytes 0-111) and its length capped at 0xFFFF (u16 at 112 + 2j).  A probe
// then reads one 128-byte line per three steps instead of an index
// descriptor and a key line per step, and takes exactly Go's steps, so any
// index -- sorted or not -- lands where Seek lands.  Blocks: with D =
// bitlen(max_nidx) levels, the top block holds the first t = D - 3(G - 1)
// levels (G = ceil(D / 3) groups); group g >= 1 holds 2^t 8^(g-1) blocks,
// block i's child c (the three steps taken in it, first step in the high
// bit) being block 8i + c of the next group (the top block's children: its
// exit c < 2^t).  Node j of a block (0-6, breadth-first) lies on the path
// (block path, bits of j + 1 below the leading one; 1 = the right half).
struct TreeShape {
    uint32_t D, G, t;
    uint64_t blocks;
};

__host__ __device__ inline TreeShape tree_shape(uint32_t max_nidx) {
    TreeShape T{0, 0, 0, 0};
    while (T.D < 32 && (max_nidx >> T.D)) T.D++;
    if (T.D == 0) return T;
    T.G = (T.D + 2) / 3;
    T.t = T.D - 3 * (T.G - 1);
    T.blocks = 1 + ((1ull << T.t) * (((1ull << (3 * (T.G - 1))) - 1) / 7));
    return T;
}


// One thread per (table, block, node slot 0-7; slot 7 idle).
__global__ __launch_bounds__(256) void get_tree_build_kernel(GetArgs a, uint8_t *tree, TreeShape T) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t f = gid / (8 * T.blocks);
    if (f >= a.nfile) return;
    const uint64_t b = (gid - f * 8 * T.blocks) >> 3;
    const uint32_t j = (uint32_t)(gid & 7);
    const uint32_t n = a.meta[f].nidx;
    if (j == 7 || n > a.tree_nidx) return;
    // the block's group g and index i in it, its root's depth and path
    uint64_t off = 1, cnt = 1ull << T.t, i = 0;
    uint32_t depth = 0;
    if (b > 0) {
        depth = T.t;
        while (b >= off + cnt) {
            off += cnt;
            cnt *= 8;
            depth += 3;
        }
        i = b - off;
    }
    const uint32_t levels = b == 0 ? T.t : 3;
    const uint32_t ld = 31 - __builtin_clz(j + 1);
    if (ld >= levels) return;
    const uint64_t path = (i << ld) | (uint64_t)(j + 1 - (1u << ld));
    depth += ld;
    uint32_t l = 0, r = n;
    for (uint32_t s = depth; s-- > 0 && l < r;) {
        const uint32_t mid = l + (r - l) / 2;
        if ((path >> s) & 1) l = mid + 1;
        else r = mid;
    }
    uint32_t kw[4] = {0, 0, 0, 0}, len = 0;  // an empty interval is never walked
    if (l < r) {
        const uint64_t base = a.rec_base ? a.rec_base[f] : a.file_off[f] / 4;
        const lsm_rec_desc d = a.idx_desc[base + l + (r - l) / 2];
        key_prefix(a.img + d.rec_off + 4, d.key_len, kw);
        len = d.key_len < 0xFFFFu ? d.key_len : 0xFFFFu;
    }
    uint8_t *blk = tree + f * a.tree_stride + b * 128;
    u32x4 o;
    o.x = kw[0]; o.y = kw[1]; o.z = kw[2]; o.w = kw[3];
    *reinterpret_cast<u32x4 *>(blk + 16 * j) = o;
    *reinterpret_cast<uint16_t *>(blk + 112 + 2 * j) = (uint16_t)len;
}

// Go's comparison of index entry (prefix ew, length el -- exact up to 16,
// capped past it -- at mid) against the probe: the prefix, then the lengths
// when either key fits in 16 bytes (the bytes both hold are then all in the
// prefixes), the bytes past 16 otherwise.
__device__ __forceinline__ int tree_cmp(const GetArgs &a, uint64_t base, uint32_t mid, const uint32_t ew[4],
                                        uint32_t el, const uint32_t kw[4], uint64_t kl, const uint8_t *kp) {
    int c = prefix_cmp(ew, kw);
    if (c == 0) {
        if (el <= 16 || kl <= 16) {
            c = (uint64_t)el < kl ? -1 : (uint64_t)el > kl ? 1 : 0;
        } else {
            const lsm_rec_desc d = a.idx_desc[base + mid];
            c = bound_cmp(ew, d.key_len, a.img + d.rec_off + 4, kw, kl, kp);
        }
    }
    return c;
}

// searchFromTable past MayContain (manager.go:209-223) on table t: Go's
// bisection (through the Seek tree, or over the index), the exact-match
// test, then GetValueByOffset (sstable.go:271-296).  -> a lsm_get_result;
// the value's view in v on LSM_GET_FOUND.
__device__ __forceinline__ int32_t get_in_table(const GetArgs &a, uint32_t t, const uint32_t kw[4],
                                                uint64_t kl, const uint8_t *kp, lsm_rec_desc &v) {
    int32_t res = LSM_GET_ABSENT;
    // the table's top tree block is loaded beside its meta (its address does
    // not depend on the index size): one dependent round trip fewer
    u32x4 top[8];
    const uint8_t *tb = a.tree + (uint64_t)t * a.tree_stride;
    if (a.tree) {
        const u32x4 *B = reinterpret_cast<const u32x4 *>(tb);
#pragma unroll
        for (int q = 0; q < 8; q++) top[q] = B[q];
    }
    const lsm_sst_meta &M = a.meta[t];
    const uint64_t fo = a.file_off[t], fl = a.file_len[t];
    const uint64_t base = a.rec_base ? a.rec_base[t] : fo / 4;
    const uint32_t n = M.nidx;
    uint32_t left = 0, right = n;
    bool hit = false;
    if (a.tree && n <= a.tree_nidx) {
        // Go's bisection through the Seek tree: one 128-byte block per
        // three steps.  The final left is the midpoint of the last step
        // that set right, so Indexes[left].Key == target is that step's
        // comparison being 0 (hit).
        uint64_t off = 0, cnt = 1, bi = 0;
        uint32_t levels = a.tree_top;
        // the steps of one block (nodes nd), then the child block's position
        auto walk_block = [&](const u32x4 (&nd)[8]) {
            uint32_t j = 0;
#pragma unroll
            for (uint32_t d = 0; d < 3; d++) {
                if (d >= levels || left >= right) break;
                u32x4 e = nd[0];
                if (d == 1) e = j == 1 ? nd[1] : nd[2];
                if (d == 2) {
                    const u32x4 lo = j == 3 ? nd[3] : nd[4], hi = j == 5 ? nd[5] : nd[6];
                    e = j < 5 ? lo : hi;
                }
                const uint32_t lw = j < 2 ? nd[7].x : j < 4 ? nd[7].y : j < 6 ? nd[7].z : nd[7].w;
                const uint32_t el = (lw >> (16 * (j & 1))) & 0xFFFFu;
                const uint32_t ew[4] = {e.x, e.y, e.z, e.w};
                const uint32_t mid = left + (right - left) / 2;
                const int c = tree_cmp(a, base, mid, ew, el, kw, kl, kp);
                if (c < 0) {
                    left = mid + 1;
                    j = 2 * j + 2;
                } else {
                    right = mid;
                    hit = c == 0;
                    j = 2 * j + 1;
                }
            }
            // the child block: group g + 1, index 8 bi + the exit's rank
            bi = off == 0 ? j - ((1u << levels) - 1) : 8 * bi + (j - 7);
            off += cnt;
            cnt = off == 1 ? (1ull << a.tree_top) : cnt * 8;
            levels = 3;
        };
        if (left < right) walk_block(top);  // the top block, already loaded
        while (left < right) {
            const u32x4 *B = reinterpret_cast<const u32x4 *>(tb + (off + bi) * 128);
            u32x4 nd[8];
#pragma unroll
            for (int q = 0; q < 8; q++) nd[q] = B[q];
            walk_block(nd);
        }
    } else {
        // Go's bisection over the index (a variant loading both possible
        // next midpoints' entries before each compare measured slower:
        // 0.549 vs 0.375 ms per 1M-key Get, 3.0 GB of HBM traffic per
        // call -- round 5, A/B)
        while (left < right) {
            const uint32_t mid = left + (right - left) / 2;
            const lsm_rec_desc d = a.idx_desc[base + mid];
            const uint8_t *ep = a.img + d.rec_off + 4;
            uint32_t ew[4];
            key_prefix(ep, d.key_len, ew);
            const int c = bound_cmp_fast(ew, d.key_len, ep, kw, kl, kp);
            if (c < 0) left = mid + 1;  // Indexes[mid].Key < target
            else right = mid;
        }
        if (left < n) {
            const lsm_rec_desc d = a.idx_desc[base + left];
            const uint8_t *ep = a.img + d.rec_off + 4;
            hit = d.key_len == kl && go_cmp(ep, d.key_len, kp, kl) == 0;
        }
    }
    if (hit) {
        const int64_t off = a.idx_value[base + left];
        if (off < 0) {
            res = LSM_GET_SEEK_FAILED;  // file.Seek to a negative offset
        } else {
            // Value.DecodeFrom from the file at off: u32 length, cap, bytes
            const uint64_t rem = (uint64_t)off < fl ? fl - (uint64_t)off : 0;
            if (rem < 4) {
                res = LSM_GET_VALUE_LENGTH;
            } else {
                const uint8_t *vp = a.img + fo + (uint64_t)off;
                const uint32_t vl = (uint32_t)vp[0] | (uint32_t)vp[1] << 8 | (uint32_t)vp[2] << 16 |
                                    (uint32_t)vp[3] << 24;
                if (vl > (1u << 30)) res = LSM_GET_VALUE_TOO_LONG;
                else if (rem - 4 < vl) res = LSM_GET_VALUE_SHORT;
                else {
                    res = LSM_GET_FOUND;
                    v = lsm_rec_desc{fo + (uint64_t)off, 0, vl};
                }
            }
        }
    }
    return res;
}

__global__ __launch_bounds__(256) void level_get_kernel(GetArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nkeys) return;
    int32_t res = LSM_GET_ABSENT;
    lsm_rec_desc v{0, 0, 0};
    const int32_t t = a.table[i];
    if (a.may[i] && t >= 0 && (uint32_t)t < a.nfile) {
        const uint64_t k0 = a.koff[i], kl = a.koff[i + 1] - k0;
        const uint8_t *kp = a.keys + k0;
        uint32_t kw[4];
        key_prefix(kp, kl, kw);
        res = get_in_table(a, (uint32_t)t, kw, kl, kp, v);
    }
    a.result[i] = res;
    a.value[i] = v;
}

// ---- level 0: Manager.searchFromLevel0 (manager.go:160-176) ---------------
//
// Level 0's tables overlap (each is one memtable flush, newest first:
// addNewSSTables prepends, manager.go:284-287), so a key is searched in every
// table in order: searchFromTable (:209-223) -- MayContain (the range check,
// then Filter.Test), Seek, the value -- and the first non-nil value or error
// ends the search.  One thread per key: the key is hashed once, the tables'
// bounds and filter shapes are staged per workgroup in LDS tiles, and a
// false positive or a Seek miss moves on to the next table.
constexpr uint32_t kL0Threads = 256;
constexpr uint32_t kL0Tile = 64;

// Filter.Test (bloom.go:371-379) of an image's stored filter, every m (the
// per-probe path's form: sixteen bit reads in flight at a time).
__device__ __forceinline__ uint32_t filter_test_any(const McFile &F, const uint64_t h[4], const uint8_t *img) {
    const uint64_t m = F.m;
    // hashNum 0: true; m == 0 < k: Go panics, answered false
    uint32_t r = F.k == 0 || m != 0;
    for (uint32_t j0 = 0; j0 < F.k && r; j0 += 16) {
        uint32_t bits = 1;
#pragma unroll
        for (uint32_t u = 0; u < 16; u++) {
            const uint32_t j = j0 + u;
            if (j < F.k) {
                const uint64_t x = location(h[0], h[1], h[2], h[3], j);
                const uint64_t p = m < (1ull << 63) ? mod_barrett(x, m, F.mr) : x % m;
                bits &= p < F.nbits ? (uint32_t)(img[F.words_at + 8 * (p >> 6) + 7 - ((p & 63) >> 3)] >> (p & 7)) & 1
                                    : 0u;
            }
        }
        r &= bits;
    }
    return r;
}

__global__ __launch_bounds__(kL0Threads) void level0_get_kernel(GetArgs a, int32_t *table_out) {
    __shared__ McFile tile[kL0Tile];
    const uint64_t i = (uint64_t)blockIdx.x * kL0Threads + threadIdx.x;
    const bool act = i < a.nkeys;
    uint64_t k0 = 0, kl = 0;
    uint32_t kw[4] = {0, 0, 0, 0};
    if (act) {
        k0 = a.koff[i];
        kl = a.koff[i + 1] - k0;
        key_prefix(a.keys + k0, kl, kw);
    }
    const uint8_t *kp = a.keys + k0;
    uint64_t h[4] = {0, 0, 0, 0};
    bool hashed = false, done = !act;
    int32_t res = LSM_GET_ABSENT, tab = -1;
    lsm_rec_desc v{0, 0, 0};
    for (uint32_t f0 = 0; f0 < a.nfile; f0 += kL0Tile) {
        const uint32_t nt = a.nfile - f0 < kL0Tile ? a.nfile - f0 : kL0Tile;
        __syncthreads();  // the previous tile is consumed
        for (uint32_t t = threadIdx.x; t < nt; t += kL0Threads) tile[t] = mc_file(a.img, a.file_off, a.meta[f0 + t], f0 + t);
        __syncthreads();
        for (uint32_t t = 0; t < nt && !done; t++) {
            const McFile &F = tile[t];
            // MayContain (sstable.go:300-305): a table whose header or filter
            // did not decode answers false (the Manager never loads one)
            if (!F.ok) continue;
            if (bound_cmp_fast(F.lo, F.lo_len, a.img + F.lo_at, kw, kl, kp) > 0 ||
                bound_cmp_fast(F.hi, F.hi_len, a.img + F.hi_at, kw, kl, kp) < 0)
                continue;
            if (!hashed) {
                sum256(kp, kl, h);
                hashed = true;
            }
            if (!filter_test_any(F, h, a.img)) continue;
            const int32_t r = get_in_table(a, f0 + t, kw, kl, kp, v);
            if (r != LSM_GET_ABSENT) {  // a value or an error: the search ends
                res = r;
                tab = (int32_t)(f0 + t);
                done = true;
            }
        }
    }
    if (act) {
        a.result[i] = res;
        a.value[i] = v;
        table_out[i] = tab;
    }
}

// ---- the whole tree: Manager.Search (manager.go:99-133) --------------------
//
// Level 0 as searchFromLevel0 (:160-176), then each non-empty level 1..6 as
// searchFromLevelWithSparseIndex + searchFromTable (:178-223); the first value
// or error ends a key's search.  The tree is one table list, level L being
// tables [start[L], start[L + 1]); files = lsm_level_index_build over it.
// One thread per key does the whole of Search: the key is hashed once (at its
// first table whose range admits it), a deeper level is searched only while
// the key is still unanswered, and the filter bits are read from the image.
// (The tables' MinKey prefixes staged in LDS for the sort.Search steps gave
// 0.508 against 0.518 ms per 1M keys on the bench tree: not kept.)
// A grouped form (every level's candidates classified and hashed once, one
// filter test per table from LDS as lv_test_kernel, then the Gets in Manager
// order) measured slower on the bench tree, 1.21 against 0.52 ms per 1M keys
// (DESIGN.md sections 5 and 7): its passes are short latency-bound launches and the
// test's one workgroup per table follows the tree's skew.
constexpr uint32_t kSrLevels = LSM_SEARCH_LEVELS;
constexpr uint32_t kSrMaxGrid = 8192;  // workgroups (grid-stride past them)

struct SrShape {
    uint32_t start[kSrLevels + 1];
};

// lsm_db_get's instantiation (DB): database.Get's second half.  A key the
// memtables answered (db.mem_result, lsm_memtable_search's) does none of the
// search -- no hash, no filter test, no Seek -- and keeps the value view the
// memtable search wrote; the others run Search as below and db.src says where
// Get's value lies.  lsm_search's kernel (search_body<false>) compiles none of
// this and takes the arguments it always took.
struct SrDb {
    const int32_t *mem_result;
    int32_t *src;
    int mode;
};

template <bool DB>
__device__ __forceinline__ void search_body(const GetArgs &a, const McFile *files, const SrShape &S,
                                            int32_t *level_out, int32_t *table_out, const SrDb &db) {
    const uint32_t n0 = S.start[1];
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.nkeys;
         i += (uint64_t)gridDim.x * 256) {
        if constexpr (DB) {
            // database.go:29: `if value != nil` -- EXACT sends a tombstone's nil on to the tables
            const int32_t m = db.mem_result[i];
            if (m == LSM_MEM_VALUE || (m == LSM_MEM_DELETED && db.mode == LSM_DBGET_TOMBSTONE_HIDES)) {
                a.result[i] = LSM_GET_ABSENT;
                table_out[i] = -1;
                level_out[i] = -1;
                db.src[i] = LSM_SRC_MEMTABLE;
                continue;
            }
        }
        const uint64_t k0 = a.koff[i], kl = a.koff[i + 1] - k0;
        const uint8_t *kp = a.keys + k0;
        uint32_t kw[4];
        key_prefix(kp, kl, kw);
        uint64_t h[4] = {0, 0, 0, 0};
        bool hashed = false;
        int32_t res = LSM_GET_ABSENT, tab = -1, lev = -1;
        lsm_rec_desc v{0, 0, 0};
        // step s: level-0 table s, then level s - n0 + 1
        for (uint32_t s = 0; s < n0 + kSrLevels - 1 && res == LSM_GET_ABSENT; s++) {
            const uint32_t L = s < n0 ? 0 : s - n0 + 1;
            uint32_t f = s;
            bool in_range;
            if (L == 0) {  // searchFromLevel0: every table, MayContain's range check
                const McFile &F = files[f];
                in_range = F.ok && bound_cmp_fast(F.lo, F.lo_len, a.img + F.lo_at, kw, kl, kp) <= 0 &&
                           bound_cmp_fast(F.hi, F.hi_len, a.img + F.hi_at, kw, kl, kp) >= 0;
            } else {  // searchFromLevelWithSparseIndex over the level's sub-range
                const uint32_t base = S.start[L], n = S.start[L + 1] - base;
                if (n == 0) continue;  // manager.go:194: no candidate in an empty level
                auto lo_at = [&](uint32_t x, uint32_t bw[4]) {
                    for (int j = 0; j < 4; j++) bw[j] = files[base + x].lo[j];
                };
                const uint32_t lo = lv_search(n, lo_at, files + base, a.img, kw, kl, kp);
                f = base + (lo ? lo - 1 : 0);  // manager.go:189-191
                const McFile &F = files[f];
                // MayContain: lo > 0 means MinKey <= key; then MaxKey >= key
                in_range = lo > 0 && F.ok && bound_cmp_fast(F.hi, F.hi_len, a.img + F.hi_at, kw, kl, kp) >= 0;
            }
            if (!in_range) continue;
            if (!hashed) {
                sum256(kp, kl, h);
                hashed = true;
            }
            const McFile &F = files[f];
            // Filter.Test as each level's own entry runs it (they differ only
            // on a corrupted m >= 2^63): lsm_level0_get's, lv_probe_kernel's.
            // All k bits in flight: reading the first two bits first (they
            // reject most absent keys of a 15 % full filter) measured slower,
            // 0.588 against 0.518 ms per 1M keys
            const uint32_t pass = L == 0 ? filter_test_any(F, h, a.img)
                                         : filter_test<false>(F, h, nullptr, 0, a.img + F.words_at);
            if (!pass) continue;
            res = get_in_table(a, f, kw, kl, kp, v);
            if (res != LSM_GET_ABSENT) {  // a value or an error: the search ends
                tab = (int32_t)f;
                lev = (int32_t)L;
            }
        }
        a.result[i] = res;
        a.value[i] = v;
        table_out[i] = tab;
        level_out[i] = lev;
        if constexpr (DB) db.src[i] = res == LSM_GET_ABSENT ? LSM_SRC_NONE : LSM_SRC_SSTABLE;
    }
}

// lsm_search's kernel: its arguments are what they were before lsm_db_get
__global__ __launch_bounds__(256) void search_kernel(GetArgs a, const McFile *files, SrShape S,
                                                     int32_t *level_out, int32_t *table_out) {
    search_body<false>(a, files, S, level_out, table_out, SrDb{});
}

__global__ __launch_bounds__(256) void db_search_kernel(GetArgs a, const McFile *files, SrShape S,
                                                        int32_t *level_out, int32_t *table_out, SrDb db) {
    search_body<true>(a, files, S, level_out, table_out, db);
}

template <int G>
int launch_encode_blocks(const EncodeBlocksArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(encode_blocks_kernel<G>, dim3(a.nblk), dim3(kWave * kEncWaves), 0, s, a);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

constexpr uint64_t kSliceBitsMax = 100ull * 1024 * 8;  // 100 KiB of LDS per slice

uint64_t slice_bits_for(uint64_t m) {
    uint64_t nslices = (m + kSliceBitsMax - 1) / kSliceBitsMax;
    if (nslices == 0) nslices = 1;
    uint64_t sb = (m + nslices - 1) / nslices;
    return (sb + 63) / 64 * 64;
}

}  // namespace
}  // namespace lsm

using namespace lsm;

extern "C" uint64_t lsm_encoded_size_host(int grammar, const uint64_t *koff, const uint64_t *voff,
                                          uint64_t r0, uint64_t r1) {
    uint64_t n = r1 - r0;
    switch (grammar) {
    case LSM_GRAMMAR_V: return 4 * n + (voff[r1] - voff[r0]);
    case LSM_GRAMMAR_KV: return 8 * n + (koff[r1] - koff[r0]) + (voff[r1] - voff[r0]);
    case LSM_GRAMMAR_IDX: return 12 * n + (koff[r1] - koff[r0]);
    default: return 0;
    }
}

extern "C" int lsm_encode_blocks(lsm_ctx *ctx, int grammar, const uint8_t *d_keys,
                                 const uint64_t *d_koff, const uint8_t *d_vals,
                                 const uint64_t *d_voff, const int64_t *d_idx_off,
                                 const uint64_t *d_rec_start, uint32_t nblk, uint8_t *d_out,
                                 const uint64_t *d_out_off, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nblk == 0) return 0;
    if (!d_rec_start || !d_out || !d_out_off) return LSM_EINVAL;
    if (grammar < LSM_GRAMMAR_V || grammar > LSM_GRAMMAR_IDX) return LSM_EINVAL;
    if (grammar != LSM_GRAMMAR_V && (!d_keys || !d_koff)) return LSM_EINVAL;
    if (grammar != LSM_GRAMMAR_IDX && (!d_vals || !d_voff)) return LSM_EINVAL;
    if (grammar == LSM_GRAMMAR_IDX && !d_idx_off) return LSM_EINVAL;
    EncodeBlocksArgs a;
    a.S.keys = d_keys;
    a.S.koff = d_koff;
    a.S.vals = d_vals;
    a.S.voff = d_voff;
    a.S.idx_off = d_idx_off;
    a.S.idx_base = 0;
    a.S.rs = 0;
    a.S.vrs = 0;
    a.rec_start = d_rec_start;
    a.nblk = nblk;
    a.out = d_out;
    a.out_off = d_out_off;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (grammar) {
    case LSM_GRAMMAR_V: return launch_encode_blocks<LSM_GRAMMAR_V>(a, s);
    case LSM_GRAMMAR_KV: return launch_encode_blocks<LSM_GRAMMAR_KV>(a, s);
    default: return launch_encode_blocks<LSM_GRAMMAR_IDX>(a, s);
    }
}

extern "C" uint64_t lsm_filter_block_size(uint64_t m) { return 32 + 8 * ((m + 63) / 64); }

extern "C" uint64_t lsm_segment_files_host(const uint64_t *koff, const uint64_t *voff, uint64_t n,
                                           uint64_t threshold, uint64_t *file_start) {
    // Builder.Add accumulates EstimateSize = 4+k+4+v+8 (kv.go:118-121) and the
    // driver flushes once size >= threshold (builder.go:40-42, merge.go:118-121);
    // leftovers form a last file (merge.go:125-128).  The running size of a file
    // starting at record s after record j is 16*(j+1-s) + K(j+1)-K(s) +
    // V(j+1)-V(s), monotone in j, so each boundary is a binary search.
    uint64_t nf = 0, s = 0;
    while (s < n) {
        file_start[nf++] = s;
        if (!threshold) { s = n; break; }
        const uint64_t base = 16 * s + koff[s] + voff[s];
        // smallest t in (s, n] with 16t + K(t) + V(t) - base >= threshold
        uint64_t lo = s + 1, hi = n + 1;
        while (lo < hi) {
            uint64_t mid = lo + (hi - lo) / 2;
            if (16 * mid + koff[mid] + voff[mid] - base >= threshold) hi = mid;
            else lo = mid + 1;
        }
        s = lo > n ? n : lo;
    }
    file_start[nf] = n;
    return nf;
}

extern "C" uint64_t lsm_sst_image_size_host(const uint64_t *koff, const uint64_t *voff,
                                            uint64_t r0, uint64_t r1, uint64_t m) {
    uint64_t hdr = 8;
    if (r1 > r0) hdr += (koff[r0 + 1] - koff[r0]) + (koff[r1] - koff[r1 - 1]);
    return hdr + lsm_filter_block_size(m) + lsm_encoded_size_host(LSM_GRAMMAR_V, koff, voff, r0, r1) +
           lsm_encoded_size_host(LSM_GRAMMAR_IDX, koff, voff, r0, r1) + 32;
}

// Filters of one or two LDS slices with 32-bit bit positions (go-lsm's 1.6
// Mbit default is two) hash each key once; larger ones hash per slice.
static uint32_t bloom_slices(uint64_t m) {
    const uint64_t sb = slice_bits_for(m);
    return (uint32_t)((m + sb - 1) / sb);
}
static bool hash_once_bloom(uint64_t m) { return m <= (1ull << 30) && bloom_slices(m) <= 2; }
// two slices and k <= 16: the split build (hash in sst_regions_kernel,
// bloom_or_kernel; a file's hash records are addressed by one 32-bit buffer
// offset, so at most 2^27 records per file)
static bool split_bloom(uint64_t m, uint32_t k, uint64_t max_file_records) {
    return hash_once_bloom(m) && bloom_slices(m) == 2 && m <= (1ull << kHashRecBits) && k <= kSplitMaxK &&
           max_file_records <= (1ull << 27);
}

extern "C" size_t lsm_build_sst_workspace_bytes(uint32_t nfile, uint32_t max_file_records,
                                                uint64_t m, uint32_t k) {
    // the slice-1 position lists of the two-slice hash-once filter
    if (!hash_once_bloom(m) || bloom_slices(m) < 2) return 16;
    const uint64_t kk = k ? k : 1;
    if (split_bloom(m, (uint32_t)kk, max_file_records))  // a hash record per key
        return (size_t)(4ull * kHashRecDwords * nfile * (uint64_t)max_file_records + 16);
    return (size_t)(kk * nfile * (uint64_t)max_file_records * 4 + 16);
}

static uint64_t barrett_recip(uint64_t m) { return ~0ull / m; }

// The stream build's plan outputs (lsm_build_sst_stream): nfile is then the
// bound nfile_max, the real count is *dnf on the device.
struct StreamGrid {
    const uint32_t *span_file;
    const FileDesc *desc;
    const uint32_t *plan;
    uint32_t span_max;
    const uint64_t *dnf;
};

static int build_sst_impl(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                          const uint8_t *d_vals, const uint64_t *d_voff,
                          const uint64_t *d_file_start, uint32_t nfile,
                          uint32_t max_file_records, uint64_t m, uint32_t k, uint8_t *d_out,
                          const uint64_t *d_file_off, int64_t *d_footer, void *d_workspace,
                          size_t ws_bytes, void *stream, const VViewArgs *views,
                          const StreamGrid *sg = nullptr) {
    if (!ctx || m == 0 || m >= (1ull << 63)) return LSM_EINVAL;
    if (nfile == 0) return 0;
    if (!d_keys || !d_koff || (!d_vals && !views) || !d_voff || !d_file_start || !d_out ||
        !d_file_off)
        return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nwords = (m + 63) / 64;
    const uint32_t kk = k ? k : 1;  // NewBloomFilter max(1, k) bloom.go:95-101
    const uint32_t chunks = (max_file_records + kSstChunkRecs - 1) / kSstChunkRecs;

    SstArgs a;
    a.keys = d_keys;
    a.koff = d_koff;
    a.vals = d_vals;
    a.voff = d_voff;
    a.file_start = d_file_start;
    a.out = d_out;
    a.file_off = d_file_off;
    a.footer = d_footer;
    a.m = m;
    a.nwords = nwords;
    a.k = kk;
    a.skip_v = views != nullptr;
    a.hrec = nullptr;
    a.hm = a.hrl = a.hrh = 0;
    a.span_file = sg ? sg->span_file : nullptr;
    a.desc = sg ? sg->desc : nullptr;
    a.plan = sg ? sg->plan : nullptr;

    // Bloom: filter words go straight into each image (big-endian).
    const uint64_t sb = slice_bits_for(m);
    bool forked = false, split = false;
    if (hash_once_bloom(m)) {
        // the stream build's records are indexed by stream position (16 n bytes)
        const size_t need = sg ? 0 : lsm_build_sst_workspace_bytes(nfile, max_file_records, m, kk);
        if (need > 16 && (!d_workspace || ws_bytes < need)) return LSM_ESPACE;
        if (split_bloom(m, kk, max_file_records)) {
            // Filter.Add's key hash runs inside the region writer (the keys
            // are gathered there anyway, sstable.go:322-326 feeds data, index
            // and filter in one pass); the per-slice ORs follow on the same
            // stream and store the filter words into the images.
            const uint64_t mr = barrett_recip(m);
            a.hrec = static_cast<uint32_t *>(d_workspace);
            a.hm = (uint32_t)m;
            a.hrl = (uint32_t)mr;
            a.hrh = (uint32_t)(mr >> 32);
            split = true;
        } else {
            BloomFileArgs b;
            b.keys = d_keys;
            b.koff = d_koff;
            b.file_start = d_file_start;
            b.nkeys = 0;
            b.m = m;
            b.mrecip = barrett_recip(m);
            b.k = kk;
            b.c64 = (uint32_t)((~0ull % m + 1) % m);
            b.split = (uint32_t)sb;
            b.pos = static_cast<uint32_t *>(d_workspace);
            b.maxr = max_file_records;
            b.nwords = nwords;
            b.out = d_out;
            b.file_off = d_file_off;
            b.bitmap = nullptr;
            // fork: the filters first on the caller's stream (each
            // workgroup needs 100 KiB of a CU's LDS, so they must be placed
            // before the regions fill the CUs), the regions and the framing
            // on the side stream beside them; joined below
            LSM_HIP_CHECK(hipEventRecord(ctx->fork, s));
            hipLaunchKernelGGL(bloom_file_kernel, dim3(nfile), dim3(1024), (size_t)(sb / 8), s, b);
            LSM_HIP_CHECK(hipGetLastError());
            LSM_HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->fork, 0));
            forked = true;
        }
    } else {
        BloomArgs b;
        b.keys = d_keys;
        b.koff = d_koff;
        b.file_start = d_file_start;
        b.m = m;
        b.mrecip = barrett_recip(m);
        b.k = kk;
        b.slice_bits = sb;
        b.nwords = nwords;
        b.bitmap = nullptr;
        b.nkeys = 0;
        b.out = d_out;
        b.file_off = d_file_off;
        const uint32_t nslices = (uint32_t)((m + sb - 1) / sb);
        hipLaunchKernelGGL(bloom_slices_kernel, dim3(nfile, nslices), dim3(1024), (size_t)(sb / 8), s, b);
        LSM_HIP_CHECK(hipGetLastError());
    }


    hipStream_t rs = forked ? ctx->side : s;  // the regions' stream
    // With views the V region is a copy independent of the IDX region and of
    // the filter: it runs on the side stream beside them (joined below).
    const bool vfork = views && chunks && !forked;
    if (vfork) {
        LSM_HIP_CHECK(hipEventRecord(ctx->fork, s));
        LSM_HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->fork, 0));
    }
    hipStream_t vs = vfork ? ctx->side : rs;  // the V region's stream
    // Past the fork every error still joins: kernels already queued on the
    // side stream must be ordered before the caller's stream (which may free
    // the outputs once the call returns an error).
    int rc = 0;
#define LSM_TRY(expr)                                   \
    do {                                                \
        const hipError_t _e = (expr);                   \
        if (_e != hipSuccess && rc == 0) rc = -(1000 + (int)_e); \
    } while (0)
    if (sg) {
        if (sg->span_max)
            hipLaunchKernelGGL((sst_regions_kernel<true, true>), dim3(sg->span_max), dim3(kRegWaves * kWave), 0,
                               rs, a);
        LSM_TRY(hipGetLastError());
    } else if (chunks) {
        const uint32_t rspans = (max_file_records + kRegSpanRecs - 1) / kRegSpanRecs;
        if (a.skip_v)
            hipLaunchKernelGGL((sst_regions_kernel<false, false>), dim3(nfile, rspans), dim3(kRegWaves * kWave), 0,
                               rs, a);
        else
            hipLaunchKernelGGL((sst_regions_kernel<true, false>), dim3(nfile, rspans), dim3(kRegWaves * kWave), 0,
                               rs, a);
        LSM_TRY(hipGetLastError());
        if (views && rc == 0) {
            // V descriptors: the records are copied whole (runs); KV
            // descriptors: each record assembled from its value view
            if (views->vd)
                hipLaunchKernelGGL(sst_vregion_runs_kernel, dim3(nfile, chunks), dim3(256), 0, vs, a,
                                   *views);
            else
                hipLaunchKernelGGL(sst_vregion_views_kernel, dim3(nfile, chunks), dim3(256), 0, vs,
                                   a, *views);
            LSM_TRY(hipGetLastError());
        }
    }
    if (rc == 0 && !split) {
        hipLaunchKernelGGL(sst_meta_kernel, dim3(nfile), dim3(kWave), 0, rs, a);
        LSM_TRY(hipGetLastError());
    } else if (rc == 0) {
        BloomOrArgs bo{};
        bo.file_start = d_file_start;
        bo.rec = a.hrec;
        bo.m = (uint32_t)m;
        bo.k = kk;
        bo.c64 = (uint32_t)((~0ull % m + 1) % m);
        // kOrSlices word-aligned slices per filter, one workgroup each
        const uint64_t osb = ((m + kOrSlices - 1) / kOrSlices + 63) / 64 * 64;
        bo.split = (uint32_t)osb;
        bo.nwords = nwords;
        bo.koff = d_koff;
        bo.out = d_out;
        bo.file_off = d_file_off;
        bo.nfiles = nfile;
        bo.dnf = sg ? sg->dnf : nullptr;
        hipLaunchKernelGGL(bloom_or_kernel, dim3((nfile + 7) / 8 * 16), dim3(1024), (size_t)(osb / 8), s,
                           bo, a);
        LSM_TRY(hipGetLastError());
    }
    if (forked || vfork) {  // join (also after an error): the caller's stream waits for the side
        LSM_TRY(hipEventRecord(ctx->join, ctx->side));
        LSM_TRY(hipStreamWaitEvent(s, ctx->join, 0));
    }
#undef LSM_TRY
    return rc;
}

extern "C" int lsm_build_sst(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                             const uint8_t *d_vals, const uint64_t *d_voff,
                             const uint64_t *d_file_start, uint32_t nfile,
                             uint32_t max_file_records, uint64_t m, uint32_t k, uint8_t *d_out,
                             const uint64_t *d_file_off, int64_t *d_footer, void *d_workspace,
                             size_t ws_bytes, void *stream) {
    if (!d_vals && nfile) return LSM_EINVAL;
    return build_sst_impl(ctx, d_keys, d_koff, d_vals, d_voff, d_file_start, nfile,
                          max_file_records, m, k, d_out, d_file_off, d_footer, d_workspace,
                          ws_bytes, stream, nullptr);
}

extern "C" int lsm_build_sst_views(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                                   const uint8_t *d_bytes, const lsm_rec_desc *d_key_desc,
                                   const lsm_rec_desc *d_val_desc, const uint32_t *d_idx,
                                   const uint64_t *d_voff, const uint64_t *d_file_start,
                                   uint32_t nfile, uint32_t max_file_records, uint64_t m,
                                   uint32_t k, uint8_t *d_out, const uint64_t *d_file_off,
                                   int64_t *d_footer, void *d_workspace, size_t ws_bytes,
                                   void *stream) {
    if (nfile && (!d_bytes || !d_key_desc || !d_idx)) return LSM_EINVAL;
    VViewArgs v;
    v.bytes = d_bytes;
    v.kd = reinterpret_cast<const u32x4 *>(d_key_desc);
    v.vd = reinterpret_cast<const u32x4 *>(d_val_desc);
    v.idx = d_idx;
    return build_sst_impl(ctx, d_keys, d_koff, nullptr, d_voff, d_file_start, nfile,
                          max_file_records, m, k, d_out, d_file_off, d_footer, d_workspace,
                          ws_bytes, stream, &v);
}

// ---- the builder path over one sorted stream (ABI 7) ------------------------

// Each file but the last holds EstimateSize sums >= threshold, so
// (nfile - 1) * threshold <= 16 n + key bytes + value bytes.
extern "C" uint32_t lsm_stream_max_files(uint64_t n, uint64_t key_bytes, uint64_t val_bytes,
                                         uint64_t threshold) {
    if (n == 0) return 0;
    if (threshold == 0) return 1;
    uint64_t b = (16 * n + key_bytes + val_bytes) / threshold + 1;
    if (b > n) b = n;
    return b > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)b;
}

// every record adds at least 16 to the running size, so a file reaches the
// threshold within ceil(threshold / 16) records
static uint64_t stream_max_recs(uint64_t n, uint64_t threshold) {
    if (threshold == 0) return n;
    const uint64_t r = (threshold + 15) / 16;
    return r < n ? r : n;
}
static uint64_t stream_span_max(uint64_t n, uint32_t nfile_max) {
    return (n + kRegSpanRecs - 1) / kRegSpanRecs + nfile_max;
}
static bool stream_split(uint64_t n, uint64_t threshold, uint64_t m, uint32_t k) {
    return split_bloom(m, k ? k : 1, stream_max_recs(n, threshold));
}

struct StreamWs {
    FileDesc *desc;
    uint32_t *plan;
    uint32_t *span_file;
    void *rest;  // the hash records (split build) or lsm_build_sst's workspace
    size_t rest_bytes;
};
static size_t stream_ws_layout(uint8_t *base, uint64_t n, uint64_t threshold, uint32_t nfile_max,
                               uint64_t m, uint32_t k, StreamWs *w) {
    size_t o = 64ull * nfile_max;
    const size_t pl = o;
    o += 256;
    const size_t sp = o;
    o += (4 * stream_span_max(n, nfile_max) + 255) / 256 * 256;
    const size_t rest = stream_split(n, threshold, m, k)
                            ? 4ull * kHashRecDwords * n + 16
                            : lsm_build_sst_workspace_bytes(nfile_max, (uint32_t)stream_max_recs(n, threshold), m,
                                                            k ? k : 1);
    if (w) {
        w->desc = reinterpret_cast<FileDesc *>(base);
        w->span_file = reinterpret_cast<uint32_t *>(base + sp);
        w->plan = reinterpret_cast<uint32_t *>(base + pl);
        w->rest = base + o;
        w->rest_bytes = rest;
    }
    return o + rest;
}

extern "C" size_t lsm_build_sst_stream_workspace_bytes(uint64_t n, uint64_t threshold, uint32_t nfile_max,
                                                       uint64_t m, uint32_t k) {
    return stream_ws_layout(nullptr, n, threshold, nfile_max, m, k, nullptr);
}

extern "C" uint64_t lsm_build_sst_stream_out_bytes(uint64_t n, uint64_t key_bytes, uint64_t val_bytes,
                                                   uint32_t nfile_max, uint64_t m, uint32_t align) {
    return (uint64_t)nfile_max * (lsm_filter_block_size(m) + 40 + (align ? align : 1) - 1) + 16 * n +
           3 * key_bytes + val_bytes;
}

static StreamPlanArgs stream_plan_args(const uint64_t *d_koff, const uint64_t *d_voff, uint64_t n,
                                       uint64_t threshold, uint32_t nfile_max, uint64_t *d_file_start,
                                       uint64_t *d_counts) {
    StreamPlanArgs p{};
    p.koff = d_koff;
    p.voff = d_voff;
    p.n = n;
    p.T = threshold;
    p.nfile_max = nfile_max;
    p.file_start = d_file_start;
    p.counts = d_counts;
    return p;
}

extern "C" int lsm_segment_files(lsm_ctx *ctx, const uint64_t *d_koff, const uint64_t *d_voff, uint64_t n,
                                 uint64_t threshold, uint32_t nfile_max, uint64_t *d_file_start,
                                 uint64_t *d_counts, void *stream) {
    if (!ctx || !d_file_start || !d_counts || (n && (!d_koff || !d_voff))) return LSM_EINVAL;
    const StreamPlanArgs p = stream_plan_args(d_koff, d_voff, n, threshold, nfile_max, d_file_start, d_counts);
    hipLaunchKernelGGL(sst_stream_plan_kernel, dim3(1), dim3(kSegThreads), 0, static_cast<hipStream_t>(stream), p);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int lsm_build_sst_stream(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                                    const uint8_t *d_vals, const uint64_t *d_voff, uint64_t n,
                                    uint64_t threshold, uint32_t nfile_max, uint64_t m, uint32_t k,
                                    uint32_t align, uint8_t *d_out, uint64_t *d_file_start,
                                    uint64_t *d_file_off, int64_t *d_footer, uint64_t *d_counts,
                                    void *d_workspace, size_t ws_bytes, void *stream) {
    if (!ctx || m == 0 || m >= (1ull << 63) || align == 0) return LSM_EINVAL;
    if (!d_file_start || !d_file_off || !d_counts) return LSM_EINVAL;
    if (n && (!d_keys || !d_koff || !d_vals || !d_voff || !d_out || !d_workspace)) return LSM_EINVAL;
    const uint64_t span_max = stream_span_max(n, nfile_max);
    if (span_max > 0x7FFFFFFFull) return LSM_EINVAL;
    StreamWs w;
    const size_t need = stream_ws_layout(static_cast<uint8_t *>(d_workspace), n, threshold, nfile_max, m, k, &w);
    if (ws_bytes < need) return LSM_ESPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    StreamPlanArgs p = stream_plan_args(d_koff, d_voff, n, threshold, nfile_max, d_file_start, d_counts);
    p.span_max = (uint32_t)span_max;
    p.filter_bytes = lsm_filter_block_size(m);
    p.align = align;
    p.file_off = d_file_off;
    p.desc = w.desc;
    p.span_file = w.span_file;
    p.plan = w.plan;
    hipLaunchKernelGGL(sst_stream_plan_kernel, dim3(1), dim3(kSegThreads), 0, s, p);
    LSM_HIP_CHECK(hipGetLastError());
    if (n == 0 || nfile_max == 0) return 0;
    const uint32_t maxr = (uint32_t)stream_max_recs(n, threshold);
    if (stream_split(n, threshold, m, k)) {
        // go-lsm's filter shape: every launch sized on the bounds, the counts
        // stay on the device
        StreamGrid g{w.span_file, w.desc, w.plan, (uint32_t)span_max, d_counts};
        return build_sst_impl(ctx, d_keys, d_koff, d_vals, d_voff, d_file_start, nfile_max, maxr, m, k, d_out,
                              d_file_off, d_footer, w.rest, w.rest_bytes, stream, nullptr, &g);
    }
    // other filter shapes size their launches on the real counts: read back
    uint64_t *h = static_cast<uint64_t *>(ctx->host_rb);
    LSM_HIP_CHECK(hipMemcpyAsync(h, d_counts, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    LSM_HIP_CHECK(hipStreamSynchronize(s));
    if (h[3]) return LSM_ESPACE;
    return build_sst_impl(ctx, d_keys, d_koff, d_vals, d_voff, d_file_start, (uint32_t)h[0], (uint32_t)h[1], m, k,
                          d_out, d_file_off, d_footer, w.rest, w.rest_bytes, stream, nullptr);
}

extern "C" int lsm_bloom_probe(lsm_ctx *ctx, const uint64_t *d_words, uint64_t m, uint32_t k,
                               const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                               uint8_t *d_hit, void *stream) {
    if (!ctx || m == 0 || m >= (1ull << 63)) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (!d_words || !d_keys || !d_koff || !d_hit) return LSM_EINVAL;
    uint32_t grid = (uint32_t)((nkeys + 255) / 256);
    hipLaunchKernelGGL(bloom_probe_kernel, dim3(grid), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_words, m, barrett_recip(m), k ? k : 1,
                       d_keys, d_koff, nkeys, d_hit);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" size_t lsm_may_contain_workspace_bytes(uint32_t nfile, uint64_t nkeys) {
    size_t t = 0;
    mc_ws_layout(nullptr, nfile, nkeys, &t);
    return t;
}

extern "C" int lsm_may_contain(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                               const lsm_sst_meta *d_meta, uint32_t nfile, const uint8_t *d_keys,
                               const uint64_t *d_koff, uint64_t nkeys, uint8_t *d_hit,
                               void *d_workspace, size_t ws_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0 || nfile == 0) return 0;
    if (!d_img || !d_file_off || !d_meta || !d_keys || !d_koff || !d_hit || !d_workspace)
        return LSM_EINVAL;
    size_t need = 0;
    const McWs w = mc_ws_layout(static_cast<uint8_t *>(d_workspace), nfile, nkeys, &need);
    if (ws_bytes < need) return LSM_ESPACE;
    const uint64_t grid = (nkeys + kMcThreads - 1) / kMcThreads;
    if (grid > 0x7FFFFFFFull) return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nkeys > 0xFFFFFFFFull) {  // list entries are 32-bit: the per-probe path
        LSM_HIP_CHECK(hipMemsetAsync(w.flag, 0, 4, s));
    } else {
        hipLaunchKernelGGL(mc_prep_kernel, dim3(1), dim3(256), 0, s, d_img, d_file_off, d_meta, nfile, w);
        // passes of up to 2M probes (the test kernel's segment table), as the
        // level search runs them
        const uint64_t pass = (uint64_t)kLvMaxWgs * kLvProbes;
        for (uint64_t k0 = 0; k0 < nkeys; k0 += pass) {
            const uint64_t n = nkeys - k0 < pass ? nkeys - k0 : pass;
            const uint32_t nwg = (uint32_t)((n + kMcGroupProbes - 1) / kMcGroupProbes);
            hipLaunchKernelGGL(mc_classify_kernel, dim3(nwg), dim3(kMcGroupThreads), 0, s, d_img, nfile,
                               d_keys, d_koff, k0, k0 + n, w, nwg, d_hit);
            hipLaunchKernelGGL(lv_test_kernel<true>, dim3(nfile), dim3(kLvThreads), kMcLdsBytes, s,
                               d_img, nfile, nwg, w.lv, k0, d_hit, (const uint32_t *)w.flag);
        }
    }
    const uint32_t pgrid = grid < kMcProbeGrid ? (uint32_t)grid : kMcProbeGrid;
    hipLaunchKernelGGL(may_contain_kernel, dim3(pgrid), dim3(kMcThreads), 0, s, d_img,
                       d_file_off, d_meta, nfile, d_keys, d_koff, nkeys, d_hit,
                       (const uint32_t *)w.flag);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" size_t lsm_level_may_contain_workspace_bytes(uint32_t nfile, uint64_t nkeys) {
    size_t total = 0;
    lv_ws_layout(nullptr, nfile, nkeys, &total);
    return total;
}

// The search over an index whose table array is `files` (lsm_level_index_build
// output, or the workspace's own copy built just before).
static int level_search(hipStream_t s, const uint8_t *d_img, const McFile *files, uint32_t nfile,
                        const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                        int32_t *d_table, uint8_t *d_may, LvWs w) {
    w.files = const_cast<McFile *>(files);
    if (nfile > kLvMaxFiles || nkeys > 0xFFFFFFFFull) {
        const uint64_t g = (nkeys + 255) / 256;
        hipLaunchKernelGGL(lv_probe_kernel, dim3(g < 4096 ? (uint32_t)g : 4096u), dim3(256), 0, s,
                           d_img, nfile, d_keys, d_koff, nkeys, w, d_table, d_may);
    } else {
        // passes of up to 2M probes (the test kernel's segment table)
        const uint64_t pass = (uint64_t)kLvMaxWgs * kLvProbes;
        for (uint64_t k0 = 0; k0 < nkeys; k0 += pass) {
            const uint64_t n = nkeys - k0 < pass ? nkeys - k0 : pass;
            const uint32_t nwg = (uint32_t)((n + kLvProbes - 1) / kLvProbes);
            hipLaunchKernelGGL(lv_classify_kernel, dim3(nwg), dim3(kLvThreads), 0, s, d_img, nfile,
                               d_keys, d_koff, k0, k0 + n, w, nwg, d_table, d_may);
            hipLaunchKernelGGL(lv_test_kernel<false>, dim3(nfile), dim3(kLvThreads), kMcLdsBytes, s,
                               d_img, nfile, nwg, w, k0, d_may, nullptr);
        }
    }
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int lsm_level_may_contain(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                                     const lsm_sst_meta *d_meta, uint32_t nfile,
                                     const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                                     int32_t *d_table, uint8_t *d_may, void *d_workspace,
                                     size_t ws_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (!d_keys || !d_koff || !d_table || !d_may) return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nfile == 0) {  // an empty level: no candidate (manager.go:194), nothing may be there
        LSM_HIP_CHECK(hipMemsetAsync(d_table, 0xFF, 4 * nkeys, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_may, 0, nkeys, s));
        return 0;
    }
    if (!d_img || !d_file_off || !d_meta || !d_workspace) return LSM_EINVAL;
    size_t need = 0;
    const LvWs w = lv_ws_layout(static_cast<uint8_t *>(d_workspace), nfile, nkeys, &need);
    if (ws_bytes < need) return LSM_ESPACE;
    hipLaunchKernelGGL(lv_prep_kernel, dim3((nfile + 255) / 256), dim3(256), 0, s, d_img, d_file_off,
                       d_meta, nfile, w);
    return level_search(s, d_img, w.files, nfile, d_keys, d_koff, nkeys, d_table, d_may, w);
}

extern "C" size_t lsm_level_index_bytes(uint32_t nfile) {
    return sizeof(McFile) * (size_t)(nfile ? nfile : 1);
}

extern "C" int lsm_level_index_build(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                                     const lsm_sst_meta *d_meta, uint32_t nfile, void *d_index,
                                     void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nfile == 0) return 0;
    if (!d_img || !d_file_off || !d_meta || !d_index) return LSM_EINVAL;
    LvWs w{};
    w.files = static_cast<McFile *>(d_index);
    hipLaunchKernelGGL(lv_prep_kernel, dim3((nfile + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_img, d_file_off, d_meta, nfile, w);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int lsm_level_may_contain_indexed(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index,
                                             uint32_t nfile, const uint8_t *d_keys,
                                             const uint64_t *d_koff, uint64_t nkeys, int32_t *d_table,
                                             uint8_t *d_may, void *d_workspace, size_t ws_bytes,
                                             void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (!d_keys || !d_koff || !d_table || !d_may) return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nfile == 0) {
        LSM_HIP_CHECK(hipMemsetAsync(d_table, 0xFF, 4 * nkeys, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_may, 0, nkeys, s));
        return 0;
    }
    if (!d_img || !d_index || !d_workspace) return LSM_EINVAL;
    size_t need = 0;
    const LvWs w = lv_ws_layout(static_cast<uint8_t *>(d_workspace), nfile, nkeys, &need);
    if (ws_bytes < need) return LSM_ESPACE;
    return level_search(s, d_img, static_cast<const McFile *>(d_index), nfile, d_keys, d_koff, nkeys,
                        d_table, d_may, w);
}

static GetArgs get_args(const uint8_t *d_img, const uint64_t *d_file_off, const uint64_t *d_file_len,
                        const lsm_sst_meta *d_meta, uint32_t nfile, const uint64_t *d_rec_base,
                        const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value) {
    GetArgs a{};
    a.img = d_img;
    a.file_off = d_file_off;
    a.file_len = d_file_len;
    a.meta = d_meta;
    a.nfile = nfile;
    a.rec_base = d_rec_base;
    a.idx_desc = d_idx_desc;
    a.idx_value = d_idx_value;
    return a;
}

extern "C" size_t lsm_level_get_tree_bytes(uint32_t nfile, uint32_t max_nidx) {
    return (size_t)nfile * tree_shape(max_nidx).blocks * 128;
}

extern "C" int lsm_level_get_tree_build(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                                        const lsm_sst_meta *d_meta, uint32_t nfile,
                                        const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                                        uint32_t max_nidx, void *d_tree, size_t tree_bytes,
                                        void *stream) {
    if (!ctx) return LSM_EINVAL;
    const TreeShape T = tree_shape(max_nidx);
    if (nfile == 0 || T.D == 0) return 0;
    if (!d_img || !d_file_off || !d_meta || !d_idx_desc || !d_tree) return LSM_EINVAL;
    if (tree_bytes < lsm_level_get_tree_bytes(nfile, max_nidx)) return LSM_ESPACE;
    GetArgs a = get_args(d_img, d_file_off, nullptr, d_meta, nfile, d_rec_base, d_idx_desc, nullptr);
    a.tree_nidx = max_nidx;
    a.tree_top = T.t;
    a.tree_stride = T.blocks * 128;
    const uint64_t grid = ((uint64_t)nfile * T.blocks * 8 + 255) / 256;
    if (grid > 0x7FFFFFFFull) return LSM_EINVAL;
    hipLaunchKernelGGL(get_tree_build_kernel, dim3((uint32_t)grid), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a, static_cast<uint8_t *>(d_tree), T);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

// The Seek tree of a Get: it must span nfile tables of tree_nidx entries
// (a tree built for fewer tables would be read past its end).
static int get_tree_args(GetArgs &a, uint32_t nfile, const void *d_tree, uint32_t tree_nidx,
                         size_t tree_bytes) {
    const TreeShape T = tree_shape(tree_nidx);
    if (!d_tree || !T.D) return 0;
    if (tree_bytes < lsm_level_get_tree_bytes(nfile, tree_nidx)) return LSM_ESPACE;
    a.tree = static_cast<const uint8_t *>(d_tree);
    a.tree_nidx = tree_nidx;
    a.tree_top = T.t;
    a.tree_stride = T.blocks * 128;
    return 0;
}

extern "C" int lsm_level_get(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                             const uint64_t *d_file_len, const lsm_sst_meta *d_meta, uint32_t nfile,
                             const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                             const int64_t *d_idx_value, const uint8_t *d_keys, const uint64_t *d_koff,
                             uint64_t nkeys, const int32_t *d_table, const uint8_t *d_may,
                             int32_t *d_result, lsm_rec_desc *d_value, const void *d_tree,
                             uint32_t tree_nidx, size_t tree_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (!d_keys || !d_koff || !d_table || !d_may || !d_result || !d_value) return LSM_EINVAL;
    if (nfile && (!d_img || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value))
        return LSM_EINVAL;
    GetArgs a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc,
                         d_idx_value);
    a.keys = d_keys;
    a.koff = d_koff;
    a.nkeys = nkeys;
    a.table = d_table;
    a.may = d_may;
    a.result = d_result;
    a.value = d_value;
    const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
    if (rc) return rc;
    const uint64_t grid = (nkeys + 255) / 256;
    if (grid > 0x7FFFFFFFull) return LSM_EINVAL;
    hipLaunchKernelGGL(level_get_kernel, dim3((uint32_t)grid), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int lsm_level_search_get(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index, uint32_t nfile,
                                    const uint64_t *d_file_off, const uint64_t *d_file_len,
                                    const lsm_sst_meta *d_meta, const uint64_t *d_rec_base,
                                    const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
                                    const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                                    int32_t *d_table, uint8_t *d_may, int32_t *d_result, lsm_rec_desc *d_value,
                                    const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
                                    void *d_workspace, size_t ws_bytes, void *stream) {
    // the level search (classify + per-table filter test), then the Get per
    // probe at full occupancy: a Get inside the per-table test (its LDS
    // refilled with the tree's top groups, one 1,024-thread workgroup per
    // table) measured slower, 0.123-0.144 against 0.113 ms per 1M-key call
    // 
    const int rc = lsm_level_may_contain_indexed(ctx, d_img, d_index, nfile, d_keys, d_koff, nkeys, d_table,
                                                 d_may, d_workspace, ws_bytes, stream);
    if (rc) return rc;
    return lsm_level_get(ctx, d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc, d_idx_value,
                         d_keys, d_koff, nkeys, d_table, d_may, d_result, d_value, d_tree, tree_nidx, tree_bytes,
                         stream);
}

extern "C" int lsm_level0_get(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                              const uint64_t *d_file_len, const lsm_sst_meta *d_meta, uint32_t nfile,
                              const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                              const int64_t *d_idx_value, const uint8_t *d_keys, const uint64_t *d_koff,
                              uint64_t nkeys, int32_t *d_table, int32_t *d_result, lsm_rec_desc *d_value,
                              const void *d_tree, uint32_t tree_nidx, size_t tree_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (!d_keys || !d_koff || !d_table || !d_result || !d_value) return LSM_EINVAL;
    if (nfile && (!d_img || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value))
        return LSM_EINVAL;
    GetArgs a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc,
                         d_idx_value);
    a.keys = d_keys;
    a.koff = d_koff;
    a.nkeys = nkeys;
    a.result = d_result;
    a.value = d_value;
    const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
    if (rc) return rc;
    const uint64_t grid = (nkeys + kL0Threads - 1) / kL0Threads;
    if (grid > 0x7FFFFFFFull) return LSM_EINVAL;
    hipLaunchKernelGGL(level0_get_kernel, dim3((uint32_t)grid), dim3(kL0Threads), 0,
                       static_cast<hipStream_t>(stream), a, d_table);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

// The tree's shape from level_start; false when it does not start at 0 or decreases.
static bool search_shape(const uint32_t *level_start, SrShape &S) {
    for (uint32_t L = 0; L <= kSrLevels; L++) {
        S.start[L] = level_start[L];
        if (L && S.start[L] < S.start[L - 1]) return false;
    }
    return S.start[0] == 0;
}

// One thread per key holds its whole state: nothing per probe is kept between
// launches, so the size depends on neither nkeys nor the tree.
constexpr size_t kSrWsBytes = 256;

extern "C" size_t lsm_search_workspace_bytes(const uint32_t *level_start, uint64_t nkeys) {
    SrShape S{};
    (void)nkeys;
    if (!level_start || !search_shape(level_start, S) || S.start[kSrLevels] == 0) return 0;
    return kSrWsBytes;
}

extern "C" int lsm_search(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index,
                          const uint32_t *level_start, const uint64_t *d_file_off,
                          const uint64_t *d_file_len, const lsm_sst_meta *d_meta,
                          const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                          const int64_t *d_idx_value, const uint8_t *d_keys, const uint64_t *d_koff,
                          uint64_t nkeys, int32_t *d_level, int32_t *d_table, int32_t *d_result,
                          lsm_rec_desc *d_value, const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
                          void *d_workspace, size_t ws_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    SrShape S{};
    if (!level_start || !search_shape(level_start, S)) return LSM_EINVAL;
    if (!d_keys || !d_koff || !d_level || !d_table || !d_result || !d_value) return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t nfile = S.start[kSrLevels];
    if (nfile == 0) {  // an empty tree: every key absent
        LSM_HIP_CHECK(hipMemsetAsync(d_level, 0xFF, 4 * nkeys, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_table, 0xFF, 4 * nkeys, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_result, 0, 4 * nkeys, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_value, 0, sizeof(lsm_rec_desc) * nkeys, s));
        return 0;
    }
    if (!d_img || !d_index || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value ||
        !d_workspace)
        return LSM_EINVAL;
    if (ws_bytes < kSrWsBytes) return LSM_ESPACE;
    GetArgs a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc,
                         d_idx_value);
    a.keys = d_keys;
    a.koff = d_koff;
    a.nkeys = nkeys;
    a.result = d_result;
    a.value = d_value;
    const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
    if (rc) return rc;
    const McFile *files = static_cast<const McFile *>(d_index);
    const uint64_t g = (nkeys + 255) / 256;
    const dim3 grid(g < kSrMaxGrid ? (uint32_t)g : kSrMaxGrid);
    hipLaunchKernelGGL(search_kernel, grid, dim3(256), 0, s, a, files, S, d_level, d_table);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" size_t lsm_db_get_workspace_bytes(const uint32_t *level_start, uint64_t nkeys) {
    return lsm_search_workspace_bytes(level_start, nkeys);
}

extern "C" int lsm_db_get(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc,
                          const uint32_t *d_idx, const uint64_t *d_file_start, uint32_t nlog,
                          const void *d_mem_index, size_t mem_index_bytes, const uint8_t *d_img,
                          const void *d_index, const uint32_t *level_start, const uint64_t *d_file_off,
                          const uint64_t *d_file_len, const lsm_sst_meta *d_meta, const uint64_t *d_rec_base,
                          const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value, const void *d_tree,
                          uint32_t tree_nidx, size_t tree_bytes, const uint8_t *d_keys,
                          const uint64_t *d_koff, uint64_t nkeys, int mode, int32_t *d_mem_result,
                          int32_t *d_log, uint32_t *d_slot, int32_t *d_level, int32_t *d_table,
                          int32_t *d_result, lsm_rec_desc *d_value, int32_t *d_src, void *d_workspace,
                          size_t ws_bytes, void *stream) {
    if (!ctx || (mode != LSM_DBGET_EXACT && mode != LSM_DBGET_TOMBSTONE_HIDES)) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    SrShape S{};
    if (!level_start || !search_shape(level_start, S)) return LSM_EINVAL;
    if (!d_keys || !d_koff || !d_level || !d_table || !d_result || !d_value || !d_src) return LSM_EINVAL;
    const uint32_t nfile = S.start[kSrLevels];
    // an empty tree needs none of the tree's buffers: every level of S is empty
    // and the kernel reads no table
    GetArgs a{};
    if (nfile) {
        if (!d_img || !d_index || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value ||
            !d_workspace)
            return LSM_EINVAL;
        if (ws_bytes < kSrWsBytes) return LSM_ESPACE;
        a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc, d_idx_value);
        const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
        if (rc) return rc;
    }
    a.keys = d_keys;
    a.koff = d_koff;
    a.nkeys = nkeys;
    a.result = d_result;
    a.value = d_value;
    // every check of both halves is made before the first launch
    const int rc = lsm_memtable_search(ctx, d_bytes, d_desc, d_idx, d_file_start, nlog, d_mem_index,
                                       mem_index_bytes, d_keys, d_koff, nkeys, d_mem_result, d_log, d_slot,
                                       d_value, stream);
    if (rc) return rc;
    const uint64_t g = (nkeys + 255) / 256;
    const dim3 grid(g < kSrMaxGrid ? (uint32_t)g : kSrMaxGrid);
    hipLaunchKernelGGL(db_search_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a,
                       static_cast<const McFile *>(d_index), S, d_level, d_table,
                       SrDb{d_mem_result, d_src, mode});
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int lsm_sum256(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                          uint64_t nkeys, uint64_t *d_h, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (!d_keys || !d_koff || !d_h) return LSM_EINVAL;
    uint32_t grid = (uint32_t)((nkeys + 255) / 256);
    hipLaunchKernelGGL(sum256_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_keys, d_koff, nkeys, d_h);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int lsm_bloom_build(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                               uint64_t nkeys, uint64_t m, uint32_t k, uint64_t *d_words,
                               void *stream) {
    if (!ctx || m == 0 || m >= (1ull << 63) || !d_words) return LSM_EINVAL;
    if (nkeys && (!d_keys || !d_koff)) return LSM_EINVAL;
    BloomArgs b;
    b.keys = d_keys;
    b.koff = d_koff;
    b.file_start = nullptr;
    b.m = m;
    b.mrecip = barrett_recip(m);
    b.k = k ? k : 1;
    b.slice_bits = slice_bits_for(m);
    b.nwords = (m + 63) / 64;
    b.bitmap = d_words;
    b.nkeys = nkeys;
    b.out = nullptr;
    b.file_off = nullptr;
    const uint32_t nslices = (uint32_t)((m + b.slice_bits - 1) / b.slice_bits);
    hipLaunchKernelGGL(bloom_slices_kernel, dim3(1, nslices), dim3(1024),
                       (size_t)(b.slice_bits / 8), static_cast<hipStream_t>(stream), b);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}
