// encode.hip — batched record encode and fused-bloom .sst build (gfx950).
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
#include "hashrec.h"
#include "murmur.h"
#include "scan.h"

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
// leaves per key its 16-byte hash record (hashrec.h: store_hash_rec, the
// record's layout); bloom_or_kernel then rebuilds the k locations of every
// key of its filter from them (additions only) and ORs those of its slice
// into LDS.
constexpr uint32_t kOrSlices = 2;  // bloom_or_kernel workgroups per filter

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
        Sum2 tot;
        const Sum2 x = wg_excl_scan<kSegThreads, seg_barrier>(
            Sum2{(sz + a.align - 1) / a.align * a.align, nsp}, &tot);
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



// ---- hash ------------------------------------------------------------------

__global__ __launch_bounds__(256) void sum256_kernel(const uint8_t *keys, const uint64_t *koff,
                                                     uint64_t n, uint64_t *out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t h[4];
    uint64_t k0 = koff[i];
    sum256(keys + k0, koff[i + 1] - k0, h);
    for (int j = 0; j < 4; j++) out[4 * i + j] = h[j];
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
