// decode.hip — batched record decode of length-prefixed blocks on gfx950.
//
// One wavefront (and one workgroup) owns one block: go-lsm's blocks are
// independent units, so the parallelism is across blocks.  The
// chase itself is decode_core.h's; here are its kernel and launch, the
// planning scans, the largest-first schedule, the dense compaction of decoded
// records and the lsm_decode_blocks* entries.  The whole-.sst decode (f1) is
// sstdec.hip, the WAL replay (f4) wal.hip.
#include <stdlib.h>
#include <string.h>

#include "decode_core.h"
#include "scan.h"

namespace lsm {
namespace {

// One wave (and one workgroup) per block; NCH x 1 KiB ring plus a guard
// dword so linear reads of a block's last field stay inside the array.
// PAD: kFitPad bytes of LDS more (fewer waves per CU), for launches whose
// blocks the caller declared to fit the ring.
template <int G, uint32_t NCH, bool ARENA, bool BIG = false, bool PAD = false>
__global__ __launch_bounds__(64) void decode_v2_kernel(DecodeArgs a) {
    static_assert(!PAD || (!ARENA && NCH == kRingChunks), "the pad is the 8 KiB DESC ring's");
    __shared__ __attribute__((aligned(16)))
    uint32_t ring[NCH * kChunk / 4 + 4 + (PAD ? kFitPad / 4 : 0)];
    __shared__ uint32_t tab[ARENA ? 129 : 1];
    // a caller's launch order (largest first) is kept as given.  Large blocks
    // (the 16 KiB ring) go XCD-contiguous: 64 KiB blocks 87.9 -> 86.2 us.
    // Small blocks keep the dispatch order: XCD-contiguous 4 KiB blocks
    // measured 76.7 -> 80.0 us (eight separate address streams; the chip
    // streams one interleaved window faster).
    const uint32_t b = a.order ? uni(a.order[blockIdx.x])
                               : NCH >= 16 ? xcd_linear(blockIdx.x, a.nblk) : blockIdx.x;
    const uint64_t off = uni64(a.blk_off[b]);
    const uint32_t n = uni(a.blk_len[b]);
    const bool lin = ((off & 15) + (uint64_t)n + 15) / 16 * 16 <= NCH * kChunk;
    if (ARENA) {
        // one instantiation, the ring form a runtime flag: with both forms
        // inlined the register allocator needs 248 VGPRs (and spills) for
        // what each alone does in 96
        decode_block_v2<G, NCH, false, true>(a, b, ring, tab, off, n, lin);
    } else if (lin && !BIG) {
        // (a launch above kBigLaunch blocks keeps the general chase: for 1M
        // blocks the straight-line path measured 844 against 755 us at 19
        // waves per CU and 755-765 against 752-755 us with the pad)
        decode_block_lin<G, NCH, BIG>(a, b, ring, off, n);
    } else if (lin) {
        decode_block_v2<G, NCH, true, false, BIG>(a, b, ring, tab, off, n);
    } else {
        decode_block_v2<G, NCH, false, false, BIG>(a, b, ring, tab, off, n);
    }
}

// ---- planning: exclusive scans over per-block quantities (scan.h) --------

__device__ __forceinline__ uint64_t plan_value(int mode, uint32_t len) {
    switch (mode) {
    case 0: return len / 4;   // V
    case 1: return len / 8;   // KV
    case 2: return len / 12;  // IDX
    default: return len;      // arena bytes
    }
}

__global__ __launch_bounds__(kScanThreads) void plan_tile_sums(int mode, const uint32_t *len,
                                                               uint32_t n, uint64_t *partial) {
    uint64_t s = 0;
    uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanPer;
    for (uint32_t j = 0; j < kScanPer; j++)
        if (i0 + j < n) s += plan_value(mode, len[i0 + j]);
    uint64_t tot;
    wg_excl_scan<kScanThreads>(s, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kScanThreads) void plan_tile_apply(int mode, const uint32_t *len,
                                                                uint32_t n,
                                                                const uint64_t *partial,
                                                                uint64_t *out) {
    uint64_t vals[kScanPer];
    uint64_t s = 0;
    uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanPer;
    for (uint32_t j = 0; j < kScanPer; j++) {
        vals[j] = (i0 + j < n) ? plan_value(mode, len[i0 + j]) : 0;
        s += vals[j];
    }
    uint64_t tot;
    uint64_t pre = wg_excl_scan<kScanThreads>(s, &tot) + partial[blockIdx.x];
    for (uint32_t j = 0; j < kScanPer; j++) {
        if (i0 + j < n) out[i0 + j] = pre;
        pre += vals[j];
    }
}

// Tile sums of a scan over n values: one u64 each, and never an empty workspace.
uint32_t plan_tiles(uint32_t n) {
    const uint32_t ntiles = (n + kScanTile - 1) / kScanTile;
    return ntiles ? ntiles : 1;
}
size_t plan_ws_bytes(uint32_t n) { return (size_t)plan_tiles(n) * 8; }

int plan_scan(int mode, const uint32_t *d_len, uint32_t n, uint64_t *d_out, void *ws,
              size_t ws_bytes, hipStream_t s) {
    const uint32_t ntiles = plan_tiles(n);
    if (ws_bytes < plan_ws_bytes(n) || (!ws && n)) return LSM_ESPACE;
    uint64_t *partial = static_cast<uint64_t *>(ws);
    if (n == 0) {
        LSM_HIP_CHECK(hipMemsetAsync(d_out, 0, 8, s));
        return 0;
    }
    hipLaunchKernelGGL(plan_tile_sums, dim3(ntiles), dim3(kScanThreads), 0, s, mode, d_len, n,
                       partial);
    hipLaunchKernelGGL(scan_partials_kernel<uint64_t>, dim3(1), dim3(kPartThreads), 0, s, partial,
                       ntiles, d_out, n);
    hipLaunchKernelGGL(plan_tile_apply, dim3(ntiles), dim3(kScanThreads), 0, s, mode, d_len, n,
                       partial, d_out);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

// fit: the caller declared every block to fit the 8 KiB ring (kFitPad).
template <int G, bool ARENA, uint32_t NCH = kRingChunks>
int launch_decode(const DecodeArgs &a, hipStream_t s, bool fit = false) {
    static_assert(NCH >= 2, "a record header may straddle two ring chunks");
    constexpr bool kCanPad = !ARENA && NCH == kRingChunks && G != LSM_GRAMMAR_IDX;
    const bool big = !ARENA && NCH == kRingChunks && a.nblk > kBigLaunch && !a.order;
    if (kCanPad && fit && !big)
        hipLaunchKernelGGL((decode_v2_kernel<G, NCH, false, false, kCanPad>), dim3(a.nblk), dim3(kWave), 0, s, a);
    else if (big)
        hipLaunchKernelGGL((decode_v2_kernel<G, NCH, false, true>), dim3(a.nblk), dim3(kWave), 0, s, a);
    else
        hipLaunchKernelGGL((decode_v2_kernel<G, NCH, ARENA>), dim3(a.nblk), dim3(kWave), 0, s, a);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- largest-first block schedule --------------------------------------------
//
// One wave decodes one block, and a block's chase cannot be split, so a
// batch of mixed sizes ends with a tail of the large blocks dispatched last
// streaming alone at a single wave's rate (config 5: 246 us as generated,
// 175 us with the blocks sorted largest first).  lsm_decode_blocks_scheduled
// orders the launch by size class, largest first -- quarter-octave classes
// (the leading bit and the two below it), so the order is close to sorted --
// with two small kernels and no atomics outside LDS: per tile of blocks a
// class histogram, then per tile the scatter of its block ids behind the
// larger classes and behind the earlier tiles' blocks of the same class.
// Every output is addressed by block id, so the results do not depend on
// the order.
constexpr uint32_t kSchedSub = 2;  // bits below the leading one that split an octave
constexpr uint32_t kSchedClasses = (33 - kSchedSub) << kSchedSub;
constexpr uint32_t kSchedThreads = 1024;
constexpr uint32_t kSchedPer = 16;  // blocks per thread
constexpr uint32_t kSchedTile = kSchedThreads * kSchedPer;
static_assert(kSchedClasses <= kSchedThreads, "one thread per class");

__device__ __forceinline__ uint32_t size_class(uint32_t n) {
    if (n < (1u << kSchedSub)) return n;
    const uint32_t l = 31 - __clz(n);  // kSchedSub..31
    return ((l - kSchedSub + 1) << kSchedSub) | ((n >> (l - kSchedSub)) & ((1u << kSchedSub) - 1));
}

// Class counters are kept per lane (h2[c][lane]): the lanes of one LDS
// atomic never share an address (a batch has few classes, and 64 lanes on one
// counter serialize: 7.6 us for the histogram of config 5's 37k blocks).
constexpr uint32_t kSchedLaneWords = kSchedClasses * kWave;

__device__ __forceinline__ void sched_count(const uint32_t *len, uint32_t nblk, uint32_t t0,
                                            uint32_t (*h2)[kWave], uint32_t n[kSchedPer]) {
    for (uint32_t i = threadIdx.x; i < kSchedLaneWords; i += kSchedThreads) (&h2[0][0])[i] = 0;
#pragma unroll
    for (uint32_t u = 0; u < kSchedPer; u++) {
        const uint32_t i = t0 + u * kSchedThreads;
        n[u] = i < nblk ? len[i] : 0;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < kSchedPer; u++)
        if (t0 + u * kSchedThreads < nblk) atomicAdd(&h2[size_class(n[u])][lane_id()], 1u);
    __syncthreads();
}

__global__ __launch_bounds__(kSchedThreads) void sched_hist_kernel(const uint32_t *len, uint32_t nblk,
                                                                  uint32_t *hist) {
    __shared__ uint32_t h2[kSchedClasses][kWave];
    const uint32_t t0 = blockIdx.x * kSchedTile + threadIdx.x;
    uint32_t n[kSchedPer];
    sched_count(len, nblk, t0, h2, n);
    // a wave per class: the 64 lane counters summed
    for (uint32_t c = threadIdx.x / kWave; c < kSchedClasses; c += kSchedThreads / kWave) {
        uint32_t tot;
        wave_excl_scan(h2[c][lane_id()], &tot);
        if (lane_id() == 0) hist[blockIdx.x * kSchedClasses + c] = tot;
    }
}

__global__ __launch_bounds__(kSchedThreads) void sched_scatter_kernel(const uint32_t *len,
                                                                     uint32_t nblk, uint32_t ntile,
                                                                     const uint32_t *hist,
                                                                     uint32_t *order) {
    constexpr uint32_t kScan = 128;  // classes padded to a power of two
    static_assert(kSchedClasses <= kScan && kScan <= kSchedThreads, "one thread per class");
    __shared__ uint32_t tot[kScan], base[kScan], h[kScan], suf[2][kScan];
    const uint32_t t = threadIdx.x;
    if (t < kScan) {
        uint32_t all = 0, before = 0;
        if (t < kSchedClasses) {
            for (uint32_t w0 = 0; w0 < ntile; w0 += 4) {  // four tiles' counts in flight
                uint32_t x[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) x[k] = w0 + k < ntile ? hist[(w0 + k) * kSchedClasses + t] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    all += x[k];
                    before += w0 + k < blockIdx.x ? x[k] : 0u;
                }
            }
        }
        tot[t] = all;
        base[t] = before;
        h[t] = 0;
        suf[0][t] = all;
    }
    __syncthreads();
    // every block of a larger class comes first: suffix sums over the classes
    // (a log-step scan; a serial sum per class was 124 dependent LDS reads)
    uint32_t sp = 0;
    for (uint32_t d = 1; d < kScan; d <<= 1) {
        if (t < kScan) suf[sp ^ 1][t] = suf[sp][t] + (t + d < kScan ? suf[sp][t + d] : 0u);
        sp ^= 1;
        __syncthreads();
    }
    if (t < kScan) base[t] += suf[sp][t] - tot[t];
    __syncthreads();
    const uint32_t t0 = blockIdx.x * kSchedTile + threadIdx.x;
    uint32_t n[kSchedPer];
#pragma unroll
    for (uint32_t u = 0; u < kSchedPer; u++) {
        const uint32_t i = t0 + u * kSchedThreads;
        n[u] = i < nblk ? len[i] : 0;
    }
#pragma unroll
    for (uint32_t u = 0; u < kSchedPer; u++) {
        const uint32_t i = t0 + u * kSchedThreads;
        if (i < nblk) {
            const uint32_t c = size_class(n[u]);
            order[base[c] + atomicAdd(&h[c], 1u)] = i;
        }
    }
}

}  // namespace
}  // namespace lsm

using namespace lsm;

extern "C" uint64_t lsm_max_records(int grammar, uint64_t len) {
    switch (grammar) {
    case LSM_GRAMMAR_V: return len / 4;
    case LSM_GRAMMAR_KV: return len / 8;
    case LSM_GRAMMAR_IDX: return len / 12;
    default: return 0;
    }
}

extern "C" size_t lsm_plan_workspace_bytes(uint32_t nblk) { return plan_ws_bytes(nblk); }

extern "C" int lsm_plan_rec_base(lsm_ctx *ctx, int grammar, const uint32_t *d_blk_len,
                                 uint32_t nblk, uint64_t *d_rec_base, void *d_workspace,
                                 size_t ws_bytes, void *stream) {
    if (!ctx || !d_rec_base || (nblk && !d_blk_len)) return LSM_EINVAL;
    if (grammar < LSM_GRAMMAR_V || grammar > LSM_GRAMMAR_IDX) return LSM_EINVAL;
    int mode = grammar == LSM_GRAMMAR_V ? 0 : grammar == LSM_GRAMMAR_KV ? 1 : 2;
    return plan_scan(mode, d_blk_len, nblk, d_rec_base, d_workspace, ws_bytes,
                     static_cast<hipStream_t>(stream));
}

extern "C" int lsm_plan_arena_base(lsm_ctx *ctx, const uint32_t *d_blk_len, uint32_t nblk,
                                   uint64_t *d_arena_base, void *d_workspace, size_t ws_bytes,
                                   void *stream) {
    if (!ctx || !d_arena_base || (nblk && !d_blk_len)) return LSM_EINVAL;
    return plan_scan(3, d_blk_len, nblk, d_arena_base, d_workspace, ws_bytes,
                     static_cast<hipStream_t>(stream));
}

// ---- compaction: decoded records -> one dense array -----------------------
//
// The decode writes block b's records at its capacity slots (rec_base or
// offset-addressed), so the per-record arrays are sparse.  A consumer on the
// host (or the next stage) wants them dense: out_base = exclusive scan of
// nrec (plan_scan), then one wave per block copies its nrec descriptors
// (16 B per lane, coalesced) and IDX values.
__global__ __launch_bounds__(256) void compact_kernel(int grammar, const uint64_t *blk_off,
                                                      uint32_t nblk, const u32x4 *desc,
                                                      const int64_t *idx, const uint64_t *rec_base,
                                                      const uint32_t *nrec, const uint64_t *out_base,
                                                      u32x4 *dense, int64_t *dense_idx) {
    const uint32_t b = uni(blockIdx.x * 4 + threadIdx.x / kWave);
    if (b >= nblk) return;
    const uint32_t R = grammar == LSM_GRAMMAR_V ? 4 : grammar == LSM_GRAMMAR_KV ? 8 : 12;
    const uint64_t src = rec_base ? uni64(rec_base[b]) : uni64(blk_off[b]) / R;
    const uint64_t dst = uni64(out_base[b]);
    const uint32_t n = uni(nrec[b]);
    for (uint32_t i = lane_id(); i < n; i += kWave) {
        dense[dst + i] = __builtin_nontemporal_load(&desc[src + i]);
        if (dense_idx) dense_idx[dst + i] = idx[src + i];
    }
}

extern "C" int lsm_compact_records(lsm_ctx *ctx, int grammar, const uint64_t *d_blk_off,
                                   uint32_t nblk, const lsm_decode_out *out, lsm_rec_desc *d_dense,
                                   int64_t *d_dense_idx, uint64_t *d_dense_base, void *d_workspace,
                                   size_t ws_bytes, void *stream) {
    if (!ctx || !out || !d_dense_base) return LSM_EINVAL;
    if (grammar < LSM_GRAMMAR_V || grammar > LSM_GRAMMAR_IDX) return LSM_EINVAL;
    if (nblk && (!out->desc || !out->nrec || !d_dense || (!out->rec_base && !d_blk_off)))
        return LSM_EINVAL;
    if (d_dense_idx && (grammar != LSM_GRAMMAR_IDX || !out->idx_value)) return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = plan_scan(3, out->nrec, nblk, d_dense_base, d_workspace, ws_bytes, s);
    if (rc) return rc;
    if (nblk == 0) return 0;
    hipLaunchKernelGGL(compact_kernel, dim3((nblk + 3) / 4), dim3(256), 0, s, grammar, d_blk_off,
                       nblk, reinterpret_cast<const u32x4 *>(out->desc), out->idx_value,
                       out->rec_base, out->nrec, d_dense_base, reinterpret_cast<u32x4 *>(d_dense),
                       d_dense_idx);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

// The arguments the three decode entries share.  kDecodeEmpty: valid, and
// nothing to decode (the entry returns 0 without looking at the pointers).
constexpr int kDecodeEmpty = 1;
static int decode_check(lsm_ctx *ctx, int grammar, const uint8_t *d_in, const uint64_t *d_blk_off,
                        const uint32_t *d_blk_len, uint32_t nblk, const lsm_decode_out *out) {
    if (!ctx || !out) return LSM_EINVAL;
    if (nblk == 0) return kDecodeEmpty;
    if (!d_in || !d_blk_off || !d_blk_len || !out->desc || !out->nrec || !out->status)
        return LSM_EINVAL;
    if (grammar < LSM_GRAMMAR_V || grammar > LSM_GRAMMAR_IDX) return LSM_EINVAL;
    return 0;
}

static DecodeArgs decode_args(const uint8_t *d_in, const uint64_t *d_blk_off,
                              const uint32_t *d_blk_len, uint32_t nblk, const lsm_decode_out *out,
                              const uint32_t *order) {
    DecodeArgs a;
    a.in = d_in;
    a.blk_off = d_blk_off;
    a.blk_len = d_blk_len;
    a.nblk = nblk;
    a.desc = reinterpret_cast<u32x4 *>(out->desc);
    a.rec_base = out->rec_base;
    a.nrec = out->nrec;
    a.status = out->status;
    a.idx_value = out->idx_value;
    a.key_arena = out->key_arena;
    a.val_arena = out->val_arena;
    a.arena_base = out->arena_base;
    a.key_arena_off = out->key_arena_off;
    a.val_arena_off = out->val_arena_off;
    a.order = order;
    return a;
}

// The kernel of a grammar and output mode on a ring of NCH chunks.  fit: the
// caller's bound says every block fits the 8 KiB ring (launch_decode); it
// only reaches the DESC kernels of V and KV on that ring.
template <uint32_t NCH>
static int dispatch_decode(int grammar, bool arena, const DecodeArgs &a, hipStream_t s,
                           bool fit = false) {
    fit = fit && NCH == kRingChunks;
    switch (grammar) {
    case LSM_GRAMMAR_V: return arena ? launch_decode<LSM_GRAMMAR_V, true, NCH>(a, s)
                                     : launch_decode<LSM_GRAMMAR_V, false, NCH>(a, s, fit);
    case LSM_GRAMMAR_KV: return arena ? launch_decode<LSM_GRAMMAR_KV, true, NCH>(a, s)
                                      : launch_decode<LSM_GRAMMAR_KV, false, NCH>(a, s, fit);
    default: return arena ? launch_decode<LSM_GRAMMAR_IDX, true, NCH>(a, s)
                          : launch_decode<LSM_GRAMMAR_IDX, false, NCH>(a, s);
    }
}

// lsm_decode_blocks on the 8 KiB ring, with or without the caller's bound.
static int decode_blocks_8k(lsm_ctx *ctx, int grammar, const uint8_t *d_in,
                            const uint64_t *d_blk_off, const uint32_t *d_blk_len, uint32_t nblk,
                            const lsm_decode_out *out, void *stream, bool fit) {
    if (const int rc = decode_check(ctx, grammar, d_in, d_blk_off, d_blk_len, nblk, out))
        return rc == kDecodeEmpty ? 0 : rc;
    return dispatch_decode<kRingChunks>(grammar, out->key_arena || out->val_arena,
                                        decode_args(d_in, d_blk_off, d_blk_len, nblk, out, nullptr),
                                        static_cast<hipStream_t>(stream), fit);
}

extern "C" int lsm_decode_blocks(lsm_ctx *ctx, int grammar, const uint8_t *d_in,
                                 const uint64_t *d_blk_off, const uint32_t *d_blk_len,
                                 uint32_t nblk, const lsm_decode_out *out, void *stream) {
    return decode_blocks_8k(ctx, grammar, d_in, d_blk_off, d_blk_len, nblk, out, stream, false);
}

// A caller that knows its blocks are large (max_blk_len > 32 KiB: 64 KiB data
// blocks, whole index regions) gets a 16 KiB ring: twice the bytes in flight
// per wave (6,400 x 64 KiB blocks: 89.5 against 92.6 us).  The hint only
// picks the ring; any block length decodes correctly either way.
extern "C" int lsm_decode_blocks_hinted(lsm_ctx *ctx, int grammar, const uint8_t *d_in,
                                        const uint64_t *d_blk_off, const uint32_t *d_blk_len,
                                        uint32_t nblk, uint32_t max_blk_len,
                                        const lsm_decode_out *out, void *stream) {
    // A bound of 3 KiB to the 8 KiB ring's size (any block start: 15 bytes of
    // lead) declares blocks of go-lsm's own size class, which all take the
    // straight-line path: the DESC kernel then holds kFitPad of LDS more.  A
    // block longer than the bound still decodes correctly, only slower.
    if (max_blk_len <= 32 * 1024)
        return decode_blocks_8k(ctx, grammar, d_in, d_blk_off, d_blk_len, nblk, out, stream,
                                max_blk_len > kFitMin &&
                                    max_blk_len + 15 <= kRingChunks * kChunk);
    if (const int rc = decode_check(ctx, grammar, d_in, d_blk_off, d_blk_len, nblk, out))
        return rc == kDecodeEmpty ? 0 : rc;
    return dispatch_decode<2 * kRingChunks>(grammar, out->key_arena || out->val_arena,
                                            decode_args(d_in, d_blk_off, d_blk_len, nblk, out, nullptr),
                                            static_cast<hipStream_t>(stream));
}

extern "C" size_t lsm_decode_schedule_workspace_bytes(uint32_t nblk) {
    const uint64_t ntile = ((uint64_t)nblk + kSchedTile - 1) / kSchedTile;
    return 4ull * kSchedClasses * ntile + 4ull * nblk + 16;
}

extern "C" int lsm_decode_blocks_scheduled(lsm_ctx *ctx, int grammar, const uint8_t *d_in,
                                           const uint64_t *d_blk_off, const uint32_t *d_blk_len,
                                           uint32_t nblk, const lsm_decode_out *out,
                                           void *d_workspace, size_t ws_bytes, void *stream) {
    if (const int rc = decode_check(ctx, grammar, d_in, d_blk_off, d_blk_len, nblk, out))
        return rc == kDecodeEmpty ? 0 : rc;
    if (!d_workspace || ws_bytes < lsm_decode_schedule_workspace_bytes(nblk)) return LSM_ESPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t ntile = (nblk + kSchedTile - 1) / kSchedTile;
    uint32_t *order = static_cast<uint32_t *>(d_workspace);
    uint32_t *hist = order + nblk;
    hipLaunchKernelGGL(sched_hist_kernel, dim3(ntile), dim3(kSchedThreads), 0, s, d_blk_len, nblk,
                       hist);
    hipLaunchKernelGGL(sched_scatter_kernel, dim3(ntile), dim3(kSchedThreads), 0, s, d_blk_len, nblk,
                       ntile, hist, order);
    LSM_HIP_CHECK(hipGetLastError());
    // mixed sizes: a 2 KiB ring, the most waves per CU (config 5: 201 us, 4 KiB
    // 215 us, 8 KiB 231 us; the 8 KiB ring streams uniform 64 KiB blocks
    // fastest: 92 against 100 us with 4 KiB).  Quarter-octave classes measured
    // the same as sixteenth-octave ones.
    return dispatch_decode<kRingChunks / 4>(grammar, out->key_arena || out->val_arena,
                                            decode_args(d_in, d_blk_off, d_blk_len, nblk, out, order), s);
}

