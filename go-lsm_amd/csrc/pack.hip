// pack.hip — lsm_pack_results: the answered bytes of a batched read (views
// into the WAL bytes and the .sst images) packed into two CSR arenas.
//
// The slots o = q * limit + j of the producers' ragged output become dense
// entries by one scan over the slots of {live, key length, value length}:
//   1. pack_scan_tiles: the sums of each tile of kScanTile slots;
//   2. scan_partials_kernel (scan.h) over the tile sums, the totals {E, K, V}
//      behind them -- two launches, the byte sums as a Sum2 and the live
//      counts as u64: over one Sum3 its eight loads in flight spill (132 bytes
//      of scratch a lane at its 1,024 threads);
//   3. pack_scan_apply: each live slot's entry number e and its offsets
//      (d_koff, d_voff, d_entry_slot), d_row_start at the first slot of a
//      row, the entry's two absolute source addresses in the workspace, the
//      counts and the overflow flag;
//   4. pack_copy_kernel: a wave per 64 entries, merge.hip's gather_copy_kernel
//      plan over absolute source addresses (skipped by the sizing call; on
//      overflow every wave leaves after one comparison of the totals).
// Slots that are not live are never read (descriptor or source word).
#include "common.h"
#include "scan.h"

namespace lsm {
namespace {

constexpr uint32_t kPackThreads = 256;
static_assert(kPackThreads == kScanThreads, "the per-tile scan kernels run kScanTile values a workgroup");

// live slots, key bytes and value bytes scanned together
struct Sum3 {
    uint64_t e, k, v;
};
__device__ __forceinline__ Sum3 operator+(const Sum3 &a, const Sum3 &b) {
    return Sum3{a.e + b.e, a.k + b.k, a.v + b.v};
}
__device__ __forceinline__ Sum3 wave_excl_sum(const Sum3 &v, Sum3 *total) {
    Sum3 x;
    x.e = wave_excl_scan64(v.e, &total->e);
    x.k = wave_excl_scan64(v.k, &total->k);
    x.v = wave_excl_scan64(v.v, &total->v);
    return x;
}

struct PackIn {
    const uint8_t *bytes, *img;
    const int32_t *src;
    const lsm_rec_desc *key, *value;
    const uint32_t *count;
    uint32_t nslot, limit;
};

// What a slot adds to the scan, and where its bytes lie.
struct Slot {
    uint32_t q, j;
    uint32_t live, kl, vl;
    uint64_t ka, va;  // absolute source addresses (the base chosen by d_src)
};

__device__ __forceinline__ Slot pack_slot(const PackIn &p, uint32_t o) {
    Slot s{};
    s.q = p.limit == 1 ? o : o / p.limit;
    s.j = o - s.q * p.limit;
    // j < limit always: a count above limit is clamped by that
    if (p.count && s.j >= p.count[s.q]) return s;
    s.live = 1;
    const int32_t src = p.src ? p.src[o] : (int32_t)LSM_SRC_SSTABLE;
    const uint8_t *base = src == LSM_SRC_MEMTABLE ? p.bytes : src == LSM_SRC_SSTABLE ? p.img : nullptr;
    if (!base) return s;  // LSM_SRC_NONE, or no buffer for the source: an entry of no bytes
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    const u32x4 v = reinterpret_cast<const u32x4 *>(p.value)[o];
    s.vl = v.w;
    s.va = b + ((uint64_t)v.y << 32 | v.x) + 4;
    if (p.key) {
        const u32x4 k = reinterpret_cast<const u32x4 *>(p.key)[o];
        s.kl = k.z;
        s.ka = b + ((uint64_t)k.y << 32 | k.x) + 4;
    }
    return s;
}

// The tile sums and, behind them, the totals: {K, V} and E (scan_partials_kernel's two arrays).
struct PackPart {
    Sum2 *kv;
    uint64_t *e;
};

__global__ __launch_bounds__(kPackThreads) void pack_scan_tiles(PackIn p, PackPart part) {
    Sum3 s{};
    const uint64_t o0 = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanPer;
    for (uint32_t t = 0; t < kScanPer; t++) {
        if (o0 + t < p.nslot) {
            const Slot x = pack_slot(p, (uint32_t)(o0 + t));
            s = s + Sum3{x.live, x.kl, x.vl};
        }
    }
    Sum3 tot;
    wg_excl_scan<kPackThreads>(s, &tot);
    if (threadIdx.x == 0) {
        part.kv[blockIdx.x] = Sum2{tot.k, tot.v};
        part.e[blockIdx.x] = tot.e;
    }
}

struct PackOut {
    uint64_t *row_start;
    uint32_t *entry_slot;  // optional
    uint64_t *koff;        // null: no keys
    uint64_t *voff;
    uint64_t *counts;
    uint64_t *ksrc, *vsrc;  // workspace, per entry
    uint64_t nrow;
    uint64_t key_cap, val_cap;
    uint8_t *keys, *vals;
    uint32_t ntiles;
};

__device__ __forceinline__ Sum3 pack_part(const PackPart &part, uint32_t t) {
    const Sum2 kv = part.kv[t];
    return Sum3{part.e[t], kv.s, kv.c};
}

__device__ __forceinline__ bool pack_overflow(const PackOut &w, const Sum3 &total) {
    return (w.keys && total.k > w.key_cap) || (w.vals && total.v > w.val_cap);
}

__global__ __launch_bounds__(kPackThreads) void pack_scan_apply(PackIn p, PackPart part, PackOut w) {
    Slot x[kScanPer];
    Sum3 s{};
    const uint64_t o0 = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanPer;
    for (uint32_t t = 0; t < kScanPer; t++) {
        x[t] = Slot{};
        if (o0 + t < p.nslot) {
            x[t] = pack_slot(p, (uint32_t)(o0 + t));
            s = s + Sum3{x[t].live, x[t].kl, x[t].vl};
        }
    }
    Sum3 tot;
    Sum3 at = wg_excl_scan<kPackThreads>(s, &tot) + pack_part(part, blockIdx.x);
    for (uint32_t t = 0; t < kScanPer; t++) {
        if (o0 + t < p.nslot) {
            if (x[t].j == 0) w.row_start[x[t].q] = at.e;
            if (x[t].live) {
                if (w.entry_slot) w.entry_slot[at.e] = (uint32_t)(o0 + t);
                if (w.koff) w.koff[at.e] = at.k;
                w.voff[at.e] = at.v;
                w.ksrc[at.e] = x[t].ka;
                w.vsrc[at.e] = x[t].va;
            }
        }
        at = at + Sum3{x[t].live, x[t].kl, x[t].vl};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const Sum3 T = pack_part(part, w.ntiles);
        w.row_start[w.nrow] = T.e;
        if (w.koff) w.koff[T.e] = T.k;
        w.voff[T.e] = T.v;
        w.counts[0] = T.e;
        w.counts[1] = T.k;
        w.counts[2] = T.v;
        w.counts[3] = pack_overflow(w, T) ? 1 : 0;
    }
}

// The copy: gather_copy_kernel's plan (merge.hip).  One wave per 64 entries.
// Their keys form one contiguous output range and their values another; both
// are cut into 16-byte chunks (aligned in the output) numbered in one space,
// keys first:
//   1. each lane marks, in an LDS map, the chunks that start inside its key
//      or its value;
//   2. lanes take four chunks at a time and issue every source load before
//      any store: a chunk inside one key or value is five aligned source
//      dwords funnel-shifted into one 16-byte store; any other chunk (it
//      straddles entries or an end of the range) is queued;
//   3. the queue is drained four lanes per chunk, a dword (or its bytes) each.
// Chunks are handled kMapChunks at a time (any string length).  LDS holds each
// entry's absolute source address, so the two source buffers cost nothing; an
// entry of length 0 owns no chunk and no byte, so it is never loaded from.
constexpr uint32_t kMapChunks = 1024;
constexpr uint32_t kUnroll = 4;

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Unaligned little-endian u32 at address a: two aligned dwords and a funnel shift.
__device__ __forceinline__ uint32_t ld_u32_at(uintptr_t a) {
    const gptr_t<const uint32_t> q = gbl_at<const uint32_t>(a & ~(uintptr_t)3);
    return funnel(q[0], q[1], (uint32_t)a);
}

__global__ __launch_bounds__(kPackThreads) void pack_copy_kernel(PackPart part, PackOut o) {
    const Sum3 T = pack_part(part, o.ntiles);
    if (pack_overflow(o, T)) return;  // no byte of either arena
    constexpr uint32_t W = kPackThreads / kWave;
    __shared__ uint64_t s_dst[W][2][kWave + 1];
    __shared__ uint64_t s_src[W][2][kWave];
    __shared__ uint8_t s_map[W][kMapChunks];
    __shared__ uint16_t s_q[W][kMapChunks];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    const uint64_t j0 = ((uint64_t)blockIdx.x * W + w) * kWave;
    if (j0 >= T.e) return;
    const uint32_t cnt = T.e - j0 < kWave ? (uint32_t)(T.e - j0) : kWave;
    const bool on[2] = {o.keys != nullptr, o.vals != nullptr};
    uint64_t d0[2] = {0, 0}, d1[2] = {0, 0};
    if (lane < cnt) {
        const uint64_t j = j0 + lane;
        if (on[0]) {
            d0[0] = o.koff[j];
            d1[0] = o.koff[j + 1];
            s_src[w][0][lane] = o.ksrc[j];
        }
        if (on[1]) {
            d0[1] = o.voff[j];
            d1[1] = o.voff[j + 1];
            s_src[w][1][lane] = o.vsrc[j];
        }
        s_dst[w][0][lane] = d0[0];
        s_dst[w][1][lane] = d0[1];
    }
    if (lane == 0) {
        s_dst[w][0][cnt] = on[0] ? o.koff[j0 + cnt] : 0;
        s_dst[w][1][cnt] = on[1] ? o.voff[j0 + cnt] : 0;
    }
    wave_sync();
    uint64_t A[2], B[2], X[2];
    uint32_t nc[2];
    for (int h = 0; h < 2; h++) {
        A[h] = s_dst[w][h][0];
        B[h] = s_dst[w][h][cnt];
        X[h] = A[h] & ~(uint64_t)15;
        nc[h] = B[h] > A[h] ? (uint32_t)((B[h] - X[h] + 15) / 16) : 0;
    }
    const gptr_t<uint8_t> dsts[2] = {gbl(o.keys), gbl(o.vals)};
    const uint32_t nchunk = nc[0] + nc[1];
    for (uint32_t P = 0; P < nchunk; P += kMapChunks) {
        const uint32_t np = nchunk - P < kMapChunks ? nchunk - P : kMapChunks;
        // 1. chunks whose first byte lies in my key / value
        for (int h = 0; h < 2; h++) {
            if (lane < cnt && d1[h] > d0[h]) {
                const uint64_t lo = d0[h] > X[h] ? (d0[h] - X[h] + 15) / 16 : 0;
                const uint64_t hi = (d1[h] - 1 - X[h]) / 16;
                const uint64_t base = h ? nc[0] : 0;
                const uint64_t c_lo = base + lo > P ? base + lo : P;
                const uint64_t c_hi = base + hi < (uint64_t)P + np - 1 ? base + hi : (uint64_t)P + np - 1;
                for (uint64_t c = c_lo; c <= c_hi; c++) s_map[w][c - P] = (uint8_t)lane;
            }
        }
        wave_sync();
        // 2. chunks inside one key / value, four per lane per round; queue the rest
        uint32_t qn = 0;
        for (uint32_t c0 = 0; c0 < np; c0 += kUnroll * kWave) {
            uint32_t q[kUnroll][5];
            uint32_t sh[kUnroll];
            gptr_t<uint8_t> out[kUnroll];
            bool reg[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) {
                const uint32_t c = c0 + u * kWave + lane;
                reg[u] = false;
                out[u] = nullptr;
                sh[u] = 0;
                if (c < np) {
                    const uint32_t cid = P + c;
                    const int h = cid >= nc[0];
                    const uint64_t x = X[h] + 16 * (uint64_t)(cid - (h ? nc[0] : 0));
                    if (x >= A[h] && x + 16 <= B[h]) {
                        const uint32_t r = s_map[w][c];
                        const uint64_t e0 = s_dst[w][h][r], e1 = s_dst[w][h][r + 1];
                        if (x + 16 <= e1) {
                            reg[u] = true;
                            const uintptr_t sa = (uintptr_t)(s_src[w][h][r] + (x - e0));
                            const gptr_t<const uint32_t> qa = gbl_at<const uint32_t>(sa & ~(uintptr_t)3);
                            sh[u] = (uint32_t)sa;
                            out[u] = dsts[h] + x;
#pragma unroll
                            for (int t = 0; t < 5; t++) q[u][t] = qa[t];
                        }
                    }
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) {
                if (reg[u]) {
                    u32x4 v;
                    v.x = funnel(q[u][0], q[u][1], sh[u]);
                    v.y = funnel(q[u][1], q[u][2], sh[u]);
                    v.z = funnel(q[u][2], q[u][3], sh[u]);
                    v.w = funnel(q[u][3], q[u][4], sh[u]);
                    *(gptr_t<u32x4>)out[u] = v;
                }
                const uint32_t c = c0 + u * kWave + lane;
                const bool irr = c < np && !reg[u];
                const uint64_t im = __ballot(irr);
                if (irr) s_q[w][qn + mbcnt(im)] = (uint16_t)c;
                qn += (uint32_t)__builtin_popcountll(im);
            }
        }
        wave_sync();
        // 3. queued chunks, four lanes (one dword each) per chunk
        for (uint32_t i0 = 0; i0 < qn; i0 += kWave / 4) {
            const uint32_t i = i0 + lane / 4;
            if (i >= qn) continue;
            const uint32_t c = s_q[w][i], cid = P + c;
            const int h = cid >= nc[0];
            const uint64_t x = X[h] + 16 * (uint64_t)(cid - (h ? nc[0] : 0));
            const uint64_t xd = x + 4 * (lane & 3);
            if (xd >= B[h]) continue;
            uint32_t r = x >= A[h] ? s_map[w][c] : 0;
            const uint64_t *sd = s_dst[w][h];
            const uint64_t *ss = s_src[w][h];
            const gptr_t<uint8_t> dst = dsts[h];
            while (r + 1 < cnt && xd >= sd[r + 1]) r++;
            if (xd >= A[h] && xd + 4 <= B[h] && xd >= sd[r] && xd + 4 <= sd[r + 1]) {
                *(gptr_t<uint32_t>)(dst + xd) = ld_u32_at((uintptr_t)(ss[r] + (xd - sd[r])));
            } else {
                for (uint32_t u = 0; u < 4; u++) {
                    const uint64_t b = xd + u;
                    if (b < A[h] || b >= B[h]) continue;
                    while (b >= sd[r + 1]) r++;
                    dst[b] = *gbl_at<const uint8_t>((uintptr_t)(ss[r] + (b - sd[r])));
                }
            }
        }
        wave_sync();
    }
}

// ---- workspace ------------------------------------------------------------

struct PackWs {
    PackPart part;  // the tile sums, the totals behind them
    uint64_t *ksrc, *vsrc;
    size_t total;
};

PackWs pack_ws_layout(uint8_t *base, uint64_t nslot) {
    PackWs w{};
    WsCursor c{base, 0};
    const size_t ntiles = (size_t)((nslot + kScanTile - 1) / kScanTile);
    w.part.kv = c.take<Sum2>(ntiles + 1);
    w.part.e = c.take<uint64_t>(ntiles + 1);
    w.ksrc = c.take<uint64_t>((size_t)nslot);
    w.vsrc = c.take<uint64_t>((size_t)nslot);
    w.total = c.at;
    return w;
}

}  // namespace
}  // namespace lsm

using namespace lsm;

extern "C" size_t lsm_pack_results_workspace_bytes(uint64_t nrow, uint32_t limit) {
    if (nrow == 0 || limit == 0) return 0;
    uint64_t nslot;
    if (__builtin_mul_overflow(nrow, (uint64_t)limit, &nslot)) return SIZE_MAX;
    if (nslot >= (1ull << 59)) return SIZE_MAX;  // 16 bytes a slot and the tile sums leave 64 bits
    return pack_ws_layout(nullptr, nslot).total;
}

extern "C" int lsm_pack_results(lsm_ctx *ctx, const uint8_t *d_bytes, const uint8_t *d_img, const int32_t *d_src,
                                const lsm_rec_desc *d_key, const lsm_rec_desc *d_value, const uint32_t *d_count,
                                uint64_t nrow, uint32_t limit, uint8_t *d_keys, uint64_t key_cap, uint8_t *d_vals,
                                uint64_t val_cap, uint64_t *d_row_start, uint32_t *d_entry_slot, uint64_t *d_koff,
                                uint64_t *d_voff, uint64_t *d_counts, void *d_workspace, size_t ws_bytes,
                                void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nrow == 0) return 0;
    if (limit == 0 || nrow >= (1ull << 32) || nrow * limit >= (1ull << 32)) return LSM_EINVAL;
    if (!d_value || !d_row_start || !d_voff || !d_counts) return LSM_EINVAL;
    if (d_key && !d_koff) return LSM_EINVAL;
    if (d_keys && !d_key) return LSM_EINVAL;
    if (!d_src && !d_img) return LSM_EINVAL;
    const uint64_t nslot = nrow * limit;
    const PackWs ws = pack_ws_layout(static_cast<uint8_t *>(d_workspace), nslot);
    if (!d_workspace || ws_bytes < ws.total) return LSM_ESPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PackIn p{};
    p.bytes = d_bytes;
    p.img = d_img;
    p.src = d_src;
    p.key = d_key;
    p.value = d_value;
    p.count = d_count;
    p.nslot = (uint32_t)nslot;
    p.limit = limit;
    PackOut o{};
    o.row_start = d_row_start;
    o.entry_slot = d_entry_slot;
    o.koff = d_key ? d_koff : nullptr;
    o.voff = d_voff;
    o.counts = d_counts;
    o.ksrc = ws.ksrc;
    o.vsrc = ws.vsrc;
    o.nrow = nrow;
    o.key_cap = key_cap;
    o.val_cap = val_cap;
    o.keys = d_keys;
    o.vals = d_vals;
    const uint32_t ntiles = (uint32_t)((nslot + kScanTile - 1) / kScanTile);
    o.ntiles = ntiles;
    hipLaunchKernelGGL(pack_scan_tiles, dim3(ntiles), dim3(kPackThreads), 0, s, p, ws.part);
    LSM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(scan_partials_kernel<Sum2>, dim3(1), dim3(kPartThreads), 0, s, ws.part.kv, ntiles,
                       ws.part.kv, ntiles);
    LSM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(scan_partials_kernel<uint64_t>, dim3(1), dim3(kPartThreads), 0, s, ws.part.e, ntiles,
                       ws.part.e, ntiles);
    LSM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pack_scan_apply, dim3(ntiles), dim3(kPackThreads), 0, s, p, ws.part, o);
    LSM_HIP_CHECK(hipGetLastError());
    if (!d_keys && !d_vals) return 0;  // the sizing call
    const uint32_t grid = (uint32_t)((nslot + kPackThreads - 1) / kPackThreads);
    hipLaunchKernelGGL(pack_copy_kernel, dim3(grid), dim3(kPackThreads), 0, s, ws.part, o);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}
