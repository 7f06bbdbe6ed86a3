// scan.h — the workgroup exclusive scan and the scan of the tile sums, one
// copy for decode.hip (u64 sums), merge.hip and encode.hip (pairs of sums).
//
// A long scan runs as three launches: per tile of kScanTile values a sum
// (the caller's kernel, fused with its loads), scan_partials_kernel over the
// tile sums, then per tile the scan proper plus its tile's prefix (the
// caller's kernel again, fused with its stores).
#pragma once

#include "common.h"

namespace lsm {
namespace {

// Two sums scanned together (bytes and counts, sizes and spans).
struct Sum2 {
    uint64_t s, c;
};
__device__ __forceinline__ Sum2 operator+(const Sum2 &a, const Sum2 &b) {
    return Sum2{a.s + b.s, a.c + b.c};
}

__device__ __forceinline__ uint64_t wave_excl_sum(uint64_t v, uint64_t *total) {
    return wave_excl_scan64(v, total);
}
__device__ __forceinline__ Sum2 wave_excl_sum(const Sum2 &v, Sum2 *total) {
    Sum2 x;
    x.s = wave_excl_scan64(v.s, &total->s);
    x.c = wave_excl_scan64(v.c, &total->c);
    return x;
}

// N per-wave sums in LDS (of the calling kernel: one set per instantiation).
// A pair's two sums keep an LDS array each: over one array of pairs
// sst_stream_plan_kernel spills 17 VGPRs instead of 13 (b128 reads), and over
// two rows of one array the one-workgroup scans of merge.hip change their
// VGPR count.
template <class T, uint32_t N>
struct WaveSums {
    static __device__ __forceinline__ T *wsum_row() {
        __shared__ T v[N];
        return v;
    }
    static __device__ __forceinline__ T wsum_get(uint32_t i) { return wsum_row()[i]; }
    static __device__ __forceinline__ void wsum_set(uint32_t i, const T &x) { wsum_row()[i] = x; }
};
template <uint32_t N>
struct WaveSums<Sum2, N> {
    static __device__ __forceinline__ Sum2 wsum_get(uint32_t i) {
        return Sum2{WaveSums<uint64_t, N>::wsum_get(i), wsum_c_row()[i]};
    }
    static __device__ __forceinline__ void wsum_set(uint32_t i, const Sum2 &x) {
        WaveSums<uint64_t, N>::wsum_set(i, x.s);
        wsum_c_row()[i] = x.c;
    }
    static __device__ __forceinline__ uint64_t *wsum_c_row() {
        __shared__ uint64_t v[N];
        return v;
    }
};

__device__ __forceinline__ void wg_barrier() { __syncthreads(); }

// Exclusive sums of v over a workgroup of THREADS threads, *total = the sum
// over all of them.  BARRIER: the workgroup barrier of the calling kernel.
template <uint32_t THREADS, void (*BARRIER)() = wg_barrier, class T>
__device__ __forceinline__ T wg_excl_scan(const T &v, T *total) {
    constexpr uint32_t NW = THREADS / kWave;
    using lds = WaveSums<T, NW>;
    T wt;
    const T x = wave_excl_sum(v, &wt);
    const uint32_t w = threadIdx.x / kWave;
    if (lane_id() == 0) lds::wsum_set(w, wt);
    BARRIER();
    T pre{}, tot{};
    for (uint32_t i = 0; i < NW; i++) {
        if (i < w) pre = pre + lds::wsum_get(i);
        tot = tot + lds::wsum_get(i);
    }
    BARRIER();
    *total = tot;
    return x + pre;
}

// Values per thread and per tile of the per-tile kernels (256 threads).
// 16 per thread (lanes 128 B apart) measured 1% slower on the compaction's
// plan scan; on the merge's (lanes 256 B apart, strided stores) A/B compact
// 1.359 -> 1.348 ms.
constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kScanPer = 2;
constexpr uint32_t kScanTile = kScanThreads * kScanPer;

// One pass over the tile sums by 1,024 threads: each a contiguous stretch of
// them (8 loads in flight together), one block scan of the stretch sums (a
// loop of 256-thread block scans over 256-tile chunks took 16 us for 6,400
// tiles: a round trip per chunk).  partial[t] becomes the sum of the tiles
// before t, out[n] the sum of all.
constexpr uint32_t kPartThreads = 1024;

template <class T>
__global__ __launch_bounds__(kPartThreads) void scan_partials_kernel(T *partial, uint32_t ntiles,
                                                                     T *out, uint32_t n) {
    const uint32_t per = (ntiles + kPartThreads - 1) / kPartThreads, b = threadIdx.x * per;
    const uint32_t e = b + per < ntiles ? b + per : ntiles;
    T s{};
    for (uint32_t i0 = b; i0 < e; i0 += 8) {
        T v[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) v[k] = i0 + k < e ? partial[i0 + k] : T{};
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) s = s + v[k];
    }
    T tot;
    T pre = wg_excl_scan<kPartThreads>(s, &tot);
    for (uint32_t i0 = b; i0 < e; i0 += 8) {
        T v[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) v[k] = i0 + k < e ? partial[i0 + k] : T{};
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            if (i0 + k < e) partial[i0 + k] = pre;
            pre = pre + v[k];
        }
    }
    if (threadIdx.x == 0) out[n] = tot;
}

}  // namespace
}  // namespace lsm
