// mtsort.h — the segmented (key, position) sort shared by memtable.hip (a
// log's records) and write.hip (a log's ops): the LDS tile sort and the
// rank-merge pass, over any key source S with
//   uint32_t span(uint32_t w, uint32_t *base) const   segment w = positions [*base, *base + n)
//   Key16 key16(uint32_t pos) const                   the key's first 16 bytes
//   int cmp_tail(uint32_t a, uint32_t b) const        keys whose first 16 bytes are equal
#pragma once

#include "common.h"

namespace lsm {
namespace {

constexpr uint32_t kTile = 1024;     // records per LDS tile (LSM_MEMTABLE_TILE)
constexpr uint32_t kThreads = 256;   // every other kernel's workgroup
// the tile sort's workgroup: one compare-exchange per thread and stage (its 55
// barrier-separated stages are latency, not throughput)
constexpr uint32_t kSortThreads = kTile / 2;
constexpr uint32_t kPad = 0xFFFFFFFFu;  // position of a tile's padding element

__device__ __forceinline__ uint64_t load8(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// A key's first 16 bytes as two big-endian integers, zero padded: compared as
// (hi, lo) they order keys that differ there; equal, with either key at most
// 16 bytes long, the shorter key is a prefix of the other and sorts first.
struct alignas(16) Key16 {
    uint64_t hi, lo;
};

// 8 key bytes from `at` as a big-endian integer, zero padded past the key.
// Reads 8 bytes whatever the key's length (the input slack covers them).
__device__ __forceinline__ uint64_t key_word(const uint8_t *key, uint32_t klen, uint32_t at) {
    if (klen <= at) return 0;
    uint64_t v = __builtin_bswap64(load8(key + at));
    const uint32_t left = klen - at;
    if (left < 8) v &= ~0ull << (8 * (8 - left));
    return v;
}

// Keys (pa, la) and (pb, lb) whose first 16 bytes are equal: <0, 0, >0 in Go
// string order, either key anywhere (a node against a probe key).
__device__ int key_cmp_tail_at(const uint8_t *pa, uint32_t la, const uint8_t *pb, uint32_t lb) {
    const uint32_t lm = la < lb ? la : lb;
    for (uint32_t j = 16; j < lm; j += 8) {
        const uint64_t x = key_word(pa, lm, j), y = key_word(pb, lm, j);
        if (x != y) return x < y ? -1 : 1;
    }
    return la == lb ? 0 : (la < lb ? -1 : 1);
}

// (key, position) order; a padding element sorts last.
template <class S>
__device__ __forceinline__ bool item_less(const S &L, Key16 ka, uint32_t a, Key16 kb, uint32_t b) {
    if (a == kPad) return false;
    if (b == kPad) return true;
    if (ka.hi != kb.hi) return ka.hi < kb.hi;
    if (ka.lo != kb.lo) return ka.lo < kb.lo;
    const int c = L.cmp_tail(a, b);
    return c ? c < 0 : a < b;
}

// ---- tile sort: one workgroup per tile of one segment -------------------------

template <class S>
__global__ __launch_bounds__(kSortThreads) void mt_tile_sort(S L, Key16 *key_out, uint32_t *pos_out) {
    __shared__ uint64_t s_hi[kTile], s_lo[kTile];
    __shared__ uint32_t s_pos[kTile];
    const uint32_t w = blockIdx.y;
    uint32_t base;
    const uint32_t n = L.span(w, &base);
    const uint32_t t0 = blockIdx.x * kTile;
    if (t0 >= n) return;
    const uint32_t cnt = n - t0 < kTile ? n - t0 : kTile;
    for (uint32_t i = threadIdx.x; i < kTile; i += kSortThreads) {
        if (i < cnt) {
            const uint32_t slot = base + t0 + i;
            const Key16 k = L.key16(slot);
            s_hi[i] = k.hi;
            s_lo[i] = k.lo;
            s_pos[i] = slot;
        } else {
            s_hi[i] = s_lo[i] = ~0ull;
            s_pos[i] = kPad;
        }
    }
    __syncthreads();
    // the smallest power of two that holds the tile's records
    uint32_t m = 2;
    while (m < cnt) m <<= 1;
    for (uint32_t k = 2; k <= m; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < m / 2; t += kSortThreads) {
                const uint32_t lo = 2 * t - (t & (j - 1)), hi = lo + j;
                const bool up = (lo & k) == 0;
                const Key16 ka{s_hi[lo], s_lo[lo]}, kb{s_hi[hi], s_lo[hi]};
                const uint32_t a = s_pos[lo], b = s_pos[hi];
                if (item_less(L, kb, b, ka, a) == up) {
                    s_hi[lo] = kb.hi;
                    s_lo[lo] = kb.lo;
                    s_pos[lo] = b;
                    s_hi[hi] = ka.hi;
                    s_lo[hi] = ka.lo;
                    s_pos[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < cnt; i += kSortThreads) {  // the keys travel with the indices
        key_out[base + t0 + i] = Key16{s_hi[i], s_lo[i]};
        pos_out[base + t0 + i] = s_pos[i];
    }
}

// ---- merge pass: runs of `run` elements joined in pairs --------------------

// Each element finds its place by counting the partner run's smaller
// elements (a bisection; the order is total, so the places are distinct).  A
// run without a partner is copied.
template <class S>
__global__ __launch_bounds__(kThreads) void mt_merge_pass(S L, uint32_t run, const Key16 *key_in,
                                                         const uint32_t *pos_in, Key16 *key_out,
                                                         uint32_t *pos_out) {
    const uint32_t w = blockIdx.y;
    uint32_t base;
    const uint32_t n = L.span(w, &base);
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const Key16 ka = key_in[base + i];
    const uint32_t a = pos_in[base + i];
    const uint32_t r = i / run;
    const uint64_t other = (uint64_t)(r ^ 1) * run;  // the partner run's start
    uint32_t cnt = 0;
    if (other < n) {
        const uint32_t o0 = (uint32_t)other;
        const uint32_t olen = n - o0 < run ? n - o0 : run;
        uint32_t lo = 0, hi = olen;
        while (lo < hi) {  // one 16-byte gather per step; the position only when the 16 bytes tie
            const uint32_t mid = (lo + hi) >> 1;
            const Key16 kb = key_in[base + o0 + mid];
            bool less;
            if (kb.hi != ka.hi) less = kb.hi < ka.hi;
            else if (kb.lo != ka.lo) less = kb.lo < ka.lo;
            else less = item_less(L, kb, pos_in[base + o0 + mid], ka, a);
            if (less) lo = mid + 1;
            else hi = mid;
        }
        cnt = lo;
    }
    const uint32_t pair0 = (r & ~1u) * run;  // < n
    const uint32_t dst = base + pair0 + (i - r * run) + cnt;
    key_out[dst] = ka;
    pos_out[dst] = a;
}

// Sorts every segment of L by (key, position): tiles, then merge passes over
// the ping-pong buffers.  maxn bounds a segment's length; the grid covers
// nseg segments.  Returns the buffer index that holds the result.
template <class S>
int mt_sort_segments(const S &L, uint32_t nseg, uint32_t maxn, Key16 *const key[2], uint32_t *const pos[2],
                     hipStream_t s) {
    const uint32_t ntile = (maxn + kTile - 1) / kTile, nblk = (maxn + kThreads - 1) / kThreads;
    int cur = 0;
    if (ntile) {
        hipLaunchKernelGGL(mt_tile_sort<S>, dim3(ntile, nseg), dim3(kSortThreads), 0, s, L, key[0], pos[0]);
        for (uint64_t run = kTile; run < maxn; run *= 2) {
            hipLaunchKernelGGL(mt_merge_pass<S>, dim3(nblk, nseg), dim3(kThreads), 0, s, L, (uint32_t)run,
                               key[cur], pos[cur], key[cur ^ 1], pos[cur ^ 1]);
            cur ^= 1;
        }
    }
    return cur;
}

}  // namespace
}  // namespace lsm
