// lookup.hip — the SSTable read path (gfx950): the bloom probe, batched
// SSTable.MayContain, the level search, the Seek tree and the Gets,
// Manager.Search and the SSTable half of database.Get.
//
// Every entry works on .sst images as they lie in device memory (the images,
// their lsm_sst_meta and decoded index blocks: decode.hip's outputs) and on a
// CSR batch of probe keys.  Shared by the sections below: McFile (a table's
// search view), the bound comparisons on 16-byte big-endian key prefixes,
// lv_search (Go's sort.Search over the tables) and the filter tests.  The
// 16-byte hash record the grouped filter test reads is the .sst builder's
// (hashrec.h).
#include "common.h"
#include "hashrec.h"
#include "murmur.h"
#include "seek.h"

namespace lsm {
namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// ---- bloom probe -----------------------------------------------------------

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

// The search view of table f.  ByBytes: the bound prefixes by be_word_at
// under a select, may_contain_kernel's form (with key_prefix's loads, or with
// the byte loads under the branch, that kernel takes 85-87 VGPRs against 80
// and loses an occupancy step).
template <bool ByBytes = false>
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
    if (ByBytes) {
        for (uint32_t j = 0; j < 4; j++) {
            F.lo[j] = F.ok ? be_word_at(base + M.min_key_off, M.min_key_len, j) : 0;
            F.hi[j] = F.ok ? be_word_at(base + M.max_key_off, M.max_key_len, j) : 0;
        }
    } else if (F.ok) {
        key_prefix(base + M.min_key_off, M.min_key_len, F.lo);
        key_prefix(base + M.max_key_off, M.max_key_len, F.hi);
    }
    F.lo_at = fo + M.min_key_off;
    F.hi_at = fo + M.max_key_off;
    F.words_at = fo + M.filter_words_off;
    // k from the file (no max(1, k) on a decoded filter); Test's early exit
    // ends a probe at its first clear bit, a corrupted k beyond kMcMaxK is
    // capped (deviations)
    F.k = M.filter_k < kMcMaxK ? (uint32_t)M.filter_k : kMcMaxK;
    F.m = M.filter_m;
    F.mr = M.filter_m ? ~0ull / M.filter_m : 0;
    F.nbits = M.filter_nbits;
    return F;
}

// lv_search's accessor for MinKey prefixes staged in LDS
struct LdsPrefixes {
    const uint4 *s;
    __device__ __forceinline__ void operator()(uint32_t h, uint32_t bw[4]) const {
        const uint4 v = s[h];
        bw[0] = v.x; bw[1] = v.y; bw[2] = v.z; bw[3] = v.w;
    }
};

// Filter.Test (bloom.go:371-379) of an image's stored filter, every m (the
// per-probe path's form: sixteen bit reads in flight at a time).  Test's
// answer is the AND of all k bits (its early exit changes nothing).
__device__ __forceinline__ uint32_t filter_test_any(const McFile &F, const uint64_t h[4], const uint8_t *img) {
    const uint64_t m = F.m;
    // hashNum 0: true (bloom.go:373 loop never runs); m == 0 < k: Go's
    // location() divides by zero and panics, answered false
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
            for (uint32_t t = threadIdx.x; t < nt; t += kMcThreads)
                tile[t] = mc_file<true>(img, file_off, meta[f0 + t], f0 + t);
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
                auto lo_tile = [&](uint32_t x, uint32_t bw[4]) {
                    for (int j = 0; j < 4; j++) bw[j] = tile[x].lo[j];
                };
                const uint32_t lo = lv_search(nt, lo_tile, tile, img, kw, kl, kp);  // first t with MinKey > key
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
                        bound_cmp_fast(F.hi, F.hi_len, img + F.hi_at, kw, kl, kp) >= 0)
                        r = filter_test_any(F, h, img);
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
// order with disjoint ranges, at most kLvMaxFiles files): each probe has at
// most one candidate file.  mc_classify_kernel hashes the candidates once and
// groups each workgroup's by file into its slots (the level search's layout,
// LvWs), and lv_test_kernel<true> (one workgroup per file) stages the filter
// in LDS and tests its probes' bits there: the filter bits are read once from
// HBM instead of once per probe bit.
constexpr uint32_t kMcLdsBytes = 144 * 1024;  // filter words staged in LDS per file
constexpr uint32_t kMcNone = 0xFFFFFFFFu;

// A table whose filter takes the 16-byte hash record of the encode path
// (store_hash_rec: m <= 2^21, k <= 16; go-lsm's 1.6 Mbit, k = 16): classify
// stores the record for the table's m, and the test rebuilds the locations
// from it by additions -- 16 bytes per probe through the workspace instead
// of the 32-byte sum256, and no modulo in the test.
__device__ __forceinline__ bool lv_compact(const McFile &F) {
    return F.m != 0 && F.m <= (1ull << kHashRecBits) && F.k <= kSplitMaxK;
}

// The classify workgroup of the level search and of the grouped path above
constexpr uint32_t kLvThreads = 1024;
constexpr uint32_t kLvPer = 2;  // probes per thread
constexpr uint32_t kLvProbes = kLvThreads * kLvPer;
constexpr uint32_t kLvMaxFiles = 2048;  // LDS bounds + counters; more files: the per-probe kernels
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

struct McWs {
    uint32_t *flag;     // [0] = 1: grouped path
    McFile *files;
    LvWs lv;            // the probes grouped by candidate file, as the level search's
};

LvWs lv_ws_layout(WsCursor &c, uint32_t nfile, uint64_t nkeys) {
    LvWs w{};
    const uint64_t pass = nkeys < (uint64_t)kLvMaxWgs * kLvProbes ? nkeys : (uint64_t)kLvMaxWgs * kLvProbes;
    const uint64_t nwg = (pass + kLvProbes - 1) / kLvProbes;
    const size_t nf = nfile ? nfile : 1, ng = nwg ? nwg : 1;
    w.files = c.take<McFile>(nf);
    w.grid = c.take<uint32_t>(nf * ng);
    w.cnt = c.take<uint32_t>(nf * ng);
    w.ids = c.take<uint32_t>(ng * kLvProbes);
    w.rec = c.take<u32x4>(ng * kLvProbes);
    w.ext = c.take<u32x4>(ng * kLvProbes);
    return w;
}

McWs mc_ws_layout(WsCursor &c, uint32_t nfile, uint64_t nkeys) {
    McWs w{};
    w.flag = c.take<uint32_t>(4);
    w.files = c.take<McFile>(nfile ? nfile : 1);
    w.lv = lv_ws_layout(c, nfile, nkeys);
    w.lv.files = w.files;
    return w;
}

// Probe p of this thread in a classify pass that starts at probe k_begin.
__device__ __forceinline__ uint64_t lv_probe(uint64_t k_begin, uint32_t p) {
    return k_begin + (uint64_t)blockIdx.x * kLvProbes + p * kLvThreads + threadIdx.x;
}

// A classify thread's probes: offset and length (0, 0 past nkeys), the first
// 16 key bytes zeroed past the key (sum256_pre takes them) and as prefix words.
struct LvKeys {
    uint64_t k0[kLvPer], kl[kLvPer], f0[kLvPer], f1[kLvPer];
    uint32_t kw[kLvPer][4];
};

// Every probe's first 16 key bytes (dword loads; batches are 16-byte padded):
// all offset loads, then all key loads in flight, then the arithmetic.
__device__ __forceinline__ void lv_load_keys(const uint8_t *keys, const uint64_t *koff, uint64_t k_begin,
                                             uint64_t nkeys, LvKeys &K) {
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        const uint64_t i = lv_probe(k_begin, p);
        K.k0[p] = i < nkeys ? koff[i] : 0;
        K.kl[p] = i < nkeys ? koff[i + 1] - K.k0[p] : 0;
    }
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        const uint64_t i = lv_probe(k_begin, p);
        K.f0[p] = i < nkeys ? ldg_u64_unaligned(keys + K.k0[p]) : 0;
        K.f1[p] = i < nkeys ? ldg_u64_unaligned(keys + K.k0[p] + 8) : 0;
    }
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) prefix_words(K.f0[p], K.f1[p], K.kl[p], K.kw[p]);
}

// Exclusive prefix sum of v over the kLvThreads-thread block through the LDS
// row `part`, which is left holding the inclusive sums (part[kLvThreads - 1]:
// the total).  Not scan.h's wave-sum scan: the classify kernels read the row back.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t *part, uint32_t v) {
    const uint32_t t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kLvThreads; d <<= 1) {
        const uint32_t x = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    return part[t] - v;
}

// The tail of both classify kernels.  Each candidate probe p (cand[p] its
// table, kMcNone for none; rank[p] its arrival among the workgroup's probes
// of that table, counted in lh; hh[p] its sum256) goes to the workgroup's
// slots grouped by table: exclusive scan of the per-table counts (<= 2,048
// tables, 2 per thread), the workgroup's (start, count) per table to the
// table-major grid, then the ids and the hash records.
__device__ __forceinline__ void lv_scatter(const LvWs &w, uint32_t nfile, uint32_t nwg, uint64_t k_begin,
                                           uint32_t *lh, uint32_t *part, const uint32_t (&cand)[kLvPer],
                                           const uint32_t (&rank)[kLvPer], uint64_t (&hh)[kLvPer][4]) {
    const uint32_t t = threadIdx.x;
    __syncthreads();  // the counts are complete, part is free
    const uint32_t c0 = 2 * t < nfile ? lh[2 * t] : 0u, c1 = 2 * t + 1 < nfile ? lh[2 * t + 1] : 0u;
    const uint32_t ex = block_excl_scan(part, c0 + c1);
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
        const uint64_t slot = (uint64_t)blockIdx.x * kLvProbes + lh[cand[p]] + rank[p];
        w.ids[slot] = (uint32_t)(lv_probe(k_begin, p) - k_begin);
        const McFile &F = w.files[cand[p]];
        if (lv_compact(F)) {  // 16 bytes, and no modulo in the test
            store_hash_rec(hh[p], (uint32_t)F.m, (uint32_t)F.mr, (uint32_t)(F.mr >> 32),
                           reinterpret_cast<uint32_t *>(w.rec + slot));
        } else {
            *(gptr_t<u64x2>)gbl(w.rec + slot) = u64x2{hh[p][0], hh[p][1]};
            *(gptr_t<u64x2>)gbl(w.ext + slot) = u64x2{hh[p][2], hh[p][3]};
        }
    }
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
    if (nfile > kLvMaxFiles) ok = false;
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
__global__ __launch_bounds__(kLvThreads) void mc_classify_kernel(const uint8_t *img, uint32_t nfile,
                                                                 const uint8_t *keys, const uint64_t *koff,
                                                                 uint64_t k_begin, uint64_t nkeys, McWs w,
                                                                 uint32_t nwg, uint8_t *hit) {
    __shared__ uint4 slo[kLvMaxFiles], shi[kLvMaxFiles];
    __shared__ uint32_t lh[kLvMaxFiles];
    __shared__ uint32_t part[kLvThreads];
    if (!w.flag[0]) return;
    const uint32_t t = threadIdx.x;
    for (uint32_t f = threadIdx.x; f < nfile; f += kLvThreads) {
        const McFile &F = w.files[f];
        slo[f] = make_uint4(F.lo[0], F.lo[1], F.lo[2], F.lo[3]);
        shi[f] = make_uint4(F.hi[0], F.hi[1], F.hi[2], F.hi[3]);
        lh[f] = 0;
    }
    LvKeys K;  // all loads in flight before the search
    lv_load_keys(keys, koff, k_begin, nkeys, K);
    __syncthreads();
    uint32_t cand[kLvPer], rank[kLvPer];
    uint64_t hh[kLvPer][4];
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) cand[p] = kMcNone;
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        if (lv_probe(k_begin, p) >= nkeys) break;
        const uint8_t *kp = keys + K.k0[p];
        // first file with MinKey > key
        const uint32_t lo = lv_search(nfile, LdsPrefixes{slo}, w.files, img, K.kw[p], K.kl[p], kp);
        if (lo > 0) {
            const uint4 v = shi[lo - 1];
            const uint32_t bw[4] = {v.x, v.y, v.z, v.w};
            int r = prefix_cmp(bw, K.kw[p]);
            if (r == 0) {
                const McFile &F = w.files[lo - 1];
                r = bound_cmp(bw, F.hi_len, img + F.hi_at, K.kw[p], K.kl[p], kp);
            }
            if (r >= 0) {  // only candidates are ever tested
                cand[p] = lo - 1;
                rank[p] = atomicAdd(&lh[lo - 1], 1u);
                sum256_pre(kp, K.kl[p], K.f0[p], K.f1[p], hh[p]);
            }
        }
    }
    {   // the workgroup's rows of the hit matrix, written once: 0 except the
        // candidate's 1 (the test clears it when a bit is 0), 16-byte stores;
        // the candidates through LDS (the scan's row, free until the scan)
        uint16_t *scand = reinterpret_cast<uint16_t *>(part);
#pragma unroll
        for (uint32_t p = 0; p < kLvPer; p++)
            scand[p * kLvThreads + t] = cand[p] == kMcNone ? (uint16_t)0xFFFFu : (uint16_t)cand[p];
        __syncthreads();
        const uint64_t r0 = k_begin + (uint64_t)blockIdx.x * kLvProbes;
        const uint64_t r1 = r0 + kLvProbes < nkeys ? r0 + kLvProbes : nkeys;
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
        for (uint32_t x = t; x < n16; x += kLvThreads) {
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
    lv_scatter(w.lv, nfile, nwg, k_begin, lh, part, cand, rank, hh);
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
    LvKeys K;
    lv_load_keys(keys, koff, k_begin, nkeys, K);
    __syncthreads();
    uint32_t cand[kLvPer], rank[kLvPer];
    uint64_t hh[kLvPer][4];
#pragma unroll
    for (uint32_t p = 0; p < kLvPer; p++) {
        const uint64_t i = lv_probe(k_begin, p);
        cand[p] = kMcNone;
        if (i >= nkeys) continue;
        const uint8_t *kp = keys + K.k0[p];
        const uint32_t lo = lv_search(nfile, LdsPrefixes{slo}, w.files, img, K.kw[p], K.kl[p], kp);
        const uint32_t idx = lo ? lo - 1 : 0;  // manager.go:189-191
        table[i] = (int32_t)idx;
        // MayContain (sstable.go:301): lo > 0 means f(lo - 1) was evaluated
        // false, i.e. MinKey <= key; then MaxKey >= key and a decoded filter
        bool test = false;
        if (lo > 0) {
            const McFile &F = w.files[idx];
            if (F.ok) {
                int r = prefix_cmp(F.hi, K.kw[p]);
                if (r == 0) r = bound_cmp(F.hi, F.hi_len, img + F.hi_at, K.kw[p], K.kl[p], kp);
                test = r >= 0;
            }
        }
        may[i] = test ? 1 : 0;  // the test clears a candidate whose bit is 0
        if (!test) continue;
        cand[p] = idx;
        rank[p] = atomicAdd(&lh[idx], 1u);
        sum256_pre(kp, K.kl[p], K.f0[p], K.f1[p], hh[p]);
    }
    lv_scatter(w, nfile, nwg, k_begin, lh, part, cand, rank, hh);
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
    const uint32_t ex = block_excl_scan(part, c);
    if (t < nwg) sb[t] = ex;
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

// ---- batched Get past MayContain (seek.h: Iterator.Seek + GetValueByOffset,
// the Seek tree's layout) ------------------------------------------------------
//
// The Seek tree's build: one thread per (table, block, node slot 0-7; slot 7 idle).
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

// searchFromTable past MayContain (manager.go:209-223) on table t: Go's
// bisection (through the Seek tree, or over the index), the exact-match
// test, then GetValueByOffset (sstable.go:271-296).  -> a lsm_get_result;
// the value's view in v on LSM_GET_FOUND.  The two halves are seek.h's, shared
// with the range scans (treescan.hip).
__device__ __forceinline__ int32_t get_in_table(const GetArgs &a, uint32_t t, const uint32_t kw[4],
                                                uint64_t kl, const uint8_t *kp, lsm_rec_desc &v) {
    SeekTable T;
    bool hit;
    const uint32_t left = seek_in_table<true>(a, t, kw, kl, kp, T, hit);
    int32_t res = LSM_GET_ABSENT;
    if (hit) res = value_by_offset(a, T, left, v);
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
constexpr uint32_t kSrMaxGrid = 8192;  // workgroups (grid-stride past them)

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

}  // namespace
}  // namespace lsm

using namespace lsm;

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

// The classify + test passes of up to 2M probes (the test kernel's segment
// table): launch(k0, k1, nwg) runs probes [k0, k1) in nwg classify workgroups.
template <class Launch>
static void lv_passes(uint64_t nkeys, Launch launch) {
    const uint64_t pass = (uint64_t)kLvMaxWgs * kLvProbes;
    for (uint64_t k0 = 0; k0 < nkeys; k0 += pass) {
        const uint64_t n = nkeys - k0 < pass ? nkeys - k0 : pass;
        launch(k0, k0 + n, (uint32_t)((n + kLvProbes - 1) / kLvProbes));
    }
}

extern "C" size_t lsm_may_contain_workspace_bytes(uint32_t nfile, uint64_t nkeys) {
    WsCursor c{nullptr, 0};
    mc_ws_layout(c, nfile, nkeys);
    return c.at;
}

extern "C" int lsm_may_contain(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                               const lsm_sst_meta *d_meta, uint32_t nfile, const uint8_t *d_keys,
                               const uint64_t *d_koff, uint64_t nkeys, uint8_t *d_hit,
                               void *d_workspace, size_t ws_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0 || nfile == 0) return 0;
    if (!d_img || !d_file_off || !d_meta || !d_keys || !d_koff || !d_hit || !d_workspace)
        return LSM_EINVAL;
    WsCursor c{static_cast<uint8_t *>(d_workspace), 0};
    const McWs w = mc_ws_layout(c, nfile, nkeys);
    if (ws_bytes < c.at) return LSM_ESPACE;
    const uint64_t grid = (nkeys + kMcThreads - 1) / kMcThreads;
    if (grid > 0x7FFFFFFFull) return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nkeys > 0xFFFFFFFFull) {  // list entries are 32-bit: the per-probe path
        LSM_HIP_CHECK(hipMemsetAsync(w.flag, 0, 4, s));
    } else {
        hipLaunchKernelGGL(mc_prep_kernel, dim3(1), dim3(256), 0, s, d_img, d_file_off, d_meta, nfile, w);
        lv_passes(nkeys, [&](uint64_t k0, uint64_t k1, uint32_t nwg) {
            hipLaunchKernelGGL(mc_classify_kernel, dim3(nwg), dim3(kLvThreads), 0, s, d_img, nfile,
                               d_keys, d_koff, k0, k1, w, nwg, d_hit);
            hipLaunchKernelGGL(lv_test_kernel<true>, dim3(nfile), dim3(kLvThreads), kMcLdsBytes, s,
                               d_img, nfile, nwg, w.lv, k0, d_hit, (const uint32_t *)w.flag);
        });
    }
    const uint32_t pgrid = grid < kMcProbeGrid ? (uint32_t)grid : kMcProbeGrid;
    hipLaunchKernelGGL(may_contain_kernel, dim3(pgrid), dim3(kMcThreads), 0, s, d_img,
                       d_file_off, d_meta, nfile, d_keys, d_koff, nkeys, d_hit,
                       (const uint32_t *)w.flag);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" size_t lsm_level_may_contain_workspace_bytes(uint32_t nfile, uint64_t nkeys) {
    WsCursor c{nullptr, 0};
    lv_ws_layout(c, nfile, nkeys);
    return c.at;
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
        lv_passes(nkeys, [&](uint64_t k0, uint64_t k1, uint32_t nwg) {
            hipLaunchKernelGGL(lv_classify_kernel, dim3(nwg), dim3(kLvThreads), 0, s, d_img, nfile,
                               d_keys, d_koff, k0, k1, w, nwg, d_table, d_may);
            hipLaunchKernelGGL(lv_test_kernel<false>, dim3(nfile), dim3(kLvThreads), kMcLdsBytes, s,
                               d_img, nfile, nwg, w, k0, d_may, nullptr);
        });
    }
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

// Both level searches: over d_index (lsm_level_may_contain_indexed), or, with
// d_index null, over the table array built from d_file_off / d_meta into the
// workspace first (lsm_level_may_contain).
static int level_may_contain(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index,
                             const uint64_t *d_file_off, const lsm_sst_meta *d_meta, uint32_t nfile,
                             const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                             int32_t *d_table, uint8_t *d_may, void *d_workspace, size_t ws_bytes,
                             void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (!d_keys || !d_koff || !d_table || !d_may) return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nfile == 0) {  // an empty level: no candidate (manager.go:194), nothing may be there
        LSM_HIP_CHECK(hipMemsetAsync(d_table, 0xFF, 4 * nkeys, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_may, 0, nkeys, s));
        return 0;
    }
    if (!d_img || !(d_index || (d_file_off && d_meta)) || !d_workspace) return LSM_EINVAL;
    WsCursor c{static_cast<uint8_t *>(d_workspace), 0};
    const LvWs w = lv_ws_layout(c, nfile, nkeys);
    if (ws_bytes < c.at) return LSM_ESPACE;
    const McFile *files = static_cast<const McFile *>(d_index);
    if (!files) {
        hipLaunchKernelGGL(lv_prep_kernel, dim3((nfile + 255) / 256), dim3(256), 0, s, d_img, d_file_off,
                           d_meta, nfile, w);
        files = w.files;
    }
    return level_search(s, d_img, files, nfile, d_keys, d_koff, nkeys, d_table, d_may, w);
}

extern "C" int lsm_level_may_contain(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                                     const lsm_sst_meta *d_meta, uint32_t nfile,
                                     const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                                     int32_t *d_table, uint8_t *d_may, void *d_workspace,
                                     size_t ws_bytes, void *stream) {
    return level_may_contain(ctx, d_img, nullptr, d_file_off, d_meta, nfile, d_keys, d_koff, nkeys, d_table,
                             d_may, d_workspace, ws_bytes, stream);
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
    return level_may_contain(ctx, d_img, d_index, nullptr, nullptr, nfile, d_keys, d_koff, nkeys, d_table,
                             d_may, d_workspace, ws_bytes, stream);
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
                         d_idx_value, d_keys, d_koff, nkeys, d_result, d_value);
    a.table = d_table;
    a.may = d_may;
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
                         d_idx_value, d_keys, d_koff, nkeys, d_result, d_value);
    const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
    if (rc) return rc;
    const uint64_t grid = (nkeys + kL0Threads - 1) / kL0Threads;
    if (grid > 0x7FFFFFFFull) return LSM_EINVAL;
    hipLaunchKernelGGL(level0_get_kernel, dim3((uint32_t)grid), dim3(kL0Threads), 0,
                       static_cast<hipStream_t>(stream), a, d_table);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
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
                         d_idx_value, d_keys, d_koff, nkeys, d_result, d_value);
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
    GetArgs a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc, d_idx_value,
                         d_keys, d_koff, nkeys, d_result, d_value);
    // an empty tree needs none of the tree's buffers: every level of S is empty
    // and the kernel reads no table
    if (nfile) {
        if (!d_img || !d_index || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value ||
            !d_workspace)
            return LSM_EINVAL;
        if (ws_bytes < kSrWsBytes) return LSM_ESPACE;
        const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
        if (rc) return rc;
    }
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
