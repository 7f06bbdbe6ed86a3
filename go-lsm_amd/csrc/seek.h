// seek.h — the SSTable read path's shared pieces: Go string comparison over
// 16-byte big-endian key prefixes, the level's sparse-index search, and the two
// halves of searchFromTable past MayContain -- Iterator.Seek's bisection
// (through the Seek tree or over the index) and GetValueByOffset.  lookup.hip
// (the Gets and Search) and treescan.hip (the range scans) run this one copy.
#pragma once

#include "common.h"
#include "murmur.h"

namespace lsm {

struct McFile {
    uint32_t lo[4], hi[4];  // first 16 bytes of min / max key, big-endian, zero padded
    uint32_t lo_len, hi_len;
    uint32_t ok;            // header and filter decoded (lsm_sst_meta.stage not 1 or 2)
    uint32_t k;             // filter k, capped so a probe always ends
    uint64_t lo_at, hi_at;  // image offsets of the min / max key bytes
    uint64_t words_at;      // image offset of the first filter word
    uint64_t m, mr, nbits;  // filter m, its Barrett reciprocal, stored bit count
};

// Big-endian prefix word j of key bytes [p, p + len), zero padded, by byte
// loads that read nothing past len: the probe keys of the two per-probe
// kernels and may_contain_kernel's tile (everything else takes key_prefix's
// 16-byte read).
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

// A key's first 16 bytes as loaded (f0, f1): the bytes past len zeroed in
// place, then the four big-endian prefix words.
__device__ __forceinline__ void prefix_words(uint64_t &f0, uint64_t &f1, uint64_t len, uint32_t kw[4]) {
    if (len < 8) { f0 &= len ? (~0ull >> (64 - 8 * len)) : 0; f1 = 0; }
    else if (len < 16) f1 &= len > 8 ? (~0ull >> (128 - 8 * len)) : 0;
    kw[0] = __builtin_bswap32((uint32_t)f0);
    kw[1] = __builtin_bswap32((uint32_t)(f0 >> 32));
    kw[2] = __builtin_bswap32((uint32_t)f1);
    kw[3] = __builtin_bswap32((uint32_t)(f1 >> 32));
}

// key bytes [p, p + len) as four big-endian words, zero padded past len
// (reads 16 bytes at p: the input slack covers a key that ends a buffer)
__device__ __forceinline__ void key_prefix(const uint8_t *p, uint64_t len, uint32_t kw[4]) {
    uint64_t f0 = ldg_u64_unaligned(p), f1 = ldg_u64_unaligned(p + 8);
    prefix_words(f0, f1, len, kw);
}

// sort.Search(n, MinKey_h > key) exactly as Go's sort.go runs it: the first
// of the nfile tables whose MinKey > key.  lo_prefix(h, bw) gives table h's
// MinKey prefix (from LDS or from files); the full keys only on a prefix tie.
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

// Table t as a Get addresses it: its image, its slots of the decoded index
// and the entries the decode kept.
struct SeekTable {
    uint64_t fo, fl, base;
    uint32_t n;
};

// Iterator.Seek (index.go:157-181) on table t: Go's bisection, through the
// Seek tree or over the index.  -> left, the first entry whose key >= the
// target (T.n when there is none); T = the table.  Exact: a Get's exact-match
// test, hit = Indexes[left].Key == target (Valid's second half for a Get) --
// the Seek tree's last step that set right knows it, the walk over the index
// compares entry left; a scan asks for the lower bound alone.
template <bool Exact>
__device__ __forceinline__ uint32_t seek_in_table(const GetArgs &a, uint32_t t, const uint32_t kw[4],
                                                  uint64_t kl, const uint8_t *kp, SeekTable &T, bool &hit) {
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
    T.fo = a.file_off[t];
    T.fl = a.file_len[t];
    T.base = a.rec_base ? a.rec_base[t] : T.fo / 4;
    T.n = M.nidx;
    const uint64_t base = T.base;
    const uint32_t n = T.n;
    uint32_t left = 0, right = n;
    hit = false;
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
        if (Exact && left < n) {
            const lsm_rec_desc d = a.idx_desc[base + left];
            const uint8_t *ep = a.img + d.rec_off + 4;
            hit = d.key_len == kl && go_cmp(ep, d.key_len, kp, kl) == 0;
        }
    }
    return left;
}

// GetValueByOffset (sstable.go:271-296) at offset `off` of table T's file.
// -> a lsm_get_result; the value's view in v on LSM_GET_FOUND.
__device__ __forceinline__ int32_t value_at_offset(const GetArgs &a, const SeekTable &T, int64_t off,
                                                   lsm_rec_desc &v) {
    int32_t res;
    if (off < 0) {
        res = LSM_GET_SEEK_FAILED;  // file.Seek to a negative offset
    } else {
        // Value.DecodeFrom from the file at off: u32 length, cap, bytes
        const uint64_t rem = (uint64_t)off < T.fl ? T.fl - (uint64_t)off : 0;
        if (rem < 4) {
            res = LSM_GET_VALUE_LENGTH;
        } else {
            const uint8_t *vp = a.img + T.fo + (uint64_t)off;
            const uint32_t vl = (uint32_t)vp[0] | (uint32_t)vp[1] << 8 | (uint32_t)vp[2] << 16 |
                                (uint32_t)vp[3] << 24;
            if (vl > (1u << 30)) res = LSM_GET_VALUE_TOO_LONG;
            else if (rem - 4 < vl) res = LSM_GET_VALUE_SHORT;
            else {
                res = LSM_GET_FOUND;
                v = lsm_rec_desc{T.fo + (uint64_t)off, 0, vl};
            }
        }
    }
    return res;
}

// Iterator.Value -> GetValueByOffset of entry `slot` of table T.
__device__ __forceinline__ int32_t value_by_offset(const GetArgs &a, const SeekTable &T, uint32_t slot,
                                                   lsm_rec_desc &v) {
    return value_at_offset(a, T, a.idx_value[T.base + slot], v);
}

// ---- host side: the arguments of a Get ---------------------------------------

// The tables of a Get and, for the entries that take probes, the probe keys
// and the per-probe outputs.
static inline GetArgs get_args(const uint8_t *d_img, const uint64_t *d_file_off, const uint64_t *d_file_len,
                               const lsm_sst_meta *d_meta, uint32_t nfile, const uint64_t *d_rec_base,
                               const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
                               const uint8_t *d_keys = nullptr, const uint64_t *d_koff = nullptr,
                               uint64_t nkeys = 0, int32_t *d_result = nullptr,
                               lsm_rec_desc *d_value = nullptr) {
    GetArgs a{};
    a.keys = d_keys;
    a.koff = d_koff;
    a.nkeys = nkeys;
    a.result = d_result;
    a.value = d_value;
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

// The Seek tree of a Get: it must span nfile tables of tree_nidx entries
// (a tree built for fewer tables would be read past its end).
static inline int get_tree_args(GetArgs &a, uint32_t nfile, const void *d_tree, uint32_t tree_nidx,
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

// The tree's shape: level L is tables [start[L], start[L + 1]).
constexpr uint32_t kSrLevels = LSM_SEARCH_LEVELS;

struct SrShape {
    uint32_t start[kSrLevels + 1];
};

// The tree's shape from level_start; false when it does not start at 0 or decreases.
static inline bool search_shape(const uint32_t *level_start, SrShape &S) {
    for (uint32_t L = 0; L <= kSrLevels; L++) {
        S.start[L] = level_start[L];
        if (L && S.start[L] < S.start[L - 1]) return false;
    }
    return S.start[0] == 0;
}

}  // namespace lsm
