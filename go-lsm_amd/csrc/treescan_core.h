// treescan_core.h — the device code the two batched range scans share:
// treescan.hip (lsm_tree_scan, the SSTable tree alone) and dbscan.hip
// (lsm_db_scan, the memtables in front of it).  A source's head and a range's
// bounds, the wave-wide minimum, a table source's Seek / Next (place,
// seek_source), the order of two heads, the tombstone test and a head's form
// in the workspace.  Header-only, as decode_core.h is.
#pragma once

#include "common.h"
#include "murmur.h"
#include "seek.h"

namespace lsm {
namespace {

constexpr uint32_t kTsThreads = 256;                 // four waves, a range each
constexpr uint32_t kTsWaves = kTsThreads / kWave;
constexpr uint32_t kTsMaxGrid = 2048;                // workgroups (the waves stride over the ranges)
constexpr uint32_t kTsNone = 0xFFFFFFFFu;
constexpr size_t kTsHeadBytes = 32;                  // a head in the workspace: two 16-byte words
constexpr uint32_t kTsSeekMaxGrid = 16384;           // the Seeks' workgroups (grid-stride past them)

struct ScanArgs {
    const uint8_t *lo, *hi;
    const uint64_t *lo_off, *hi_off;
    const uint8_t *flags;
    uint64_t nq;
    uint32_t limit;
    int mode;
    uint32_t nsrc, rounds;
    uint32_t *count;
    uint8_t *more;
    lsm_rec_desc *key, *value;
    int32_t *table, *result;
    u32x4 *ws;
};

// A source's head entry: entry `ent` of table `tab` (kTsNone: the source is
// exhausted, or past the range's end), its key's prefix and length.
struct Head {
    uint32_t kw[4];
    uint32_t klen, tab, ent;
};

// One end of a range.
struct Bound {
    uint32_t w[4];
    uint64_t len;
    const uint8_t *p;
    bool none;  // LSM_SCAN_NO_UPPER
};

// The least value over the wave, in every lane (DPP row shifts and the row
// broadcasts, as wave_incl_scan; the whole wave must be active).  row0: only
// lanes 0-15 hold values that count (at most 16 sources), so the first row's
// four shifts are the whole reduction.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v, bool row0) {
    const uint32_t l = lane_id(), rl = l & 15;
    uint32_t t;
    t = dpp_mov<0x111>(v); v = rl >= 1 && t < v ? t : v;
    t = dpp_mov<0x112>(v); v = rl >= 2 && t < v ? t : v;
    t = dpp_mov<0x114>(v); v = rl >= 4 && t < v ? t : v;
    t = dpp_mov<0x118>(v); v = rl >= 8 && t < v ? t : v;
    if (row0) return (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
    t = dpp_mov<0x142>(v); v = (l & 31) >= 16 && t < v ? t : v;
    t = dpp_mov<0x143>(v); v = l >= 32 && t < v ? t : v;
    return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1);
}

__device__ __forceinline__ uint64_t table_base(const GetArgs &a, uint32_t t) {
    return a.rec_base ? a.rec_base[t] : a.file_off[t] / 4;
}

// The entries of table t that take part: nidx of a table SSTable.DecodeFrom
// loads (sstable.go:101-125 reads header, filter, footer and index; the data
// block is compaction's, so its damage -- stages 5 and 6 -- keeps the table in
// the Manager, and Search answers from it), else 0.
__device__ __forceinline__ uint32_t table_entries(const GetArgs &a, uint32_t t) {
    const lsm_sst_meta &M = a.meta[t];
    return M.stage == LSM_SST_OK || M.stage == LSM_SST_DATA || M.stage == LSM_SST_MISMATCH ? M.nidx : 0;
}

// The next table of [t + 1, end) that takes part, or kTsNone.
__device__ __forceinline__ uint32_t next_table(const GetArgs &a, uint32_t t, uint32_t end) {
    for (uint32_t u = t + 1; u < end; u++)
        if (table_entries(a, u)) return u;
    return kTsNone;
}

__device__ __forceinline__ const uint8_t *entry_key(const GetArgs &a, uint32_t tab, uint32_t ent,
                                                    uint32_t &len) {
    const lsm_rec_desc d = a.idx_desc[table_base(a, tab) + ent];
    len = d.key_len;
    return a.img + d.rec_off + 4;
}

// The source's head at entry `ent` of table `tab`, its tables ending at `end`:
// Valid / Key after a Seek or a Next (iterator.go).  Past a table's last entry
// the walk goes on at entry 0 of the next table that takes part.  The
// boundary-key rule: a table's last key that is also the next table's first is
// answered by the next table -- the one the sparse index picks for it
// (manager.go:186-192) -- so the cursor moves there.  A key at or past the
// range's end exhausts the source.  tab only grows: the walk terminates on any
// index.
__device__ __forceinline__ void place(const GetArgs &a, const Bound &hi, uint32_t tab, uint32_t ent,
                                      uint32_t end, Head &h) {
    h.tab = kTsNone;
    const uint8_t *kp = nullptr;
    while (tab != kTsNone) {
        const uint32_t n = table_entries(a, tab);
        if (ent >= n) {
            tab = next_table(a, tab, end);
            ent = 0;
            continue;
        }
        kp = entry_key(a, tab, ent, h.klen);
        if (ent + 1 == n) {
            const uint32_t u = next_table(a, tab, end);
            if (u != kTsNone) {
                uint32_t fl;
                const uint8_t *fp = entry_key(a, u, 0, fl);
                if (fl == h.klen && go_cmp(fp, fl, kp, h.klen) == 0) {
                    tab = u;
                    ent = 0;
                    continue;
                }
            }
        }
        break;
    }
    if (tab == kTsNone) return;
    key_prefix(kp, h.klen, h.kw);
    if (!hi.none && bound_cmp_fast(h.kw, h.klen, kp, hi.w, hi.len, hi.p) >= 0) return;
    h.tab = tab;
    h.ent = ent;
}

// Where source src's tables end: a level-0 table is its own source, level L's
// tables end at start[L + 1].
__device__ __forceinline__ uint32_t source_end(const SrShape &S, uint32_t src) {
    const uint32_t n0 = S.start[1];
    if (src < n0) return src + 1;
    uint32_t end = 0;
#pragma unroll
    for (uint32_t L = 1; L < kSrLevels; L++)
        if (src - n0 + 1 == L) end = S.start[L + 1];
    return end;
}

// Iterator.Seek(lo) on source src -> its first head.
__device__ __forceinline__ void seek_source(const GetArgs &a, const McFile *files, const SrShape &S,
                                            uint32_t src, const Bound &lo, const Bound &hi, Head &h) {
    const uint32_t n0 = S.start[1];
    uint32_t tab = src, end = src + 1;
    if (src >= n0) {
        // the level's table as searchFromLevelWithSparseIndex picks it
        uint32_t base = 0;
#pragma unroll
        for (uint32_t L = 1; L < kSrLevels; L++)
            if (src - n0 + 1 == L) base = S.start[L];
        end = source_end(S, src);
        h.tab = kTsNone;
        if (end <= base) return;
        auto lo_at = [&](uint32_t x, uint32_t bw[4]) {
            for (int j = 0; j < 4; j++) bw[j] = files[base + x].lo[j];
        };
        const uint32_t i = lv_search(end - base, lo_at, files + base, a.img, lo.w, lo.len, lo.p);
        tab = base + (i ? i - 1 : 0);  // manager.go:189-191
    }
    uint32_t ent = 0;
    if (table_entries(a, tab)) {
        SeekTable T;
        bool hit;
        ent = seek_in_table<false>(a, tab, lo.w, lo.len, lo.p, T, hit);
    }
    place(a, hi, tab, ent, end, h);
}

// Go string order of two heads whose keys are in the image: <0, 0, >0.
__device__ __forceinline__ int head_cmp(const GetArgs &a, const Head &x, const Head &y) {
    int c = prefix_cmp(x.kw, y.kw);
    if (c == 0) {
        if (x.klen <= 16 || y.klen <= 16) {
            c = x.klen < y.klen ? -1 : x.klen > y.klen ? 1 : 0;
        } else {
            uint32_t xl, yl;
            const uint8_t *xp = entry_key(a, x.tab, x.ent, xl), *yp = entry_key(a, y.tab, y.ent, yl);
            c = go_cmp(xp + 16, xl - 16, yp + 16, yl - 16);
        }
    }
    return c;
}

// kv.DeletedValue, "～DELETED～" (kv/kv.go:29-31): exactly those 13 bytes.
__device__ __forceinline__ bool is_tombstone_value(const uint8_t *img, const lsm_rec_desc &v) {
    if (v.val_len != 13) return false;
    const uint8_t tomb[13] = {0xEF, 0xBD, 0x9E, 'D', 'E', 'L', 'E', 'T', 'E', 'D', 0xEF, 0xBD, 0x9E};
    const uint8_t *p = img + v.rec_off + 4;
    bool eq = true;
#pragma unroll
    for (int i = 0; i < 13; i++) eq = eq && p[i] == tomb[i];
    return eq;
}

// A head in the workspace: source src of range q at (q * nsrc + src) * 2.
__device__ __forceinline__ Head load_head(const u32x4 *w) {
    const u32x4 p = w[0], s = w[1];
    return Head{{p.x, p.y, p.z, p.w}, s.x, s.y, s.z};
}

__device__ __forceinline__ void store_head(u32x4 *w, const Head &h) {
    u32x4 p, s;
    p.x = h.kw[0]; p.y = h.kw[1]; p.z = h.kw[2]; p.w = h.kw[3];
    s.x = h.klen; s.y = h.tab; s.z = h.ent; s.w = 0;
    w[0] = p;
    w[1] = s;
}

__device__ __forceinline__ void load_bounds(const ScanArgs &sc, uint64_t q, Bound &lo, Bound &hi) {
    const uint64_t l0 = sc.lo_off[q], h0 = sc.hi_off[q];
    lo.len = sc.lo_off[q + 1] - l0;
    lo.p = sc.lo + l0;
    lo.none = false;
    key_prefix(lo.p, lo.len, lo.w);
    hi.len = sc.hi_off[q + 1] - h0;
    hi.p = sc.hi + h0;
    hi.none = (sc.flags[q] & LSM_SCAN_NO_UPPER) != 0;
    key_prefix(hi.p, hi.len, hi.w);
}

}  // namespace
}  // namespace lsm
