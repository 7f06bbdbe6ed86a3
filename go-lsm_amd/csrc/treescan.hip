// treescan.hip — the batched range scans: lsm_tree_scan over the SSTable tree
// and lsm_db_scan with the memtables in front of it.  The ordered read
// go-lsm's pieces add up to -- sstable.Iterator (sstable/iterator.go:9-73)
// over block.Iterator.Seek / Next / Valid / Key (sstable/block/index.go:
// 157-181), one per source, merged in Manager.Search's order (manager.go:
// 99-133), behind memtable.Manager.Search's (memtable/manager.go:61-74: Mem,
// then the IMems newest first).
//
// One wave per range, one lane per source.  Source s < nlog is the memtable of
// log nlog - 1 - s: its slice of d_idx (lsm_memtable_order, LSM_MEMTABLE_ALL),
// the nodes in key order.  Past them level-0 table t is source nlog + t, level
// L >= 1 (its tables walked one after the other) source nlog + n0 + L - 1.
// lsm_tree_scan is the scan with nlog = 0: its kernels (DB = false) hold no
// memtable code.
//
// A lane enters a table source with the Seek the Gets run (seek.h: the sparse
// index picks the table of a level >= 1, then Go's bisection through the Seek
// tree or over the index), a memtable source with the lower bound of lo over
// its slice -- one Key16 gather per step from lsm_memtable_search's index
// where the log's nodes lie inside the indexed count, d_idx -> d_desc -> key
// otherwise -- and keeps its cursor and its head entry's 16-byte big-endian
// prefix and length.  A head is {prefix, klen, tab, ent}: a table and its
// entry, or a log and the position in d_idx; a table head's key bytes are in
// d_img, a memtable head's in d_bytes, and the source's number tells which.
// A step is a wave-wide minimum over the prefixes (four 32-bit DPP reductions,
// then the lengths; the bytes past 16 only when every tied key is longer than
// that), the lowest source among the equal keys answers, and every lane whose
// head equals the minimum advances: the loads of the sources' next heads are
// all in flight together.  More than 64 sources run the same step with each
// lane's heads kept in the workspace, one per round of 64 sources.
//
// Two launches: the Seeks run first, one thread per (range, source), and leave
// each source's first head in the workspace; the walk's kernel then carries
// none of the bisection's registers (the Seek tree's blocks) and runs at five
// waves per SIMD against three, which is what a chain of dependent loads is
// short of (profiles/scan_resources.md).
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

// The memtables: lsm_memtable_search's inputs.  index[p] is node d_idx[p]'s
// Key16 {bytes 0-7, bytes 8-15 as big-endian integers} as four 32-bit words.
struct MemArgs {
    const uint8_t *bytes;
    const lsm_rec_desc *desc;
    const uint32_t *idx;
    const uint64_t *file_start;
    uint32_t nlog;
    const uint64_t *index_hdr;  // or NULL: no index
    const u32x4 *index;
    uint64_t index_cap;  // nodes the index buffer has room for
};

// A source's head entry: entry `ent` of table `tab`, or position `ent` of
// d_idx in log `tab` (kTsNone: the source is exhausted, or past the range's
// end), its key's prefix and length.
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

// ---- a table source -----------------------------------------------------------

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

// Where table source src's tables end: a level-0 table is its own source,
// level L's tables end at start[L + 1].
__device__ __forceinline__ uint32_t source_end(const SrShape &S, uint32_t src) {
    const uint32_t n0 = S.start[1];
    if (src < n0) return src + 1;
    uint32_t end = 0;
#pragma unroll
    for (uint32_t L = 1; L < kSrLevels; L++)
        if (src - n0 + 1 == L) end = S.start[L + 1];
    return end;
}

// Iterator.Seek(lo) on table source src -> its first head.
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

// ---- a memtable source ----------------------------------------------------------

// The nodes the index vouches for: those its build wrote, within the buffer.
__device__ __forceinline__ uint64_t mem_indexed(const MemArgs &m) {
    if (!m.index_hdr) return 0;
    const uint64_t n = m.index_hdr[0];
    return n < m.index_cap ? n : m.index_cap;
}

// An index element as the walk's prefix words.
__device__ __forceinline__ void index_prefix(const u32x4 k, uint32_t kw[4]) {
    kw[0] = k.y;
    kw[1] = k.x;
    kw[2] = k.w;
    kw[3] = k.z;
}

// The node at position p of d_idx: its descriptor, its key bytes.
__device__ __forceinline__ const uint8_t *node_key(const MemArgs &m, uint32_t p, lsm_rec_desc &d) {
    d = m.desc[m.idx[p]];
    return m.bytes + d.rec_off + 4;
}

// The memtable source's head at position p of log w's nodes [.., end): Valid /
// Key after a Seek or a Next.  Past the log's last node the source is
// exhausted; so it is at a key at or past the range's end.  Positions are
// 32-bit: nslot < 2^32 - 1.
__device__ __forceinline__ void mem_place(const MemArgs &m, uint64_t nindexed, const Bound &hi, uint32_t w,
                                          uint32_t p, uint32_t end, Head &h) {
    h.tab = kTsNone;
    h.ent = p;
    if (p >= end) return;
    u32x4 k{};
    const bool indexed = end <= nindexed;
    if (indexed) k = m.index[p];
    lsm_rec_desc d;
    const uint8_t *kp = node_key(m, p, d);
    h.klen = d.key_len;
    if (indexed) index_prefix(k, h.kw);
    else key_prefix(kp, h.klen, h.kw);
    if (!hi.none && bound_cmp_fast(h.kw, h.klen, kp, hi.w, hi.len, hi.p) >= 0) return;
    h.tab = w;
}

// The memtable Seek: the first node of log w with key >= lo (the lower bound
// over its slice of d_idx; the skiplist's own steps are not observable).
__device__ __forceinline__ void mem_seek(const MemArgs &m, uint64_t nindexed, uint32_t w, const Bound &lo,
                                         const Bound &hi, Head &h) {
    uint32_t left = (uint32_t)m.file_start[w], right = (uint32_t)m.file_start[w + 1];
    const uint32_t end = right;
    const bool indexed = end <= nindexed;
    while (left < right) {
        const uint32_t mid = left + (right - left) / 2;
        uint32_t nw[4];
        int c;
        if (indexed) {
            index_prefix(m.index[mid], nw);
            c = prefix_cmp(nw, lo.w);
            if (c == 0) {  // a 16-byte tie: the node itself
                lsm_rec_desc d;
                const uint8_t *np = node_key(m, mid, d);
                c = bound_cmp(nw, d.key_len, np, lo.w, lo.len, lo.p);
            }
        } else {
            lsm_rec_desc d;
            const uint8_t *np = node_key(m, mid, d);
            key_prefix(np, d.key_len, nw);
            c = bound_cmp_fast(nw, d.key_len, np, lo.w, lo.len, lo.p);
        }
        if (c < 0) left = mid + 1;
        else right = mid;
    }
    mem_place(m, nindexed, hi, w, left, end, h);
}

// ---- heads of either kind -------------------------------------------------------
//
// DB: the scan has memtable sources, and `mem` says whether this head's is
// one.  Without DB every head is a table's, and m is not read.

// A head's key bytes, in the buffer of its kind.
template <bool DB>
__device__ __forceinline__ const uint8_t *head_key(const GetArgs &a, const MemArgs &m, bool mem, uint32_t tab,
                                                   uint32_t ent, uint32_t &len) {
    if constexpr (DB) {
        if (mem) {
            lsm_rec_desc d;
            const uint8_t *p = node_key(m, ent, d);
            len = d.key_len;
            return p;
        }
    }
    return entry_key(a, tab, ent, len);
}

// Go string order of two heads: <0, 0, >0.
template <bool DB>
__device__ __forceinline__ int head_cmp(const GetArgs &a, const MemArgs &m, const Head &x, bool xmem,
                                        const Head &y, bool ymem) {
    int c = prefix_cmp(x.kw, y.kw);
    if (c == 0) {
        if (x.klen <= 16 || y.klen <= 16) {
            c = x.klen < y.klen ? -1 : x.klen > y.klen ? 1 : 0;
        } else {
            uint32_t xl, yl;
            const uint8_t *xp = head_key<DB>(a, m, xmem, x.tab, x.ent, xl);
            const uint8_t *yp = head_key<DB>(a, m, ymem, y.tab, y.ent, yl);
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

// ---- the two launches -----------------------------------------------------------

// The Seeks, one thread per (range, source): every lane of a wave runs a
// bisection (the walk's waves have a lane per source, few of them live), and
// the walk's kernel carries none of the Seek's registers.  The heads go to the
// workspace.
template <bool DB>
__device__ __forceinline__ void scan_seek(GetArgs a, const McFile *files, SrShape S, MemArgs m, ScanArgs sc) {
    const uint64_t total = sc.nq * sc.nsrc;
    const uint32_t nlog = DB ? m.nlog : 0;
    const uint64_t nindexed = DB ? mem_indexed(m) : 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t q = i / sc.nsrc;
        const uint32_t src = (uint32_t)(i - q * sc.nsrc);
        Bound lo, hi;
        load_bounds(sc, q, lo, hi);
        Head h;
        h.tab = kTsNone;
        // an empty range (lo >= hi) has no head
        if (hi.none || bound_cmp_fast(lo.w, lo.len, lo.p, hi.w, hi.len, hi.p) < 0) {
            if (src < nlog) mem_seek(m, nindexed, nlog - 1 - src, lo, hi, h);
            else seek_source(a, files, S, src - nlog, lo, hi, h);
        }
        store_head(sc.ws + i * 2, h);
    }
}

// The walk, one wave per range.  Wide: more than 64 sources, the lane's heads
// (source r * 64 + lane in round r) stay in the workspace; otherwise its one
// head is kept in registers.
template <bool Wide, bool DB>
__device__ __forceinline__ void scan_walk(GetArgs a, SrShape S, MemArgs m, ScanArgs sc, int32_t *src_out) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * kTsWaves + threadIdx.x / kWave;
    const uint64_t nwave = (uint64_t)gridDim.x * kTsWaves;
    const uint32_t rounds = Wide ? sc.rounds : 1;
    const bool row0 = !Wide && sc.nsrc <= 16;
    const uint32_t nlog = DB ? m.nlog : 0;
    const uint64_t nindexed = DB ? mem_indexed(m) : 0;
    u32x4 *wsw = nullptr;  // the range's heads
    Head h1;
    h1.tab = kTsNone;
    // the tree's register path: the table of h1 -- its entries, its first slot
    // of the decoded index -- and the head's rec_off (what its descriptor holds)
    uint32_t n1 = 0;
    uint64_t base1 = 0, roff1 = 0;
    auto refresh1 = [&]() {
        if (h1.tab == kTsNone) return;
        n1 = table_entries(a, h1.tab);
        base1 = table_base(a, h1.tab);
        roff1 = a.idx_desc[base1 + h1.ent].rec_off;
    };
    // a lane past the last source has no head
    auto get = [&](uint32_t r) {
        if constexpr (!Wide) {
            return h1;
        } else {
            Head h;
            h.tab = kTsNone;
            if (r * kWave + lane < sc.nsrc) h = load_head(wsw + (r * kWave + lane) * 2);
            return h;
        }
    };
    auto put = [&](uint32_t r, const Head &h) {
        if constexpr (!Wide) h1 = h;
        else store_head(wsw + (r * kWave + lane) * 2, h);
    };
    for (uint64_t q = wave; q < sc.nq; q += nwave) {
        Bound lo, hi;
        load_bounds(sc, q, lo, hi);
        uint32_t count = 0, more = 0;
        // Next on source src, whose head is x
        auto next = [&](const Head &x, uint32_t src, Head &h) {
            if (src < nlog) mem_place(m, nindexed, hi, x.tab, x.ent + 1, (uint32_t)m.file_start[x.tab + 1], h);
            else place(a, hi, x.tab, x.ent + 1, source_end(S, src - nlog), h);
        };
        // the heads the Seeks left (none for an empty range)
        wsw = sc.ws + q * sc.nsrc * 2;
        if constexpr (!Wide) {
            h1.tab = kTsNone;
            if (lane < sc.nsrc) h1 = load_head(wsw + lane * 2);
            if constexpr (!DB) refresh1();
        }
        for (;;) {
            // the lane's least head, the lower source on equal keys
            Head b = get(0);
            uint32_t bsrc = lane;
            for (uint32_t r = 1; r < rounds; r++) {
                const Head x = get(r);
                const uint32_t xsrc = r * kWave + lane;
                if (x.tab != kTsNone &&
                    (b.tab == kTsNone || head_cmp<DB>(a, m, x, xsrc < nlog, b, bsrc < nlog) < 0)) {
                    b = x;
                    bsrc = xsrc;
                }
            }
            const bool bmem = bsrc < nlog;
            bool cand = b.tab != kTsNone;
            if (__ballot(cand) == 0) break;  // every source is exhausted
            // the wave's least key: the prefix word by word, then the length
            uint32_t mw[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                mw[j] = wave_min_u32(cand ? b.kw[j] : ~0u, row0);
                cand = cand && b.kw[j] == mw[j];
            }
            const uint32_t ml = wave_min_u32(cand ? (b.klen < 17u ? b.klen : 17u) : ~0u, row0);
            if (ml <= 16) {
                // a key of at most 16 bytes sorts before every longer one it prefixes
                cand = cand && b.klen == ml;
            } else {
                // every tied key goes on past 16 bytes: compare those against the
                // lowest tied lane's (its kind travels with its tab / ent), moving
                // to a lane that holds a smaller key
                uint32_t lead = (uint32_t)__ffsll((long long)__ballot(cand)) - 1;
                for (;;) {
                    const uint32_t ltab = (uint32_t)__shfl((int)b.tab, (int)lead);
                    const uint32_t lent = (uint32_t)__shfl((int)b.ent, (int)lead);
                    const bool lmem = (uint32_t)__shfl((int)bsrc, (int)lead) < nlog;
                    int c = 1;
                    if (cand) {
                        uint32_t xl, yl;
                        const uint8_t *xp = head_key<DB>(a, m, bmem, b.tab, b.ent, xl);
                        const uint8_t *yp = head_key<DB>(a, m, lmem, ltab, lent, yl);
                        c = go_cmp(xp + 16, xl - 16, yp + 16, yl - 16);
                    }
                    const uint64_t less = __ballot(cand && c < 0);
                    if (less == 0) {
                        cand = cand && c == 0;
                        break;
                    }
                    lead = (uint32_t)__ffsll((long long)less) - 1;
                }
            }
            // the lowest source among the equal keys answers: the newest memtable
            // that holds the key, else Search's table (manager.go:99-133)
            const uint32_t wsrc = wave_min_u32(cand ? bsrc : ~0u, row0);
            const uint32_t wl = wsrc & (kWave - 1);
            const bool winner = cand && bsrc == wsrc;
            if (count == sc.limit && sc.mode == LSM_SCAN_RAW) {
                more = 1;  // a further key of the range
                break;
            }
            int32_t res = LSM_GET_ABSENT;
            lsm_rec_desc kd{0, 0, 0}, v{0, 0, 0};
            if constexpr (!Wide && !DB) {
                // The tree's register walk.  One step in two dependent round trips:
                // the winner's value offset and its table (wave-uniform addresses:
                // every lane reads them) beside each advancing lane's next
                // descriptor, then the value's length beside the next key's bytes.
                // A lane at its table's last two entries takes place()'s path (the
                // next table, the boundary key) instead.
                const uint32_t wtab = (uint32_t)__builtin_amdgcn_readlane((int)b.tab, (int)wl);
                const uint32_t went = (uint32_t)__builtin_amdgcn_readlane((int)b.ent, (int)wl);
                const uint64_t wslot =
                    ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(base1 >> 32), (int)wl) << 32 |
                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base1, (int)wl)) + went;
                const bool fast = cand && b.ent + 2 < n1;
                const int64_t voff = a.idx_value[wslot];
                const lsm_rec_desc nd = a.idx_desc[fast ? base1 + b.ent + 1 : wslot];
                SeekTable T;
                T.fo = a.file_off[wtab];
                T.fl = a.file_len[wtab];
                T.base = 0;
                T.n = 0;
                const uint8_t *np = a.img + nd.rec_off + 4;
                uint64_t f0 = ldg_u64_unaligned(np), f1 = ldg_u64_unaligned(np + 8);
                // its value as lsm_level_get gives it (GetValueByOffset)
                res = value_at_offset(a, T, voff, v);
                const bool emits =
                    !(sc.mode == LSM_SCAN_LIVE && res == LSM_GET_FOUND && is_tombstone_value(a.img, v));
                if (emits) {
                    if (count == sc.limit) {
                        more = 1;
                        break;
                    }
                    if (winner) {
                        const uint64_t o = (uint64_t)q * sc.limit + count;
                        sc.key[o] = lsm_rec_desc{roff1, b.klen, 8};  // as the decode's descriptor holds it
                        sc.value[o] = v;
                        sc.table[o] = (int32_t)b.tab;
                        sc.result[o] = res;
                    }
                    count++;
                }
                // Next on every source whose head is this key
                if (fast) {
                    h1.klen = nd.key_len;
                    prefix_words(f0, f1, h1.klen, h1.kw);
                    h1.ent = b.ent + 1;
                    roff1 = nd.rec_off;
                    if (!hi.none && bound_cmp_fast(h1.kw, h1.klen, np, hi.w, hi.len, hi.p) >= 0) h1.tab = kTsNone;
                } else if (cand) {
                    Head h;
                    next(b, lane, h);
                    h1 = h;
                    refresh1();
                }
                continue;
            }
            // the answering entry: a memtable node's own descriptor, or the
            // table's value as lsm_level_get gives it (GetValueByOffset)
            bool emit = false;
            if (winner) {
                if (bmem) {
                    node_key(m, b.ent, kd);
                    v = lsm_rec_desc{kd.rec_off + 4 + kd.key_len, 0, kd.val_len};
                    res = LSM_GET_FOUND;
                    emit = !(sc.mode == LSM_SCAN_LIVE && is_tombstone_value(m.bytes, v));
                } else {
                    SeekTable T;
                    T.fo = a.file_off[b.tab];
                    T.fl = a.file_len[b.tab];
                    T.base = table_base(a, b.tab);
                    T.n = 0;
                    // (built from its fields as v is: assigned whole, kd takes an LDS slot
                    // in tree_scan_kernel<true>, profiles/scan_resources.md)
                    const lsm_rec_desc d = a.idx_desc[T.base + b.ent];
                    kd = lsm_rec_desc{d.rec_off, d.key_len, d.val_len};
                    res = value_by_offset(a, T, b.ent, v);
                    emit = !(sc.mode == LSM_SCAN_LIVE && res == LSM_GET_FOUND && is_tombstone_value(a.img, v));
                }
            }
            const bool emits = __ballot(emit) != 0;
            if (emits) {
                if (count == sc.limit) {
                    more = 1;
                    break;
                }
                if (winner) {
                    const uint64_t o = (uint64_t)q * sc.limit + count;
                    sc.key[o] = kd;
                    sc.value[o] = v;
                    sc.table[o] = (int32_t)b.tab;
                    sc.result[o] = res;
                    if constexpr (DB) src_out[o] = bmem ? LSM_SRC_MEMTABLE : LSM_SRC_SSTABLE;
                }
                count++;
            }
            // Next on every source whose head is this key
            if constexpr (!Wide) {
                if (cand) {
                    Head h;
                    next(b, lane, h);
                    h1 = h;
                }
            } else {
                const uint32_t wtab = (uint32_t)__shfl((int)b.tab, (int)wl);
                const uint32_t went = (uint32_t)__shfl((int)b.ent, (int)wl);
                const Head mh{{mw[0], mw[1], mw[2], mw[3]}, (uint32_t)__shfl((int)b.klen, (int)wl), wtab, went};
                for (uint32_t r = 0; r < rounds; r++) {
                    const Head x = get(r);
                    const uint32_t xsrc = r * kWave + lane;
                    if (x.tab == kTsNone || head_cmp<DB>(a, m, x, xsrc < nlog, mh, wsrc < nlog) != 0) continue;
                    Head h;
                    next(x, xsrc, h);
                    put(r, h);
                }
            }
        }
        if (lane == 0) {
            sc.count[q] = count;
            sc.more[q] = (uint8_t)more;
        }
    }
}

// The kernels: the tree's take no memtables and write no d_src.  The bodies
// take the arguments by value, as a kernel does: by reference the same code
// is scheduled further from the form that was measured
// (profiles/scan_resources.md).
__global__ __launch_bounds__(256) void tree_scan_seek_kernel(GetArgs a, const McFile *files, SrShape S,
                                                            ScanArgs sc) {
    scan_seek<false>(a, files, S, MemArgs{}, sc);
}

template <bool Wide>
__global__ __launch_bounds__(kTsThreads) void tree_scan_kernel(GetArgs a, SrShape S, ScanArgs sc) {
    scan_walk<Wide, false>(a, S, MemArgs{}, sc, nullptr);
}

__global__ __launch_bounds__(256) void db_scan_seek_kernel(GetArgs a, const McFile *files, SrShape S, MemArgs m,
                                                          ScanArgs sc) {
    scan_seek<true>(a, files, S, m, sc);
}

template <bool Wide>
__global__ __launch_bounds__(kTsThreads) void db_scan_kernel(GetArgs a, SrShape S, MemArgs m, ScanArgs sc,
                                                            int32_t *src_out) {
    scan_walk<Wide, true>(a, S, m, sc, src_out);
}

}  // namespace
}  // namespace lsm

using namespace lsm;

// Sources: one per memtable, one per level-0 table, one per level 1..6.
static uint64_t scan_sources(uint32_t nlog, const SrShape &S) {
    return (uint64_t)nlog + S.start[1] + (kSrLevels - 1);
}

// A head per range and source, left by the Seeks for the walk; none when there
// is neither a memtable nor a table.  A size no buffer has when the product
// leaves 64 bits.
static size_t scan_ws_bytes(uint32_t nlog, const SrShape &S, uint64_t nq) {
    if ((uint64_t)nlog + S.start[kSrLevels] == 0) return 0;
    const uint64_t nsrc = scan_sources(nlog, S);
    if (nq > (~(uint64_t)0 / kTsHeadBytes) / nsrc) return ~(size_t)0;
    return (size_t)(nq * nsrc * kTsHeadBytes);
}

extern "C" size_t lsm_tree_scan_workspace_bytes(const uint32_t *level_start, uint64_t nq) {
    return lsm_db_scan_workspace_bytes(0, level_start, nq);
}

extern "C" size_t lsm_db_scan_workspace_bytes(uint32_t nlog, const uint32_t *level_start, uint64_t nq) {
    SrShape S{};
    if (!level_start || !search_shape(level_start, S)) return 0;
    return scan_ws_bytes(nlog, S, nq);
}

// Both entry points: the checks, the kernels' arguments, the two launches.
// db: lsm_db_scan's call, which has a d_src; lsm_tree_scan's passes nlog = 0
// and no memtable input.  nlog == 0 runs the tree's kernels either way, every
// entry then a table's.
static int scan(bool db, lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc, const uint32_t *d_idx,
                const uint64_t *d_file_start, uint32_t nlog, const void *d_mem_index, size_t mem_index_bytes,
                const uint8_t *d_img, const void *d_index, const uint32_t *level_start,
                const uint64_t *d_file_off, const uint64_t *d_file_len, const lsm_sst_meta *d_meta,
                const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
                const void *d_tree, uint32_t tree_nidx, size_t tree_bytes, const uint8_t *d_lo,
                const uint64_t *d_lo_off, const uint8_t *d_hi, const uint64_t *d_hi_off, const uint8_t *d_flags,
                uint64_t nq, uint32_t limit, int mode, uint32_t *d_count, uint8_t *d_more, lsm_rec_desc *d_key,
                lsm_rec_desc *d_value, int32_t *d_src, int32_t *d_table, int32_t *d_result, void *d_workspace,
                size_t ws_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nq == 0) return 0;
    SrShape S{};
    if (!level_start || !search_shape(level_start, S)) return LSM_EINVAL;
    if (limit == 0 || nq >= (1ull << 32) || nq * limit >= (1ull << 32)) return LSM_EINVAL;
    if (mode != LSM_SCAN_RAW && mode != LSM_SCAN_LIVE) return LSM_EINVAL;
    if (nlog > 65535 || scan_sources(nlog, S) > 0xFFFFFFFFull) return LSM_EINVAL;
    if (!d_lo || !d_lo_off || !d_hi || !d_hi_off || !d_flags || !d_count || !d_more || !d_key || !d_value ||
        (db && !d_src) || !d_table || !d_result)
        return LSM_EINVAL;
    if (nlog && (!d_bytes || !d_desc || !d_idx || !d_file_start)) return LSM_EINVAL;
    const uint32_t nfile = S.start[kSrLevels];
    if (nfile && (!d_img || !d_index || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value))
        return LSM_EINVAL;
    // the index's header: what an index of one node holds before that node
    const size_t index_min = lsm_memtable_search_index_bytes(1), index_hdr = index_min - sizeof(u32x4);
    if (d_mem_index && mem_index_bytes < index_min) return LSM_ESPACE;
    GetArgs a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc, d_idx_value);
    if (nfile) {
        const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
        if (rc) return rc;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t need = scan_ws_bytes(nlog, S, nq);
    if (need == 0) {  // neither a memtable nor a table: nothing in any range, and no workspace
        LSM_HIP_CHECK(hipMemsetAsync(d_count, 0, 4 * nq, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_more, 0, nq, s));
        return 0;
    }
    if (!d_workspace || ws_bytes < need) return LSM_ESPACE;
    MemArgs m{};
    m.bytes = d_bytes;
    m.desc = d_desc;
    m.idx = d_idx;
    m.file_start = d_file_start;
    m.nlog = nlog;
    if (d_mem_index) {
        const uint8_t *p = static_cast<const uint8_t *>(d_mem_index);
        m.index_hdr = reinterpret_cast<const uint64_t *>(p);
        m.index = reinterpret_cast<const u32x4 *>(p + index_hdr);
        m.index_cap = (mem_index_bytes - index_hdr) / sizeof(u32x4);
    }
    ScanArgs sc{};
    sc.lo = d_lo;
    sc.hi = d_hi;
    sc.lo_off = d_lo_off;
    sc.hi_off = d_hi_off;
    sc.flags = d_flags;
    sc.nq = nq;
    sc.limit = limit;
    sc.mode = mode;
    sc.nsrc = (uint32_t)scan_sources(nlog, S);
    sc.rounds = (sc.nsrc + kWave - 1) / kWave;
    sc.count = d_count;
    sc.more = d_more;
    sc.key = d_key;
    sc.value = d_value;
    sc.table = d_table;
    sc.result = d_result;
    sc.ws = static_cast<u32x4 *>(d_workspace);
    const McFile *files = static_cast<const McFile *>(d_index);
    const uint64_t gs = (nq * sc.nsrc + 255) / 256;
    const dim3 sgrid(gs < kTsSeekMaxGrid ? (uint32_t)gs : kTsSeekMaxGrid);
    if (nlog) hipLaunchKernelGGL(db_scan_seek_kernel, sgrid, dim3(256), 0, s, a, files, S, m, sc);
    else hipLaunchKernelGGL(tree_scan_seek_kernel, sgrid, dim3(256), 0, s, a, files, S, sc);
    LSM_HIP_CHECK(hipGetLastError());
    const uint64_t g = (nq + kTsWaves - 1) / kTsWaves;
    const dim3 grid(g < kTsMaxGrid ? (uint32_t)g : kTsMaxGrid);
    const bool wide = sc.rounds > 1;
    if (nlog && wide) hipLaunchKernelGGL(db_scan_kernel<true>, grid, dim3(kTsThreads), 0, s, a, S, m, sc, d_src);
    else if (nlog) hipLaunchKernelGGL(db_scan_kernel<false>, grid, dim3(kTsThreads), 0, s, a, S, m, sc, d_src);
    else if (wide) hipLaunchKernelGGL(tree_scan_kernel<true>, grid, dim3(kTsThreads), 0, s, a, S, sc);
    else hipLaunchKernelGGL(tree_scan_kernel<false>, grid, dim3(kTsThreads), 0, s, a, S, sc);
    LSM_HIP_CHECK(hipGetLastError());
    if (db && !nlog)
        LSM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_src), LSM_SRC_SSTABLE,
                                        (size_t)(nq * limit), s));
    return 0;
}

extern "C" int lsm_tree_scan(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index,
                             const uint32_t *level_start, const uint64_t *d_file_off,
                             const uint64_t *d_file_len, const lsm_sst_meta *d_meta,
                             const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                             const int64_t *d_idx_value, const void *d_tree, uint32_t tree_nidx,
                             size_t tree_bytes, const uint8_t *d_lo, const uint64_t *d_lo_off,
                             const uint8_t *d_hi, const uint64_t *d_hi_off, const uint8_t *d_flags,
                             uint64_t nq, uint32_t limit, int mode, uint32_t *d_count, uint8_t *d_more,
                             lsm_rec_desc *d_key, lsm_rec_desc *d_value, int32_t *d_table,
                             int32_t *d_result, void *d_workspace, size_t ws_bytes, void *stream) {
    return scan(false, ctx, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, d_img, d_index, level_start,
                d_file_off, d_file_len, d_meta, d_rec_base, d_idx_desc, d_idx_value, d_tree, tree_nidx, tree_bytes,
                d_lo, d_lo_off, d_hi, d_hi_off, d_flags, nq, limit, mode, d_count, d_more, d_key, d_value, nullptr,
                d_table, d_result, d_workspace, ws_bytes, stream);
}

extern "C" int lsm_db_scan(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc, const uint32_t *d_idx,
                           const uint64_t *d_file_start, uint32_t nlog, const void *d_mem_index,
                           size_t mem_index_bytes, const uint8_t *d_img, const void *d_index,
                           const uint32_t *level_start, const uint64_t *d_file_off, const uint64_t *d_file_len,
                           const lsm_sst_meta *d_meta, const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                           const int64_t *d_idx_value, const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
                           const uint8_t *d_lo, const uint64_t *d_lo_off, const uint8_t *d_hi,
                           const uint64_t *d_hi_off, const uint8_t *d_flags, uint64_t nq, uint32_t limit, int mode,
                           uint32_t *d_count, uint8_t *d_more, lsm_rec_desc *d_key, lsm_rec_desc *d_value,
                           int32_t *d_src, int32_t *d_table, int32_t *d_result, void *d_workspace,
                           size_t ws_bytes, void *stream) {
    return scan(true, ctx, d_bytes, d_desc, d_idx, d_file_start, nlog, d_mem_index, mem_index_bytes, d_img, d_index,
                level_start, d_file_off, d_file_len, d_meta, d_rec_base, d_idx_desc, d_idx_value, d_tree, tree_nidx,
                tree_bytes, d_lo, d_lo_off, d_hi, d_hi_off, d_flags, nq, limit, mode, d_count, d_more, d_key,
                d_value, d_src, d_table, d_result, d_workspace, ws_bytes, stream);
}
