// dbscan.hip — the batched range scan with the memtables in front
// (lsm_db_scan): lsm_tree_scan's merge (treescan.hip, treescan_core.h) over
// nlog further sources, one per memtable, that answer before every table --
// memtable.Manager.Search's order (memtable/manager.go:61-74: Mem, then the
// IMems newest first), then Manager.Search's (manager.go:99-133).
//
// Source s < nlog is the memtable of log nlog - 1 - s: its slice of d_idx
// (lsm_memtable_order, LSM_MEMTABLE_ALL), the nodes in key order.  Its Seek
// is the lower bound of lo over that slice -- one Key16 gather per step from
// lsm_memtable_search's index where the log's nodes lie inside the indexed
// count, d_idx -> d_desc -> key otherwise -- and its Next is the next position
// of d_idx.  A memtable head is {prefix, klen, tab = the log, ent = the
// position in d_idx}; its key bytes are in d_bytes, a table head's in d_img,
// and the source's number tells which.  Sources nlog .. are lsm_tree_scan's.
//
// Two launches, as lsm_tree_scan: the Seeks, one thread per (range, source),
// leave the first heads in the workspace; the walk runs a wave per range and a
// lane per source, the head in registers up to 64 sources, in the workspace
// (a round of 64 sources at a time) past that.  Every lane whose head is the
// emitted key advances in the same step, so their loads are in flight
// together.  nlog == 0 runs lsm_tree_scan itself.
#include "treescan_core.h"

namespace lsm {
namespace {

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

// A head's key bytes, in the buffer of its kind.
__device__ __forceinline__ const uint8_t *head_key(const GetArgs &a, const MemArgs &m, bool mem, uint32_t tab,
                                                   uint32_t ent, uint32_t &len) {
    if (mem) {
        lsm_rec_desc d;
        const uint8_t *p = node_key(m, ent, d);
        len = d.key_len;
        return p;
    }
    return entry_key(a, tab, ent, len);
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

// Go string order of two heads of either kind: <0, 0, >0.
__device__ __forceinline__ int db_head_cmp(const GetArgs &a, const MemArgs &m, const Head &x, bool xmem,
                                           const Head &y, bool ymem) {
    int c = prefix_cmp(x.kw, y.kw);
    if (c == 0) {
        if (x.klen <= 16 || y.klen <= 16) {
            c = x.klen < y.klen ? -1 : x.klen > y.klen ? 1 : 0;
        } else {
            uint32_t xl, yl;
            const uint8_t *xp = head_key(a, m, xmem, x.tab, x.ent, xl);
            const uint8_t *yp = head_key(a, m, ymem, y.tab, y.ent, yl);
            c = go_cmp(xp + 16, xl - 16, yp + 16, yl - 16);
        }
    }
    return c;
}

// The Seeks, one thread per (range, source); the heads go to the workspace.
__global__ __launch_bounds__(256) void db_scan_seek_kernel(GetArgs a, const McFile *files, SrShape S, MemArgs m,
                                                          ScanArgs sc) {
    const uint64_t total = sc.nq * sc.nsrc;
    const uint64_t nindexed = mem_indexed(m);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t q = i / sc.nsrc;
        const uint32_t src = (uint32_t)(i - q * sc.nsrc);
        Bound lo, hi;
        load_bounds(sc, q, lo, hi);
        Head h;
        h.tab = kTsNone;
        // an empty range (lo >= hi) has no head
        if (hi.none || bound_cmp_fast(lo.w, lo.len, lo.p, hi.w, hi.len, hi.p) < 0) {
            if (src < m.nlog) mem_seek(m, nindexed, m.nlog - 1 - src, lo, hi, h);
            else seek_source(a, files, S, src - m.nlog, lo, hi, h);
        }
        store_head(sc.ws + i * 2, h);
    }
}

// The walk, one wave per range.  Wide: more than 64 sources, the lane's heads
// (source r * 64 + lane in round r) stay in the workspace; otherwise its one
// head is kept in registers.
template <bool Wide>
__global__ __launch_bounds__(kTsThreads) void db_scan_kernel(GetArgs a, SrShape S, MemArgs m, ScanArgs sc,
                                                            int32_t *src_out) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * kTsWaves + threadIdx.x / kWave;
    const uint64_t nwave = (uint64_t)gridDim.x * kTsWaves;
    const uint32_t rounds = Wide ? sc.rounds : 1;
    const bool row0 = !Wide && sc.nsrc <= 16;
    const uint64_t nindexed = mem_indexed(m);
    u32x4 *wsw = nullptr;  // the range's heads
    Head h1;
    h1.tab = kTsNone;
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
        // the heads the Seeks left (none for an empty range)
        wsw = sc.ws + q * sc.nsrc * 2;
        if constexpr (!Wide) {
            h1.tab = kTsNone;
            if (lane < sc.nsrc) h1 = load_head(wsw + lane * 2);
        }
        for (;;) {
            // the lane's least head, the lower source on equal keys
            Head b = get(0);
            uint32_t bsrc = lane;
            for (uint32_t r = 1; r < rounds; r++) {
                const Head x = get(r);
                const uint32_t xsrc = r * kWave + lane;
                if (x.tab != kTsNone &&
                    (b.tab == kTsNone || db_head_cmp(a, m, x, xsrc < m.nlog, b, bsrc < m.nlog) < 0)) {
                    b = x;
                    bsrc = xsrc;
                }
            }
            const bool bmem = bsrc < m.nlog;
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
                    const bool lmem = (uint32_t)__shfl((int)bsrc, (int)lead) < m.nlog;
                    int c = 1;
                    if (cand) {
                        uint32_t xl, yl;
                        const uint8_t *xp = head_key(a, m, bmem, b.tab, b.ent, xl);
                        const uint8_t *yp = head_key(a, m, lmem, ltab, lent, yl);
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
            // that holds the key, else Search's table
            const uint32_t wsrc = wave_min_u32(cand ? bsrc : ~0u, row0);
            const uint32_t wl = wsrc & (kWave - 1);
            const bool winner = cand && bsrc == wsrc;
            if (count == sc.limit && sc.mode == LSM_SCAN_RAW) {
                more = 1;  // a further key of the range
                break;
            }
            // the answering entry: a memtable node's own descriptor, or the
            // table's value as lsm_level_get gives it (GetValueByOffset)
            int32_t res = LSM_GET_ABSENT;
            lsm_rec_desc kd{0, 0, 0}, v{0, 0, 0};
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
                    kd = a.idx_desc[T.base + b.ent];
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
                    src_out[o] = bmem ? LSM_SRC_MEMTABLE : LSM_SRC_SSTABLE;
                }
                count++;
            }
            // Next on every source whose head is this key
            if constexpr (!Wide) {
                if (cand) {
                    Head h;
                    if (bmem) mem_place(m, nindexed, hi, b.tab, b.ent + 1, (uint32_t)m.file_start[b.tab + 1], h);
                    else place(a, hi, b.tab, b.ent + 1, source_end(S, lane - m.nlog), h);
                    h1 = h;
                }
            } else {
                const uint32_t wtab = (uint32_t)__shfl((int)b.tab, (int)wl);
                const uint32_t went = (uint32_t)__shfl((int)b.ent, (int)wl);
                const bool wmem = wsrc < m.nlog;
                const Head mh{{mw[0], mw[1], mw[2], mw[3]}, (uint32_t)__shfl((int)b.klen, (int)wl), wtab, went};
                for (uint32_t r = 0; r < rounds; r++) {
                    const Head x = get(r);
                    const uint32_t xsrc = r * kWave + lane;
                    const bool xmem = xsrc < m.nlog;
                    if (x.tab == kTsNone || db_head_cmp(a, m, x, xmem, mh, wmem) != 0) continue;
                    Head h;
                    if (xmem) mem_place(m, nindexed, hi, x.tab, x.ent + 1, (uint32_t)m.file_start[x.tab + 1], h);
                    else place(a, hi, x.tab, x.ent + 1, source_end(S, xsrc - m.nlog), h);
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

}  // namespace
}  // namespace lsm

using namespace lsm;

// Sources: one per memtable, one per level-0 table, one per level 1..6.
static uint64_t db_scan_sources(uint32_t nlog, const SrShape &S) {
    return (uint64_t)nlog + S.start[1] + (kSrLevels - 1);
}

// A head per range and source.  A size no buffer has when the product leaves
// 64 bits (scan_ws_bytes' rule).
static size_t db_scan_ws_bytes(uint32_t nlog, const SrShape &S, uint64_t nq) {
    if ((uint64_t)nlog + S.start[kSrLevels] == 0) return 0;
    const uint64_t nsrc = db_scan_sources(nlog, S);
    if (nq > (~(uint64_t)0 / kTsHeadBytes) / nsrc) return ~(size_t)0;
    return (size_t)(nq * nsrc * kTsHeadBytes);
}

extern "C" size_t lsm_db_scan_workspace_bytes(uint32_t nlog, const uint32_t *level_start, uint64_t nq) {
    SrShape S{};
    if (!level_start || !search_shape(level_start, S)) return 0;
    return db_scan_ws_bytes(nlog, S, nq);
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
    if (!ctx) return LSM_EINVAL;
    if (nq == 0) return 0;
    SrShape S{};
    if (!level_start || !search_shape(level_start, S)) return LSM_EINVAL;
    if (limit == 0 || nq >= (1ull << 32) || nq * limit >= (1ull << 32)) return LSM_EINVAL;
    if (mode != LSM_SCAN_RAW && mode != LSM_SCAN_LIVE) return LSM_EINVAL;
    if (nlog > 65535) return LSM_EINVAL;
    if (!d_lo || !d_lo_off || !d_hi || !d_hi_off || !d_flags || !d_count || !d_more || !d_key || !d_value ||
        !d_src || !d_table || !d_result)
        return LSM_EINVAL;
    if (nlog && (!d_bytes || !d_desc || !d_idx || !d_file_start)) return LSM_EINVAL;
    const uint32_t nfile = S.start[kSrLevels];
    if (nfile && (!d_img || !d_index || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value))
        return LSM_EINVAL;
    if (db_scan_sources(nlog, S) > 0xFFFFFFFFull) return LSM_EINVAL;
    // the index's header: what an index of one node holds before that node
    const size_t index_min = lsm_memtable_search_index_bytes(1), index_hdr = index_min - sizeof(u32x4);
    if (d_mem_index && mem_index_bytes < index_min) return LSM_ESPACE;
    GetArgs a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc, d_idx_value);
    if (nfile) {
        const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
        if (rc) return rc;
    }
    const size_t need = db_scan_ws_bytes(nlog, S, nq);
    if (need && (!d_workspace || ws_bytes < need)) return LSM_ESPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nlog == 0) {
        // the tree alone: lsm_tree_scan's kernels (its checks pass: they are
        // the ones above), every entry a table's
        const int rc = lsm_tree_scan(ctx, d_img, d_index, level_start, d_file_off, d_file_len, d_meta, d_rec_base,
                                     d_idx_desc, d_idx_value, d_tree, tree_nidx, tree_bytes, d_lo, d_lo_off, d_hi,
                                     d_hi_off, d_flags, nq, limit, mode, d_count, d_more, d_key, d_value, d_table,
                                     d_result, d_workspace, ws_bytes, stream);
        if (rc) return rc;
        if (nfile)
            LSM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_src), LSM_SRC_SSTABLE,
                                            (size_t)(nq * limit), s));
        return 0;
    }
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
    sc.nsrc = (uint32_t)db_scan_sources(nlog, S);
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
    hipLaunchKernelGGL(db_scan_seek_kernel, dim3(gs < kTsSeekMaxGrid ? (uint32_t)gs : kTsSeekMaxGrid), dim3(256), 0,
                       s, a, files, S, m, sc);
    LSM_HIP_CHECK(hipGetLastError());
    const uint64_t g = (nq + kTsWaves - 1) / kTsWaves;
    const dim3 grid(g < kTsMaxGrid ? (uint32_t)g : kTsMaxGrid);
    if (sc.rounds > 1)
        hipLaunchKernelGGL(db_scan_kernel<true>, grid, dim3(kTsThreads), 0, s, a, S, m, sc, d_src);
    else
        hipLaunchKernelGGL(db_scan_kernel<false>, grid, dim3(kTsThreads), 0, s, a, S, m, sc, d_src);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}
