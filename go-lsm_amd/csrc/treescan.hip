// treescan.hip — the batched range scan over the SSTable tree (lsm_tree_scan):
// the ordered read go-lsm's pieces add up to -- sstable.Iterator
// (sstable/iterator.go:9-73) over block.Iterator.Seek / Next / Valid / Key
// (sstable/block/index.go:157-181), one per source, merged in Manager.Search's
// order (manager.go:99-133).
//
// One wave per range, one lane per source: level-0 table s is source s, level
// L >= 1 (its tables walked one after the other) is source n0 + L - 1.  A lane
// enters its source with the Seek the Gets run (seek.h: the sparse index picks
// the table of a level >= 1, then Go's bisection through the Seek tree or over
// the index) and keeps its cursor and its head entry's 16-byte big-endian
// prefix and length in registers.  A step is a wave-wide minimum over the
// prefixes (four 32-bit DPP reductions, then the lengths; the bytes past 16
// only when every tied key is longer than that), the lowest source among the
// equal keys answers, and every lane whose head equals the minimum advances:
// the loads of the sources' next heads are all in flight together.  More than
// 64 sources (a level 0 wider than 58 tables) run the same step with each
// lane's heads kept in the workspace, one per round of 64 sources.
//
// Two launches: the Seeks run first, one thread per (range, source), and leave
// each source's first head in the workspace; the walk's kernel then carries
// none of the bisection's registers (the Seek tree's blocks) and runs at five
// waves per SIMD against three, which is what a chain of dependent loads is
// short of (profiles/treescan_resources.md).
#include "treescan_core.h"

namespace lsm {
namespace {

// The Seeks, one thread per (range, source): every lane of a wave runs a
// bisection (the walk's waves have a lane per source, few of them live), and
// the walk's kernel carries none of the Seek's registers.  The heads go to the
// workspace.
__global__ __launch_bounds__(256) void tree_scan_seek_kernel(GetArgs a, const McFile *files, SrShape S,
                                                            ScanArgs sc) {
    const uint64_t total = sc.nq * sc.nsrc;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t q = i / sc.nsrc;
        const uint32_t src = (uint32_t)(i - q * sc.nsrc);
        Bound lo, hi;
        load_bounds(sc, q, lo, hi);
        Head h;
        h.tab = kTsNone;
        // an empty range (lo >= hi) has no head
        if (hi.none || bound_cmp_fast(lo.w, lo.len, lo.p, hi.w, hi.len, hi.p) < 0)
            seek_source(a, files, S, src, lo, hi, h);
        store_head(sc.ws + i * 2, h);
    }
}

// The walk, one wave per range.  Wide: more than 64 sources, the lane's heads
// (source r * 64 + lane in round r) stay in the workspace; otherwise its one
// head is kept in registers.
template <bool Wide>
__global__ __launch_bounds__(kTsThreads) void tree_scan_kernel(GetArgs a, SrShape S, ScanArgs sc) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * kTsWaves + threadIdx.x / kWave;
    const uint64_t nwave = (uint64_t)gridDim.x * kTsWaves;
    const uint32_t rounds = Wide ? sc.rounds : 1;
    const bool row0 = !Wide && sc.nsrc <= 16;
    u32x4 *wsw = nullptr;  // the range's heads
    Head h1;
    h1.tab = kTsNone;
    // the register path's table of h1: its entries, its first slot of the
    // decoded index, and the head's rec_off (what its descriptor holds)
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
        // the heads the Seeks left (none for an empty range)
        wsw = sc.ws + q * sc.nsrc * 2;
        if constexpr (!Wide) {
            h1.tab = kTsNone;
            if (lane < sc.nsrc) h1 = load_head(wsw + lane * 2);
            refresh1();
        }
        for (;;) {
            // the lane's least head, the lower source on equal keys
            Head b = get(0);
            uint32_t bsrc = lane;
            for (uint32_t r = 1; r < rounds; r++) {
                const Head x = get(r);
                if (x.tab != kTsNone && (b.tab == kTsNone || head_cmp(a, x, b) < 0)) {
                    b = x;
                    bsrc = r * kWave + lane;
                }
            }
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
                // lowest tied lane's, moving to a lane that holds a smaller key
                uint32_t lead = (uint32_t)__ffsll((long long)__ballot(cand)) - 1;
                for (;;) {
                    const uint32_t ltab = (uint32_t)__shfl((int)b.tab, (int)lead);
                    const uint32_t lent = (uint32_t)__shfl((int)b.ent, (int)lead);
                    int c = 1;
                    if (cand) {
                        uint32_t xl, yl;
                        const uint8_t *xp = entry_key(a, b.tab, b.ent, xl);
                        const uint8_t *yp = entry_key(a, ltab, lent, yl);
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
            // the lowest source among the equal keys answers (manager.go:99-133)
            const uint32_t wsrc = wave_min_u32(cand ? bsrc : ~0u, row0);
            const uint32_t wl = wsrc & (kWave - 1);
            const bool winner = cand && bsrc == wsrc;
            if (count == sc.limit && sc.mode == LSM_SCAN_RAW) {
                more = 1;  // a further key of the range
                break;
            }
            int32_t res = LSM_GET_ABSENT;
            lsm_rec_desc v{0, 0, 0};
            if constexpr (!Wide) {
                // One step in two dependent round trips: the winner's value offset
                // and its table (wave-uniform addresses: every lane reads them)
                // beside each advancing lane's next descriptor, then the value's
                // length beside the next key's bytes.  A lane at its table's last
                // two entries takes place()'s path (the next table, the boundary
                // key) instead.
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
                    place(a, hi, b.tab, b.ent + 1, source_end(S, lane), h);
                    h1 = h;
                    refresh1();
                }
                continue;
            }
            // the workspace path: its value as lsm_level_get gives it (GetValueByOffset)
            bool emit = false;
            if (winner) {
                SeekTable T;
                T.fo = a.file_off[b.tab];
                T.fl = a.file_len[b.tab];
                T.base = table_base(a, b.tab);
                T.n = 0;
                res = value_by_offset(a, T, b.ent, v);
                emit = !(sc.mode == LSM_SCAN_LIVE && res == LSM_GET_FOUND && is_tombstone_value(a.img, v));
            }
            const bool emits = __ballot(emit) != 0;
            if (emits) {
                if (count == sc.limit) {
                    more = 1;
                    break;
                }
                if (winner) {
                    const uint64_t o = (uint64_t)q * sc.limit + count;
                    sc.key[o] = a.idx_desc[table_base(a, b.tab) + b.ent];
                    sc.value[o] = v;
                    sc.table[o] = (int32_t)b.tab;
                    sc.result[o] = res;
                }
                count++;
            }
            // Next on every source whose head is this key
            {
                const uint32_t wtab = (uint32_t)__shfl((int)b.tab, (int)wl);
                const uint32_t went = (uint32_t)__shfl((int)b.ent, (int)wl);
                Head m{{mw[0], mw[1], mw[2], mw[3]}, (uint32_t)__shfl((int)b.klen, (int)wl), wtab, went};
                for (uint32_t r = 0; r < rounds; r++) {
                    const Head x = get(r);
                    if (x.tab == kTsNone || head_cmp(a, x, m) != 0) continue;
                    Head h;
                    place(a, hi, x.tab, x.ent + 1, source_end(S, r * kWave + lane), h);
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

// Sources: one per level-0 table, one per level 1..6.
static uint64_t scan_sources(const SrShape &S) { return (uint64_t)S.start[1] + (kSrLevels - 1); }

// A head per range and source, left by the Seeks for the walk.  A size no
// buffer has when the product leaves 64 bits.
static size_t scan_ws_bytes(const SrShape &S, uint64_t nq) {
    const uint64_t nsrc = scan_sources(S);
    if (nq > (~(uint64_t)0 / kTsHeadBytes) / nsrc) return ~(size_t)0;
    return (size_t)(nq * nsrc * kTsHeadBytes);
}

extern "C" size_t lsm_tree_scan_workspace_bytes(const uint32_t *level_start, uint64_t nq) {
    SrShape S{};
    if (!level_start || !search_shape(level_start, S) || S.start[kSrLevels] == 0) return 0;
    return scan_ws_bytes(S, nq);
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
    if (!ctx) return LSM_EINVAL;
    if (nq == 0) return 0;
    SrShape S{};
    if (!level_start || !search_shape(level_start, S)) return LSM_EINVAL;
    if (limit == 0 || nq >= (1ull << 32) || nq * limit >= (1ull << 32)) return LSM_EINVAL;
    if (scan_sources(S) > 0xFFFFFFFFull) return LSM_EINVAL;
    if (mode != LSM_SCAN_RAW && mode != LSM_SCAN_LIVE) return LSM_EINVAL;
    if (!d_lo || !d_lo_off || !d_hi || !d_hi_off || !d_flags || !d_count || !d_more || !d_key || !d_value ||
        !d_table || !d_result)
        return LSM_EINVAL;
    const uint32_t nfile = S.start[kSrLevels];
    if (nfile && (!d_img || !d_index || !d_file_off || !d_file_len || !d_meta || !d_idx_desc || !d_idx_value))
        return LSM_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GetArgs a = get_args(d_img, d_file_off, d_file_len, d_meta, nfile, d_rec_base, d_idx_desc, d_idx_value);
    if (nfile) {
        const int rc = get_tree_args(a, nfile, d_tree, tree_nidx, tree_bytes);
        if (rc) return rc;
        if (!d_workspace || ws_bytes < scan_ws_bytes(S, nq)) return LSM_ESPACE;
    } else {  // an empty tree: nothing in any range
        LSM_HIP_CHECK(hipMemsetAsync(d_count, 0, 4 * nq, s));
        LSM_HIP_CHECK(hipMemsetAsync(d_more, 0, nq, s));
        return 0;
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
    sc.nsrc = (uint32_t)scan_sources(S);
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
    hipLaunchKernelGGL(tree_scan_seek_kernel, dim3(gs < kTsSeekMaxGrid ? (uint32_t)gs : kTsSeekMaxGrid), dim3(256),
                       0, s, a, files, S, sc);
    LSM_HIP_CHECK(hipGetLastError());
    const uint64_t g = (nq + kTsWaves - 1) / kTsWaves;
    const dim3 grid(g < kTsMaxGrid ? (uint32_t)g : kTsMaxGrid);
    if (sc.rounds > 1)
        hipLaunchKernelGGL(tree_scan_kernel<true>, grid, dim3(kTsThreads), 0, s, a, S, sc);
    else
        hipLaunchKernelGGL(tree_scan_kernel<false>, grid, dim3(kTsThreads), 0, s, a, S, sc);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}
