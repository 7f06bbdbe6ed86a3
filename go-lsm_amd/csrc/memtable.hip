// memtable.hip — the memtable's result on the device (lsm_memtable_order).
//
// A go-lsm memtable is a skiplist in which a later Add of a key replaces the
// earlier pair (memtable/skiplist/skiplist.go:83-118); MemTable.Insert appends
// to the WAL before AddPair (memtable.go:68-78).  Its contents are therefore
// "the last record of each key of its WAL, in key order": a segmented sort
// with last-writer-wins over lsm_wal_replay's descriptors.
//
// Per log: tiles of kTile records are sorted in LDS (bitonic, on each key's
// first 16 bytes; the rest from the log on a tie), log2(tiles) rank-merge
// passes join them over ping-pong buffers of (16 key bytes, slot), and
// the finish keeps the last element of each run of equal keys, applies
// IMemTable.RangeScan's cut and compacts the survivors' slots across logs.
// The order is total -- (key, slot) -- so no pass needs to be stable.  The
// sort itself is mtsort.h's, shared with write.hip.
#include "mtsort.h"

namespace {

using namespace lsm;

constexpr uint32_t kTombBit = 0x80000000u;
constexpr uint64_t kOverflowBit = 1ull << 63;

struct Logs {
    const uint8_t *bytes;
    const lsm_rec_desc *desc;
    const uint64_t *rec_base;  // or NULL: base = log_off[w] / 8
    const uint64_t *log_off;
    const uint32_t *nrec;
    const int32_t *status;
    uint32_t nlog;
    uint32_t nslot;
    uint32_t maxrec;
    // mtsort.h's key source: the records of log w, a slot's key
    __device__ __forceinline__ uint32_t span(uint32_t w, uint32_t *base) const;
    __device__ __forceinline__ Key16 key16(uint32_t slot) const;
    __device__ __forceinline__ int cmp_tail(uint32_t a, uint32_t b) const;
};

// The records of log w this call orders: [*base, *base + n) of desc.  A log
// whose replay failed, or whose records do not fit maxrec / nslot, has none.
__device__ __forceinline__ uint32_t log_span(const Logs &L, uint32_t w, uint32_t *base, bool *overflow) {
    const uint64_t b = L.rec_base ? L.rec_base[w] : L.log_off[w] / 8;
    const uint32_t n = L.nrec[w];
    const bool failed = L.status[w] != 0;
    const bool over = !failed && (n > L.maxrec || b > L.nslot || n > L.nslot - b);
    if (overflow) *overflow = over;
    *base = (uint32_t)b;
    return failed || over ? 0 : n;
}

__device__ __forceinline__ Key16 key16_of(const Logs &L, uint32_t slot) {
    const lsm_rec_desc d = L.desc[slot];
    const uint8_t *key = L.bytes + d.rec_off + 4;
    return Key16{key_word(key, d.key_len, 0), key_word(key, d.key_len, 8)};
}

// Keys a and b (slots) whose first 16 bytes are equal: <0, 0, >0 in Go string order.
__device__ int key_cmp_tail(const Logs &L, uint32_t a, uint32_t b) {
    const lsm_rec_desc da = L.desc[a], db = L.desc[b];
    const uint32_t la = da.key_len, lb = db.key_len;
    const uint32_t lm = la < lb ? la : lb;
    if (lm > 16) {
        const uint8_t *pa = L.bytes + da.rec_off + 4, *pb = L.bytes + db.rec_off + 4;
        for (uint32_t j = 16; j < lm; j += 8) {
            const uint64_t x = key_word(pa, lm, j), y = key_word(pb, lm, j);
            if (x != y) return x < y ? -1 : 1;
        }
    }
    return la == lb ? 0 : (la < lb ? -1 : 1);
}

__device__ __forceinline__ uint32_t Logs::span(uint32_t w, uint32_t *base) const {
    return log_span(*this, w, base, nullptr);
}
__device__ __forceinline__ Key16 Logs::key16(uint32_t slot) const { return key16_of(*this, slot); }
__device__ __forceinline__ int Logs::cmp_tail(uint32_t a, uint32_t b) const { return key_cmp_tail(*this, a, b); }

// kv.DeletedValue (kv/kv.go:29-31), 13 bytes; IsDeleted compares the whole value.
__device__ bool is_tombstone_rec(const uint8_t *bytes, const lsm_rec_desc d) {
    if (d.val_len != 13) return false;
    const uint8_t t[13] = {0xEF, 0xBD, 0x9E, 'D', 'E', 'L', 'E', 'T', 'E', 'D', 0xEF, 0xBD, 0x9E};
    const uint8_t *v = bytes + d.rec_off + 8 + d.key_len;
    bool eq = true;
    for (int i = 0; i < 13; i++) eq &= v[i] == t[i];
    return eq;
}

__device__ bool is_tombstone(const Logs &L, uint32_t slot) { return is_tombstone_rec(L.bytes, L.desc[slot]); }

// ---- finish -----------------------------------------------------------------

// The least of a workgroup's candidate ranks (kPad: none) -> blk[b].  The
// candidates of all workgroups of a log are reduced by mt_min_blocks: one
// atomic per wave on the log's word serialised every wave of the log.
__device__ __forceinline__ void block_min_out(uint32_t cand, uint32_t *s_min, uint32_t *out) {
    if (threadIdx.x == 0) *s_min = kPad;
    __syncthreads();
    const uint64_t any = __ballot(cand != kPad);
    // ranks rise with the lane: the wave's first candidate is its least
    if (any && lane_id() == (uint32_t)__ffsll((long long)any) - 1) atomicMin(s_min, cand);
    __syncthreads();
    if (threadIdx.x == 0) *out = *s_min;
}

// flag[base + i] = 1 when sorted element i is the last of its key (the
// memtable's node), | kTombBit when its value is the tombstone; the
// workgroup's survivor count goes to blkcnt.
__global__ __launch_bounds__(kThreads) void mt_flag(Logs L, const Key16 *key, const uint32_t *pos,
                                                   uint32_t *flag, uint32_t *blkcnt, uint32_t nblk) {
    __shared__ uint32_t s_cnt;
    const uint32_t w = blockIdx.y;
    uint32_t base;
    const uint32_t n = log_span(L, w, &base, nullptr);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t f = 0;
    if (i < n) {
        const uint32_t a = pos[base + i];
        bool last = i + 1 == n;
        if (!last) {
            const uint32_t b = pos[base + i + 1];
            const Key16 ka = key[base + i], kb = key[base + i + 1];
            last = ka.hi != kb.hi || ka.lo != kb.lo || key_cmp_tail(L, a, b) != 0;
        }
        if (last) f = 1 | (is_tombstone(L, a) ? kTombBit : 0);
        flag[base + i] = f;
    }
    const uint64_t bal = __ballot(f != 0);
    if (lane_id() == 0 && bal) atomicAdd(&s_cnt, (uint32_t)__popcll(bal));
    __syncthreads();
    if (threadIdx.x == 0) blkcnt[(size_t)w * nblk + blockIdx.x] = s_cnt;
}

// One wave per log: blkcnt -> exclusive offsets, the log's node count; lead
// and cut start at that count (RangeScan's window [lead, cut) is then empty
// until mt_rank / mt_cut lower them).
__global__ __launch_bounds__(kWave) void mt_scan_blocks(uint32_t *blkcnt, uint32_t nblk, uint32_t *total,
                                                       uint32_t *lead, uint32_t *cut) {
    const uint32_t w = blockIdx.x;
    uint32_t *c = blkcnt + (size_t)w * nblk;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += kWave) {
        const uint32_t b = b0 + lane_id();
        const uint32_t v = b < nblk ? c[b] : 0;
        uint32_t sum;
        const uint32_t ex = wave_excl_scan(v, &sum);
        if (b < nblk) c[b] = carry + ex;
        carry += sum;
    }
    if (lane_id() == 0) {
        total[w] = carry;
        lead[w] = carry;
        cut[w] = carry;
    }
}

// flag -> the node's rank in its log (| kTombBit), kPad for a replaced record;
// RANGESCAN: the workgroup's first node that is no tombstone goes to its
// blkoff word; the least of a log's is lead (SeekToFirst, iterator.go:27-33).
__global__ __launch_bounds__(kThreads) void mt_rank(Logs L, uint32_t *flag, uint32_t *blkoff, uint32_t nblk,
                                                   int scan) {
    __shared__ uint32_t s_wave[kThreads / kWave];
    __shared__ uint32_t s_min;
    const uint32_t w = blockIdx.y;
    uint32_t base;
    const uint32_t n = log_span(L, w, &base, nullptr);
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t f = i < n ? flag[base + i] : 0;
    const uint64_t bal = __ballot(f != 0);
    const uint32_t wv = threadIdx.x / kWave;
    if (lane_id() == 0) s_wave[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = blkoff[(size_t)w * nblk + blockIdx.x];
    for (uint32_t k = 0; k < wv; k++) before += s_wave[k];
    const uint32_t r = before + mbcnt(bal);
    if (i < n) flag[base + i] = f ? r | (f & kTombBit) : kPad;
    if (scan == LSM_MEMTABLE_RANGESCAN)  // the offset was read above: the word now holds the candidate
        block_min_out(f && !(f & kTombBit) ? r : kPad, &s_min, &blkoff[(size_t)w * nblk + blockIdx.x]);
}

// RANGESCAN: the first tombstone past lead ends the scan (Valid,
// iterator.go:68-70, ends the loop of imemtable.go:46-53 there): the
// workgroup's candidate, reduced to cut by mt_min_blocks.
__global__ __launch_bounds__(kThreads) void mt_cut(Logs L, const uint32_t *rank, const uint32_t *lead,
                                                  uint32_t *blk, uint32_t nblk) {
    __shared__ uint32_t s_min;
    const uint32_t w = blockIdx.y;
    uint32_t base;
    const uint32_t n = log_span(L, w, &base, nullptr);
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t f = i < n ? rank[base + i] : kPad;
    const uint32_t r = f & ~kTombBit;
    block_min_out(f != kPad && (f & kTombBit) && r > lead[w] ? r : kPad, &s_min,
                  &blk[(size_t)w * nblk + blockIdx.x]);
}

// One wave per log: dst[w] = the least candidate of the log's workgroups, when
// there is one (dst starts at the log's node count).
__global__ __launch_bounds__(kWave) void mt_min_blocks(const uint32_t *blk, uint32_t nblk, uint32_t *dst) {
    const uint32_t w = blockIdx.x;
    uint32_t m = kPad;
    for (uint32_t b = lane_id(); b < nblk; b += kWave) {
        const uint32_t v = blk[(size_t)w * nblk + b];
        m = v < m ? v : m;
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o);
        m = v < m ? v : m;
    }
    if (lane_id() == 0 && m != kPad) dst[w] = m;
}

// One wave: each log's delivered count -> file_start (exclusive scan) and the
// three counts.  ALL: lead = 0 and cut = the node count.
__global__ __launch_bounds__(kWave) void mt_scan_logs(Logs L, int scan, const uint32_t *total, uint32_t *lead,
                                                     uint32_t *cut, uint64_t *file_start, uint64_t *counts) {
    uint64_t carry = 0;
    uint32_t nonempty = 0, most = 0, over = 0;
    for (uint32_t w0 = 0; w0 < L.nlog; w0 += kWave) {
        const uint32_t w = w0 + lane_id();
        uint64_t v = 0;
        if (w < L.nlog) {
            uint32_t base;
            bool o;
            log_span(L, w, &base, &o);
            over |= o;
            if (scan == LSM_MEMTABLE_ALL) {
                lead[w] = 0;
                cut[w] = total[w];
            }
            v = cut[w] - lead[w];  // lead <= cut <= total
            nonempty += v != 0;
            most = v > most ? (uint32_t)v : most;
        }
        uint64_t sum;
        const uint64_t ex = wave_excl_scan64(v, &sum);
        if (w < L.nlog) file_start[w] = carry + ex;
        carry += sum;
    }
    __shared__ uint32_t s_ne[kWave], s_most[kWave], s_over[kWave];
    s_ne[lane_id()] = nonempty;
    s_most[lane_id()] = most;
    s_over[lane_id()] = over;
    __syncthreads();
    if (lane_id() == 0) {
        uint32_t ne = 0, mo = 0, ov = 0;
        for (int k = 0; k < kWave; k++) {
            ne += s_ne[k];
            mo = s_most[k] > mo ? s_most[k] : mo;
            ov |= s_over[k];
        }
        file_start[L.nlog] = carry;
        counts[0] = carry;
        counts[1] = ne;
        counts[2] = (uint64_t)mo | (ov ? kOverflowBit : 0);
    }
}

__global__ __launch_bounds__(kThreads) void mt_emit(Logs L, const uint32_t *pos, const uint32_t *rank,
                                                   const uint32_t *lead, const uint32_t *cut,
                                                   const uint64_t *file_start, uint32_t *idx) {
    const uint32_t w = blockIdx.y;
    uint32_t base;
    const uint32_t n = log_span(L, w, &base, nullptr);
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = rank[base + i];
    if (f == kPad) return;
    const uint32_t r = f & ~kTombBit, l = lead[w];
    if (r < l || r >= cut[w]) return;
    idx[file_start[w] + (r - l)] = pos[base + i];
}

// ---- search: memtable.Manager.Search over the ordered memtables -------------
//
// SkipList.Search (skiplist.go:60-79) finds the node with exactly the key;
// Manager.Search (memtable/manager.go:61-74) asks Mem, then IMems newest
// first, and the first table that holds the key ends the search, tombstone or
// not.  A memtable here is its log's slice of d_idx (lsm_memtable_order,
// LSM_MEMTABLE_ALL): the nodes in key order, so the skiplist's walk is a
// bisection (its steps are not observable).  One thread per key runs the
// whole of Manager.Search, log nlog - 1 down to 0.  Keys are unique within a
// log, so a three-way compare ends the bisection on the first equal node.
// Without the index a step is three dependent loads (d_idx -> d_desc -> key
// bytes); the index holds each node's Key16 in d_idx order, one 16-byte
// gather per step, the node itself only on a 16-byte tie.
constexpr uint32_t kMsMaxGrid = 2048;  // workgroups: 2,048 resident threads on each of 256 CUs
constexpr size_t kMsHeader = 256;      // the index's header: {nodes indexed}, padded to 256 bytes

struct MsArgs {
    const uint8_t *bytes;
    const lsm_rec_desc *desc;
    const uint32_t *idx;
    const uint64_t *file_start;
    uint32_t nlog;
    const uint64_t *index_hdr;  // or NULL: no index
    const Key16 *index;
    uint64_t index_cap;  // nodes the index buffer has room for
    const uint8_t *keys;
    const uint64_t *koff;
    uint64_t nkeys;
    int32_t *mem_result, *log;
    uint32_t *slot;
    lsm_rec_desc *value;
};

__global__ __launch_bounds__(kThreads) void mt_search(MsArgs a) {
    // the nodes the index vouches for: those its build wrote, within the buffer
    uint64_t nindexed = 0;
    if (a.index_hdr) {
        nindexed = a.index_hdr[0];
        nindexed = nindexed < a.index_cap ? nindexed : a.index_cap;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < a.nkeys;
         i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t k0 = a.koff[i], kl64 = a.koff[i + 1] - k0;
        int32_t res = LSM_MEM_MISS, lg = -1;
        uint32_t sl = kPad;
        lsm_rec_desc v{0, 0, 0};
        // a node's key is at most kKeyCap bytes (kv.go:84): a longer probe equals none
        if (kl64 <= kKeyCap) {
            const uint32_t kl = (uint32_t)kl64;
            const uint8_t *kp = a.keys + k0;
            const Key16 pk{key_word(kp, kl, 0), key_word(kp, kl, 8)};
            for (uint32_t w = a.nlog; w-- > 0 && res == LSM_MEM_MISS;) {
                uint64_t lo = a.file_start[w], hi = a.file_start[w + 1];
                const bool indexed = hi <= nindexed;
                while (lo < hi) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    uint32_t s = kPad;
                    lsm_rec_desc d{0, 0, 0};
                    Key16 nk;
                    if (indexed) {
                        nk = a.index[mid];
                    } else {
                        s = a.idx[mid];
                        d = a.desc[s];
                        const uint8_t *np = a.bytes + d.rec_off + 4;
                        nk = Key16{key_word(np, d.key_len, 0), key_word(np, d.key_len, 8)};
                    }
                    int c;
                    if (nk.hi != pk.hi) c = nk.hi < pk.hi ? -1 : 1;
                    else if (nk.lo != pk.lo) c = nk.lo < pk.lo ? -1 : 1;
                    else {
                        if (indexed) {
                            s = a.idx[mid];
                            d = a.desc[s];
                        }
                        c = key_cmp_tail_at(a.bytes + d.rec_off + 4, d.key_len, kp, kl);
                    }
                    if (c == 0) {  // (value, true), or (nil, true) for a tombstone: the search ends
                        lg = (int32_t)w;
                        sl = s;
                        if (is_tombstone_rec(a.bytes, d)) {
                            res = LSM_MEM_DELETED;
                        } else {
                            res = LSM_MEM_VALUE;
                            v = lsm_rec_desc{d.rec_off + 4 + d.key_len, 0, d.val_len};
                        }
                        break;
                    }
                    if (c < 0) lo = mid + 1;
                    else hi = mid;
                }
            }
        }
        a.mem_result[i] = res;
        a.log[i] = lg;
        a.slot[i] = sl;
        a.value[i] = v;
    }
}

// index[p] = the Key16 of node d_idx[p], p < d_file_start[nlog] (read here)
// and < cap; the header records how many were written.
__global__ __launch_bounds__(kThreads) void mt_index_build(const uint8_t *bytes, const lsm_rec_desc *desc,
                                                          const uint32_t *idx, const uint64_t *file_start,
                                                          uint32_t nlog, uint64_t cap, uint64_t *hdr,
                                                          Key16 *index) {
    uint64_t n = file_start[nlog];
    n = n < cap ? n : cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[0] = n;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (uint64_t)gridDim.x * kThreads) {
        const lsm_rec_desc d = desc[idx[p]];
        const uint8_t *key = bytes + d.rec_off + 4;
        index[p] = Key16{key_word(key, d.key_len, 0), key_word(key, d.key_len, 8)};
    }
}

struct Ws {
    Key16 *key[2];
    uint32_t *pos[2];
    uint32_t *blkcnt, *total, *lead, *cut;
};

uint32_t blocks_per_log(uint32_t maxrec) { return (maxrec + kThreads - 1) / kThreads; }

Ws ws_layout(WsCursor &c, uint32_t nlog, uint64_t nslot, uint32_t maxrec) {
    Ws w;
    for (int i = 0; i < 2; i++) w.key[i] = c.take<Key16>(nslot);
    for (int i = 0; i < 2; i++) w.pos[i] = c.take<uint32_t>(nslot);
    w.blkcnt = c.take<uint32_t>((size_t)nlog * blocks_per_log(maxrec));
    w.total = c.take<uint32_t>(nlog);
    w.lead = c.take<uint32_t>(nlog);
    w.cut = c.take<uint32_t>(nlog);
    return w;
}

}  // namespace

extern "C" size_t lsm_memtable_order_workspace_bytes(uint32_t nlog, uint64_t nslot,
                                                     uint32_t max_log_records) {
    if (nlog == 0) return 0;
    WsCursor c{nullptr, 0};
    ws_layout(c, nlog, nslot, max_log_records);
    return c.at;
}

extern "C" int lsm_memtable_order(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc,
                                  const uint64_t *d_rec_base, const uint64_t *d_log_off,
                                  const uint32_t *d_nrec, const int32_t *d_status, uint32_t nlog,
                                  uint64_t nslot, uint32_t max_log_records, int scan, uint32_t *d_idx,
                                  uint64_t *d_file_start, uint64_t *d_counts, void *d_ws,
                                  size_t ws_bytes, void *stream) {
    if (!ctx || (scan != LSM_MEMTABLE_ALL && scan != LSM_MEMTABLE_RANGESCAN)) return LSM_EINVAL;
    if (nlog == 0) return 0;
    // slots are u32 indices (d_idx); a rank keeps its top bit for the tombstone
    if (nslot >= 0xFFFFFFFFull || max_log_records >= 0x80000000u || nlog > 65535) return LSM_EINVAL;
    if (!d_nrec || !d_status || !d_file_start || !d_counts || (!d_rec_base && !d_log_off))
        return LSM_EINVAL;
    if (nslot && max_log_records && (!d_bytes || !d_desc || !d_idx)) return LSM_EINVAL;
    if (!d_ws || ws_bytes < lsm_memtable_order_workspace_bytes(nlog, nslot, max_log_records))
        return LSM_ESPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsCursor c{static_cast<uint8_t *>(d_ws), 0};
    const Ws ws = ws_layout(c, nlog, nslot, max_log_records);
    // with no slot or no admitted record every log is empty (or overflows)
    const Logs L{d_bytes, d_desc, d_rec_base, d_log_off, d_nrec, d_status, nlog, (uint32_t)nslot,
                 nslot ? max_log_records : 0};
    const uint32_t nblk = blocks_per_log(max_log_records);
    const int cur = mt_sort_segments(L, nlog, L.maxrec, ws.key, ws.pos, s);
    uint32_t *flag = ws.pos[cur ^ 1];  // the idle index buffer: flags, then ranks
    if (nblk)
        hipLaunchKernelGGL(mt_flag, dim3(nblk, nlog), dim3(kThreads), 0, s, L, ws.key[cur], ws.pos[cur], flag,
                           ws.blkcnt, nblk);
    hipLaunchKernelGGL(mt_scan_blocks, dim3(nlog), dim3(kWave), 0, s, ws.blkcnt, nblk, ws.total, ws.lead,
                       ws.cut);
    if (nblk) {
        hipLaunchKernelGGL(mt_rank, dim3(nblk, nlog), dim3(kThreads), 0, s, L, flag, ws.blkcnt, nblk, scan);
        if (scan == LSM_MEMTABLE_RANGESCAN) {
            hipLaunchKernelGGL(mt_min_blocks, dim3(nlog), dim3(kWave), 0, s, ws.blkcnt, nblk, ws.lead);
            hipLaunchKernelGGL(mt_cut, dim3(nblk, nlog), dim3(kThreads), 0, s, L, flag, ws.lead, ws.blkcnt, nblk);
            hipLaunchKernelGGL(mt_min_blocks, dim3(nlog), dim3(kWave), 0, s, ws.blkcnt, nblk, ws.cut);
        }
    }
    hipLaunchKernelGGL(mt_scan_logs, dim3(1), dim3(kWave), 0, s, L, scan, ws.total, ws.lead, ws.cut,
                       d_file_start, d_counts);
    if (nblk)
        hipLaunchKernelGGL(mt_emit, dim3(nblk, nlog), dim3(kThreads), 0, s, L, ws.pos[cur], flag, ws.lead,
                           ws.cut, d_file_start, d_idx);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" size_t lsm_memtable_search_index_bytes(uint64_t nnode_max) {
    return nnode_max ? kMsHeader + sizeof(Key16) * (size_t)nnode_max : 0;
}

extern "C" int lsm_memtable_search_index_build(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc,
                                               const uint32_t *d_idx, const uint64_t *d_file_start,
                                               uint32_t nlog, uint64_t nnode_max, void *d_index,
                                               size_t index_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nlog == 0 || nnode_max == 0) return 0;
    if (nlog > 65535 || nnode_max >= 0xFFFFFFFFull || !d_bytes || !d_desc || !d_idx || !d_file_start)
        return LSM_EINVAL;
    if (!d_index || index_bytes < lsm_memtable_search_index_bytes(nnode_max)) return LSM_ESPACE;
    uint8_t *p = static_cast<uint8_t *>(d_index);
    const uint64_t g = (nnode_max + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(mt_index_build, dim3(g < kMsMaxGrid ? (uint32_t)g : kMsMaxGrid), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_bytes, d_desc, d_idx, d_file_start, nlog, nnode_max,
                       reinterpret_cast<uint64_t *>(p), reinterpret_cast<Key16 *>(p + kMsHeader));
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int lsm_memtable_search(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc,
                                   const uint32_t *d_idx, const uint64_t *d_file_start, uint32_t nlog,
                                   const void *d_index, size_t index_bytes, const uint8_t *d_keys,
                                   const uint64_t *d_koff, uint64_t nkeys, int32_t *d_mem_result,
                                   int32_t *d_log, uint32_t *d_slot, lsm_rec_desc *d_value, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (nkeys == 0) return 0;
    if (nlog > 65535 || !d_keys || !d_koff || !d_mem_result || !d_log || !d_slot || !d_value)
        return LSM_EINVAL;
    if (nlog && (!d_bytes || !d_desc || !d_idx || !d_file_start)) return LSM_EINVAL;
    if (d_index && index_bytes < lsm_memtable_search_index_bytes(1)) return LSM_ESPACE;
    MsArgs a{};
    a.bytes = d_bytes;
    a.desc = d_desc;
    a.idx = d_idx;
    a.file_start = d_file_start;
    a.nlog = nlog;
    if (d_index && nlog) {
        const uint8_t *p = static_cast<const uint8_t *>(d_index);
        a.index_hdr = reinterpret_cast<const uint64_t *>(p);
        a.index = reinterpret_cast<const Key16 *>(p + kMsHeader);
        a.index_cap = (index_bytes - kMsHeader) / sizeof(Key16);
    }
    a.keys = d_keys;
    a.koff = d_koff;
    a.nkeys = nkeys;
    a.mem_result = d_mem_result;
    a.log = d_log;
    a.slot = d_slot;
    a.value = d_value;
    const uint64_t g = (nkeys + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(mt_search, dim3(g < kMsMaxGrid ? (uint32_t)g : kMsMaxGrid), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}
