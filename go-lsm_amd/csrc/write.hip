// write.hip — database.Put / database.Delete for a batch (lsm_db_write): the
// write-ahead logs go-lsm appends, with memtable rotation, and the descriptors
// lsm_wal_replay would return for them ("The write side").
//
// Manager.Insert / Delete (memtable/manager.go:40-106) walk a batch serially:
// CanInsert against sizeInBytes, promoteLocked, MemTable.Delete's conditional
// (key, nil) record, then wal.Append of KeyValuePair.EncodeTo.  In closed form
// (e[i] = 16 + len(key) + len(value), a Delete's value the 13 tombstone bytes):
//   rotation   op i starts a new log exactly when size + e[i] > mem_max, size
//              the sum of e since the log's first op (+ mem_size0 in log 0);
//   the extra  Delete i also appends (key, "") to L(i), the log current before
//              it, when an earlier op of L(i) has its key (or, for log 0, a
//              node passed in has it), immediately before its own position;
//   the bytes  per log, in op order, [extra][main], u32 klen | key | u32 vlen |
//              value.
// Passes: scan of e; each op's next log start (a bisection of the scan) and
// the chase through them; each op's log; per log the ops sorted by (key,
// position) with mtsort.h, the Deletes' presence from the sorted neighbour,
// the previous log or the nodes; scan of (bytes, records) per op; per-log
// offsets; the emit.
#include "mtsort.h"
#include "scan.h"

namespace {

using namespace lsm;

constexpr uint32_t kTombLen = 13;  // kv.DeletedValue (kv/kv.go:29-31)
__device__ const uint8_t kTomb[16] = {0xEF, 0xBD, 0x9E, 'D', 'E', 'L', 'E', 'T', 'E', 'D', 0xEF, 0xBD, 0x9E};

struct Batch {
    const uint8_t *keys;
    const uint64_t *koff;
    const uint8_t *vals;
    const uint64_t *voff;
    const uint8_t *op;
    uint32_t n;
};

__device__ __forceinline__ uint32_t klen_of(const Batch &b, uint32_t i) {
    return (uint32_t)(b.koff[i + 1] - b.koff[i]);
}
// the main record's value length: a Delete's CSR value is ignored
__device__ __forceinline__ uint32_t vlen_of(const Batch &b, uint32_t i) {
    return b.op[i] ? kTombLen : (uint32_t)(b.voff[i + 1] - b.voff[i]);
}
// KeyValuePair.EstimateSize (kv.go:118-121) of op i's main pair
__device__ __forceinline__ uint64_t est_of(const Batch &b, uint32_t i) {
    return 16ull + klen_of(b, i) + vlen_of(b, i);
}

// The current memtable's nodes, in key order.
struct Nodes {
    const uint8_t *bytes;
    const lsm_rec_desc *desc;
    const uint32_t *idx;
    uint64_t n;
};

// The rotation's result, kept in the workspace: hdr[0] = nlog, 0 after an
// overflow, so that every later kernel finds nothing to do.
struct Rot {
    const uint32_t *hdr;
    const uint32_t *ls;  // log w = ops [ls[w], ls[w + 1])
};

// mtsort.h's key source: the ops of log w, an op's key.
struct OpKeys {
    Batch b;
    Rot r;
    __device__ __forceinline__ uint32_t span(uint32_t w, uint32_t *base) const {
        if (w >= r.hdr[0]) return 0;
        *base = r.ls[w];
        return r.ls[w + 1] - r.ls[w];
    }
    __device__ __forceinline__ Key16 key16(uint32_t i) const {
        const uint8_t *k = b.keys + b.koff[i];
        const uint32_t kl = klen_of(b, i);
        return Key16{key_word(k, kl, 0), key_word(k, kl, 8)};
    }
    __device__ __forceinline__ int cmp_tail(uint32_t x, uint32_t y) const {
        return key_cmp_tail_at(b.keys + b.koff[x], klen_of(b, x), b.keys + b.koff[y], klen_of(b, y));
    }
};

// ---- scans over the ops (scan.h's three launches) ---------------------------

template <class T, class F>
__device__ __forceinline__ void tile_sum(F f, uint32_t n, T *partial) {
    T v{};
    for (uint32_t k = 0; k < kScanPer; k++) {
        const uint64_t i = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanPer + k;
        if (i < n) v = v + f((uint32_t)i);
    }
    T tot;
    wg_excl_scan<kScanThreads>(v, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <class T, class F>
__device__ __forceinline__ void tile_scan(F f, uint32_t n, const T *partial, T *out) {
    T v[kScanPer], s{};
    for (uint32_t k = 0; k < kScanPer; k++) {
        const uint64_t i = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanPer + k;
        v[k] = i < n ? f((uint32_t)i) : T{};
        s = s + v[k];
    }
    T tot;
    T pre = wg_excl_scan<kScanThreads>(s, &tot) + partial[blockIdx.x];
    for (uint32_t k = 0; k < kScanPer; k++) {
        const uint64_t i = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanPer + k;
        if (i < n) out[i] = pre;
        pre = pre + v[k];
    }
}

__global__ __launch_bounds__(kScanThreads) void wr_est_sum(Batch b, uint64_t *partial) {
    tile_sum<uint64_t>([&](uint32_t i) { return est_of(b, i); }, b.n, partial);
}
__global__ __launch_bounds__(kScanThreads) void wr_est_scan(Batch b, const uint64_t *partial, uint64_t *E) {
    tile_scan<uint64_t>([&](uint32_t i) { return est_of(b, i); }, b.n, partial, E);
}

// (bytes, records) op i appends: its main record, and a Delete's (key, "").
__device__ __forceinline__ Sum2 stream_of(const Batch &b, const uint8_t *extra, uint32_t i) {
    const uint32_t kl = klen_of(b, i), ex = extra[i];
    return Sum2{8ull + kl + vlen_of(b, i) + (ex ? 8ull + kl : 0), 1ull + ex};
}
__global__ __launch_bounds__(kScanThreads) void wr_stream_sum(Batch b, Rot r, const uint8_t *extra, Sum2 *partial) {
    if (r.hdr[0] == 0) return;
    tile_sum<Sum2>([&](uint32_t i) { return stream_of(b, extra, i); }, b.n, partial);
}
__global__ __launch_bounds__(kScanThreads) void wr_stream_scan(Batch b, Rot r, const uint8_t *extra,
                                                              const Sum2 *partial, Sum2 *X) {
    if (r.hdr[0] == 0) return;
    tile_scan<Sum2>([&](uint32_t i) { return stream_of(b, extra, i); }, b.n, partial, X);
}

// ---- rotation ---------------------------------------------------------------

// next[i] = the op that opens the next log when a log opens at op i: the log
// holds op i however large, then every op j while E[j + 1] - E[i] <= mem_max.
__global__ __launch_bounds__(kThreads) void wr_next(uint32_t n, const uint64_t *E, uint64_t mem_max,
                                                   uint32_t *next) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    const uint64_t lim = E[i] + mem_max;
    uint32_t lo = i + 1, hi = n;  // the first b > i with E[b + 1] > lim, or n
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (E[mid + 1] > lim) hi = mid;
        else lo = mid + 1;
    }
    next[i] = lo;
}

// The chase: log 0 = the ops that fit beside mem_size0 (none when op 0 does
// not), then from log start to log start through next[].  One dependent load
// per log: serial as in the reference, but over logs, not ops.
__global__ __launch_bounds__(kWave) void wr_chase(uint32_t n, const uint64_t *E, const uint32_t *next,
                                                 uint64_t mem_size0, uint64_t mem_max, uint32_t nlog_max,
                                                 uint32_t *ls, uint32_t *hdr, uint64_t *counts) {
    if (threadIdx.x != 0) return;
    uint32_t a = 0;
    if (mem_size0 <= mem_max) {
        const uint64_t lim = mem_max - mem_size0;
        uint32_t lo = 0, hi = n;  // the first b with E[b + 1] > lim, or n
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (E[mid + 1] > lim) hi = mid;
            else lo = mid + 1;
        }
        a = lo;
    }
    ls[0] = 0;
    uint32_t nlog = 1;
    bool over = false;
    while (a < n) {
        if (nlog == nlog_max) {
            over = true;
            break;
        }
        ls[nlog++] = a;
        a = next[a];
    }
    if (over) {
        hdr[0] = 0;
        for (int k = 0; k < 6; k++) counts[k] = k == 3;
        return;
    }
    ls[nlog] = n;
    hdr[0] = nlog;
}

// seg[i] = op i's log: the last w with ls[w] <= i (an empty log 0 shares its
// start with log 1).
__global__ __launch_bounds__(kThreads) void wr_seg(uint32_t n, Rot r, uint32_t *seg) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t nlog = r.hdr[0];
    if (i >= n || nlog == 0) return;
    uint32_t lo = 0, hi = nlog;  // the first w with ls[w] > i
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r.ls[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    seg[i] = lo - 1;
}

// ---- presence -----------------------------------------------------------------

// Is the key (kp, kl, its first 16 bytes k) one of the nodes?  mt_search's compare.
__device__ bool in_nodes(const Nodes &c, const uint8_t *kp, uint32_t kl, Key16 k) {
    uint64_t lo = 0, hi = c.n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const lsm_rec_desc d = c.desc[c.idx[mid]];
        const uint8_t *np = c.bytes + d.rec_off + 4;
        const Key16 nk{key_word(np, d.key_len, 0), key_word(np, d.key_len, 8)};
        int cmp;
        if (nk.hi != k.hi) cmp = nk.hi < k.hi ? -1 : 1;
        else if (nk.lo != k.lo) cmp = nk.lo < k.lo ? -1 : 1;
        else cmp = key_cmp_tail_at(np, d.key_len, kp, kl);
        if (cmp == 0) return true;
        if (cmp < 0) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// extra[i] = 1 when Delete i appends (key, "") to L(i), the log current before
// it.  One thread per sorted element p of log w (op i = pos[base + p]):
//   i does not open its log: L(i) = w, and an earlier op of w has the key
//     exactly when the sorted predecessor carries it ((key, position) order);
//   i opens log w > 0: L(i) = w - 1, whose sorted ops are bisected;
//   no hit and L(i) = 0: the nodes of the memtable passed in.
__global__ __launch_bounds__(kThreads) void wr_presence(OpKeys S, Nodes cur, const Key16 *key,
                                                       const uint32_t *pos, uint8_t *extra) {
    const uint32_t w = blockIdx.y;
    uint32_t base = 0;
    const uint32_t n = S.span(w, &base);
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = pos[base + p];
    bool ex = false;
    if (S.b.op[i]) {
        const Key16 k = key[base + p];
        uint32_t L = w;
        if (i != base) {
            if (p > 0) {
                const Key16 kj = key[base + p - 1];
                ex = kj.hi == k.hi && kj.lo == k.lo && S.cmp_tail(pos[base + p - 1], i) == 0;
            }
        } else if (w > 0) {
            L = w - 1;
            const uint32_t b0 = S.r.ls[L];
            uint32_t lo = 0, hi = base - b0;
            while (lo < hi && !ex) {
                const uint32_t mid = (lo + hi) >> 1;
                const Key16 kb = key[b0 + mid];
                int c;
                if (kb.hi != k.hi) c = kb.hi < k.hi ? -1 : 1;
                else if (kb.lo != k.lo) c = kb.lo < k.lo ? -1 : 1;
                else c = S.cmp_tail(pos[b0 + mid], i);
                ex = c == 0;
                if (c < 0) lo = mid + 1;
                else hi = mid;
            }
        }
        if (!ex && L == 0 && cur.n) ex = in_nodes(cur, S.b.keys + S.b.koff[i], klen_of(S.b, i), k);
    }
    extra[i] = ex;
}

// ---- layout ---------------------------------------------------------------------

struct Out {
    uint8_t *wal;
    uint64_t *log_start, *wal_off;
    uint32_t *wal_len;
    lsm_rec_desc *desc;  // or NULL
    uint64_t *rec_base;
    uint32_t *main_slot;  // or NULL
    uint64_t *counts;
};

// The stream position (bytes, records) at which log w starts: before op
// ls[w]'s main record, after its (key, "") -- that one closes log w - 1.
__device__ __forceinline__ Sum2 log_stream_start(const Batch &b, const Rot &r, const uint8_t *extra,
                                                 const Sum2 *X, uint32_t w, uint32_t nlog) {
    if (w == 0) return Sum2{0, 0};
    if (w == nlog) return X[b.n];
    const uint32_t i = r.ls[w];
    Sum2 s = X[i];
    if (extra[i]) s = s + Sum2{8ull + klen_of(b, i), 1};
    return s;
}

// One wave: per log its stream start, length, record base and aligned offset;
// the counts.
__global__ __launch_bounds__(kWave) void wr_logs(Batch b, Rot r, const uint8_t *extra, const Sum2 *X,
                                                const uint64_t *E, uint64_t mem_size0, uint32_t align,
                                                Sum2 *logS, Out o) {
    const uint32_t nlog = r.hdr[0];
    if (nlog == 0) return;
    uint64_t carry = 0, most = 0;
    for (uint32_t w0 = 0; w0 < nlog; w0 += kWave) {
        const uint32_t w = w0 + lane_id();
        uint64_t rounded = 0;
        if (w < nlog) {
            const Sum2 s0 = log_stream_start(b, r, extra, X, w, nlog);
            const Sum2 s1 = log_stream_start(b, r, extra, X, w + 1, nlog);
            const uint64_t len = s1.s - s0.s, nrec = s1.c - s0.c;
            logS[w] = s0;
            o.wal_len[w] = (uint32_t)len;
            o.rec_base[w] = s0.c;
            o.log_start[w] = r.ls[w];
            rounded = (len + align - 1) / align * align;
            most = nrec > most ? nrec : most;
        }
        uint64_t sum;
        const uint64_t ex = wave_excl_scan64(rounded, &sum);
        if (w < nlog) o.wal_off[w] = carry + ex;
        carry += sum;
    }
    most = wave_max64(most);
    if (lane_id() == 0) {
        const Sum2 tot = X[b.n];
        o.wal_off[nlog] = carry;
        o.rec_base[nlog] = tot.c;
        o.log_start[nlog] = b.n;
        o.counts[0] = nlog;
        o.counts[1] = tot.c;
        o.counts[2] = carry;
        o.counts[3] = 0;
        o.counts[4] = most;
        o.counts[5] = E[b.n] - E[r.ls[nlog - 1]] + (nlog == 1 ? mem_size0 : 0);
    }
}

// ---- emit -----------------------------------------------------------------------

// One wave per 64 ops.  The ops' records (up to 128) go to a table in LDS:
// destination, lengths, source addresses, log.  Records of one log are
// contiguous in d_wal, so each run of one log is written as 16-byte aligned
// units, a lane per unit: the lane finds its first record by bisection of the
// table, then walks the unit's 16 bytes through the records (length fields
// from registers, key and value bytes from the arenas, the tombstone from a
// constant), and stores the unit with one 16-byte store; a unit cut by the
// run's first or last byte is stored by bytes.
constexpr uint32_t kEmitOps = kWave;
constexpr uint32_t kEmitRecs = 2 * kEmitOps;

__global__ __launch_bounds__(kWave) void wr_emit(Batch b, Rot r, const uint32_t *seg, const uint8_t *extra,
                                                const Sum2 *X, const Sum2 *logS, Out o) {
    __shared__ uint64_t t_dst[kEmitRecs], t_ks[kEmitRecs], t_vs[kEmitRecs];
    __shared__ uint32_t t_kl[kEmitRecs], t_vl[kEmitRecs], t_log[kEmitRecs];
    if (r.hdr[0] == 0) return;
    const uint64_t i0 = (uint64_t)blockIdx.x * kEmitOps;
    const uint32_t i = (uint32_t)i0 + lane_id();
    const uint32_t iend = i0 + kEmitOps < b.n ? (uint32_t)i0 + kEmitOps : b.n;
    const uint64_t c0 = X[i0].c;
    const uint32_t nrec = (uint32_t)(X[iend].c - c0);
    if (i < b.n) {
        const uint32_t w = seg[i], ex = extra[i];
        const uint32_t kl = klen_of(b, i), vl = vlen_of(b, i);
        const Sum2 x = X[i];
        const uint64_t ks = reinterpret_cast<uintptr_t>(b.keys + b.koff[i]);
        const uint64_t vs = b.op[i] ? reinterpret_cast<uintptr_t>(kTomb)
                                    : reinterpret_cast<uintptr_t>(b.vals + b.voff[i]);
        uint32_t c = (uint32_t)(x.c - c0);
        uint64_t at = x.s;
        if (ex) {  // (key, ""): in the log current before op i
            const uint32_t L = (w > 0 && i == r.ls[w]) ? w - 1 : w;
            const uint64_t dst = o.wal_off[L] + (at - logS[L].s);
            t_dst[c] = dst;
            t_ks[c] = ks;
            t_vs[c] = vs;
            t_kl[c] = kl;
            t_vl[c] = 0;
            t_log[c] = L;
            if (o.desc) o.desc[x.c] = lsm_rec_desc{dst, kl, 0};
            c++;
            at += 8ull + kl;
        }
        const uint64_t dst = o.wal_off[w] + (at - logS[w].s);
        t_dst[c] = dst;
        t_ks[c] = ks;
        t_vs[c] = vs;
        t_kl[c] = kl;
        t_vl[c] = vl;
        t_log[c] = w;
        if (o.desc) o.desc[x.c + ex] = lsm_rec_desc{dst, kl, vl};
        if (o.main_slot) o.main_slot[i] = (uint32_t)(x.c + ex);
    }
    __syncthreads();
    // the runs: a record starts one when its log differs from its predecessor's
    const uint32_t ca = lane_id(), cb = lane_id() + kWave;
    const uint64_t m0 = __ballot(ca < nrec && (ca == 0 || t_log[ca] != t_log[ca - 1]));
    const uint64_t m1 = __ballot(cb < nrec && t_log[cb] != t_log[cb - 1]);
    const uintptr_t wal0 = reinterpret_cast<uintptr_t>(o.wal);
    const uint64_t tomb = reinterpret_cast<uintptr_t>(kTomb);
    uint32_t cs = 0;
    while (cs < nrec) {
        // the next run start after cs, or nrec
        uint32_t ce = nrec;
        {
            const uint32_t from = cs + 1;
            const uint64_t r0 = from < 64 ? m0 >> from << from : 0;
            const uint64_t r1 = from < 64 ? m1 : (from < 128 ? m1 >> (from - 64) << (from - 64) : 0);
            if (r0) ce = (uint32_t)__ffsll((long long)r0) - 1;
            else if (r1) ce = 64 + (uint32_t)__ffsll((long long)r1) - 1;
        }
        const uint64_t A = wal0 + t_dst[cs];
        const uint64_t B = wal0 + t_dst[ce - 1] + 8 + t_kl[ce - 1] + t_vl[ce - 1];
        for (uint64_t U = (A & ~15ull) + 16ull * lane_id(); U < B; U += 16ull * kWave) {
            const uint64_t q0 = U > A ? U : A;
            uint32_t lo = cs, hi = ce - 1;  // the last record with dst <= q0
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (wal0 + t_dst[mid] <= q0) lo = mid;
                else hi = mid - 1;
            }
            uint32_t c = lo;
            uint64_t rd = wal0 + t_dst[c], ks = t_ks[c], vs = t_vs[c];
            uint32_t kl = t_kl[c], vl = t_vl[c];
            uint64_t addr[16];
            uint32_t imm[16];
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) {
                const uint64_t q = U + k;
                addr[k] = tomb;
                imm[k] = 0x100;  // >= 0x100: the byte comes from memory
                if (q < A || q >= B) continue;
                while (q >= rd + 8 + kl + vl && c + 1 < ce) {  // the next record (q < B: there is one)
                    c++;
                    rd = wal0 + t_dst[c];
                    ks = t_ks[c];
                    vs = t_vs[c];
                    kl = t_kl[c];
                    vl = t_vl[c];
                }
                const uint64_t off = q - rd;
                if (off < 4) imm[k] = (kl >> (8 * (uint32_t)off)) & 0xFF;
                else if (off < 4ull + kl) addr[k] = ks + (off - 4);
                else if (off < 8ull + kl) imm[k] = (vl >> (8 * (uint32_t)(off - 4 - kl))) & 0xFF;
                else addr[k] = vs + (off - 8 - kl);
            }
            uint32_t by[16];
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) by[k] = *gbl_at<const uint8_t>(addr[k]);
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) by[k] = imm[k] < 0x100 ? imm[k] : by[k];
            if (U >= A && U + 16 <= B) {
                u32x4 v;
                v.x = by[0] | by[1] << 8 | by[2] << 16 | by[3] << 24;
                v.y = by[4] | by[5] << 8 | by[6] << 16 | by[7] << 24;
                v.z = by[8] | by[9] << 8 | by[10] << 16 | by[11] << 24;
                v.w = by[12] | by[13] << 8 | by[14] << 16 | by[15] << 24;
                *gbl_at<u32x4>(U) = v;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 16; k++)
                    if (U + k >= A && U + k < B) *gbl_at<uint8_t>(U + k) = (uint8_t)by[k];
            }
        }
        cs = ce;
    }
}

struct Ws {
    uint64_t *E, *epart;
    uint32_t *next, *seg, *ls, *hdr;
    Key16 *key[2];
    uint32_t *pos[2];
    uint8_t *extra;
    Sum2 *X, *xpart, *logS;
};

uint32_t scan_tiles(uint64_t n) { return (uint32_t)((n + kScanTile - 1) / kScanTile); }

Ws ws_layout(WsCursor &c, uint64_t n, uint32_t nlog_max) {
    Ws w;
    w.E = c.take<uint64_t>(n + 1);
    w.epart = c.take<uint64_t>(scan_tiles(n));
    w.next = c.take<uint32_t>(n);
    w.seg = c.take<uint32_t>(n);
    w.ls = c.take<uint32_t>((size_t)nlog_max + 1);
    w.hdr = c.take<uint32_t>(1);
    for (int i = 0; i < 2; i++) w.key[i] = c.take<Key16>(n);
    for (int i = 0; i < 2; i++) w.pos[i] = c.take<uint32_t>(n);
    w.extra = c.take<uint8_t>(n);
    w.X = c.take<Sum2>(n + 1);
    w.xpart = c.take<Sum2>(scan_tiles(n));
    w.logS = c.take<Sum2>((size_t)nlog_max + 1);
    return w;
}

// The most ops one log can hold: est >= 16 each and their sum <= mem_max, or
// the one op a log always holds.
uint32_t max_log_ops(uint64_t n, uint64_t mem_max) {
    const uint64_t m = mem_max / 16 > 1 ? mem_max / 16 : 1;
    return (uint32_t)(m < n ? m : n);
}

}  // namespace

// Two consecutive logs hold est sums (mem_size0 counted in log 0) of more than
// mem_max together: the later one was opened because its first op did not fit
// beside the earlier one's sum, and it holds that op.  So floor(T / (mem_max
// + 1)) bounds the disjoint pairs, T = mem_size0 + the sum of est <=
// mem_size0 + 29 n + key_bytes + val_bytes (a Delete's value is 13 bytes
// whatever its CSR range holds); one more log may be left over.
extern "C" uint32_t lsm_db_write_max_logs(uint64_t n, uint64_t key_bytes, uint64_t val_bytes,
                                          uint64_t mem_size0, uint64_t mem_max) {
    if (n == 0) return 1;
    const uint64_t T = mem_size0 + 29 * n + key_bytes + val_bytes;
    uint64_t bound = 2 * (T / (mem_max + 1)) + 2;
    if (bound > n + 1) bound = n + 1;  // log 0 and a log per op
    return bound > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bound;
}

// Every op a Delete with its (key, ""): 2 (8 + klen) + 13; a Put: 8 + klen +
// vlen; each log rounded up to align.
extern "C" uint64_t lsm_db_write_out_bytes(uint64_t n, uint64_t key_bytes, uint64_t val_bytes,
                                           uint32_t nlog_max, uint32_t align) {
    if (n == 0) return 0;
    const uint64_t pad = align ? align - 1 : 0;
    return 29 * n + 2 * key_bytes + val_bytes + (uint64_t)nlog_max * pad;
}

extern "C" size_t lsm_db_write_workspace_bytes(uint64_t n, uint32_t nlog_max, uint64_t mem_max) {
    (void)mem_max;  // a log's op bound sizes grids, not buffers
    if (n == 0) return 0;
    WsCursor c{nullptr, 0};
    ws_layout(c, n, nlog_max);
    return c.at;
}

extern "C" int lsm_db_write(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff, const uint8_t *d_vals,
                            const uint64_t *d_voff, const uint8_t *d_op, uint64_t n, uint64_t mem_size0,
                            uint64_t mem_max, const uint8_t *d_cur_bytes, const lsm_rec_desc *d_cur_desc,
                            const uint32_t *d_cur_idx, uint64_t cur_nnode, uint32_t nlog_max, uint32_t align,
                            uint8_t *d_wal, uint64_t *d_log_start, uint64_t *d_wal_off, uint32_t *d_wal_len,
                            lsm_rec_desc *d_desc, uint64_t *d_rec_base, uint32_t *d_main_slot,
                            uint64_t *d_counts, void *d_ws, size_t ws_bytes, void *stream) {
    if (!ctx) return LSM_EINVAL;
    if (n == 0) return 0;
    if (!d_keys || !d_koff || !d_vals || !d_voff || !d_op || !d_wal || !d_log_start || !d_wal_off ||
        !d_wal_len || !d_rec_base || !d_counts)
        return LSM_EINVAL;
    if (mem_max == 0 || mem_max > (1ull << 30) || align == 0 || n >= (1ull << 31) || nlog_max == 0 ||
        nlog_max > 65535)
        return LSM_EINVAL;
    if (d_cur_idx && (!d_cur_bytes || !d_cur_desc)) return LSM_EINVAL;
    if (!d_ws || ws_bytes < lsm_db_write_workspace_bytes(n, nlog_max, mem_max)) return LSM_ESPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsCursor c{static_cast<uint8_t *>(d_ws), 0};
    const Ws ws = ws_layout(c, n, nlog_max);
    const Batch b{d_keys, d_koff, d_vals, d_voff, d_op, (uint32_t)n};
    const Rot rot{ws.hdr, ws.ls};
    const OpKeys S{b, rot};
    const Nodes cur{d_cur_bytes, d_cur_desc, d_cur_idx, d_cur_idx ? cur_nnode : 0};
    const Out o{d_wal, d_log_start, d_wal_off, d_wal_len, d_desc, d_rec_base, d_main_slot, d_counts};
    const uint32_t ntile = scan_tiles(n), nop = (uint32_t)((n + kThreads - 1) / kThreads);

    hipLaunchKernelGGL(wr_est_sum, dim3(ntile), dim3(kScanThreads), 0, s, b, ws.epart);
    hipLaunchKernelGGL(scan_partials_kernel<uint64_t>, dim3(1), dim3(kPartThreads), 0, s, ws.epart, ntile, ws.E,
                       (uint32_t)n);
    hipLaunchKernelGGL(wr_est_scan, dim3(ntile), dim3(kScanThreads), 0, s, b, ws.epart, ws.E);
    hipLaunchKernelGGL(wr_next, dim3(nop), dim3(kThreads), 0, s, b.n, ws.E, mem_max, ws.next);
    hipLaunchKernelGGL(wr_chase, dim3(1), dim3(kWave), 0, s, b.n, ws.E, ws.next, mem_size0, mem_max, nlog_max,
                       ws.ls, ws.hdr, d_counts);
    hipLaunchKernelGGL(wr_seg, dim3(nop), dim3(kThreads), 0, s, b.n, rot, ws.seg);

    const uint32_t maxops = max_log_ops(n, mem_max);
    const int at = mt_sort_segments(S, nlog_max, maxops, ws.key, ws.pos, s);
    hipLaunchKernelGGL(wr_presence, dim3((maxops + kThreads - 1) / kThreads, nlog_max), dim3(kThreads), 0, s, S,
                       cur, ws.key[at], ws.pos[at], ws.extra);

    hipLaunchKernelGGL(wr_stream_sum, dim3(ntile), dim3(kScanThreads), 0, s, b, rot, ws.extra, ws.xpart);
    hipLaunchKernelGGL(scan_partials_kernel<Sum2>, dim3(1), dim3(kPartThreads), 0, s, ws.xpart, ntile, ws.X,
                       (uint32_t)n);
    hipLaunchKernelGGL(wr_stream_scan, dim3(ntile), dim3(kScanThreads), 0, s, b, rot, ws.extra, ws.xpart, ws.X);
    hipLaunchKernelGGL(wr_logs, dim3(1), dim3(kWave), 0, s, b, rot, ws.extra, ws.X, ws.E, mem_size0, align,
                       ws.logS, o);
    hipLaunchKernelGGL(wr_emit, dim3((uint32_t)((n + kEmitOps - 1) / kEmitOps)), dim3(kWave), 0, s, b, rot,
                       ws.seg, ws.extra, ws.X, ws.logS, o);
    LSM_HIP_CHECK(hipGetLastError());
    return 0;
}
