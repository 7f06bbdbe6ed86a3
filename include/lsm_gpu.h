/*
 * lsm_gpu.h — C ABI of the MI355X (gfx950) SSTable block codec.
 *
 * Drop-in boundary for the go-lsm hot path (xmh1011/go-lsm @ 2025-08-24):
 * the Go methods it replaces are cited per entry point.  Plain pointers and
 * sizes only; `stream` is an opaque hipStream_t (NULL = default stream).
 * Every launch entry point is asynchronous on `stream`, performs no device
 * allocation and no host synchronisation (hipGraph-capturable) -- except
 * lsm_merge_kvs, which synchronizes `stream` (its radix passes are chosen
 * from key statistics read back to the host); the caller owns every buffer
 * and the library keeps no pointer after the call returns.  lsm_build_sst
 * and lsm_build_sst_views may run part of their launches on the context's
 * side stream, forked from `stream` by an event and joined back into it
 * before they return (so a context serves one caller thread at a time).
 *
 * Device input buffers (blocks, images, logs, key and value arenas) must be
 * readable up to LSM_INPUT_SLACK bytes past the next multiple of 16 bytes
 * after their last byte: roundup16(n) + 32.  The kernels stream 16-byte
 * aligned chunks, and key hashing / bound prefixes load 8-byte words at any
 * key start (up to key_start + 20 for a key ending the buffer).  Bytes past a
 * block or key are never interpreted.  lsm_dev_alloc pads by this much.
 *
 * Return convention: 0 = ok; negative = LSM_E* (argument error) or
 * -(1000 + hipError_t) for a HIP runtime error.
 */
#ifndef LSM_GPU_H
#define LSM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v3: the input slack grew from 16 to 32 bytes (a binding built for v2 pads
 * too little); lsm_input_slack() reports it at run time.
 * v4: lsm_merge_kvs_tie writes 3 h_counts entries; lsm_merge_kvs keeps the
 * v2 / v3 contract of exactly 2 ({nout, nfiles}).
 * v5: lsm_merge_kvs_async and lsm_gather_kvs_dev (the merge's counts stay on
 * the device; the gather reads its pair count there); the level sparse index
 * (lsm_level_index_build, lsm_level_may_contain_indexed).
 * v6: lsm_level_get (the batched Get past MayContain: Seek + the value) and
 * its Seek tree (lsm_level_get_tree_bytes, lsm_level_get_tree_build);
 * lsm_compact_merge_async (the join and the merge as one call).
 * v7: the builder rule on the device (lsm_segment_files) and the builder path
 * over one sorted stream as one call (lsm_build_sst_stream: rule, layout and
 * images with the fused bloom, no host round trip); lsm_level_get takes the
 * Seek tree's size; lsm_level0_get (searchFromLevel0 over every table);
 * lsm_level_search_get (a level's search and Get in one call);
 * lsm_goheap_pop_order_host reports its phases, lsm_goheap_replays;
 * lsm_build_flags.
 * Added within v7 (backward compatible, the version stays 7; a binding finds
 * them by symbol lookup): lsm_search and lsm_search_workspace_bytes
 * (Manager.Search over a whole tree in one call); lsm_memtable_order and
 * lsm_memtable_order_workspace_bytes (a memtable's contents from its WAL);
 * lsm_memtable_search with lsm_memtable_search_index_bytes / _index_build
 * (memtable.Manager.Search over those memtables) and lsm_db_get with
 * lsm_db_get_workspace_bytes (database.Get in one call); lsm_tree_scan and
 * lsm_tree_scan_workspace_bytes (batched range scan over a whole tree);
 * lsm_db_scan and lsm_db_scan_workspace_bytes (that scan with the memtables in
 * front: the batched database scan); lsm_pack_results and
 * lsm_pack_results_workspace_bytes (the answered bytes of those four reads
 * packed into two CSR arenas on the device); lsm_merge_plan (the ordering
 * plan the last merge call chose, read-only). */
#define LSM_ABI_VERSION 7
#define LSM_INPUT_SLACK 32  /* readable bytes past roundup16(n) of any device input */

/* Record grammars (all fixed-width little-endian). */
enum lsm_grammar {
    LSM_GRAMMAR_V = 0,   /* ([u32 vlen][value])*            sstable/block/data.go:26-79   */
    LSM_GRAMMAR_KV = 1,  /* ([u32 klen][key][u32 vlen][v])*  kv/kv.go:46-115, wal/wal.go:107 */
    LSM_GRAMMAR_IDX = 2, /* ([u32 klen][key][i64 offset])*   sstable/block/index.go:30-101 */
};

/* Per-block decode status (d_status[b]); d_nrec[b] always counts the
 * records decoded before the status was raised (data.go:75 keeps them). */
enum lsm_status {
    LSM_OK = 0,
    LSM_ST_TRUNC_LEN_PREFIX = 1, /* 1-3 bytes left for a leading u32 length: data.go:65 "read value length failed", kv.go:80 "decode key length" */
    LSM_ST_TRUNC_KEY = 2,        /* kv.go:90 "decode key"                          */
    LSM_ST_KEY_TOO_LONG = 3,     /* kv.go:84 "invalid key length: %d" (> 1<<20)   */
    LSM_ST_TRUNC_VLEN = 4,       /* kv.go:98 "decode value length"                 */
    LSM_ST_VAL_TOO_LONG = 5,     /* kv.go:102 "invalid value length: %d" (> 1<<30) */
    LSM_ST_TRUNC_VAL = 6,        /* data.go:71 "read value data failed", kv.go:108 "decode value" */
    LSM_ST_IDX_OVERRUN = 7,      /* an index entry crosses the block's end: see below */
    LSM_ST_CAPACITY = 8,         /* record capacity rec_base[b+1]-rec_base[b] exhausted (not a reference error) */
};

/* LSM_ST_CAPACITY and a reference error in one block.  A record takes its
 * slot only after it has passed every check of the reference, and capacity is
 * raised by the first such record that finds no slot.  So a block (or a log of
 * lsm_wal_replay) with more valid records than slots reports LSM_ST_CAPACITY
 * with d_nrec = the capacity, whatever error follows those records; one whose
 * valid records all fit -- exactly enough slots included -- reports the
 * reference's own status.  No slot past the capacity is written. */

/* LSM_ST_IDX_OVERRUN and the reference's three messages.  IndexBlock.DecodeFrom
 * (index.go:61-101) reads an entry whole -- Key.DecodeFrom, then the i64
 * offset -- and only then compares totalRead with the size.  Which error Go
 * returns for an entry that crosses the block's end therefore depends on the
 * bytes its io.Reader holds PAST the block:
 *   - enough bytes (SSTable.DecodeFrom's reader is the whole file, the footer
 *     follows the index, sstable.go:122; index_test.go's reader holds the
 *     whole buffer): "unexpected EOF: size limit reached while reading key
 *     length" (index.go:88-91);
 *   - the reader ends inside the key length or the key (a reader cut at the
 *     block): "decode index key length failed" (index.go:73-76);
 *   - the reader ends inside the offset: "decode index offset failed"
 *     (index.go:81-84).
 * The library never reads past blk_len, so it reports this one status for
 * all three, with d_nrec = the entries before the crossing one -- what Go
 * appended in every case (the oracle, oracle/lsm_oracle.c, follows the first
 * reading: bytes past the block present).  A binding that needs Go's message
 * picks it from the bytes its own reader holds past the block. */

enum lsm_error {
    LSM_EINVAL = -1,  /* bad argument                        */
    LSM_ENODEV = -2,  /* no gfx950 device / device not found  */
    LSM_ENOMEM = -3,  /* host allocation failed              */
    LSM_ESPACE = -4,  /* workspace too small                 */
};

/* One decoded record: a zero-copy view into the input buffer.
 *   KV : key  = d_in[rec_off+4 .. +key_len), value = d_in[rec_off+8+key_len .. +val_len)
 *   V  : key_len = 0, value = d_in[rec_off+4 .. +val_len)
 *   IDX: key  = d_in[rec_off+4 .. +key_len), val_len = 8 (the i64 offset follows the key) */
typedef struct lsm_rec_desc {
    uint64_t rec_off;
    uint32_t key_len;
    uint32_t val_len;
} lsm_rec_desc;

/* Outputs of lsm_decode_blocks.  Record i of block b goes to slot
 * base(b) + i of every per-record array, where
 *   rec_base != NULL : base(b) = rec_base[b], capacity rec_base[b+1]-rec_base[b]
 *                      (lsm_plan_rec_base computes a dense-capacity plan);
 *   rec_base == NULL : offset-addressed, base(b) = blk_off[b] / R and capacity
 *                      (blk_off[b]+blk_len[b]) / R - base(b), R = 4 (V), 8 (KV),
 *                      12 (IDX) -- disjoint for non-overlapping blocks, no plan
 *                      needed; per-record arrays need (input bytes / R) + 1 slots. */
typedef struct lsm_decode_out {
    lsm_rec_desc *desc;         /* required                                         */
    const uint64_t *rec_base;   /* optional, nblk+1 entries (see above)             */
    uint32_t *nrec;             /* required, nblk                                   */
    int32_t *status;            /* required, nblk                                   */
    int64_t *idx_value;         /* IDX only, optional: the entry's i64 offset       */
    /* Materialized ("ARENA") mode, all optional.  Keys / values of block b are
     * packed, in record order, from key_arena + A(b) / val_arena + A(b), where
     * A(b) = arena_base[b] (lsm_plan_arena_base: exclusive scan of blk_len) or,
     * with arena_base == NULL, A(b) = blk_off[b] (arenas mirror the input's
     * addressing; a block's keys or values never exceed blk_len bytes). */
    uint8_t *key_arena;
    uint8_t *val_arena;
    const uint64_t *arena_base; /* optional, nblk+1                                 */
    uint64_t *key_arena_off;    /* optional per record: absolute offset in key_arena */
    uint64_t *val_arena_off;    /* optional per record: absolute offset in val_arena */
} lsm_decode_out;

typedef struct lsm_ctx lsm_ctx;

/* ---- context ------------------------------------------------------------ */

int lsm_abi_version(void);
/* LSM_INPUT_SLACK of the loaded library: a binding checks it at load time. */
int lsm_input_slack(void);
/* Identity of the sources the library was compiled from (16 hex digits,
 * go-lsm_amd/build_id.py): a binding shipped beside the sources compares it
 * and refuses a stale prebuilt library.  Not part of the Go surface. */
const char *lsm_build_id(void);
/* "HIPCC|ARCH|HIPFLAGS" the library was compiled with: the build id hashes
 * these with the sources, so a binding recomputes the id from this string. */
const char *lsm_build_flags(void);
/* One context per goroutine / OS thread (callers are concurrent goroutines,
 * sstable_test.go:379-400); no hidden global mutable state. */
int lsm_ctx_create(int device, lsm_ctx **out);
int lsm_ctx_destroy(lsm_ctx *ctx);
/* Number of compute units of the context's device (grid sizing). */
int lsm_ctx_num_cus(const lsm_ctx *ctx);

/* ---- memory / stream plumbing (so a cgo or C++ host needs no HIP headers) -- */

/* Device allocation, rounded up to 16 bytes plus 16 bytes of slack (the
 * readability contract above).  Not for use inside a timed/captured region. */
int lsm_dev_alloc(lsm_ctx *ctx, size_t bytes, void **out);
int lsm_dev_free(lsm_ctx *ctx, void *p);
/* Pinned (page-locked) host memory for asynchronous H2D/D2H staging. */
int lsm_host_alloc_pinned(lsm_ctx *ctx, size_t bytes, void **out);
int lsm_host_free_pinned(lsm_ctx *ctx, void *p);
int lsm_memcpy_h2d(lsm_ctx *ctx, void *d_dst, const void *h_src, size_t bytes, void *stream);
int lsm_memcpy_d2h(lsm_ctx *ctx, void *h_dst, const void *d_src, size_t bytes, void *stream);
int lsm_memset_dev(lsm_ctx *ctx, void *d_dst, int value, size_t bytes, void *stream);
int lsm_stream_create(lsm_ctx *ctx, void **out);
int lsm_stream_destroy(lsm_ctx *ctx, void *stream);
int lsm_stream_sync(lsm_ctx *ctx, void *stream);

/* ---- planning ------------------------------------------------------------ */

/* Largest record count a block of `len` bytes can hold: KV len/8, V len/4,
 * IDX len/12 (every record carries at least its fixed-width fields). */
uint64_t lsm_max_records(int grammar, uint64_t len);
size_t lsm_plan_workspace_bytes(uint32_t nblk);
/* d_rec_base[0..nblk] = exclusive scan of lsm_max_records(grammar, blk_len[b]). */
int lsm_plan_rec_base(lsm_ctx *ctx, int grammar, const uint32_t *d_blk_len, uint32_t nblk,
                      uint64_t *d_rec_base, void *d_workspace, size_t ws_bytes, void *stream);
/* d_arena_base[0..nblk] = exclusive scan of blk_len[b]. */
int lsm_plan_arena_base(lsm_ctx *ctx, const uint32_t *d_blk_len, uint32_t nblk,
                        uint64_t *d_arena_base, void *d_workspace, size_t ws_bytes, void *stream);

/* ---- decode ---------------------------------------------------------------- */

/* Batch decode of independent blocks [blk_off[b], blk_off[b]+blk_len[b]).
 * Replaces, per block:
 *   V   : block.DataBlock.DecodeFrom(r, size)      sstable/block/data.go:49-79
 *   KV  : kv.KeyValuePair.DecodeFrom loop           kv/kv.go:77-115, wal/wal.go:106-118
 *   IDX : block.IndexBlock.DecodeFrom(r, size)     sstable/block/index.go:61-101
 * and, composed by the host layer, SSTable.DecodeDataBlock/GetDataBlockFromFile
 * (sstable/sstable.go:214-246).  One wavefront owns one block: the block is
 * streamed into an LDS ring and the record boundaries are chased there. */
int lsm_decode_blocks(lsm_ctx *ctx, int grammar, const uint8_t *d_in, const uint64_t *d_blk_off,
                      const uint32_t *d_blk_len, uint32_t nblk, const lsm_decode_out *out,
                      void *stream);

/* lsm_decode_blocks with the caller's upper bound on the block lengths: above
 * 32 KiB a larger per-wave LDS ring is used (more bytes in flight per wave).
 * The hint only selects the ring; results are identical for any input, also
 * when a block is longer than the hint. */
int lsm_decode_blocks_hinted(lsm_ctx *ctx, int grammar, const uint8_t *d_in,
                             const uint64_t *d_blk_off, const uint32_t *d_blk_len, uint32_t nblk,
                             uint32_t max_blk_len, const lsm_decode_out *out, void *stream);

/* lsm_decode_blocks for a batch whose block sizes vary: the blocks are
 * launched largest first (a device-side bucketing of d_blk_len by power-of-
 * two size class, part of this call), so the batch does not end on a tail of
 * large blocks each streamed by a single wave.  Outputs are addressed by
 * block id exactly as in lsm_decode_blocks (identical results).  Workspace:
 * lsm_decode_schedule_workspace_bytes(nblk). */
size_t lsm_decode_schedule_workspace_bytes(uint32_t nblk);
int lsm_decode_blocks_scheduled(lsm_ctx *ctx, int grammar, const uint8_t *d_in,
                                const uint64_t *d_blk_off, const uint32_t *d_blk_len,
                                uint32_t nblk, const lsm_decode_out *out, void *d_workspace,
                                size_t ws_bytes, void *stream);

/* Compact the records of a finished lsm_decode_blocks into one dense array:
 * d_dense_base[0..nblk] = exclusive scan of nrec (d_dense_base[nblk] = total)
 * and block b's records land at d_dense[d_dense_base[b] ..] (and IDX values
 * at d_dense_idx, optional).  `out` is the lsm_decode_out the decode used
 * (its rec_base, or offset addressing with d_blk_off).  Workspace:
 * lsm_plan_workspace_bytes(nblk).  This is the hand-off a host consumer
 * copies back (GetKeyValuePairs' record list, sstable.go:248-268). */
int lsm_compact_records(lsm_ctx *ctx, int grammar, const uint64_t *d_blk_off, uint32_t nblk,
                        const lsm_decode_out *out, lsm_rec_desc *d_dense, int64_t *d_dense_idx,
                        uint64_t *d_dense_base, void *d_workspace, size_t ws_bytes, void *stream);

/* ---- WAL replay ------------------------------------------------------------ */

/* wal.Recover (wal/wal.go:95-121) of nwal write-ahead logs, each read whole
 * into device memory (io.ReadAll, :101) at [wal_off[w], wal_off[w]+wal_len[w]):
 * KeyValuePair.DecodeFrom (kv/kv.go:77-115) looped while bytes remain
 * (:107-118).  The records decoded before an error are delivered (Recover has
 * already called back for them, :117) and status[w] names the error, which
 * Recover returns as "failed to read wal <file>: <err>".  Outputs and
 * placement as lsm_decode_blocks with LSM_GRAMMAR_KV, one block per log
 * (descriptors only; no arenas).  A log is decoded by many waves (16 KiB
 * segments, guessed entry points, an exact stitch), so the records are the
 * serial chase's.  max_wal_len >= every wal_len[w] sizes the grid and the
 * workspace (a longer log is chased by one wave); workspace:
 * lsm_wal_replay_workspace_bytes(nwal, max_wal_len). */
size_t lsm_wal_replay_workspace_bytes(uint32_t nwal, uint32_t max_wal_len);
int lsm_wal_replay(lsm_ctx *ctx, const uint8_t *d_wal, const uint64_t *d_wal_off,
                   const uint32_t *d_wal_len, uint32_t nwal, uint32_t max_wal_len,
                   const lsm_decode_out *out, void *d_workspace, size_t ws_bytes, void *stream);

/* ---- memtable flush (added within ABI 7) ----------------------------------- */

/* The contents of nlog memtables from their WALs, in one asynchronous call:
 * what IMemTable.RangeScan (memtable/imemtable.go:46-53) hands to
 * BuildSSTableFromIMemTable (sstable/builder.go:22-31) on every eviction
 * (sstable/manager.go:74-95) and on recovery (memtable/manager.go:140-180).
 * A memtable is a skiplist in which a later Add of a key replaces the earlier
 * pair (skiplist/skiplist.go:83-118), and MemTable.Insert appends to the WAL
 * before AddPair (memtable.go:68-78), so its nodes are exactly the last
 * record of each key of its log, in key order.
 *
 * Input: lsm_wal_replay's outputs as they are (KV descriptors d_desc into
 * d_bytes, d_nrec, d_status) in either placement -- d_rec_base (nlog + 1
 * entries), or NULL for offset addressing, base(w) = d_log_off[w] / 8.  nslot
 * is the number of entries of d_desc (< 2^32 - 1); max_log_records bounds
 * every d_nrec[w] (lsm_max_records(LSM_GRAMMAR_KV, max_wal_len); < 2^31) and,
 * with nlog (<= 65535) and nslot, sizes every launch and the workspace.
 *
 * Per log w with d_status[w] == 0: its records sorted by key in Go string
 * order (bytewise, unsigned, a proper prefix first; any key length), of equal
 * keys the one at the greatest input position kept.  A log with a non-zero
 * status contributes nothing (wal.Recover returned an error, memtable.go:
 * 133-139; the caller has the status).  Logs never interact.  The kept
 * records' slots (indices into d_desc) go to d_idx[d_file_start[w] ..
 * d_file_start[w + 1]), dense across logs; d_idx holds as many entries as the
 * logs have records (nslot always suffices).
 *   LSM_MEMTABLE_ALL: every node, tombstones (kv.DeletedValue, kv.go:29-31:
 *     a value of exactly those 13 bytes) included -- the memtable's whole
 *     contents, and the mode to use.
 *   LSM_MEMTABLE_RANGESCAN: RangeScan as written, `for SeekToFirst(); Valid();
 *     Next()` (skiplist/iterator.go:27-33, 68-70): the tombstones at the front
 *     are skipped and delivery STOPS before the first tombstone after that,
 *     so the pairs behind it never reach the SSTable.  The reference's exact
 *     output, as LSM_TIE_GOHEAP is for the merge; not the recommended mode.
 * d_counts (device, 3 entries) = {pairs delivered, logs with at least one
 * pair, the most pairs in one log} -- what the build's launch needs.  A log
 * with d_nrec[w] > max_log_records (or whose records pass nslot) is not
 * indexed: it gets no pairs and bit 63 of d_counts[2] is set.
 * nlog == 0 returns 0 with nothing written.  No host synchronisation, no
 * read-back and no device allocation: the call can be captured in a graph.
 * Workspace: lsm_memtable_order_workspace_bytes (40 bytes per slot). */
enum lsm_memtable_scan {
    LSM_MEMTABLE_ALL = 0,       /* every node of the skiplist, tombstones included            */
    LSM_MEMTABLE_RANGESCAN = 1, /* IMemTable.RangeScan as written (imemtable.go:46-53), exact */
};
#define LSM_MEMTABLE_TILE 1024 /* records sorted in LDS by one workgroup */
#define LSM_MEMTABLE_OVERFLOW (1ull << 63) /* in d_counts[2] */
size_t lsm_memtable_order_workspace_bytes(uint32_t nlog, uint64_t nslot, uint32_t max_log_records);
int lsm_memtable_order(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc,
                       const uint64_t *d_rec_base, const uint64_t *d_log_off, const uint32_t *d_nrec,
                       const int32_t *d_status, uint32_t nlog, uint64_t nslot,
                       uint32_t max_log_records, int scan, uint32_t *d_idx, uint64_t *d_file_start,
                       uint64_t *d_counts, void *d_ws, size_t ws_bytes, void *stream);

/* ---- memtable search and database.Get (added within ABI 7) ----------------- */

/* Batched memtable.Manager.Search (memtable/manager.go:61-74) over the
 * memtables lsm_memtable_order delivers: the first half of database.Get
 * (database/database.go:24-40).  SkipList.Search (skiplist/skiplist.go:60-79)
 * finds the node with exactly the key: no node is (nil, false), a node whose
 * value IsDeleted (exactly the 13 bytes of kv.DeletedValue, kv.go:29-43) is
 * (nil, true), any other node (value, true).  Manager.Search asks Mem, then
 * IMems from the last to the first; the first table with ok == true ends the
 * search, also when what it returns is nil: a tombstone in a newer memtable
 * hides a value in an older one.  Manager.Recover (manager.go:140-180) lists
 * the WALs by ascending id, the last one becomes Mem, so for logs given OLDEST
 * FIRST the search visits log nlog - 1, nlog - 2, ..., 0.
 *
 * d_bytes / d_desc are lsm_memtable_order's inputs, d_idx / d_file_start its
 * outputs with LSM_MEMTABLE_ALL: log w's nodes are d_idx[d_file_start[w] ..
 * d_file_start[w + 1]), in key order.  A failed, empty or overflowed log has
 * no nodes there and answers nothing.  The probe keys are CSR (d_keys,
 * d_koff with nkeys + 1 entries) under the input-slack contract; they are
 * compared in Go string order over any key length (a probe longer than
 * 1 << 20 bytes, kv.go:84, equals no node).  Per key, for the first log
 * searched that holds a node with exactly that key:
 *   d_mem_result[i] = LSM_MEM_VALUE or LSM_MEM_DELETED, d_log[i] = that log,
 *   d_slot[i] = the node's index in d_desc, d_value[i] = {rec_off = the offset
 *   in d_bytes of the value's u32 length prefix (desc.rec_off + 4 + key_len),
 *   key_len = 0, val_len} for LSM_MEM_VALUE -- lsm_level_get's view
 *   convention -- and all zero for LSM_MEM_DELETED;
 * when no log holds it: LSM_MEM_MISS, -1, 0xFFFFFFFF, all zero.
 * nlog == 0 answers every key LSM_MEM_MISS.
 *
 * What the WAL alone can and cannot say:
 *   - Empty values.  A replayed empty value is make([]byte, 0), non-nil: a
 *     found value of length 0 (LSM_MEM_VALUE, val_len 0), and Get returns it.
 *     A live Put(key, nil) holds Go's nil and falls through to the tables; the
 *     WAL encodes both as an empty value and the library follows the replayed
 *     form.
 *   - Delete on a full memtable.  Live, when Manager.Delete meets a full
 *     memtable the old memtable's node is unlinked and the new Mem holds the
 *     tombstone; replayed, the old log ends in (key, "").  The newer log is
 *     searched first in both cases, so the answer is the same while both logs
 *     are passed.
 *   - LSM_MEMTABLE_RANGESCAN's d_idx is a subset of the nodes: searching it is
 *     not Manager.Search, and the call cannot detect it.  Pass the
 *     LSM_MEMTABLE_ALL order.
 *
 * d_index (optional): lsm_memtable_search_index_build's buffer.  It holds each
 * node's first 16 key bytes in d_idx order (behind a 256-byte header with the
 * number of nodes indexed), so a bisection step is one 16-byte gather and the
 * node is read only on a 16-byte tie; without it a step is three dependent
 * loads (d_idx -> d_desc -> the key).  The answers are identical.  It is built
 * once per set of memtables and valid while d_idx is; nnode_max >=
 * d_file_start[nlog] (nslot always suffices; the count is read on the device).
 * A log whose nodes pass the indexed count (an index built with a smaller
 * nnode_max) is searched through d_idx.  lsm_memtable_search_index_bytes(0)
 * = 0; the build with nlog == 0 or nnode_max == 0 returns 0.
 *
 * Argument checks, in this order, all before any launch: ctx == NULL ->
 * LSM_EINVAL; nkeys == 0 -> 0; nlog > 65535 or a required pointer NULL ->
 * LSM_EINVAL; d_index != NULL with index_bytes below
 * lsm_memtable_search_index_bytes(1) (no index fits) -> LSM_ESPACE.  The search
 * is not told nnode_max, so that is all it can refuse: an index passed with an
 * index_bytes smaller than it was built with does not fail, it serves only the
 * logs whose nodes lie inside index_bytes and the others take the slower walk
 * through d_idx (same answers).  Pass the size the build was given.
 * lsm_memtable_search_index_build's checks, in this order, all before its
 * launch: ctx == NULL -> LSM_EINVAL; nlog == 0 or nnode_max == 0 -> 0 (nothing
 * written); nlog > 65535, nnode_max >= 2^32 - 1 (slots are u32) or a NULL
 * d_bytes / d_desc / d_idx / d_file_start -> LSM_EINVAL; d_index == NULL or
 * index_bytes below lsm_memtable_search_index_bytes(nnode_max) -> LSM_ESPACE.
 * One launch, one thread per key (grid-stride past 2,048 workgroups); no host
 * synchronisation, no read-back, no device allocation, no workspace: both
 * calls can be captured in a graph. */
enum lsm_mem_result { LSM_MEM_MISS = 0, LSM_MEM_VALUE = 1, LSM_MEM_DELETED = 2 };
size_t lsm_memtable_search_index_bytes(uint64_t nnode_max);
int lsm_memtable_search_index_build(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc,
                                    const uint32_t *d_idx, const uint64_t *d_file_start, uint32_t nlog,
                                    uint64_t nnode_max, void *d_index, size_t index_bytes, void *stream);
int lsm_memtable_search(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_desc,
                        const uint32_t *d_idx, const uint64_t *d_file_start, uint32_t nlog,
                        const void *d_index, size_t index_bytes, const uint8_t *d_keys,
                        const uint64_t *d_koff, uint64_t nkeys, int32_t *d_mem_result, int32_t *d_log,
                        uint32_t *d_slot, lsm_rec_desc *d_value, void *stream);

/* ---- whole .sst files ------------------------------------------------------ */

/* Per-file result of lsm_decode_sst.  Offsets are relative to the file image. */
typedef struct lsm_sst_meta {
    uint64_t min_key_off, min_key_len, max_key_off, max_key_len; /* Header      header.go:40-52 */
    uint64_t filter_m, filter_k, filter_nbits;                   /* Filter      bloom.go:453-469 */
    uint64_t filter_words_off; /* first filter word (u64 big-endian, bitset v1.22.0 WriteTo)   */
    int64_t data_off, data_size, idx_off, idx_size;              /* Footer      footer.go:58-70 */
    int32_t stage;   /* enum lsm_sst_stage: the first step that failed, 0 = none               */
    int32_t status;  /* lsm_status of a failing index (stage 4) or data (stage 5) decode       */
    uint32_t nidx;   /* index entries decoded (those before an error are kept, index.go:94)  */
    uint32_t ndata;  /* values decoded (those before an error are kept, data.go:75)          */
} lsm_sst_meta;

enum lsm_sst_stage {
    LSM_SST_OK = 0,
    LSM_SST_HEADER = 1,   /* sstable.go:101-104 "decode Header failed"                       */
    LSM_SST_FILTER = 2,   /* sstable.go:106-109 "decode FilterBlock failed"                  */
    LSM_SST_FOOTER = 3,   /* sstable.go:112-115 "decode Footer failed" (file < 32 bytes)     */
    LSM_SST_INDEX = 4,    /* sstable.go:118-125 seek / "decode IndexBlock failed"            */
    LSM_SST_DATA = 5,     /* sstable.go:214-225 seek / "decode DataBlock failed"             */
    LSM_SST_MISMATCH = 6, /* sstable.go:254-257 "mismatched DataBlock and IndexBlock entries" */
};

size_t lsm_decode_sst_workspace_bytes(uint32_t nfile);

/* Decode nfile whole .sst images [file_off[f], file_off[f] + file_len[f]) of
 * d_img: SSTable.DecodeFrom (sstable.go:87-128: header, filter, footer, the
 * IndexBlock chase), DecodeDataBlock (:214-225: the DataBlock chase over
 * DataHandle, data.go:49-79) and GetKeyValuePairs (:248-268: the positional
 * join) in one call.  Entry i of file f goes to slot base(f) + i of
 * d_idx_desc / d_idx_value (key view + i64 offset) and of d_data_desc (value
 * view); record i is (key of idx entry i, value i) for
 * i < (stage == 0 && nidx && ndata ? nidx : 0).  base(f) = d_rec_base[f]
 * with capacity d_rec_base[f+1] - base(f), or with d_rec_base == NULL,
 * file_off[f] / 4 with capacity (file_off[f] + file_len[f]) / 4 - base(f).
 * The results equal the reference's serial chases; the index and the values
 * are verified in parallel (stride hypothesis, index offsets) and chased
 * exactly from the first entry the verification cannot vouch for.
 * Workspace: lsm_decode_sst_workspace_bytes(nfile). */
int lsm_decode_sst(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                   const uint64_t *d_file_len, uint32_t nfile, const uint64_t *d_rec_base,
                   lsm_sst_meta *d_meta, lsm_rec_desc *d_idx_desc, int64_t *d_idx_value,
                   lsm_rec_desc *d_data_desc, void *d_workspace, size_t ws_bytes, void *stream);

/* Batched SSTable.MayContain (sstable.go:300-305) of nkeys keys (CSR, as in
 * lsm_bloom_probe) against nfile .sst images: the key range check against
 * the header's MinKey / MaxKey in Go string order, then Filter.Test
 * (bloom.go:371-379) on the filter block as stored in the image.  d_meta is
 * lsm_decode_sst's output for the same images; a file whose header or filter
 * did not decode (stage 1 or 2) reports 0.  d_hit[i * nfile + f] = 1 when
 * key i may be in file f.  Deviations on corrupted filters only: m == 0
 * reports 0 (Go divides by zero) and k is capped at 4096 probes.
 * When every file decoded, the files are in key order with disjoint ranges
 * (a level >= 1 set), nfile <= 2048 and nkeys < 2^32, the probes are grouped
 * by their one candidate file and each filter is tested from LDS; otherwise
 * every key is checked against every file.  The workspace holds the grouping (see
 * lsm_may_contain_workspace_bytes); d_hit is written whole either way. */
size_t lsm_may_contain_workspace_bytes(uint32_t nfile, uint64_t nkeys);
int lsm_may_contain(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                    const lsm_sst_meta *d_meta, uint32_t nfile, const uint8_t *d_keys,
                    const uint64_t *d_koff, uint64_t nkeys, uint8_t *d_hit, void *d_workspace,
                    size_t ws_bytes, void *stream);

/* Batched Manager.searchFromLevelWithSparseIndex (sstable/manager.go:178-207)
 * up to searchFromTable's MayContain (:209-212) for a level >= 1: the nfile
 * images are the level's tables in sparse-index order (sorted by MinKey,
 * manager.go:290-303), d_meta their lsm_decode_sst output.  For key i:
 * sort.Search (Go's exact bisection) for the first table whose MinKey > key
 * (bytes.Compare), index-- when > 0 (:186-192), then SSTable.MayContain
 * (sstable.go:300-305) of that one table: d_table[i] = the candidate (-1 when
 * the level is empty), d_may[i] = 1 when the table may hold the key.
 * Deviation (corrupted tables only): a table whose header did not decode
 * searches as the zero Header (MinKey "") and, like one whose filter did not
 * decode, answers 0 -- go-lsm's Manager.Recover (manager.go:226-275) would
 * have failed on such a file and never listed it in the level, so the
 * reference has no answer to restate; filter deviations as lsm_may_contain.  Level 0 (searchFromLevel0, :160-176, every table in
 * order): lsm_may_contain for the may-bits, lsm_level0_get for the Get.
 * Workspace: lsm_level_may_contain_workspace_bytes. */
size_t lsm_level_may_contain_workspace_bytes(uint32_t nfile, uint64_t nkeys);
int lsm_level_may_contain(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                          const lsm_sst_meta *d_meta, uint32_t nfile, const uint8_t *d_keys,
                          const uint64_t *d_koff, uint64_t nkeys, int32_t *d_table,
                          uint8_t *d_may, void *d_workspace, size_t ws_bytes, void *stream);
/* The level's sparse index (ABI 5) -- Manager's sparseIndexes[level-1]
 * (manager.go:183-187): each table's MinKey / MaxKey prefixes and filter shape,
 * parsed from the images once and kept while the level is unchanged, as the
 * Manager keeps its loaded SSTables.  d_index: lsm_level_index_bytes(nfile)
 * bytes; it refers to offsets inside d_img, so the searches pass the same
 * d_img.  lsm_level_may_contain_indexed = lsm_level_may_contain without
 * parsing the headers again (same outputs, same workspace). */
size_t lsm_level_index_bytes(uint32_t nfile);
int lsm_level_index_build(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                          const lsm_sst_meta *d_meta, uint32_t nfile, void *d_index, void *stream);
int lsm_level_may_contain_indexed(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index,
                                  uint32_t nfile, const uint8_t *d_keys, const uint64_t *d_koff,
                                  uint64_t nkeys, int32_t *d_table, uint8_t *d_may,
                                  void *d_workspace, size_t ws_bytes, void *stream);

/* Batched searchFromTable past its MayContain (sstable/manager.go:209-223):
 * for key i with d_may[i] = 1 (lsm_level_may_contain's answer for table
 * d_table[i]), Iterator.Seek over that table's IndexBlock (sstable/block/
 * index.go:157-181: Go's bisection for the first entry whose key >= the
 * target, valid only on an exact match) and Iterator.Value ->
 * GetValueByOffset (sstable.go:271-296: Value.DecodeFrom, kv.go:181-200, at
 * the entry's offset in the file).  The index is lsm_decode_sst's output for
 * the same images (d_meta, d_idx_desc, d_idx_value, with the same
 * d_rec_base or offset placement); file f is d_img[file_off[f] ..
 * + file_len[f]).  d_result[i] is a lsm_get_result; on LSM_GET_FOUND
 * d_value[i] is a view of the value {rec_off = offset in d_img of its u32
 * length prefix, key_len = 0, val_len}; otherwise d_value[i] is zero.  The
 * Seek runs over the nidx entries the decode kept (a table whose index did
 * not decode is one the Manager would not have loaded, manager.go:226-275).
 * d_tree (or NULL) is the level's Seek tree from lsm_level_get_tree_build
 * over the same decoded tables with max_nidx = tree_nidx; tables with more
 * index entries than that walk the index.  The steps are Go's either way, so
 * the answers are the same with and without the tree.  tree_bytes (ABI 7) is
 * the tree buffer's size: below lsm_level_get_tree_bytes(nfile, tree_nidx) (a
 * tree built for fewer tables) the call returns LSM_ESPACE.  A tree built for
 * an earlier state of the level with the same shape cannot be detected: the
 * caller rebuilds it whenever the level's tables change, as it re-decodes
 * them. */
enum lsm_get_result {
    LSM_GET_ABSENT = 0,         /* (nil, nil): not MayContain, or no entry equals the key        */
    LSM_GET_FOUND = 1,          /* the value, d_value[i]                                          */
    LSM_GET_SEEK_FAILED = 2,    /* negative offset: sstable.go:284-287 "seek to offset failed"  */
    LSM_GET_VALUE_LENGTH = 3,   /* < 4 bytes left: kv.go:183-186 "decode value length"          */
    LSM_GET_VALUE_TOO_LONG = 4, /* kv.go:188-190 "invalid value length: %d" (> 1<<30)           */
    LSM_GET_VALUE_SHORT = 5,    /* kv.go:192-196 "decode value"                                  */
};
int lsm_level_get(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                  const uint64_t *d_file_len, const lsm_sst_meta *d_meta, uint32_t nfile,
                  const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                  const int64_t *d_idx_value, const uint8_t *d_keys, const uint64_t *d_koff,
                  uint64_t nkeys, const int32_t *d_table, const uint8_t *d_may, int32_t *d_result,
                  lsm_rec_desc *d_value, const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
                  void *stream);

/* The whole batched Get of one level >= 1 in one call (ABI 7):
 * Manager.searchFromLevelWithSparseIndex (manager.go:178-207) and
 * searchFromTable (:209-223) -- lsm_level_may_contain_indexed's outputs
 * (d_table, d_may) and lsm_level_get's (d_result, d_value) for the same
 * inputs, queued on one stream.  d_index: lsm_level_index_build; the decode
 * outputs and the tree as lsm_level_get.  Workspace:
 * lsm_level_may_contain_workspace_bytes. */
int lsm_level_search_get(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index, uint32_t nfile,
                         const uint64_t *d_file_off, const uint64_t *d_file_len,
                         const lsm_sst_meta *d_meta, const uint64_t *d_rec_base,
                         const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
                         const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                         int32_t *d_table, uint8_t *d_may, int32_t *d_result, lsm_rec_desc *d_value,
                         const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
                         void *d_workspace, size_t ws_bytes, void *stream);

/* Batched Manager.searchFromLevel0 (sstable/manager.go:160-176) for level 0,
 * whose tables overlap: the nfile images are the level's tables in the
 * Manager's order (newest first -- addNewSSTables prepends, manager.go:
 * 284-287), with lsm_decode_sst's outputs as for lsm_level_get.  Per key i,
 * searchFromTable (:209-223) on table 0, 1, ...: MayContain (sstable.go:
 * 300-305: the range check, then Filter.Test), Iterator.Seek, the value; a
 * false positive or a Seek miss goes on to the next table, the first value or
 * error ends the search (`return nil, err`).  d_table[i] = the table that
 * answered (LSM_GET_FOUND or an error code in d_result[i], the value's view
 * in d_value[i] as lsm_level_get), -1 with LSM_GET_ABSENT when none did.
 * MayContain's deviations are lsm_may_contain's (corrupted filters only).
 * d_tree / tree_nidx / tree_bytes as lsm_level_get (the level-0 tables'
 * Seek tree, or NULL). */
int lsm_level0_get(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                   const uint64_t *d_file_len, const lsm_sst_meta *d_meta, uint32_t nfile,
                   const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc,
                   const int64_t *d_idx_value, const uint8_t *d_keys, const uint64_t *d_koff,
                   uint64_t nkeys, int32_t *d_table, int32_t *d_result, lsm_rec_desc *d_value,
                   const void *d_tree, uint32_t tree_nidx, size_t tree_bytes, void *stream);

/* Batched Manager.Search (sstable/manager.go:99-133) over a whole tree in one
 * asynchronous call (added within ABI 7): what database.Get reaches the
 * SSTables through.  The tree is one table list of nfile = level_start[7]
 * images in one d_img, decoded by one lsm_decode_sst; tables
 * [level_start[L], level_start[L + 1]) are level L (level_start is a HOST
 * array of LSM_SEARCH_LEVELS + 1 entries, level_start[0] = 0, non-decreasing
 * or the call returns LSM_EINVAL; go-lsm's 2^(L+1) cap per level is not
 * enforced).  Level 0 is in the Manager's order, newest first, as for
 * lsm_level0_get; each level >= 1 is in sparse-index order, as for
 * lsm_level_may_contain.  d_index is lsm_level_index_build over the whole
 * list, d_tree lsm_level_get_tree_build over the whole list (or NULL); both
 * work per table.  Per key i: level 0 as searchFromLevel0 (:160-176), then
 * each non-empty level 1..6 as searchFromLevelWithSparseIndex +
 * searchFromTable (:178-223); the first result other than LSM_GET_ABSENT -- a
 * value or any error code -- ends that key's search.  A found value that is
 * empty or the tombstone bytes (kv.go:29-31) is a found value: Search and
 * database.Get do not interpret it.  waitForCompactionIfNeeded is host locking
 * and stays with the binding.  Corrupted tables answer as in lsm_level0_get
 * (level 0) and lsm_level_may_contain (levels >= 1).
 * d_result[i] / d_value[i] as lsm_level_get; d_table[i] = the answering
 * table's index in the tree's list and d_level[i] its level, both -1 when the
 * key is absent.  nkeys == 0 returns 0; an empty tree answers every key
 * absent; LSM_ESPACE for a workspace or a tree buffer that is too small.
 * One launch whatever the tree's depth and nkeys: one thread per key runs the
 * whole of Search -- the key hashed once, a deeper level searched only while
 * the key is unanswered, so no work is spent on keys an earlier level
 * answered.  No host round trip, no read-back (the call can be captured in a
 * graph) and no device allocation.
 * Workspace: lsm_search_workspace_bytes = 256 for every non-empty tree and
 * every nkeys (0 for an empty tree, or a level_start that does not start at 0
 * or decreases): a thread holds its key's whole state, nothing per probe is
 * kept between launches.  The buffer is reserved for a grouped form of the
 * search; a smaller one returns LSM_ESPACE. */
#define LSM_SEARCH_LEVELS 7 /* minSSTableLevel .. maxSSTableLevel, manager.go:21-22 */
size_t lsm_search_workspace_bytes(const uint32_t *level_start, uint64_t nkeys);
int lsm_search(lsm_ctx *ctx, const uint8_t *d_img, const void *d_index,
               const uint32_t *level_start, /* HOST, LSM_SEARCH_LEVELS + 1 entries */
               const uint64_t *d_file_off, const uint64_t *d_file_len, const lsm_sst_meta *d_meta,
               const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
               const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
               int32_t *d_level, int32_t *d_table, int32_t *d_result, lsm_rec_desc *d_value,
               const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
               void *d_workspace, size_t ws_bytes, void *stream);

/* Batched range scan over a whole tree in one asynchronous call (added within
 * ABI 7): the ordered read go-lsm's iterators add up to -- sstable.Iterator
 * (sstable/iterator.go:9-73) over block.Iterator.Seek / Next / Valid / Key /
 * ValueOffset (sstable/block/index.go:157-181), the shape database.Iterator
 * (database/iterator.go) declares.  The tree is lsm_search's, argument for
 * argument.  For each of nq ranges [lo, hi) in Go string order (CSR: lo of
 * range q is d_lo[d_lo_off[q] .. d_lo_off[q + 1]), hi likewise; input-slack
 * contract; d_flags[q] & LSM_SCAN_NO_UPPER: no upper bound, hi is ignored) it
 * returns up to `limit` entries in ascending key order, each key once,
 * answered by the table Manager.Search (manager.go:99-133) answers it from:
 * the scan of a range is Search applied to every key the tree holds in it.
 *   Which tables take part: table t that Go would have loaded and that has
 *     entries -- d_meta[t].stage is LSM_SST_OK, LSM_SST_DATA or
 *     LSM_SST_MISMATCH, and nidx > 0.  SSTable.DecodeFrom (sstable.go:101-125)
 *     reads header, filter, footer and index; the data block is read only for
 *     compaction, so a table with a damaged data block is in the Manager,
 *     Search and lsm_search answer from it, and so does the scan.  Stages 1-4
 *     are DecodeFrom's failures: such a table is in no Manager and stays out.
 *     A table's entries are the nidx index entries the decode kept, in index
 *     order.  A level-0 table is one source; level 0's sources come in
 *     the tree's order (newest first), then the levels in order.  The tables
 *     of a level >= 1 that take part form one source, walked one after the
 *     other in sparse-index order.
 *   The Seek: a table is entered by Iterator.Seek(lo), Go's bisection for the
 *     first entry with key >= lo (index.go:157-181) -- the bisection
 *     lsm_level_get runs, through the Seek tree or over the index, so d_tree
 *     == NULL and a tree give identical output (a tree buffer below
 *     lsm_level_get_tree_bytes(nfile, tree_nidx): LSM_ESPACE).  In a level
 *     >= 1 the table entered is the one the sparse index picks (manager.go:
 *     186-192); a Seek that runs off its end goes on at entry 0 of the next
 *     table.
 *   Which source answers: the first source, in the order above, that holds
 *     the key -- Search's order.  The filters are not consulted: the Builder
 *     added every key of a table's index to its filter.  Deviation: with a
 *     corrupted filter lsm_search can miss a key that the scan returns.
 *   The boundary key: within a level >= 1 a key can be both the last key of
 *     table f and the first of table f + 1 (the merge forgets the last written
 *     key at every flush, merge.go:57-85, so compaction outputs do this).  The
 *     entry of f + 1 answers, once: f + 1 is the table the sparse index picks
 *     for the key, so it is what Search returns, though it is the older pair.
 *   Preconditions: every participating table's index is strictly ascending;
 *     the tables of a level >= 1 are in MinKey order with ranges that meet at
 *     most in one boundary key.  Outside them the output is unspecified, but
 *     every access stays inside the caller's buffers and every walk ends.
 *   Emission: entry j of range q is at q * limit + j.  d_key = the answering
 *     index entry's descriptor as d_idx_desc holds it {rec_off into d_img,
 *     key_len, val_len = 8}; d_table = the answering table's position in the
 *     tree's list; d_result / d_value exactly lsm_level_get's for that entry
 *     (GetValueByOffset, sstable.go:271-296): LSM_GET_FOUND with the value's
 *     view, or an error code with a zero view -- an entry whose value read
 *     fails is emitted with its code, as Search returns that error for the
 *     key.  d_key / d_value are what lsm_gather_kvs takes as d_key_desc /
 *     d_val_desc.
 *   Modes: LSM_SCAN_RAW -- a value of exactly the 13 tombstone bytes (kv.go:
 *     29-31) is an ordinary value, as for Search.  LSM_SCAN_LIVE -- a key whose
 *     answering entry is LSM_GET_FOUND with exactly those bytes is not emitted
 *     and does not count towards limit.  In both the tombstone hides the key
 *     in every later source.
 *   Counts: d_count[q] <= limit entries were emitted; d_more[q] = 1 exactly
 *     when the walk stopped at limit and a further key of the range would
 *     have been emitted in this mode (LIVE: a tail of tombstones gives 0).
 *     Slots j >= d_count[q] are unspecified.  An empty range (lo >= hi) and an
 *     empty tree give count 0, more 0.
 * Checks, in this order, before any launch: ctx == NULL -> LSM_EINVAL; nq == 0
 * -> 0, nothing written; LSM_EINVAL for a level_start that does not start at 0
 * or decreases, limit == 0, nq * limit >= 2^32, an unknown mode, a NULL d_lo /
 * d_lo_off / d_hi / d_hi_off / d_flags or output pointer, a non-empty tree
 * with a NULL tree input other than d_rec_base / d_tree; LSM_ESPACE for the
 * tree buffer or the workspace.  Workspace: lsm_tree_scan_workspace_bytes =
 * 32 bytes per range and source (a source per level-0 table and one per level
 * 1..6), 0 for an empty tree or a level_start that does not start at 0 or
 * decreases.  Two launches on the stream: the Seeks, one thread per range and
 * source, leave each source's first entry in the workspace; the walk runs a
 * wave per range with a lane per source, any level-0 width (past 64 sources
 * the lanes' cursors stay in the workspace).  No host synchronisation, no
 * read-back, no device allocation, no pointer kept. */
enum lsm_scan_mode { LSM_SCAN_RAW = 0, LSM_SCAN_LIVE = 1 };
#define LSM_SCAN_NO_UPPER 1u /* bit 0 of d_flags[q]: the range has no upper bound, hi is ignored */
size_t lsm_tree_scan_workspace_bytes(const uint32_t *level_start, uint64_t nq);
int lsm_tree_scan(lsm_ctx *ctx,
                  /* the tree: exactly lsm_search's inputs, with the same meaning */
                  const uint8_t *d_img, const void *d_index,
                  const uint32_t *level_start, /* HOST, LSM_SEARCH_LEVELS + 1 entries */
                  const uint64_t *d_file_off, const uint64_t *d_file_len, const lsm_sst_meta *d_meta,
                  const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
                  const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
                  /* the ranges: [lo, hi) in Go string order, CSR, input-slack contract */
                  const uint8_t *d_lo, const uint64_t *d_lo_off, const uint8_t *d_hi,
                  const uint64_t *d_hi_off, const uint8_t *d_flags, uint64_t nq, uint32_t limit, int mode,
                  /* outputs: range q's entries at [q * limit, q * limit + d_count[q]) */
                  uint32_t *d_count, uint8_t *d_more, lsm_rec_desc *d_key, lsm_rec_desc *d_value,
                  int32_t *d_table, int32_t *d_result,
                  void *d_workspace, size_t ws_bytes, void *stream);

/* database.Get (database/database.go:24-40) of nkeys keys in one asynchronous
 * call: lsm_memtable_search over the memtables (its arguments, d_mem_index /
 * mem_index_bytes being its d_index / index_bytes), then lsm_search (its
 * arguments) for the keys the memtables did not answer.
 *   LSM_DBGET_EXACT: Get as written -- `if value != nil return value`, else
 *     SSTables.Search.  A key goes on to the tables unless its memtable result
 *     is LSM_MEM_VALUE: a key whose memtable answer is a tombstone is searched
 *     in the tables and can come back with an older value, or with a table's
 *     tombstone bytes as an ordinary value.  What go-lsm does today; exact in
 *     the sense of LSM_TIE_GOHEAP and LSM_MEMTABLE_RANGESCAN.
 *   LSM_DBGET_TOMBSTONE_HIDES: only LSM_MEM_MISS goes on.  A LSM_MEM_DELETED
 *     key ends with d_src = LSM_SRC_MEMTABLE, d_result = LSM_GET_ABSENT and a
 *     zero value.  The recommended mode.
 * Any other mode returns LSM_EINVAL.
 * d_mem_result / d_log / d_slot: lsm_memtable_search's, for every key.
 * d_level / d_table / d_result: lsm_search's for the keys that went on, error
 * codes included; -1, -1, LSM_GET_ABSENT for the others.  d_value[i] = the
 * returned value's view and d_src[i] the buffer it points into:
 * LSM_SRC_MEMTABLE (d_bytes), LSM_SRC_SSTABLE (d_img; also for a table's error
 * code, with a zero view), LSM_SRC_NONE when Get returns (nil, nil).
 * A key the memtables answered costs no table work (no hash, no filter test,
 * no Seek): lsm_search's kernel, instantiated with the memtable result as a
 * per-key input, skips it.  nlog == 0 reduces to lsm_search's answers, an
 * empty tree to the memtables'.  Two launches; no host synchronisation, no
 * read-back, no device allocation (capturable).  Checks: ctx == NULL or an
 * unknown mode -> LSM_EINVAL; nkeys == 0 -> 0; then lsm_search's and
 * lsm_memtable_search's.  Workspace: lsm_db_get_workspace_bytes (lsm_search's;
 * LSM_ESPACE below it). */
enum lsm_db_get_mode { LSM_DBGET_EXACT = 0, LSM_DBGET_TOMBSTONE_HIDES = 1 };
enum lsm_get_source { LSM_SRC_NONE = -1, LSM_SRC_MEMTABLE = 0, LSM_SRC_SSTABLE = 1 };
size_t lsm_db_get_workspace_bytes(const uint32_t *level_start, uint64_t nkeys);
int lsm_db_get(lsm_ctx *ctx,
               /* the memtables: lsm_memtable_search's inputs */
               const uint8_t *d_bytes, const lsm_rec_desc *d_desc, const uint32_t *d_idx,
               const uint64_t *d_file_start, uint32_t nlog, const void *d_mem_index,
               size_t mem_index_bytes,
               /* the tree: lsm_search's inputs */
               const uint8_t *d_img, const void *d_index,
               const uint32_t *level_start, /* HOST, LSM_SEARCH_LEVELS + 1 entries */
               const uint64_t *d_file_off, const uint64_t *d_file_len, const lsm_sst_meta *d_meta,
               const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
               const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
               const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys, int mode,
               int32_t *d_mem_result, int32_t *d_log, uint32_t *d_slot, int32_t *d_level,
               int32_t *d_table, int32_t *d_result, lsm_rec_desc *d_value, int32_t *d_src,
               void *d_workspace, size_t ws_bytes, void *stream);

/* Batched range scan over the memtables and the tree in one asynchronous call
 * (added within ABI 7): lsm_tree_scan with the memtables in front, the step
 * that took lsm_search to lsm_db_get.  The memtables are lsm_memtable_search's
 * inputs (logs OLDEST FIRST, d_mem_index / mem_index_bytes its d_index /
 * index_bytes), the tree is lsm_search's, argument for argument, the ranges,
 * limit and mode are lsm_tree_scan's.  With an empty tree it is the batched
 * memtable range query (memtable/iterator.go leaves that as a TODO).
 *   Sources, in answering order: the memtable of log nlog - 1 (Mem), then logs
 *     nlog - 2 .. 0 -- memtable.Manager.Search's order (memtable/manager.go:
 *     61-74) -- then lsm_tree_scan's sources, unchanged: each level-0 table in
 *     the tree's order, then one source per level 1..6.  Source s < nlog is log
 *     nlog - 1 - s.  A log with no nodes (failed, empty or overflowed:
 *     d_file_start[w] == d_file_start[w + 1]) is a source that never has a
 *     head.
 *   The memtable Seek: a memtable source is entered at its first node with key
 *     >= lo, the lower bound over d_idx[d_file_start[w] .. d_file_start[w + 1]),
 *     and advances node by node in d_idx order.  d_idx must be the
 *     LSM_MEMTABLE_ALL order; a LSM_MEMTABLE_RANGESCAN order is a subset and
 *     cannot be detected (lsm_memtable_search's caveat).
 *   Which source answers: each key is emitted once, from the first source in
 *     that order that holds it.  As the existing calls: the scan of a range
 *     is, for every distinct key any source holds in [lo, hi),
 *     lsm_memtable_search's answer when that is not LSM_MEM_MISS, else
 *     lsm_search's.
 *   Modes (lsm_scan_mode): LSM_SCAN_RAW -- a tombstone is an ordinary value;
 *     for a memtable node d_value is the view of its 13 bytes
 *     (lsm_memtable_search zeroes that view, the scan does not).
 *     LSM_SCAN_LIVE -- a key whose answering entry is a tombstone (a memtable
 *     node with exactly kv.DeletedValue, or a table entry that is
 *     LSM_GET_FOUND with those bytes) is not emitted and does not count
 *     towards limit.  In both the tombstone hides the key in every later
 *     source.  A replayed empty value (key, "") is a found value of length 0 in
 *     both modes, as lsm_memtable_search documents.
 *   Emission at slot o = q * limit + j: d_src[o] = LSM_SRC_MEMTABLE or
 *     LSM_SRC_SSTABLE.  A memtable entry: d_key[o] = d_desc[slot] verbatim (the
 *     KV descriptor into d_bytes), d_value[o] = {rec_off + 4 + key_len, 0,
 *     val_len}, d_table[o] = the log w, d_result[o] = LSM_GET_FOUND.  A table
 *     entry: exactly lsm_tree_scan's four outputs.  d_count / d_more as in
 *     lsm_tree_scan (LIVE: a tail of tombstones gives more = 0); slots past
 *     d_count[q] are unspecified.
 *   Deviation: skiplist.Iterator skips deleted nodes in Seek and its Valid()
 *     is false at a tombstone (skiplist/iterator.go:49-70), so a `for Valid()`
 *     loop stops at the first tombstone -- the quirk LSM_MEMTABLE_RANGESCAN
 *     restates for the flush.  go-lsm has no database iterator to be exact to,
 *     so the scan offers no "exact" mode: every node takes part.
 *   Degenerate inputs: nlog == 0 gives lsm_tree_scan's outputs with d_src =
 *     LSM_SRC_SSTABLE; an empty tree scans the memtables alone (the tree
 *     pointers may be NULL); with both empty d_count and d_more are zeroed by
 *     memsets and the call returns 0.
 * Checks, in this order, all before any launch: ctx == NULL -> LSM_EINVAL; nq
 * == 0 -> 0, nothing written; LSM_EINVAL for a level_start that does not start
 * at 0 or that decreases, limit == 0, nq >= 2^32 or nq * limit >= 2^32, an
 * unknown mode, nlog > 65535, a NULL range, flag or output pointer (d_src
 * included), nlog > 0 with a NULL d_bytes / d_desc / d_idx / d_file_start, a
 * non-empty tree with a NULL tree input other than d_rec_base / d_tree;
 * LSM_ESPACE for d_mem_index != NULL with mem_index_bytes below
 * lsm_memtable_search_index_bytes(1), a tree buffer below
 * lsm_level_get_tree_bytes(nfile, tree_nidx), a NULL or short workspace.
 * Workspace: lsm_db_scan_workspace_bytes = 32 * nq * (nlog + level_start[1] +
 * 6) bytes when nlog + nfile > 0 (a head per range and source); 0 when both
 * are empty or level_start is bad; SIZE_MAX when the product leaves 64 bits.
 * Two launches on the stream: the Seeks, one thread per range and source (a
 * memtable thread bisects its log's nodes, through the index where the log
 * lies inside the indexed count), then the walk, a wave per range and a lane
 * per source, any width.  No host synchronisation, no read-back, no device
 * allocation, no pointer kept (capturable).  d_mem_index and d_tree are
 * optional; the output is identical with and without each. */
size_t lsm_db_scan_workspace_bytes(uint32_t nlog, const uint32_t *level_start, uint64_t nq);
int lsm_db_scan(lsm_ctx *ctx,
                /* the memtables: lsm_memtable_search's inputs, logs OLDEST FIRST */
                const uint8_t *d_bytes, const lsm_rec_desc *d_desc, const uint32_t *d_idx,
                const uint64_t *d_file_start, uint32_t nlog, const void *d_mem_index,
                size_t mem_index_bytes,
                /* the tree: lsm_search's inputs, argument for argument */
                const uint8_t *d_img, const void *d_index,
                const uint32_t *level_start, /* HOST, LSM_SEARCH_LEVELS + 1 entries */
                const uint64_t *d_file_off, const uint64_t *d_file_len, const lsm_sst_meta *d_meta,
                const uint64_t *d_rec_base, const lsm_rec_desc *d_idx_desc, const int64_t *d_idx_value,
                const void *d_tree, uint32_t tree_nidx, size_t tree_bytes,
                /* the ranges: lsm_tree_scan's */
                const uint8_t *d_lo, const uint64_t *d_lo_off, const uint8_t *d_hi,
                const uint64_t *d_hi_off, const uint8_t *d_flags, uint64_t nq, uint32_t limit, int mode,
                /* outputs: range q's entries at [q * limit, q * limit + d_count[q]) */
                uint32_t *d_count, uint8_t *d_more, lsm_rec_desc *d_key, lsm_rec_desc *d_value,
                int32_t *d_src, int32_t *d_table, int32_t *d_result,
                void *d_workspace, size_t ws_bytes, void *stream);

/* The answered bytes of a batched read packed into two CSR arenas, in one
 * asynchronous call (added within ABI 7): what turns the views lsm_search,
 * lsm_db_get, lsm_tree_scan and lsm_db_scan return into bytes a host fetches
 * with two D2H copies, with no host copy of the logs or the images.
 *   Slots and entries: the input is nrow rows of `limit` slots, slot o = q *
 *     limit + j.  A slot is live when j < min(d_count[q], limit) (a count above
 *     limit is clamped); with d_count == NULL every slot is live.  The Get shape
 *     is nrow = nkeys, limit = 1, d_count = NULL: entry e is key e, whatever it
 *     answered.  The live slots are numbered densely as entries, rows in order
 *     and j ascending within a row: d_row_start[q] = the first entry of row q,
 *     d_row_start[nrow] = E; d_entry_slot[e] = o when that array is given (what
 *     picks d_table / d_result / d_src for the entries).  The descriptors and
 *     the source word of a slot that is not live are never read.
 *   Bytes of an entry: the source is d_src ? d_src[o] : LSM_SRC_SSTABLE, the
 *     base d_bytes for LSM_SRC_MEMTABLE and d_img for LSM_SRC_SSTABLE.  Any
 *     other source (LSM_SRC_NONE), or a source whose base is NULL, gives the
 *     entry a key and a value of length 0; it is still an entry.  Otherwise the
 *     key is d_key[o].key_len bytes at base + d_key[o].rec_off + 4 (the IDX
 *     descriptor lsm_tree_scan emits, and the KV descriptor lsm_db_scan emits
 *     for a memtable node), the value d_value[o].val_len bytes at base +
 *     d_value[o].rec_off + 4 (lsm_level_get's view).  A zero view (a miss, a
 *     tombstone of lsm_memtable_search, an error code) packs nothing; a length
 *     of 0 issues no source load.  d_key == NULL: keys are not packed (d_koff
 *     and d_keys are not touched, d_counts[1] = 0).
 *   Offsets and counts: d_koff / d_voff (E + 1 entries written, nrow * limit +
 *     1 allocated) are the exclusive scans of those lengths over the entries,
 *     d_koff[E] = K, d_voff[E] = V; key e is d_keys[d_koff[e] .. d_koff[e+1]),
 *     values alike -- a CSR batch as lsm_encode_blocks or lsm_build_sst_stream
 *     read.  d_counts = {E, K, V, overflow}.
 *   Capacity: if d_keys != NULL and K > key_cap, or d_vals != NULL and V >
 *     val_cap, d_counts[3] = 1 and no byte of either arena is written; the
 *     offsets, d_row_start, d_entry_slot and d_counts[0..2] are written in full
 *     all the same.  A NULL arena is skipped and its cap ignored; with both
 *     NULL the call is the sizing call.  Bytes outside [0, K) of d_keys and
 *     [0, V) of d_vals are never written: the arenas need no slack.  The
 *     sources are under the input-slack contract.
 *   Preconditions: every live view lies inside its buffer (the four producers
 *     guarantee that); offsets are not validated.  d_keys and d_vals are 16-byte
 *     aligned, as every device allocation is (the copy stores 16-byte chunks
 *     aligned in the arena); the sources may have any alignment.
 * Checks, in this order, all before any launch: ctx == NULL -> LSM_EINVAL; nrow
 * == 0 -> 0, nothing written; LSM_EINVAL for limit == 0, nrow * limit >= 2^32,
 * a NULL d_value / d_row_start / d_voff / d_counts, d_key != NULL with d_koff
 * == NULL, d_keys != NULL with d_key == NULL, d_src == NULL with d_img == NULL;
 * LSM_ESPACE for a NULL or short workspace.
 * Workspace, with n = nrow * limit, t = ceil(n / 512) + 1 and r(x) = x rounded
 * up to 256: lsm_pack_results_workspace_bytes = r(16 * t) + r(8 * t) + 2 * r(8
 * * n) (the scan's tile sums -- byte sums and live counts -- and each entry's
 * two source addresses); 0 for nrow == 0 or limit == 0; SIZE_MAX when the
 * product or the formula leaves 64 bits.
 * Five launches on the stream, four for the sizing call: the tile sums of
 * {live, key bytes, value bytes} over the slots, the scan of the tile sums
 * (two launches: the byte sums, the live counts), the slots' scan (entries,
 * offsets, row starts, counts and the overflow flag), then the copy, a wave
 * per 64 entries (it compares the totals with the caps itself).  No host
 * synchronisation, no read-back, no device allocation, no pointer kept
 * (capturable). */
size_t lsm_pack_results_workspace_bytes(uint64_t nrow, uint32_t limit);
int lsm_pack_results(lsm_ctx *ctx,
                     const uint8_t *d_bytes,    /* what LSM_SRC_MEMTABLE views point into (may be NULL) */
                     const uint8_t *d_img,      /* what LSM_SRC_SSTABLE views point into (may be NULL)  */
                     const int32_t *d_src,      /* per slot, lsm_get_source; NULL = every slot LSM_SRC_SSTABLE */
                     const lsm_rec_desc *d_key, /* per slot, or NULL: keys are not packed */
                     const lsm_rec_desc *d_value, /* per slot, required */
                     const uint32_t *d_count,   /* per row, or NULL: every row holds `limit` live slots */
                     uint64_t nrow, uint32_t limit,
                     uint8_t *d_keys, uint64_t key_cap, uint8_t *d_vals, uint64_t val_cap,
                     uint64_t *d_row_start,     /* nrow + 1 */
                     uint32_t *d_entry_slot,    /* optional, nrow * limit */
                     uint64_t *d_koff, uint64_t *d_voff, /* nrow * limit + 1 each; d_koff optional iff d_key == NULL */
                     uint64_t *d_counts,        /* 4: {entries E, key bytes K, value bytes V, overflow} */
                     void *d_workspace, size_t ws_bytes, void *stream);

/* database.Put / database.Delete (database/database.go:42-59) of a batch of n
 * operations in one asynchronous call: the write-ahead logs go-lsm would
 * append, byte for byte, with memtable rotation, and the descriptors
 * lsm_wal_replay would return for them ("The write side").
 * The batch is CSR with the input-slack contract: op i has key
 * d_keys[d_koff[i] .. d_koff[i+1]), value d_vals[d_voff[i] .. d_voff[i+1]) and
 * kind d_op[i] (0 = Put, anything else = Delete; a Delete's value range is
 * ignored).  Ops apply in order to the current memtable, whose sizeInBytes
 * (memtable.go:112-121) is mem_size0 on entry; est(pair) = 16 + len(key) +
 * len(value) (kv.go:118-121); mem_max is maxMemoryTableSize.
 *   Put (manager.go:40-59): when size + est > mem_max the memtable is promoted
 *     and an empty one takes over; then the pair is appended and size += est.
 *   Delete (manager.go:76-106): when the memtable current BEFORE any promotion
 *     holds the key, (key, nil) -- klen | key | vlen = 0 -- is appended to its
 *     log, size unchanged (memtable.go:84-96); then (key, kv.DeletedValue) is
 *     put like any pair (est = 16 + len(key) + 13).
 * Log 0 is the memtable current on entry (it holds no op when op 0 does not
 * fit); every further log holds its first op however large.  A key is in a
 * memtable exactly when its log holds a record of the key, or, for log 0,
 * when it is one of the nodes passed in: d_cur_idx[0 .. cur_nnode) =
 * lsm_memtable_order(LSM_MEMTABLE_ALL)'s d_idx slice of that one log (slots in
 * key order) over d_cur_bytes / d_cur_desc; NULL or cur_nnode == 0 = empty.
 * Outputs, for s < nlog = d_counts[0]:
 *   log s = d_wal[d_wal_off[s] .. + d_wal_len[s]); d_wal_off[s + 1] =
 *     d_wal_off[s] + roundup(d_wal_len[s], align), so every log starts at a
 *     multiple of align and the bytes between logs are untouched;
 *   d_log_start[s] = the first op of log s (d_log_start[nlog] = n);
 *   d_rec_base[s] = the records of the logs before s (d_rec_base[nlog] = all);
 *   d_desc (optional, 2n entries): record r of log s at slot d_rec_base[s] + r,
 *     rec_off relative to d_wal -- lsm_wal_replay's rec_base placement, which
 *     lsm_memtable_order, lsm_memtable_search and lsm_db_get take as they are
 *     (nrec[s] = d_rec_base[s + 1] - d_rec_base[s], status 0);
 *   d_main_slot[i] (optional): the slot of op i's Put / tombstone record (a
 *     Delete's (key, nil) record, when it has one, is the slot before);
 *   d_counts = {nlog, records, bytes = d_wal_off[nlog], overflow, most records
 *     in one log, sizeInBytes of log nlog - 1 after the batch (the next call's
 *     mem_size0)}.
 * Logs s < nlog - 1 are promoted memtables; evicting and flushing the 11th
 * (promoteLocked), file ids and I/O stay with the caller.
 * nlog_max < the logs the rule needs: d_counts = {0, 0, 0, 1, 0, 0} and no
 * other output is promised (as lsm_segment_files).  lsm_db_write_max_logs
 * always suffices; lsm_db_write_out_bytes bounds d_counts[2] from host-known
 * sums (key_bytes = d_koff[n], val_bytes = d_voff[n]).  nlog_max and mem_max
 * also size the presence launches (nlog_max logs of up to mem_max / 16 ops):
 * pass the bound, not 65535.
 * Checks, in this order, before any launch: ctx == NULL -> LSM_EINVAL; n == 0
 * -> 0, nothing written; LSM_EINVAL for a NULL d_keys, d_koff, d_vals, d_voff,
 * d_op, d_wal, d_log_start, d_wal_off, d_wal_len, d_rec_base or d_counts,
 * mem_max == 0 or > 1 << 30, align == 0, n >= 2^31, nlog_max == 0 or > 65535,
 * d_cur_idx != NULL with a NULL d_cur_bytes or d_cur_desc;
 * then LSM_ESPACE for a NULL or short workspace.  No host synchronisation, no
 * read-back, no device allocation (capturable); no pointer is kept. */
enum lsm_write_op { LSM_OP_PUT = 0, LSM_OP_DELETE = 1 };
uint32_t lsm_db_write_max_logs(uint64_t n, uint64_t key_bytes, uint64_t val_bytes, uint64_t mem_size0,
                               uint64_t mem_max);
uint64_t lsm_db_write_out_bytes(uint64_t n, uint64_t key_bytes, uint64_t val_bytes, uint32_t nlog_max,
                                uint32_t align);
size_t lsm_db_write_workspace_bytes(uint64_t n, uint32_t nlog_max, uint64_t mem_max);
int lsm_db_write(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff, const uint8_t *d_vals,
                 const uint64_t *d_voff, const uint8_t *d_op, uint64_t n, uint64_t mem_size0,
                 uint64_t mem_max, const uint8_t *d_cur_bytes, const lsm_rec_desc *d_cur_desc,
                 const uint32_t *d_cur_idx, uint64_t cur_nnode, uint32_t nlog_max, uint32_t align,
                 uint8_t *d_wal, uint64_t *d_log_start, uint64_t *d_wal_off, uint32_t *d_wal_len,
                 lsm_rec_desc *d_desc, uint64_t *d_rec_base, uint32_t *d_main_slot, uint64_t *d_counts,
                 void *d_workspace, size_t ws_bytes, void *stream);

/* The Seek tree of a level for lsm_level_get, built once when the level is
 * loaded (the Manager keeps each table's decoded IndexBlock in memory,
 * manager.go:226-275; Seek bisects it, index.go:157-181).  Go's bisection
 * over n entries visits a fixed tree of midpoints whatever the keys hold; the
 * tree stores, per table, each midpoint's 16-byte key prefix and length in
 * 128-byte blocks of three levels, so a Seek reads one line per three steps.
 * Tables with nidx <= max_nidx are built; lsm_level_get_tree_bytes(nfile,
 * max_nidx) bytes (about 18 per entry at max_nidx).  Asynchronous. */
size_t lsm_level_get_tree_bytes(uint32_t nfile, uint32_t max_nidx);
int lsm_level_get_tree_build(lsm_ctx *ctx, const uint8_t *d_img, const uint64_t *d_file_off,
                             const lsm_sst_meta *d_meta, uint32_t nfile, const uint64_t *d_rec_base,
                             const lsm_rec_desc *d_idx_desc, uint32_t max_nidx, void *d_tree,
                             size_t tree_bytes, void *stream);

/* ---- encode ---------------------------------------------------------------- */

/* Batch encode of a columnar record batch (CSR: record i's key is
 * d_keys[d_koff[i] .. d_koff[i+1]), value d_vals[d_voff[i] .. d_voff[i+1])).
 * Block b holds records [rec_start[b], rec_start[b+1]) and is written
 * contiguously at d_out + out_off[b]; bytes between blocks are untouched.
 * Replaces KeyValuePair.EncodeTo (kv.go:46-74), DataBlock.EncodeTo
 * (data.go:26-45 / Value.EncodeTo kv.go:165-178) and IndexBlock.Encode
 * (index.go:47-58; d_idx_off[i] is record i's i64 offset, IDX only). */
uint64_t lsm_encoded_size_host(int grammar, const uint64_t *koff, const uint64_t *voff,
                               uint64_t r0, uint64_t r1);
int lsm_encode_blocks(lsm_ctx *ctx, int grammar, const uint8_t *d_keys, const uint64_t *d_koff,
                      const uint8_t *d_vals, const uint64_t *d_voff, const int64_t *d_idx_off,
                      const uint64_t *d_rec_start, uint32_t nblk, uint8_t *d_out,
                      const uint64_t *d_out_off, void *stream);

/* ---- .sst build (builder path + fused bloom) ------------------------------ */

/* Builder flush rule on host-resident CSR offsets: Builder.Add/ShouldFlush
 * (builder.go:34-42, EstimateSize kv.go:118-121) as driven by
 * CompactAndMergeKVs (merge.go:106-123).  threshold 0 = never flush
 * (BuildSSTableFromIMemTable builder.go:22-31); go-lsm uses 2 MiB
 * (sstable.go:21).  Writes file_start[0..nfile] (file_start[nfile] = n);
 * returns nfile.  file_start must hold n+1 entries. */
uint64_t lsm_segment_files_host(const uint64_t *koff, const uint64_t *voff, uint64_t n,
                                uint64_t threshold, uint64_t *file_start);
/* Exact .sst image size of records [r0, r1) (host-resident CSR offsets). */
uint64_t lsm_sst_image_size_host(const uint64_t *koff, const uint64_t *voff, uint64_t r0,
                                 uint64_t r1, uint64_t m);
/* Filter block bytes for m bits: 8 + 24 + 8*ceil(m/64) (bloom.go:472-491). */
uint64_t lsm_filter_block_size(uint64_t m);
/* Device workspace lsm_build_sst needs for nfile files of at most
 * max_file_records records each: when the filter splits into two LDS slices
 * (go-lsm's default m), a 16-byte hash record per key (k <= 16: the key hash
 * runs inside the region writer) or the slice-1 bit positions (k u32 per
 * record); else a token 16 bytes. */
size_t lsm_build_sst_workspace_bytes(uint32_t nfile, uint32_t max_file_records, uint64_t m,
                                     uint32_t k);

/* Build nfile .sst images: file f holds records [file_start[f], file_start[f+1])
 * and its image (Header | Filter | V data | IDX index | Footer) is written at
 * d_out + file_off[f].  Replaces Builder.Add/Build (builder.go:34-59),
 * SSTable.Add (sstable.go:322-326), bloom Filter.Add (bloom.go:175-181,
 * murmur.go:245-275) and SSTable.EncodeTo (sstable.go:131-193).  The bloom
 * (m bits, k hashes; go-lsm default 1,600,000 / 16, bloom.go:79-82) is
 * built in LDS slices and its words are stored straight into each image;
 * for the default shape each key is hashed by the kernel that writes its
 * index entry.
 * d_footer (optional) gets {dataOff, dataSize, idxOff, idxSize} per file.
 * max_file_records must be >= every file_start[f+1]-file_start[f] (it sizes
 * the grid and the workspace).  Requires m >= 1. */
int lsm_build_sst(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                  const uint8_t *d_vals, const uint64_t *d_voff, const uint64_t *d_file_start,
                  uint32_t nfile, uint32_t max_file_records, uint64_t m, uint32_t k,
                  uint8_t *d_out, const uint64_t *d_file_off, int64_t *d_footer,
                  void *d_workspace, size_t ws_bytes, void *stream);

/* lsm_build_sst with the values read in place: value i of the batch is the
 * value of pair d_idx[i], a view into d_bytes (d_val_desc[d_idx[i]], a V
 * descriptor; or, d_val_desc == NULL, the value of KV descriptor
 * d_key_desc[d_idx[i]]); d_voff is the exclusive scan of those value lengths.
 * The keys come packed (d_keys / d_koff).  That is the output of
 * lsm_merge_kvs + lsm_gather_kvs(..., d_vals = NULL, ...): the values are not
 * copied twice.  Same images as lsm_build_sst. */
int lsm_build_sst_views(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                        const uint8_t *d_bytes, const lsm_rec_desc *d_key_desc,
                        const lsm_rec_desc *d_val_desc, const uint32_t *d_idx,
                        const uint64_t *d_voff, const uint64_t *d_file_start, uint32_t nfile,
                        uint32_t max_file_records, uint64_t m, uint32_t k, uint8_t *d_out,
                        const uint64_t *d_file_off, int64_t *d_footer, void *d_workspace,
                        size_t ws_bytes, void *stream);

/* ---- bloom probe (verification side, Filter.Test bloom.go:371-379) ------- */

/* Standalone bloom build: Filter.Add of every key (bloom.go:175-181) into
 * d_words (ceil(m/64) native u64 words, zeroed by the call). */
int lsm_bloom_build(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                    uint64_t m, uint32_t k, uint64_t *d_words, void *stream);

/* d_hit[i] = Filter.Test(key i) against the filter words of one .sst
 * (native u64 words, bit p -> word p>>6 bit p&63). */
int lsm_bloom_probe(lsm_ctx *ctx, const uint64_t *d_words, uint64_t m, uint32_t k,
                    const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
                    uint8_t *d_hit, void *stream);
/* sum256 (murmur.go:245-275) of each key: d_h[4*i .. 4*i+3]. */
int lsm_sum256(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff, uint64_t nkeys,
               uint64_t *d_h, void *stream);

/* ---- compaction merge ------------------------------- */

/* Replaces CompactAndMergeKVs (sstable/merge.go:42-94) up to the builder:
 * the n pairs are views into d_bytes -- key i at d_key_desc[i].rec_off + 4,
 * d_key_desc[i].key_len bytes (an IDX or KV descriptor); value i at
 * d_val_desc[i].rec_off + 4, d_val_desc[i].val_len bytes (a V descriptor) or,
 * with d_val_desc == NULL, right after the key of a KV descriptor
 * (d_key_desc[i].val_len bytes).  That is the output of lsm_decode_sst (f1)
 * or of a KV decode / WAL replay, with no copy.
 *
 * Pairs leave in key order (Go string order, bytewise); equal keys leave in
 * input order -- merge.go:41's contract, "the newest pair comes first and
 * wins".  lsm_merge_kvs_tie with LSM_TIE_GOHEAP reproduces container/heap's
 * own tie order instead (the reference's exact output; a host replay of the
 * heap over device-computed key ranks).  Per
 * pair, as merge.go:57-85: a key equal to the last written non-empty key is
 * skipped; a tombstone (kv.DeletedValue) is dropped when level >= 6
 * (maxSSTableLevel); otherwise it is written; a file is flushed when the
 * EstimateSize sum (16 + key + value bytes, kv.go:118-121) reaches
 * threshold (maxSSTableSize, 2 MiB; must be > 0) and the last written key is
 * forgotten at each flush.
 *
 * Outputs: d_out[0 .. nout) = input indices of the written pairs, in order;
 * d_file_start[0 .. nfiles] = each file's first position in d_out (optional,
 * n + 1 entries), d_file_start[nfiles] = nout; lsm_merge_kvs_tie's h_counts
 * (host, 3 entries) = {nout, nfiles, the most pairs in one file} (the last
 * sizes lsm_build_sst's max_file_records with no second read-back; ABI 4).
 * Synchronizes the stream (the radix passes are chosen from key statistics). */
size_t lsm_merge_kvs_workspace_bytes(uint64_t n);
enum lsm_tie {
    LSM_TIE_INPUT = 0,   /* equal keys in input order (merge.go:41's contract)              */
    LSM_TIE_GOHEAP = 1,  /* equal keys in container/heap's pop order (merge.go:47-66, exact) */
};
/* lsm_merge_kvs = lsm_merge_kvs_tie(..., LSM_TIE_INPUT, ...) with h_counts
 * holding 2 entries, {nout, nfiles} (unchanged since v2).  Same workspace. */
int lsm_merge_kvs_tie(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_key_desc,
                      const lsm_rec_desc *d_val_desc, uint64_t n, int level, uint64_t threshold,
                      int tie, uint32_t *d_out, uint64_t *d_file_start, uint64_t *h_counts,
                      void *d_ws, size_t ws_bytes, void *stream);
/* container/heap's pop order over dense key ranks (host, no device): Push of
 * 0 .. n-1, then Pop until empty, Less = rank <; order[j] = the j-th popped
 * index.  What LSM_TIE_GOHEAP replays.  phase_ns (optional, 2 entries): the
 * nanoseconds of the push and the pop phases (ABI 7).
 * LSM_TIE_GOHEAP skips the replay when every key is distinct (the device's
 * group count equals n): the heap then pops in key order, which the sort
 * already is -- both tie modes give the same output.  lsm_goheap_replays
 * counts the replays a context has run. */
int lsm_goheap_pop_order_host(const uint32_t *rank, uint64_t n, uint32_t *order, uint64_t *phase_ns);
uint64_t lsm_goheap_replays(const lsm_ctx *ctx);
/* The ordering plan the host chose in the context's last lsm_merge_kvs /
 * _tie / _async / lsm_compact_merge_async call, for tests and diagnosis
 * (read-only; host words kept in the context: no kernel, copy or
 * synchronisation).  plan[LSM_MERGE_PLAN_WORDS]:
 *   [0] order kind: 0 = no key bit varies (the identity order), 1 = LSD radix
 *       passes, 2 = the merge path (one sorted run holds at least half the pairs)
 *   [1] packed key width of the merge path: 32 or 64; 0 off the merge path
 *   [2] how the merge path ordered the pairs outside the run: 0 = there were
 *       none (or no merge path), 1 = k-way rank of their sorted runs, 2 = radix sort
 *   [3] LSD radix passes over all pairs
 *   [4] D, the 8-byte chunks of the longest key
 *   [5], [6] the longest sorted run of the input, [run_s, run_e)
 *   [7] the input's descents (key(i) < key(i - 1)), saturated at 2^32 - 1
 * All zero before the first call, after a call with n == 0 and after a call
 * that failed before it chose.  Returns LSM_EINVAL for a null argument. */
#define LSM_MERGE_PLAN_WORDS 8
int lsm_merge_plan(const lsm_ctx *ctx, uint32_t *plan);
int lsm_merge_kvs(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_key_desc,
                  const lsm_rec_desc *d_val_desc, uint64_t n, int level, uint64_t threshold,
                  uint32_t *d_out, uint64_t *d_file_start, uint64_t *h_counts, void *d_ws,
                  size_t ws_bytes, void *stream);
/* lsm_merge_kvs_tie without its closing read-back (ABI 5): the counts {nout,
 * nfiles, the most pairs in one file} go to d_counts (device, 3 entries) and
 * the call returns with the file walk and the emit still queued.  The
 * key-statistics read-back that picks the radix passes stays (and, for
 * LSM_TIE_GOHEAP, the host replay).  A compaction reads d_counts while its
 * gather (lsm_gather_kvs_dev) runs: the stream does not idle for the read. */
int lsm_merge_kvs_async(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_key_desc,
                        const lsm_rec_desc *d_val_desc, uint64_t n, int level, uint64_t threshold,
                        int tie, uint32_t *d_out, uint64_t *d_file_start, uint64_t *d_counts,
                        void *d_ws, size_t ws_bytes, void *stream);

/* The selected pairs d_idx[0 .. nout) as a CSR record batch -- the input of
 * lsm_build_sst: keys packed into d_keys with d_koff[0 .. nout], values into
 * d_vals with d_voff[0 .. nout] (the arenas must hold the selected bytes; the
 * input's totals always suffice).  d_vals == NULL packs the keys only (d_voff
 * is still written) for lsm_build_sst_views.  Asynchronous. */
size_t lsm_gather_kvs_workspace_bytes(uint64_t nout);
int lsm_gather_kvs(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_key_desc,
                   const lsm_rec_desc *d_val_desc, const uint32_t *d_idx, uint64_t nout,
                   uint8_t *d_keys, uint64_t *d_koff, uint8_t *d_vals, uint64_t *d_voff,
                   void *d_ws, size_t ws_bytes, void *stream);
/* lsm_gather_kvs with the pair count on the device (ABI 5): nout = *d_nout
 * (lsm_merge_kvs_async's d_counts[0]), at most nout_max, which sizes the
 * launches, the workspace (lsm_gather_kvs_workspace_bytes(nout_max)) and
 * d_koff / d_voff (nout_max + 1 entries).  Asynchronous. */
int lsm_gather_kvs_dev(lsm_ctx *ctx, const uint8_t *d_bytes, const lsm_rec_desc *d_key_desc,
                       const lsm_rec_desc *d_val_desc, const uint32_t *d_idx, const uint64_t *d_nout,
                       uint64_t nout_max, uint8_t *d_keys, uint64_t *d_koff, uint8_t *d_vals,
                       uint64_t *d_voff, void *d_ws, size_t ws_bytes, void *stream);

/* lsm_sst_pairs + lsm_merge_kvs_async in one call (ABI 6): the join of the
 * decoded files and CompactAndMergeKVs over it, queued in that order on
 * `stream` (compaction.go:173-193 then :49-95).  n = the join's pair count
 * (d_prefix[nfile], e.g. the sum of the decoded nidx of the files that
 * decoded), known to the caller; outputs, workspace
 * (lsm_merge_kvs_workspace_bytes(n)) and d_counts exactly as the two calls.
 * Waits on the host for the merge's key statistics, as lsm_merge_kvs_async
 * does; the join's own count d_prefix[nfile] comes back with them, and a call
 * whose n differs returns LSM_EINVAL before any pass indexes past the join
 * (the join's outputs and the statistics pass are then the only work done).  (Statistics taken before the join, to overlap their read-back with
 * it, measured slower and are not used: DESIGN.md section 7.) */
int lsm_compact_merge_async(lsm_ctx *ctx, const uint8_t *d_img, const lsm_sst_meta *d_meta,
                            const uint64_t *d_file_off, uint32_t nfile, const lsm_rec_desc *d_idx_desc,
                            const lsm_rec_desc *d_data_desc, uint64_t n, lsm_rec_desc *d_key_out,
                            lsm_rec_desc *d_val_out, uint64_t *d_prefix, int level, uint64_t threshold,
                            int tie, uint32_t *d_out, uint64_t *d_file_start, uint64_t *d_counts,
                            void *d_ws, size_t ws_bytes, void *stream);

/* The positional join of decoded files in file order -- loadLevelData's
 * allPairs (compaction.go:173-193) over GetKeyValuePairs (sstable.go:248-268):
 * d_key_out / d_val_out = the files' index (key) and data (value) descriptors
 * from lsm_decode_sst's outputs (file f's entries at slot d_file_off[f] / 4),
 * densely, file after file; files that failed (stage != 0) or hold no data or
 * no index entries contribute nothing.  d_prefix[0 .. nfile] = each file's
 * first output slot, d_prefix[nfile] = the total.  Asynchronous. */
int lsm_sst_pairs(lsm_ctx *ctx, const lsm_sst_meta *d_meta, const uint64_t *d_file_off,
                  uint32_t nfile, const lsm_rec_desc *d_idx_desc, const lsm_rec_desc *d_data_desc,
                  lsm_rec_desc *d_key_out, lsm_rec_desc *d_val_out, uint64_t *d_prefix,
                  void *stream);

/* ---- the builder path over one sorted stream (ABI 7) ----------------------- */

/* The builder rule on the device: lsm_segment_files_host's file starts for
 * the device CSR offsets d_koff / d_voff (n + 1 entries each) -- Builder.Add /
 * ShouldFlush (builder.go:34-42, EstimateSize kv.go:118-121) as driven by
 * CompactAndMergeKVs (merge.go:106-128); threshold 0 = never flush.  Writes
 * d_file_start[0 .. nfile] (d_file_start[nfile] = n; nfile_max + 1 entries)
 * and d_counts (device, 4 entries) = {nfile, the most records in one file, 0,
 * overflow}.  nfile_max = lsm_stream_max_files(n, key bytes, value bytes,
 * threshold) always suffices; with a smaller bound a stream needing more files
 * gets nfile = 0 and overflow = 1.  One workgroup; asynchronous. */
uint32_t lsm_stream_max_files(uint64_t n, uint64_t key_bytes, uint64_t val_bytes, uint64_t threshold);
int lsm_segment_files(lsm_ctx *ctx, const uint64_t *d_koff, const uint64_t *d_voff, uint64_t n,
                      uint64_t threshold, uint32_t nfile_max, uint64_t *d_file_start,
                      uint64_t *d_counts, void *stream);

/* Builder.Add / ShouldFlush / Build over one sorted record stream, every file
 * flushed at `threshold` (merge.go:106-128's loop; sstable.go:21's 2 MiB in
 * go-lsm), with SSTable.Add / EncodeTo and Filter.Add for every file -- the
 * rule (lsm_segment_files), the layout (lsm_sst_layout's: each image at a
 * multiple of `align` in d_out) and the images (lsm_build_sst's bytes) in one
 * call, with no host round trip for go-lsm's filter shape (two LDS slices,
 * k <= 16): every launch is sized on nfile_max and the counts stay on the
 * device.  Other filter shapes read the counts back (the call synchronizes).
 * Outputs: d_file_start (nfile_max + 1), d_file_off (nfile_max + 1: the last
 * entry used is the total), d_footer (optional, 4 * nfile_max), d_counts (4:
 * {nfile, most records in a file, image bytes, overflow}); d_out must hold
 * lsm_build_sst_stream_out_bytes(...) bytes, the workspace
 * lsm_build_sst_stream_workspace_bytes(...).  Same images, file for file, as
 * lsm_segment_files_host + lsm_build_sst. */
size_t lsm_build_sst_stream_workspace_bytes(uint64_t n, uint64_t threshold, uint32_t nfile_max,
                                            uint64_t m, uint32_t k);
uint64_t lsm_build_sst_stream_out_bytes(uint64_t n, uint64_t key_bytes, uint64_t val_bytes,
                                        uint32_t nfile_max, uint64_t m, uint32_t align);
int lsm_build_sst_stream(lsm_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_koff,
                         const uint8_t *d_vals, const uint64_t *d_voff, uint64_t n,
                         uint64_t threshold, uint32_t nfile_max, uint64_t m, uint32_t k,
                         uint32_t align, uint8_t *d_out, uint64_t *d_file_start,
                         uint64_t *d_file_off, int64_t *d_footer, uint64_t *d_counts,
                         void *d_workspace, size_t ws_bytes, void *stream);

/* .sst image size of each file f = records [d_file_start[f], d_file_start[f+1])
 * of a device CSR batch (as lsm_sst_image_size_host, sstable.go:131-193). */
int lsm_sst_image_sizes(lsm_ctx *ctx, const uint64_t *d_koff, const uint64_t *d_voff,
                        const uint64_t *d_file_start, uint32_t nfile, uint64_t m,
                        uint64_t *d_size, void *stream);

/* The images' layout without a host round trip: d_size[f] as
 * lsm_sst_image_sizes, d_file_off[f] = the sum of the earlier sizes, each
 * rounded up to `align` (> 0), and d_file_off[nfile] = the total (nfile + 1
 * entries) -- lsm_build_sst's d_file_off, ready on the device.  The output
 * buffer can be sized from host-known bounds: the total is at most
 * nfile * (lsm_filter_block_size(m) + 40 + align - 1) + 16 * nrec
 * + 3 * key bytes + value bytes.  Asynchronous. */
int lsm_sst_layout(lsm_ctx *ctx, const uint64_t *d_koff, const uint64_t *d_voff,
                   const uint64_t *d_file_start, uint32_t nfile, uint64_t m, uint32_t align,
                   uint64_t *d_size, uint64_t *d_file_off, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_GPU_H */
