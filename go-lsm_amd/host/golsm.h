// golsm.h — C++ host mirror of go-lsm's block-codec surface over the C ABI.
//
// go-lsm is Go and no Go toolchain exists in this image, so the host side
// above include/lsm_gpu.h is C++ mirroring the reference's types and methods
// (names, argument meaning, error text):
//   block.DataBlock   sstable/block/data.go:15-91
//   block.IndexBlock  sstable/block/index.go:12-113
//   block.Header      sstable/block/header.go:12-52
//   block.Footer      sstable/block/footer.go:11-102
//   bloom.Filter      sstable/bloom/bloom.go:74-491
//   sstable.SSTable   sstable/sstable.go:33-326
//   sstable.Builder   sstable/builder.go:9-59
// Every record decode/encode, the bloom build and probe run on the GPU
// (liblsm_gpu.so); only fixed-size framing (header, footer, filter words) is
// parsed on the host.  There is no CPU fallback: without a gfx950 device
// Device() throws.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "lsm_gpu.h"

namespace golsm {

// Go's `error`: an empty message is nil.
class Error {
  public:
    Error() = default;
    explicit Error(std::string m) : msg_(std::move(m)) {}
    explicit operator bool() const { return !msg_.empty(); }
    const std::string &Message() const { return msg_; }
    // fmt.Errorf("prefix: %w", err)
    Error Wrap(const std::string &prefix) const {
        return msg_.empty() ? Error() : Error(prefix + ": " + msg_);
    }

  private:
    std::string msg_;
};

using Bytes = std::vector<uint8_t>;

// io.Reader over an in-memory byte range (bytes.Reader, or a file read whole).
class Reader {
  public:
    Reader(const uint8_t *p, size_t n) : p_(p), n_(n) {}
    explicit Reader(const Bytes &b) : p_(b.data()), n_(b.size()) {}
    size_t Len() const { return n_ - pos_; }
    const uint8_t *Cur() const { return p_ + pos_; }
    void Skip(size_t k) { pos_ += k < Len() ? k : Len(); }
    size_t Pos() const { return pos_; }
    void Seek(size_t pos) { pos_ = pos < n_ ? pos : n_; }
    size_t Size() const { return n_; }
    const uint8_t *Data() const { return p_; }

  private:
    const uint8_t *p_;
    size_t n_;
    size_t pos_ = 0;
};

// io.Writer appending to a byte buffer (bytes.Buffer).
struct Buffer {
    Bytes data;
    void Write(const uint8_t *p, size_t n) { data.insert(data.end(), p, p + n); }
    size_t Len() const { return data.size(); }
};

// One lsm_ctx + HIP stream + grow-only staging buffers.  One per OS thread
// (go-lsm decodes from concurrent goroutines, sstable_test.go:379-400).
class Device {
  public:
    explicit Device(int ordinal = 0);
    ~Device();
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    static Device &ThisThread();  // device 0, created on first use per thread

    lsm_ctx *ctx() const { return ctx_; }
    void *stream() const { return stream_; }
    void *Dev(int slot, size_t bytes);   // grow-only device buffer
    void *Host(int slot, size_t bytes);  // grow-only pinned host buffer
    void H2D(void *d, const void *h, size_t n);
    void D2H(void *h, const void *d, size_t n);
    void Sync();

  private:
    static constexpr int kSlots = 48;
    lsm_ctx *ctx_ = nullptr;
    void *stream_ = nullptr;
    void *dev_[kSlots] = {};
    size_t dcap_[kSlots] = {};
    void *host_[kSlots] = {};
    size_t hcap_[kSlots] = {};
};

namespace kv {
using Key = std::string;
using Value = Bytes;
extern const std::string kDeletedValue;  // "～DELETED～" kv/kv.go:30

struct KeyValuePair {
    Key key;
    Value value;
    bool IsDeleted() const;        // kv.go:40-43
    uint64_t EstimateSize() const; // kv.go:118-121
};
}  // namespace kv

namespace block {

struct DataBlock {
    std::vector<kv::Value> Entries;
    Error EncodeTo(Buffer &w) const;               // data.go:26-45
    Error DecodeFrom(Reader &r, int64_t size);     // data.go:49-79 (size <= 0: unlimited)
    void Add(kv::Value v) { Entries.push_back(std::move(v)); }
    int Len() const { return (int)Entries.size(); }
};

struct IndexEntry {
    kv::Key Key;
    int64_t Offset;
};

struct IndexBlock {
    std::vector<IndexEntry> Indexes;
    int64_t Encode(Buffer &w, Error *err = nullptr) const;  // index.go:47-58
    Error DecodeFrom(Reader &r, int64_t size);              // index.go:61-101
    void Add(const kv::Key &k, int64_t off) { Indexes.push_back({k, off}); }
    int Len() const { return (int)Indexes.size(); }
    // Iterator.Seek (index.go:157-181): exact-match binary search, -1 if absent
    int Seek(const kv::Key &target) const;
};

struct Header {
    kv::Key MinKey, MaxKey;
    Error EncodeTo(Buffer &w) const;  // header.go:25-37
    Error DecodeFrom(Reader &r);      // header.go:40-52
};

constexpr int kFooterSize = 32;  // footer.go:23
constexpr int kHandleSize = 16;  // footer.go:24

struct Handle {
    int64_t Offset = 0, Size = 0;
    Error EncodeTo(Buffer &w) const;  // footer.go:94-102
    Error DecodeFrom(Reader &r);      // footer.go:73-91
};

struct Footer {
    Handle DataHandle, IndexHandle;
    Error EncodeTo(Buffer &w) const;  // footer.go:43-55
    Error DecodeFrom(Reader &r);      // footer.go:58-70
};

}  // namespace block

namespace bloom {

constexpr uint64_t kDefaultM = 1600000;  // bloom.go:80
constexpr uint64_t kDefaultK = 16;       // bloom.go:81

// Filter over native u64 words (bit p -> word p>>6, bit p&63).  Add() queues
// keys; they are hashed into the words on the GPU (lsm_bloom_build) in one
// batch the next time the words are needed.
class Filter {
  public:
    Filter(uint64_t m, uint64_t k);  // NewBloomFilter bloom.go:95-101 (m, k >= 1)
    static Filter Default() { return Filter(kDefaultM, kDefaultK); }
    Filter &Add(const uint8_t *data, size_t n);  // bloom.go:175-181
    Filter &AddString(const std::string &s) { return Add((const uint8_t *)s.data(), s.size()); }
    bool Test(const uint8_t *data, size_t n);    // bloom.go:371-379 (GPU probe)
    bool TestString(const std::string &s) { return Test((const uint8_t *)s.data(), s.size()); }
    bool MayContain(const kv::Key &k) { return TestString(k); }  // bloom.go:448-450
    Error EncodeTo(Buffer &w);    // bloom.go:472-491
    Error DecodeFrom(Reader &r);  // bloom.go:453-469
    uint64_t Cap() const { return m_; }
    uint64_t K() const { return k_; }
    const std::vector<uint64_t> &Words();
    bool Equal(Filter &g);        // bloom.go:318-321
    bool OnlyPending() const { return !built_; }
    const std::vector<std::string> &Pending() const { return pending_; }

  private:
    void Flush();
    uint64_t m_, k_;
    std::vector<uint64_t> words_;
    std::vector<std::string> pending_;
    bool built_ = false;  // words_ carry bits not derived from pending_
};

}  // namespace bloom

namespace sstable {

constexpr uint64_t kMaxSSTableSize = 2 * 1024 * 1024;  // sstable.go:21

class SSTable {
  public:
    block::Header Header;
    bloom::Filter FilterBlock = bloom::Filter::Default();
    block::IndexBlock IndexBlock;
    block::DataBlock DataBlock;
    block::Footer Footer;

    void Add(const kv::KeyValuePair &p);              // sstable.go:322-326
    Error EncodeImage(Bytes *out);                     // sstable.go:131-193, in memory
    Error EncodeTo(const std::string &path);           // sstable.go:131-193
    Error DecodeImage(const Bytes &img);               // sstable.go:87-128, in memory
    Error DecodeFrom(const std::string &path);         // sstable.go:87-128
    Error DecodeDataBlock(const Bytes &img);           // sstable.go:214-225
    std::vector<kv::KeyValuePair> GetDataBlockFromFile(const std::string &path, Error *err);
    std::vector<kv::KeyValuePair> GetKeyValuePairs(Error *err) const;  // sstable.go:248-268
    kv::Value GetValueByOffset(int64_t offset, Error *err);           // sstable.go:271-296
    bool MayContain(const kv::Key &key);                                // sstable.go:300-305
    const std::string &FilePath() const { return path_; }
    int level = 0;  // sstable.go:46 (set by NewSSTableWithLevel / CompactAndMergeKVs)

  private:
    std::string path_;
    Bytes image_;  // the file bytes once encoded/decoded (GetValueByOffset)
};

class Builder {  // builder.go:9-59
  public:
    void Add(const kv::KeyValuePair &p);
    bool ShouldFlush() const { return size_ >= kMaxSSTableSize; }
    void Finalize();
    SSTable &Build();
    uint64_t Size() const { return size_; }
    void SetSize(uint64_t s) { size_ = s; }
    SSTable &Table() { return table_; }

  private:
    SSTable table_;
    uint64_t size_ = 0;
};

// Batch entry points: the GPU's natural granularity.
// Decode many V-grammar data regions at once (compaction input,
// compaction.go:173-220); errs[i] uses the reference's error text.
std::vector<std::vector<kv::Value>> DecodeDataBlocks(const std::vector<Bytes> &regions,
                                                     std::vector<Error> *errs);
// Whole .sst images -> KV pairs in one launch (lsm_decode_sst): per image
// SSTable.DecodeFrom + DecodeDataBlock + GetKeyValuePairs (sstable.go:87-128,
// 214-268), the batch form of compaction's loadLevelData (compaction.go:
// 173-220).  errs[i] carries the reference's error prefix for the failing
// step ("decode Header failed", ..., "mismatched DataBlock and IndexBlock
// entries").
std::vector<std::vector<kv::KeyValuePair>> DecodeFiles(const std::vector<Bytes> &images,
                                                       std::vector<Error> *errs);
// Builder flush rule + SSTable.EncodeTo for a sorted batch in one launch:
// threshold 0 = one file (memtable flush), kMaxSSTableSize = CompactAndMergeKVs.
std::vector<Bytes> BuildImages(const std::vector<kv::KeyValuePair> &sorted, uint64_t threshold,
                               uint64_t m = bloom::kDefaultM, uint64_t k = bloom::kDefaultK);
// The same for given file boundaries: file f = sorted[starts[f], starts[f+1]).
std::vector<Bytes> BuildImagesAt(const std::vector<kv::KeyValuePair> &sorted,
                                 const std::vector<uint64_t> &starts,
                                 uint64_t m = bloom::kDefaultM, uint64_t k = bloom::kDefaultK);
// CompactAndMergeKVs (merge.go:42-94) over lsm_merge_kvs: pairs in key order,
// a key equal to the last written one skipped, tombstones dropped at level 6,
// a new table at every 2 MiB of EstimateSize, the last written key forgotten
// at each flush.  Pairs with equal keys leave in input order (merge.go:41's
// contract; container/heap's own order is unspecified).  The
// tables are returned as decoded from their built images, level set.
std::vector<SSTable> CompactAndMergeKVs(const std::vector<kv::KeyValuePair> &kvs, int level);
// What Manager.CreateNewSSTable (sstable/manager.go:74-95) does for each
// IMemTable -- BuildSSTableFromIMemTable (builder.go:22-31) over
// IMemTable.RangeScan, then SSTable.EncodeTo -- for every memtable at once,
// from the memtables' own WAL bytes instead of a walk of the skiplist:
// lsm_wal_replay -> lsm_memtable_order -> lsm_gather_kvs_dev -> lsm_sst_layout
// -> lsm_build_sst_views.  images[w] is log w's level-0 .sst image, empty when
// its memtable delivers no pair or its replay failed ((*status)[w], the
// lsm_status wal.Recover's error maps to).  scan: LSM_MEMTABLE_ALL (every
// node, tombstones included) or LSM_MEMTABLE_RANGESCAN (RangeScan as written:
// delivery stops at the first inner tombstone).
std::vector<Bytes> BuildSSTablesFromWALs(const std::vector<Bytes> &wals, int scan,
                                         std::vector<int32_t> *status = nullptr,
                                         uint64_t m = bloom::kDefaultM, uint64_t k = bloom::kDefaultK);
// Range scans over a whole tree in one call (lsm_tree_scan): what a
// database.Iterator over the SSTables delivers -- sstable.Iterator
// (sstable/iterator.go:9-73) per table, merged in Manager.Search's order.
// `images` are the tree's tables in lsm_search's order (level 0 newest first,
// each deeper level by MinKey), level_start (LSM_SEARCH_LEVELS + 1 entries)
// ending at images.size().  Per range [lo, hi) (no_upper: hi ignored) up to
// `limit` entries in key order, each key once with the entry of the table
// Search answers it from: its key, the answering table, result (LSM_GET_FOUND,
// or Search's error code with an empty value) and the value's bytes.  mode is a
// lsm_scan_mode: LSM_SCAN_LIVE leaves out keys whose answering value is the
// tombstone, LSM_SCAN_RAW returns it as a value.  more: the walk stopped at
// limit with a further entry to deliver.  No ranges or no images: no device
// call.  Throws std::invalid_argument for an unknown mode, limit == 0 or a
// level_start that does not end at images.size().
struct ScanRange {
    kv::Key lo, hi;
    bool no_upper = false;
};
struct ScanEntry {
    kv::Key key;
    kv::Value value;
    int32_t table = -1;
    int32_t result = LSM_GET_ABSENT;
};
struct ScanResult {
    std::vector<ScanEntry> entries;
    bool more = false;
};
std::vector<ScanResult> ScanImages(const std::vector<Bytes> &images, const uint32_t *level_start,
                                   const std::vector<ScanRange> &ranges, uint32_t limit,
                                   int mode = LSM_SCAN_LIVE);

}  // namespace sstable

// Go's package is `memtable`; the namespace is `memtables` because a mirror
// test that does `using namespace golsm` has a function named `memtable`
// (tests/cpp/memtable_mirror_test.cpp), which the package's name would hide.
namespace memtables {
// Manager.Search (memtable/manager.go:61-74) of every key over the memtables
// recovered from `wals` (oldest first; the last is Mem, manager.go:140-180):
// lsm_wal_replay -> lsm_memtable_order (LSM_MEMTABLE_ALL) ->
// lsm_memtable_search_index_build -> lsm_memtable_search.  The newest log
// holding the key answers: result is a lsm_mem_result, log that log (-1 on a
// miss), value the node's value for LSM_MEM_VALUE (empty for a tombstone: Go's
// nil).  No logs or no keys: every key misses, no device call.
struct SearchResult {
    int32_t result = LSM_MEM_MISS;
    int32_t log = -1;
    kv::Value value;
};
std::vector<SearchResult> SearchWALs(const std::vector<Bytes> &wals, const std::vector<kv::Key> &keys);
}  // namespace memtables

namespace database {
// database.Get (database/database.go:24-40) of every key over lsm_db_get: the
// memtables recovered from `wals` (as memtables::SearchWALs), then
// sstable.Manager.Search over `images` -- the tree's tables in lsm_search's
// order (level 0 newest first, each deeper level by MinKey), level_start
// (LSM_SEARCH_LEVELS + 1 entries) ending at images.size().  mode is a
// lsm_db_get_mode.  src is a lsm_get_source and says where Get's value came
// from: LSM_SRC_MEMTABLE (value copied from the logs), LSM_SRC_SSTABLE (from
// the images; result > LSM_GET_FOUND is Search's error and value is empty),
// LSM_SRC_NONE for (nil, nil).  mem_result / log as SearchWALs; level / table /
// result as lsm_search for the keys that went on to the tables, -1 / -1 /
// LSM_GET_ABSENT for the others.  No keys, or neither logs nor images: no
// device call.  Throws std::invalid_argument for an unknown mode or a
// level_start that does not end at images.size().
struct GetResult {
    int32_t src = LSM_SRC_NONE;
    int32_t mem_result = LSM_MEM_MISS;
    int32_t log = -1;
    int32_t level = -1, table = -1;
    int32_t result = LSM_GET_ABSENT;
    kv::Value value;
};
std::vector<GetResult> GetFromWALs(const std::vector<Bytes> &wals, const std::vector<Bytes> &images,
                                   const uint32_t *level_start, const std::vector<kv::Key> &keys,
                                   int mode = LSM_DBGET_TOMBSTONE_HIDES);

// The database's range scan over lsm_db_scan: sstable::ScanImages with the
// memtables recovered from `wals` (oldest first, as GetFromWALs) in front.
// lsm_wal_replay -> lsm_memtable_order (LSM_MEMTABLE_ALL) ->
// lsm_memtable_search_index_build -> lsm_decode_sst -> lsm_level_get_tree_build
// -> lsm_db_scan, with the memtable index and the Seek tree.  Per range up to
// `limit` entries in key order, each key once, answered by the newest memtable
// that holds it, else by the table Search answers it from: src is
// LSM_SRC_MEMTABLE (table = the log, result = LSM_GET_FOUND, value the node's
// bytes -- the 13 tombstone bytes in LSM_SCAN_RAW) or LSM_SRC_SSTABLE (as
// ScanImages).  mode is a lsm_scan_mode: LSM_SCAN_LIVE leaves out a key whose
// answering entry is a tombstone, which hides it in every older source in both
// modes.  No ranges, or neither logs nor images: no device call.  Throws
// std::invalid_argument as ScanImages does.
struct ScanEntry {
    kv::Key key;
    kv::Value value;
    int32_t src = LSM_SRC_NONE;
    int32_t table = -1;
    int32_t result = LSM_GET_ABSENT;
};
struct ScanResult {
    std::vector<ScanEntry> entries;
    bool more = false;
};
std::vector<ScanResult> ScanFromWALs(const std::vector<Bytes> &wals, const std::vector<Bytes> &images,
                                     const uint32_t *level_start, const std::vector<sstable::ScanRange> &ranges,
                                     uint32_t limit, int mode = LSM_SCAN_LIVE);
// ScanFromWALs for a tree that lives on the device: the same calls, then
// lsm_pack_results (the sizing call, its counts read back, the packing call at
// exactly K and V bytes).  Every entry's key and value come from the two
// packed arenas, each copied back with one D2H, as are row_start, entry_slot,
// koff, voff and the per-slot src / table / result; the views are not copied
// back and the host's `wals` and `images` are not sliced.  Same results as
// ScanFromWALs, entry for entry.
std::vector<ScanResult> ScanFromWALsPacked(const std::vector<Bytes> &wals, const std::vector<Bytes> &images,
                                           const uint32_t *level_start,
                                           const std::vector<sstable::ScanRange> &ranges, uint32_t limit,
                                           int mode = LSM_SCAN_LIVE);
// database.Put / database.Delete (database/database.go:42-59) of a batch over
// lsm_db_write: memtable.Manager.Insert / Delete (memtable/manager.go:40-106)
// applied in order -- CanInsert against sizeInBytes (memtable.go:112-121),
// promoteLocked when the pair does not fit, MemTable.Delete's (key, nil) record
// when the current memtable holds the key (memtable.go:84-96), wal.Append of
// KeyValuePair.EncodeTo (wal.go:85-92, kv.go:46-74).  mem_size0 is Mem's
// sizeInBytes on entry, current_wal its log so far (its skiplist is recovered
// from it, lsm_wal_replay -> lsm_memtable_order; empty = an empty skiplist).
// logs[0] is what the batch appends to Mem's log (empty when op 0 already
// rotates), logs[s > 0] the log of each memtable the batch opens: every log
// but the last belongs to a memtable promoteLocked froze, the last to the new
// Mem, whose sizeInBytes is mem_size.  A Delete's value is ignored.  Evicting
// the 11th frozen memtable (sstable::BuildSSTablesFromWALs), WAL file ids and
// I/O stay with the caller.  No ops: no device call.  Throws
// std::invalid_argument for an unknown op or mem_max outside [1, 1 << 30].
constexpr uint64_t kMaxMemTableSize = 2 * 1024 * 1024;  // maxMemoryTableSize
struct WriteOp {
    int op = LSM_OP_PUT;  // a lsm_write_op
    kv::Key key;
    kv::Value value;
};
struct WriteResult {
    std::vector<Bytes> logs;
    uint64_t mem_size = 0;
};
WriteResult WriteBatch(const std::vector<WriteOp> &ops, uint64_t mem_size0 = 0,
                       uint64_t mem_max = kMaxMemTableSize, const Bytes &current_wal = {});
}  // namespace database
}  // namespace golsm
