// golsm.cpp — C++ host mirror of go-lsm's block codec over include/lsm_gpu.h.
// See golsm.h.  Record decode/encode, bloom build and probe are GPU launches;
// the host only packs buffers, parses fixed framing and formats errors with
// the reference's text.
#include "golsm.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <memory>
#include <stdexcept>

namespace golsm {

namespace {

uint32_t ld32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
uint64_t ld64(const uint8_t *p) { return (uint64_t)ld32(p) | (uint64_t)ld32(p + 4) << 32; }
uint64_t ld64be(const uint8_t *p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v = v << 8 | p[i];
    return v;
}
void put32(Buffer &w, uint32_t v) {
    uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    w.Write(b, 4);
}
void put64(Buffer &w, uint64_t v) {
    put32(w, (uint32_t)v);
    put32(w, (uint32_t)(v >> 32));
}
void put64be(Buffer &w, uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * (7 - i)));
    w.Write(b, 8);
}

void check(int rc, const char *what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + " failed with code " + std::to_string(rc));
}

const char *eof_or_unexpected(size_t got) { return got == 0 ? "EOF" : "unexpected EOF"; }

size_t pad16(size_t n) { return ((n + 15) & ~(size_t)15) + LSM_INPUT_SLACK; }

// One-launch batch decode of host blocks; descriptors come back per block.
struct Decoded {
    std::vector<int32_t> status;
    std::vector<uint32_t> nrec;
    std::vector<std::vector<lsm_rec_desc>> desc;  // rec_off relative to the block
    std::vector<std::vector<int64_t>> idx;        // IDX offsets
};

Decoded gpu_decode(int grammar, const std::vector<std::pair<const uint8_t *, size_t>> &blocks) {
    Device &d = Device::ThisThread();
    const size_t nb = blocks.size();
    Decoded out;
    out.status.assign(nb, 0);
    out.nrec.assign(nb, 0);
    out.desc.resize(nb);
    out.idx.resize(nb);
    if (nb == 0) return out;
    std::vector<uint64_t> off(nb);
    std::vector<uint32_t> len(nb);
    size_t total = 0;
    for (size_t i = 0; i < nb; i++) {
        off[i] = total;
        len[i] = (uint32_t)blocks[i].second;
        total += (blocks[i].second + 15) & ~(size_t)15;
    }
    uint8_t *h_in = (uint8_t *)d.Host(0, pad16(total));
    std::memset(h_in, 0, pad16(total));
    for (size_t i = 0; i < nb; i++) std::memcpy(h_in + off[i], blocks[i].first, blocks[i].second);
    void *d_in = d.Dev(0, pad16(total));
    void *d_off = d.Dev(1, nb * 8);
    void *d_len = d.Dev(2, nb * 4);
    void *d_nrec = d.Dev(3, nb * 4);
    void *d_st = d.Dev(4, nb * 4);
    const uint64_t R = grammar == LSM_GRAMMAR_V ? 4 : grammar == LSM_GRAMMAR_KV ? 8 : 12;
    const size_t cap = total / R + 1;
    void *d_desc = d.Dev(5, cap * sizeof(lsm_rec_desc));
    void *d_idx = grammar == LSM_GRAMMAR_IDX ? d.Dev(6, cap * 8) : nullptr;
    d.H2D(d_in, h_in, pad16(total));
    d.H2D(d_off, off.data(), nb * 8);
    d.H2D(d_len, len.data(), nb * 4);
    lsm_decode_out o{};
    o.desc = (lsm_rec_desc *)d_desc;
    o.nrec = (uint32_t *)d_nrec;
    o.status = (int32_t *)d_st;
    o.idx_value = (int64_t *)d_idx;
    check(lsm_decode_blocks(d.ctx(), grammar, (const uint8_t *)d_in, (const uint64_t *)d_off,
                            (const uint32_t *)d_len, (uint32_t)nb, &o, d.stream()),
          "lsm_decode_blocks");
    d.D2H(out.nrec.data(), d_nrec, nb * 4);
    d.D2H(out.status.data(), d_st, nb * 4);
    d.Sync();
    for (size_t i = 0; i < nb; i++) {
        const size_t base = off[i] / R, k = out.nrec[i];
        out.desc[i].resize(k);
        if (k) d.D2H(out.desc[i].data(), (lsm_rec_desc *)d_desc + base, k * sizeof(lsm_rec_desc));
        if (d_idx) {
            out.idx[i].resize(k);
            if (k) d.D2H(out.idx[i].data(), (int64_t *)d_idx + base, k * 8);
        }
    }
    d.Sync();
    for (size_t i = 0; i < nb; i++)
        for (auto &x : out.desc[i]) x.rec_off -= off[i];
    return out;
}

// One-launch encode of a CSR batch as one block.
Bytes gpu_encode(int grammar, const Bytes &keys, const std::vector<uint64_t> &koff,
                 const Bytes &vals, const std::vector<uint64_t> &voff,
                 const std::vector<int64_t> &idx_off) {
    Device &d = Device::ThisThread();
    const uint64_t n = (grammar == LSM_GRAMMAR_V ? voff.size() : koff.size()) - 1;
    const uint64_t size = lsm_encoded_size_host(grammar, koff.data(), voff.data(), 0, n);
    Bytes out(size);
    if (n == 0) return out;
    void *d_keys = d.Dev(0, pad16(keys.size()));
    void *d_koff = d.Dev(1, koff.size() * 8);
    void *d_vals = d.Dev(2, pad16(vals.size()));
    void *d_voff = d.Dev(3, voff.size() * 8);
    void *d_io = d.Dev(4, (idx_off.size() + 1) * 8);
    void *d_rs = d.Dev(5, 16);
    void *d_oo = d.Dev(6, 8);
    void *d_out = d.Dev(7, pad16(size));
    if (!keys.empty()) d.H2D(d_keys, keys.data(), keys.size());
    d.H2D(d_koff, koff.data(), koff.size() * 8);
    if (!vals.empty()) d.H2D(d_vals, vals.data(), vals.size());
    d.H2D(d_voff, voff.data(), voff.size() * 8);
    if (!idx_off.empty()) d.H2D(d_io, idx_off.data(), idx_off.size() * 8);
    const uint64_t rs[2] = {0, n}, oo = 0;
    d.H2D(d_rs, rs, 16);
    d.H2D(d_oo, &oo, 8);
    check(lsm_encode_blocks(d.ctx(), grammar, (const uint8_t *)d_keys, (const uint64_t *)d_koff,
                            (const uint8_t *)d_vals, (const uint64_t *)d_voff,
                            grammar == LSM_GRAMMAR_IDX ? (const int64_t *)d_io : nullptr,
                            (const uint64_t *)d_rs, 1, (uint8_t *)d_out, (const uint64_t *)d_oo,
                            d.stream()),
          "lsm_encode_blocks");
    d.D2H(out.data(), d_out, size);
    d.Sync();
    return out;
}

template <class T, class F>
void csr(const std::vector<T> &items, F get, Bytes *data, std::vector<uint64_t> *off) {
    off->assign(items.size() + 1, 0);
    size_t tot = 0;
    for (size_t i = 0; i < items.size(); i++) {
        tot += get(items[i]).size();
        (*off)[i + 1] = tot;
    }
    data->resize(tot);
    size_t p = 0;
    for (auto &it : items) {
        const auto &v = get(it);
        if (!v.empty()) std::memcpy(data->data() + p, v.data(), v.size());
        p += v.size();
    }
}

}  // namespace

// ---- Device -----------------------------------------------------------------

Device::Device(int ordinal) {
    check(lsm_ctx_create(ordinal, &ctx_), "lsm_ctx_create (a gfx950 GPU is required)");
    check(lsm_stream_create(ctx_, &stream_), "lsm_stream_create");
}

Device::~Device() {
    for (int i = 0; i < kSlots; i++) {
        if (dev_[i]) lsm_dev_free(ctx_, dev_[i]);
        if (host_[i]) lsm_host_free_pinned(ctx_, host_[i]);
    }
    if (stream_) lsm_stream_destroy(ctx_, stream_);
    if (ctx_) lsm_ctx_destroy(ctx_);
}

Device &Device::ThisThread() {
    thread_local std::unique_ptr<Device> d;
    if (!d) d.reset(new Device(0));
    return *d;
}

void *Device::Dev(int slot, size_t bytes) {
    if (bytes > dcap_[slot]) {
        if (dev_[slot]) check(lsm_dev_free(ctx_, dev_[slot]), "lsm_dev_free");
        dev_[slot] = nullptr;
        size_t c = bytes < 4096 ? 4096 : bytes + bytes / 4;
        check(lsm_dev_alloc(ctx_, c, &dev_[slot]), "lsm_dev_alloc");
        dcap_[slot] = c;
    }
    return dev_[slot];
}

void *Device::Host(int slot, size_t bytes) {
    if (bytes > hcap_[slot]) {
        if (host_[slot]) check(lsm_host_free_pinned(ctx_, host_[slot]), "lsm_host_free_pinned");
        host_[slot] = nullptr;
        size_t c = bytes < 4096 ? 4096 : bytes + bytes / 4;
        check(lsm_host_alloc_pinned(ctx_, c, &host_[slot]), "lsm_host_alloc_pinned");
        hcap_[slot] = c;
    }
    return host_[slot];
}

void Device::H2D(void *dd, const void *h, size_t n) {
    check(lsm_memcpy_h2d(ctx_, dd, h, n, stream_), "lsm_memcpy_h2d");
}
void Device::D2H(void *h, const void *dd, size_t n) {
    check(lsm_memcpy_d2h(ctx_, h, dd, n, stream_), "lsm_memcpy_d2h");
}
void Device::Sync() { check(lsm_stream_sync(ctx_, stream_), "lsm_stream_sync"); }

// ---- kv -----------------------------------------------------------------------

namespace kv {
const std::string kDeletedValue = "\xef\xbd\x9e" "DELETED" "\xef\xbd\x9e";

bool KeyValuePair::IsDeleted() const {
    return value.size() == kDeletedValue.size() &&
           std::memcmp(value.data(), kDeletedValue.data(), value.size()) == 0;
}
uint64_t KeyValuePair::EstimateSize() const { return 4 + key.size() + 4 + value.size() + 8; }
}  // namespace kv

// ---- block ----------------------------------------------------------------------

namespace block {

Error DataBlock::EncodeTo(Buffer &w) const {
    Bytes vals;
    std::vector<uint64_t> voff;
    csr(Entries, [](const kv::Value &v) -> const kv::Value & { return v; }, &vals, &voff);
    std::vector<uint64_t> koff(voff.size(), 0);
    Bytes enc = gpu_encode(LSM_GRAMMAR_V, Bytes(), koff, vals, voff, {});
    w.Write(enc.data(), enc.size());
    return Error();
}

Error DataBlock::DecodeFrom(Reader &r, int64_t size) {
    // size > 0: io.LimitReader(r, size); otherwise read to EOF (data.go:51-54)
    const size_t n = size > 0 ? std::min((size_t)size, r.Len()) : r.Len();
    const uint8_t *p = r.Cur();
    Decoded dec = gpu_decode(LSM_GRAMMAR_V, {{p, n}});
    size_t end = 0;
    for (auto &ds : dec.desc[0]) {
        Entries.emplace_back(p + ds.rec_off + 4, p + ds.rec_off + 4 + ds.val_len);
        end = ds.rec_off + 4 + ds.val_len;
    }
    r.Skip(n);  // ReadFull/binary.Read drain the limited reader up to the failure
    switch (dec.status[0]) {
    case LSM_OK: return Error();
    case LSM_ST_TRUNC_LEN_PREFIX:
        return Error("read value length failed: unexpected EOF");
    case LSM_ST_TRUNC_VAL:
        return Error(std::string("read value data failed: ") + eof_or_unexpected(n - end - 4));
    default: return Error("decode status " + std::to_string(dec.status[0]));
    }
}

int64_t IndexBlock::Encode(Buffer &w, Error *err) const {
    Bytes keys;
    std::vector<uint64_t> koff;
    csr(Indexes, [](const IndexEntry &e) -> const std::string & { return e.Key; }, &keys, &koff);
    std::vector<int64_t> io;
    for (auto &e : Indexes) io.push_back(e.Offset);
    std::vector<uint64_t> voff(koff.size(), 0);
    Bytes enc = gpu_encode(LSM_GRAMMAR_IDX, keys, koff, Bytes(), voff, io);
    w.Write(enc.data(), enc.size());
    if (err) *err = Error();
    return (int64_t)enc.size();
}

Error IndexBlock::DecodeFrom(Reader &r, int64_t size) {
    Indexes.clear();  // index.go:63
    if (size < 0)
        return Error("invalid size: " + std::to_string(size) + ", must be non-negative");
    // Entries lie inside the size limit; the underlying stream may be shorter.
    const size_t avail = r.Len();
    const size_t n = std::min((size_t)size, avail);
    const uint8_t *p = r.Cur();
    Decoded dec = gpu_decode(LSM_GRAMMAR_IDX, {{p, n}});
    size_t pos = 0;
    for (size_t i = 0; i < dec.desc[0].size(); i++) {
        const auto &ds = dec.desc[0][i];
        Indexes.push_back({kv::Key((const char *)p + ds.rec_off + 4, ds.key_len), dec.idx[0][i]});
        pos = ds.rec_off + 12 + ds.key_len;
    }
    // A limit past the end of the stream can never be reached: the loop keeps
    // reading until a read hits EOF, even when the entries tile the stream.
    if (dec.status[0] == LSM_OK && (size_t)size <= avail) {
        r.Skip(pos);
        return Error();
    }
    // Reproduce the reference's message for the failing entry (index.go:70-91):
    // it reads past the limit from the stream, which may or may not hold the bytes.
    const size_t rem = avail - pos;
    r.Skip(avail);
    if (rem < 4)
        return Error(std::string("decode index key length failed: decode key keyLen: ") +
                     eof_or_unexpected(rem));
    const uint32_t kl = ld32(p + pos);
    if (rem - 4 < kl)
        return Error(std::string("decode index key length failed: decode key bytes: ") +
                     eof_or_unexpected(rem - 4));
    if (rem - 4 - kl < 8)
        return Error(std::string("decode index offset failed: ") + eof_or_unexpected(rem - 4 - kl));
    return Error("unexpected EOF: size limit reached while reading key length");
}

int IndexBlock::Seek(const kv::Key &target) const {
    auto it = std::lower_bound(Indexes.begin(), Indexes.end(), target,
                               [](const IndexEntry &e, const kv::Key &t) { return e.Key < t; });
    if (it == Indexes.end() || it->Key != target) return -1;
    return (int)(it - Indexes.begin());
}

static Error decode_key(Reader &r, kv::Key *k) {  // kv.Key.DecodeFrom kv.go:124-139
    if (r.Len() < 4) {
        Error e(std::string("decode key keyLen: ") + eof_or_unexpected(r.Len()));
        r.Skip(r.Len());
        return e;
    }
    const uint32_t kl = ld32(r.Cur());
    r.Skip(4);
    if (r.Len() < kl) {
        Error e(std::string("decode key bytes: ") + eof_or_unexpected(r.Len()));
        r.Skip(r.Len());
        return e;
    }
    k->assign((const char *)r.Cur(), kl);
    r.Skip(kl);
    return Error();
}

Error Header::EncodeTo(Buffer &w) const {
    put32(w, (uint32_t)MinKey.size());
    w.Write((const uint8_t *)MinKey.data(), MinKey.size());
    put32(w, (uint32_t)MaxKey.size());
    w.Write((const uint8_t *)MaxKey.data(), MaxKey.size());
    return Error();
}

Error Header::DecodeFrom(Reader &r) {
    Error e = decode_key(r, &MinKey);
    if (e) return e.Wrap("decode min key");
    return decode_key(r, &MaxKey);  // header.go:46-49 returns it unwrapped
}

Error Handle::EncodeTo(Buffer &w) const {
    put64(w, (uint64_t)Offset);
    put64(w, (uint64_t)Size);
    return Error();
}

Error Handle::DecodeFrom(Reader &r) {
    if (r.Len() < (size_t)kHandleSize) {
        Error e(std::string("decode footer failed: ") + eof_or_unexpected(r.Len()));
        r.Skip(r.Len());
        return e;
    }
    Offset = (int64_t)ld64(r.Cur());
    Size = (int64_t)ld64(r.Cur() + 8);
    r.Skip(kHandleSize);
    return Error();
}

Error Footer::EncodeTo(Buffer &w) const {
    DataHandle.EncodeTo(w);
    IndexHandle.EncodeTo(w);
    return Error();
}

Error Footer::DecodeFrom(Reader &r) {
    Error e = DataHandle.DecodeFrom(r);
    if (e) return e.Wrap("decode data handle failed");
    e = IndexHandle.DecodeFrom(r);
    if (e) return e.Wrap("decode index handle failed");
    return Error();
}

}  // namespace block

// ---- bloom ----------------------------------------------------------------------

namespace bloom {

Filter::Filter(uint64_t m, uint64_t k)
    : m_(m ? m : 1), k_(k ? k : 1), words_((m_ + 63) / 64, 0) {}

Filter &Filter::Add(const uint8_t *data, size_t n) {
    pending_.emplace_back((const char *)data, n);
    return *this;
}

void Filter::Flush() {
    if (pending_.empty()) return;
    Device &d = Device::ThisThread();
    Bytes keys;
    std::vector<uint64_t> koff;
    csr(pending_, [](const std::string &s) -> const std::string & { return s; }, &keys, &koff);
    const size_t nw = words_.size();
    void *d_keys = d.Dev(0, pad16(keys.size()));
    void *d_koff = d.Dev(1, koff.size() * 8);
    void *d_words = d.Dev(2, nw * 8);
    if (!keys.empty()) d.H2D(d_keys, keys.data(), keys.size());
    d.H2D(d_koff, koff.data(), koff.size() * 8);
    check(lsm_bloom_build(d.ctx(), (const uint8_t *)d_keys, (const uint64_t *)d_koff,
                          pending_.size(), m_, (uint32_t)k_, (uint64_t *)d_words, d.stream()),
          "lsm_bloom_build");
    std::vector<uint64_t> fresh(nw);
    d.D2H(fresh.data(), d_words, nw * 8);
    d.Sync();
    for (size_t i = 0; i < nw; i++) words_[i] |= fresh[i];  // Merge = bitset union
    pending_.clear();
    built_ = true;
}

const std::vector<uint64_t> &Filter::Words() {
    Flush();
    return words_;
}

bool Filter::Test(const uint8_t *data, size_t n) {
    Flush();
    Device &d = Device::ThisThread();
    const size_t nw = words_.size();
    void *d_words = d.Dev(2, nw * 8);
    void *d_key = d.Dev(3, pad16(n));
    void *d_koff = d.Dev(4, 16);
    void *d_hit = d.Dev(5, 16);
    d.H2D(d_words, words_.data(), nw * 8);
    if (n) d.H2D(d_key, data, n);
    const uint64_t ko[2] = {0, n};
    d.H2D(d_koff, ko, 16);
    check(lsm_bloom_probe(d.ctx(), (const uint64_t *)d_words, m_, (uint32_t)k_,
                          (const uint8_t *)d_key, (const uint64_t *)d_koff, 1, (uint8_t *)d_hit,
                          d.stream()),
          "lsm_bloom_probe");
    uint8_t hit = 0;
    d.D2H(&hit, d_hit, 1);
    d.Sync();
    return hit != 0;
}

Error Filter::EncodeTo(Buffer &w) {
    Flush();
    const uint64_t nw = words_.size();
    put64(w, 24 + 8 * nw);  // length prefix, bloom.go:478
    put64be(w, m_);         // WriteTo: arraySize, hashNum, bitset length, words
    put64be(w, k_);
    put64be(w, m_);
    for (uint64_t x : words_) put64be(w, x);
    return Error();
}

Error Filter::DecodeFrom(Reader &r) {
    if (r.Len() < 8) {
        Error e(std::string("decode filter length: ") + eof_or_unexpected(r.Len()));
        r.Skip(r.Len());
        return e;
    }
    const uint64_t L = ld64(r.Cur());
    r.Skip(8);
    if (r.Len() < L) {
        Error e(std::string("decode filter data: ") + eof_or_unexpected(r.Len()));
        r.Skip(r.Len());
        return e;
    }
    const uint8_t *p = r.Cur();
    r.Skip(L);
    if (L < 24) return Error("unexpected EOF");
    const uint64_t m = ld64be(p), k = ld64be(p + 8), nbits = ld64be(p + 16);
    const uint64_t nw = nbits / 64 + ((nbits & 63) != 0);  // no (nbits + 63) overflow
    if (nw > (L - 24) / 8) return Error("unexpected EOF");
    m_ = m;
    k_ = k;
    words_.assign(nw, 0);
    for (uint64_t i = 0; i < nw; i++) words_[i] = ld64be(p + 24 + 8 * i);
    pending_.clear();
    built_ = true;
    return Error();
}

bool Filter::Equal(Filter &g) { return m_ == g.m_ && k_ == g.k_ && Words() == g.Words(); }

}  // namespace bloom

// ---- sstable ----------------------------------------------------------------------

namespace sstable {

void SSTable::Add(const kv::KeyValuePair &p) {
    DataBlock.Add(p.value);
    IndexBlock.Add(p.key, 0);
    FilterBlock.AddString(p.key);
}

Error SSTable::EncodeImage(Bytes *out) {
    const size_t n = DataBlock.Entries.size();
    if (IndexBlock.Indexes.size() < n) return Error("index block shorter than data block");
    bool fused = FilterBlock.OnlyPending() && IndexBlock.Indexes.size() == n &&
                 FilterBlock.Pending().size() == n;
    for (size_t i = 0; fused && i < n; i++) fused = FilterBlock.Pending()[i] == IndexBlock.Indexes[i].Key;
    if (fused) {
        if (n) fused = Header.MinKey == IndexBlock.Indexes[0].Key && Header.MaxKey == IndexBlock.Indexes[n - 1].Key;
        else fused = Header.MinKey.empty() && Header.MaxKey.empty();
    }
    if (fused) {
        // Builder path: one lsm_build_sst launch (bloom fused, sstable.go:131-193)
        Device &d = Device::ThisThread();
        Bytes keys, vals;
        std::vector<uint64_t> koff, voff;
        csr(IndexBlock.Indexes, [](const block::IndexEntry &e) -> const std::string & { return e.Key; }, &keys, &koff);
        csr(DataBlock.Entries, [](const kv::Value &v) -> const kv::Value & { return v; }, &vals, &voff);
        const uint64_t m = FilterBlock.Cap(), k = FilterBlock.K();
        const uint64_t size = lsm_sst_image_size_host(koff.data(), voff.data(), 0, n, m);
        void *d_keys = d.Dev(0, pad16(keys.size()));
        void *d_koff = d.Dev(1, koff.size() * 8);
        void *d_vals = d.Dev(2, pad16(vals.size()));
        void *d_voff = d.Dev(3, voff.size() * 8);
        void *d_fs = d.Dev(4, 16);
        void *d_fo = d.Dev(5, 8);
        void *d_out = d.Dev(6, pad16(size));
        void *d_foot = d.Dev(7, 32);
        const size_t ws = lsm_build_sst_workspace_bytes(1, (uint32_t)n, m, (uint32_t)k);
        void *d_ws = d.Dev(8, ws);
        if (!keys.empty()) d.H2D(d_keys, keys.data(), keys.size());
        d.H2D(d_koff, koff.data(), koff.size() * 8);
        if (!vals.empty()) d.H2D(d_vals, vals.data(), vals.size());
        d.H2D(d_voff, voff.data(), voff.size() * 8);
        const uint64_t fs[2] = {0, n}, fo = 0;
        d.H2D(d_fs, fs, 16);
        d.H2D(d_fo, &fo, 8);
        check(lsm_build_sst(d.ctx(), (const uint8_t *)d_keys, (const uint64_t *)d_koff,
                            (const uint8_t *)d_vals, (const uint64_t *)d_voff,
                            (const uint64_t *)d_fs, 1, (uint32_t)n, m, (uint32_t)k,
                            (uint8_t *)d_out, (const uint64_t *)d_fo, (int64_t *)d_foot, d_ws, ws,
                            d.stream()),
              "lsm_build_sst");
        out->resize(size);
        int64_t foot[4];
        d.D2H(out->data(), d_out, size);
        d.D2H(foot, d_foot, 32);
        d.Sync();
        Footer.DataHandle = {foot[0], foot[1]};
        Footer.IndexHandle = {foot[2], foot[3]};
        for (size_t i = 0; i < n; i++)  // EncodeTo rewrites the offsets (sstable.go:164-169)
            IndexBlock.Indexes[i].Offset = foot[0] + (int64_t)(4 * i + voff[i]);
    } else {
        // General path: framing on the host, both regions encoded on the GPU.
        Buffer w;
        Header.EncodeTo(w);
        FilterBlock.EncodeTo(w);
        const int64_t data_off = (int64_t)w.Len();
        int64_t cur = data_off;
        for (size_t i = 0; i < n; i++) {
            IndexBlock.Indexes[i].Offset = cur;
            cur += 4 + (int64_t)DataBlock.Entries[i].size();
        }
        DataBlock.EncodeTo(w);
        Footer.DataHandle = {data_off, (int64_t)w.Len() - data_off};
        const int64_t idx_off = (int64_t)w.Len();
        Footer.IndexHandle = {idx_off, IndexBlock.Encode(w)};
        Footer.EncodeTo(w);
        *out = std::move(w.data);
    }
    image_ = *out;
    return Error();
}

Error SSTable::EncodeTo(const std::string &path) {
    Bytes img;
    Error e = EncodeImage(&img);
    if (e) return e;
    std::error_code ec;
    const auto dir = std::filesystem::path(path).parent_path();
    if (!dir.empty() && !std::filesystem::create_directories(dir, ec) && ec)
        return Error("create directory failed: mkdir " + dir.string() + ": " + ec.message());
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) return Error("open file error: " + path);
    f.write((const char *)img.data(), (std::streamsize)img.size());
    path_ = path;
    return f ? Error() : Error("encode SSTable failed: write " + path);
}

Error SSTable::DecodeImage(const Bytes &img) {
    Reader r(img);
    Error e = Header.DecodeFrom(r);
    if (e) return e.Wrap("decode Header failed");
    e = FilterBlock.DecodeFrom(r);
    if (e) return e.Wrap("decode FilterBlock failed");
    if (img.size() < (size_t)block::kFooterSize)
        return Error("decode Footer failed: seek to footer position failed: invalid argument");
    Reader fr(img.data() + img.size() - block::kFooterSize, block::kFooterSize);
    e = Footer.DecodeFrom(fr);
    if (e) return e.Wrap("decode Footer failed").Wrap("decode Footer failed");
    const int64_t io = Footer.IndexHandle.Offset;
    if (io < 0) return Error("seek to index block position failed: invalid argument");
    Reader ir(img.data() + std::min((size_t)io, img.size()), img.size() - std::min((size_t)io, img.size()));
    e = IndexBlock.DecodeFrom(ir, Footer.IndexHandle.Size);
    if (e) return e.Wrap("decode IndexBlock failed");
    image_ = img;
    return Error();
}

Error SSTable::DecodeFrom(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return Error("open file error: open " + path + ": no such file or directory");
    Bytes img((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    path_ = path;
    return DecodeImage(img);
}

Error SSTable::DecodeDataBlock(const Bytes &img) {
    const int64_t off = Footer.DataHandle.Offset;
    if (off < 0) return Error("seek to IndexBlock position failed: invalid argument");
    const size_t o = std::min((size_t)off, img.size());
    Reader r(img.data() + o, img.size() - o);
    Error e = DataBlock.DecodeFrom(r, Footer.DataHandle.Size);
    if (e) return e.Wrap("decode DataBlock failed");
    return Error();
}

std::vector<kv::KeyValuePair> SSTable::GetDataBlockFromFile(const std::string &path, Error *err) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        *err = Error("open file error: open " + path + ": no such file or directory");
        return {};
    }
    Bytes img((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    Error e = DecodeDataBlock(img);
    if (e) {
        *err = e.Wrap("decode DataBlock failed");
        return {};
    }
    return GetKeyValuePairs(err);
}

std::vector<kv::KeyValuePair> SSTable::GetKeyValuePairs(Error *err) const {
    *err = Error();
    if (DataBlock.Len() == 0 || IndexBlock.Len() == 0) return {};
    if (DataBlock.Len() != IndexBlock.Len()) {
        *err = Error("mismatched DataBlock and IndexBlock entries");
        return {};
    }
    std::vector<kv::KeyValuePair> pairs;
    pairs.reserve(DataBlock.Entries.size());
    for (size_t i = 0; i < DataBlock.Entries.size(); i++)
        pairs.push_back({IndexBlock.Indexes[i].Key, DataBlock.Entries[i]});
    return pairs;
}

kv::Value SSTable::GetValueByOffset(int64_t offset, Error *err) {
    // Point read (not the batched path): Value.DecodeFrom at the offset.
    *err = Error();
    if (offset < 0) {
        *err = Error("seek to offset failed: seek " + path_ + ": invalid argument");
        return {};
    }
    if ((size_t)offset > image_.size()) offset = (int64_t)image_.size();
    Reader r(image_.data() + offset, image_.size() - (size_t)offset);
    if (r.Len() < 4) {
        *err = Error(std::string("decode value failed: decode value length: ") + eof_or_unexpected(r.Len()));
        return {};
    }
    const uint32_t vl = ld32(r.Cur());
    if (vl > (1u << 30)) {
        *err = Error("decode value failed: invalid value length: " + std::to_string(vl));
        return {};
    }
    if (r.Len() - 4 < vl) {
        *err = Error(std::string("decode value failed: decode value: ") + eof_or_unexpected(r.Len() - 4));
        return {};
    }
    return kv::Value(r.Cur() + 4, r.Cur() + 4 + vl);
}

bool SSTable::MayContain(const kv::Key &key) {
    if (Header.MinKey > key || Header.MaxKey < key) return false;
    return FilterBlock.MayContain(key);
}

void Builder::Add(const kv::KeyValuePair &p) {
    table_.Add(p);
    size_ += p.EstimateSize();
}

void Builder::Finalize() {
    if (table_.DataBlock.Len() > 0)
        table_.Header = {table_.IndexBlock.Indexes.front().Key,
                         table_.IndexBlock.Indexes[table_.DataBlock.Len() - 1].Key};
}

SSTable &Builder::Build() {
    Finalize();
    return table_;
}

std::vector<std::vector<kv::Value>> DecodeDataBlocks(const std::vector<Bytes> &regions,
                                                     std::vector<Error> *errs) {
    std::vector<std::pair<const uint8_t *, size_t>> blocks;
    for (auto &r : regions) blocks.push_back({r.data(), r.size()});
    Decoded dec = gpu_decode(LSM_GRAMMAR_V, blocks);
    std::vector<std::vector<kv::Value>> out(regions.size());
    errs->assign(regions.size(), Error());
    for (size_t i = 0; i < regions.size(); i++) {
        const uint8_t *p = regions[i].data();
        size_t end = 0;
        for (auto &ds : dec.desc[i]) {
            out[i].emplace_back(p + ds.rec_off + 4, p + ds.rec_off + 4 + ds.val_len);
            end = ds.rec_off + 4 + ds.val_len;
        }
        if (dec.status[i] == LSM_ST_TRUNC_LEN_PREFIX) (*errs)[i] = Error("read value length failed: unexpected EOF");
        else if (dec.status[i] == LSM_ST_TRUNC_VAL)
            (*errs)[i] = Error(std::string("read value data failed: ") + eof_or_unexpected(regions[i].size() - end - 4));
        else if (dec.status[i] != LSM_OK) (*errs)[i] = Error("decode status " + std::to_string(dec.status[i]));
    }
    return out;
}

static std::string status_text(int grammar, int32_t st) {
    switch (st) {
    case LSM_ST_TRUNC_LEN_PREFIX:
        return grammar == LSM_GRAMMAR_V ? "read value length failed: unexpected EOF"
                                        : "decode key length: unexpected EOF";
    case LSM_ST_TRUNC_VAL: return "read value data failed: unexpected EOF";
    case LSM_ST_IDX_OVERRUN: return "unexpected EOF: size limit reached while reading key length";
    case LSM_ST_CAPACITY: return "record capacity exhausted";
    default: return "decode status " + std::to_string(st);
    }
}

std::vector<std::vector<kv::KeyValuePair>> DecodeFiles(const std::vector<Bytes> &images,
                                                       std::vector<Error> *errs) {
    Device &d = Device::ThisThread();
    const size_t n = images.size();
    std::vector<std::vector<kv::KeyValuePair>> out(n);
    errs->assign(n, Error());
    if (n == 0) return out;
    std::vector<uint64_t> off(n), len(n);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = total;
        len[i] = images[i].size();
        total += (images[i].size() + 15) & ~(size_t)15;
    }
    uint8_t *h_in = (uint8_t *)d.Host(0, pad16(total));
    std::memset(h_in, 0, pad16(total));
    for (size_t i = 0; i < n; i++) std::memcpy(h_in + off[i], images[i].data(), images[i].size());
    const size_t cap = total / 4 + 1;
    void *d_in = d.Dev(0, pad16(total));
    void *d_off = d.Dev(1, n * 8);
    void *d_len = d.Dev(2, n * 8);
    void *d_meta = d.Dev(3, n * sizeof(lsm_sst_meta));
    void *d_idesc = d.Dev(4, cap * sizeof(lsm_rec_desc));
    void *d_ival = d.Dev(5, cap * 8);
    void *d_ddesc = d.Dev(6, cap * sizeof(lsm_rec_desc));
    const size_t ws = lsm_decode_sst_workspace_bytes((uint32_t)n);
    void *d_ws = d.Dev(7, ws);
    d.H2D(d_in, h_in, pad16(total));
    d.H2D(d_off, off.data(), n * 8);
    d.H2D(d_len, len.data(), n * 8);
    check(lsm_decode_sst(d.ctx(), (const uint8_t *)d_in, (const uint64_t *)d_off,
                         (const uint64_t *)d_len, (uint32_t)n, nullptr, (lsm_sst_meta *)d_meta,
                         (lsm_rec_desc *)d_idesc, (int64_t *)d_ival, (lsm_rec_desc *)d_ddesc, d_ws,
                         ws, d.stream()),
          "lsm_decode_sst");
    std::vector<lsm_sst_meta> meta(n);
    d.D2H(meta.data(), d_meta, n * sizeof(lsm_sst_meta));
    d.Sync();
    static const char *const kStage[] = {"", "decode Header failed", "decode FilterBlock failed",
                                         "decode Footer failed", "decode IndexBlock failed",
                                         "decode DataBlock failed",
                                         "mismatched DataBlock and IndexBlock entries"};
    for (size_t f = 0; f < n; f++) {
        const lsm_sst_meta &m = meta[f];
        if (m.stage != LSM_SST_OK) {
            // The batch decides THAT file f fails and at which step; the
            // reference's full error text depends on the bytes at the failing
            // read, so it is rendered by the one-file path (also on the GPU),
            // which walks the same steps (sstable.go:87-127, 214-268).
            SSTable t;
            Error e = t.DecodeImage(images[f]);
            if (!e) e = t.DecodeDataBlock(images[f]);
            if (!e) t.GetKeyValuePairs(&e);
            if (!e) {  // cannot happen when the two paths agree; keep the step
                std::string msg = kStage[m.stage];
                if (m.status)
                    msg += ": " + status_text(m.stage == LSM_SST_INDEX ? LSM_GRAMMAR_IDX : LSM_GRAMMAR_V,
                                              m.status);
                e = Error(msg);
            }
            (*errs)[f] = e;
            continue;
        }
        if (m.nidx == 0 || m.ndata == 0) continue;  // GetKeyValuePairs' (nil, nil)
        std::vector<lsm_rec_desc> ki(m.nidx), vi(m.ndata);
        const size_t base = off[f] / 4;
        d.D2H(ki.data(), (lsm_rec_desc *)d_idesc + base, m.nidx * sizeof(lsm_rec_desc));
        d.D2H(vi.data(), (lsm_rec_desc *)d_ddesc + base, m.ndata * sizeof(lsm_rec_desc));
        d.Sync();
        const uint8_t *img = images[f].data();
        out[f].reserve(m.nidx);
        for (uint32_t i = 0; i < m.nidx; i++) {
            const uint64_t ko = ki[i].rec_off - off[f] + 4, vo = vi[i].rec_off - off[f] + 4;
            out[f].push_back({kv::Key((const char *)img + ko, ki[i].key_len),
                              kv::Value(img + vo, img + vo + vi[i].val_len)});
        }
    }
    return out;
}

std::vector<Bytes> BuildImages(const std::vector<kv::KeyValuePair> &sorted, uint64_t threshold,
                               uint64_t m, uint64_t k) {
    std::vector<uint64_t> koff(1, 0), voff(1, 0);
    for (auto &p : sorted) {
        koff.push_back(koff.back() + p.key.size());
        voff.push_back(voff.back() + p.value.size());
    }
    const uint64_t n = sorted.size();
    std::vector<uint64_t> fs(n + 2);
    const uint64_t nf = lsm_segment_files_host(koff.data(), voff.data(), n, threshold, fs.data());
    fs.resize(nf + 1);
    return BuildImagesAt(sorted, fs, m, k);
}

std::vector<Bytes> BuildImagesAt(const std::vector<kv::KeyValuePair> &sorted,
                                 const std::vector<uint64_t> &fs, uint64_t m, uint64_t k) {
    Device &d = Device::ThisThread();
    Bytes keys, vals;
    std::vector<uint64_t> koff, voff;
    csr(sorted, [](const kv::KeyValuePair &p) -> const std::string & { return p.key; }, &keys, &koff);
    csr(sorted, [](const kv::KeyValuePair &p) -> const kv::Value & { return p.value; }, &vals, &voff);
    const uint64_t nf = fs.empty() ? 0 : fs.size() - 1;
    std::vector<uint64_t> fo(nf), sz(nf);
    uint64_t total = 0, maxr = 0;
    for (uint64_t f = 0; f < nf; f++) {
        sz[f] = lsm_sst_image_size_host(koff.data(), voff.data(), fs[f], fs[f + 1], m);
        fo[f] = total;
        total += (sz[f] + 15) & ~(uint64_t)15;
        maxr = std::max(maxr, fs[f + 1] - fs[f]);
    }
    std::vector<Bytes> out(nf);
    if (nf == 0) return out;
    void *d_keys = d.Dev(0, pad16(keys.size()));
    void *d_koff = d.Dev(1, koff.size() * 8);
    void *d_vals = d.Dev(2, pad16(vals.size()));
    void *d_voff = d.Dev(3, voff.size() * 8);
    void *d_fs = d.Dev(4, fs.size() * 8);
    void *d_fo = d.Dev(5, fo.size() * 8);
    void *d_out = d.Dev(6, pad16(total));
    const size_t ws = lsm_build_sst_workspace_bytes((uint32_t)nf, (uint32_t)maxr, m, (uint32_t)k);
    void *d_ws = d.Dev(8, ws);
    if (!keys.empty()) d.H2D(d_keys, keys.data(), keys.size());
    d.H2D(d_koff, koff.data(), koff.size() * 8);
    if (!vals.empty()) d.H2D(d_vals, vals.data(), vals.size());
    d.H2D(d_voff, voff.data(), voff.size() * 8);
    d.H2D(d_fs, fs.data(), fs.size() * 8);
    d.H2D(d_fo, fo.data(), fo.size() * 8);
    check(lsm_build_sst(d.ctx(), (const uint8_t *)d_keys, (const uint64_t *)d_koff,
                        (const uint8_t *)d_vals, (const uint64_t *)d_voff, (const uint64_t *)d_fs,
                        (uint32_t)nf, (uint32_t)maxr, m, (uint32_t)k, (uint8_t *)d_out,
                        (const uint64_t *)d_fo, nullptr, d_ws, ws, d.stream()),
          "lsm_build_sst");
    for (uint64_t f = 0; f < nf; f++) {
        out[f].resize(sz[f]);
        d.D2H(out[f].data(), (uint8_t *)d_out + fo[f], sz[f]);
    }
    d.Sync();
    return out;
}

std::vector<SSTable> CompactAndMergeKVs(const std::vector<kv::KeyValuePair> &kvs, int level) {
    std::vector<SSTable> results;
    const size_t n = kvs.size();
    if (n == 0) return results;  // no builder.size: no table (merge.go:88-91)
    Device &d = Device::ThisThread();
    // the pairs as views: [4 bytes][key] [4 bytes][value], the IDX / V
    // descriptor convention (bytes at rec_off + 4)
    size_t total = 0;
    for (auto &p : kvs) total += 8 + p.key.size() + p.value.size();
    uint8_t *h = (uint8_t *)d.Host(0, pad16(total));
    std::vector<lsm_rec_desc> kd(n), vd(n);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const kv::KeyValuePair &p = kvs[i];
        kd[i] = lsm_rec_desc{at, (uint32_t)p.key.size(), 0};
        std::memset(h + at, 0, 4);
        std::memcpy(h + at + 4, p.key.data(), p.key.size());
        at += 4 + p.key.size();
        vd[i] = lsm_rec_desc{at, 0, (uint32_t)p.value.size()};
        std::memset(h + at, 0, 4);
        if (!p.value.empty()) std::memcpy(h + at + 4, p.value.data(), p.value.size());
        at += 4 + p.value.size();
    }
    std::memset(h + at, 0, pad16(total) - at);
    void *d_buf = d.Dev(0, pad16(total));
    void *d_kd = d.Dev(1, n * sizeof(lsm_rec_desc));
    void *d_vd = d.Dev(2, n * sizeof(lsm_rec_desc));
    void *d_out = d.Dev(3, n * 4);
    void *d_fs = d.Dev(4, (n + 1) * 8);
    const size_t ws = lsm_merge_kvs_workspace_bytes(n);
    void *d_ws = d.Dev(5, ws);
    d.H2D(d_buf, h, pad16(total));
    d.H2D(d_kd, kd.data(), n * sizeof(lsm_rec_desc));
    d.H2D(d_vd, vd.data(), n * sizeof(lsm_rec_desc));
    uint64_t counts[2] = {0, 0};
    check(lsm_merge_kvs(d.ctx(), (const uint8_t *)d_buf, (const lsm_rec_desc *)d_kd,
                        (const lsm_rec_desc *)d_vd, n, level, kMaxSSTableSize, (uint32_t *)d_out,
                        (uint64_t *)d_fs, counts, d_ws, ws, d.stream()),
          "lsm_merge_kvs");
    std::vector<uint32_t> out(counts[0]);
    std::vector<uint64_t> fs(counts[1] + 1);
    if (counts[0]) d.D2H(out.data(), d_out, counts[0] * 4);
    d.D2H(fs.data(), d_fs, fs.size() * 8);
    d.Sync();
    std::vector<kv::KeyValuePair> written;
    written.reserve(out.size());
    for (uint32_t i : out) written.push_back(kvs[i]);
    const std::vector<Bytes> images = BuildImagesAt(written, fs);
    for (const Bytes &img : images) {
        SSTable t;
        Error e = t.DecodeImage(img);
        if (!e) e = t.DecodeDataBlock(img);
        if (e) throw std::runtime_error("CompactAndMergeKVs: built image does not decode: " + e.Message());
        t.level = level;
        results.push_back(std::move(t));
    }
    return results;
}

// wal.Recover of every log and the memtables' order on the device (slots 0-9):
// lsm_wal_replay (offset-addressed: log w's records at slot off[w] / 8), then
// lsm_memtable_order.  h = the logs as uploaded (pinned host copy).
struct OrderedWALs {
    size_t nlog, total;
    uint64_t nslot;
    uint8_t *h;
    void *d_wal, *d_desc, *d_st, *d_idx;
    uint64_t *d_fsc;  // file starts (nlog + 1), then the three counts
};

static OrderedWALs ReplayAndOrder(Device &d, const std::vector<Bytes> &wals, int scan) {
    OrderedWALs r{};
    const size_t nlog = r.nlog = wals.size();
    std::vector<uint64_t> off(nlog);
    std::vector<uint32_t> len(nlog);
    size_t total = 0, max_len = 0;
    for (size_t w = 0; w < nlog; w++) {
        off[w] = total;
        len[w] = (uint32_t)wals[w].size();
        max_len = std::max(max_len, wals[w].size());
        total += (wals[w].size() + 15) & ~(size_t)15;
    }
    r.total = total;
    uint8_t *h = r.h = (uint8_t *)d.Host(0, pad16(total));
    std::memset(h, 0, pad16(total));
    for (size_t w = 0; w < nlog; w++)
        if (!wals[w].empty()) std::memcpy(h + off[w], wals[w].data(), wals[w].size());
    const uint64_t nslot = r.nslot = total / 8 + 1;
    const uint32_t maxrec = (uint32_t)lsm_max_records(LSM_GRAMMAR_KV, max_len);
    void *d_wal = r.d_wal = d.Dev(0, pad16(total));
    void *d_off = d.Dev(1, nlog * 8);
    void *d_len = d.Dev(2, nlog * 4);
    void *d_desc = r.d_desc = d.Dev(3, nslot * sizeof(lsm_rec_desc));
    void *d_nrec = d.Dev(4, nlog * 4);
    void *d_st = r.d_st = d.Dev(5, nlog * 4);
    const size_t wws = lsm_wal_replay_workspace_bytes((uint32_t)nlog, (uint32_t)max_len);
    void *d_wws = d.Dev(6, wws);
    d.H2D(d_wal, h, pad16(total));
    d.H2D(d_off, off.data(), nlog * 8);
    d.H2D(d_len, len.data(), nlog * 4);
    lsm_decode_out o{};
    o.desc = (lsm_rec_desc *)d_desc;
    o.nrec = (uint32_t *)d_nrec;
    o.status = (int32_t *)d_st;
    check(lsm_wal_replay(d.ctx(), (const uint8_t *)d_wal, (const uint64_t *)d_off, (const uint32_t *)d_len,
                         (uint32_t)nlog, (uint32_t)max_len, &o, d_wws, wws, d.stream()),
          "lsm_wal_replay");
    // the memtables: each log's last record per key, in key order
    void *d_idx = r.d_idx = d.Dev(7, nslot * 4);
    uint64_t *d_fsc = r.d_fsc = (uint64_t *)d.Dev(8, (nlog + 1 + 3) * 8);
    const size_t ows = lsm_memtable_order_workspace_bytes((uint32_t)nlog, nslot, maxrec);
    void *d_ows = d.Dev(9, ows);
    check(lsm_memtable_order(d.ctx(), (const uint8_t *)d_wal, (const lsm_rec_desc *)d_desc, nullptr,
                             (const uint64_t *)d_off, (const uint32_t *)d_nrec, (const int32_t *)d_st,
                             (uint32_t)nlog, nslot, maxrec, scan, (uint32_t *)d_idx, d_fsc,
                             d_fsc + nlog + 1, d_ows, ows, d.stream()),
          "lsm_memtable_order");
    return r;
}

std::vector<Bytes> BuildSSTablesFromWALs(const std::vector<Bytes> &wals, int scan,
                                         std::vector<int32_t> *status, uint64_t m, uint64_t k) {
    const size_t nlog = wals.size();
    std::vector<Bytes> out(nlog);
    if (status) status->assign(nlog, 0);
    if (nlog == 0) return out;  // nothing to flush: no device call
    Device &d = Device::ThisThread();
    const OrderedWALs r = ReplayAndOrder(d, wals, scan);
    const size_t total = r.total;
    const uint64_t nslot = r.nslot;
    void *d_wal = r.d_wal, *d_desc = r.d_desc, *d_st = r.d_st, *d_idx = r.d_idx;
    uint64_t *d_fsc = r.d_fsc;
    // their keys packed; the values stay in the WAL bytes
    const uint64_t nout_max = std::min<uint64_t>(nslot, total / 8);
    void *d_keys = d.Dev(10, pad16(total));
    void *d_koff = d.Dev(11, (nout_max + 1) * 8);
    void *d_voff = d.Dev(12, (nout_max + 1) * 8);
    const size_t gws = lsm_gather_kvs_workspace_bytes(nout_max);
    void *d_gws = d.Dev(13, gws);
    check(lsm_gather_kvs_dev(d.ctx(), (const uint8_t *)d_wal, (const lsm_rec_desc *)d_desc, nullptr,
                             (const uint32_t *)d_idx, d_fsc + nlog + 1, nout_max, (uint8_t *)d_keys,
                             (uint64_t *)d_koff, nullptr, (uint64_t *)d_voff, d_gws, gws, d.stream()),
          "lsm_gather_kvs_dev");
    std::vector<uint64_t> fsc(nlog + 1 + 3);
    std::vector<int32_t> st(nlog);
    d.D2H(fsc.data(), d_fsc, fsc.size() * 8);  // the one read-back before the build
    d.D2H(st.data(), d_st, nlog * 4);
    d.Sync();
    if (status) *status = st;
    // one file per non-empty memtable (an empty one has no Header to encode)
    std::vector<uint64_t> fs;
    std::vector<size_t> log_of;
    for (size_t w = 0; w < nlog; w++)
        if (fsc[w + 1] > fsc[w]) {
            fs.push_back(fsc[w]);
            log_of.push_back(w);
        }
    const uint32_t nf = (uint32_t)fs.size();
    if (nf == 0) return out;
    fs.push_back(fsc[nlog]);
    const uint32_t maxr = (uint32_t)(fsc[nlog + 3] & ~LSM_MEMTABLE_OVERFLOW);
    void *d_fs = d.Dev(14, fs.size() * 8);
    void *d_sz = d.Dev(15, nf * 8);
    void *d_fo = d.Dev(16, (nf + 1) * 8);
    d.H2D(d_fs, fs.data(), fs.size() * 8);
    check(lsm_sst_layout(d.ctx(), (const uint64_t *)d_koff, (const uint64_t *)d_voff, (const uint64_t *)d_fs,
                         nf, m, 16, (uint64_t *)d_sz, (uint64_t *)d_fo, d.stream()),
          "lsm_sst_layout");
    const size_t bound = nf * (lsm_filter_block_size(m) + 40 + 15) + 16 * fsc[nlog] + 4 * total;
    void *d_out = d.Dev(17, pad16(bound));
    const size_t bws = lsm_build_sst_workspace_bytes(nf, maxr, m, (uint32_t)k);
    void *d_bws = d.Dev(18, bws);
    check(lsm_build_sst_views(d.ctx(), (const uint8_t *)d_keys, (const uint64_t *)d_koff,
                              (const uint8_t *)d_wal, (const lsm_rec_desc *)d_desc, nullptr,
                              (const uint32_t *)d_idx, (const uint64_t *)d_voff, (const uint64_t *)d_fs, nf,
                              maxr, m, (uint32_t)k, (uint8_t *)d_out, (const uint64_t *)d_fo, nullptr, d_bws,
                              bws, d.stream()),
          "lsm_build_sst_views");
    std::vector<uint64_t> sz(nf), fo(nf + 1);
    d.D2H(sz.data(), d_sz, nf * 8);
    d.D2H(fo.data(), d_fo, (nf + 1) * 8);
    d.Sync();
    for (uint32_t f = 0; f < nf; f++) {
        out[log_of[f]].resize(sz[f]);
        d.D2H(out[log_of[f]].data(), (uint8_t *)d_out + fo[f], sz[f]);
    }
    d.Sync();
    return out;
}

// A tree on the device (slots 20-28): the images in one buffer, decoded, and
// the sparse index over them -- what lsm_search, lsm_db_get and lsm_tree_scan
// take.  h_img is the host copy the value views are read from.
struct DeviceTree {
    uint8_t *h_img = nullptr;
    void *d_img = nullptr, *d_off = nullptr, *d_len = nullptr, *d_meta = nullptr, *d_idesc = nullptr,
         *d_ival = nullptr, *d_index = nullptr;
};

static DeviceTree UploadTree(Device &d, const std::vector<Bytes> &images) {
    DeviceTree t;
    const size_t nfile = images.size();
    if (!nfile) return t;
    std::vector<uint64_t> off(nfile), len(nfile);
    size_t total = 0;
    for (size_t f = 0; f < nfile; f++) {
        off[f] = total;
        len[f] = images[f].size();
        total += (images[f].size() + 15) & ~(size_t)15;
    }
    t.h_img = (uint8_t *)d.Host(2, pad16(total));
    std::memset(t.h_img, 0, pad16(total));
    for (size_t f = 0; f < nfile; f++) std::memcpy(t.h_img + off[f], images[f].data(), images[f].size());
    const size_t cap = total / 4 + 1;
    t.d_img = d.Dev(20, pad16(total));
    t.d_off = d.Dev(21, nfile * 8);
    t.d_len = d.Dev(22, nfile * 8);
    t.d_meta = d.Dev(23, nfile * sizeof(lsm_sst_meta));
    t.d_idesc = d.Dev(24, cap * sizeof(lsm_rec_desc));
    t.d_ival = d.Dev(25, cap * 8);
    void *d_ddesc = d.Dev(26, cap * sizeof(lsm_rec_desc));
    const size_t dws = lsm_decode_sst_workspace_bytes((uint32_t)nfile);
    void *d_dws = d.Dev(27, dws);
    d.H2D(t.d_img, t.h_img, pad16(total));
    d.H2D(t.d_off, off.data(), nfile * 8);
    d.H2D(t.d_len, len.data(), nfile * 8);
    check(lsm_decode_sst(d.ctx(), (const uint8_t *)t.d_img, (const uint64_t *)t.d_off, (const uint64_t *)t.d_len,
                         (uint32_t)nfile, nullptr, (lsm_sst_meta *)t.d_meta, (lsm_rec_desc *)t.d_idesc,
                         (int64_t *)t.d_ival, (lsm_rec_desc *)d_ddesc, d_dws, dws, d.stream()),
          "lsm_decode_sst");
    t.d_index = d.Dev(28, lsm_level_index_bytes((uint32_t)nfile));
    check(lsm_level_index_build(d.ctx(), (const uint8_t *)t.d_img, (const uint64_t *)t.d_off,
                                (const lsm_sst_meta *)t.d_meta, (uint32_t)nfile, t.d_index, d.stream()),
          "lsm_level_index_build");
    d.Sync();  // off / len are read by the copies queued above
    return t;
}

// lsm_memtable_search's index over r's nodes (slot 16); *ib = its bytes.
static void *BuildSearchIndex(Device &d, const OrderedWALs &r, size_t *ib) {
    *ib = lsm_memtable_search_index_bytes(r.nslot);
    void *d_index = d.Dev(16, *ib);
    check(lsm_memtable_search_index_build(d.ctx(), (const uint8_t *)r.d_wal, (const lsm_rec_desc *)r.d_desc,
                                          (const uint32_t *)r.d_idx, r.d_fsc, (uint32_t)r.nlog, r.nslot, d_index,
                                          *ib, d.stream()),
          "lsm_memtable_search_index_build");
    return d_index;
}

// n keys as a CSR on the device: the bytes (zero padded to 16) in slot dslot
// by way of pinned slot hslot, the offsets in slot dslot + 1.  off is the
// offsets' host copy, which the queued upload reads.
struct DeviceCSR {
    void *d_bytes = nullptr, *d_off = nullptr;
    std::vector<uint64_t> off;
};

template <class F>
static DeviceCSR UploadCSR(Device &d, size_t n, F key, int dslot, int hslot) {
    DeviceCSR c;
    c.off.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) c.off[i + 1] = c.off[i] + key(i).size();
    const size_t bytes = pad16(c.off[n]);
    uint8_t *h = (uint8_t *)d.Host(hslot, bytes);
    std::memset(h, 0, bytes);
    for (size_t i = 0; i < n; i++) std::memcpy(h + c.off[i], key(i).data(), key(i).size());
    c.d_bytes = d.Dev(dslot, bytes);
    c.d_off = d.Dev(dslot + 1, (n + 1) * 8);
    d.H2D(c.d_bytes, h, bytes);
    d.H2D(c.d_off, c.off.data(), (n + 1) * 8);
    return c;
}

// The probe keys of a Search or a Get (slots 10-11).
static DeviceCSR UploadKeys(Device &d, const std::vector<kv::Key> &keys) {
    return UploadCSR(d, keys.size(), [&](size_t i) -> const kv::Key & { return keys[i]; }, 10, 1);
}

// The ranges of a scan (slots 10-14) and its outputs (15, 30-34), n = nq *
// limit entries; Read queues the outputs' copies back.
struct DeviceScan {
    DeviceCSR lo, hi;
    void *d_flags, *d_count, *d_more, *d_key, *d_value, *d_table, *d_result;
    std::vector<uint32_t> count;
    std::vector<uint8_t> more;
    std::vector<lsm_rec_desc> key, value;
    std::vector<int32_t> table, result;

    DeviceScan(Device &d, const std::vector<ScanRange> &ranges, size_t n)
        : count(ranges.size()), more(ranges.size()), key(n), value(n), table(n), result(n) {
        const size_t nq = ranges.size();
        lo = UploadCSR(d, nq, [&](size_t q) -> const kv::Key & { return ranges[q].lo; }, 10, 1);
        hi = UploadCSR(d, nq, [&](size_t q) -> const kv::Key & { return ranges[q].hi; }, 12, 3);
        uint8_t *h_flags = (uint8_t *)d.Host(4, pad16(nq));
        std::memset(h_flags, 0, pad16(nq));
        for (size_t q = 0; q < nq; q++) h_flags[q] = ranges[q].no_upper ? LSM_SCAN_NO_UPPER : 0;
        d_flags = d.Dev(14, pad16(nq));
        d.H2D(d_flags, h_flags, pad16(nq));
        d_count = d.Dev(15, nq * 4);
        d_more = d.Dev(30, pad16(nq));
        d_key = d.Dev(31, n * sizeof(lsm_rec_desc));
        d_value = d.Dev(32, n * sizeof(lsm_rec_desc));
        d_table = d.Dev(33, n * 4);
        d_result = d.Dev(34, n * 4);
    }

    void Read(Device &d) {
        d.D2H(count.data(), d_count, count.size() * 4);
        d.D2H(more.data(), d_more, more.size());
        d.D2H(key.data(), d_key, key.size() * sizeof(lsm_rec_desc));
        d.D2H(value.data(), d_value, value.size() * sizeof(lsm_rec_desc));
        d.D2H(table.data(), d_table, table.size() * 4);
        d.D2H(result.data(), d_result, result.size() * 4);
    }
};

std::vector<ScanResult> ScanImages(const std::vector<Bytes> &images, const uint32_t *level_start,
                                   const std::vector<ScanRange> &ranges, uint32_t limit, int mode) {
    if (mode != LSM_SCAN_RAW && mode != LSM_SCAN_LIVE) throw std::invalid_argument("ScanImages: unknown mode");
    if (limit == 0) throw std::invalid_argument("ScanImages: limit is 0");
    if (!level_start || level_start[LSM_SEARCH_LEVELS] != images.size())
        throw std::invalid_argument("ScanImages: level_start does not end at the number of images");
    const size_t nq = ranges.size();
    if ((uint64_t)nq * limit >= (1ull << 32)) throw std::invalid_argument("ScanImages: too many entries");
    std::vector<ScanResult> out(nq);
    // no range, or no table: nothing in any range; no device call
    if (nq == 0 || images.empty()) return out;
    Device &d = Device::ThisThread();
    const DeviceTree t = UploadTree(d, images);
    // the ranges (slots 10-14), the outputs (15, 30-34) and the workspace (35)
    const size_t n = nq * (size_t)limit;
    DeviceScan sc(d, ranges, n);
    const size_t ws = lsm_tree_scan_workspace_bytes(level_start, nq);
    void *d_ws = d.Dev(35, ws ? ws : 16);
    // no Seek tree: the Seek walks each table's decoded index (the same answers)
    check(lsm_tree_scan(d.ctx(), (const uint8_t *)t.d_img, t.d_index, level_start, (const uint64_t *)t.d_off,
                        (const uint64_t *)t.d_len, (const lsm_sst_meta *)t.d_meta, nullptr,
                        (const lsm_rec_desc *)t.d_idesc, (const int64_t *)t.d_ival, nullptr, 0, 0,
                        (const uint8_t *)sc.lo.d_bytes, (const uint64_t *)sc.lo.d_off,
                        (const uint8_t *)sc.hi.d_bytes, (const uint64_t *)sc.hi.d_off,
                        (const uint8_t *)sc.d_flags, nq, limit, mode, (uint32_t *)sc.d_count,
                        (uint8_t *)sc.d_more, (lsm_rec_desc *)sc.d_key, (lsm_rec_desc *)sc.d_value,
                        (int32_t *)sc.d_table, (int32_t *)sc.d_result, d_ws, ws, d.stream()),
          "lsm_tree_scan");
    sc.Read(d);
    d.Sync();
    for (size_t q = 0; q < nq; q++) {
        out[q].more = sc.more[q] != 0;
        out[q].entries.resize(sc.count[q]);
        for (uint32_t j = 0; j < sc.count[q]; j++) {
            const size_t o = q * (size_t)limit + j;
            const lsm_rec_desc &k = sc.key[o], &v = sc.value[o];
            ScanEntry &e = out[q].entries[j];
            e.key.assign((const char *)t.h_img + k.rec_off + 4, k.key_len);
            e.table = sc.table[o];
            e.result = sc.result[o];
            if (e.result == LSM_GET_FOUND)
                e.value.assign(t.h_img + v.rec_off + 4, t.h_img + v.rec_off + 4 + v.val_len);
        }
    }
    return out;
}

}  // namespace sstable

namespace memtables {

std::vector<SearchResult> SearchWALs(const std::vector<Bytes> &wals, const std::vector<kv::Key> &keys) {
    std::vector<SearchResult> out(keys.size());
    if (wals.empty() || keys.empty()) return out;  // every key misses: no device call
    Device &d = Device::ThisThread();
    const sstable::OrderedWALs r = sstable::ReplayAndOrder(d, wals, LSM_MEMTABLE_ALL);
    const size_t nkeys = keys.size();
    const sstable::DeviceCSR k = sstable::UploadKeys(d, keys);
    void *d_res = d.Dev(12, nkeys * 4);
    void *d_log = d.Dev(13, nkeys * 4);
    void *d_slot = d.Dev(14, nkeys * 4);
    void *d_val = d.Dev(15, nkeys * sizeof(lsm_rec_desc));
    size_t ib = 0;
    void *d_index = sstable::BuildSearchIndex(d, r, &ib);
    check(lsm_memtable_search(d.ctx(), (const uint8_t *)r.d_wal, (const lsm_rec_desc *)r.d_desc,
                              (const uint32_t *)r.d_idx, r.d_fsc, (uint32_t)r.nlog, d_index, ib,
                              (const uint8_t *)k.d_bytes, (const uint64_t *)k.d_off, nkeys, (int32_t *)d_res,
                              (int32_t *)d_log, (uint32_t *)d_slot, (lsm_rec_desc *)d_val, d.stream()),
          "lsm_memtable_search");
    std::vector<int32_t> res(nkeys), log(nkeys);
    std::vector<lsm_rec_desc> val(nkeys);
    d.D2H(res.data(), d_res, nkeys * 4);
    d.D2H(log.data(), d_log, nkeys * 4);
    d.D2H(val.data(), d_val, nkeys * sizeof(lsm_rec_desc));
    d.Sync();
    for (size_t i = 0; i < nkeys; i++) {
        out[i].result = res[i];
        out[i].log = log[i];
        if (res[i] == LSM_MEM_VALUE)  // the view is into the uploaded logs
            out[i].value.assign(r.h + val[i].rec_off + 4, r.h + val[i].rec_off + 4 + val[i].val_len);
    }
    return out;
}

}  // namespace memtables

namespace database {

std::vector<GetResult> GetFromWALs(const std::vector<Bytes> &wals, const std::vector<Bytes> &images,
                                   const uint32_t *level_start, const std::vector<kv::Key> &keys,
                                   int mode) {
    if (mode != LSM_DBGET_EXACT && mode != LSM_DBGET_TOMBSTONE_HIDES)
        throw std::invalid_argument("GetFromWALs: unknown mode");
    if (!level_start || level_start[LSM_SEARCH_LEVELS] != images.size())
        throw std::invalid_argument("GetFromWALs: level_start does not end at the number of images");
    std::vector<GetResult> out(keys.size());
    // no memtable and no table: every Get is (nil, nil); no device call
    if (keys.empty() || (wals.empty() && images.empty())) return out;
    Device &d = Device::ThisThread();
    const size_t nkeys = keys.size(), nlog = wals.size();
    // the memtables (slots 0-9 and 16), when there are logs
    sstable::OrderedWALs r{};
    void *d_mem_index = nullptr;
    size_t ib = 0;
    if (nlog) {
        r = sstable::ReplayAndOrder(d, wals, LSM_MEMTABLE_ALL);
        d_mem_index = sstable::BuildSearchIndex(d, r, &ib);
    }
    // the tree (slots 20-28): the images in one buffer, decoded, and the sparse index over them
    const sstable::DeviceTree t = sstable::UploadTree(d, images);
    uint8_t *h_img = t.h_img;
    void *d_img = t.d_img, *d_off = t.d_off, *d_len = t.d_len, *d_meta = t.d_meta, *d_idesc = t.d_idesc,
         *d_ival = t.d_ival, *d_index = t.d_index;
    // the keys (slots 10-11) and the outputs (12-15, 30-33)
    const sstable::DeviceCSR k = sstable::UploadKeys(d, keys);
    void *d_res = d.Dev(12, nkeys * 4), *d_log = d.Dev(13, nkeys * 4), *d_slot = d.Dev(14, nkeys * 4);
    void *d_val = d.Dev(15, nkeys * sizeof(lsm_rec_desc));
    void *d_level = d.Dev(30, nkeys * 4), *d_table = d.Dev(31, nkeys * 4), *d_tres = d.Dev(32, nkeys * 4);
    void *d_src = d.Dev(33, nkeys * 4);
    const size_t ws = lsm_db_get_workspace_bytes(level_start, nkeys);
    void *d_ws = d.Dev(34, ws ? ws : 16);
    // no Seek tree: the Seek walks each table's decoded index (the same answers)
    check(lsm_db_get(d.ctx(), (const uint8_t *)r.d_wal, (const lsm_rec_desc *)r.d_desc,
                     (const uint32_t *)r.d_idx, r.d_fsc, (uint32_t)nlog, d_mem_index, ib,
                     (const uint8_t *)d_img, d_index, level_start, (const uint64_t *)d_off,
                     (const uint64_t *)d_len, (const lsm_sst_meta *)d_meta, nullptr,
                     (const lsm_rec_desc *)d_idesc, (const int64_t *)d_ival, nullptr, 0, 0,
                     (const uint8_t *)k.d_bytes, (const uint64_t *)k.d_off, nkeys, mode, (int32_t *)d_res,
                     (int32_t *)d_log, (uint32_t *)d_slot, (int32_t *)d_level, (int32_t *)d_table,
                     (int32_t *)d_tres, (lsm_rec_desc *)d_val, (int32_t *)d_src, d_ws, ws, d.stream()),
          "lsm_db_get");
    std::vector<int32_t> res(nkeys), log(nkeys), level(nkeys), table(nkeys), tres(nkeys), src(nkeys);
    std::vector<lsm_rec_desc> val(nkeys);
    d.D2H(res.data(), d_res, nkeys * 4);
    d.D2H(log.data(), d_log, nkeys * 4);
    d.D2H(level.data(), d_level, nkeys * 4);
    d.D2H(table.data(), d_table, nkeys * 4);
    d.D2H(tres.data(), d_tres, nkeys * 4);
    d.D2H(src.data(), d_src, nkeys * 4);
    d.D2H(val.data(), d_val, nkeys * sizeof(lsm_rec_desc));
    d.Sync();
    for (size_t i = 0; i < nkeys; i++) {
        GetResult &g = out[i];
        g.src = src[i];
        g.mem_result = res[i];
        g.log = log[i];
        g.level = level[i];
        g.table = table[i];
        g.result = tres[i];
        // d_src says which buffer the view is into: the logs or the images
        const uint8_t *base = src[i] == LSM_SRC_MEMTABLE ? r.h : src[i] == LSM_SRC_SSTABLE ? h_img : nullptr;
        const bool has = src[i] == LSM_SRC_MEMTABLE ? res[i] == LSM_MEM_VALUE
                                                    : src[i] == LSM_SRC_SSTABLE && tres[i] == LSM_GET_FOUND;
        if (base && has) g.value.assign(base + val[i].rec_off + 4, base + val[i].rec_off + 4 + val[i].val_len);
    }
    return out;
}

std::vector<ScanResult> ScanFromWALs(const std::vector<Bytes> &wals, const std::vector<Bytes> &images,
                                     const uint32_t *level_start, const std::vector<sstable::ScanRange> &ranges,
                                     uint32_t limit, int mode) {
    if (mode != LSM_SCAN_RAW && mode != LSM_SCAN_LIVE) throw std::invalid_argument("ScanFromWALs: unknown mode");
    if (limit == 0) throw std::invalid_argument("ScanFromWALs: limit is 0");
    if (!level_start || level_start[LSM_SEARCH_LEVELS] != images.size())
        throw std::invalid_argument("ScanFromWALs: level_start does not end at the number of images");
    const size_t nq = ranges.size(), nlog = wals.size(), nfile = images.size();
    if ((uint64_t)nq * limit >= (1ull << 32)) throw std::invalid_argument("ScanFromWALs: too many entries");
    if (nlog > 65535) throw std::invalid_argument("ScanFromWALs: more than 65535 logs");
    std::vector<ScanResult> out(nq);
    // no range, or neither a memtable nor a table: nothing in any range; no device call
    if (nq == 0 || (nlog == 0 && nfile == 0)) return out;
    Device &d = Device::ThisThread();
    // the memtables (slots 0-9 and 16), when there are logs
    sstable::OrderedWALs r{};
    void *d_mem_index = nullptr;
    size_t ib = 0;
    if (nlog) {
        r = sstable::ReplayAndOrder(d, wals, LSM_MEMTABLE_ALL);
        d_mem_index = sstable::BuildSearchIndex(d, r, &ib);
    }
    // the tree (slots 20-28) and its Seek tree (slot 29), sized for the largest table
    const sstable::DeviceTree t = sstable::UploadTree(d, images);
    void *d_tree = nullptr;
    uint32_t tree_nidx = 0;
    size_t tree_bytes = 0;
    if (nfile) {
        std::vector<lsm_sst_meta> meta(nfile);
        d.D2H(meta.data(), t.d_meta, nfile * sizeof(lsm_sst_meta));
        d.Sync();
        for (const lsm_sst_meta &m : meta) tree_nidx = std::max(tree_nidx, m.nidx);
        tree_bytes = lsm_level_get_tree_bytes((uint32_t)nfile, tree_nidx);
        if (tree_bytes) {
            d_tree = d.Dev(29, tree_bytes);
            check(lsm_level_get_tree_build(d.ctx(), (const uint8_t *)t.d_img, (const uint64_t *)t.d_off,
                                           (const lsm_sst_meta *)t.d_meta, (uint32_t)nfile, nullptr,
                                           (const lsm_rec_desc *)t.d_idesc, tree_nidx, d_tree, tree_bytes,
                                           d.stream()),
                  "lsm_level_get_tree_build");
        }
    }
    // the ranges (slots 10-14), the outputs (15, 30-34, 36) and the workspace (35)
    const size_t n = nq * (size_t)limit;
    sstable::DeviceScan sc(d, ranges, n);
    void *d_src = d.Dev(36, n * 4);
    const size_t ws = lsm_db_scan_workspace_bytes((uint32_t)nlog, level_start, nq);
    void *d_ws = d.Dev(35, ws ? ws : 16);
    check(lsm_db_scan(d.ctx(), (const uint8_t *)r.d_wal, (const lsm_rec_desc *)r.d_desc, (const uint32_t *)r.d_idx,
                      r.d_fsc, (uint32_t)nlog, d_mem_index, ib, (const uint8_t *)t.d_img, t.d_index, level_start,
                      (const uint64_t *)t.d_off, (const uint64_t *)t.d_len, (const lsm_sst_meta *)t.d_meta, nullptr,
                      (const lsm_rec_desc *)t.d_idesc, (const int64_t *)t.d_ival, d_tree, tree_nidx, tree_bytes,
                      (const uint8_t *)sc.lo.d_bytes, (const uint64_t *)sc.lo.d_off, (const uint8_t *)sc.hi.d_bytes,
                      (const uint64_t *)sc.hi.d_off, (const uint8_t *)sc.d_flags, nq, limit, mode,
                      (uint32_t *)sc.d_count, (uint8_t *)sc.d_more, (lsm_rec_desc *)sc.d_key,
                      (lsm_rec_desc *)sc.d_value, (int32_t *)d_src, (int32_t *)sc.d_table, (int32_t *)sc.d_result,
                      d_ws, ws, d.stream()),
          "lsm_db_scan");
    std::vector<int32_t> src(n);
    sc.Read(d);
    d.D2H(src.data(), d_src, n * 4);
    d.Sync();
    for (size_t q = 0; q < nq; q++) {
        out[q].more = sc.more[q] != 0;
        out[q].entries.resize(sc.count[q]);
        for (uint32_t j = 0; j < sc.count[q]; j++) {
            const size_t o = q * (size_t)limit + j;
            const lsm_rec_desc &k = sc.key[o], &v = sc.value[o];
            ScanEntry &e = out[q].entries[j];
            // d_src says which buffer the views are into: the logs or the images
            const uint8_t *base = src[o] == LSM_SRC_MEMTABLE ? r.h : t.h_img;
            e.key.assign((const char *)base + k.rec_off + 4, k.key_len);
            e.src = src[o];
            e.table = sc.table[o];
            e.result = sc.result[o];
            if (e.result == LSM_GET_FOUND) e.value.assign(base + v.rec_off + 4, base + v.rec_off + 4 + v.val_len);
        }
    }
    return out;
}

std::vector<ScanResult> ScanFromWALsPacked(const std::vector<Bytes> &wals, const std::vector<Bytes> &images,
                                           const uint32_t *level_start,
                                           const std::vector<sstable::ScanRange> &ranges, uint32_t limit,
                                           int mode) {
    if (mode != LSM_SCAN_RAW && mode != LSM_SCAN_LIVE)
        throw std::invalid_argument("ScanFromWALsPacked: unknown mode");
    if (limit == 0) throw std::invalid_argument("ScanFromWALsPacked: limit is 0");
    if (!level_start || level_start[LSM_SEARCH_LEVELS] != images.size())
        throw std::invalid_argument("ScanFromWALsPacked: level_start does not end at the number of images");
    const size_t nq = ranges.size(), nlog = wals.size(), nfile = images.size();
    if ((uint64_t)nq * limit >= (1ull << 32)) throw std::invalid_argument("ScanFromWALsPacked: too many entries");
    if (nlog > 65535) throw std::invalid_argument("ScanFromWALsPacked: more than 65535 logs");
    std::vector<ScanResult> out(nq);
    // no range, or neither a memtable nor a table: nothing in any range; no device call
    if (nq == 0 || (nlog == 0 && nfile == 0)) return out;
    Device &d = Device::ThisThread();
    // the memtables, the tree and its Seek tree: ScanFromWALs's setup, slot for slot
    sstable::OrderedWALs r{};
    void *d_mem_index = nullptr;
    size_t ib = 0;
    if (nlog) {
        r = sstable::ReplayAndOrder(d, wals, LSM_MEMTABLE_ALL);
        d_mem_index = sstable::BuildSearchIndex(d, r, &ib);
    }
    const sstable::DeviceTree t = sstable::UploadTree(d, images);
    void *d_tree = nullptr;
    uint32_t tree_nidx = 0;
    size_t tree_bytes = 0;
    if (nfile) {
        std::vector<lsm_sst_meta> meta(nfile);
        d.D2H(meta.data(), t.d_meta, nfile * sizeof(lsm_sst_meta));
        d.Sync();
        for (const lsm_sst_meta &m : meta) tree_nidx = std::max(tree_nidx, m.nidx);
        tree_bytes = lsm_level_get_tree_bytes((uint32_t)nfile, tree_nidx);
        if (tree_bytes) {
            d_tree = d.Dev(29, tree_bytes);
            check(lsm_level_get_tree_build(d.ctx(), (const uint8_t *)t.d_img, (const uint64_t *)t.d_off,
                                           (const lsm_sst_meta *)t.d_meta, (uint32_t)nfile, nullptr,
                                           (const lsm_rec_desc *)t.d_idesc, tree_nidx, d_tree, tree_bytes,
                                           d.stream()),
                  "lsm_level_get_tree_build");
        }
    }
    const size_t n = nq * (size_t)limit;
    sstable::DeviceScan sc(d, ranges, n);
    void *d_src = d.Dev(36, n * 4);
    const size_t ws = lsm_db_scan_workspace_bytes((uint32_t)nlog, level_start, nq);
    void *d_ws = d.Dev(35, ws ? ws : 16);
    check(lsm_db_scan(d.ctx(), (const uint8_t *)r.d_wal, (const lsm_rec_desc *)r.d_desc, (const uint32_t *)r.d_idx,
                      r.d_fsc, (uint32_t)nlog, d_mem_index, ib, (const uint8_t *)t.d_img, t.d_index, level_start,
                      (const uint64_t *)t.d_off, (const uint64_t *)t.d_len, (const lsm_sst_meta *)t.d_meta, nullptr,
                      (const lsm_rec_desc *)t.d_idesc, (const int64_t *)t.d_ival, d_tree, tree_nidx, tree_bytes,
                      (const uint8_t *)sc.lo.d_bytes, (const uint64_t *)sc.lo.d_off, (const uint8_t *)sc.hi.d_bytes,
                      (const uint64_t *)sc.hi.d_off, (const uint8_t *)sc.d_flags, nq, limit, mode,
                      (uint32_t *)sc.d_count, (uint8_t *)sc.d_more, (lsm_rec_desc *)sc.d_key,
                      (lsm_rec_desc *)sc.d_value, (int32_t *)d_src, (int32_t *)sc.d_table, (int32_t *)sc.d_result,
                      d_ws, ws, d.stream()),
          "lsm_db_scan");
    // the pack (slots 37-44): the sizing call, its counts read back, then the arenas at exactly K and V
    uint64_t *d_row_start = (uint64_t *)d.Dev(37, (nq + 1) * 8);
    uint32_t *d_entry_slot = (uint32_t *)d.Dev(38, n * 4);
    uint64_t *d_koff = (uint64_t *)d.Dev(39, (n + 1) * 8), *d_voff = (uint64_t *)d.Dev(40, (n + 1) * 8);
    uint64_t *d_counts = (uint64_t *)d.Dev(41, 4 * 8);
    const size_t pws = lsm_pack_results_workspace_bytes(nq, limit);
    void *d_pws = d.Dev(42, pws);
    auto pack = [&](uint8_t *d_keys, uint64_t key_cap, uint8_t *d_vals, uint64_t val_cap) {
        check(lsm_pack_results(d.ctx(), (const uint8_t *)r.d_wal, (const uint8_t *)t.d_img, (const int32_t *)d_src,
                               (const lsm_rec_desc *)sc.d_key, (const lsm_rec_desc *)sc.d_value,
                               (const uint32_t *)sc.d_count, nq, limit, d_keys, key_cap, d_vals, val_cap,
                               d_row_start, d_entry_slot, d_koff, d_voff, d_counts, d_pws, pws, d.stream()),
              "lsm_pack_results");
    };
    pack(nullptr, 0, nullptr, 0);
    uint64_t counts[4] = {0, 0, 0, 0};
    d.D2H(counts, d_counts, sizeof counts);
    d.Sync();
    const uint64_t E = counts[0], K = counts[1], V = counts[2];
    uint8_t *d_keys = (uint8_t *)d.Dev(43, K ? K : 1), *d_vals = (uint8_t *)d.Dev(44, V ? V : 1);
    pack(d_keys, K, d_vals, V);
    // one D2H per arena and per side array; the views and the host's logs and images are not consulted
    std::vector<uint8_t> keys(K), vals(V), more(nq);
    std::vector<uint64_t> row_start(nq + 1), koff(E + 1), voff(E + 1);
    std::vector<uint32_t> entry_slot(E);
    std::vector<int32_t> src(n), table(n), result(n);
    if (K) d.D2H(keys.data(), d_keys, K);
    if (V) d.D2H(vals.data(), d_vals, V);
    d.D2H(row_start.data(), d_row_start, (nq + 1) * 8);
    if (E) d.D2H(entry_slot.data(), d_entry_slot, E * 4);
    d.D2H(koff.data(), d_koff, (E + 1) * 8);
    d.D2H(voff.data(), d_voff, (E + 1) * 8);
    d.D2H(counts, d_counts, sizeof counts);
    d.D2H(more.data(), sc.d_more, nq);
    d.D2H(src.data(), d_src, n * 4);
    d.D2H(table.data(), sc.d_table, n * 4);
    d.D2H(result.data(), sc.d_result, n * 4);
    d.Sync();
    if (counts[3]) throw std::runtime_error("ScanFromWALsPacked: the arenas sized by the sizing call overflowed");
    for (size_t q = 0; q < nq; q++) {
        out[q].more = more[q] != 0;
        out[q].entries.resize(row_start[q + 1] - row_start[q]);
        for (uint64_t e = row_start[q]; e < row_start[q + 1]; e++) {
            const size_t o = entry_slot[e];
            ScanEntry &x = out[q].entries[e - row_start[q]];
            x.key.assign((const char *)keys.data() + koff[e], koff[e + 1] - koff[e]);
            x.src = src[o];
            x.table = table[o];
            x.result = result[o];
            if (x.result == LSM_GET_FOUND) x.value.assign(vals.data() + voff[e], vals.data() + voff[e + 1]);
        }
    }
    return out;
}

WriteResult WriteBatch(const std::vector<WriteOp> &ops, uint64_t mem_size0, uint64_t mem_max,
                       const Bytes &current_wal) {
    for (const WriteOp &op : ops)
        if (op.op != LSM_OP_PUT && op.op != LSM_OP_DELETE) throw std::invalid_argument("WriteBatch: unknown op");
    if (mem_max == 0 || mem_max > (1ull << 30)) throw std::invalid_argument("WriteBatch: mem_max out of range");
    WriteResult out;
    out.mem_size = mem_size0;
    out.logs.resize(1);  // Mem, untouched
    const size_t n = ops.size();
    if (n == 0) return out;  // nothing to append: no device call
    Device &d = Device::ThisThread();
    // the current memtable's nodes (slots 0-9), when its log holds records
    sstable::OrderedWALs r{};
    uint64_t nnode = 0;
    if (!current_wal.empty()) {
        r = sstable::ReplayAndOrder(d, {current_wal}, LSM_MEMTABLE_ALL);
        uint64_t fs[2];
        int32_t st = 0;
        d.D2H(fs, r.d_fsc, sizeof fs);
        d.D2H(&st, r.d_st, 4);
        d.Sync();
        if (st != 0) throw std::runtime_error("WriteBatch: failed to read the current wal");
        nnode = fs[1] - fs[0];
    }
    // the batch, CSR (slots 20-24)
    std::vector<uint64_t> koff(n + 1, 0), voff(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        koff[i + 1] = koff[i] + ops[i].key.size();
        voff[i + 1] = voff[i] + ops[i].value.size();
    }
    const size_t kbytes = koff[n], vbytes = voff[n];
    uint8_t *hk = (uint8_t *)d.Host(20, pad16(kbytes));
    uint8_t *hv = (uint8_t *)d.Host(21, pad16(vbytes));
    uint8_t *hop = (uint8_t *)d.Host(22, pad16(n));
    std::memset(hk, 0, pad16(kbytes));
    std::memset(hv, 0, pad16(vbytes));
    std::memset(hop, 0, pad16(n));
    for (size_t i = 0; i < n; i++) {
        std::memcpy(hk + koff[i], ops[i].key.data(), ops[i].key.size());
        if (!ops[i].value.empty()) std::memcpy(hv + voff[i], ops[i].value.data(), ops[i].value.size());
        hop[i] = (uint8_t)ops[i].op;
    }
    void *d_keys = d.Dev(20, pad16(kbytes));
    void *d_vals = d.Dev(21, pad16(vbytes));
    void *d_op = d.Dev(22, pad16(n));
    void *d_koff = d.Dev(23, (n + 1) * 8);
    void *d_voff = d.Dev(24, (n + 1) * 8);
    d.H2D(d_keys, hk, pad16(kbytes));
    d.H2D(d_vals, hv, pad16(vbytes));
    d.H2D(d_op, hop, pad16(n));
    d.H2D(d_koff, koff.data(), (n + 1) * 8);
    d.H2D(d_voff, voff.data(), (n + 1) * 8);
    // outputs (slots 25-29): the logs; log_start, wal_off, rec_base and the counts in one buffer
    const uint32_t nlog_max = lsm_db_write_max_logs(n, kbytes, vbytes, mem_size0, mem_max);
    if (nlog_max > 65535) throw std::invalid_argument("WriteBatch: the batch needs more than 65535 logs");
    const uint32_t align = 16;
    const uint64_t out_bytes = lsm_db_write_out_bytes(n, kbytes, vbytes, nlog_max, align);
    const size_t m = (size_t)nlog_max + 1;
    void *d_wal = d.Dev(25, pad16(out_bytes));
    uint64_t *d_meta = (uint64_t *)d.Dev(26, (3 * m + 6) * 8);
    void *d_len = d.Dev(27, (size_t)nlog_max * 4);
    const size_t ws = lsm_db_write_workspace_bytes(n, nlog_max, mem_max);
    void *d_ws = d.Dev(28, ws);
    check(lsm_db_write(d.ctx(), (const uint8_t *)d_keys, (const uint64_t *)d_koff, (const uint8_t *)d_vals,
                       (const uint64_t *)d_voff, (const uint8_t *)d_op, n, mem_size0, mem_max,
                       nnode ? (const uint8_t *)r.d_wal : nullptr, nnode ? (const lsm_rec_desc *)r.d_desc : nullptr,
                       nnode ? (const uint32_t *)r.d_idx : nullptr, nnode, nlog_max, align, (uint8_t *)d_wal,
                       d_meta, d_meta + m, (uint32_t *)d_len, nullptr, d_meta + 2 * m, nullptr, d_meta + 3 * m,
                       d_ws, ws, d.stream()),
          "lsm_db_write");
    std::vector<uint64_t> meta(3 * m + 6);
    std::vector<uint32_t> len(nlog_max);
    d.D2H(meta.data(), d_meta, meta.size() * 8);
    d.D2H(len.data(), d_len, len.size() * 4);
    d.Sync();
    const uint64_t *counts = meta.data() + 3 * m;
    if (counts[3]) throw std::runtime_error("WriteBatch: lsm_db_write overflowed its own log bound");
    const size_t nlog = counts[0];
    out.logs.resize(nlog);
    out.mem_size = counts[5];
    for (size_t s = 0; s < nlog; s++) {
        out.logs[s].resize(len[s]);
        if (len[s]) d.D2H(out.logs[s].data(), (const uint8_t *)d_wal + meta[m + s], len[s]);
    }
    d.Sync();
    return out;
}

}  // namespace database
}  // namespace golsm
