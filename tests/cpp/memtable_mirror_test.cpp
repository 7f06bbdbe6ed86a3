// memtable_mirror_test — golsm::sstable::BuildSSTablesFromWALs (the memtable
// flush over the C ABI) against the mirror's own Builder path: a std::map
// plays the skiplist (a later Add replaces the pair, skiplist.go:83-118), the
// loop of IMemTable.RangeScan (imemtable.go:46-53) walks it, and BuildImages
// with threshold 0 is BuildSSTableFromIMemTable + EncodeTo.
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "golsm.h"

using namespace golsm;

static int g_fail = 0, g_checks = 0;
static const char *g_case = "";

#define CHECK(c)                                                              \
    do {                                                                      \
        g_checks++;                                                           \
        if (!(c)) {                                                           \
            g_fail++;                                                         \
            std::printf("FAIL %s: %s (line %d)\n", g_case, #c, __LINE__);    \
        }                                                                     \
    } while (0)

static void put(Bytes &log, const std::string &k, const std::string &v) {
    auto u32 = [&](uint32_t x) {
        for (int i = 0; i < 4; i++) log.push_back((uint8_t)(x >> (8 * i)));
    };
    u32((uint32_t)k.size());
    log.insert(log.end(), k.begin(), k.end());
    u32((uint32_t)v.size());
    log.insert(log.end(), v.begin(), v.end());
}

// The pairs RangeScan (or a walk of every node) delivers for the given writes.
static std::vector<kv::KeyValuePair> memtable(const std::vector<std::pair<std::string, std::string>> &writes,
                                              int scan) {
    std::map<std::string, std::string> list;
    for (auto &w : writes) list[w.first] = w.second;
    std::vector<kv::KeyValuePair> out;
    auto it = list.begin();
    if (scan == LSM_MEMTABLE_RANGESCAN)
        while (it != list.end() && it->second == kv::kDeletedValue) ++it;  // SeekToFirst
    for (; it != list.end(); ++it) {
        if (scan == LSM_MEMTABLE_RANGESCAN && it->second == kv::kDeletedValue) break;  // Valid
        out.push_back({it->first, kv::Value(it->second.begin(), it->second.end())});
    }
    return out;
}

static void TestFlushNoLogs() {  // host only: nothing to flush, no device call
    std::vector<int32_t> st(3, 7);
    CHECK(sstable::BuildSSTablesFromWALs({}, LSM_MEMTABLE_ALL, &st).empty());
    CHECK(st.empty());
}

static void TestFlushVsBuilder() {
    std::mt19937_64 rng(11);
    std::vector<std::vector<std::pair<std::string, std::string>>> writes(5);
    for (int i = 0; i < 3000; i++) {  // overwrites, deletes, more than one sort tile
        const std::string k = "key" + std::to_string(rng() % 1500);
        writes[0].push_back({k, rng() % 50 == 0 ? kv::kDeletedValue : "v" + std::to_string(i)});
    }
    writes[1] = {};  // an empty memtable: no image
    writes[2] = {{"b", "1"}, {"a", "2"}, {"c", kv::kDeletedValue}, {"d", "4"}, {"a", "3"}, {"", "e"}};
    writes[3] = {{"x", "1"}, {"y", "2"}};  // cut below: wal.Recover fails
    writes[4] = {{"t", kv::kDeletedValue}};
    std::vector<Bytes> wals(5);
    for (size_t w = 0; w < wals.size(); w++)
        for (auto &p : writes[w]) put(wals[w], p.first, p.second);
    wals[3].pop_back();
    for (int scan : {LSM_MEMTABLE_ALL, LSM_MEMTABLE_RANGESCAN}) {
        std::vector<int32_t> st;
        const std::vector<Bytes> got = sstable::BuildSSTablesFromWALs(wals, scan, &st, 4096, 4);
        CHECK(got.size() == 5 && st.size() == 5);
        for (size_t w = 0; w < wals.size(); w++) {
            CHECK((st[w] != 0) == (w == 3));
            const auto pairs = w == 3 ? std::vector<kv::KeyValuePair>() : memtable(writes[w], scan);
            if (pairs.empty()) {
                CHECK(got[w].empty());
                continue;
            }
            const std::vector<Bytes> want = sstable::BuildImages(pairs, 0, 4096, 4);
            CHECK(want.size() == 1 && got[w] == want[0]);
        }
        // RangeScan stops at "c": "d" never reaches the table
        sstable::SSTable t;
        CHECK(!t.DecodeImage(got[2]) && !t.DecodeDataBlock(got[2]));
        CHECK(t.IndexBlock.Len() == (scan == LSM_MEMTABLE_ALL ? 5 : 3));
        CHECK(got[4].empty() == (scan == LSM_MEMTABLE_RANGESCAN));
    }
}

int main(int argc, char **argv) {
    struct Case {
        const char *name;
        void (*fn)();
    } cases[] = {{"TestFlushNoLogs", TestFlushNoLogs}, {"TestFlushVsBuilder", TestFlushVsBuilder}};
    for (auto &c : cases) {
        if (argc > 1 && std::strcmp(argv[1], c.name) != 0) continue;
        g_case = c.name;
        const int before = g_fail;
        try {
            c.fn();
        } catch (const std::exception &e) {
            g_fail++;
            std::printf("FAIL %s: exception: %s\n", c.name, e.what());
        }
        if (g_fail == before) std::printf("PASS %s\n", c.name);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
