// pack_mirror_test — golsm::database::ScanFromWALsPacked (the scan's entries
// out of lsm_pack_results's two arenas) against golsm::database::ScanFromWALs
// (the entries sliced from the host's logs and images), entry for entry, on
// db_scan_mirror_test's databases: four logs (one empty, one that fails to
// recover) over two level-0 tables and levels 1 and 3, the memtables alone,
// the tree alone; tombstones, empty values, the empty key.
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <stdexcept>
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

using Table = std::map<std::string, std::string>;

static void put(Bytes &log, const std::string &k, const std::string &v) {
    auto u32 = [&](uint32_t x) {
        for (int i = 0; i < 4; i++) log.push_back((uint8_t)(x >> (8 * i)));
    };
    u32((uint32_t)k.size());
    log.insert(log.end(), k.begin(), k.end());
    u32((uint32_t)v.size());
    log.insert(log.end(), v.begin(), v.end());
}

static std::vector<Bytes> Images(const std::vector<std::vector<Table>> &levels, uint32_t *level_start) {
    std::vector<Bytes> images;
    level_start[0] = 0;
    for (size_t L = 0; L < LSM_SEARCH_LEVELS; L++) {
        if (L < levels.size()) {
            for (const Table &t : levels[L]) {
                std::vector<kv::KeyValuePair> pairs;
                for (const auto &kv : t) pairs.push_back({kv.first, kv::Value(kv.second.begin(), kv.second.end())});
                const auto img = sstable::BuildImages(pairs, 0, 4096, 4);
                images.push_back(img.at(0));
            }
        }
        level_start[L + 1] = (uint32_t)images.size();
    }
    return images;
}

static void TestPackedNothing() {  // host only: no device call; bad arguments throw
    const uint32_t empty[LSM_SEARCH_LEVELS + 1] = {};
    CHECK(database::ScanFromWALsPacked({}, {}, empty, {}, 4).empty());
    const auto r = database::ScanFromWALsPacked({}, {}, empty, {{"a", "b", false}, {"", "", true}}, 4, LSM_SCAN_RAW);
    CHECK(r.size() == 2 && r[0].entries.empty() && !r[0].more && r[1].entries.empty() && !r[1].more);
    Bytes log;
    put(log, "a", "1");
    CHECK(database::ScanFromWALsPacked({log}, {}, empty, {}, 4).empty());  // no ranges
    auto throws = [&](const uint32_t *ls, uint32_t limit, int mode) {
        try {
            database::ScanFromWALsPacked({}, {}, ls, {{"a", "b", false}}, limit, mode);
        } catch (const std::invalid_argument &) {
            return true;
        }
        return false;
    };
    CHECK(throws(empty, 0, LSM_SCAN_LIVE));
    CHECK(throws(empty, 4, 2));
    const uint32_t one[LSM_SEARCH_LEVELS + 1] = {0, 1, 1, 1, 1, 1, 1, 1};
    CHECK(throws(one, 4, LSM_SCAN_LIVE));
    CHECK(throws(nullptr, 4, LSM_SCAN_LIVE));
    CHECK(!throws(empty, 4, LSM_SCAN_LIVE));
}

static void Same(const std::vector<database::ScanResult> &want, const std::vector<database::ScanResult> &got,
                 int *entries, int *from_mem, int *tombs, int *empties) {
    CHECK(got.size() == want.size());
    for (size_t q = 0; q < want.size() && q < got.size(); q++) {
        CHECK(got[q].more == want[q].more);
        CHECK(got[q].entries.size() == want[q].entries.size());
        for (size_t j = 0; j < want[q].entries.size() && j < got[q].entries.size(); j++) {
            const auto &a = want[q].entries[j], &b = got[q].entries[j];
            CHECK(b.key == a.key);
            CHECK(b.value == a.value);
            CHECK(b.src == a.src);
            CHECK(b.table == a.table);
            CHECK(b.result == a.result);
            *entries += 1;
            *from_mem += a.src == LSM_SRC_MEMTABLE;
            *tombs += std::string(a.value.begin(), a.value.end()) == kv::kDeletedValue;
            *empties += a.value.empty();
        }
    }
}

static void TestPackedVsSliced() {
    // db_scan_mirror_test's TestScanVsMaps generator, seed and ranges
    std::mt19937_64 rng(47);
    auto key = [](int i) {
        char b[16];
        std::snprintf(b, sizeof b, "key%04d", i);
        return std::string(b);
    };
    int entries = 0, from_mem = 0, tombs = 0, empties = 0;
    for (int round = 0; round < 4; round++) {
        // round 2: the memtables alone; round 3: the tree alone
        std::vector<std::vector<Table>> levels(round == 2 ? 0 : 4);
        if (round != 2) {
            for (int t = 0; t < 2; t++) {
                Table tab;
                for (int j = 0; j < 60; j++) {
                    const int i = (int)(rng() % 400);
                    tab[key(i)] = rng() % 5 == 0 ? kv::kDeletedValue : "0." + std::to_string(t) + "." + std::to_string(i);
                }
                levels[0].push_back(tab);
            }
            for (int L : {1, 3}) {
                const int c = L == 1 ? 3 : 2;
                for (int t = 0; t < c; t++) {
                    Table tab;
                    const int a = t * 400 / c, b = (t + 1) * 400 / c;
                    for (int i = a + (int)(rng() % 3); i < b; i += 1 + (int)(rng() % 4))
                        tab[key(i)] = rng() % 7 == 0 ? kv::kDeletedValue : std::to_string(L) + "." + std::to_string(i);
                    levels[L].push_back(tab);
                }
            }
        }
        const size_t nlog = round == 3 ? 0 : 4;
        std::vector<Bytes> wals(nlog);
        for (size_t w = 0; w < nlog; w++) {
            if (w == 1) continue;  // an empty memtable
            for (int i = 0; i < 80; i++) {
                const std::string k = key((int)(rng() % 400));
                const std::string v = rng() % 6 == 0 ? kv::kDeletedValue : rng() % 15 == 0 ? "" : "m" + std::to_string(w) + "." + std::to_string(i);
                put(wals[w], k, v);
            }
        }
        if (nlog) {
            put(wals[2], "cut", "short");  // wal.Recover fails on log 2: it is a source without a head
            wals[2].pop_back();
            put(wals[3], "", "empty key");
        }
        uint32_t level_start[LSM_SEARCH_LEVELS + 1];
        const auto images = Images(levels, level_start);
        std::vector<sstable::ScanRange> ranges = {{"", "", true}, {"key0100", "key0100", false},
                                                  {"key0300", "key0200", false}, {"zzz", "", true},
                                                  {"", "key0010", false}};
        for (int q = 0; q < 40; q++) {
            const int a = (int)(rng() % 400), b = a + (int)(rng() % 60);
            ranges.push_back({key(a) + (rng() % 4 ? "" : "x"), key(b), rng() % 3 == 0});
        }
        for (int mode : {LSM_SCAN_RAW, LSM_SCAN_LIVE})
            for (uint32_t limit : {1u, 7u, 1000u})
                Same(database::ScanFromWALs(wals, images, level_start, ranges, limit, mode),
                     database::ScanFromWALsPacked(wals, images, level_start, ranges, limit, mode), &entries,
                     &from_mem, &tombs, &empties);
    }
    // what makes the comparison meaningful
    CHECK(entries > 5000 && from_mem > 1000 && from_mem < entries && tombs > 100 && empties > 10);
}

int main(int argc, char **argv) {
    struct {
        const char *name;
        void (*fn)();
    } tests[] = {{"TestPackedNothing", TestPackedNothing}, {"TestPackedVsSliced", TestPackedVsSliced}};
    for (auto &t : tests) {
        if (argc > 1 && std::strcmp(argv[1], t.name) != 0) continue;
        g_case = t.name;
        const int before = g_fail;
        try {
            t.fn();
        } catch (const std::exception &e) {
            g_fail++;
            std::printf("FAIL %s: exception %s\n", t.name, e.what());
        }
        if (g_fail == before) std::printf("PASS %s\n", t.name);
    }
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
