// db_scan_mirror_test — golsm::database::ScanFromWALs (range scans over
// lsm_db_scan) against the database restated with std::maps: a key is answered
// by the newest log that holds it (its last record there), else by the first
// table, in Manager.Search's order, that does; a tombstone answers too and
// hides every older entry; a range delivers its keys in order up to the limit,
// LIVE leaving out the tombstones.
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

struct Answer {
    int src, table;
    std::string value;
};

static void put(Bytes &log, const std::string &k, const std::string &v) {
    auto u32 = [&](uint32_t x) {
        for (int i = 0; i < 4; i++) log.push_back((uint8_t)(x >> (8 * i)));
    };
    u32((uint32_t)k.size());
    log.insert(log.end(), k.begin(), k.end());
    u32((uint32_t)v.size());
    log.insert(log.end(), v.begin(), v.end());
}

// mems[w] = log w's memtable (oldest first); levels[L] = the level's tables, in the tree's order
static std::map<std::string, Answer> Answers(const std::vector<Table> &mems,
                                             const std::vector<std::vector<Table>> &levels) {
    std::map<std::string, Answer> want;
    for (size_t w = mems.size(); w-- > 0;)  // newest first
        for (const auto &kv : mems[w]) want.emplace(kv.first, Answer{LSM_SRC_MEMTABLE, (int)w, kv.second});
    int first = 0;
    for (size_t L = 0; L < levels.size(); L++) {
        const int n = (int)levels[L].size();
        for (int i = 0; i < n; i++) {
            // level 0: newest first; deeper: a boundary key is the later table's
            const int t = L == 0 ? i : n - 1 - i;
            for (const auto &kv : levels[L][t]) want.emplace(kv.first, Answer{LSM_SRC_SSTABLE, first + t, kv.second});
        }
        first += n;
    }
    return want;
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

static void Compare(const std::map<std::string, Answer> &want, const std::vector<sstable::ScanRange> &ranges,
                    const std::vector<database::ScanResult> &got, uint32_t limit, int mode, int *from_mem) {
    CHECK(got.size() == ranges.size());
    for (size_t q = 0; q < ranges.size() && q < got.size(); q++) {
        std::vector<std::pair<std::string, Answer>> exp;
        bool more = false;
        for (auto it = want.lower_bound(ranges[q].lo); it != want.end(); ++it) {
            if (!ranges[q].no_upper && !(it->first < ranges[q].hi)) break;
            if (mode == LSM_SCAN_LIVE && it->second.value == kv::kDeletedValue) continue;
            if (exp.size() == limit) {
                more = true;
                break;
            }
            exp.push_back(*it);
        }
        CHECK(got[q].more == more);
        CHECK(got[q].entries.size() == exp.size());
        for (size_t j = 0; j < exp.size() && j < got[q].entries.size(); j++) {
            const auto &e = got[q].entries[j];
            CHECK(e.key == exp[j].first);
            CHECK(e.src == exp[j].second.src);
            CHECK(e.table == exp[j].second.table);
            CHECK(e.result == LSM_GET_FOUND);
            CHECK(std::string(e.value.begin(), e.value.end()) == exp[j].second.value);
            *from_mem += e.src == LSM_SRC_MEMTABLE;
        }
    }
}

static void TestScanNothing() {  // host only: no device call; bad arguments throw
    const uint32_t empty[LSM_SEARCH_LEVELS + 1] = {};
    CHECK(database::ScanFromWALs({}, {}, empty, {}, 4).empty());
    const auto r = database::ScanFromWALs({}, {}, empty, {{"a", "b", false}, {"", "", true}}, 4, LSM_SCAN_RAW);
    CHECK(r.size() == 2 && r[0].entries.empty() && !r[0].more && r[1].entries.empty() && !r[1].more);
    Bytes log;
    put(log, "a", "1");
    CHECK(database::ScanFromWALs({log}, {}, empty, {}, 4).empty());  // no ranges
    auto throws = [&](const uint32_t *ls, uint32_t limit, int mode) {
        try {
            database::ScanFromWALs({}, {}, ls, {{"a", "b", false}}, limit, mode);
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

static void TestScanVsMaps() {
    std::mt19937_64 rng(47);
    auto key = [](int i) {
        char b[16];
        std::snprintf(b, sizeof b, "key%04d", i);
        return std::string(b);
    };
    int from_mem = 0;
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
        std::vector<Table> mems(nlog);
        std::vector<Bytes> wals(nlog);
        for (size_t w = 0; w < nlog; w++) {
            if (w == 1) continue;  // an empty memtable
            for (int i = 0; i < 80; i++) {
                const std::string k = key((int)(rng() % 400));
                const std::string v = rng() % 6 == 0 ? kv::kDeletedValue : rng() % 15 == 0 ? "" : "m" + std::to_string(w) + "." + std::to_string(i);
                put(wals[w], k, v);
                mems[w][k] = v;
            }
        }
        if (nlog) {
            put(wals[2], "cut", "short");  // wal.Recover fails on log 2: it is a source without a head
            wals[2].pop_back();
            mems[2].clear();
            put(wals[3], "", "empty key");
            mems[3][""] = "empty key";
        }
        uint32_t level_start[LSM_SEARCH_LEVELS + 1];
        const auto images = Images(levels, level_start);
        const auto want = Answers(mems, levels);
        std::vector<sstable::ScanRange> ranges = {{"", "", true}, {"key0100", "key0100", false},
                                                  {"key0300", "key0200", false}, {"zzz", "", true},
                                                  {"", "key0010", false}};
        for (int q = 0; q < 40; q++) {
            const int a = (int)(rng() % 400), b = a + (int)(rng() % 60);
            ranges.push_back({key(a) + (rng() % 4 ? "" : "x"), key(b), rng() % 3 == 0});
        }
        for (int mode : {LSM_SCAN_RAW, LSM_SCAN_LIVE})
            for (uint32_t limit : {1u, 7u, 1000u})
                Compare(want, ranges, database::ScanFromWALs(wals, images, level_start, ranges, limit, mode), limit,
                        mode, &from_mem);
    }
    CHECK(from_mem > 1000);
}

int main(int argc, char **argv) {
    struct {
        const char *name;
        void (*fn)();
    } tests[] = {{"TestScanNothing", TestScanNothing}, {"TestScanVsMaps", TestScanVsMaps}};
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
