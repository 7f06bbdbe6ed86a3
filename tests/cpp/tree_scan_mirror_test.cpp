// tree_scan_mirror_test — golsm::sstable::ScanImages (range scans over
// lsm_tree_scan) against the tree restated with std::maps: a key is answered
// by the first table, in Manager.Search's order, that holds it (level 0 newest
// first, then the levels; within a level the later table on a boundary key),
// and a range delivers its keys in order up to the limit, LIVE leaving out the
// tombstones.
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
    int table;
    std::string value;
};

// levels[L] = the level's tables, in the tree's order
static std::map<std::string, Answer> Answers(const std::vector<std::vector<Table>> &levels) {
    std::map<std::string, Answer> want;
    int first = 0;
    for (size_t L = 0; L < levels.size(); L++) {
        const int n = (int)levels[L].size();
        for (int i = 0; i < n; i++) {
            // level 0: newest first; deeper: a boundary key is the later table's
            const int t = L == 0 ? i : n - 1 - i;
            for (const auto &kv : levels[L][t]) want.emplace(kv.first, Answer{first + t, kv.second});
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
                    const std::vector<sstable::ScanResult> &got, uint32_t limit, int mode) {
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
            CHECK(e.table == exp[j].second.table);
            CHECK(e.result == LSM_GET_FOUND);
            CHECK(std::string(e.value.begin(), e.value.end()) == exp[j].second.value);
        }
    }
}

static void TestScanNothing() {  // host only: no device call; bad arguments throw
    const uint32_t empty[LSM_SEARCH_LEVELS + 1] = {};
    CHECK(sstable::ScanImages({}, empty, {}, 4).empty());
    const auto r = sstable::ScanImages({}, empty, {{"a", "b", false}, {"", "", true}}, 4, LSM_SCAN_RAW);
    CHECK(r.size() == 2 && r[0].entries.empty() && !r[0].more && r[1].entries.empty() && !r[1].more);
    auto throws = [&](const uint32_t *ls, uint32_t limit, int mode) {
        try {
            sstable::ScanImages({}, ls, {{"a", "b", false}}, limit, mode);
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
    std::mt19937_64 rng(31);
    auto key = [](int i) {
        char b[16];
        std::snprintf(b, sizeof b, "key%04d", i);
        return std::string(b);
    };
    for (int round = 0; round < 4; round++) {
        std::vector<std::vector<Table>> levels(4);
        // level 0: overlapping tables; levels 1 and 3: disjoint slices (level 2 stays empty)
        const int n0 = round == 3 ? 5 : 2;
        for (int t = 0; t < n0; t++) {
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
                if (t > 0 && round % 2) tab[levels[L][t - 1].rbegin()->first] = "boundary";  // shared with the table before
                levels[L].push_back(tab);
            }
        }
        if (round == 0) levels[0][0][""] = "empty key";
        uint32_t level_start[LSM_SEARCH_LEVELS + 1];
        const auto images = Images(levels, level_start);
        const auto want = Answers(levels);
        std::vector<sstable::ScanRange> ranges = {{"", "", true}, {"key0100", "key0100", false},
                                                  {"key0300", "key0200", false}, {"zzz", "", true},
                                                  {"", "key0010", false}};
        for (int q = 0; q < 40; q++) {
            const int a = (int)(rng() % 400), b = a + (int)(rng() % 60);
            ranges.push_back({key(a) + (rng() % 4 ? "" : "x"), key(b), rng() % 3 == 0});
        }
        for (int mode : {LSM_SCAN_RAW, LSM_SCAN_LIVE})
            for (uint32_t limit : {1u, 7u, 1000u})
                Compare(want, ranges, sstable::ScanImages(images, level_start, ranges, limit, mode), limit, mode);
    }
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
