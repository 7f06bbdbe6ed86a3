// memtable_search_mirror_test — golsm::memtables::SearchWALs (Manager.Search
// over the C ABI) against std::maps playing the skiplists: a later Add of a
// key replaces the pair (skiplist.go:83-118), the newest memtable holding the
// key answers, a tombstone there is (nil, true) and ends the search.  And
// golsm::database::GetFromWALs (database.Get over lsm_db_get) against those
// maps plus a lookup in the tables' own pairs, in both modes.
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

static void put(Bytes &log, const std::string &k, const std::string &v) {
    auto u32 = [&](uint32_t x) {
        for (int i = 0; i < 4; i++) log.push_back((uint8_t)(x >> (8 * i)));
    };
    u32((uint32_t)k.size());
    log.insert(log.end(), k.begin(), k.end());
    u32((uint32_t)v.size());
    log.insert(log.end(), v.begin(), v.end());
}

static void TestSearchNothing() {  // host only: no logs, or no keys -- no device call
    CHECK(memtables::SearchWALs({}, {}).empty());
    const auto r = memtables::SearchWALs({}, {"a", ""});
    CHECK(r.size() == 2 && r[0].result == LSM_MEM_MISS && r[1].log == -1 && r[0].value.empty());
    Bytes log;
    put(log, "a", "1");
    CHECK(memtables::SearchWALs({log}, {}).empty());
}

static void TestSearchVsMaps() {
    std::mt19937_64 rng(12);
    const size_t nlog = 5;
    std::vector<std::map<std::string, std::string>> lists(nlog);
    std::vector<Bytes> wals(nlog);
    for (size_t w = 0; w < nlog; w++) {
        if (w == 1) continue;  // an empty memtable
        const int n = w == 0 ? 3000 : 400;  // more than one sort tile in the oldest
        for (int i = 0; i < n; i++) {
            const std::string k = "key" + std::to_string(rng() % 1500);
            const std::string v = rng() % 8 == 0 ? kv::kDeletedValue : rng() % 20 == 0 ? "" : "v" + std::to_string(i);
            put(wals[w], k, v);
            lists[w][k] = v;
        }
    }
    put(wals[3], "cut", "short");  // wal.Recover fails on log 3: it answers nothing
    wals[3].pop_back();
    lists[3].clear();
    std::vector<kv::Key> keys = {"", "key", "zzz", "cut"};
    for (int i = 0; i < 1600; i++) keys.push_back("key" + std::to_string(i));
    const auto got = memtables::SearchWALs(wals, keys);
    CHECK(got.size() == keys.size());
    int seen[3] = {0, 0, 0}, hidden = 0;
    for (size_t i = 0; i < keys.size(); i++) {
        int want = LSM_MEM_MISS, log = -1;
        std::string value;
        for (size_t w = nlog; w-- > 0 && log < 0;) {
            auto it = lists[w].find(keys[i]);
            if (it == lists[w].end()) continue;
            log = (int)w;
            want = it->second == kv::kDeletedValue ? LSM_MEM_DELETED : LSM_MEM_VALUE;
            if (want == LSM_MEM_VALUE) value = it->second;
            for (size_t o = 0; o < w; o++)
                hidden += want == LSM_MEM_DELETED && lists[o].count(keys[i]) && lists[o][keys[i]] != kv::kDeletedValue;
        }
        seen[want]++;
        CHECK(got[i].result == want && got[i].log == log);
        CHECK(std::string(got[i].value.begin(), got[i].value.end()) == value);
    }
    CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0 && hidden > 0);
}

static void TestGetNothing() {  // host only: no keys, or neither logs nor tables -- no device call
    const uint32_t none[LSM_SEARCH_LEVELS + 1] = {0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(database::GetFromWALs({}, {}, none, {}).empty());
    for (int mode : {LSM_DBGET_EXACT, LSM_DBGET_TOMBSTONE_HIDES}) {
        const auto r = database::GetFromWALs({}, {}, none, {"a", ""}, mode);
        CHECK(r.size() == 2);
        for (auto &g : r)
            CHECK(g.src == LSM_SRC_NONE && g.mem_result == LSM_MEM_MISS && g.log == -1 && g.level == -1 &&
                  g.table == -1 && g.result == LSM_GET_ABSENT && g.value.empty());
    }
    Bytes log;
    put(log, "a", "1");
    CHECK(database::GetFromWALs({log}, {}, none, {}).empty());
    bool threw = false;
    try {
        database::GetFromWALs({}, {}, none, {"a"}, 2);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
}

typedef std::map<std::string, std::string> List;

// The tree: level 0 = tables 0 (newest) and 1, overlapping; level 1 = tables 2
// and 3, disjoint and in key order.  Search answers from the first of them
// that holds the key (a filter's false positive only costs a Seek that misses).
static void TestGetVsMaps() {
    std::mt19937_64 rng(13);
    auto key = [](uint64_t i) { return "key" + std::to_string(1000 + i % 1000); };  // fixed width: key order = id order
    std::vector<List> tabs(4);
    for (int i = 0; i < 200; i++) tabs[0][key(rng())] = "t0." + std::to_string(i);
    for (int i = 0; i < 200; i++) tabs[1][key(rng())] = i % 9 == 0 ? kv::kDeletedValue : "t1." + std::to_string(i);
    for (int i = 0; i < 300; i++) {
        const uint64_t id = rng() % 1000;
        tabs[id < 500 ? 2 : 3][key(id)] = "deep." + std::to_string(i);
    }
    tabs[3]["key1999"] = "only in a table";
    tabs[2]["key1000"] = "under a tombstone";
    tabs[0].erase("key1000");
    tabs[1].erase("key1000");
    tabs[0]["key1001"] = "in both: the table's";
    std::vector<Bytes> images;
    for (auto &t : tabs) {
        std::vector<kv::KeyValuePair> pairs;
        for (auto &p : t) pairs.push_back({p.first, kv::Value(p.second.begin(), p.second.end())});
        const std::vector<Bytes> im = sstable::BuildImages(pairs, 0, 4096, 4);
        CHECK(im.size() == 1);
        images.push_back(im[0]);
    }
    const uint32_t level_start[LSM_SEARCH_LEVELS + 1] = {0, 2, 4, 4, 4, 4, 4, 4};
    const int level_of[4] = {0, 0, 1, 1};
    // three memtables, oldest first
    std::vector<List> lists(3);
    std::vector<Bytes> wals(3);
    auto write = [&](size_t w, const std::string &k, const std::string &v) {
        put(wals[w], k, v);
        lists[w][k] = v;
    };
    for (size_t w = 0; w < 3; w++)
        for (int i = 0; i < 250; i++)
            write(w, key(rng()), rng() % 6 == 0 ? kv::kDeletedValue : rng() % 15 == 0 ? "" : "m" + std::to_string(w) + "." + std::to_string(i));
    for (size_t w = 0; w < 3; w++) {  // keep the named cases clear of the random writes
        for (const char *k : {"key1000", "key1001", "key1999"}) {
            if (lists[w].erase(k)) {  // rebuild the log without it
                wals[w].clear();
                for (auto &p : lists[w]) put(wals[w], p.first, p.second);
            }
        }
    }
    write(0, "key1000", "older memtable value");
    write(2, "key1000", kv::kDeletedValue);  // a tombstone over a table's value (and an older memtable's)
    write(1, "key1001", "in both: the memtable's");
    std::vector<kv::Key> keys = {"", "key", "zzz", "key1000", "key1001", "key1999"};
    for (int i = 0; i < 1000; i++) keys.push_back(key(i));
    for (size_t nlog : {size_t(3), size_t(0)}) {
        const std::vector<Bytes> logs(wals.begin(), wals.begin() + nlog);
        for (int mode : {LSM_DBGET_EXACT, LSM_DBGET_TOMBSTONE_HIDES}) {
            const auto got = database::GetFromWALs(logs, images, level_start, keys, mode);
            CHECK(got.size() == keys.size());
            int srcs[3] = {0, 0, 0}, uncovered = 0, hid = 0;
            for (size_t i = 0; i < keys.size(); i++) {
                int mres = LSM_MEM_MISS, log = -1;
                std::string mval;
                for (size_t w = nlog; w-- > 0 && log < 0;) {
                    auto it = lists[w].find(keys[i]);
                    if (it == lists[w].end()) continue;
                    log = (int)w;
                    mres = it->second == kv::kDeletedValue ? LSM_MEM_DELETED : LSM_MEM_VALUE;
                    mval = it->second;
                }
                int table = -1;
                std::string tval;
                for (int t = 0; t < 4 && table < 0; t++) {
                    auto it = tabs[t].find(keys[i]);
                    if (it != tabs[t].end()) {
                        table = t;
                        tval = it->second;
                    }
                }
                const bool on = mres == LSM_MEM_MISS || (mres == LSM_MEM_DELETED && mode == LSM_DBGET_EXACT);
                const auto &g = got[i];
                CHECK(g.mem_result == mres && g.log == log);
                const std::string value(g.value.begin(), g.value.end());
                if (!on) {  // the memtables' answer: a value, or nil for the hiding tombstone
                    CHECK(g.src == LSM_SRC_MEMTABLE && g.table == -1 && g.level == -1 && g.result == LSM_GET_ABSENT);
                    CHECK(value == (mres == LSM_MEM_VALUE ? mval : std::string()));
                    hid += mres == LSM_MEM_DELETED && table >= 0;
                } else if (table >= 0) {  // Search's value, a table's tombstone bytes included
                    CHECK(g.src == LSM_SRC_SSTABLE && g.table == table && g.level == level_of[table] &&
                          g.result == LSM_GET_FOUND);
                    CHECK(value == tval);
                    uncovered += mres == LSM_MEM_DELETED;
                } else {
                    CHECK(g.src == LSM_SRC_NONE && g.table == -1 && g.level == -1 && g.result == LSM_GET_ABSENT &&
                          value.empty());
                }
                srcs[g.src + 1]++;
            }
            const auto &tomb = got[3], &both = got[4], &deep = got[5];
            if (nlog == 0) {  // lsm_search's answers
                CHECK(srcs[1] == 0 && srcs[0] > 0 && srcs[2] > 0);
                CHECK(tomb.src == LSM_SRC_SSTABLE && tomb.table == 2);
                CHECK(std::string(both.value.begin(), both.value.end()) == "in both: the table's");
            } else {
                CHECK(srcs[0] > 0 && srcs[1] > 0 && srcs[2] > 0);
                CHECK(tomb.mem_result == LSM_MEM_DELETED && tomb.log == 2);
                if (mode == LSM_DBGET_EXACT) {
                    CHECK(tomb.src == LSM_SRC_SSTABLE && tomb.level == 1 && uncovered > 1 && hid == 0);
                    CHECK(std::string(tomb.value.begin(), tomb.value.end()) == "under a tombstone");
                } else {
                    CHECK(tomb.src == LSM_SRC_MEMTABLE && tomb.value.empty() && hid > 1 && uncovered == 0);
                }
                CHECK(both.src == LSM_SRC_MEMTABLE && both.log == 1);
                CHECK(std::string(both.value.begin(), both.value.end()) == "in both: the memtable's");
            }
            CHECK(deep.src == LSM_SRC_SSTABLE && deep.table == 3 && deep.level == 1);
        }
    }
    // an empty tree: the memtables' answers
    const uint32_t none[LSM_SEARCH_LEVELS + 1] = {0, 0, 0, 0, 0, 0, 0, 0};
    const auto mem_only = database::GetFromWALs(wals, {}, none, keys, LSM_DBGET_EXACT);
    const auto searched = memtables::SearchWALs(wals, keys);
    for (size_t i = 0; i < keys.size(); i++) {
        CHECK(mem_only[i].mem_result == searched[i].result && mem_only[i].log == searched[i].log);
        CHECK(mem_only[i].value == searched[i].value && mem_only[i].table == -1);
        CHECK(mem_only[i].src == (searched[i].result == LSM_MEM_VALUE ? LSM_SRC_MEMTABLE : LSM_SRC_NONE));
    }
}

int main(int argc, char **argv) {
    struct Case {
        const char *name;
        void (*fn)();
    } cases[] = {{"TestSearchNothing", TestSearchNothing}, {"TestSearchVsMaps", TestSearchVsMaps},
                 {"TestGetNothing", TestGetNothing}, {"TestGetVsMaps", TestGetVsMaps}};
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
