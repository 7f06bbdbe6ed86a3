// db_write_mirror_test — golsm::database::WriteBatch (database.Put / Delete
// over lsm_db_write) against memtable.Manager restated with std::maps playing
// the skiplists: CanInsert, promoteLocked, MemTable.Delete's (key, nil) record
// when the current memtable holds the key, then the pair's append.
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

// memtable.Manager over maps: Mem and the logs of the memtables it froze.
struct Manager {
    uint64_t mem_max;
    std::map<std::string, std::string> list;  // Mem's skiplist
    uint64_t size = 0;                         // Mem's sizeInBytes
    std::vector<Bytes> logs{Bytes()};          // appended by this Manager; the last is Mem's

    void Insert(const std::string &k, const std::string &v) {  // manager.go:40-59
        const uint64_t est = 16 + k.size() + v.size();
        if (size + est > mem_max) {  // !CanInsert: promoteLocked
            list.clear();
            size = 0;
            logs.emplace_back();
        }
        put(logs.back(), k, v);
        list[k] = v;
        size += est;
    }
    void Delete(const std::string &k) {  // manager.go:76-106
        if (list.count(k)) put(logs.back(), k, "");  // MemTable.Delete, memtable.go:84-96
        Insert(k, kv::kDeletedValue);
    }
    void Apply(const std::vector<database::WriteOp> &ops) {
        for (const auto &op : ops) {
            if (op.op == LSM_OP_PUT) Insert(op.key, std::string(op.value.begin(), op.value.end()));
            else Delete(op.key);
        }
    }
};

static std::vector<database::WriteOp> RandomOps(std::mt19937_64 &rng, int n, int nkeys) {
    std::vector<database::WriteOp> ops(n);
    for (auto &op : ops) {
        op.key = rng() % 50 == 0 ? "" : "key" + std::to_string(rng() % nkeys);
        if (rng() % 3 == 0) {
            op.op = LSM_OP_DELETE;
            if (rng() % 2) op.value = {'x', 'y'};  // ignored
        } else {
            const std::string v = rng() % 9 == 0 ? kv::kDeletedValue : std::string(rng() % 40, 'v');
            op.value.assign(v.begin(), v.end());
        }
    }
    return ops;
}

static void TestWriteNothing() {  // host only: no ops -- no device call; bad arguments throw
    const auto r = database::WriteBatch({}, 123, 1000);
    CHECK(r.logs.size() == 1 && r.logs[0].empty() && r.mem_size == 123);
    database::WriteOp bad;
    bad.op = 7;
    bool threw = false;
    try {
        database::WriteBatch({bad});
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        database::WriteBatch({database::WriteOp()}, 0, 0);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    CHECK(database::kMaxMemTableSize == 2u * 1024 * 1024);
}

static void TestWriteVsMaps() {
    std::mt19937_64 rng(21);
    for (int round = 0; round < 6; round++) {
        const uint64_t mem_max = round == 0 ? 60000 : 200 + rng() % 3000;  // round 0: a log past one sort tile
        const auto ops = RandomOps(rng, round == 0 ? 3000 : 500, round == 0 ? 40 : 12);
        // a memtable that already holds pairs, on odd rounds
        Manager m{mem_max};
        Bytes current;
        if (round % 2) {
            for (int i = 0; i < 4; i++) m.Insert("key" + std::to_string(rng() % 12), i % 3 ? "old" : kv::kDeletedValue);
            m.Delete("key3");
            CHECK(m.logs.size() == 1);  // at most 169 of the 200 bytes: still the one memtable
            current = m.logs[0];
            m.logs[0].clear();
        }
        const uint64_t size0 = m.size;
        m.Apply(ops);
        const auto got = database::WriteBatch(ops, size0, mem_max, current);
        CHECK(got.logs.size() == m.logs.size());
        CHECK(got.mem_size == m.size);
        for (size_t s = 0; s < m.logs.size() && s < got.logs.size(); s++) CHECK(got.logs[s] == m.logs[s]);
        if (round) CHECK(m.logs.size() > 3);
        // two calls over the halves: the second continues the first's open log
        const size_t cut = ops.size() / 3;
        const std::vector<database::WriteOp> a(ops.begin(), ops.begin() + cut), b(ops.begin() + cut, ops.end());
        const auto ra = database::WriteBatch(a, size0, mem_max, current);
        Bytes open = ra.logs.size() == 1 ? current : Bytes();
        open.insert(open.end(), ra.logs.back().begin(), ra.logs.back().end());
        const auto rb = database::WriteBatch(b, ra.mem_size, mem_max, open);
        std::vector<Bytes> joined(ra.logs.begin(), ra.logs.end());
        joined.back().insert(joined.back().end(), rb.logs[0].begin(), rb.logs[0].end());
        joined.insert(joined.end(), rb.logs.begin() + 1, rb.logs.end());
        CHECK(joined == got.logs);
        CHECK(rb.mem_size == got.mem_size);
    }
}

int main(int argc, char **argv) {
    struct {
        const char *name;
        void (*fn)();
    } tests[] = {{"TestWriteNothing", TestWriteNothing}, {"TestWriteVsMaps", TestWriteVsMaps}};
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
