// CPU test of resolve_schema (cassandra_amd/csrc/sstable_meta.h) for tables
// with several complex columns. Plain host C++, no HIP.
//
// usage: multi_cpx_schema_test <Statistics.db of a widened sstable>
//   the sstable has two simple blob columns then the map columns zm, zn, zo
#include "../../cassandra_amd/csrc/sstable_meta.h"

#include <cstdio>
#include <cstdlib>
#include <functional>

using namespace gpuc;

#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);    \
            fprintf(stderr, __VA_ARGS__);                                      \
            fprintf(stderr, "\n");                                             \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static const char* BYTES_T = "org.apache.cassandra.db.marshal.BytesType";
static const char* LONG_T = "org.apache.cassandra.db.marshal.LongType";
static const char* CTR_T = "org.apache.cassandra.db.marshal.CounterColumnType";
static const char* MAP_T =
    "org.apache.cassandra.db.marshal.MapType(org.apache.cassandra.db.marshal.BytesType,"
    "org.apache.cassandra.db.marshal.BytesType)";
static const char* MAP_LONG_T =
    "org.apache.cassandra.db.marshal.MapType(org.apache.cassandra.db.marshal.LongType,"
    "org.apache.cassandra.db.marshal.BytesType)";

// the message of the exception a callable ends with ("" = none)
static std::string refusal(const std::function<void()>& fn) {
    try { fn(); }
    catch (const std::exception& e) { return *e.what() ? e.what() : "?"; }
    return "";
}

static HStatistics table(const std::vector<const char*>& types) {
    HStatistics st;
    for (size_t i = 0; i < types.size(); i++) {
        std::string nm = "c" + std::to_string(100 + i);
        st.regular_cols.push_back({bytes(nm.begin(), nm.end()), types[i]});
    }
    return st;
}

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: %s <Statistics.db>", argv[0]);
    bytes b;
    {
        FILE* f = fopen(argv[1], "rb");
        CHECK(f, "cannot open %s", argv[1]);
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
        fclose(f);
    }
    // a widened Statistics.db: two simple columns, three trailing maps
    HostSchema hs = resolve_schema(parse_statistics(b));
    CHECK(hs.n_cpx == 3, "n_cpx = %u", hs.n_cpx);
    CHECK(hs.col_fixed == std::vector<int32_t>({-1, -1}), "%zu simple columns", hs.col_fixed.size());
    CHECK(!hs.counters, "counters");

    // hand-built headers
    hs = resolve_schema(table({MAP_T, MAP_T}));  // no simple column at all
    CHECK(hs.n_cpx == 2 && hs.col_fixed.empty(), "maps only: %u", hs.n_cpx);
    hs = resolve_schema(table({LONG_T, BYTES_T, MAP_T}));
    CHECK(hs.n_cpx == 1 && hs.col_fixed == std::vector<int32_t>({8, -1}), "one map");
    hs = resolve_schema(table({LONG_T}));
    CHECK(hs.n_cpx == 0 && hs.col_fixed == std::vector<int32_t>({8}), "no map");

    std::string r = refusal([] { resolve_schema(table({BYTES_T, MAP_T, BYTES_T})); });
    CHECK(r.find("must follow every simple") != std::string::npos, "map before simple: '%s'",
          r.c_str());
    r = refusal([] { resolve_schema(table({MAP_T, BYTES_T, MAP_T})); });
    CHECK(!r.empty(), "map, simple, map accepted");
    r = refusal([] { resolve_schema(table({CTR_T, MAP_T})); });
    CHECK(r.find("counter") != std::string::npos, "counter table with a map: '%s'", r.c_str());
    r = refusal([] { resolve_schema(table({BYTES_T, MAP_LONG_T})); });
    CHECK(r.find("unsupported column type") != std::string::npos, "map<bigint,blob>: '%s'",
          r.c_str());
    {   // complex static columns stay rejected
        HStatistics st = table({BYTES_T, MAP_T});
        st.static_cols.push_back({bytes{'s'}, MAP_T});
        r = refusal([&] { resolve_schema(st); });
        CHECK(r.find("unsupported static column type") != std::string::npos, "map static: '%s'",
              r.c_str());
    }
    {   // the subset bitmap stays below 64 bits: 61 + 2 fits, 62 + 2 does not
        std::vector<const char*> t(61, BYTES_T);
        t.push_back(MAP_T);
        t.push_back(MAP_T);
        hs = resolve_schema(table(t));
        CHECK(hs.n_cpx == 2 && hs.col_fixed.size() == 61, "61 + 2");
        t.insert(t.begin(), BYTES_T);
        r = refusal([&] { resolve_schema(table(t)); });
        CHECK(r.find("63") != std::string::npos, "62 + 2: '%s'", r.c_str());
    }
    printf("OK\n");
    return 0;
}
