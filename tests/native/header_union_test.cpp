// CPU test of resolve_job_schema (cassandra_amd/csrc/sstable_meta.h): the
// union header of a job whose inputs list different columns, the per-source
// maps into it, and every rejection. Plain host C++, no HIP.
//
// usage: header_union_test <U1 Statistics.db x4> <U4 Statistics.db x3>
//   U1 (tests/header_union_tables.py): {a,c}; {b,zm}+{s2}; {}; {a,zm}+{s1}
//   U4: {a,zm1}; {zm1,zm2}; {a,zm2}
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

static const std::string BYTES_T = "org.apache.cassandra.db.marshal.BytesType";
static const std::string LONG_T = "org.apache.cassandra.db.marshal.LongType";
static const std::string UTF8_T = "org.apache.cassandra.db.marshal.UTF8Type";
static const std::string CTR_T = "org.apache.cassandra.db.marshal.CounterColumnType";
static const std::string MAP_T =
    "org.apache.cassandra.db.marshal.MapType(org.apache.cassandra.db.marshal.BytesType,"
    "org.apache.cassandra.db.marshal.BytesType)";
static const std::string MAP_LONG_T =
    "org.apache.cassandra.db.marshal.MapType(org.apache.cassandra.db.marshal.LongType,"
    "org.apache.cassandra.db.marshal.BytesType)";

using Col = std::pair<std::string, std::string>;
using U8 = std::vector<uint8_t>;

static HStatistics header(const std::vector<Col>& regular, const std::vector<Col>& statics = {}) {
    HStatistics st;
    st.key_type = LONG_T;
    st.clustering_types = {LONG_T};
    for (auto& c : regular) st.regular_cols.push_back({bytes(c.first.begin(), c.first.end()), c.second});
    for (auto& c : statics) st.static_cols.push_back({bytes(c.first.begin(), c.first.end()), c.second});
    return st;
}
static std::string names(const std::vector<std::pair<bytes, std::string>>& cols) {
    std::string s;
    for (auto& c : cols) s += (s.empty() ? "" : ",") + std::string(c.first.begin(), c.first.end());
    return s;
}
// what a callable ends with: "" none, "U:<msg>" unsupported_error, "E:<msg>" any other
static std::string refusal(const std::function<void()>& fn) {
    try { fn(); }
    catch (const unsupported_error& e) { return std::string("U:") + e.what(); }
    catch (const std::exception& e) { return std::string("E:") + e.what(); }
    return "";
}
static bool unsupported_naming(const std::string& r, const char* column) {
    return r.compare(0, 2, "U:") == 0 && r.find(std::string("'") + column + "'") != std::string::npos;
}
static HStatistics load(const char* path) {
    bytes b;
    FILE* f = fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return parse_statistics(b);
}
static void check_source(const JobSchema& js, size_t s, const U8& col, const U8& cpx, const U8& st) {
    const SourceColumns& sc = js.src[s];
    CHECK(sc.col_map == col && sc.n_cols == col.size(), "source %zu simple map (%u)", s, sc.n_cols);
    CHECK(sc.cpx_map == cpx && sc.n_cpx == cpx.size(), "source %zu complex map (%u)", s, sc.n_cpx);
    CHECK(sc.static_map == st && sc.n_static == st.size(), "source %zu static map (%u)", s, sc.n_static);
}

int main(int argc, char** argv) {
    CHECK(argc == 8, "usage: %s <4 U1 Statistics.db> <3 U4 Statistics.db>", argv[0]);
    {   // U1, from the authored files
        std::vector<HStatistics> st;
        for (int i = 1; i <= 4; i++) st.push_back(load(argv[i]));
        JobSchema js = resolve_job_schema(st, 4);
        CHECK(names(js.header.regular_cols) == "a,b,c,zm", "U1 regular: %s", names(js.header.regular_cols).c_str());
        CHECK(names(js.header.static_cols) == "s1,s2", "U1 static: %s", names(js.header.static_cols).c_str());
        CHECK(js.header.regular_cols[1].second == LONG_T && js.header.regular_cols[3].second == MAP_T, "U1 types");
        CHECK(js.header.key_type == st[0].key_type && js.header.clustering_types == st[0].clustering_types &&
              js.header.partitioner == st[0].partitioner && js.header.min_timestamp == st[0].min_timestamp,
              "the rest of the header is input 0's");
        CHECK(js.schema.col_fixed == std::vector<int32_t>({-1, 8, -1}) && js.schema.n_cpx == 1, "U1 widths");
        CHECK(js.schema.static_fixed == std::vector<int32_t>({-1, 8}), "U1 static widths");
        CHECK(js.src.size() == 4, "%zu sources", js.src.size());
        check_source(js, 0, {0, 2}, {}, {});
        check_source(js, 1, {1}, {0}, {1});
        check_source(js, 2, {}, {}, {});        // empty regular header, no statics
        check_source(js, 3, {0}, {0}, {0});
        // the union does not depend on the order of the inputs
        std::vector<HStatistics> rev(st.rbegin(), st.rend());
        JobSchema jr = resolve_job_schema(rev, 4);
        CHECK(jr.header.regular_cols == js.header.regular_cols && jr.header.static_cols == js.header.static_cols,
              "union depends on the input order");
        check_source(jr, 3, {0, 2}, {}, {});
        // the last two as tombstone sources: they add no column
        JobSchema jt = resolve_job_schema({st[1], st[3], st[2], st[3]}, 2);
        CHECK(names(jt.header.regular_cols) == "a,b,zm" && names(jt.header.static_cols) == "s1,s2", "data union");
        check_source(jt, 0, {1}, {0}, {1});
        check_source(jt, 1, {0}, {0}, {0});
        check_source(jt, 2, {}, {}, {});
        check_source(jt, 3, {0}, {0}, {0});
        // {a,c} as a tombstone source of {b,zm}: c (and a) shadow nothing
        std::string r = refusal([&] { resolve_job_schema({st[1], st[0]}, 1); });
        CHECK(unsupported_naming(r, "a") && r.find("tombstone source") != std::string::npos, "'%s'", r.c_str());
        // an empty header alone: the union has no regular column
        r = refusal([&] { resolve_job_schema({st[2]}, 1); });
        CHECK(r.find("regular columns") != std::string::npos, "empty union: '%s'", r.c_str());
    }
    {   // U4: a header with no simple column in the middle
        std::vector<HStatistics> st;
        for (int i = 5; i <= 7; i++) st.push_back(load(argv[i]));
        JobSchema js = resolve_job_schema(st, 3);
        CHECK(names(js.header.regular_cols) == "a,zm1,zm2", "U4 regular: %s", names(js.header.regular_cols).c_str());
        CHECK(js.schema.col_fixed == std::vector<int32_t>({-1}) && js.schema.n_cpx == 2, "U4 widths");
        check_source(js, 0, {0}, {0}, {});
        check_source(js, 1, {}, {0, 1}, {});
        check_source(js, 2, {0}, {1}, {});
        // single source: the header as it stands, identity maps
        JobSchema j1 = resolve_job_schema({st[1]}, 1);
        CHECK(names(j1.header.regular_cols) == "zm1,zm2" && j1.schema.col_fixed.empty() && j1.schema.n_cpx == 2, "U4 single");
        check_source(j1, 0, {}, {0, 1}, {});
    }
    {   // identity: equal headers are taken as they stand, whatever their order
        HStatistics h = header({{"val0", BYTES_T}, {"val1", LONG_T}, {"val10", BYTES_T}, {"val2", BYTES_T}, {"zm", MAP_T}},
                               {{"s0", BYTES_T}});
        HStatistics g = header({{"val0", BYTES_T}, {"val1", BYTES_T}, {"val2", BYTES_T}, {"val10", BYTES_T}});
        JobSchema js = resolve_job_schema({h, h, h}, 2);
        CHECK(js.header.regular_cols == h.regular_cols && js.header.static_cols == h.static_cols, "identity header");
        HostSchema one = resolve_schema(h);
        CHECK(js.schema.col_fixed == one.col_fixed && js.schema.n_cpx == one.n_cpx &&
              js.schema.static_fixed == one.static_fixed && js.schema.ck_widths == one.ck_widths, "identity schema");
        for (size_t s = 0; s < 3; s++) check_source(js, s, {0, 1, 2, 3}, {0}, {0});
        js = resolve_job_schema({g, g}, 2);     // not in name order, but the same in every input
        CHECK(js.header.regular_cols == g.regular_cols, "equal headers keep their order");
        check_source(js, 1, {0, 1, 2, 3}, {}, {});
    }
    {   // Columns order: simple by name, then complex by name; a prefix before its extensions
        HStatistics x = header({{"b", BYTES_T}, {"bb", LONG_T}, {"a", MAP_T}});
        HStatistics y = header({{"\x80", BYTES_T}, {"zz", MAP_T}});
        HStatistics z = header({{"B", BYTES_T}, {"a", MAP_T}, {"zz", MAP_T}});
        JobSchema js = resolve_job_schema({x, y, z}, 3);
        CHECK(names(js.header.regular_cols) == "B,b,bb,\x80,a,zz", "order: %s", names(js.header.regular_cols).c_str());
        check_source(js, 0, {1, 2}, {0}, {});
        check_source(js, 1, {3}, {1}, {});
        check_source(js, 2, {0}, {0, 1}, {});
    }
    // ---- rejections: unsupported_error, the column named ----
    std::string r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}, {"b", LONG_T}}), header({{"b", BYTES_T}})}, 2); });
    CHECK(unsupported_naming(r, "b"), "b bigint/blob: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}}, {{"s", LONG_T}}), header({{"a", BYTES_T}}, {{"s", BYTES_T}})}, 2); });
    CHECK(unsupported_naming(r, "s"), "static s bigint/blob: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}, {"b", LONG_T}}), header({{"b", BYTES_T}})}, 1); });
    CHECK(unsupported_naming(r, "b"), "type conflict with a tombstone source: '%s'", r.c_str());
    {
        HStatistics t = header({{"a", BYTES_T}});
        t.clustering_types = {UTF8_T};
        r = refusal([&] { resolve_job_schema({header({{"a", BYTES_T}, {"b", BYTES_T}}), t}, 2); });
        CHECK(r.compare(0, 2, "U:") == 0 && r.find("clustering") != std::string::npos, "clustering: '%s'", r.c_str());
        r = refusal([&] { resolve_job_schema({header({{"a", BYTES_T}}), t}, 1); });
        CHECK(r.compare(0, 2, "U:") == 0 && r.find("clustering") != std::string::npos, "clustering of a source: '%s'", r.c_str());
        t = header({{"a", BYTES_T}});
        t.key_type = BYTES_T;
        r = refusal([&] { resolve_job_schema({header({{"a", BYTES_T}, {"b", BYTES_T}}), t}, 2); });
        CHECK(r.compare(0, 2, "U:") == 0 && r.find("key type") != std::string::npos, "key type: '%s'", r.c_str());
    }
    // a header out of Columns order is no subsequence of the union
    r = refusal([] { resolve_job_schema({header({{"b", BYTES_T}, {"a", BYTES_T}}), header({{"a", BYTES_T}})}, 2); });
    CHECK(unsupported_naming(r, "a") && r.find("Columns order") != std::string::npos, "b,a: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"zm", MAP_T}, {"zz", BYTES_T}}), header({{"zz", BYTES_T}})}, 2); });
    CHECK(unsupported_naming(r, "zz") && r.find("Columns order") != std::string::npos, "map first: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}}, {{"t", BYTES_T}, {"s", BYTES_T}}), header({{"a", BYTES_T}})}, 2); });
    CHECK(unsupported_naming(r, "s") && r.find("Columns order") != std::string::npos, "statics t,s: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}}), header({{"b", BYTES_T}, {"a", BYTES_T}})}, 1); });
    CHECK(unsupported_naming(r, "b"), "tombstone source out of the union: '%s'", r.c_str());
    // a tombstone source with a column that no compacting input has
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}}), header({{"a", BYTES_T}, {"b", BYTES_T}})}, 1); });
    CHECK(unsupported_naming(r, "b") && r.find("tombstone source") != std::string::npos, "'%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}}), header({{"a", BYTES_T}}, {{"s", BYTES_T}})}, 1); });
    CHECK(unsupported_naming(r, "s") && r.find("tombstone source") != std::string::npos, "'%s'", r.c_str());
    // the existing rejections, unchanged, now on the union
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}}), header({{"b", BYTES_T}}, {{"s", MAP_T}})}, 2); });
    CHECK(r.find("unsupported static column type") != std::string::npos, "map static: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"c1", CTR_T}}), header({{"c1", CTR_T}, {"zm", MAP_T}})}, 2); });
    CHECK(r.find("counter") != std::string::npos, "counter table with a map: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"c1", CTR_T}}), header({{"c2", BYTES_T}})}, 2); });
    CHECK(r.find("counter") != std::string::npos, "counter and blob: '%s'", r.c_str());
    r = refusal([] { resolve_job_schema({header({{"a", BYTES_T}}), header({{"zm", MAP_LONG_T}})}, 2); });
    CHECK(r.find("unsupported column type") != std::string::npos, "map<bigint,blob>: '%s'", r.c_str());
    {   // the limits apply to the union: 40 + 40 distinct columns do not fit, 40 + 23 do
        std::vector<Col> lo, hi, hi2;
        for (int i = 0; i < 40; i++) lo.push_back({"a" + std::to_string(100 + i), BYTES_T});
        for (int i = 0; i < 40; i++) hi.push_back({"b" + std::to_string(100 + i), BYTES_T});
        hi2.assign(hi.begin(), hi.begin() + 23);
        r = refusal([&] { resolve_job_schema({header(lo), header(hi)}, 2); });
        CHECK(r.find("63") != std::string::npos, "80 columns: '%s'", r.c_str());
        JobSchema js = resolve_job_schema({header(lo), header(hi2)}, 2);
        CHECK(js.schema.col_fixed.size() == 63 && js.src[1].col_map.front() == 40 && js.src[1].col_map.back() == 62, "63 columns");
        r = refusal([&] { resolve_job_schema({header({{"a", BYTES_T}}, lo), header({{"a", BYTES_T}}, hi)}, 2); });
        CHECK(r.find("63") != std::string::npos, "80 statics: '%s'", r.c_str());
    }
    printf("OK\n");
    return 0;
}
