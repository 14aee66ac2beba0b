// CPU test of the clustering type resolution (cassandra_amd/csrc/sstable_meta.h):
// ReversedType(T) clustering columns, TimestampType, and every refusal.
// Plain host C++, no HIP.
//
// usage: desc_schema_test                      the resolver checks
//        desc_schema_test <Statistics.db>      prints the HEADER clustering
//                                              type strings parse_statistics
//                                              reads, one per line
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

static const std::string M = "org.apache.cassandra.db.marshal.";
static std::string rev(const std::string& t) { return M + "ReversedType(" + t + ")"; }

static HStatistics header(const std::vector<std::string>& ck) {
    HStatistics st;
    st.key_type = M + "LongType";
    st.clustering_types = ck;
    st.regular_cols.push_back({bytes{'v'}, M + "BytesType"});
    return st;
}
// what a callable ends with: "" none, "U:<msg>" unsupported_error, "E:<msg>" any other
static std::string refusal(const std::function<void()>& fn) {
    try { fn(); }
    catch (const unsupported_error& e) { return std::string("U:") + e.what(); }
    catch (const std::exception& e) { return std::string("E:") + e.what(); }
    return "";
}
static void refused_naming(const HStatistics& st, const std::string& type) {
    std::string r = refusal([&] { resolve_schema(st); });
    CHECK(r.compare(0, 2, "U:") == 0, "not an unsupported_error: '%s'", r.c_str());
    CHECK(r.find(type) != std::string::npos, "'%s' does not carry %s", r.c_str(), type.c_str());
}

int main(int argc, char** argv) {
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        CHECK(f, "cannot open %s", argv[1]);
        bytes b;
        uint8_t buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
        fclose(f);
        HStatistics st = parse_statistics(b);
        for (auto& t : st.clustering_types) printf("%s\n", t.c_str());
        HostSchema hs = resolve_schema(st);
        printf("desc_mask=%u\n", hs.ck_desc_mask());
        return 0;
    }

    // the 12 accepted clustering strings: width of the inner type, flag
    const std::pair<const char*, int32_t> base[6] = {
        {"LongType", 8}, {"Int32Type", 4}, {"UTF8Type", -1},
        {"AsciiType", -1}, {"BytesType", -1}, {"TimestampType", 8}};
    for (auto& [name, width] : base) {
        for (int desc = 0; desc < 2; desc++) {
            std::string t = desc ? rev(M + name) : M + name;
            HostSchema hs = resolve_schema(header({t}));
            CHECK(hs.ck_widths.size() == 1 && hs.ck_widths[0] == width, "%s: width %d", t.c_str(),
                  hs.ck_widths.empty() ? 0 : hs.ck_widths[0]);
            CHECK(hs.ck_desc.size() == 1 && hs.ck_desc[0] == desc, "%s: flag", t.c_str());
            CHECK(hs.ck_desc_mask() == (uint32_t)desc, "%s: mask", t.c_str());
        }
    }
    // the flag is per component
    {
        HostSchema hs = resolve_schema(
            header({M + "LongType", rev(M + "UTF8Type"), M + "Int32Type", rev(M + "TimestampType")}));
        CHECK(hs.ck_desc_mask() == 0b1010u, "mask %u", hs.ck_desc_mask());
        CHECK(hs.ck_widths == (std::vector<int32_t>{8, -1, 4, 8}), "widths");
    }
    // TimestampType as a regular and as a static column: 8 bytes
    {
        HStatistics st = header({rev(M + "TimestampType")});
        st.regular_cols.push_back({bytes{'w'}, M + "TimestampType"});
        st.static_cols.push_back({bytes{'s'}, M + "TimestampType"});
        HostSchema hs = resolve_schema(st);
        CHECK(hs.col_fixed == (std::vector<int32_t>{-1, 8}), "regular widths");
        CHECK(hs.static_fixed == (std::vector<int32_t>{8}), "static width");
    }
    // refusals, the type string in the message
    refused_naming(header({rev(rev(M + "LongType"))}), rev(rev(M + "LongType")));
    refused_naming(header({rev(M + "UUIDType")}), rev(M + "UUIDType"));
    refused_naming(header({M + "UUIDType"}), M + "UUIDType");
    refused_naming(header({M + "ReversedType(" + M + "LongType"}), "ReversedType(");  // unclosed
    {
        HStatistics st = header({M + "LongType"});
        st.key_type = rev(M + "LongType");
        refused_naming(st, st.key_type);
    }
    {
        HStatistics st = header({M + "LongType"});
        st.regular_cols.push_back({bytes{'w'}, rev(M + "LongType")});
        refused_naming(st, rev(M + "LongType"));
    }
    {
        HStatistics st = header({M + "LongType"});
        st.static_cols.push_back({bytes{'s'}, rev(M + "BytesType")});
        refused_naming(st, rev(M + "BytesType"));
    }
    // one input ascending, one descending over the same base type
    {
        std::vector<HStatistics> stats = {header({M + "LongType"}), header({rev(M + "LongType")})};
        std::string r = refusal([&] { resolve_job_schema(stats, 2); });
        CHECK(r == "U:inputs differ in their clustering types", "'%s'", r.c_str());
        stats[0] = stats[1];
        JobSchema js = resolve_job_schema(stats, 2);
        CHECK(js.schema.ck_desc_mask() == 1u, "job mask");
        CHECK(js.header.clustering_types[0] == rev(M + "LongType"), "output header keeps the string");
    }
    printf("desc_schema_test OK\n");
    return 0;
}
