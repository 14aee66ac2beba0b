// CPU test of the collection types: the type-string parser and resolve_schema
// (cassandra_amd/csrc/sstable_meta.h) and the cell-path comparator the
// kernels run (cassandra_amd/csrc/cell_path.h). Plain host C++, no HIP.
#include "../../cassandra_amd/csrc/sstable_meta.h"
#include "../../cassandra_amd/csrc/cell_path.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static const std::string BYTES_T = M + "BytesType", UTF8_T = M + "UTF8Type",
                         ASCII_T = M + "AsciiType", INT32_T = M + "Int32Type",
                         LONG_T = M + "LongType", TS_T = M + "TimestampType",
                         UUID_T = M + "UUIDType";
static std::string set_of(const std::string& k) { return M + "SetType(" + k + ")"; }
static std::string list_of(const std::string& k) { return M + "ListType(" + k + ")"; }
static std::string map_of(const std::string& k, const std::string& v) {
    return M + "MapType(" + k + "," + v + ")";
}
static std::string frozen(const std::string& t) { return M + "FrozenType(" + t + ")"; }

using Col = std::pair<std::string, std::string>;
static HStatistics header(const std::vector<Col>& regular, const std::vector<Col>& statics = {}) {
    HStatistics st;
    st.key_type = BYTES_T;
    for (auto& c : regular) st.regular_cols.push_back({bytes(c.first.begin(), c.first.end()), c.second});
    for (auto& c : statics) st.static_cols.push_back({bytes(c.first.begin(), c.first.end()), c.second});
    return st;
}
static std::string names(const std::vector<std::pair<bytes, std::string>>& cols) {
    std::string s;
    for (auto& c : cols) s += (s.empty() ? "" : ",") + std::string(c.first.begin(), c.first.end());
    return s;
}
// the message of the exception a callable ends with ("" = none); "U:" marks
// an unsupported_error
static std::string refusal(const std::function<void()>& fn) {
    try { fn(); }
    catch (const unsupported_error& e) { return std::string("U:") + e.what(); }
    catch (const std::exception& e) { return *e.what() ? e.what() : "?"; }
    return "";
}

// ---- the comparator's reference: plain integer compares --------------------
static int sgn(long long a, long long b) { return (a > b) - (a < b); }
static void be(int64_t v, int w, uint8_t* out) {
    for (int i = 0; i < w; i++) out[i] = (uint8_t)((uint64_t)v >> (8 * (w - 1 - i)));
}
static int norm(int c) { return (c > 0) - (c < 0); }

int main() {
    // ---- parser: every accepted string ----
    const std::string keys[6] = {BYTES_T, UTF8_T, ASCII_T, INT32_T, LONG_T, TS_T};
    const int32_t key_w[6] = {0, 0, 0, 4, 8, 8};
    const std::string vals[5] = {BYTES_T, UTF8_T, ASCII_T, frozen(list_of(INT32_T)),
                                 frozen(map_of(UTF8_T, set_of(LONG_T)))};
    for (int k = 0; k < 6; k++) {
        CollectionType c = collection_type(set_of(keys[k]));
        CHECK(c.is_set && c.key_width == key_w[k], "set of %s", keys[k].c_str());
        for (auto& v : vals) {
            if (keys[k] == LONG_T && v == BYTES_T) continue;  // held back, below
            c = collection_type(map_of(keys[k], v));
            CHECK(!c.is_set && c.key_width == key_w[k], "map %s -> %s", keys[k].c_str(), v.c_str());
        }
    }
    {   // top-level comma only
        std::vector<std::string> a = type_args(map_of(UTF8_T, frozen(map_of(ASCII_T, BYTES_T))));
        CHECK(a.size() == 2 && a[0] == UTF8_T && a[1] == frozen(map_of(ASCII_T, BYTES_T)),
              "%zu args", a.size());
        a = type_args(frozen(map_of(ASCII_T, BYTES_T)));
        CHECK(a.size() == 1 && a[0] == map_of(ASCII_T, BYTES_T), "frozen arg");
        CHECK(!refusal([] { type_args(M + "MapType(a,(b)"); }).empty(), "unbalanced");
        CHECK(!refusal([] { type_args(M + "MapType(a))(b)"); }).empty(), "unbalanced 2");
    }
    CHECK(frozen_type(frozen(map_of(ASCII_T, BYTES_T))) && !frozen_type(map_of(ASCII_T, BYTES_T)) &&
          !frozen_type(M + "FrozenType(x"), "frozen_type");
    CHECK(multicell_type(list_of(UTF8_T)) && multicell_type(set_of(UTF8_T)) &&
          !multicell_type(frozen(map_of(ASCII_T, BYTES_T))) && !multicell_type(BYTES_T), "multicell_type");

    // ---- parser: every refusal names the whole type string ----
    auto refused = [](const std::string& t, const char* also) {
        std::string r = refusal([&] { collection_type(t); });
        CHECK(r.find("unsupported column type " + t) == 0, "'%s' for %s", r.c_str(), t.c_str());
        CHECK(r.find(also) != std::string::npos, "'%s' lacks '%s'", r.c_str(), also);
    };
    refused(list_of(UTF8_T), "TimeUUIDType");
    refused(list_of(frozen(list_of(UTF8_T))), "TimeUUIDType");
    for (auto& v : {INT32_T, LONG_T, TS_T}) refused(map_of(UTF8_T, v), "length prefix");
    refused(map_of(frozen(list_of(UTF8_T)), BYTES_T), "key type");
    refused(set_of(frozen(set_of(UTF8_T))), "key type");
    refused(set_of(UUID_T), "key type");
    refused(map_of(UTF8_T, UUID_T), "value type");
    refused(map_of(UTF8_T, set_of(UTF8_T)), "value type");      // nested multi-cell
    refused(map_of(UTF8_T, M + "ReversedType(" + UTF8_T + ")"), "value type");
    refused(map_of(LONG_T, BYTES_T), "held back");  // pinned by the earlier native tests
    refused(set_of(UTF8_T + "," + UTF8_T), "");                  // arity
    refused(M + "MapType(" + UTF8_T + ")", "");
    refused(M + "SetType(" + UTF8_T, "");                        // no closing bracket

    // ---- resolve_schema: masks and widths ----
    {
        HostSchema hs = resolve_schema(header(
            {{"a", BYTES_T}, {"f", frozen(list_of(INT32_T))}, {"l", LONG_T},
             {"z0", map_of(BYTES_T, BYTES_T)}, {"z1", set_of(INT32_T)}, {"z2", map_of(TS_T, UTF8_T)},
             {"z3", set_of(ASCII_T)}, {"z4", map_of(LONG_T, frozen(set_of(UTF8_T)))}},
            {{"s", frozen(set_of(INT32_T))}}));
        CHECK(hs.col_fixed == std::vector<int32_t>({-1, -1, 8}), "simple widths");
        CHECK(hs.static_fixed == std::vector<int32_t>({-1}), "static widths");
        CHECK(hs.n_cpx == 5, "n_cpx %u", hs.n_cpx);
        CHECK(hs.cpx_key_w == std::vector<uint8_t>({0, 4, 8, 0, 8}), "key widths");
        CHECK(hs.cpx_set == std::vector<uint8_t>({0, 1, 0, 1, 0}), "sets");
        CHECK(hs.cpx_key_signed_mask() == 0x16 && hs.cpx_key_w8_mask() == 0x14 &&
              hs.cpx_is_set_mask() == 0x0A, "masks %llx %llx %llx",
              (unsigned long long)hs.cpx_key_signed_mask(), (unsigned long long)hs.cpx_key_w8_mask(),
              (unsigned long long)hs.cpx_is_set_mask());
        for (uint32_t x = 0; x < 5; x++)
            CHECK(cpx_key_width(hs.cpx_key_signed_mask(), hs.cpx_key_w8_mask(), x) == hs.cpx_key_w[x],
                  "width of column %u", x);
        // all byte-ordered: every mask zero, as before these types
        hs = resolve_schema(header({{"a", BYTES_T}, {"zm", map_of(BYTES_T, BYTES_T)}, {"zn", set_of(UTF8_T)}}));
        CHECK(hs.n_cpx == 2 && !hs.cpx_key_signed_mask() && !hs.cpx_key_w8_mask() &&
              hs.cpx_is_set_mask() == 2, "byte-ordered masks");
        // bit 62: the last complex column a header can hold
        std::vector<Col> many;
        for (int i = 0; i < 63; i++) many.push_back({"z" + std::to_string(100 + i), i == 62 ? set_of(LONG_T) : set_of(UTF8_T)});
        hs = resolve_schema(header(many));
        CHECK(hs.n_cpx == 63 && hs.cpx_key_signed_mask() == 1ull << 62 &&
              hs.cpx_key_w8_mask() == 1ull << 62 && hs.cpx_is_set_mask() == (1ull << 63) - 1, "63 sets");
    }
    {   // refusals of resolve_schema: the exception type they had before
        std::string r = refusal([] { resolve_schema(header({{"a", BYTES_T}, {"zl", list_of(UTF8_T)}})); });
        CHECK(r.find("unsupported column type " + list_of(UTF8_T)) == 0, "list: '%s'", r.c_str());
        r = refusal([] { resolve_schema(header({{"a", BYTES_T}}, {{"s", set_of(UTF8_T)}})); });
        CHECK(r.find("unsupported static column type " + set_of(UTF8_T)) == 0, "static set: '%s'", r.c_str());
        r = refusal([] { resolve_schema(header({{"zs", set_of(UTF8_T)}, {"zz", frozen(set_of(UTF8_T))}})); });
        CHECK(r.find("must follow every simple") != std::string::npos, "frozen after a set: '%s'", r.c_str());
        r = refusal([] { resolve_schema(header({{"c", M + "CounterColumnType"}, {"zs", set_of(UTF8_T)}})); });
        CHECK(r.find("counter") != std::string::npos, "counter with a set: '%s'", r.c_str());
        // FrozenType is never a clustering or key type
        HStatistics st = header({{"a", BYTES_T}});
        st.clustering_types = {frozen(list_of(UTF8_T))};
        r = refusal([&] { resolve_schema(st); });
        CHECK(r.find("unsupported clustering type") != std::string::npos, "frozen ck: '%s'", r.c_str());
    }

    // ---- union order ----
    {
        const std::string FZ = frozen(map_of(UTF8_T, INT32_T));
        HStatistics x = header({{"a", BYTES_T}, {"m", FZ}});
        HStatistics y = header({{"a", BYTES_T}, {"b", set_of(INT32_T)}, {"c", map_of(UTF8_T, UTF8_T)}});
        JobSchema js = resolve_job_schema({x, y}, 2);
        // the frozen column (its string holds "MapType(") stays with the simple ones
        CHECK(names(js.header.regular_cols) == "a,m,b,c", "order: %s", names(js.header.regular_cols).c_str());
        CHECK(js.schema.col_fixed.size() == 2 && js.schema.n_cpx == 2 &&
              js.schema.cpx_key_signed_mask() == 1 && js.schema.cpx_is_set_mask() == 1, "union schema");
        CHECK(js.src[0].col_map == std::vector<uint8_t>({0, 1}) && js.src[0].cpx_map.empty() &&
              js.src[1].col_map == std::vector<uint8_t>({0}) &&
              js.src[1].cpx_map == std::vector<uint8_t>({0, 1}), "maps");
        // a list sorts as complex, so its refusal names it (not "Columns order")
        HStatistics z = header({{"a", BYTES_T}, {"d", list_of(UTF8_T)}});
        std::string r = refusal([&] { resolve_job_schema({x, y, z}, 3); });
        CHECK(r.find("unsupported column type " + list_of(UTF8_T)) == 0, "list in a union: '%s'", r.c_str());
        // one name, two collection types: the existing type-conflict refusal
        HStatistics w = header({{"a", BYTES_T}, {"b", set_of(UTF8_T)}});
        r = refusal([&] { resolve_job_schema({y, w}, 2); });
        CHECK(r.compare(0, 2, "U:") == 0 && r.find("'b'") != std::string::npos &&
              r.find(set_of(UTF8_T)) != std::string::npos && r.find(set_of(INT32_T)) != std::string::npos,
              "conflict: '%s'", r.c_str());
    }

    // ---- comparator ----
    for (int w : {4, 8}) {
        const int64_t mn = w == 4 ? INT32_MIN : INT64_MIN, mx = w == 4 ? INT32_MAX : INT64_MAX;
        const int64_t v[] = {mn, mn + 1, -256, -255, -2, -1, 0, 1, 2, 127, 128, 255, 256, mx - 1, mx};
        for (int64_t a : v)
            for (int64_t b : v) {
                uint8_t pa[8], pb[8];
                be(a, w, pa);
                be(b, w, pb);
                CHECK(norm(cell_path_cmp(pa, w, pb, w, true)) == sgn(a, b), "signed w=%d %lld %lld", w,
                      (long long)a, (long long)b);
                // the byte order of the same bytes: unsigned integers
                uint64_t ua = w == 4 ? (uint32_t)a : (uint64_t)a, ub = w == 4 ? (uint32_t)b : (uint64_t)b;
                CHECK(norm(cell_path_cmp(pa, w, pb, w, false)) == (ua > ub) - (ua < ub),
                      "unsigned w=%d %lld %lld", w, (long long)a, (long long)b);
            }
    }
    {   // byte-ordered keys: memcmp then length; and the signed form over
        // unequal lengths stays a total order (first byte signed, shorter first)
        const std::vector<bytes> ps = {{}, {0x00}, {0x00, 0x00}, {'a'}, {'a', 'b'}, {'b'}, {0x7f},
                                       {0x80}, {0x80, 0x00}, {0xff}, {0xff, 0xff}};
        for (auto& a : ps)
            for (auto& b : ps) {
                int want = a < b ? -1 : (b < a ? 1 : 0);  // vector<uint8_t>: unsigned lex, prefix first
                CHECK(norm(cell_path_cmp(a.data(), (uint32_t)a.size(), b.data(), (uint32_t)b.size(), false)) == want,
                      "bytes");
                bytes fa = a, fb = b;
                if (!fa.empty()) fa[0] ^= 0x80;
                if (!fb.empty()) fb[0] ^= 0x80;
                want = fa < fb ? -1 : (fb < fa ? 1 : 0);
                CHECK(norm(cell_path_cmp(a.data(), (uint32_t)a.size(), b.data(), (uint32_t)b.size(), true)) == want,
                      "signed, any length");
            }
    }
    printf("collection_types_test OK\n");
    return 0;
}
