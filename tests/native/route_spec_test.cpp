// CPU test of cassandra_amd/csrc/route_spec.h (host-only; plain g++, no HIP):
// the token -> output lookup that the routing kernel also runs, and the spec
// check of gpuc_compact_routed.
//
//   route_spec_test
//
// For every generated routing table the lookup must equal an independent
// linear scan with the interval test written out, on every bound, every
// bound +- 1 (without overflow at INT64_MIN / INT64_MAX) and a sweep of other
// tokens; every malformed spec must be refused with its index in the message.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../cassandra_amd/csrc/route_spec.h"

using namespace gpuc;

static int g_fail = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);               \
            fprintf(stderr, "\n");                      \
            g_fail++;                                   \
        }                                               \
    } while (0)

struct Table {
    std::vector<const char*> bases;
    std::vector<int64_t> lo, hi;
    std::vector<int32_t> out;
    int32_t dflt = 0;
    void add(int64_t l, int64_t h, int32_t o) {
        lo.push_back(l);
        hi.push_back(h);
        out.push_back(o);
    }
    gpuc_route_spec spec() const {
        return gpuc_route_spec{(uint32_t)bases.size(), bases.data(), (uint32_t)lo.size(),
                               lo.data(), hi.data(), out.data(), dflt};
    }
};

static const char* BASES[] = {"/o/oa-1-big", "/o/oa-2-big", "/o/oa-3-big", "/o/oa-4-big",
                              "/o/oa-5-big"};

static Table table(uint32_t n_outputs, int32_t dflt) {
    Table t;
    for (uint32_t i = 0; i < n_outputs; i++) t.bases.push_back(BASES[i]);
    t.dflt = dflt;
    return t;
}

// independent of route_output_of: every range's [lo, hi] tested in turn
static int32_t linear_output(const Table& t, int64_t token) {
    for (size_t i = 0; i < t.lo.size(); i++)
        if (t.lo[i] <= token && token <= t.hi[i]) return t.out[i];
    return t.dflt;
}

static uint64_t g_lookups = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rng() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static void check_table(const char* name, const Table& t) {
    gpuc_route_spec s = t.spec();
    std::string e = route_spec_error(&s);
    CHECK(e.empty(), "%s: well-formed spec refused: %s", name, e.c_str());
    if (!e.empty()) return;
    std::vector<int64_t> probes{INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX};
    for (int which = 0; which < 2; which++)
        for (int64_t b : which ? t.hi : t.lo) {
            probes.push_back(b);
            if (b != INT64_MIN) probes.push_back(b - 1);
            if (b != INT64_MAX) probes.push_back(b + 1);
        }
    for (int i = 0; i < 4000; i++) probes.push_back((int64_t)rng());
    uint64_t in_range = 0, dropped = 0;
    for (int64_t tok : probes) {
        int32_t got = route_output_of(s.range_lo, s.range_hi, s.range_output, s.n_ranges,
                                      s.default_output, tok);
        int32_t want = linear_output(t, tok);
        CHECK(got == want, "%s: token %lld -> %d, linear scan says %d", name, (long long)tok,
              got, want);
        in_range += want != t.dflt;
        dropped += want == -1;
        g_lookups++;
    }
    printf("table %s: %zu ranges, %zu probes, %llu off the default, %llu dropped\n", name,
           t.lo.size(), probes.size(), (unsigned long long)in_range,
           (unsigned long long)dropped);
}

static int g_refused = 0;
static void expect_refused(const char* name, const gpuc_route_spec* s, const char* match) {
    std::string e = route_spec_error(s);
    CHECK(!e.empty(), "%s: malformed spec accepted", name);
    CHECK(e.find(match) != std::string::npos, "%s: message '%s' does not name '%s'", name,
          e.c_str(), match);
    if (!e.empty()) g_refused++;
}

int main() {
    // ---- lookups ----
    {
        Table t = table(1, 0);  // no range: everything is the default
        check_table("none", t);
        Table d = table(2, -1);
        check_table("none_drop", d);
    }
    {
        Table t = table(2, 1);
        t.add(-100, 100, 0);
        check_table("one", t);
        Table s = table(2, 0);
        s.add(7, 7, 1);  // single token
        check_table("one_single", s);
        Table w = table(2, -1);
        w.add(INT64_MIN, INT64_MAX, 1);  // the whole ring
        check_table("one_whole", w);
    }
    {
        Table t = table(3, 2);
        t.add(INT64_MIN, -5, 0);
        t.add(-4, INT64_MAX, 1);  // adjacent, both extremes
        check_table("two_extremes", t);
        Table u = table(3, 0);
        u.add(INT64_MIN, INT64_MIN, 2);
        u.add(INT64_MAX, INT64_MAX, -1);  // single tokens at the extremes, one dropped
        check_table("two_singles", u);
    }
    for (int variant = 0; variant < 3; variant++) {
        // about 1000 ranges over the whole ring: widths from single tokens to
        // wide, gaps of 0 (adjacent, lo[i+1] == hi[i] + 1) and more, -1 outputs
        Table t = table(5, variant == 1 ? -1 : 3);
        const int N = 1000 + variant;
        const uint64_t step = UINT64_MAX / (uint64_t)N;
        int64_t cur = INT64_MIN;  // next free token
        for (int i = 0; i < N; i++) {
            const bool last = i == N - 1;
            uint64_t r = rng();
            uint64_t gap = (i == 0 && variant != 2) ? 0 : (r % 4 == 0 ? 0 : (r >> 8) % (step / 4));
            uint64_t width = (r >> 3) % 5 == 0 ? 0 : (r >> 20) % (step / 2);
            int64_t l = (int64_t)((uint64_t)cur + gap);
            int64_t h = (int64_t)((uint64_t)l + width);
            if (last && variant != 2) h = INT64_MAX;
            int32_t o = (r >> 40) % 7 == 0 ? -1 : (int32_t)((r >> 44) % 5);
            t.add(l, h, o);
            if (h == INT64_MAX) break;
            cur = h + 1;
        }
        if (variant != 2) {
            CHECK(t.lo.front() == INT64_MIN, "first range must start at INT64_MIN");
            CHECK(t.hi.back() == INT64_MAX, "last range must end at INT64_MAX");
        }
        size_t adjacent = 0, single = 0, drop = 0;
        for (size_t i = 0; i < t.lo.size(); i++) {
            single += t.lo[i] == t.hi[i];
            drop += t.out[i] == -1;
            if (i + 1 < t.lo.size()) adjacent += t.lo[i + 1] == t.hi[i] + 1;
        }
        CHECK(adjacent > 50 && single > 50 && drop > 50,
              "generated table lacks cases: %zu adjacent, %zu single, %zu dropped", adjacent,
              single, drop);
        std::string nm = "many" + std::to_string(variant);
        check_table(nm.c_str(), t);
    }

    // ---- malformed specs ----
    {
        const int64_t lo[] = {0, 20, 40}, hi[] = {10, 30, 50};
        const int32_t out[] = {0, 1, -1};
        const char* b3[] = {"/o/a", "/o/b", "/o/c"};
        const gpuc_route_spec good{3, b3, 3, lo, hi, out, 2};
        CHECK(route_spec_error(&good).empty(), "good spec refused: %s",
              route_spec_error(&good).c_str());
        expect_refused("null_spec", nullptr, "NULL");
        gpuc_route_spec s = good;
        s.output_bases = nullptr;
        expect_refused("null_bases", &s, "output_bases");
        s = good; s.range_lo = nullptr;
        expect_refused("null_lo", &s, "range_lo");
        s = good; s.range_hi = nullptr;
        expect_refused("null_hi", &s, "range_hi");
        s = good; s.range_output = nullptr;
        expect_refused("null_out", &s, "range_output");
        s = good; s.n_outputs = 0;
        expect_refused("no_outputs", &s, "n_outputs");
        s = good; s.n_outputs = 33;  // checked before output_bases[3..] is read
        expect_refused("too_many_outputs", &s, "33");
        const char* bnull[] = {"/o/a", nullptr, "/o/c"};
        s = good; s.output_bases = bnull;
        expect_refused("null_base", &s, "base 1");
        const char* bempty[] = {"/o/a", "/o/b", ""};
        s = good; s.output_bases = bempty;
        expect_refused("empty_base", &s, "base 2");
        const char* bdup[] = {"/o/a", "/o/b", "/o/a"};
        s = good; s.output_bases = bdup;
        expect_refused("equal_bases", &s, "0 and 2");
        const int64_t lo_gt[] = {0, 31, 40};
        s = good; s.range_lo = lo_gt;
        expect_refused("lo_above_hi", &s, "range 1");
        const int64_t lo_touch[] = {0, 20, 30};
        s = good; s.range_lo = lo_touch;  // hi[1] == lo[2]
        expect_refused("touching", &s, "range 2");
        const int64_t lo_unord[] = {0, 5, 40};
        s = good; s.range_lo = lo_unord;  // hi[0] > lo[1]
        expect_refused("overlapping", &s, "range 1");
        const int32_t out_hi[] = {0, 3, -1};
        s = good; s.range_output = out_hi;
        expect_refused("output_too_high", &s, "range 1");
        const int32_t out_lo[] = {0, 1, -2};
        s = good; s.range_output = out_lo;
        expect_refused("output_too_low", &s, "range 2");
        s = good; s.default_output = 3;
        expect_refused("default_too_high", &s, "default_output");
        s = good; s.default_output = -2;
        expect_refused("default_too_low", &s, "default_output");
        // no ranges: the three arrays may be NULL
        s = good; s.n_ranges = 0; s.range_lo = s.range_hi = nullptr; s.range_output = nullptr;
        CHECK(route_spec_error(&s).empty(), "rangeless spec with NULL arrays refused");
    }
    printf("%d malformed specs refused\n", g_refused);
    printf("%llu lookups checked\n", (unsigned long long)g_lookups);
    if (g_fail) {
        printf("FAILED route_spec (%d)\n", g_fail);
        return 1;
    }
    printf("OK route_spec\n");
    return 0;
}
