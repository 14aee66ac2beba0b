// CPU test of cassandra_amd/csrc/merkle_spec.h (host-only; plain g++, no HIP):
// the token -> leaf lookup that the leaf assignment kernel also runs, the host
// reducer, and the spec check of gpuc_validate_merkle.
//
//   merkle_spec_test <validate file>
//
// The file holds the oracle's validate records (token i64 BE + 32-byte hash),
// token-sorted. For every tree layout, lookup + reducer must equal an
// independent assignment that scans the leaves linearly with the interval
// test written out; every malformed spec must be refused with its tree or
// leaf index in the message.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../cassandra_amd/csrc/merkle_spec.h"

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

struct Trees {
    std::vector<int64_t> left;
    std::vector<uint32_t> begin{0};
    std::vector<int64_t> right;
    void add(int64_t l, std::vector<int64_t> rs) {
        left.push_back(l);
        right.insert(right.end(), rs.begin(), rs.end());
        begin.push_back((uint32_t)right.size());
    }
    gpuc_merkle_spec spec() const {
        return gpuc_merkle_spec{(uint32_t)left.size(), left.data(), begin.data(), right.data()};
    }
};

// independent of merkle_leaf_of: every leaf's (lo, hi] tested in turn
static int64_t linear_leaf(const Trees& t, int64_t token) {
    for (size_t tr = 0; tr < t.left.size(); tr++) {
        int64_t lo = t.left[tr];
        for (uint32_t i = t.begin[tr]; i < t.begin[tr + 1]; i++) {
            if (lo < token && token <= t.right[i]) return i;
            lo = t.right[i];
        }
    }
    return -1;
}

static uint64_t g_lookups = 0;
static void check_layout(const char* name, const Trees& t, const std::vector<int64_t>& tok,
                         const std::vector<uint8_t>& hash) {
    gpuc_merkle_spec s = t.spec();
    std::string e = merkle_spec_error(&s);
    CHECK(e.empty(), "%s: well-formed spec refused: %s", name, e.c_str());
    if (!e.empty()) return;
    const size_t nl = t.right.size();
    // the lookup on every record token and on every bound and its neighbours
    std::vector<int64_t> probes(tok);
    for (int64_t b : t.right) {
        probes.push_back(b);
        if (b > INT64_MIN) probes.push_back(b - 1);
        if (b < INT64_MAX) probes.push_back(b + 1);
    }
    for (int64_t b : t.left) {
        probes.push_back(b);
        if (b > INT64_MIN) probes.push_back(b - 1);
        if (b < INT64_MAX) probes.push_back(b + 1);
    }
    probes.push_back(INT64_MIN);
    probes.push_back(INT64_MAX);
    probes.push_back(0);
    probes.push_back(-1);
    for (int64_t p : probes) {
        int64_t got = merkle_leaf_of(s.tree_left, s.leaf_begin, s.leaf_right, s.n_trees, p);
        int64_t want = linear_leaf(t, p);
        CHECK(got == want, "%s: token %lld -> leaf %lld, linear scan says %lld", name,
              (long long)p, (long long)got, (long long)want);
        g_lookups++;
    }
    // the reducer against a linear-scan reduction
    std::vector<uint8_t> lh(nl * 32, 0), ref(nl * 32, 0);
    std::vector<uint64_t> lc(nl, 0), refc(nl, 0);
    uint64_t in_tree = merkle_reduce_host(s, tok.data(), hash.data(), tok.size(), lh.data(),
                                          lc.data());
    uint64_t ref_in = 0;
    for (size_t r = 0; r < tok.size(); r++) {
        int64_t leaf = linear_leaf(t, tok[r]);
        if (leaf < 0) continue;
        for (int b = 0; b < 32; b++) ref[leaf * 32 + b] ^= hash[r * 32 + b];
        refc[leaf]++;
        ref_in++;
    }
    CHECK(in_tree == ref_in, "%s: %llu records in trees, linear scan %llu", name,
          (unsigned long long)in_tree, (unsigned long long)ref_in);
    CHECK(lh == ref, "%s: leaf hashes differ from the linear-scan reduction", name);
    CHECK(lc == refc, "%s: leaf counts differ from the linear-scan reduction", name);
    printf("layout %-22s %zu trees %zu leaves, %llu of %zu records in trees\n", name,
           t.left.size(), nl, (unsigned long long)in_tree, tok.size());
}

static int g_errors = 0;
static void expect_error(const char* name, const gpuc_merkle_spec* s, const char* must_name) {
    std::string e = merkle_spec_error(s);
    CHECK(!e.empty(), "%s: malformed spec accepted", name);
    CHECK(e.find(must_name) != std::string::npos, "%s: message \"%s\" does not name \"%s\"",
          name, e.c_str(), must_name);
    g_errors++;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <validate file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> raw;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
    if (raw.size() % 40 || raw.size() < 40 * 400) {
        fprintf(stderr, "%s: %zu bytes is not >= 400 whole records\n", argv[1], raw.size());
        return 2;
    }
    const size_t n = raw.size() / 40;
    std::vector<int64_t> T(n);
    std::vector<uint8_t> H(n * 32);
    for (size_t r = 0; r < n; r++) {
        uint64_t v = 0;
        for (int b = 0; b < 8; b++) v = (v << 8) | raw[r * 40 + b];
        T[r] = (int64_t)v;
        memcpy(&H[r * 32], &raw[r * 40 + 8], 32);
    }
    for (size_t r = 1; r < n; r++)
        if (T[r] < T[r - 1]) { fprintf(stderr, "records are not token-sorted\n"); return 2; }

    {   // one leaf over the whole ring
        Trees t;
        t.add(INT64_MIN, {INT64_MAX});
        check_layout("one leaf", t, T, H);
    }
    {   // bounds equal to record tokens: a record ON a bound belongs to the left leaf
        Trees t;
        t.add(T[5], {T[6], T[7], T[100], T[101], T[n / 2], T[n - 2]});
        check_layout("bounds on tokens", t, T, H);
    }
    {   // INT64_MIN / INT64_MAX ends, splits on both sides of zero and at zero
        Trees t;
        t.add(INT64_MIN, {INT64_MIN + 1, -4611686018427387904LL, -1, 0, 1,
                          4611686018427387904LL, INT64_MAX - 1, INT64_MAX});
        check_layout("int64 ends", t, T, H);
    }
    {   // several trees with gaps; two trees that touch; a one-token tree
        Trees t;
        t.add(INT64_MIN, {T[10]});
        t.add(T[20], {T[30], T[31], T[40]});
        t.add(T[40], {T[50]});                  // touches the tree before it
        t.add(T[200] - 1, {T[200]});            // holds exactly one token
        t.add(T[n - 50], {T[n - 10], INT64_MAX});
        check_layout("trees with gaps", t, T, H);
    }
    {   // more leaves than records
        Trees t;
        std::vector<int64_t> rs;
        const int L = 4096;
        for (int i = 0; i < L; i++) {
            __int128 span = (__int128)INT64_MAX - (__int128)INT64_MIN;
            rs.push_back((int64_t)((__int128)INT64_MIN + span * (i + 1) / L));
        }
        t.add(INT64_MIN, rs);
        check_layout("4096 even leaves", t, T, H);
    }

    // ---- malformed specs: each refused, with the index named ----
    {
        Trees ok;
        ok.add(0, {10, 20});
        ok.add(30, {40});
        gpuc_merkle_spec s = ok.spec();
        CHECK(merkle_spec_error(&s).empty(), "base spec refused");

        expect_error("NULL spec", nullptr, "NULL");
        gpuc_merkle_spec b = s;
        b.tree_left = nullptr;
        expect_error("NULL tree_left", &b, "tree_left");
        b = s;
        b.leaf_begin = nullptr;
        expect_error("NULL leaf_begin", &b, "leaf_begin");
        b = s;
        b.leaf_right = nullptr;
        expect_error("NULL leaf_right", &b, "leaf_right");
        b = s;
        b.n_trees = 0;
        expect_error("no trees", &b, "n_trees");

        uint32_t begin_nz[] = {1, 2, 3};
        b = s;
        b.leaf_begin = begin_nz;
        expect_error("leaf_begin[0] != 0", &b, "leaf_begin[0]");
        uint32_t begin_empty[] = {0, 2, 2};  // tree 1 has no leaf
        b = s;
        b.leaf_begin = begin_empty;
        expect_error("empty tree", &b, "tree 1");
        uint32_t begin_back[] = {0, 2, 1};
        b = s;
        b.leaf_begin = begin_back;
        expect_error("leaf_begin decreasing", &b, "tree 1");

        int64_t left_hi[] = {10, 30};  // tree 0's first leaf (10) not above its left (10)
        b = s;
        b.tree_left = left_hi;
        expect_error("first leaf not above left", &b, "leaf 0");
        int64_t left_hi1[] = {0, 40};  // tree 1's first leaf is flat leaf 2
        b = s;
        b.tree_left = left_hi1;
        expect_error("first leaf of tree 1 not above left", &b, "leaf 2");
        int64_t right_eq[] = {10, 10, 40};
        b = s;
        b.leaf_right = right_eq;
        expect_error("leaf_right not ascending", &b, "leaf 1");
        int64_t left_overlap[] = {0, 19};  // tree 1 starts below tree 0's end (20)
        b = s;
        b.tree_left = left_overlap;
        expect_error("overlapping trees", &b, "tree 1");
        int64_t left_unordered[] = {30, 0};
        int64_t right_unordered[] = {40, 50, 10};
        b = s;
        b.tree_left = left_unordered;
        b.leaf_right = right_unordered;
        expect_error("unordered trees", &b, "tree 1");

        // 2^31 leaves: refused from leaf_begin alone, leaf_right is never read
        uint32_t begin_huge[] = {0, 0x80000000u};
        int64_t one_right[] = {10};
        gpuc_merkle_spec h{1, left_hi, begin_huge, one_right};
        expect_error("2^31 leaves", &h, "2147483648");
        uint32_t begin_max[] = {0, 0x7FFFFFFFu};  // the limit itself passes the count check
        gpuc_merkle_spec m{1, left_hi, begin_max, one_right};
        (void)m;  // (its leaf_right would have to hold 2^31 - 1 entries: not walked here)
    }

    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("OK merkle_spec: %llu lookups over %zu records, %d malformed specs refused\n",
           (unsigned long long)g_lookups, n, g_errors);
    return 0;
}
