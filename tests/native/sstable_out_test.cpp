// CPU test of cassandra_amd/csrc/sstable_out.h: the host-only output component
// builders must regenerate the oracle's own bytes from what sstable_meta.h
// parses out of an oracle-written sstable. Plain host C++, no HIP.
//
// usage: sstable_out_test [wide=]<oa base> ... bti=<oa base>,<da base> ...
//   wide=  the input's Index.db must carry a promoted-index payload
//   bti=   the same table written as `oa` and as `da`
#include "../../cassandra_amd/csrc/sstable_out.h"

#include <cstdio>
#include <cstdlib>

using namespace gpuc;

static int g_checks = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        g_checks++;                                                            \
        if (!(cond)) {                                                         \
            fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);    \
            fprintf(stderr, __VA_ARGS__);                                      \
            fprintf(stderr, "\n");                                             \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static bytes slurp(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    bytes b;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}
static bytes of_text(const std::string& s) { return bytes(s.begin(), s.end()); }

static uint32_t crc32_of(const bytes& b) {
    uint32_t tab[256];
    crc32_make_table(tab);
    return crc32_update_t(0, b.data(), b.size(), tab);
}

// the fold's threaded branch (more than 4096 chunks) against a straight CRC
static void check_fold_threads() {
    const uint32_t n = 5000;
    bytes image;
    std::vector<uint32_t> crcs(n), sizes(n);
    uint64_t x = 12345;
    for (uint32_t c = 0; c < n; c++) {
        bytes payload(1 + splitmix64(c) % 61);
        for (auto& v : payload) { x = splitmix64(x); v = (uint8_t)x; }
        sizes[c] = (uint32_t)payload.size();
        crcs[c] = crc32_of(payload);
        image.insert(image.end(), payload.begin(), payload.end());
        put_be32(image, crcs[c]);
    }
    CHECK(fold_digest(crcs, sizes) == crc32_of(image), "threaded fold");
    CHECK(fold_digest({}, {}) == 0, "empty fold");
}

struct Table {
    std::string base;
    bytes data, index;
    HCompressionInfo ci;
    HStatistics st;
};

// the components every format has; returns the parsed table
static Table check_common(const std::string& base, bool bti) {
    const char* b = base.c_str();
    Table t;
    t.base = base;
    t.data = slurp(base + "-Data.db");
    bytes ci_b = slurp(base + "-CompressionInfo.db");
    t.ci = parse_compression_info(ci_b);
    t.st = parse_statistics(slurp(base + "-Statistics.db"));
    if (!bti) t.index = slurp(base + "-Index.db");

    // chunk sizes from the parsed offset table, CRC words from Data.db
    auto frames = chunk_frames(t.ci, t.data.size(), 0, t.ci.offsets.size());
    std::vector<uint32_t> sizes, crcs;
    for (auto& f : frames) {
        sizes.push_back(f.comp_len);
        const uint8_t* p = t.data.data() + f.off + f.comp_len;
        crcs.push_back(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]);
    }
    CHECK(!sizes.empty(), "%s: no chunks", b);
    CHECK(compression_info_db(t.ci.snappy, t.ci.chunk_len, t.ci.data_len, sizes) == ci_b,
          "%s: CompressionInfo.db", b);

    uint32_t digest = fold_digest(crcs, sizes);
    CHECK(digest == crc32_of(t.data), "%s: fold %u is not the CRC-32 of Data.db", b, digest);
    CHECK(of_text(digest_text(digest)) == slurp(base + "-Digest.crc32"), "%s: Digest.crc32", b);

    CHECK(of_text(toc_text(bti)) == slurp(base + "-TOC.txt"), "%s: TOC.txt", b);

    bytes filter = slurp(base + "-Filter.db");
    HReader r(filter);
    uint32_t k = r.be32(), words = r.be32();
    CHECK(filter.size() == 8 + (size_t)words * 8, "%s: Filter.db length", b);
    CHECK(filter_db((int)k, bytes(filter.begin() + 8, filter.end())) == filter, "%s: Filter.db", b);
    CHECK((int)k == bloom_spec_001().k, "%s: bloom hash count %u", b, k);
    return t;
}

// largest promoted-index payload and the number of entries of an Index.db
static void index_shape(const Table& t, uint64_t* entries, uint64_t* max_promoted) {
    HReader r(t.index);
    *entries = *max_promoted = 0;
    while (r.pos < r.len) {
        r.skip(r.be16());
        r.uvint();
        uint64_t promoted = r.uvint();
        r.skip(promoted);
        *max_promoted = std::max(*max_promoted, promoted);
        ++*entries;
    }
}

static Table check_oa(const std::string& base, bool wide) {
    Table t = check_common(base, false);
    uint64_t entries, max_promoted;
    index_shape(t, &entries, &max_promoted);
    CHECK(!wide || max_promoted > 0, "%s: no promoted index in a wide table", base.c_str());
    bytes want = slurp(base + "-Summary.db");
    CHECK(summary_db(t.index.data(), t.index.size()) == want, "%s: Summary.db", base.c_str());
    // one Summary entry per 128 partitions
    HReader r(want);
    r.be32();
    CHECK(r.be32() == (entries + 127) / 128, "%s: Summary.db entry count", base.c_str());
    printf("%s: %llu partitions, promoted index up to %llu bytes, %zu chunks\n", base.c_str(),
           (unsigned long long)entries, (unsigned long long)max_promoted, t.ci.offsets.size());
    return t;
}

static void check_bti_pair(const std::string& oa_base, const std::string& da_base, bool wide) {
    Table oa = check_oa(oa_base, wide);
    Table da = check_common(da_base, true);
    CHECK(oa.data == da.data, "%s / %s: Data.db differs between the formats", oa_base.c_str(),
          da_base.c_str());
    std::vector<int32_t> ckw;
    for (auto& ct : oa.st.clustering_types) ckw.push_back(ck_type_width(ct));
    bti::bytes parts, rows;
    build_bti_from_index_image(oa.index.data(), oa.index.size(), oa.ci.data_len, ckw, &parts, &rows);
    bytes want_rows = slurp(da_base + "-Rows.db");
    CHECK(parts == slurp(da_base + "-Partitions.db"), "%s: Partitions.db", da_base.c_str());
    CHECK(rows == want_rows, "%s: Rows.db", da_base.c_str());
    CHECK(!wide || !want_rows.empty(), "%s: no row index in a wide table", da_base.c_str());
}

int main(int argc, char** argv) {
    check_fold_threads();
    int n_oa = 0, n_pairs = 0;
    for (int a = 1; a < argc; a++) {
        std::string arg = argv[a];
        bool wide = arg.compare(0, 5, "wide=") == 0;
        if (wide) arg = arg.substr(5);
        if (arg.compare(0, 4, "bti=") == 0) {
            size_t comma = arg.find(',');
            CHECK(comma != std::string::npos, "argument %s", argv[a]);
            check_bti_pair(arg.substr(4, comma - 4), arg.substr(comma + 1), wide);
            n_pairs++;
        } else {
            check_oa(arg, wide);
            n_oa++;
        }
    }
    CHECK(n_oa + n_pairs > 0, "no inputs");
    printf("OK %d checks over %d tables and %d oa/da pairs\n", g_checks, n_oa, n_pairs);
    return 0;
}
