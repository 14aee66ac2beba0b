// CPU pin for chunk lengths up to 64 KiB (one snappy fragment), over the
// chunklen_cases.h sweep, byte for byte:
//   * snappy_model.h vs the system libsnappy (skipped with "nolib" as argv[1]
//     where the library is absent);
//   * the wave-window decompositions vs that model: snappy_wave_mirror.h (the
//     kernel's control flow as it stands) at every length, and the original
//     snappy_sim.h at the lengths it was written for (<= 16 KiB: behind its
//     first aborting probe it indexes the probe-offset table without a bound,
//     which only a longer input can run off).
#include "snappy_sim.h"
#include "snappy_wave_mirror.h"
#include "chunklen_cases.h"
#include "../../oracle/src/snappy_ref.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    using namespace gpuc;
    const bool have_lib = !(argc > 1 && !strcmp(argv[1], "nolib"));
    std::vector<uint8_t> src;
    std::vector<uint16_t> ta(SNP_MAX_TABLE), tb(SNP_MAX_TABLE);
    int fails = 0, cases = 0;
    auto differ = [&](const char* what, int mode, int n, const std::vector<uint8_t>& a, size_t la,
                      const std::vector<uint8_t>& b, size_t lb) {
        if (la == lb && memcmp(a.data(), b.data(), la) == 0) return;
        size_t d = 0;
        while (d < std::min(la, lb) && a[d] == b[d]) d++;
        printf("MISMATCH %s mode=%d n=%d want=%zu got=%zu first_diff=%zu\n", what, mode, n, la, lb, d);
        fails++;
    };
    for (int mode = 0; mode < chunklen::N_MODES && fails <= 4; mode++) {
        for (int idx = 0; idx < chunklen::n_cases_per_mode() && fails <= 4; idx++) {
            int n = chunklen::case_length(mode, idx);
            chunklen::fill(src, n, mode, idx);
            const size_t cap = 32 + (size_t)n + n / 6 + 16;  // snappy MaxCompressedLength + slack
            std::vector<uint8_t> model(cap), got(cap);
            uint32_t ts = snp_table_size((uint32_t)n);
            int lm = snp_compress(src.data(), (uint32_t)n, model.data(), ta.data(), ts);
            if (have_lib) {
                std::vector<uint8_t> ref(snappy_ref_max_compressed_length(n));
                size_t ref_len = ref.size();
                if (!snappy_ref_compress((const char*)src.data(), n, (char*)ref.data(), &ref_len)) {
                    printf("libsnappy compress failed\n");
                    return 2;
                }
                differ("model-vs-libsnappy", mode, n, ref, ref_len, model, (size_t)lm);
                cases++;
            }
            int lw = snpmirror::compress(src.data(), (uint32_t)n, got.data(), tb.data(), ts);
            differ("mirror-vs-model", mode, n, model, (size_t)lm, got, (size_t)lw);
            cases++;
            if (n <= 16384) {
                int ls = snp_sim_compress(src.data(), (uint32_t)n, got.data(), tb.data(), ts);
                differ("sim-vs-model", mode, n, model, (size_t)lm, got, (size_t)ls);
                cases++;
            }
        }
    }
    printf(fails ? "chunklen snappy FAILED (%d)\n" : "chunklen snappy OK (%d cases%s)\n",
           fails ? fails : cases, have_lib ? "" : ", libsnappy leg skipped");
    return fails ? 1 : 0;
}
