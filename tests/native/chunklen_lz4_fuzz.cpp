// CPU pin for chunk lengths up to 64 KiB: the scalar LZ4 model (lz4_model.h)
// and the wave-window simulator (lz4_sim.h) against the system liblz4, byte
// for byte, over the chunklen_cases.h sweep. 64 KiB is the last length of
// liblz4's byU16 regime (positions up to 65535 in the u16 table).
#include "lz4_sim.h"
#include "chunklen_cases.h"
#include "../../oracle/src/lz4_ref.h"
#include <cstdio>
#include <cstring>
#include <vector>

int main() {
    std::vector<uint8_t> src, ref, got;
    std::vector<uint16_t> table(LZ4M_HASHTABLESIZE_U16);
    int fails = 0, cases = 0;
    for (int mode = 0; mode < chunklen::N_MODES; mode++) {
        for (int idx = 0; idx < chunklen::n_cases_per_mode(); idx++) {
            int n = chunklen::case_length(mode, idx);
            chunklen::fill(src, n, mode, idx);
            int bound = LZ4_compressBound(n);
            ref.assign(bound, 0xAA);
            int ra = LZ4_compress_default((const char*)src.data(), (char*)ref.data(), n, bound);
            for (int which = 0; which < 2; which++) {
                got.assign(bound, 0xBB);
                memset(table.data(), 0, table.size() * 2);
                int rb = which == 0 ? lz4m_compress(src.data(), n, got.data(), table.data())
                                    : sim_compress(src.data(), n, got.data(), table.data());
                if (ra != rb || memcmp(ref.data(), got.data(), ra) != 0) {
                    int d = 0;
                    while (d < ra && d < rb && ref[d] == got[d]) d++;
                    printf("MISMATCH %s mode=%d n=%d ref=%d got=%d first_diff=%d\n",
                           which ? "sim" : "model", mode, n, ra, rb, d);
                    if (++fails > 4) return 1;
                }
                cases++;
            }
        }
    }
    printf(fails ? "chunklen lz4 FAILED (%d)\n" : "chunklen lz4 OK (%d cases, liblz4 %s)\n",
           fails ? fails : cases, LZ4_versionString());
    return fails ? 1 : 0;
}
