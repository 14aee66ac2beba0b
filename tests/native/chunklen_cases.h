// Shared case sweep for the chunk-length fuzzers (chunklen_lz4_fuzz.cpp,
// chunklen_snappy_fuzz.cpp): the eight content modes of lz4_wave_sim.cpp over
// every length at which a codec can change behaviour between 1 byte and one
// 64 KiB chunk, plus random lengths up to 64 KiB.
#pragma once
#include <cstdint>
#include <vector>

namespace chunklen {

inline uint64_t sm(uint64_t x) {
    x += 0x9E3779B97f4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

constexpr int N_MODES = 8;

// fixed lengths: tiny / LZ4 MFLIMIT edge (12, 13) / around 4 KiB / the three
// large power-of-two chunks / the last u16 position (65535, 65536)
inline const std::vector<int>& fixed_lengths() {
    static const std::vector<int> v{1, 12, 13, 4095, 4096, 4097, 16384, 32768, 65535, 65536};
    return v;
}
constexpr int N_RANDOM = 6;  // random lengths per mode, 1..65536

inline int case_length(int mode, int idx) {
    const auto& f = fixed_lengths();
    if (idx < (int)f.size()) return f[idx];
    return 1 + (int)(sm(0xC0FFEEull + mode * 131 + idx) % 65536);
}
inline int n_cases_per_mode() { return (int)fixed_lengths().size() + N_RANDOM; }

inline void fill(std::vector<uint8_t>& src, int n, int mode, int idx) {
    uint64_t seed = (uint64_t)mode * 1000 + idx;
    src.resize(n);
    for (int i = 0; i < n; i++) {
        uint64_t r = sm(seed * 1315423911ULL + (uint64_t)(i / 8));
        switch (mode) {
            case 0: src[i] = (uint8_t)sm(seed + i); break;                          // random
            case 1: src[i] = 0; break;                                              // zeros
            case 2: src[i] = (uint8_t)(r >> (8 * (i % 8))); break;                  // random qwords
            case 3: src[i] = (i % 3) ? (uint8_t)('a' + (i % 17)) : (uint8_t)sm(seed + i); break;
            case 4: src[i] = (uint8_t)('a' + (sm(seed + i / 4) % 26)); break;       // 4-byte runs
            case 5: src[i] = (i % 512 == 0) ? (uint8_t)sm(seed + i) : 0x42; break;  // sparse change
            case 6: src[i] = (uint8_t)((i / 100) & 0xFF); break;                    // 100-byte runs
            default: src[i] = (uint8_t)(sm(seed + i) % 4); break;                   // 2-bit alphabet
        }
    }
}

}  // namespace chunklen
