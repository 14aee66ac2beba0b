// CPU mirror of snp_wave_compress (cassandra_amd/csrc/snappy_wave.h) as the
// kernel stands today, for inputs up to one 64 KiB fragment. It differs from
// snappy_sim.h (the original planning simulator, valid for 16 KiB chunks) in
// exactly the two places the kernel does:
//   * probe indices past the end of the offset table are treated as an
//     aborting probe (position ip_limit + 16, increment 1) instead of being
//     looked up — at 64 KiB the lanes behind the first aborting probe run off
//     the table, which a 16 KiB chunk never reaches;
//   * in-window duplicate groups come from hash equality between lanes (the
//     kernel's hash-bit ballots), not from an LDS marker round.
// Everything else (emit helpers, match length, copy loop) is the model's.
#pragma once
#include "../../cassandra_amd/csrc/snappy_model.h"
#include <cstring>
#include <vector>

namespace snpmirror {

constexpr int W = 64;

// same table the host uploads (gpucompact.cpp ensure_crc_tables)
inline const std::vector<uint32_t>& probe_offsets() {
    static const std::vector<uint32_t> t = [] {
        std::vector<uint32_t> off{0};
        uint32_t skip = 32, o = 0;
        while (o < (1u << 16) + 128) {
            uint32_t inc = skip >> 5;
            skip += inc;
            o += inc;
            off.push_back(o);
        }
        return off;
    }();
    return t;
}

inline int compress(const uint8_t* s, uint32_t n, uint8_t* dst, uint16_t* table,
                    uint32_t table_size) {
    using namespace gpuc;
    const auto& OFF = probe_offsets();
    const uint32_t off_n = (uint32_t)OFF.size();
    uint8_t* op = dst;
    {
        uint32_t v = n;
        while (v >= 0x80) { *op++ = (uint8_t)(v | 0x80); v >>= 7; }
        *op++ = (uint8_t)v;
    }
    memset(table, 0, table_size * sizeof(uint16_t));
    const int shift = 32 - __builtin_ctz(table_size);
    const int ip_limit = (int)n - (int)SNP_INPUT_MARGIN;
    int ip = 1, next_emit = 0;
    auto rd32 = [&](int p) { return snp_load32(s + p); };

    if ((int)n >= (int)SNP_INPUT_MARGIN) {
        while (true) {
            int match = -1;
            {
                uint32_t k0 = 0;
                const int S0 = ip;
                bool found = false, aborted = false;
                while (true) {
                    int p[W], cand[W];
                    uint32_t v[W], h[W], cv[W];
                    uint16_t t[W];
                    bool valid[W], m[W];
                    for (int l = 0; l < W; l++) {
                        uint32_t mi = k0 + (uint32_t)l;
                        p[l] = mi + 1 < off_n ? S0 + (int)OFF[mi] : ip_limit + 16;
                        int inc = mi + 1 < off_n ? (int)(OFF[mi + 1] - OFF[mi]) : 1;
                        valid[l] = p[l] + inc <= ip_limit;
                        v[l] = (p[l] >= 0 && p[l] + 4 <= (int)n) ? rd32(p[l]) : 0;
                        h[l] = snp_hash(v[l], shift);
                        t[l] = table[h[l]];
                    }
                    for (int l = 0; l < W; l++) {
                        int pred = -1;
                        for (int j = l - 1; j >= 0; j--)
                            if (h[j] == h[l]) { pred = j; break; }
                        cand[l] = pred >= 0 ? p[pred] : (int)t[l];
                        // the kernel loads the table candidate on valid lanes only
                        cv[l] = pred >= 0 ? v[pred] : (valid[l] ? rd32((int)t[l]) : 0);
                        m[l] = valid[l] && cv[l] == v[l];
                    }
                    int first_abort = W, first_event = W;
                    for (int l = 0; l < W; l++) if (!valid[l]) { first_abort = l; break; }
                    for (int l = 0; l < W; l++) if (m[l]) { first_event = l; break; }
                    bool have_match = first_event < first_abort && first_event < W;
                    int commit_hi = have_match ? first_event
                                               : (first_abort < W ? first_abort - 1 : W - 1);
                    for (int l = 0; l <= commit_hi; l++) table[h[l]] = (uint16_t)p[l];
                    if (have_match) {
                        ip = p[first_event];
                        match = cand[first_event];
                        found = true;
                    } else if (first_abort < W) {
                        aborted = true;
                    }
                    if (found || aborted) break;
                    k0 += W;
                }
                if (aborted) goto emit_remainder;
            }
            op = snp_emit_literal(op, s + next_emit, ip - next_emit);
            while (true) {
                int base = ip;
                int matched = 4 + snp_match_length(s + match + 4, s + ip + 4, s + n);
                ip += matched;
                op = snp_emit_copy(op, (size_t)(base - match), matched);
                next_emit = ip;
                if (ip >= ip_limit) goto emit_remainder;
                uint64_t input_bytes = snp_load64(s + ip - 1);
                table[snp_hash((uint32_t)input_bytes, shift)] = (uint16_t)(ip - 1);
                uint32_t cur_hash = snp_hash((uint32_t)(input_bytes >> 8), shift);
                int candidate = table[cur_hash];
                uint32_t candidate_bytes = rd32(candidate);
                table[cur_hash] = (uint16_t)ip;
                if ((uint32_t)(input_bytes >> 8) != candidate_bytes) break;
                match = candidate;
            }
            ip++;
        }
    }
emit_remainder:
    if (next_emit < (int)n) op = snp_emit_literal(op, s + next_emit, (int)n - next_emit);
    return (int)(op - dst);
}

}  // namespace snpmirror
