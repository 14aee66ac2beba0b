// PRODUCT — host-only code for gpuc_compact_routed's routing table
// (gpuc_route_spec, include/gpucompact.h): the spec check and the token ->
// output lookup. The lookup is GPUC_HD: the routing kernel (k_route_parts,
// kernels_rows.hip) and the plain-g++ native test
// (tests/native/route_spec_test.cpp) run the same function.
//
// Range i covers [range_lo[i], range_hi[i]], both ends inclusive; compares
// are signed. A checked spec has lo[i] <= hi[i] < lo[i+1], so range_hi is
// strictly ascending and one binary search finds the only candidate range.
// Repairs over vnodes hand over hundreds to thousands of ranges, hence no
// linear scan (token_kept's, for keep_ranges, stays as it is).
#pragma once
#include <stdint.h>
#include <string>

#include "codec.h"
#include "../../include/gpucompact.h"

namespace gpuc {

constexpr uint32_t ROUTE_MAX_OUTPUTS = 32;

// Output of `token`: range_output of the range that holds it, else
// default_output; -1 means drop. The arrays are a checked gpuc_route_spec's
// (host or device copies); n_ranges may be 0.
GPUC_HD inline int32_t route_output_of(const int64_t* lo, const int64_t* hi, const int32_t* out,
                                       uint32_t n_ranges, int32_t default_output,
                                       int64_t token) {
    // first range whose hi is >= token
    uint32_t a = 0, b = n_ranges;
    while (a < b) {
        uint32_t mid = a + ((b - a) >> 1);
        if (hi[mid] < token) a = mid + 1;
        else b = mid;
    }
    if (a < n_ranges && lo[a] <= token) return out[a];
    return default_output;
}

// Empty string when the spec is well formed, else the reason, naming the
// output or range index. Counts are checked before what they index is read.
inline std::string route_spec_error(const gpuc_route_spec* s) {
    if (!s) return "route spec is NULL";
    if (s->n_outputs == 0 || s->n_outputs > ROUTE_MAX_OUTPUTS)
        return "route spec: n_outputs is " + std::to_string(s->n_outputs) + ", must be 1.." +
               std::to_string(ROUTE_MAX_OUTPUTS);
    if (!s->output_bases) return "route spec: output_bases is NULL";
    if (s->n_ranges) {
        if (!s->range_lo) return "route spec: range_lo is NULL";
        if (!s->range_hi) return "route spec: range_hi is NULL";
        if (!s->range_output) return "route spec: range_output is NULL";
    }
    for (uint32_t o = 0; o < s->n_outputs; o++) {
        if (!s->output_bases[o] || !s->output_bases[o][0])
            return "route spec: output base " + std::to_string(o) + " is NULL or empty";
        for (uint32_t p = 0; p < o; p++)
            if (std::string(s->output_bases[p]) == s->output_bases[o])
                return "route spec: output bases " + std::to_string(p) + " and " +
                       std::to_string(o) + " are equal";
    }
    const int64_t n_out = (int64_t)s->n_outputs;
    if (s->default_output < -1 || s->default_output >= n_out)
        return "route spec: default_output " + std::to_string(s->default_output) +
               " is outside -1.." + std::to_string(n_out - 1);
    for (uint32_t i = 0; i < s->n_ranges; i++) {
        if (s->range_lo[i] > s->range_hi[i])
            return "route spec: range " + std::to_string(i) + " has lo above hi";
        if (i > 0 && s->range_hi[i - 1] >= s->range_lo[i])
            return "route spec: range " + std::to_string(i) +
                   " starts at or below the end of range " + std::to_string(i - 1) +
                   " (ranges must be ascending and disjoint)";
        if (s->range_output[i] < -1 || s->range_output[i] >= n_out)
            return "route spec: range_output of range " + std::to_string(i) + " is " +
                   std::to_string(s->range_output[i]) + ", outside -1.." +
                   std::to_string(n_out - 1);
    }
    return "";
}

}  // namespace gpuc
