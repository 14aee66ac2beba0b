/* Pure-C consumer of the libcassandra_gpucompact C ABI — demonstrates the
 * drop-in boundary (include/gpucompact.h) without C++ or Python. The Java
 * side would bind the same symbols via Panama FFI.
 *
 *   gpuc_cli compact <out_base> [chunk=<bytes>] [--max-output-bytes N] <in_base> [<in_base> ...]
 *       chunk=: output chunk length (power of two, 1024..65536); default is
 *       the chunk length of the first input
 *       --max-output-bytes N: start a new output sstable (generation of
 *       out_base, +1, +2, ...) once the estimated on-disk size exceeds N
 *       (MaxSSTableSizeWriter); prints the number of outputs
 *   gpuc_cli anticompact <full_base> <transient_base> <unrepaired_base> full=lo:hi,... [trans=lo:hi,...] <in_base> [<in_base> ...]
 *       one anticompaction in one call (gpuc_compact_routed): partitions whose
 *       token lies in a full= range (both bounds inclusive) go to full_base,
 *       those in a trans= range to transient_base, the rest to
 *       unrepaired_base; an output that receives nothing creates no file
 *   gpuc_cli verify  <base>
 *   gpuc_cli scrub   <out_base> <in_base>
 */
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../include/gpucompact.h"

/* "lo:hi,lo:hi,..." appended to lo/hi/out as ranges of output `o`; returns
 * the new count, or -1 on a malformed list or more than cap ranges */
static int parse_ranges(const char* s, int32_t o, int64_t* lo, int64_t* hi, int32_t* out,
                        int n, int cap) {
    while (*s) {
        char* e;
        if (n >= cap) return -1;
        lo[n] = strtoll(s, &e, 10);
        if (e == s || *e != ':') return -1;
        s = e + 1;
        hi[n] = strtoll(s, &e, 10);
        if (e == s || (*e != ',' && *e != 0)) return -1;
        out[n++] = o;
        s = *e ? e + 1 : e;
    }
    return n;
}

int main(int argc, char** argv) {
    char err[256] = {0};
    if (argc < 3) {
        fprintf(stderr, "usage: %s compact|anticompact|verify|scrub ...\n", argv[0]);
        return 2;
    }
    printf("%s | devices: %d\n", gpuc_version(), gpuc_device_count());
    if (!strcmp(argv[1], "verify")) {
        int rc = gpuc_verify(argv[2], 0, err, sizeof err);
        printf("verify rc=%d %s\n", rc, err);
        return rc;
    }
    if (!strcmp(argv[1], "scrub")) {
        uint64_t kept = 0, dropped = 0;
        int rc = gpuc_scrub(argv[3], argv[2], 0, &kept, &dropped, err, sizeof err);
        printf("scrub rc=%d kept=%llu dropped=%llu %s\n", rc,
               (unsigned long long)kept, (unsigned long long)dropped, err);
        return rc;
    }
    if (!strcmp(argv[1], "compact")) {
        const char* ins[64];
        int first = 3;
        uint32_t out_chunk = 0;
        if (argc > 3 && !strncmp(argv[3], "chunk=", 6)) {
            out_chunk = (uint32_t)strtoul(argv[3] + 6, NULL, 10);
            first = 4;
        }
        uint64_t max_out = 0;
        if (argc > first + 1 && !strcmp(argv[first], "--max-output-bytes")) {
            max_out = strtoull(argv[first + 1], NULL, 10);
            first += 2;
        }
        int k = argc - first;
        if (k < 1 || k > 64) { fprintf(stderr, "1..64 inputs\n"); return 2; }
        for (int i = 0; i < k; i++) ins[i] = argv[first + i];
        gpuc_job job;
        memset(&job, 0, sizeof job);
        job.input_bases = ins;
        job.n_inputs = (uint32_t)k;
        job.output_base = argv[2];
        job.gc_before = INT64_MIN;
        job.never_purge = 1;
        job.output_chunk_length = out_chunk;
        job.max_output_bytes = max_out;
        gpuc_result res;
        memset(&res, 0, sizeof res);
        int rc = gpuc_compact(&job, &res);
        printf("compact rc=%d in=%llu B out_parts=%llu rows=%llu outputs=%u %s\n", rc,
               (unsigned long long)res.input_uncompressed_bytes,
               (unsigned long long)res.partitions_out,
               (unsigned long long)res.rows_out, res.n_outputs, res.error);
        return rc;
    }
    if (!strcmp(argv[1], "anticompact")) {
        enum { MAXR = 4096 };
        static int64_t lo[MAXR], hi[MAXR];
        static int32_t out[MAXR];
        const char* ins[64];
        int n = 0, first = 6;
        if (argc < 7 || strncmp(argv[5], "full=", 5)) {
            fprintf(stderr, "usage: %s anticompact <full_base> <transient_base> <unrepaired_base> "
                            "full=lo:hi,... [trans=lo:hi,...] <in_base>...\n", argv[0]);
            return 2;
        }
        n = parse_ranges(argv[5] + 5, 0, lo, hi, out, n, MAXR);
        if (n >= 0 && !strncmp(argv[6], "trans=", 6)) {
            n = parse_ranges(argv[6] + 6, 1, lo, hi, out, n, MAXR);
            first = 7;
        }
        if (n < 0) { fprintf(stderr, "bad range list (lo:hi,..., at most %d)\n", MAXR); return 2; }
        /* one ascending table (insertion sort by lo); the library refuses overlaps */
        for (int i = 1; i < n; i++)
            for (int j = i; j > 0 && lo[j - 1] > lo[j]; j--) {
                int64_t t = lo[j]; lo[j] = lo[j - 1]; lo[j - 1] = t;
                t = hi[j]; hi[j] = hi[j - 1]; hi[j - 1] = t;
                int32_t u = out[j]; out[j] = out[j - 1]; out[j - 1] = u;
            }
        int k = argc - first;
        if (k < 1 || k > 64) { fprintf(stderr, "1..64 inputs\n"); return 2; }
        for (int i = 0; i < k; i++) ins[i] = argv[first + i];
        const char* bases[3] = {argv[2], argv[3], argv[4]};
        gpuc_job job;
        memset(&job, 0, sizeof job);
        job.input_bases = ins;
        job.n_inputs = k;
        job.gc_before = INT64_MIN;
        job.never_purge = 1;
        gpuc_route_spec spec;
        memset(&spec, 0, sizeof spec);
        spec.n_outputs = 3;
        spec.output_bases = bases;
        spec.n_ranges = (uint32_t)n;
        spec.range_lo = lo;
        spec.range_hi = hi;
        spec.range_output = out;
        spec.default_output = 2;
        gpuc_result res;
        gpuc_route_output ro[3];
        memset(&res, 0, sizeof res);
        memset(ro, 0, sizeof ro);
        int rc = gpuc_compact_routed(&job, &spec, &res, ro);
        printf("anticompact rc=%d in=%llu B outputs=%u full=%llu transient=%llu unrepaired=%llu "
               "partitions %s\n", rc, (unsigned long long)res.input_uncompressed_bytes,
               res.n_outputs, (unsigned long long)ro[0].partitions,
               (unsigned long long)ro[1].partitions, (unsigned long long)ro[2].partitions,
               res.error);
        return rc;
    }
    fprintf(stderr, "unknown command %s\n", argv[1]);
    return 2;
}
