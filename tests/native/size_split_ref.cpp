// TEST TOOL — cut points of a size-capped (MaxSSTableSizeWriter) compaction.
//
//   size_split_ref <R_base> <max_output_bytes>
//
// R is the ORACLE's single-output result of a compaction job. The tool walks
// R's partitions in order and decides nothing but where a new sstable
// starts; the bytes of every output come from the unmodified oracle_tool
// (`compact ... shard=first_token:last_token`).
//
// THE RULE (stated here and next to k_size_cut, and nowhere else):
//
//   Before partition p is appended, a new sstable is started iff the current
//   sstable already holds at least one partition and its estimated on-disk
//   bytes exceed max_output_bytes
//   (CompactionAwareWriter.maybeSwitchWriter,
//    MaxSSTableSizeWriter.shouldSwitchWriterInCurrentLocation).
//   The estimate is the compressed size of the chunks already FLUSHED
//   (CompressedSequentialWriter.getEstimatedOnDiskBytesWritten returns
//   chunkOffset), and a chunk is flushed lazily, when the next byte arrives
//   at a full buffer (BufferedDataOutputStreamPlus.write / doFlush), not when
//   the buffer becomes full.
//
// With E the uncompressed bytes the sstable holds after its last appended
// partition, L the chunk length and csize[c] the compressed payload length of
// its chunk c:
//   flushed(E) = 0 if E == 0, else (E - 1) / L   (E == k*L leaves chunk k-1 unflushed)
//   est(E)     = sum over c < flushed(E) of (csize[c] + 4)     (+4: the chunk CRC)
//   cut after partition i  <=>  est(E_i) > max_output_bytes    (strictly)
//
// Prints one JSON line per output: first_token, last_token, partitions.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../oracle/src/sstable.h"

using namespace oracle;

static uint64_t flushed_chunks(uint64_t E, uint32_t L) { return E ? (E - 1) / L : 0; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <R_base> <max_output_bytes>\n", argv[0]);
        return 2;
    }
    try {
        SSTable R = read_sstable(argv[1]);
        const uint64_t cap = strtoull(argv[2], nullptr, 10);
        const uint32_t L = R.comp.chunk_len;
        for (auto& p : R.parts) p.set_token();
        bytes cur;                 // uncompressed bytes of the current output
        uint64_t est = 0;          // on-disk bytes of its flushed chunks
        uint64_t done = 0;         // chunks counted in est
        size_t first = 0, count = 0;
        auto emit = [&](size_t last) {
            printf("{\"first_token\": %lld, \"last_token\": %lld, \"partitions\": %zu}\n",
                   (long long)R.parts[first].token, (long long)R.parts[last].token, count);
        };
        for (size_t i = 0; i < R.parts.size(); i++) {
            if (count > 0 && est > cap) {
                emit(i - 1);
                cur.clear();
                est = 0;
                done = 0;
                first = i;
                count = 0;
            }
            bytes index_unused;
            serialize_partition(R.parts[i], R.header, cur, index_unused);
            count++;
            // chunks are compressed independently: add the newly flushed ones
            for (const uint64_t f = flushed_chunks(cur.size(), L); done < f; done++) {
                bytes one(cur.begin() + done * L, cur.begin() + (done + 1) * L);
                est += chunk_compress(one, R.comp).file.size();  // payload + 4-byte CRC
            }
        }
        if (count) emit(R.parts.size() - 1);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "size_split_ref: %s\n", e.what());
        return 1;
    }
}
