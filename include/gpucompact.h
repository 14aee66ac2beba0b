/*
 * libcassandra_gpucompact — MI355X-native SSTable compaction, C ABI.
 *
 * Drop-in boundary: replaces the hot loop of CompactionTask.runMayThrow
 * (reference: src/java/org/apache/cassandra/db/compaction/CompactionTask.java:184-236)
 * — scanners + CompactionIterator + CompactionAwareWriter — for eligible
 * tables (big-format `oa`, Murmur3Partitioner, any partition key, up to 32
 * clustering columns of fixed (bigint/int/timestamp) or variable
 * (text/ascii/blob) width, each ascending or descending, including prefix
 * range-tombstone bounds, 1..63 regular and 1..63
 * static columns with cell subsets, LZ4 or Snappy chunk compression with any
 * power-of-two chunk_length_in_kb from 1 to 64 KiB — inputs of one job may
 * mix lengths; row, cell, partition and range tombstones all supported).
 * Chunk lengths above 64 KiB are GPUC_ERR_UNSUPPORTED (liblz4 leaves its
 * byU16 table at 65547 input bytes and snappy splits into several 64 KiB
 * fragments: different algorithms); a zero or non-power-of-two length in a
 * CompressionInfo.db is GPUC_ERR_FORMAT.
 *
 * Clustering types. A clustering column's type string is one of LongType,
 * Int32Type, TimestampType, UTF8Type, AsciiType, BytesType, or
 * org.apache.cassandra.db.marshal.ReversedType(T) with T one of those six: a
 * column declared CLUSTERING ORDER BY (... DESC). ReversedType reverses the
 * comparison of values, never the bound kinds, and serializes as T does
 * (ReversedType.valueLengthIfFixed delegates to its base type); the exact
 * string of the inputs goes into the output's HEADER and STATS components
 * unchanged, and all inputs of a job carry equal strings (one input ascending
 * and one descending over the same base type is refused). TimestampType is
 * also accepted as a simple regular or static column type. It is taken as an
 * 8-byte fixed-width value compared as a signed long:
 * TimestampType.valueLengthIfFixed() == 8 and compareCustom ==
 * LongType.compareLongs are recalled, not checked against the Java sources.
 * GPUC_ERR_UNSUPPORTED with the type string in the message: a nested
 * ReversedType(ReversedType(...)), ReversedType of any other inner type, any
 * other clustering type, and ReversedType as key type or as a regular or
 * static column type. A `da` (BTI) input, or `bti` output, of a table with a
 * descending clustering column is GPUC_ERR_UNSUPPORTED before any Data.db
 * byte is parsed: Rows.db keys are the byte-comparable form of the
 * clusterings, which ReversedType inverts. `da` tables without a descending
 * clustering column are unaffected. gpuc_flush_table takes the ReversedType
 * strings in ck_types and checks the unfiltereds of each partition under that
 * comparator: ascending rows under a descending type are an error.
 *
 * Collection columns. After its simple regular columns a table may have any
 * number of complex columns (simple + complex <= 63) of the types
 *   org.apache.cassandra.db.marshal.SetType(K)
 *   org.apache.cassandra.db.marshal.MapType(K,V)
 * K is BytesType, UTF8Type or AsciiType, whose cell paths order as unsigned
 * bytes (shorter first), or Int32Type, LongType or TimestampType, whose paths
 * order as Int32Type.compare / LongType.compareLongs do: the first byte
 * signed, the rest unsigned, which for paths of one width is numeric order
 * (TimestampType like LongType: recalled, as above). V is BytesType,
 * UTF8Type, AsciiType or FrozenType(...) with any inner text: all written as
 * vint length + bytes. A CellPath is vint length + bytes whatever K is. Type
 * strings nest; MapType(K,V) is split at its top-level comma. In a column
 * with int, bigint or timestamp keys a path that is not 4 resp. 8 bytes wide
 * (an empty one included), and in a set column a cell that carries a value,
 * is GPUC_ERR_FORMAT from compact, scrub and verify, never silently merged.
 * FrozenType(...) with any inner text is also a simple column type of regular
 * and static columns: variable width, sorted with the simple columns in
 * Columns order, compared as bytes in the Cells.reconcile tie-break, never a
 * clustering or key type. The header string form
 * org.apache.cassandra.db.marshal.FrozenType(inner) is recalled, not checked
 * against the Java sources. Still refused, with the full type string in the
 * message and with the return code each had before the types above were
 * accepted: a map with a fixed-width V (Int32Type, LongType, TimestampType:
 * the value would lose its length prefix); ListType(...), whose paths compare
 * as TimeUUIDType; FrozenType(...) as K, any other K or V, nested multi-cell
 * types, MapType(LongType,BytesType) alone among the pairings of an accepted
 * K and V (tests that predate these types pin its refusal; map<bigint,text>
 * and map<timestamp,blob> are accepted), complex static columns, complex columns in counter tables, and a
 * complex column before a simple one in the header.
 *
 * The inputs of one job may list different columns in their serialization
 * headers (sstables older than an ALTER TABLE ... ADD, flushes that held only
 * some columns). Each input is parsed under its own header; the output header
 * is the union of the compacting inputs' regular and static columns in
 * Columns order (simple columns by name, then complex columns by name; names
 * compare as unsigned bytes), as SerializationHeader.make builds it. Inputs
 * that all carry the same header keep it as it stands. Tombstone sources are
 * mapped into that union by name and add no column to it. The column limits
 * above apply to the union. GPUC_ERR_UNSUPPORTED, with the column named and
 * before any Data.db byte is parsed, when: a column name carries different
 * types in two inputs; key or clustering types differ between inputs;
 * headers differ and one of them is not in Columns order; a tombstone source
 * has a column that no compacting input has. A job carries no table metadata:
 * a dropped column's cells are not filtered by drop time, and the column stays
 * in the output header. The Java host above the seam
 * (strategies, CompactionManager, LifecycleTransaction, metrics) is
 * unchanged and binds these entry points via JNI/Panama.
 *
 * Inputs mirror what the loop consumes (CompactionTask.java:184-205):
 *   - input sstable component paths (format version `oa`)
 *   - merge params nowInSec/gcBefore (CompactionIterator.java:343-347)
 *   - purge info: token-interval -> min-timestamp table for overlapping
 *     non-compacting sources (CompactionController.getPurgeEvaluator,
 *     CompactionController.java:247-286); empty table == no overlaps
 *   - optional token-range restriction (CompactionManager.forceCompactionForTokenRange)
 * Outputs mirror what the loop produces (CompactionTask.java:206-282):
 *   - output sstable component files written under output_base (tmp names;
 *     the host renames/commits under its LifecycleTransaction)
 *   - the stats the task reports (bytes, partition/row counts, merge histogram)
 *
 * Threading: one call == one compaction task, synchronous; the host may run
 * several concurrently on different devices (concurrent_compactors).
 * All compute (decompress, decode, merge, reconcile, purge, serialize,
 * compress, CRC, bloom) runs on the GPU; the library fails with
 * GPUC_ERR_NO_GPU if no HIP device is available — there is no CPU fallback.
 */
#ifndef CASSANDRA_GPUCOMPACT_H
#define CASSANDRA_GPUCOMPACT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPUC_OK 0
#define GPUC_ERR_IO 1
#define GPUC_ERR_FORMAT 2        /* unparseable/unsupported component bytes */
#define GPUC_ERR_UNSUPPORTED 3   /* schema/feature outside current GPU scope */
#define GPUC_ERR_NO_GPU 4
#define GPUC_ERR_HIP 5
#define GPUC_ERR_INTERNAL 6
#define GPUC_ERR_CANCELLED 7     /* cancel_flag observed set (CompactionInterruptedException) */

typedef struct gpuc_purge_range {
    int64_t token_lo;   /* inclusive Murmur3 token bounds */
    int64_t token_hi;
    int64_t min_timestamp;
    /* optional bloom filter of the overlapping sstable (the raw Filter.db
       bit payload after its 8-byte header; little-endian words). When set,
       purge gating applies only to keys the bloom might contain — exactly
       CompactionController.getPurgeEvaluator's overlapIterator +
       BF.isPresent chain (CompactionController.java:247-286,308-329). NULL
       keeps the conservative interval-only behavior (never purges more than
       the JVM, may retain tombstones it would drop). */
    const uint32_t* bloom_bits;
    uint64_t bloom_bit_len;   /* number of bits (words*64 from Filter.db) */
    int32_t bloom_hash_count; /* Filter.db hash count */
} gpuc_purge_range;

typedef struct gpuc_job {
    /* input sstable path prefixes, e.g. "/data/ks/t-uuid/oa-12-big"
       (components resolved as "<base>-Data.db" etc.) */
    const char* const* input_bases;
    int32_t n_inputs;

    /* output path prefix; all component files are created as
       "<output_base>-<Component>" (host renames under its txn log) */
    const char* output_base;

    int64_t now_sec;            /* nowInSec */
    int64_t gc_before;          /* gcBefore seconds; INT64_MIN == gc nothing */
    int32_t never_purge;        /* NEVER_PURGE_TOMBSTONES / table option */
    int32_t enforce_strict_liveness;

    const gpuc_purge_range* overlaps;  /* may be NULL when n_overlaps == 0 */
    int32_t n_overlaps;

    int32_t has_token_range;    /* shard restriction (multi-GPU token sharding) */
    int64_t token_lo;           /* inclusive */
    int64_t token_hi;           /* inclusive */

    /* anticompaction split (CompactionManager.antiCompactGroup / RepairFinishedCompactionTask):
       keep only partitions whose token falls in one of these inclusive ranges
       (invert_ranges=1 keeps the complement). One anticompaction = two calls:
       ranges -> the repaired output, ranges+invert -> the unrepaired one.
       gpuc_compact_routed below writes all outputs of an anticompaction
       (three with transient replication) from ONE pass over the inputs. */
    const gpuc_purge_range* keep_ranges;  /* min_timestamp field unused */
    int32_t n_keep_ranges;
    int32_t invert_ranges;

    int32_t device;             /* HIP device ordinal */

    /* nodetool garbagecollect (CompactionIterator.GarbageSkipper): sstables
       whose tombstones/cells REMOVE shadowed data from the compacted inputs
       without being written out. cell_level_gc == TombstoneOption.CELL
       (overwritten cells also removed); 0 == TombstoneOption.ROW. */
    const char* const* tombstone_source_bases;
    int32_t n_tomb_sources;
    int32_t cell_level_gc;

    /* 0/1 = one output sstable. N>1: the job is split into N equal Murmur3
       token ranges; each produces its own complete output sstable
       (generation, generation+1, ...) — the UCS shard model / a splitting
       compaction writer. Two ranges are processed concurrently so front-phase
       kernels overlap the LDS-bound compressor. */
    int32_t n_output_shards;

    /* optional cooperative cancellation (CompactionIterator.isStopRequested,
       CompactionIterator.java:721-740): when non-NULL, polled between
       pipeline phases; a non-zero value aborts the task with
       GPUC_ERR_CANCELLED. Output files may be partially written — the host
       discards them exactly as it discards tmp files of an interrupted Java
       compaction (LifecycleTransaction abort). */
    const volatile int32_t* cancel_flag;

    /* chunk length of the output sstable(s) in BYTES (the table's current
       CompressionParams.chunk_length, as CompactionTask would pass it):
       a power of two, 1024..65536. 0 == the chunk length of input_bases[0]
       (what a compaction does when the params are unchanged). Applies to
       every shard of n_output_shards. Inputs may have any supported length,
       each its own. */
    uint32_t output_chunk_length;

    /* 0 == no size cap. Above 0 the output is split the way a Leveled
       compaction's MaxSSTableSizeWriter splits it (sstable_size_in_mb; also
       sstablesplit and --split-output): before a partition is appended, a new
       sstable is started iff the current one already holds at least one
       partition and its estimated on-disk bytes exceed max_output_bytes.
       The estimate is the compressed size (payload + 4-byte CRC) of the
       chunks already flushed, and a chunk is flushed when the next byte
       arrives at a full buffer (CompactionAwareWriter.maybeSwitchWriter,
       MaxSSTableSizeWriter.shouldSwitchWriterInCurrentLocation,
       CompressedSequentialWriter.getEstimatedOnDiskBytesWritten). Every
       output holds at least one partition; one partition larger than the cap
       is an output of its own. Outputs are named like shards: the generation
       of output_base, then +1, +2, ...; gpuc_result.n_outputs says how many.
       The front of the pipeline runs once over the whole job. Allowed with
       has_token_range, keep_ranges, overlaps, tombstone sources,
       output_chunk_length and `da` inputs; with n_output_shards > 1 it is
       GPUC_ERR_UNSUPPORTED (before any input byte is read). cancel_flag is
       also polled between outputs. */
    uint64_t max_output_bytes;
} gpuc_job;

typedef struct gpuc_result {
    uint64_t input_uncompressed_bytes;  /* ISSTableScanner.getLengthInBytes basis */
    uint64_t output_uncompressed_bytes;
    uint64_t output_compressed_bytes;   /* final Data.db size */
    uint64_t partitions_in;             /* summed over inputs (versions) */
    uint64_t partitions_out;
    uint64_t rows_in;
    uint64_t rows_out;
    uint64_t merged_counts[64];         /* merge-arity histogram (CompactionTask.java:258-273) */
    /* phase timings, milliseconds (GPU phases are HIP-event timed) */
    double ms_read_io, ms_h2d, ms_decompress, ms_parse, ms_merge, ms_reconcile,
           ms_serialize, ms_compress, ms_d2h, ms_write_io, ms_total;
    /* dominant kernel bookkeeping for the roofline report */
    char dominant_kernel[64];
    double dominant_kernel_ms;
    uint64_t dominant_kernel_launches;
    char error[256];
    uint32_t n_outputs;                 /* sstables written: 1, the shard count, or
                                           the outputs of a max_output_bytes split */
} gpuc_result;

/* One compaction task. Returns GPUC_OK or an error code (message in result->error). */
int gpuc_compact(const gpuc_job* job, gpuc_result* result);

/* One compaction routed into several sstables by token range
 * (CompactionManager.antiCompactGroup: one merge, a fully-repaired, a
 * transiently-repaired and an unrepaired writer chosen per partition by the
 * ranges its token falls in; CompactionAwareWriter.maybeSwitchWriter switching
 * data directories at disk-boundary tokens has the same shape). Merge,
 * reconcile, garbage-skip and purge run exactly as gpuc_compact runs them for
 * the job, ONCE; every surviving partition is then classified on the device
 * and the writer back end runs once per output.
 *
 * A token t goes to range_output[i] of the range with range_lo[i] <= t <=
 * range_hi[i] (both bounds inclusive, signed compares), else to
 * default_output; -1 drops the partition. Adjacent ranges may name the same
 * output and several ranges may share one; equal tokens with different keys
 * land together. Output o is byte-identical, in all component files, to what
 * gpuc_compact writes for the same job with keep_ranges == the ranges routed
 * to o (the default output: all ranges with invert_ranges). The serialization
 * header (SerializationHeader.make stats, the column union) comes from the
 * inputs and is the same for every output; statistics, bloom filter, Summary,
 * first/last key, histograms and the tombstone list are each output's own.
 *
 * An output that receives no kept partition creates NO file and reports
 * written == 0 — the reference's SSTableRewriter aborts a writer nothing was
 * appended to (recalled, not checked against the Java sources). This differs
 * on purpose from gpuc_compact, which writes one empty sstable when nothing is
 * kept.
 *
 * result: n_outputs is the number of outputs written; partitions_out,
 * rows_out, the byte counts and the ms_* writer phases are sums over the
 * outputs; partitions_in, rows_in and merged_counts are job-wide.
 * cancel_flag is also polled between outputs. job->output_base is ignored
 * and may be NULL. Accepted with has_token_range, overlaps (blooms included),
 * gc_before / never_purge, tombstone sources, output_chunk_length, Snappy,
 * `da` inputs and inputs with different headers.
 *
 * GPUC_ERR_UNSUPPORTED (message in result->error, naming the offending index
 * where one applies) before any device is probed or input byte read: a NULL
 * spec, or a NULL array with a non-zero count; n_outputs 0 or above 32; a
 * NULL or empty output base, or two equal ones; range_lo[i] > range_hi[i];
 * range_hi[i] >= range_lo[i+1]; a range_output or default_output outside
 * -1..n_outputs-1; job->n_keep_ranges > 0, n_output_shards > 1 or
 * max_output_bytes > 0. */
typedef struct gpuc_route_spec {
    uint32_t n_outputs;               /* 1..32 */
    const char* const* output_bases;  /* n_outputs path prefixes, pairwise different;
                                         job->output_base is ignored and may be NULL */
    uint32_t n_ranges;                /* may be 0 */
    const int64_t* range_lo;          /* INCLUSIVE, signed compares */
    const int64_t* range_hi;          /* INCLUSIVE; lo[i] <= hi[i], hi[i] < lo[i+1] */
    const int32_t* range_output;      /* per range: 0..n_outputs-1, or -1 == drop */
    int32_t default_output;           /* tokens in no range: 0..n_outputs-1, or -1 == drop */
} gpuc_route_spec;

typedef struct gpuc_route_output {
    uint32_t written;                 /* 0: no kept partition was routed here, no file created */
    uint64_t partitions, rows, uncompressed_bytes, compressed_bytes;
} gpuc_route_output;

int gpuc_compact_routed(const gpuc_job* job, const gpuc_route_spec* spec,
                        gpuc_result* result,
                        gpuc_route_output* outputs /* n_outputs entries; may be NULL */);

/* Synthetic sstable generation ON THE GPU using the product write path
 * (serialize+compress+index+bloom kernels — the flush-path seed).
 * Writes n_sstables sstables under dir as "oa-<first_generation+i>-big-*".
 * Spec fields mirror oracle/src/gen.h (the shared generator contract). */
typedef struct gpuc_gen_spec {
    uint64_t seed;
    uint32_t n_sstables;
    uint64_t rows_per_sstable;
    uint32_t overlap_pct;
    uint32_t value_len;
    uint32_t value_repeat_pct;
    uint32_t tombstone_pct;
    uint32_t partition_del_pct;
    uint32_t clustering_rows;   /* >0: wide partitions (LongType ck), this many rows each */
    uint32_t range_tomb_pct;    /* % of wide partitions with one range tombstone */
    uint32_t key_len;           /* partition key bytes, 8..255 (0 == 8); >8 appends salt bytes */
    uint32_t ck_text;           /* clustering values as UTF8 strings (variable width) */
    uint32_t ck_cols;           /* 0/1 = one clustering column; 2 = composite (bigint,bigint)
                                   with ck0-prefix range-tombstone bounds */
    uint32_t static_pct;        /* percent of wide partitions with a static row */
    uint32_t n_value_cols;      /* regular columns val0..valN-1 (0 == 1 column "val") */
    uint32_t col_missing_pct;   /* P(cell absent) per live row and column */
    int64_t base_ts;
    int64_t base_ldt;
    uint64_t first_generation;
    int32_t device;
    int32_t snappy;             /* 1: SnappyCompressor chunks (C3 shape) */
    uint32_t ttl_pct;           /* percent of live rows written with expiring
                                   liveness/cells (LivenessInfo.java:67,
                                   AbstractCell.java:53-76) */
    uint32_t complex_pct;       /* percent of live rows with cells in one complex
                                   column 'zm' map<blob,blob> (last regular column;
                                   ComplexColumnData.java:47) */
    uint32_t complex_del_pct;   /* percent of those rows also carrying a
                                   complexDeletion */
    int32_t bti;                /* 1: write the `da` (trie-indexed) component
                                   set (Partitions.db/Rows.db, BtiFormat.md) */
    int32_t counter;            /* 1: one CounterColumnType column with
                                   synthetic CounterContexts (CounterContext.java) */
    uint32_t chunk_length;      /* output chunk length in bytes, power of two
                                   1024..65536; 0 == 16 KiB */
} gpuc_gen_spec;

int gpuc_generate(const gpuc_gen_spec* spec, const char* dir, char* error, size_t error_len);

/* VALIDATION compaction (CompactionManager.doValidationCompaction +
 * repair/Validator.rowHash): merge + purge the inputs exactly as a
 * compaction would, then write per-partition repair digests — records of
 * (Murmur3 token, int64 BE) + 32-byte concat(murmur3_128(1000),
 * murmur3_128(2000)) hash (db/Digest.java:53-59) — to out_path instead of
 * an output sstable. The host feeds these to its MerkleTree
 * (Validator.add) itself; a repair over ranges, which wants the trees' leaf
 * hashes and not one record per partition, calls gpuc_validate_merkle below.
 * Uses the same gpuc_job fields (now/gcBefore/overlaps/has_token_range);
 * sharding/size-split/tombstone-source/keep-range modes are rejected. */
int gpuc_validate(const gpuc_job* job, const char* out_path, uint64_t* n_partitions,
                  char* error, size_t error_len);

/* VALIDATION compaction reduced to Merkle-tree leaves ON THE DEVICE
 * (Validator.add -> MerkleTree.Leaf.addHash): the same merge + purge + digest
 * as gpuc_validate, then every kept partition's 32-byte digest is XORed into
 * the leaf that holds its token. The host builds its MerkleTrees as it does
 * today (Validator.prepare / MerkleTree.init, its own midpoint arithmetic) and
 * passes only the leaf bounds; the library never splits a range. Wrapping
 * ranges are unwrapped by the host (Range.unwrap).
 *
 * Leaf i of tree t covers (prev, leaf_right[i]]: prev is tree_left[t] for the
 * tree's first leaf, leaf_right[i-1] otherwise; compares are signed 64-bit.
 * leaf_hash[i] is the XOR of the digests (the bytes gpuc_validate writes) of
 * the kept output partitions whose token lies in leaf i — equal tokens with
 * different keys share a leaf; a leaf without a partition is 32 zero bytes,
 * count 0. A partition in no tree is not validated: not digested, not counted
 * in *n_partitions. Purged partitions contribute nothing. has_token_range
 * intersects with the trees. The "XOR into the leaf, zeros when empty,
 * inner node = XOR of children" rule is the 4.0+ MerkleTree's as recalled;
 * Validator's sizeOfRange (logging only) is not produced.
 *
 * GPUC_ERR_UNSUPPORTED, with the tree or leaf index in the message and before
 * any device is probed or input byte read: a NULL spec or array; n_trees 0;
 * leaf_begin[0] != 0 or leaf_begin not strictly increasing (a tree has at
 * least one leaf); a tree's first leaf_right not above its tree_left;
 * leaf_right not strictly ascending within a tree; tree_left[t+1] below tree
 * t's last leaf_right; more than 2^31 - 1 leaves. Job modes are accepted and
 * rejected exactly as by gpuc_validate. */
typedef struct gpuc_merkle_spec {
    uint32_t n_trees;            /* repair ranges == MerkleTrees, ascending, disjoint */
    const int64_t* tree_left;    /* n_trees: EXCLUSIVE left token of each tree's range */
    const uint32_t* leaf_begin;  /* n_trees + 1 offsets into leaf_right; leaf_begin[0] == 0 */
    const int64_t* leaf_right;   /* INCLUSIVE right token of each leaf, in tree order;
                                    a tree's last entry is the right end of its range */
} gpuc_merkle_spec;

int gpuc_validate_merkle(const gpuc_job* job, const gpuc_merkle_spec* spec,
                         uint8_t* leaf_hash,         /* n_leaves * 32 bytes, out */
                         uint64_t* leaf_partitions,  /* n_leaves, out; may be NULL */
                         uint64_t* n_partitions,     /* partitions validated; may be NULL */
                         char* error, size_t error_len);

/* Memtable flush (the write-path seed): n unsorted UNIQUE-key rows ->
 * token-sorted on device -> one complete `oa` sstable under output_base.
 * Schema: `pk blob PRIMARY KEY, val blob`. values[i] == NULL makes row i a
 * row tombstone with local deletion time del_ldts[i] (else del_ldts ignored;
 * pass UINT32_MAX). Replaces the flush serialize/compress path of
 * Memtable.FlushablePartitionSet -> BigTableWriter. Always 16 KiB chunks. */
typedef struct gpuc_flush_rows {
    uint64_t n_rows;
    const uint8_t* const* keys;
    const uint16_t* key_lens;
    const int64_t* timestamps;
    const uint8_t* const* values;       /* NULL entry = row tombstone */
    const uint32_t* value_lens;
    const uint32_t* del_ldts;           /* UINT32_MAX = live */
} gpuc_flush_rows;

int gpuc_flush(const gpuc_flush_rows* rows, const char* output_base, int32_t device,
               char* error, size_t error_len);

/* ---- full-schema memtable flush ----------------------------------------
 * The real Memtable -> BigTableWriter path (Memtable.FlushablePartitionSet
 * -> SortedTablePartitionWriter): the caller hands over partitions in any
 * order (the engine token-sorts them on device, like gpuc_flush), each with
 * its partition deletion, optional static row, and its unfiltereds (rows +
 * range-tombstone markers) ALREADY in clustering order — exactly what a
 * memtable holds (reference memtables are sorted maps; flush iterates them
 * in order, Memtable.java getFlushSet). The engine validates the
 * within-partition order and key uniqueness and fails loudly on violations.
 *
 * Cell/row field conventions match the serialization they produce:
 * ldt is the u32 localDeletionTime encoding (GPUC_LDT_NONE = none), ttl 0 =
 * none, expiring cells carry ttl>0 + ldt = localExpirationTime. A cell with
 * flags bit HAS_VALUE cleared and ldt set is a cell tombstone. */
#define GPUC_LDT_NONE 0xFFFFFFFFu
#define GPUC_CELLF_PRESENT 1u   /* column set on this row */
#define GPUC_CELLF_HAS_VALUE 2u
#define GPUC_CELLF_EXPIRING 4u
#define GPUC_ROWF_HAS_ROW 1u    /* always set for rows */
#define GPUC_ROWF_LIVE_TS 2u    /* primaryKeyLivenessInfo present */
#define GPUC_ROWF_DELETED 4u    /* row deletion present */

typedef struct gpuc_cell {
    uint8_t flags;              /* GPUC_CELLF_*; 0 = column absent */
    int64_t ts;
    uint32_t ldt;               /* GPUC_LDT_NONE = live */
    int32_t ttl;                /* 0 = none */
    const uint8_t* value;
    uint32_t value_len;
} gpuc_cell;

typedef struct gpuc_cpx_cell {  /* one complex (collection) cell */
    gpuc_cell cell;
    const uint8_t* path;        /* CellPath: the map key bytes */
    uint32_t path_len;
} gpuc_cpx_cell;

typedef struct gpuc_cpx_col {   /* one complex column of one row */
    uint8_t present;            /* column set on this row */
    int64_t del_mfda;           /* complexDeletion (INT64_MIN = live) */
    uint32_t del_ldt;           /* GPUC_LDT_NONE = live */
    uint32_t n_cells;
    const gpuc_cpx_cell* cells; /* CellPath order */
} gpuc_cpx_col;

typedef struct gpuc_unfiltered {
    uint8_t kind;               /* ClusteringPrefix.Kind ordinal
                                 * (ClusteringPrefix.java:65-85): 4 = row,
                                 * 0/1/6/7 bounds, 2/5 boundaries */
    uint8_t ck_count;           /* clustering components present (rows: n_ck;
                                 * marker bounds may be shorter prefixes) */
    uint8_t row_flags;          /* GPUC_ROWF_* (rows only) */
    const uint8_t* const* ck;   /* per component: serialized value bytes */
    const uint32_t* ck_lens;
    int64_t live_ts;            /* with GPUC_ROWF_LIVE_TS */
    int32_t live_ttl;           /* >0 = ExpiringLivenessInfo */
    int64_t live_let;           /* localExpirationTime (long semantics) */
    int64_t del_mfda;           /* row deletion / marker close(or single) */
    uint32_t del_ldt;
    int64_t open_mfda;          /* boundary markers: open deletion */
    uint32_t open_ldt;
    const gpuc_cell* cells;     /* rows: schema->n_cols entries (the complex
                                 * columns' entries are ignored; see cpx_*) */
    /* legacy single-column form, read only while cpx_cols == NULL: */
    uint8_t has_cpx;            /* complex column present on this row */
    int64_t cpx_del_mfda;       /* complexDeletion */
    uint32_t cpx_del_ldt;
    uint32_t n_cpx_cells;
    const gpuc_cpx_cell* cpx_cells;  /* in CellPath order */
    /* non-NULL: schema->n_cpx entries in header order, and the five legacy
     * fields above are ignored. NULL: the legacy fields describe the one
     * complex column; with schema->n_cpx >= 2 a row with has_cpx set and
     * NULL cpx_cols is an error. Each column's paths must be strictly
     * increasing in CellPath order (unsigned bytes, shorter first). */
    const gpuc_cpx_col* cpx_cols;
} gpuc_unfiltered;

typedef struct gpuc_flush_part {
    const uint8_t* key;
    uint16_t key_len;
    int64_t pdel_mfda;          /* partition deletion (INT64_MIN = live) */
    uint32_t pdel_ldt;
    uint8_t static_flags;       /* GPUC_ROWF_*; 0 = no/empty static row */
    int64_t static_live_ts;
    int32_t static_live_ttl;
    int64_t static_live_let;
    int64_t static_del_mfda;
    uint32_t static_del_ldt;
    const gpuc_cell* static_cells;  /* schema->n_static entries when
                                     * static_flags != 0 */
    uint64_t n_unf;
    const gpuc_unfiltered* unf; /* clustering order */
} gpuc_flush_part;

typedef struct gpuc_flush_schema {
    /* AbstractType class names as the reference serializes them into the
     * Statistics.db HEADER (e.g. "org.apache.cassandra.db.marshal.LongType");
     * fixed widths are derived from the type (LongType 8, Int32Type 4,
     * otherwise variable). NULL key_type = BytesType. */
    const char* key_type;
    uint32_t n_ck;
    const char* const* ck_types;
    uint32_t n_cols;            /* regular columns, header order; the complex
                                 * (SetType / MapType) columns must be the
                                 * LAST n_cpx */
    const uint8_t* const* col_names;
    const uint32_t* col_name_lens;
    const char* const* col_types;
    uint32_t n_static;
    const uint8_t* const* static_names;
    const uint32_t* static_name_lens;
    const char* const* static_types;
    uint32_t n_cpx;             /* number of trailing complex columns (n_cols
                                 * <= 63). col_types takes the SetType(K) /
                                 * MapType(K,V) strings of the top comment,
                                 * and FrozenType(...) for a simple column.
                                 * Checked per column, the message naming it:
                                 * cells strictly ascending in the order of
                                 * K, paths 4 / 8 bytes wide under int /
                                 * bigint, timestamp keys, no value in a
                                 * set's cells */
    uint32_t column_index_size; /* 0 = 64 KiB */
    uint32_t snappy;            /* chunk codec for the output */
    uint32_t bti;               /* write the `da` (trie-indexed) components */
    /* header EncodingStats, as the reference's memtable hands its collected
     * stats to SerializationHeader.make; has_stats == 0 derives them from
     * the rows instead */
    uint8_t has_stats;
    int64_t stats_min_ts;
    int64_t stats_min_ldt;      /* long-seconds semantics */
    int32_t stats_min_ttl;
    uint32_t chunk_length;      /* output chunk length in bytes, power of two
                                 * 1024..65536; 0 == 16 KiB */
} gpuc_flush_schema;

int gpuc_flush_table(const gpuc_flush_schema* schema, const gpuc_flush_part* parts,
                     uint64_t n_partitions, const char* output_base, int32_t device,
                     char* error, size_t error_len);

/* Scrub one sstable (SortedTableScrubber): salvage every partition whose
 * byte range touches only CRC/decode-clean chunks and rewrite them as a clean
 * sstable under output_base, written at the INPUT's chunk length (recovery
 * granularity is the chunk — documented in DESIGN.md; identical to the
 * oracle's). kept/dropped may be NULL. */
int gpuc_scrub(const char* input_base, const char* output_base, int32_t device,
               uint64_t* kept, uint64_t* dropped, char* error, size_t error_len);

/* Verify one sstable (Verifier.java / sstableverify --extended semantics):
 * CompressionInfo frame walk, per-chunk CRC32, full row-format walk,
 * strict DecoratedKey order, Digest.crc32 recomputation, bloom-filter
 * rebuild compared against Filter.db. A `da` (trie-indexed) sstable takes
 * its partition positions from Partitions.db / Rows.db instead of Index.db.
 * GPUC_OK or GPUC_ERR_FORMAT with a message. */
int gpuc_verify(const char* input_base, int32_t device, char* error, size_t error_len);

/* Diagnostic: chunk-compress a host buffer exactly as the writer does (the
 * same kernel launches, not a copy) and return the Data.db image (per chunk:
 * payload, then BE CRC32) plus the CompressionInfo.db chunk offsets.
 * chunk_length: power of two 1024..65536 (0 == 16 KiB). */
int gpuc_compress_buffer(const uint8_t* data, uint64_t len, uint32_t chunk_length,
                         int32_t snappy, int32_t device, uint8_t* out, uint64_t out_cap,
                         uint64_t* out_len, uint64_t* offsets, uint32_t offsets_cap,
                         uint32_t* n_chunks, char* error, size_t error_len);

/* Diagnostic: where the size-split writer (gpuc_job.max_output_bytes) would
 * cut a stream of partitions, using the writer's own launches (chunk compress
 * + k_size_cut, not a copy). part_ends[i] is the exclusive end offset of
 * partition i in `data`, non-decreasing; an entry equal to its predecessor is
 * a dropped (zero-byte) partition, which never carries a cut. cut_after
 * receives the index of the last partition of every output but the final
 * one. chunk_length as in gpuc_compress_buffer; max_output_bytes > 0. */
int gpuc_plan_size_cuts(const uint8_t* data, uint64_t len,
                        const uint64_t* part_ends, uint64_t n_parts,
                        uint32_t chunk_length, int32_t snappy, uint64_t max_output_bytes,
                        int32_t device, uint64_t* cut_after, uint64_t cut_cap, uint64_t* n_cuts,
                        char* error, size_t error_len);

/* library/build identification */
const char* gpuc_version(void);
/* returns number of visible HIP devices (0 => gpuc_compact will fail) */
int gpuc_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* CASSANDRA_GPUCOMPACT_H */
