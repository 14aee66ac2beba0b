// PRODUCT — host-only output components of an sstable: Statistics.db,
// Summary.db, CompressionInfo.db, Filter.db, Digest.crc32, TOC.txt, the `da`
// Partitions.db/Rows.db pair and the file writers. Every function here works
// on plain host buffers and is spec'd identically in oracle/src/sstable.cpp,
// so GPU and oracle outputs are byte-identical. No HIP here: gpucompact.cpp
// includes it, and tests/native/sstable_out_test.cpp builds it with a plain
// host compiler.
#pragma once
#include "codec.h"
#include "bti_core.h"
#include "sstable_meta.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <fcntl.h>
#include <unistd.h>
#include <vector>

namespace gpuc {

// ---------------------------------------------------------------------------
// host byte helpers
// ---------------------------------------------------------------------------
inline void put_be16(bytes& o, uint16_t v) { o.push_back(v >> 8); o.push_back((uint8_t)v); }
inline void put_be32(bytes& o, uint32_t v) { for (int i = 3; i >= 0; i--) o.push_back((uint8_t)(v >> (8 * i))); }
inline void put_be64(bytes& o, uint64_t v) { for (int i = 7; i >= 0; i--) o.push_back((uint8_t)(v >> (8 * i))); }
inline void put_uvint(bytes& o, uint64_t v) {
    uint8_t tmp[9];
    int n = uvint_put(tmp, v);
    o.insert(o.end(), tmp, tmp + n);
}
inline void put_type_str(bytes& o, const std::string& s) {
    put_uvint(o, s.size());
    o.insert(o.end(), s.begin(), s.end());
}

// ---------------------------------------------------------------------------
// file writers
// ---------------------------------------------------------------------------
inline void write_file(const std::string& path, const uint8_t* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot create " + path);
    if (n && fwrite(p, 1, n, f) != n) { fclose(f); throw std::runtime_error("short write " + path); }
    fclose(f);
}
inline void write_file(const std::string& path, const bytes& b) { write_file(path, b.data(), b.size()); }
inline void write_file(const std::string& path, const std::string& s) {
    write_file(path, (const uint8_t*)s.data(), s.size());
}
// threaded pwrite of p[0, len) into an existing file at file_off
// (page-cache pwrites peak at ~4 threads: tools/wbench.c matrix)
inline void pwrite_range(const std::string& path, const uint8_t* p, size_t len, uint64_t file_off,
                         int nthreads) {
    std::vector<std::thread> th;
    size_t per = (len + nthreads - 1) / nthreads;
    for (int t = 0; t < nthreads; t++) {
        size_t o = (size_t)t * per;
        if (o >= len) break;
        size_t part = std::min(per, len - o);
        th.emplace_back([&path, p, file_off, o, part]() {
            int fd = open(path.c_str(), O_WRONLY);
            if (fd < 0) return;
            size_t done = 0;
            while (done < part) {
                ssize_t w = pwrite(fd, p + o + done, part - done, (off_t)(file_off + o + done));
                if (w <= 0) break;
                done += (size_t)w;
            }
            close(fd);
        });
    }
    for (auto& x : th) x.join();
}
inline void write_file_parallel(const std::string& path, const uint8_t* p, size_t n, int nthreads = 4) {
    // create + size, then threaded pwrite
    write_file(path, nullptr, 0);
    if (n == 0) return;
    if (truncate(path.c_str(), (off_t)n) != 0) throw std::runtime_error("truncate " + path);
    pwrite_range(path, p, n, 0, nthreads);
}

// ---------------------------------------------------------------------------
// Statistics.db
// ---------------------------------------------------------------------------
inline std::vector<int64_t> est_hist_offsets(int size) {
    std::vector<int64_t> off;
    int64_t last = 1;
    off.push_back(1);
    for (int i = 1; i < size; i++) {
        int64_t next = (int64_t)llround((double)last * 1.2);
        if (next == last) next++;
        off.push_back(next);
        last = next;
    }
    return off;
}
inline void put_est_hist(bytes& o, const std::vector<int64_t>& off, const uint64_t* buckets) {
    put_be32(o, (uint32_t)(off.size() + 1));
    for (size_t i = 0; i < off.size() + 1; i++) {
        put_be64(o, (uint64_t)off[i == 0 ? 0 : i - 1]);
        put_be64(o, buckets[i]);
    }
}
// HyperLogLogPlus(13, 25) of the partition-key hash2_64 values (clearspring
// stream-lib; MetadataCollector.java:180-183). SPARSE while under the
// 0.75*m threshold with no flagged (low-bits-zero) key: (h >>> 39) << 1,
// delta varints over the sorted set — this encoding byte-reproduces the
// reference's own oa fixtures (oracle test_compaction_hll_fixture_pin).
// NORMAL otherwise: 2^13 five-bit registers, six per big-endian 32-bit word.
inline bytes hll_bytes(const std::vector<uint64_t>& key_hashes) {
    constexpr int P = 13, SP = 25;
    bytes h;
    put_be32(h, (uint32_t)-2);
    auto pv = [&](uint32_t v) { while (v >= 0x80) { h.push_back((uint8_t)(v | 0x80)); v >>= 7; } h.push_back((uint8_t)v); };
    pv(P); pv(SP);
    std::set<uint32_t> sparse;
    bool flagged = false;
    const uint32_t threshold = (uint32_t)((1u << P) * 3 / 4);
    for (uint64_t kh : key_hashes) {
        uint32_t sidx = (uint32_t)(kh >> (64 - SP));
        if ((sidx & ((1u << (SP - P)) - 1)) == 0) { flagged = true; break; }
        sparse.insert(sidx << 1);
        if (sparse.size() > threshold) break;
    }
    if (!flagged && sparse.size() <= threshold && key_hashes.size() <= threshold) {
        pv(1 /*SPARSE*/);
        pv((uint32_t)sparse.size());
        uint32_t prev = 0;
        for (uint32_t v : sparse) { pv(v - prev); prev = v; }
    } else {
        pv(0 /*NORMAL*/);
        std::vector<uint8_t> regs(1u << P, 0);
        for (uint64_t kh : key_hashes) {
            uint32_t idx = (uint32_t)(kh >> (64 - P));
            uint64_t w = (kh << P) | (1ull << (P - 1));
            uint8_t rho = (uint8_t)(__builtin_clzll(w) + 1);
            if (rho > regs[idx]) regs[idx] = rho;
        }
        uint32_t bits = (1u << P) / 6;
        uint32_t reg_ints = (bits % 32 == 0) ? bits : bits + 1;  // RegisterSet.getSizeForCount
        std::vector<uint32_t> M(reg_ints, 0);
        for (uint32_t i = 0; i < (1u << P); i++)
            M[i / 6] |= (uint32_t)regs[i] << (5 * (i % 6));
        pv(reg_ints * 4);
        for (uint32_t wv : M) put_be32(h, wv);
    }
    bytes o;
    put_be32(o, (uint32_t)h.size());
    o.insert(o.end(), h.begin(), h.end());
    return o;
}

struct OutMeta {
    // header of the output sstable: EncodingStats bases (written as deltas)
    int64_t hdr_min_ts, hdr_min_ldt;
    int32_t hdr_min_ttl;
    TableTypes types;
    // collected stats
    int64_t min_timestamp, max_timestamp, min_ldt, max_ldt;
    int32_t min_ttl, max_ttl;
    uint64_t total_rows, total_cells;
    bool has_partition_deletions;
    bytes first_key, last_key;
    std::map<uint32_t, uint32_t> tomb_hist;
    double compression_ratio;
    uint64_t part_size_hist[156];
    uint64_t cells_hist[119];
    std::vector<uint64_t> key_hashes;  // hash2_64 per kept partition (HLL)
};

inline bytes serialize_statistics_out(const OutMeta& m) {
    bytes validation;
    {
        std::string pn = "org.apache.cassandra.dht.Murmur3Partitioner";
        put_be16(validation, (uint16_t)pn.size());
        validation.insert(validation.end(), pn.begin(), pn.end());
        uint64_t fp;
        double fpv = 0.01;
        memcpy(&fp, &fpv, 8);
        put_be64(validation, fp);
    }
    bytes compaction = hll_bytes(m.key_hashes);
    const std::vector<std::string>& ck_types = m.types.clustering_types;
    bytes stats;
    {
        static const std::vector<int64_t> ps_off = est_hist_offsets(155);
        static const std::vector<int64_t> ch_off = est_hist_offsets(118);
        put_est_hist(stats, ps_off, m.part_size_hist);
        put_est_hist(stats, ch_off, m.cells_hist);
        put_be64(stats, (uint64_t)-1LL); put_be32(stats, 0);  // commitLogUpperBound NONE
        put_be64(stats, (uint64_t)m.min_timestamp);
        put_be64(stats, (uint64_t)m.max_timestamp);
        put_be32(stats, ldt_u32(m.min_ldt));
        put_be32(stats, ldt_u32(m.max_ldt));
        put_be32(stats, (uint32_t)m.min_ttl);
        put_be32(stats, (uint32_t)m.max_ttl);
        uint64_t cr; double crv = m.compression_ratio; memcpy(&cr, &crv, 8); put_be64(stats, cr);
        put_be32(stats, 100);  // TombstoneHistogram maxBinSize
        put_be32(stats, (uint32_t)m.tomb_hist.size());
        for (auto& [pt, cnt] : m.tomb_hist) { put_be64(stats, pt); put_be32(stats, cnt); }
        put_be32(stats, 0);               // sstableLevel
        put_be64(stats, 0);               // repairedAt
        // improvedMinMax: clustering type list + covered Slice (spec'd with the
        // oracle: BOTTOM..TOP bounds, no values)
        put_uvint(stats, ck_types.size());
        for (auto& t : ck_types) put_type_str(stats, t);
        stats.push_back(1); put_be16(stats, 0);  // Slice start: INCL_START, 0 values
        stats.push_back(6); put_be16(stats, 0);  // Slice end: INCL_END, 0 values
        stats.push_back(0);               // hasLegacyCounterShards
        put_be64(stats, m.total_cells);
        put_be64(stats, m.total_rows);
        put_be64(stats, (uint64_t)-1LL); put_be32(stats, 0);  // commitLogLowerBound NONE
        put_be32(stats, 0);               // commitLogIntervals empty
        stats.push_back(0);               // pendingRepair null
        stats.push_back(0);               // isTransient
        stats.push_back(0);               // originatingHostId null
        stats.push_back(m.has_partition_deletions ? 1 : 0);
        put_uvint(stats, m.first_key.size());
        stats.insert(stats.end(), m.first_key.begin(), m.first_key.end());
        put_uvint(stats, m.last_key.size());
        stats.insert(stats.end(), m.last_key.begin(), m.last_key.end());
        uint64_t ts; double tsc = 0.0; memcpy(&ts, &tsc, 8); put_be64(stats, ts);
    }
    bytes header;
    {
        put_uvint(header, (uint64_t)(m.hdr_min_ts - TIMESTAMP_EPOCH));
        put_uvint(header, sext32(m.hdr_min_ldt - DELETION_TIME_EPOCH));
        put_uvint(header, sext32(m.hdr_min_ttl));
        put_type_str(header, m.types.key_type);
        put_uvint(header, ck_types.size());
        for (auto& t : ck_types) put_type_str(header, t);
        for (auto* cols : {&m.types.static_cols, &m.types.regular_cols}) {
            put_uvint(header, cols->size());
            for (auto& [name, t] : *cols) {
                put_uvint(header, name.size());
                header.insert(header.end(), name.begin(), name.end());
                put_type_str(header, t);
            }
        }
    }
    const bytes* comps[4] = {&validation, &compaction, &stats, &header};
    bytes out;
    uint32_t crc = 0;
    auto crc_int = [](uint32_t c, uint32_t v) {
        uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v};
        return crc32_update_bitwise(c, b, 4);
    };
    put_be32(out, 4);
    crc = crc_int(0, 4);
    put_be32(out, crc);
    uint32_t pos = 4 + 8 * 4 + 2 * 4;
    for (int i = 0; i < 4; i++) {
        put_be32(out, i);
        crc = crc_int(crc, i);
        put_be32(out, pos);
        crc = crc_int(crc, pos);
        pos += comps[i]->size() + 4;
    }
    put_be32(out, crc);
    for (int i = 0; i < 4; i++) {
        out.insert(out.end(), comps[i]->begin(), comps[i]->end());
        put_be32(out, crc32_update_bitwise(0, comps[i]->data(), comps[i]->size()));
    }
    return out;
}

// ---------------------------------------------------------------------------
// Filter.db, CompressionInfo.db, Digest.crc32, TOC.txt
// ---------------------------------------------------------------------------
// bloom spec for fp=0.01 (BloomCalculations; identical table in the oracle)
struct HBloomSpec { int k; int buckets; };
inline HBloomSpec bloom_spec_001() { return {5, 10}; }  // computeBloomSpec(20, 0.01)

inline bytes filter_db(int hash_count, const std::vector<uint8_t>& bloom_words) {
    bytes f;
    put_be32(f, (uint32_t)hash_count);
    put_be32(f, (uint32_t)(bloom_words.size() / 8));
    f.insert(f.end(), bloom_words.begin(), bloom_words.end());
    return f;
}

// chunk_sizes: compressed payload bytes per chunk (each is followed by its
// 4-byte CRC in Data.db)
inline bytes compression_info_db(bool snappy, uint32_t chunk_len, uint64_t total_unc,
                                 const std::vector<uint32_t>& chunk_sizes) {
    bytes ci;
    std::string algo = snappy ? "SnappyCompressor" : "LZ4Compressor";
    put_be16(ci, (uint16_t)algo.size());
    ci.insert(ci.end(), algo.begin(), algo.end());
    put_be32(ci, 0);
    put_be32(ci, chunk_len);
    put_be32(ci, 0x7FFFFFFF);
    put_be64(ci, total_unc);
    put_be32(ci, (uint32_t)chunk_sizes.size());
    uint64_t acc = 0;
    for (size_t i = 0; i < chunk_sizes.size(); i++) { put_be64(ci, acc + (uint64_t)i * 4); acc += chunk_sizes[i]; }
    return ci;
}

// Digest = CRC of the whole Data.db, folded from the per-chunk payload CRCs
// (CRC concatenation is associative over (crc, len)); each chunk contributes
// its payload and the 4 big-endian bytes of its own CRC.
inline uint32_t fold_digest(const std::vector<uint32_t>& chunk_crcs,
                            const std::vector<uint32_t>& chunk_sizes) {
    static const Crc32Combiner comb;
    const uint32_t n_chunks = (uint32_t)chunk_crcs.size();
    int nth = n_chunks > 4096 ? 16 : 1;
    std::vector<uint32_t> pcrc(nth, 0);
    std::vector<uint64_t> plen(nth, 0);
    uint32_t per = (n_chunks + nth - 1) / nth;
    std::vector<std::thread> th;
    for (int t = 0; t < nth; t++) {
        th.emplace_back([&, t]() {
            uint32_t c0 = t * per, c1 = std::min(n_chunks, (t + 1) * per);
            uint32_t d = 0;
            uint64_t l = 0;
            for (uint32_t c = c0; c < c1; c++) {
                d = comb.combine(d, chunk_crcs[c], chunk_sizes[c]);
                uint8_t cb[4] = {(uint8_t)(chunk_crcs[c] >> 24), (uint8_t)(chunk_crcs[c] >> 16),
                                 (uint8_t)(chunk_crcs[c] >> 8), (uint8_t)chunk_crcs[c]};
                d = comb.combine(d, crc32_update_bitwise(0, cb, 4), 4);
                l += chunk_sizes[c] + 4;
            }
            pcrc[t] = d;
            plen[t] = l;
        });
    }
    for (auto& x : th) x.join();
    uint32_t dg = 0;
    for (int t = 0; t < nth; t++) dg = comb.combine(dg, pcrc[t], plen[t]);
    return dg;
}
inline std::string digest_text(uint32_t digest) { return std::to_string(digest); }

inline std::string toc_text(bool bti) {
    return bti ? "Data.db\nStatistics.db\nDigest.crc32\nTOC.txt\nCompressionInfo.db\nFilter.db\nPartitions.db\nRows.db\n"
               : "Data.db\nStatistics.db\nDigest.crc32\nTOC.txt\nCompressionInfo.db\nFilter.db\nIndex.db\nSummary.db\n";
}

// ---------------------------------------------------------------------------
// Summary.db from the Index.db image
// ---------------------------------------------------------------------------
// IndexSummary at BASE_SAMPLING_LEVEL (IndexSummaryBuilder with empty
// Downsampling start points: entries for keys 0, 128, 256, ...), serialized
// per IndexSummary.IndexSummarySerializer.serialize — BE header, then the
// off-heap image in NATIVE (LE) order: rebased int offsets, then key bytes +
// LE u64 Index.db position; trailing first/last key with BE lengths
// (SSTableReader.saveSummary). Fixture-pinned by the oracle roundtrip of all
// four legacy_oa tables.
inline bytes summary_db(const uint8_t* idx, uint64_t idx_len) {
    const uint32_t MIN_INTERVAL = 128;
    bytes entries, s;
    std::vector<uint32_t> offs;
    const uint8_t *first_k = nullptr, *last_k = nullptr;
    uint32_t first_kl = 0, last_kl = 0;
    uint64_t q = 0, part_i = 0;
    while (q < idx_len) {
        uint64_t entry_off = q;
        uint32_t klen = ((uint32_t)idx[q] << 8) | idx[q + 1];
        const uint8_t* kp = idx + q + 2;
        q += 2 + klen;
        if (!first_k) { first_k = kp; first_kl = klen; }
        last_k = kp; last_kl = klen;
        if (part_i % MIN_INTERVAL == 0) {
            offs.push_back((uint32_t)entries.size());
            entries.insert(entries.end(), kp, kp + klen);
            for (int b = 0; b < 8; b++) entries.push_back((uint8_t)(entry_off >> (8 * b)));
        }
        // skip position + promoted-index payload vints
        (void)uvint_get(idx, &q);
        q += uvint_get(idx, &q);
        part_i++;
    }
    uint32_t cnt = (uint32_t)offs.size();
    put_be32(s, MIN_INTERVAL);
    put_be32(s, cnt);
    put_be64(s, 4ull * cnt + entries.size());
    put_be32(s, 128);
    put_be32(s, cnt);
    for (uint32_t o : offs) {
        uint32_t v = o + 4 * cnt;
        for (int b = 0; b < 4; b++) s.push_back((uint8_t)(v >> (8 * b)));
    }
    s.insert(s.end(), entries.begin(), entries.end());
    if (first_k) {
        put_be32(s, first_kl);
        s.insert(s.end(), first_k, first_k + first_kl);
        put_be32(s, last_kl);
        s.insert(s.end(), last_k, last_k + last_kl);
    }
    return s;
}

// ---------------------------------------------------------------------------
// BTI (`da`) index post-pass: Partitions.db + Rows.db built on the host
// from the big-format Index.db IMAGE the writer kernels already produced
// (the image carries keys, data positions and the promoted-index blocks —
// firstName/lastName clusterings, offsets, end-open markers — and those
// blocks ARE the bti row-index blocks: rowIndexBlockSize ==
// column_index_size, BtiFormatPartitionWriter.java:52). Byte layout pinned
// against the reference's legacy_da fixtures through the oracle
// (write_sstable(bti)) and the GPU parity suite.
// ---------------------------------------------------------------------------
inline void build_bti_from_index_image(const uint8_t* idx, uint64_t idx_len, uint64_t data_total,
                                       const std::vector<int32_t>& ck_w,
                                       bti::bytes* partitions_out, bti::bytes* rows_out) {
    uint64_t p = 0;
    bytes rows_file;
    std::vector<bti::BtiKeyEntry> pes;
    std::vector<bti::BtiRowIndexBlockSpec> pending_specs;
    std::vector<size_t> pending_idx;
    std::vector<uint64_t> part_positions;
    auto uvint = [&]() -> uint64_t { return uvint_get(idx, &p); };
    auto be_n = [&](int n) -> uint64_t {
        uint64_t v = 0;
        for (int i = 0; i < n; i++) v = (v << 8) | idx[p++];
        return v;
    };
    struct Blk {
        bytes first_bc, last_bc;
        uint64_t offset = 0;
        bool has_open = false;
        int64_t open_m = 0;
        uint32_t open_l = 0;
    };
    auto parse_prefix = [&]() -> bytes {
        uint8_t kind = idx[p++];
        uint32_t nv = kind != 4 ? (uint32_t)be_n(2) : (uint32_t)ck_w.size();
        std::vector<std::pair<const uint8_t*, uint32_t>> comps;
        std::vector<int32_t> widths;
        if (nv) {
            (void)uvint();  // 32-batch null header (0: all present)
            for (uint32_t c = 0; c < nv; c++) {
                uint32_t len = ck_w[c] > 0 ? (uint32_t)ck_w[c] : (uint32_t)uvint();
                comps.push_back({idx + p, len});
                widths.push_back(ck_w[c]);
                p += len;
            }
        }
        return bti::byte_comparable_clustering(comps, widths, kind);
    };
    while (p < idx_len) {
        uint32_t klen = (uint32_t)be_n(2);
        const uint8_t* key = idx + p;
        p += klen;
        uint64_t pos = uvint();
        uint64_t promoted = uvint();
        int64_t idxpos = ~(int64_t)pos;
        if (promoted > 0) {
            uint64_t pend = p + promoted;
            (void)uvint();  // headerLength
            bool pdel_live = idx[p] == 0x80;
            int64_t pdm = 0;
            uint32_t pdl = 0;
            if (pdel_live) {
                p += 1;
            } else {
                pdm = (int64_t)be_n(8);
                pdl = (uint32_t)be_n(4);
            }
            uint64_t nblocks = uvint();
            std::vector<Blk> blocks;
            for (uint64_t b = 0; b < nblocks; b++) {
                Blk bk;
                bk.first_bc = parse_prefix();
                bk.last_bc = parse_prefix();
                bk.offset = uvint();
                (void)uvint();  // zigzag (width - 64KiB), unused here
                bk.has_open = idx[p++] != 0;
                if (bk.has_open) {
                    if (idx[p] == 0x80) {
                        bk.has_open = false;
                        p += 1;
                    } else {
                        bk.open_m = (int64_t)be_n(8);
                        bk.open_l = (uint32_t)be_n(4);
                    }
                }
                blocks.push_back(std::move(bk));
            }
            p = pend;  // skip the block-offsets u32 table
            bti::BtiRowIndexBlockSpec spec;
            spec.partition_key.assign(key, key + klen);
            spec.data_pos = pos;
            spec.block_count = blocks.size();
            spec.pdel_live = pdel_live;
            spec.pdel_mfda = pdm;
            spec.pdel_ldt = pdl;
            bytes prev_sep, prev_max;
            for (size_t b = 0; b < blocks.size(); b++) {
                bytes bkey;
                if (b > 0) bkey = bti::bti_separator_gt(blocks[b - 1].last_bc, blocks[b].first_bc);
                bool has_od = b > 0 && blocks[b - 1].has_open;
                int ob = 1;
                while (blocks[b].offset >> (8 * ob - 1)) ob++;  // signed SizedInts
                bti::BtiRowIndexBlockSpec::Entry e;
                e.prefix = bkey;
                e.pb = ob | (has_od ? 8 : 0);
                for (int i = ob - 1; i >= 0; i--)
                    e.payload.push_back((uint8_t)(blocks[b].offset >> (8 * i)));
                if (has_od) {
                    for (int i = 7; i >= 0; i--)
                        e.payload.push_back((uint8_t)((uint64_t)blocks[b - 1].open_m >> (8 * i)));
                    for (int i = 3; i >= 0; i--)
                        e.payload.push_back((uint8_t)(blocks[b - 1].open_l >> (8 * i)));
                }
                spec.entries.push_back(std::move(e));
                prev_sep = bkey;
                prev_max = blocks[b].last_bc;
            }
            // final nudge entry; its payload (partition length - 1, the
            // END_OF_PARTITION byte's offset) is patched once the next
            // partition's position is known
            size_t cm = 0;
            while (cm < prev_max.size() && cm < prev_sep.size() && prev_max[cm] == prev_sep[cm]) cm++;
            bti::BtiRowIndexBlockSpec::Entry fin;
            fin.prefix = bti::bti_nudge(prev_max, cm);
            spec.entries.push_back(std::move(fin));
            pending_specs.push_back(std::move(spec));
            pending_idx.push_back(pes.size());
        }
        bti::BtiKeyEntry e;
        int64_t tok = murmur3_token(key, klen);
        e.byte_comparable = bti::bti_byte_comparable_m3(tok, bytes(key, key + klen));
        e.raw_key.assign(key, key + klen);
        uint64_t h2[2];
        murmur3_128(key, klen, 0, h2);
        e.hash_bits = (uint8_t)h2[1];  // DecoratedKey.filterHashLowerBits
        e.idxpos = idxpos;
        pes.push_back(std::move(e));
        part_positions.push_back(pos);
    }
    for (size_t i = 0; i < pending_specs.size(); i++) {
        auto& spec = pending_specs[i];
        size_t pi = pending_idx[i];
        uint64_t next_pos = pi + 1 < part_positions.size() ? part_positions[pi + 1] : data_total;
        uint64_t endoff = next_pos - spec.data_pos - 1;
        auto& fin = spec.entries.back();
        int ob = 1;
        while (endoff >> (8 * ob - 1)) ob++;
        fin.pb = ob;
        fin.payload.clear();
        for (int b = ob - 1; b >= 0; b--) fin.payload.push_back((uint8_t)(endoff >> (8 * b)));
        pes[pi].idxpos = (int64_t)bti::append_bti_row_index(rows_file, spec);
    }
    *partitions_out = bti::write_bti_partitions(pes);
    *rows_out = std::move(rows_file);
}

}  // namespace gpuc
