// PRODUCT — host-only input metadata of an sstable: CompressionInfo.db,
// Statistics.db and Index.db parsing, chunk framing and schema resolution.
// No HIP here: gpucompact.cpp includes it, and tests/native/sstable_meta_test.cpp
// builds it with a plain host compiler.
#pragma once
#include "codec.h"

#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace gpuc {

using bytes = std::vector<uint8_t>;

// bounds-checked big-endian reader; invariant: pos <= len
struct HReader {
    const uint8_t* p;
    size_t len, pos = 0;
    explicit HReader(const bytes& b) : p(b.data()), len(b.size()) {}
    void need(size_t n) const { if (n > len - pos) throw std::runtime_error("short read in component"); }
    void seek(size_t at) { if (at > len) throw std::runtime_error("short read in component"); pos = at; }
    uint8_t u8() { need(1); return p[pos++]; }
    uint16_t be16() { need(2); uint16_t v = ((uint16_t)p[pos] << 8) | p[pos + 1]; pos += 2; return v; }
    uint32_t be32() { need(4); uint32_t v = 0; for (int i = 0; i < 4; i++) v = (v << 8) | p[pos + i]; pos += 4; return v; }
    uint64_t be64() { need(8); uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[pos + i]; pos += 8; return v; }
    bytes take(size_t n) { need(n); bytes b(p + pos, p + pos + n); pos += n; return b; }
    void skip(size_t n) { need(n); pos += n; }
    uint64_t uvint() {
        need(1);
        // length from the first byte's leading ones, checked before the read
        uint8_t inv = (uint8_t)~p[pos];
        size_t extra = inv ? (size_t)__builtin_clz((uint32_t)inv) - 24 : 8;
        if (extra > len - pos - 1) throw std::runtime_error("vint overrun");
        uint64_t q = pos;
        uint64_t v = uvint_get(p, &q);
        pos = q;
        return v;
    }
};

// typed failures the C ABI maps to GPUC_ERR_UNSUPPORTED / GPUC_ERR_FORMAT
struct unsupported_error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct format_error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
static const char* const CHUNK_LEN_WHY =
    " (supported: powers of two from 1 KiB to 64 KiB; above 64 KiB liblz4 leaves its byU16 "
    "table and snappy splits into several 64 KiB fragments)";
// a chunk length handed in as an ARGUMENT (0 == caller's default)
inline uint32_t checked_chunk_len_arg(uint32_t len, uint32_t dflt) {
    if (len == 0) return dflt;
    if (!chunk_len_supported(len))
        throw unsupported_error("unsupported chunk_length " + std::to_string(len) + CHUNK_LEN_WHY);
    return len;
}

struct HCompressionInfo {
    uint32_t chunk_len = 16384;
    uint32_t max_compressed = 0x7FFFFFFF;
    uint64_t data_len = 0;
    bool snappy = false;  // SnappyCompressor (else LZ4Compressor)
    std::vector<uint64_t> offsets;
    // decoder sanity bound for this input's frames (codec.h)
    uint32_t max_comp() const { return snappy ? snp_max_comp(chunk_len) : lz4_max_comp(chunk_len); }
};
inline HCompressionInfo parse_compression_info(const bytes& b) {
    HReader r(b);
    uint16_t nlen = r.be16();
    bytes name = r.take(nlen);
    std::string algo((char*)name.data(), name.size());
    if (algo != "LZ4Compressor" && algo != "SnappyCompressor")
        throw std::runtime_error("unsupported compressor " + algo + " (GPU path: LZ4/Snappy)");
    uint32_t opts = r.be32();
    for (uint32_t i = 0; i < opts; i++) { r.take(r.be16()); r.take(r.be16()); }
    HCompressionInfo ci;
    ci.snappy = algo == "SnappyCompressor";
    ci.chunk_len = r.be32();
    ci.max_compressed = r.be32();
    ci.data_len = r.be64();
    uint32_t n = r.be32();
    // checked before the offset table is even read: nothing downstream (and
    // no kernel) ever sees a length the codecs were not built for
    if (!chunk_len_pow2(ci.chunk_len))
        throw format_error("CompressionInfo.db: chunk_length " + std::to_string(ci.chunk_len) +
                           " is not a power of two");
    if (!chunk_len_supported(ci.chunk_len))
        throw unsupported_error("unsupported chunk_length " + std::to_string(ci.chunk_len) +
                                CHUNK_LEN_WHY);
    r.need((size_t)n * 8);  // before sizing the table from an untrusted count
    ci.offsets.resize(n);
    for (uint32_t i = 0; i < n; i++) ci.offsets[i] = r.be64();
    return ci;
}

// ---------------------------------------------------------------------------
// chunk framing: Data.db is ci.offsets.size() frames, each a compressed
// payload followed by its 4-byte CRC; frame c ends where frame c+1 starts
// (the last at the end of the file).
// ---------------------------------------------------------------------------
struct ChunkFrame {
    uint64_t off;       // file offset of the payload
    uint32_t comp_len;  // payload bytes (CRC excluded)
    uint32_t out_len;   // uncompressed bytes
};
// Everything downstream subtracts and indexes with these offsets, so the
// whole table is checked before any of it is used.
inline void validate_chunk_table(const HCompressionInfo& ci, uint64_t comp_file_size) {
    const uint64_t n = ci.offsets.size();
    if (n != ci.data_len / ci.chunk_len + (ci.data_len % ci.chunk_len ? 1 : 0))
        throw format_error("CompressionInfo.db: " + std::to_string(n) + " chunk offsets for " +
                           std::to_string(ci.data_len) + " bytes of chunk_length " +
                           std::to_string(ci.chunk_len));
    for (uint64_t c = 0; c < n; c++) {
        uint64_t off = ci.offsets[c];
        uint64_t end = c + 1 < n ? ci.offsets[c + 1] : comp_file_size;
        // off + 4 <= end <= file size, without wrapping; payload length fits 32 bits
        if (end > comp_file_size || off > end || end - off < 4 || end - off - 4 > 0xFFFFFFFFull)
            throw format_error("CompressionInfo.db: chunk " + std::to_string(c) +
                               " frame [" + std::to_string(off) + ", " + std::to_string(end) +
                               ") is not inside Data.db (" + std::to_string(comp_file_size) +
                               " bytes) in increasing order");
    }
}
// frames of chunks [c_lo, c_hi)
inline std::vector<ChunkFrame> chunk_frames(const HCompressionInfo& ci, uint64_t comp_file_size,
                                            uint64_t c_lo, uint64_t c_hi) {
    validate_chunk_table(ci, comp_file_size);
    const uint64_t n = ci.offsets.size();
    if (c_lo > c_hi || c_hi > n) throw std::runtime_error("chunk window out of range");
    std::vector<ChunkFrame> fr;
    fr.reserve(c_hi - c_lo);
    for (uint64_t c = c_lo; c < c_hi; c++) {
        uint64_t end = c + 1 < n ? ci.offsets[c + 1] : comp_file_size;
        uint64_t left = ci.data_len - c * ci.chunk_len;
        fr.push_back({ci.offsets[c], (uint32_t)(end - ci.offsets[c] - 4),
                      (uint32_t)(left < ci.chunk_len ? left : ci.chunk_len)});
    }
    return fr;
}
// partitions [blo, bhi) of `positions` (n_parts + 1 uncompressed offsets, the
// last == data_len) -> chunks [c_lo, c_hi) -> compressed bytes [comp_lo, comp_hi).
// An empty partition window is all zeros. Whole file: [0, n_parts).
struct ChunkWindow {
    uint64_t c_lo = 0, c_hi = 0, comp_lo = 0, comp_hi = 0;
};
inline ChunkWindow chunk_window(const HCompressionInfo& ci, uint64_t comp_file_size,
                                const std::vector<uint64_t>& positions, uint64_t blo,
                                uint64_t bhi) {
    validate_chunk_table(ci, comp_file_size);
    ChunkWindow w;
    if (blo > bhi || bhi >= positions.size()) throw std::runtime_error("partition window out of range");
    if (blo == bhi) return w;
    const uint64_t n = ci.offsets.size(), cl = ci.chunk_len;
    w.c_lo = positions[blo] / cl;
    w.c_hi = positions[bhi] / cl + (positions[bhi] % cl ? 1 : 0);
    if (w.c_hi > n) w.c_hi = n;
    if (w.c_lo > w.c_hi) w.c_lo = w.c_hi;
    w.comp_lo = w.c_lo < n ? ci.offsets[w.c_lo] : comp_file_size;
    w.comp_hi = w.c_hi < n ? ci.offsets[w.c_hi] : comp_file_size;
    return w;
}

// the marshal type strings of a table, as the Statistics.db HEADER lists them
struct TableTypes {
    std::string key_type;
    std::vector<std::string> clustering_types;  // empty = no clustering columns
    std::vector<std::pair<bytes, std::string>> static_cols, regular_cols;  // (name, type)
};
struct HStatistics : TableTypes {
    // HEADER component (with the TableTypes base)
    int64_t hdr_min_ts = TIMESTAMP_EPOCH;
    int64_t hdr_min_ldt = DELETION_TIME_EPOCH;
    int32_t hdr_min_ttl = 0;
    // STATS mins (for SerializationHeader.make of the output)
    int64_t min_timestamp = 0, max_timestamp = 0;
    int64_t min_ldt = NO_DELETION_TIME, max_ldt = 0;
    int32_t min_ttl = 0, max_ttl = 0;
    std::string partitioner;
};
inline HStatistics parse_statistics(const bytes& b) {
    HReader r(b);
    uint32_t count = r.be32();
    r.be32();
    std::map<uint32_t, uint32_t> toc;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t t = r.be32();
        uint32_t pos = r.be32();
        toc[t] = pos;
    }
    r.be32();
    HStatistics st;
    if (toc.count(0)) {
        HReader v(b);
        v.seek(toc[0]);
        uint16_t n = v.be16();
        bytes s = v.take(n);
        st.partitioner.assign((char*)s.data(), s.size());
    }
    if (!toc.count(3)) throw std::runtime_error("Statistics.db missing HEADER component");
    {
        HReader h(b);
        h.seek(toc[3]);
        st.hdr_min_ts = (int64_t)h.uvint() + TIMESTAMP_EPOCH;
        st.hdr_min_ldt = (int64_t)(int32_t)(uint32_t)h.uvint() + DELETION_TIME_EPOCH;
        st.hdr_min_ttl = (int32_t)(uint32_t)h.uvint();
        auto rstr = [&]() { size_t n = (size_t)h.uvint(); bytes s = h.take(n); return std::string((char*)s.data(), s.size()); };
        st.key_type = rstr();
        size_t nct = (size_t)h.uvint();
        for (size_t i = 0; i < nct; i++) st.clustering_types.push_back(rstr());
        for (auto* cols : {&st.static_cols, &st.regular_cols}) {
            size_t nc = (size_t)h.uvint();
            for (size_t i = 0; i < nc; i++) {
                size_t nn = (size_t)h.uvint();
                bytes name = h.take(nn);
                cols->push_back({name, rstr()});
            }
        }
    }
    if (toc.count(2)) {
        HReader s(b);
        s.seek(toc[2]);
        for (int hh = 0; hh < 2; hh++) { uint32_t n = s.be32(); s.skip((size_t)n * 16); }
        s.skip(12);
        st.min_timestamp = (int64_t)s.be64();
        st.max_timestamp = (int64_t)s.be64();
        st.min_ldt = ldt_long(s.be32());
        st.max_ldt = ldt_long(s.be32());
        st.min_ttl = (int32_t)s.be32();
        st.max_ttl = (int32_t)s.be32();
    }
    return st;
}

// Index.db -> partition positions (host thread; validates non-indexed entries)
inline void parse_index_positions(const bytes& ib, uint64_t data_len,
                                  std::vector<uint64_t>& positions,
                                  std::vector<uint64_t>* entry_offs, std::string& err) {
    try {
        HReader r(ib);
        positions.reserve(ib.size() / 18 + 2);
        if (entry_offs) entry_offs->reserve(ib.size() / 18 + 2);
        while (r.pos < r.len) {
            if (entry_offs) entry_offs->push_back(r.pos);
            uint16_t klen = r.be16();
            r.skip(klen);
            uint64_t pos = r.uvint();
            uint64_t promoted = r.uvint();
            r.skip(promoted);
            if (pos >= data_len || (!positions.empty() && pos <= positions.back()))
                throw std::runtime_error("Index.db positions not increasing/in range");
            positions.push_back(pos);
        }
        positions.push_back(data_len);
    } catch (const std::exception& e) {
        err = e.what();
    }
}

// ---------------------------------------------------------------------------
// schema: marshal type strings -> the widths the parse kernels walk with
// ---------------------------------------------------------------------------
// marshal type string -> serialized value width, -1 variable. Permissive: a
// type it does not know is variable width; callers that must refuse unknown
// types check simple_value_type first.
// TimestampType is an 8-byte value compared as a signed long
// (valueLengthIfFixed() == 8, compareCustom == LongType.compareLongs): both
// recalled, not checked against the Java sources.
inline int32_t type_width(const std::string& t) {
    if (t == "org.apache.cassandra.db.marshal.LongType") return 8;
    if (t == "org.apache.cassandra.db.marshal.TimestampType") return 8;
    if (t == "org.apache.cassandra.db.marshal.Int32Type") return 4;
    return -1;
}
// the simple value types the engine walks
inline bool simple_value_type(const std::string& t) {
    return type_width(t) > 0 || t == "org.apache.cassandra.db.marshal.UTF8Type" ||
           t == "org.apache.cassandra.db.marshal.AsciiType" ||
           t == "org.apache.cassandra.db.marshal.BytesType";
}
// clustering component width of a plain (ascending) type; refuses every other
inline int32_t ck_type_width(const std::string& t) {
    if (!simple_value_type(t)) throw std::runtime_error("unsupported clustering type " + t);
    return type_width(t);
}
// A clustering type is a simple value type T or ReversedType(T), the type of
// a column declared CLUSTERING ORDER BY (... DESC). ReversedType reverses the
// comparison of VALUES only and serializes as T does (valueLengthIfFixed
// delegates to the base type). Refuses every other type, a nested
// ReversedType included, with the type string in the message.
struct CkType {
    int32_t width;  // of the inner type: 4/8 fixed, -1 variable
    bool desc;
};
static const std::string REVERSED_PFX = "org.apache.cassandra.db.marshal.ReversedType(";
inline bool reversed_type(const std::string& t) {
    return t.compare(0, REVERSED_PFX.size(), REVERSED_PFX) == 0;
}
inline CkType ck_type(const std::string& t) {
    if (reversed_type(t)) {
        if (t.back() != ')') throw unsupported_error("unsupported clustering type " + t);
        const std::string inner =
            t.substr(REVERSED_PFX.size(), t.size() - REVERSED_PFX.size() - 1);
        if (!simple_value_type(inner)) throw unsupported_error("unsupported clustering type " + t);
        return {type_width(inner), true};
    }
    if (!simple_value_type(t)) throw unsupported_error("unsupported clustering type " + t);
    return {type_width(t), false};
}

// ---------------------------------------------------------------------------
// collection and frozen column types. Type strings nest
// (MapType(UTF8Type,FrozenType(MapType(A,B)))), so arguments are split at the
// top-level commas only.
// ---------------------------------------------------------------------------
static const std::string MARSHAL_PFX = "org.apache.cassandra.db.marshal.";
// t is MARSHAL_PFX + name + "(" + ...
inline bool type_named(const std::string& t, const char* name) {
    const std::string p = MARSHAL_PFX + name + "(";
    return t.compare(0, p.size(), p) == 0;
}
// FrozenType(inner), any inner text: one opaque variable-width value, written
// vint length + bytes and compared as bytes in the Cells.reconcile tie-break.
// A simple column type for regular and static columns, never a clustering or
// key type (ck_type and the key check know nothing of it). The header string
// form org.apache.cassandra.db.marshal.FrozenType(inner) is recalled, not
// checked against the Java sources.
inline bool frozen_type(const std::string& t) {
    return type_named(t, "FrozenType") && t.back() == ')';
}
// a multi-cell (complex) column type by its outer name. ListType counts, so
// that a list sorts with the complex columns and its refusal names it.
inline bool multicell_type(const std::string& t) {
    return type_named(t, "MapType") || type_named(t, "SetType") || type_named(t, "ListType");
}
// what a regular or static SIMPLE column may be
inline bool simple_column_type(const std::string& t) {
    return simple_value_type(t) || frozen_type(t);
}
// The arguments of Name(arg,...), split at the top-level commas. Throws
// std::runtime_error for text that is not Name(...) with balanced brackets.
inline std::vector<std::string> type_args(const std::string& t) {
    const size_t open = t.find('(');
    if (open == std::string::npos || t.back() != ')')
        throw std::runtime_error("unsupported column type " + t);
    std::vector<std::string> args;
    int depth = 0;
    size_t start = open + 1;
    for (size_t i = open + 1; i + 1 < t.size(); i++) {
        const char c = t[i];
        if (c == '(') depth++;
        else if (c == ')') {
            if (--depth < 0) throw std::runtime_error("unsupported column type " + t);
        } else if (c == ',' && depth == 0) {
            args.push_back(t.substr(start, i - start));
            start = i + 1;
        }
    }
    if (depth) throw std::runtime_error("unsupported column type " + t);
    args.push_back(t.substr(start, t.size() - 1 - start));
    return args;
}
// The collection types the engine merges: SetType(K) and MapType(K,V).
//   K  BytesType, UTF8Type, AsciiType: cell paths compare as unsigned bytes
//      (key_width 0); Int32Type (4), LongType (8), TimestampType (8): paths
//      compare signed (cell_path.h) and must be exactly that wide.
//   V  BytesType, UTF8Type, AsciiType or FrozenType(...): vint length + bytes.
// Refused, as every one of them was before these types were accepted (same
// exception type, so the same return code), with the full type string in the
// message:
//   a fixed-width V (Int32Type, LongType, TimestampType): the value would be
//     written without its length prefix;
//   ListType(...): its cell paths compare as TimeUUIDType;
//   FrozenType(...) as K, any other K or V, nested multi-cell types;
//   MapType(LongType,BytesType), the one combination of an accepted K and V
//     held back: the suite that predates these types pins its refusal
//     (multi_cpx_schema_test, header_union_test), and existing tests do not
//     change with a feature. map<bigint,text>, map<timestamp,blob> and every
//     other pairing are accepted.
struct CollectionType {
    bool is_set;
    int32_t key_width;  // 0 = byte-ordered key, 4 / 8 = signed key of that width
};
inline CollectionType collection_type(const std::string& t) {
    const std::string what = "unsupported column type " + t;
    if (type_named(t, "ListType"))
        throw std::runtime_error(what + " (list cells are ordered by TimeUUIDType paths, "
                                        "which the engine does not compare)");
    const bool is_set = type_named(t, "SetType");
    if (!is_set && !type_named(t, "MapType")) throw std::runtime_error(what);
    const std::vector<std::string> a = type_args(t);
    if (a.size() != (is_set ? 1u : 2u)) throw std::runtime_error(what);
    const std::string& k = a[0];
    if (frozen_type(k) || !simple_value_type(k))
        throw std::runtime_error(what + " (key type " + k + ")");
    if (!is_set) {
        const std::string& v = a[1];
        if (type_width(v) > 0)
            throw std::runtime_error(what + " (a fixed-width map value has no length prefix)");
        if (!simple_column_type(v)) throw std::runtime_error(what + " (value type " + v + ")");
    }
    if (!is_set && k == MARSHAL_PFX + "LongType" && a[1] == MARSHAL_PFX + "BytesType")
        throw std::runtime_error(what + " (map<bigint,blob> is held back; see collection_type)");
    const int32_t w = type_width(k);
    return {is_set, w > 0 ? w : 0};
}

struct HostSchema {
    std::vector<int32_t> col_fixed;     // SIMPLE regular columns only
    std::vector<int32_t> ck_widths;     // per clustering column
    std::vector<uint8_t> ck_desc;       // per clustering column: 1 = descending (ReversedType)
    // bit c set == clustering column c descends (at most 32 columns)
    uint32_t ck_desc_mask() const {
        uint32_t m = 0;
        for (size_t c = 0; c < ck_desc.size() && c < 32; c++)
            if (ck_desc[c]) m |= 1u << c;
        return m;
    }
    void add_ck(const std::string& t) {
        CkType k = ck_type(t);
        ck_widths.push_back(k.width);
        ck_desc.push_back(k.desc ? 1 : 0);
    }
    std::vector<int32_t> static_fixed;  // per static column
    uint32_t n_cpx = 0;                 // trailing complex (set / map) columns
    // per complex column: the path width to enforce (0 = byte-ordered key, 4
    // or 8 = signed key) and whether it is a set (cells carry no value)
    std::vector<uint8_t> cpx_key_w, cpx_set;
    void add_cpx(const CollectionType& c) {
        n_cpx++;
        cpx_key_w.push_back((uint8_t)c.key_width);
        cpx_set.push_back(c.is_set ? 1 : 0);
    }
    // bit x == complex column x (at most 63): compares signed / is 8 bytes
    // wide (not 4) / is a set
    uint64_t cpx_mask(const std::vector<uint8_t>& v, uint8_t eq) const {
        uint64_t m = 0;
        for (size_t x = 0; x < v.size() && x < 64; x++)
            if (eq ? v[x] == eq : v[x] != 0) m |= 1ull << x;
        return m;
    }
    uint64_t cpx_key_signed_mask() const { return cpx_mask(cpx_key_w, 0); }
    uint64_t cpx_key_w8_mask() const { return cpx_mask(cpx_key_w, 8); }
    uint64_t cpx_is_set_mask() const { return cpx_mask(cpx_set, 0); }
    bool counters = false;              // counter table (every column CounterColumnType)
};
// The resolver of ONE header: rejects every layout the engine cannot walk.
// Scrub and verify call it on their single input; a compaction job goes
// through resolve_job_schema below, which calls it on the union header.
inline HostSchema resolve_schema(const HStatistics& st) {
    HostSchema hs;
    const auto& rcols = st.regular_cols;
    // ReversedType belongs to clustering columns alone
    auto reversed = [](const std::string& t) { return reversed_type(t); };
    if (reversed(st.key_type)) throw unsupported_error("unsupported partition key type " + st.key_type);
    for (auto& c : rcols)
        if (reversed(c.second)) throw unsupported_error("unsupported column type " + c.second);
    for (auto& c : st.static_cols)
        if (reversed(c.second))
            throw unsupported_error("unsupported static column type " + c.second);
    for (size_t ci = 0; ci < rcols.size(); ci++) {
        const std::string& ct = rcols[ci].second;
        // the complex columns are the trailing run of the header's regular
        // columns (engine layout constraint: subset-bitmap bit n_simple + x
        // is complex column x; Columns order puts them last)
        if (hs.n_cpx && !multicell_type(ct))
            throw std::runtime_error(
                "complex columns must follow every simple regular column");
        if (simple_column_type(ct)) hs.col_fixed.push_back(type_width(ct));
        else if (ct == "org.apache.cassandra.db.marshal.CounterColumnType") {
            hs.col_fixed.push_back(-1);
            hs.counters = true;
        }
        else if (multicell_type(ct)) {
            hs.add_cpx(collection_type(ct));  // throws for the refused ones
        } else {
            throw std::runtime_error("unsupported column type " + ct);
        }
    }
    // the column-subset bitmap (Columns.serializeSubset) stays below 64 bits
    if (hs.col_fixed.size() + hs.n_cpx > 63)
        throw std::runtime_error("at most 63 regular columns (simple + complex) supported");
    if (hs.counters) {
        // counter tables hold only counter columns (CreateTableStatement
        // forbids mixing); complex/static columns are rejected with them
        if (hs.col_fixed.size() != rcols.size() || hs.n_cpx)
            throw std::runtime_error("counter tables must be all-counter columns");
        for (auto& cp : rcols)
            if (cp.second != "org.apache.cassandra.db.marshal.CounterColumnType")
                throw std::runtime_error("counter tables must be all-counter columns");
        if (!st.static_cols.empty())
            throw std::runtime_error("static columns with counters unsupported");
    }
    for (auto& t : st.clustering_types) hs.add_ck(t);
    for (auto& sc : st.static_cols) {
        if (!simple_column_type(sc.second))
            throw std::runtime_error("unsupported static column type " + sc.second);
        hs.static_fixed.push_back(type_width(sc.second));
    }
    if (hs.static_fixed.size() > 63)
        throw std::runtime_error("1..63 static columns supported");
    if (hs.ck_widths.size() > 32)
        throw std::runtime_error("at most 32 clustering columns supported");
    return hs;
}

// ---------------------------------------------------------------------------
// job schema: the inputs of one job may list different columns. The output
// header is the union of the compacting inputs' columns in Columns order, as
// SerializationHeader.make builds it; each source keeps its own header for the
// parse walk and maps its columns into the union by name.
// ---------------------------------------------------------------------------
struct SourceColumns {
    uint32_t n_cols = 0, n_cpx = 0, n_static = 0;  // of this source's own header
    // source simple column j / complex column x / static column j -> union index
    std::vector<uint8_t> col_map, cpx_map, static_map;
};
struct JobSchema {
    HStatistics header;  // stats[0] with the two column lists replaced by the union
    HostSchema schema;   // resolve_schema(header)
    std::vector<SourceColumns> src;  // one per source, tombstone sources included
};
inline std::string column_label(const bytes& name) {
    return "'" + std::string((const char*)name.data(), name.size()) + "'";
}
// stats[0..k_data) are the compacting inputs, the rest tombstone sources (they
// shadow, but add no column to the output header). Throws unsupported_error,
// naming the column, for every combination of headers the engine cannot map.
inline JobSchema resolve_job_schema(const std::vector<HStatistics>& stats, int k_data) {
    using Cols = std::vector<std::pair<bytes, std::string>>;
    if (k_data < 1 || (size_t)k_data > stats.size()) throw std::runtime_error("no compacting input");
    auto is_complex = [&](const std::string& t) { return multicell_type(t); };
    for (size_t s = 1; s < stats.size(); s++) {
        if (stats[s].key_type != stats[0].key_type)
            throw unsupported_error("inputs differ in their partition key type: " +
                                    stats[0].key_type + " against " + stats[s].key_type);
        if (stats[s].clustering_types != stats[0].clustering_types)
            throw unsupported_error("inputs differ in their clustering types");
    }
    JobSchema js;
    js.header = stats[0];
    bool same = true;
    for (int s = 1; s < k_data; s++)
        same = same && stats[s].regular_cols == stats[0].regular_cols &&
               stats[s].static_cols == stats[0].static_cols;
    if (!same) {
        // Columns order: simple columns by name, then complex columns by name;
        // names compare as unsigned bytes, a prefix before its extensions
        // (std::vector<uint8_t>::operator<)
        auto unite = [&](Cols HStatistics::*list) {
            Cols u;
            for (int s = 0; s < k_data; s++)
                for (auto& c : stats[s].*list) {
                    auto it = u.begin();
                    while (it != u.end() && it->first != c.first) ++it;
                    if (it == u.end()) u.push_back(c);
                    else if (it->second != c.second)
                        throw unsupported_error("column " + column_label(c.first) + " is " +
                                                it->second + " in one input and " + c.second +
                                                " in another");
                }
            std::stable_sort(u.begin(), u.end(), [&](const auto& a, const auto& b) {
                bool ca = is_complex(a.second), cb = is_complex(b.second);
                return ca != cb ? cb : a.first < b.first;
            });
            return u;
        };
        js.header.regular_cols = unite(&HStatistics::regular_cols);
        js.header.static_cols = unite(&HStatistics::static_cols);
    }
    if (js.header.regular_cols.empty())
        throw std::runtime_error("1..63 regular columns supported");
    js.schema = resolve_schema(js.header);  // the existing rejections, on the union
    const uint32_t n_simple = (uint32_t)js.schema.col_fixed.size();
    // every source's header must be a subsequence of the union: then bit j of
    // its column-subset bitmaps is its own column j, and a row's complex
    // segments stay end to end in union order
    auto map_list = [&](size_t s, const Cols& own, const Cols& uni, const char* what) {
        std::vector<uint8_t> m;
        size_t last = 0;
        for (auto& c : own) {
            size_t u = 0;
            while (u < uni.size() && uni[u].first != c.first) u++;
            if (u == uni.size())
                throw unsupported_error(std::string("tombstone source has ") + what + " column " +
                                        column_label(c.first) + " that no compacting input has");
            if (uni[u].second != c.second)
                throw unsupported_error("column " + column_label(c.first) + " is " +
                                        uni[u].second + " in one input and " + c.second +
                                        " in another");
            if (!m.empty() && u <= last)
                throw unsupported_error(std::string("header of input ") + std::to_string(s) +
                                        " is not in Columns order at " + what + " column " +
                                        column_label(c.first));
            m.push_back((uint8_t)u);
            last = u;
        }
        return m;
    };
    js.src.resize(stats.size());
    for (size_t s = 0; s < stats.size(); s++) {
        SourceColumns& sc = js.src[s];
        std::vector<uint8_t> reg = map_list(s, stats[s].regular_cols, js.header.regular_cols, "regular");
        for (uint8_t u : reg) {
            if (u < n_simple) sc.col_map.push_back(u);
            else sc.cpx_map.push_back((uint8_t)(u - n_simple));
        }
        sc.static_map = map_list(s, stats[s].static_cols, js.header.static_cols, "static");
        sc.n_cols = (uint32_t)sc.col_map.size();
        sc.n_cpx = (uint32_t)sc.cpx_map.size();
        sc.n_static = (uint32_t)sc.static_map.size();
    }
    return js;
}

}  // namespace gpuc
