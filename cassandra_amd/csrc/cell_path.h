// PRODUCT — CellPath order of a multi-cell collection column, host and device.
// A ComplexColumnData keeps its cells in CellPath order, and that order is
// the comparator of the collection's KEY type (the element type of a set, the
// key type of a map). The merge kernel (k_reconcile_rows), the garbage-collect
// kernels (gc_path_cmp), gpuc_flush_table's order check (h_path_cmp) and the
// plain-g++ native test (tests/native/collection_types_test.cpp) all run the
// one function below. No HIP here beyond GPUC_HD.
//
//   byte-ordered keys   BytesType, UTF8Type, AsciiType: unsigned bytes, a
//                       prefix before its extensions.
//   signed keys         Int32Type, LongType, TimestampType: the first byte as
//                       a SIGNED byte, the rest unsigned (Int32Type.compare,
//                       LongType.compareLongs; TimestampType compares like
//                       LongType — recalled, see sstable_meta.h). For values
//                       of one width that is numeric signed order. It equals
//                       the byte order after XORing the first byte with 0x80,
//                       which is how it is computed here, so the compare needs
//                       no width and is total over paths of any length; the
//                       parse kernels still refuse a signed-key path that is
//                       not 4 or 8 bytes wide.
//
// On disk a CellPath is vint length + bytes whatever the key type
// (CollectionType.CollectionPathSerializer), so the type changes the order
// and nothing else.
#pragma once
#include <stdint.h>

#include "codec.h"

namespace gpuc {

// Per complex column x of a schema, as bit x of three masks (at most 63
// complex columns): the key compares signed; the signed key is 8 bytes wide
// (else 4); the column is a set (its cells carry no value).
GPUC_HD inline bool cpx_bit(uint64_t mask, uint32_t x) { return (mask >> x) & 1ull; }
// the path width a column enforces: 0 = any (byte-ordered key), else 4 or 8
GPUC_HD inline uint32_t cpx_key_width(uint64_t key_signed, uint64_t key_w8, uint32_t x) {
    return cpx_bit(key_signed, x) ? (cpx_bit(key_w8, x) ? 8u : 4u) : 0u;
}

// <0, 0, >0 as path a sorts before, with, after path b
GPUC_HD inline int cell_path_cmp(const uint8_t* pa, uint32_t la, const uint8_t* pb, uint32_t lb,
                                 bool key_signed) {
    const uint32_t n = la < lb ? la : lb;
    if (n) {
        const uint8_t flip = key_signed ? 0x80 : 0;
        const uint8_t a0 = pa[0] ^ flip, b0 = pb[0] ^ flip;
        if (a0 != b0) return a0 < b0 ? -1 : 1;
    }
    for (uint32_t i = 1; i < n; i++)
        if (pa[i] != pb[i]) return pa[i] < pb[i] ? -1 : 1;
    return la == lb ? 0 : (la < lb ? -1 : 1);
}

}  // namespace gpuc
