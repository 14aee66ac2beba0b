// TEST TOOL — widens an oracle-generated sstable to several complex columns.
//
//   widen <in_base> <out_base> <n_extra> [strip]
//
// Reads an sstable whose last regular column is the generator's map column
// `zm`, appends n_extra more map<blob,blob> columns (`zn`, `zo`, ...), fills
// them per row from a hash of (token, item index, x, generation), and
// rewrites every component with the oracle's own writer. With `strip` all
// simple regular columns are removed first (a table whose only regular
// columns are maps).
//
// Per extra column x the mode is hash % 4:
//   0  absent
//   1  a copy of the row's zm data (deletion included) with byte x appended
//      to every path (the generator's paths have one length, so the order
//      is preserved)
//   2  deletion only: mfda = the row's liveness ts,
//      ldt = header min_ldt + 1000 + (hash >> 8) % 100000
//   3  the first half of zm's cells, no deletion
// Rows without zm data: with liveness, mode 2 gives the same deletion and
// modes 1/3 a single cell {ts = liveness ts, path = {x}, 4-byte value};
// without liveness nothing is added. No timestamp or ldt falls below the
// header minimums, so the input's EncodingStats stay valid.
//
// Prints "mixed_del=<n> del_only=<n> partial=<n>": rows where one present
// complex column has a real deletion and another a live one; rows with a
// deletion-only column; rows where some but not all complex columns are
// present.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../oracle/src/sstable.h"

using namespace oracle;

static uint64_t mix(uint64_t z) {
    z += 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: widen <in_base> <out_base> <n_extra> [strip]\n");
        return 2;
    }
    const std::string in_base = argv[1], out_base = argv[2];
    const int n_extra = atoi(argv[3]);
    const bool strip = argc > 4 && !strcmp(argv[4], "strip");
    try {
        SSTable t = read_sstable(in_base);
        auto& cols = t.header.regular_cols;
        if (cols.empty() || cols.back().second != CqlType::MAP_BB || n_extra < 1 || n_extra > 20)
            throw std::runtime_error("input's last regular column must be the map column zm");
        const size_t n_old = cols.size(), zm = n_old - 1;
        for (int x = 0; x < n_extra; x++) {
            bytes nm = {(uint8_t)'z', (uint8_t)('n' + x)};
            cols.emplace_back(nm, CqlType::MAP_BB);
        }
        if (strip) cols.erase(cols.begin(), cols.begin() + zm);
        const size_t first_cpx = strip ? 0 : zm;
        const size_t n_new = cols.size(), n_cpx = n_new - first_cpx;

        uint64_t mixed_del = 0, del_only = 0, partial = 0;
        std::vector<Partition> kept_parts;
        for (Partition& p : t.parts) {
            std::vector<Unfiltered> items;
            for (size_t ii = 0; ii < p.items.size(); ii++) {
                Unfiltered& u = p.items[ii];
                if (u.kind != Unfiltered::ROW) { items.push_back(std::move(u)); continue; }
                Row& r = u.row;
                std::optional<ComplexData> base;
                if (zm < r.complex.size()) base = r.complex[zm];
                std::vector<std::optional<Cell>> cells(n_new);
                std::vector<std::optional<ComplexData>> cpx(n_new);
                if (!strip)
                    for (size_t c = 0; c < zm && c < r.cells.size(); c++) cells[c] = r.cells[c];
                cpx[first_cpx] = base;
                for (int x = 0; x < n_extra; x++) {
                    uint64_t h = mix(mix((uint64_t)p.token) ^ mix(ii * 31 + x) ^
                                     mix(t.generation * 1000003ULL + 7));
                    int mode = (int)(h % 4);
                    if (mode == 0) continue;
                    if (r.live.empty() && (!base || mode == 2)) continue;
                    DeletionTime own{r.live.ts,
                                     (uint32_t)(t.header.stats.min_ldt + 1000 + (h >> 8) % 100000)};
                    ComplexData cd;
                    if (mode == 2) {
                        cd.del = own;
                    } else if (!base) {
                        Cell c;
                        c.ts = r.live.ts;
                        c.path = {(uint8_t)x};
                        c.value = {(uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8),
                                   (uint8_t)h};
                        cd.cells.push_back(c);
                    } else if (mode == 1) {
                        cd = *base;
                        for (Cell& c : cd.cells) c.path.push_back((uint8_t)x);
                    } else {
                        size_t half = (base->cells.size() + 1) / 2;
                        cd.cells.assign(base->cells.begin(), base->cells.begin() + half);
                    }
                    if (cd.del.live() && cd.cells.empty()) continue;  // an absent column
                    cpx[first_cpx + 1 + x] = std::move(cd);
                }
                r.cells = std::move(cells);
                r.complex = std::move(cpx);
                size_t present = 0;
                bool real = false, live = false, donly = false;
                for (size_t c = first_cpx; c < n_new; c++) {
                    if (!r.complex[c]) continue;
                    present++;
                    (r.complex[c]->del.live() ? live : real) = true;
                    if (r.complex[c]->cells.empty()) donly = true;
                }
                if (real && live) mixed_del++;
                if (donly) del_only++;
                if (present && present < n_cpx) partial++;
                if (!row_is_empty(r)) items.push_back(std::move(u));
            }
            p.items = std::move(items);
            if (p.items.empty() && p.del.live() && row_is_empty(p.static_row)) continue;
            kept_parts.push_back(std::move(p));
        }
        t.parts = std::move(kept_parts);
        WriterOut w = write_sstable(t, t.bti);
        write_components(w, out_base);
        printf("mixed_del=%llu del_only=%llu partial=%llu\n", (unsigned long long)mixed_del,
               (unsigned long long)del_only, (unsigned long long)partial);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "widen: %s\n", e.what());
        return 1;
    }
}
