// PRODUCT — host side of libcassandra_gpucompact: input file I/O and the HIP
// pipeline orchestration. The bytes of the small output components are
// decided in sstable_out.h (host-only, CPU-tested); the input metadata is
// parsed in sstable_meta.h. Compiled as one TU with kernels.hip by hipcc.
//
// The host does NO data-path compute: decompress/decode/merge/reconcile/
// purge/serialize/compress/CRC/bloom all run in the kernels. There is no CPU
// fallback — gpuc_compact fails with GPUC_ERR_NO_GPU when no device exists.
#include "kernels.hip"
#include "kernels_rows.hip"
#include "bti_core.h"
#include "sstable_meta.h"
#include "sstable_out.h"
#include "../../include/gpucompact.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <future>
#include <functional>
#include <atomic>
#include <fcntl.h>
#include <unistd.h>
#include <vector>

namespace gpuc {

#define HIP_CHECK(x)                                                              \
    do {                                                                          \
        hipError_t _e = (x);                                                      \
        if (_e != hipSuccess)                                                     \
            throw std::runtime_error(std::string("HIP error: ") +                 \
                                     hipGetErrorString(_e) + " at " #x);          \
    } while (0)

// grow-only pinned staging buffers, reused across calls (hipHostMalloc is
// expensive; a compaction service reuses its staging arenas the same way)
struct PinnedSlot {
    void* p = nullptr;
    size_t cap = 0;
    void* get(size_t n) {
        if (n > cap) {
            if (p) (void)hipHostFree(p);
            size_t want = n + n / 4;
            if (hipHostMalloc(&p, want) != hipSuccess) { p = nullptr; cap = 0; return nullptr; }
            cap = want;
        }
        return p;
    }
};
static PinnedSlot g_pin_in[2][64], g_pin_out[2][4];

// GPUC_TRACE=1: wall-clock checkpoints on stderr (host-gap hunting)
static bool g_trace = getenv("GPUC_TRACE") != nullptr;
// Merkle-leaf validation (gpuc_validate_merkle). The spec is checked before it
// gets here.
struct MerkleRun {
    const gpuc_merkle_spec* spec;
    uint8_t* leaf_hash;         // n_leaves * 32, out
    uint64_t* leaf_partitions;  // n_leaves, out; may be NULL
    uint64_t n_partitions;      // out: sum of the leaf counts
};
// Routed outputs (gpuc_compact_routed). The spec is checked before it gets here.
struct RouteRun {
    const gpuc_route_spec* spec;
    gpuc_route_output* outputs;  // n_outputs, out; may be NULL
};
// What a run of run_compaction produces: at most one member is set, and with
// none set it writes sstable(s). Each entry point fills it in and passes it
// down by reference, shard workers included; the entry points' argument
// checks decide which job options a mode may be combined with.
struct CompactMode {
    const char* digest_path = nullptr;  // gpuc_validate: the digest file
    uint64_t* digest_count = nullptr;   //   out: partitions digested
    MerkleRun* merkle = nullptr;
    RouteRun* route = nullptr;
};
static double g_trace_t0 = 0;
static double wall_ms() {
    struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec / 1e6;
}
static void TR(const char* tag) {
    if (!g_trace) return;
    double t = wall_ms();
    fprintf(stderr, "[gpuc %8.1f] %s\n", t - g_trace_t0, tag);
}
static bool file_exists(const std::string& path) { return access(path.c_str(), F_OK) == 0; }


// threaded read of a whole file into (pinned) memory
static size_t file_size_of(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fclose(f);
    return (size_t)n;
}
static void read_file_range(const std::string& path, uint8_t* dst, uint64_t off, size_t n,
                            int nthreads = 3) {
    if (n == 0) return;
    std::vector<std::thread> th;
    size_t per = (n + nthreads - 1) / nthreads;
    for (int t = 0; t < nthreads; t++) {
        size_t o = (size_t)t * per;
        if (o >= n) break;
        size_t len = std::min(per, n - o);
        th.emplace_back([&, o, len]() {
            int fd = open(path.c_str(), O_RDONLY);
            if (fd < 0) return;
            size_t done = 0;
            while (done < len) {
                ssize_t r = pread(fd, dst + o + done, len - done, (off_t)(off + o + done));
                if (r <= 0) break;
                done += (size_t)r;
            }
            close(fd);
        });
    }
    for (auto& x : th) x.join();
}

static bytes read_file(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    bytes b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) { fclose(f); throw std::runtime_error("short read " + path); }
    fclose(f);
    return b;
}

// ---------------------------------------------------------------------------
// device helpers (scan, merge)
// ---------------------------------------------------------------------------
// caching device allocator: hipMalloc of multi-GB buffers costs 100+ ms, and
// every compaction call uses the same transient working set, so freed blocks
// are pooled by power-of-two size class and reused across calls.
class DevPool {
    std::mutex mu_;
    std::map<size_t, std::vector<void*>> free_;

public:
    static size_t cls(size_t n) {
        size_t c = 4096;
        while (c < n) c <<= 1;
        return c;
    }
    void* get(size_t n) {
        size_t c = cls(n);
        {
            std::lock_guard<std::mutex> g(mu_);
            auto it = free_.find(c);
            if (it != free_.end() && !it->second.empty()) {
                void* p = it->second.back();
                it->second.pop_back();
                return p;
            }
        }
        void* p = nullptr;
        if (hipMalloc(&p, c) != hipSuccess) {
            trim();
            HIP_CHECK(hipMalloc(&p, c));
        }
        return p;
    }
    void put(size_t n, void* p) {
        std::lock_guard<std::mutex> g(mu_);
        free_[cls(n)].push_back(p);
    }
    void trim() {
        std::lock_guard<std::mutex> g(mu_);
        for (auto& [c, v] : free_) {
            for (void* p : v) (void)hipFree(p);
            v.clear();
        }
    }
};
static DevPool g_dev_pool;

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    void alloc(size_t bytes_) {
        free_();
        n = bytes_ ? bytes_ : 8;
        p = g_dev_pool.get(n);
    }
    void free_() {
        if (p) {
            g_dev_pool.put(n, p);
            p = nullptr;
        }
    }
    ~DevBuf() { free_(); }
    template <typename T> T* as() const { return (T*)p; }
};
// Allocate n elements (+ pad bytes) and copy them up asynchronously: `src`
// must outlive the next synchronise of `stream`.
template <typename T>
static T* upload(DevBuf& d, const T* src, size_t n, hipStream_t stream, size_t pad = 0) {
    d.alloc(n * sizeof(T) + pad);
    if (n) HIP_CHECK(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
    return d.as<T>();
}

// exclusive scan over u64; returns total
static uint64_t exscan_u64(uint64_t* d_data, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    uint64_t n_blocks = (n + SCAN_TILE - 1) / SCAN_TILE;
    DevBuf sums, out;
    sums.alloc(n_blocks * 8);
    out.alloc(n * 8);
    hipLaunchKernelGGL(k_scan_partial, dim3((uint32_t)n_blocks), dim3(SCAN_BLOCK), 0, stream,
                       d_data, out.as<uint64_t>(), sums.as<uint64_t>(), n);
    uint64_t total = 0;
    if (n_blocks > 1) {
        total = exscan_u64(sums.as<uint64_t>(), n_blocks, stream);
        hipLaunchKernelGGL(k_scan_add, dim3((uint32_t)n_blocks), dim3(SCAN_BLOCK), 0, stream,
                           out.as<uint64_t>(), sums.as<uint64_t>(), n);
    } else {
        uint64_t s;
        HIP_CHECK(hipMemcpyAsync(&s, sums.p, 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        total = s;
    }
    if (n_blocks > 1) {
        // total = scan total of sums + last block handled inside recursion; read final element
        uint64_t last_off, last_val;
        HIP_CHECK(hipMemcpyAsync(&last_off, out.as<uint64_t>() + (n - 1), 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(&last_val, d_data + (n - 1), 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        total = last_off + last_val;
    }
    HIP_CHECK(hipMemcpyAsync(d_data, out.p, n * 8, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return total;
}

// sort MRec array (uniform-run merge rounds); returns pointer to sorted buffer
static MRec* merge_sort_recs(MRec* d_a, MRec* d_b, uint64_t n, hipStream_t stream,
                             const KeyLut& lut) {
    MRec* in = d_a;
    MRec* out = d_b;
    for (uint64_t run = 1; run < n; run *= 2) {
        if (run < 16) {
            uint64_t pairs = (n + run * 2 - 1) / (run * 2);
            hipLaunchKernelGGL(k_merge_small, dim3((uint32_t)((pairs + 255) / 256)), dim3(256), 0,
                               stream, in, out, n, run, lut);
        } else {
            uint64_t tiles = (n + MERGE_TILE - 1) / MERGE_TILE;
            hipLaunchKernelGGL(k_merge_uniform, dim3((uint32_t)((tiles + 255) / 256)), dim3(256), 0,
                               stream, in, out, n, run, lut);
        }
        std::swap(in, out);
    }
    return in;
}

// merge k pre-sorted runs (per-source) with pairwise rounds
static MRec* merge_sorted_runs(MRec* d_a, MRec* d_b, std::vector<uint64_t> runs /*boundaries, size k+1*/,
                               hipStream_t stream, const KeyLut& lut) {
    MRec* in = d_a;
    MRec* out = d_b;
    while (runs.size() > 2) {
        std::vector<MergePair> pairs;
        std::vector<uint64_t> next_runs;
        next_runs.push_back(0);
        uint64_t tile_beg = 0;
        for (size_t i = 0; i + 1 < runs.size(); i += 2) {
            MergePair p{};
            p.a_beg = runs[i];
            p.a_end = runs[i + 1];
            if (i + 2 < runs.size()) { p.b_beg = runs[i + 1]; p.b_end = runs[i + 2]; }
            else { p.b_beg = p.a_end; p.b_end = p.a_end; }
            p.out_beg = p.a_beg;
            p.tile_beg = tile_beg;
            uint64_t n_out = (p.a_end - p.a_beg) + (p.b_end - p.b_beg);
            tile_beg += (n_out + MERGE_TILE - 1) / MERGE_TILE;
            pairs.push_back(p);
            next_runs.push_back(p.b_end);
        }
        DevBuf d_pairs;
        upload(d_pairs, pairs.data(), pairs.size(), stream);
        uint64_t total_tiles = tile_beg;
        hipLaunchKernelGGL(k_merge_pairs, dim3((uint32_t)((total_tiles + 255) / 256)), dim3(256), 0,
                           stream, in, out, d_pairs.as<MergePair>(), (uint32_t)pairs.size(), total_tiles, lut);
        HIP_CHECK(hipStreamSynchronize(stream));
        std::swap(in, out);
        runs = next_runs;
    }
    return in;
}

}  // namespace gpuc

namespace gpuc {

static void init_outstats(DevBuf& d_stats, hipStream_t stream) {
    hipLaunchKernelGGL(k_init_outstats, dim3(1), dim3(64), 0, stream, d_stats.as<OutStats>());
}

static bool g_crc_tables_ready = false;
static void* g_crc256 = nullptr;  // 8x256 sliced CRC tables (first 256 = base)
static std::mutex g_crc_init_mu;
static uint32_t* g_snp_off = nullptr;   // snappy probe-offset table (device)
static uint32_t g_snp_off_n = 0;

static void ensure_crc_tables(hipStream_t stream) {
    std::lock_guard<std::mutex> crc_g(g_crc_init_mu);
    if (g_crc_tables_ready) return;
    hipLaunchKernelGGL(k_crc_init, dim3(1), dim3(256), 0, stream);
    // plain 256-entry table for the wave LZ4 kernels
    uint32_t tab[256];
    crc32_make_table(tab);
    static uint32_t tab8[8 * 256];
    crc32_make_table8(tab8);
    HIP_CHECK(hipMalloc(&g_crc256, sizeof(tab8)));
    HIP_CHECK(hipMemcpyAsync(g_crc256, tab8, sizeof(tab8), hipMemcpyHostToDevice, stream));
    {   // snappy probe offsets (snappy.cc skip heuristic: skip=32, inc=skip>>5)
        std::vector<uint32_t> off{0};
        uint32_t skip = 32, o = 0;
        while (o < (1u << 16) + 128) {
            uint32_t inc = skip >> 5;
            skip += inc;
            o += inc;
            off.push_back(o);
        }
        g_snp_off_n = (uint32_t)off.size();
        HIP_CHECK(hipMalloc(&g_snp_off, off.size() * 4));
        HIP_CHECK(hipMemcpy(g_snp_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    }
    // verify the LDS same-address write-order rule the wave compressor relies on
    unsigned int* d_probe;
    HIP_CHECK(hipMalloc(&d_probe, 8));
    hipLaunchKernelGGL(k_probe_lds_order, dim3(1), dim3(WAVE), 0, stream, d_probe);
    unsigned int probe[2];
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipMemcpy(probe, d_probe, 8, hipMemcpyDeviceToHost));
    (void)hipFree(d_probe);
    if (probe[0] != 63 || probe[1] != 0)
        throw std::runtime_error("LDS conflicting-write order is not highest-lane-wins on this device; "
                                 "wave LZ4 compressor would be incorrect (refusing to run)");
    g_crc_tables_ready = true;
}

// allocate the OutParts SoA for n entries
// allocate a StaticCols block for n partitions x n_static columns
struct StaticColsBuf {
    DevBuf flags, live_ts, live_ttl, live_let, rdel_mfda, rdel_ldt,
        cell_flags, cell_ts, cell_ldt, cell_ttl, val_addr, val_len;
    StaticCols st{};
    void alloc(uint64_t n, uint32_t n_static) {
        if (!n) n = 1;
        uint64_t ns = n * (n_static ? n_static : 1);
        flags.alloc(n); live_ts.alloc(n * 8); live_ttl.alloc(n * 4); live_let.alloc(n * 8);
        rdel_mfda.alloc(n * 8); rdel_ldt.alloc(n * 4);
        cell_flags.alloc(ns); cell_ts.alloc(ns * 8); cell_ldt.alloc(ns * 4);
        cell_ttl.alloc(ns * 4); val_addr.alloc(ns * 8); val_len.alloc(ns * 4);
        st = StaticCols{flags.as<uint8_t>(), live_ts.as<int64_t>(), live_ttl.as<int32_t>(),
                        live_let.as<int64_t>(), rdel_mfda.as<int64_t>(), rdel_ldt.as<uint32_t>(),
                        cell_flags.as<uint8_t>(), cell_ts.as<int64_t>(), cell_ldt.as<uint32_t>(),
                        cell_ttl.as<int32_t>(), val_addr.as<uint64_t>(), val_len.as<uint32_t>()};
    }
};

struct OutPartsBuf {
    DevBuf keypfx, key_addr, token, klen, pdel_mfda, pdel_ldt, row_base, row_count, keep;
    StaticColsBuf stb;
    OutParts op{};
    DevBuf merged_k;
    void alloc(uint64_t n, uint32_t n_static = 0) {
        keypfx.alloc(n * 8); key_addr.alloc(n * 8); token.alloc(n * 8); klen.alloc(n * 2);
        pdel_mfda.alloc(n * 8); pdel_ldt.alloc(n * 4);
        row_base.alloc(n * 8); row_count.alloc(n * 4); keep.alloc(n);
        merged_k.alloc(n);
        HIP_CHECK(hipMemset(merged_k.p, 0, n));
        stb.alloc(n_static ? n : 1, n_static);
        op = OutParts{keypfx.as<uint64_t>(), key_addr.as<uint64_t>(), token.as<int64_t>(),
                      stb.st, klen.as<uint16_t>(),
                      pdel_mfda.as<int64_t>(),
                      pdel_ldt.as<uint32_t>(), row_base.as<uint64_t>(), row_count.as<uint32_t>(),
                      keep.as<uint8_t>(), merged_k.as<uint8_t>()};
    }
};

// allocate an UnfCols arena for n unfiltereds
struct UnfColsBuf {
    DevBuf ck, rkind, flags, live_ts, live_ttl, live_let, rdel_mfda, rdel_ldt,
        start_mfda, start_ldt, cell_ts, cell_ldt, cell_ttl, val_addr, val_len, ck_addr, ck_len,
        cell_flags, ck_count;
    DevBuf cpx_present, cpx_del_mfda, cpx_del_ldt, cpx_start, cpx_count;  // per (row, complex column)
    DevBuf cx_ts, cx_ldt, cx_ttl, cx_flags, cx_pa, cx_pl, cx_va, cx_vl;  // cell arena
    UnfCols uc{};
    // cell arena sized AFTER the counting pass (arena capacity = total
    // complex cells); per-row arrays are allocated with the rows
    void alloc_cpx_arena(uint64_t cells) {
        if (!cells) cells = 1;
        cx_ts.alloc(cells * 8); cx_ldt.alloc(cells * 4); cx_ttl.alloc(cells * 4);
        cx_flags.alloc(cells); cx_pa.alloc(cells * 8); cx_pl.alloc(cells * 4);
        cx_va.alloc(cells * 8); cx_vl.alloc(cells * 4);
        uc.cpx = UnfCols::CpxCells{cx_ts.as<int64_t>(), cx_ldt.as<uint32_t>(), cx_ttl.as<int32_t>(),
                                   cx_flags.as<uint8_t>(), cx_pa.as<uint64_t>(), cx_pl.as<uint32_t>(),
                                   cx_va.as<uint64_t>(), cx_vl.as<uint32_t>()};
    }
    void alloc(uint64_t n, uint32_t n_cols, uint32_t n_ck, uint32_t n_cpx = 0) {
        if (!n) n = 1;
        uint64_t nc = n * n_cols;
        uint64_t nk = n * (n_ck ? n_ck : 1);
        ck.alloc(nk * 8); rkind.alloc(n); flags.alloc(n); live_ts.alloc(n * 8);
        live_ttl.alloc(n * 4); live_let.alloc(n * 8); rdel_mfda.alloc(n * 8);
        rdel_ldt.alloc(n * 4); start_mfda.alloc(n * 8); start_ldt.alloc(n * 4);
        cell_ts.alloc(nc * 8); cell_ldt.alloc(nc * 4); cell_ttl.alloc(nc * 4);
        val_addr.alloc(nc * 8); val_len.alloc(nc * 4); cell_flags.alloc(nc);
        ck_addr.alloc(nk * 8); ck_len.alloc(nk * 4); ck_count.alloc(n);
        if (n_cpx) {
            uint64_t nx = n * n_cpx;
            cpx_present.alloc(nx);
            cpx_del_mfda.alloc(nx * 8); cpx_del_ldt.alloc(nx * 4);
            cpx_start.alloc(nx * 8); cpx_count.alloc(nx * 4);
        }
        uc = UnfCols{ck.as<uint64_t>(), rkind.as<uint8_t>(), flags.as<uint8_t>(),
                     live_ts.as<int64_t>(), live_ttl.as<int32_t>(), live_let.as<int64_t>(),
                     rdel_mfda.as<int64_t>(), rdel_ldt.as<uint32_t>(), start_mfda.as<int64_t>(),
                     start_ldt.as<uint32_t>(), cell_ts.as<int64_t>(), cell_ldt.as<uint32_t>(),
                     cell_ttl.as<int32_t>(), val_addr.as<uint64_t>(), val_len.as<uint32_t>(),
                     cell_flags.as<uint8_t>(),
                     ck_addr.as<uint64_t>(), ck_len.as<uint32_t>(), ck_count.as<uint8_t>()};
        if (n_cpx) {
            uc.cpx_present = cpx_present.as<uint8_t>();
            uc.cpx_del_mfda = cpx_del_mfda.as<int64_t>();
            uc.cpx_del_ldt = cpx_del_ldt.as<uint32_t>();
            uc.cpx_start = cpx_start.as<uint64_t>();
            uc.cpx_count = cpx_count.as<uint32_t>();
        }
    }
};

struct WriteDeviceOut {
    uint64_t uncompressed_len = 0;
    uint64_t compressed_len = 0;   // final Data.db size
    uint64_t partitions = 0, rows = 0, cells = 0;
    double ms_sizes = 0, ms_serialize = 0, ms_compress = 0, ms_d2h = 0, ms_io = 0;
    uint32_t n_outputs = 1;  // sstables written (more than one only when size-split)
    // totals over several writer runs (routed outputs); start from n_outputs = 0
    void add(const WriteDeviceOut& o) {
        n_outputs += o.n_outputs;
        partitions += o.partitions;
        rows += o.rows;
        cells += o.cells;
        uncompressed_len += o.uncompressed_len;
        compressed_len += o.compressed_len;
        ms_sizes += o.ms_sizes;
        ms_serialize += o.ms_serialize;
        ms_compress += o.ms_compress;
        ms_d2h += o.ms_d2h;
        ms_io += o.ms_io;
    }
};

// The one place chunk-compress kernels are launched (sstable writer and
// gpuc_compress_buffer): m chunks of chunk_len bytes (last one short) from
// d_data -> payload slots of `stride` bytes + per-chunk size and CRC32.
static void launch_chunk_compress(bool snappy, const uint8_t* d_data, uint64_t data_len,
                                  uint8_t* d_slots, uint32_t* d_csize, uint32_t* d_ccrc,
                                  uint32_t m, uint32_t chunk_len, uint32_t stride,
                                  hipStream_t stream) {
    if (snappy)
        hipLaunchKernelGGL(k_snappy_compress_chunks, dim3(m), dim3(WAVE), 0, stream, d_data,
                           data_len, d_slots, d_csize, d_ccrc, m, (const uint32_t*)g_crc256,
                           g_snp_off, g_snp_off_n, chunk_len, stride);
    else
        hipLaunchKernelGGL(k_lz4_compress_wave_t<false>, dim3(m), dim3(WAVE), 0, stream, d_data,
                           data_len, d_slots, d_csize, d_ccrc, m, (const uint32_t*)g_crc256,
                           (uint32_t*)nullptr, chunk_len, stride);
}

// ---------------------------------------------------------------------------
// input front end shared by compact_one, gpuc_scrub and gpuc_verify:
// chunk decode -> schema upload -> parse chain. Every helper issues on the
// stream it is given and adds no synchronisation of its own (exscan_u64
// inside the parse chain synchronises to read its total).
// ---------------------------------------------------------------------------
// Owning handles: destroyed on scope exit, error paths included. Declare a
// Stream BEFORE the DevBufs used on it, so the buffers are released first.
struct Stream {
    hipStream_t s = nullptr;
    Stream() { HIP_CHECK(hipStreamCreate(&s)); }
    ~Stream() { (void)hipStreamDestroy(s); }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() { HIP_CHECK(hipEventCreate(&e)); }
    ~Event() { (void)hipEventDestroy(e); }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    operator hipEvent_t() const { return e; }
};

// synchronise `stream`, then fetch the device error word; each caller maps
// the code to its own message
static unsigned long long read_dev_error(const DevBuf& d_error, hipStream_t stream) {
    unsigned long long err = 0;
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipMemcpy(&err, d_error.p, 8, hipMemcpyDeviceToHost));
    return err;
}
// the collection-type checks of k_parse_rows (codes 19, 26): GPUC_ERR_FORMAT
static void throw_if_collection_parse_error(unsigned long long err) {
    if (err == 19)
        throw format_error("Data.db: a cell path of a collection with int, bigint or timestamp "
                           "keys does not have the width of its key type (parse error code 19)");
    if (err == 26)
        throw format_error("Data.db: a cell of a set column carries a value "
                           "(parse error code 26)");
}

// validated frames -> decoder descriptors. d_comp holds the file's bytes
// from offset comp_lo on; chunk i of the window decodes to d_out + i * chunk_len.
static std::vector<ChunkDesc> chunk_descs(const std::vector<ChunkFrame>& frames,
                                          const uint8_t* d_comp, uint64_t comp_lo,
                                          uint8_t* d_out, uint32_t chunk_len) {
    std::vector<ChunkDesc> chunks;
    chunks.reserve(frames.size());
    for (size_t i = 0; i < frames.size(); i++)
        chunks.push_back({d_comp + (frames[i].off - comp_lo), d_out + i * (uint64_t)chunk_len,
                          frames[i].comp_len, frames[i].out_len});
    return chunks;
}

// The one place chunk-decompress kernels are launched. d_bad (scrub) takes a
// per-chunk failure flag instead of failing the whole input.
static void launch_chunk_decompress(const HCompressionInfo& ci, const DevBuf& d_chunks, size_t n,
                                    const DevBuf& d_error, uint8_t* d_bad, hipStream_t stream) {
    if (!n) return;
    const dim3 grid(lz4_decomp_grid((uint32_t)n, 1));
    if (ci.snappy)
        hipLaunchKernelGGL(k_snappy_decompress_chunks, grid, dim3(WAVE), 0, stream,
                           d_chunks.as<ChunkDesc>(), (uint32_t)n, 1,
                           d_error.as<unsigned long long>(), (const uint32_t*)g_crc256, d_bad,
                           ci.max_comp());
    else
        hipLaunchKernelGGL(k_lz4_decompress_wave, grid, dim3(WAVE), 0, stream,
                           d_chunks.as<ChunkDesc>(), (uint32_t)n, 1,
                           d_error.as<unsigned long long>(), (const uint32_t*)g_crc256, d_bad,
                           ci.max_comp());
}

// whole-file ingest of scrub and verify: upload Data.db and decode every chunk.
// The caller zeroes d_error (and d_bad) on `stream` first; `file` and this
// object outlive the next synchronise of `stream`.
struct DecodedFile {
    DevBuf comp, data, chunks;
    std::vector<ChunkDesc> h_chunks;
    void issue(const HCompressionInfo& ci, const std::vector<ChunkFrame>& frames,
               const bytes& file, const DevBuf& d_error, uint8_t* d_bad, hipStream_t stream) {
        upload(comp, file.data(), file.size(), stream);
        data.alloc(ci.data_len + 16);
        h_chunks = chunk_descs(frames, comp.as<uint8_t>(), 0, data.as<uint8_t>(), ci.chunk_len);
        upload(chunks, h_chunks.data(), h_chunks.size(), stream, 16);
        launch_chunk_decompress(ci, chunks, h_chunks.size(), d_error, d_bad, stream);
    }
};

// device copy of a HostSchema's width arrays
struct DevSchema {
    DevBuf ck_w, col_fixed, static_fixed;
    // hs is read by async copies: it must outlive the next synchronise of `stream`
    SchemaParams upload(const HostSchema& hs, hipStream_t stream,
                        uint32_t column_index_size = 64 * 1024) {
        auto up = [&](DevBuf& d, const std::vector<int32_t>& h) {
            return gpuc::upload(d, h.data(), h.size(), stream, 8);
        };
        SchemaParams sch{};
        sch.n_ck = (uint32_t)hs.ck_widths.size();
        sch.ck_desc = hs.ck_desc_mask();
        sch.ck_w = up(ck_w, hs.ck_widths);
        sch.n_cols = (uint32_t)hs.col_fixed.size();
        sch.col_fixed = up(col_fixed, hs.col_fixed);
        sch.n_cpx = hs.n_cpx;
        sch.counters = hs.counters ? 1u : 0u;
        sch.n_static = (uint32_t)hs.static_fixed.size();
        sch.static_fixed = up(static_fixed, hs.static_fixed);
        sch.column_index_size = column_index_size;
        return sch;
    }
};

// Rows.db keys are the byte-comparable form of the clusterings, which
// ReversedType inverts; the BTI index of a table with a descending clustering
// column is out of scope and refused before any Data.db byte is parsed
static void refuse_bti_desc(const std::vector<std::string>& clustering_types, const char* what) {
    for (auto& t : clustering_types)
        if (ck_type(t).desc)
            throw unsupported_error(std::string(what) + " of a table with a descending clustering "
                                    "column (" + t + ") unsupported: Rows.db keys are the "
                                    "byte-comparable clusterings, which ReversedType inverts");
}

// the writer and the digest kernels decode ascending clustering encodings:
// called once, after the last comparison over `rows` (k_ck_ascending)
static void restore_ck_ascending(const OutParts& op, const UnfColsBuf& rows, uint64_t n_groups,
                                 const SchemaParams& sch, hipStream_t stream) {
    if (!sch.ck_desc || !n_groups) return;
    hipLaunchKernelGGL(k_ck_ascending, dim3((uint32_t)((n_groups + 255) / 256)), dim3(256), 0,
                       stream, op, rows.uc, n_groups, sch);
}

// the collection-type masks of a schema's complex columns (kernels_rows.hip)
static CpxTypes cpx_types(const HostSchema& hs) {
    return CpxTypes{hs.cpx_key_signed_mask(), hs.cpx_key_w8_mask(), hs.cpx_is_set_mask()};
}

// a source's own header (its counts and its maps into the union) in its SrcDesc2
static void set_src_columns(SrcDesc2& sd, const SourceColumns& sc) {
    sd.n_cols = sc.n_cols;
    sd.n_cpx = sc.n_cpx;
    sd.n_static = sc.n_static;
    std::copy(sc.col_map.begin(), sc.col_map.end(), sd.col_map);
    std::copy(sc.cpx_map.begin(), sc.cpx_map.end(), sd.cpx_map);
    std::copy(sc.static_map.begin(), sc.static_map.end(), sd.static_map);
}
// the single-source callers: the source's header IS the schema
static void set_src_identity(SrcDesc2& sd, const SchemaParams& sch) {
    sd.n_cols = sch.n_cols;
    sd.n_cpx = sch.n_cpx;
    sd.n_static = sch.n_static;
    for (uint32_t i = 0; i < 63; i++) sd.col_map[i] = sd.cpx_map[i] = sd.static_map[i] = (uint8_t)i;
}

// parsed input: per-partition columns, static rows, the unfiltered arena and
// the complex-cell bases
struct ParsedInput {
    DevBuf pdm, pdl, rcnt, rbase, kaddr, cpxtot, cpxbase;
    StaticColsBuf st;
    UnfColsBuf rows;
    ParsedCols pc{};
    uint64_t total_rows = 0, total_cpx = 0;
    CpxTypes cx{};  // of the schema it was parsed under; the merge reads it too
};
// The parse chain for n_srcs sources over `total` partitions. Pass A
// (k_parse_count) fills the merge records and partition columns; count_only
// (verify) stops there and leaves pc.st empty. Then row counts are scanned
// into row bases, the complex cells are counted and scanned when the schema
// has a complex column, and pass B (k_parse_rows) decodes the rows. The
// caller sets in.cx (cpx_types of the schema) first when the schema has typed
// or set collection columns.
// CONTRACT: a partition that either pass rejects ends its walk at once and
// leaves its remaining row slots (and the counts of the column it stopped in)
// unwritten. Every caller reads d_error (read_dev_error) after this returns
// and before ANYTHING consumes in.rows or in.pc; compaction, scrub and verify
// all throw there.
static void parse_input(ParsedInput& in, const DevBuf& d_srcs, uint32_t n_srcs, uint64_t total,
                        const DevBuf& d_recs, const SchemaParams& sch, const DevBuf& d_error,
                        const DevBuf& d_rows_in, bool count_only, hipStream_t stream) {
    ParsedCols& pc = in.pc;
    in.pdm.alloc(total * 8 + 8); pc.pdel_mfda = in.pdm.as<int64_t>();
    in.pdl.alloc(total * 4 + 8); pc.pdel_ldt = in.pdl.as<uint32_t>();
    in.rcnt.alloc(total * 4 + 8); pc.row_count = in.rcnt.as<uint32_t>();
    in.rbase.alloc(total * 8 + 8); pc.row_base = in.rbase.as<uint64_t>();
    in.kaddr.alloc(total * 8 + 8); pc.key_addr = in.kaddr.as<uint64_t>();
    if (!count_only) {
        in.st.alloc(sch.n_static ? total : 1, sch.n_static);
        pc.st = in.st.st;
    }
    const dim3 grid((uint32_t)((total + 255) / 256)), block(256);
    const SrcDesc2* srcs = d_srcs.as<SrcDesc2>();
    unsigned long long* err = d_error.as<unsigned long long>();
    if (total)
        hipLaunchKernelGGL(k_parse_count, grid, block, 0, stream, srcs, n_srcs, (uint32_t)total,
                           d_recs.as<MRec>(), pc, sch, err);
    if (count_only) return;
    if (total)
        hipLaunchKernelGGL(k_widen_u32, grid, block, 0, stream, pc.row_count, pc.row_base, total);
    in.total_rows = exscan_u64(pc.row_base, total, stream);
    // a partition that pass A rejected has no row count: the total is
    // garbage then, and pass B would write past the rows it was given. The
    // caller reads the same error word and reports it.
    if (read_dev_error(d_error, stream)) return;
    in.rows.alloc(in.total_rows, sch.n_cols, sch.n_ck, sch.n_cpx);
    if (!total) return;
    // byte-ordered tables launch the walk without the collection checks
    const bool typed = in.cx.key_signed || in.cx.is_set;
    auto rows_pass = [&](const uint64_t* cpx_bases) {
        hipLaunchKernelGGL(typed ? k_parse_rows<true> : k_parse_rows<false>, grid, block, 0, stream,
                           srcs, n_srcs, (uint32_t)total, pc, in.rows.uc, sch, in.cx, err,
                           d_rows_in.as<unsigned long long>(), cpx_bases);
    };
    if (sch.n_cpx) {
        // counting pass: full walk, per-partition complex-cell totals, which
        // size the cell arena and become each partition's base in it
        in.cpxtot.alloc(total * 4 + 8);
        pc.cpx_total = in.cpxtot.as<uint32_t>();
        rows_pass(nullptr);
        HIP_CHECK(hipMemsetAsync(d_rows_in.p, 0, 8, stream));  // recounted by the fill pass
        in.cpxbase.alloc(total * 8 + 8);
        hipLaunchKernelGGL(k_widen_u32, grid, block, 0, stream, pc.cpx_total,
                           in.cpxbase.as<uint64_t>(), total);
        in.total_cpx = exscan_u64(in.cpxbase.as<uint64_t>(), total, stream);
        in.rows.alloc_cpx_arena(in.total_cpx);
    }
    rows_pass(sch.n_cpx ? in.cpxbase.as<uint64_t>() : nullptr);
}

// ---------------------------------------------------------------------------
// group/reconcile back end shared by compact_one (data pass and
// garbage-collect source pass) and gpuc_scrub: sorted records -> groups ->
// per-group row sums -> output buffers -> k_reconcile_rows. Separate steps, so
// a caller can poll for cancellation, trace and record events between them.
// Every step issues on the stream it is given, and none launches an empty grid.
// ---------------------------------------------------------------------------
struct Groups {
    const MRec* sorted = nullptr;  // n_recs records in DecoratedKey order
    uint64_t n_recs = 0;
    DevBuf head, start, count, rows;
    uint64_t n = 0;           // groups (distinct partition keys)
    uint64_t total_rows = 0;  // upper bound of the reconciled unfiltereds
};
// step 1: group starts and g.n; synchronises to read the count
static void find_groups(Groups& g, const MRec* d_sorted, uint64_t n_recs, const KeyLut& lut,
                        hipStream_t stream) {
    g.sorted = d_sorted;
    g.n_recs = n_recs;
    g.head.alloc(n_recs * 8 + 8);
    g.start.alloc(n_recs * 8 + 8);
    g.count.alloc(8);
    if (n_recs) {
        const dim3 grid((uint32_t)((n_recs + 255) / 256)), block(256);
        hipLaunchKernelGGL(k_group_heads, grid, block, 0, stream, d_sorted, n_recs,
                           g.head.as<uint64_t>(), lut);
        exscan_u64(g.head.as<uint64_t>(), n_recs, stream);
        hipLaunchKernelGGL(k_group_starts2, grid, block, 0, stream, d_sorted, n_recs,
                           g.head.as<uint64_t>(), g.start.as<uint64_t>(), g.count.as<uint64_t>(),
                           lut);
    } else {
        HIP_CHECK(hipMemsetAsync(g.count.p, 0, 8, stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipMemcpy(&g.n, g.count.p, 8, hipMemcpyDeviceToHost));
}
// step 2: rows of each group summed over its sources, scanned into row bases
// (g.rows) and g.total_rows; exscan_u64 synchronises
static void scan_group_rows(Groups& g, const DevBuf& d_srcbases, const ParsedCols& pc,
                            hipStream_t stream) {
    g.rows.alloc(g.n * 8 + 8);
    if (g.n)
        hipLaunchKernelGGL(k_group_row_sums, dim3((uint32_t)((g.n + 255) / 256)), dim3(256), 0,
                           stream, g.sorted, g.start.as<uint64_t>(), g.n, g.n_recs,
                           d_srcbases.as<uint32_t>(), pc, g.rows.as<uint64_t>());
    g.total_rows = exscan_u64(g.rows.as<uint64_t>(), g.n, stream);
}
// step 3: the reconciled output. alloc() sizes it from the groups and resets
// the stats; launch_reconcile() fills it. Two calls, because compact_one sets
// up its purge parameters and records its reconcile event between them.
struct Reconciled {
    OutPartsBuf parts;
    UnfColsBuf rows;
    DevBuf stats;  // OutStats
    void alloc(const Groups& g, const SchemaParams& sch, uint64_t total_in_cpx,
               hipStream_t stream) {
        parts.alloc(g.n ? g.n : 1, sch.n_static);
        rows.alloc(g.total_rows, sch.n_cols, sch.n_ck, sch.n_cpx);
        if (sch.n_cpx) rows.alloc_cpx_arena(total_in_cpx);
        stats.alloc(sizeof(OutStats));
        init_outstats(stats, stream);
    }
};
// n_sources picks the kernel's per-group version capacity
static void launch_reconcile(const Groups& g, int n_sources, const DevBuf& d_srcbases,
                             const ParsedInput& in, Reconciled& out, const SchemaParams& sch,
                             const PurgeParams2& pp, const DevBuf& d_error, hipStream_t stream) {
    if (!g.n) return;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((uint32_t)((g.n + 255) / 256)), dim3(256), 0, stream,
                           g.sorted, g.start.as<uint64_t>(), g.n, g.n_recs,
                           d_srcbases.as<uint32_t>(), in.pc, in.rows.uc, out.parts.op,
                           out.rows.uc, g.rows.as<uint64_t>(), sch, in.cx, pp,
                           out.stats.as<OutStats>(),
                           d_error.as<unsigned long long>());
    };
    if (n_sources <= 8) launch(k_reconcile_rows<8>);
    else if (n_sources <= 16) launch(k_reconcile_rows<16>);
    else launch(k_reconcile_rows<64>);
}

// merged-context arena of a counter table: capacity = total input counter
// bytes (any k-way merge result is bounded by the sum of its inputs).
// Synchronises to read the total.
static uint64_t counter_arena_cap(const ParsedInput& in, uint32_t n_cols, hipStream_t stream) {
    DevBuf d_sum;
    d_sum.alloc(8);
    HIP_CHECK(hipMemsetAsync(d_sum.p, 0, 8, stream));
    uint64_t n_cells = in.total_rows * n_cols;
    if (n_cells)
        hipLaunchKernelGGL(k_sum_vallen, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0,
                           stream, in.rows.uc, n_cells, d_sum.as<unsigned long long>());
    unsigned long long total_ctr = 0;
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipMemcpy(&total_ctr, d_sum.p, 8, hipMemcpyDeviceToHost));
    return total_ctr + 64;
}

// capacity of the tombstone local-deletion-time list k_collect_rows appends to
static uint32_t tomb_list_cap(uint64_t rows, uint64_t cpx_cells, uint64_t parts,
                              const SchemaParams& sch) {
    return (uint32_t)std::min<uint64_t>(rows * ((uint64_t)sch.n_cols + sch.n_cpx + 2) + cpx_cells +
                                            parts * ((uint64_t)sch.n_static + 2) + 1024,
                                        400000000ull);
}

// OutStats keeps its signed minima and maxima sign-flipped (i64 ^ SIGN, as
// u64); `none` is what a slot nothing was folded into decodes to
static int64_t unflip(unsigned long long v) { return (int64_t)(v ^ 0x8000000000000000ULL); }
static int64_t unflip(unsigned long long v, unsigned long long untouched, int64_t none) {
    return v == untouched ? none : unflip(v);
}

// Header of freshly built rows (flush, generate): SerializationHeader.make
// takes the EncodingStats of the rows, so k_collect_rows runs once ahead of
// the writer, the minima are read back (synchronises), and the stats are
// re-initialised for the writer's own collect. n_cols is the cell stride of
// `rows`.
static HeaderStats fresh_rows_header(const OutPartsBuf& opb, const UnfColsBuf& rows,
                                     uint64_t n_parts, uint32_t n_cols, uint32_t n_cpx,
                                     DevBuf& d_stats, DevBuf& d_tomb, uint32_t tomb_cap,
                                     hipStream_t stream) {
    d_stats.alloc(sizeof(OutStats));
    init_outstats(d_stats, stream);
    d_tomb.alloc((uint64_t)tomb_cap * 4);
    hipLaunchKernelGGL(k_collect_rows, dim3((uint32_t)((n_parts + 255) / 256)), dim3(256), 0,
                       stream, opb.op, rows.uc, n_parts, n_cols, n_cpx, d_stats.as<OutStats>(),
                       d_tomb.as<uint32_t>(), tomb_cap);
    OutStats hs0;
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipMemcpy(&hs0, d_stats.p, sizeof(OutStats), hipMemcpyDeviceToHost));
    HeaderStats hs;
    hs.min_ts = unflip(hs0.min_ts_flip, ~0ull, TIMESTAMP_EPOCH);
    hs.min_ldt = unflip(hs0.min_ldt_flip, ~0ull, DELETION_TIME_EPOCH);
    if (hs.min_ldt == NO_DELETION_TIME) hs.min_ldt = DELETION_TIME_EPOCH;
    hs.min_ttl = hs0.min_ttl == 0xFFFFFFFFu ? 0 : (int32_t)hs0.min_ttl;
    init_outstats(d_stats, stream);
    return hs;
}

// ---------------------------------------------------------------------------
// shared device->files writer: sizes/scan -> serialize interleaved with
// compress -> slab drain -> component tail. `d_stats` is the device OutStats
// already filled by reconcile (or reset by fresh_rows_header); `types` and
// sp.hs give the Statistics.db header.
// ---------------------------------------------------------------------------
struct OutputOptions {
    std::string base;  // <dir>/<version>-<generation>-<format>
    bool snappy = false, bti = false;
    uint32_t chunk_len = CHUNK_LEN;
    int wslot = 0;  // pinned-arena set (shards run two at a time)
};

// the one place OutStats becomes Statistics.db input (the rest of OutMeta —
// key hashes, first/last key, tombstone histogram, ratio — is the caller's)
static void fill_meta_from_stats(OutMeta& m, const OutStats& hst, const HeaderStats& hs,
                                 const TableTypes& types) {
    m.hdr_min_ts = hs.min_ts;
    m.hdr_min_ldt = hs.min_ldt;
    m.hdr_min_ttl = hs.min_ttl;
    m.types = types;
    const bool no_ts = hst.min_ts_flip == ~0ull;
    m.min_timestamp = no_ts ? 0 : unflip(hst.min_ts_flip);
    m.max_timestamp = no_ts ? 0 : unflip(hst.max_ts_flip);
    m.min_ldt = unflip(hst.min_ldt_flip, ~0ull, NO_DELETION_TIME);
    m.max_ldt = unflip(hst.max_ldt_flip, 0, 0);
    m.min_ttl = hst.min_ttl == 0xFFFFFFFFu ? 0 : (int32_t)hst.min_ttl;
    m.max_ttl = (int32_t)hst.max_ttl;
    m.total_rows = hst.rows_out;
    m.total_cells = hst.total_cells;
    m.has_partition_deletions = hst.has_partition_deletions != 0;
    memcpy(m.part_size_hist, hst.part_size_hist, sizeof(m.part_size_hist));
    memcpy(m.cells_hist, hst.cells_hist, sizeof(m.cells_hist));
}

// One output's device image, ready to leave the device: what the drain and
// the component tail consume. The buffers stay the caller's.
struct OutputImage {
    uint64_t g0 = 0, g1 = 0;  // its groups [g0, g1)
    uint64_t total_unc = 0, total_idx = 0;
    uint32_t n_chunks = 0;
    const DevBuf *slots = nullptr, *csize = nullptr, *ccrc = nullptr;  // compressed chunks
    const DevBuf *out_index = nullptr, *bloom = nullptr;
    uint8_t* h_index = nullptr;  // pinned, total_idx bytes
    uint64_t words = 0;          // bloom words
    HBloomSpec bs{};
    OutStats hst{};
    const std::vector<Event>* ev_c = nullptr;  // per slab: its chunks are compressed
    bool index_late = false;  // Index.db image is fetched after the drain (gated on ev2)
};

// stages 3 and 4 of the writer: slab drain of the compressed chunks into
// Data.db on `cstream`, then the component tail. Returns with both streams
// idle and every component of opt.base written.
static void drain_and_finish(const OutputImage& im, const OutParts& op, const SerParams2& sp,
                             const DevBuf& d_tomb, uint32_t tomb_cap, const TableTypes& types,
                             const OutputOptions& opt, hipStream_t stream, hipStream_t cstream,
                             hipEvent_t ev2, hipEvent_t ev4, WriteDeviceOut& w) {
    const std::string& out_base = opt.base;
    const bool snappy_out = opt.snappy, bti_out = opt.bti;
    const int wslot = opt.wslot;
    const uint32_t OCL = opt.chunk_len;
    const uint32_t SLOT_STRIDE = snappy_out ? snp_slot_stride(OCL) : lz4_slot_stride(OCL);
    const uint32_t SLAB = (512u << 20) / OCL;
    const uint32_t n_chunks = im.n_chunks;
    const uint32_t n_slabs = n_chunks ? (n_chunks + SLAB - 1) / SLAB : 0;
    const uint64_t total_unc = im.total_unc, total_idx = im.total_idx, words = im.words;
    uint8_t* const h_index = im.h_index;
    const OutStats& hst = im.hst;
    const HBloomSpec& bs = im.bs;
    // ==== stage 3: slab drain ====
    std::string data_path = out_base + "-Data.db";
    write_file(data_path, nullptr, 0);  // create/truncate so writers can pwrite into it
    const uint64_t worst_slab = (uint64_t)SLAB * ((uint64_t)SLOT_STRIDE + 4);
    const int NSLOTS = 4;
    uint8_t* h_slab0 = (uint8_t*)g_pin_out[wslot][0].get(worst_slab * NSLOTS);
    if (!h_slab0) throw std::runtime_error("pinned out alloc failed");
    DevBuf d_gat[2], d_foff[2];
    if (n_slabs) {
        d_gat[0].alloc(worst_slab); d_gat[1].alloc(worst_slab);
        d_foff[0].alloc((uint64_t)SLAB * 8); d_foff[1].alloc((uint64_t)SLAB * 8);
    }
    std::vector<uint32_t> cs(n_chunks);
    std::vector<uint64_t> foff_h[2];
    foff_h[0].resize(SLAB); foff_h[1].resize(SLAB);
    std::future<void> wfut[NSLOTS];
    double t_drain0 = 0, t_drain1 = 0;
    {
        struct timespec tsd; clock_gettime(CLOCK_MONOTONIC, &tsd);
        t_drain0 = tsd.tv_sec * 1e3 + tsd.tv_nsec / 1e6;
    }
    uint64_t file_off = 0;
    double tw_comp = 0, tw_d2h = 0, tw_wfut = 0;  // drain wait breakdown (GPUC_TRACE)
    auto wallm = []() {
        struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t);
        return t.tv_sec * 1e3 + t.tv_nsec / 1e6;
    };
    for (uint32_t i = 0; i < n_slabs; i++) {
        uint32_t cb = i * SLAB, m = std::min(SLAB, n_chunks - cb);
        HIP_CHECK(hipStreamWaitEvent(cstream, (*im.ev_c)[i], 0));
        HIP_CHECK(hipMemcpyAsync(cs.data() + cb, im.csize->as<uint32_t>() + cb, (uint64_t)m * 4,
                                 hipMemcpyDeviceToHost, cstream));
        double tq0 = wallm();
        HIP_CHECK(hipStreamSynchronize(cstream));
        tw_comp += wallm() - tq0;
        auto& fo = foff_h[i & 1];
        uint64_t acc = 0;
        for (uint32_t j = 0; j < m; j++) { fo[j] = acc; acc += cs[cb + j]; }
        uint64_t slab_bytes = acc + (uint64_t)m * 4;
        HIP_CHECK(hipMemcpyAsync(d_foff[i & 1].p, fo.data(), (uint64_t)m * 8,
                                 hipMemcpyHostToDevice, cstream));
        hipLaunchKernelGGL(k_chunk_gather, dim3(m), dim3(WAVE), 0, cstream,
                           im.slots->as<uint8_t>() + (uint64_t)cb * SLOT_STRIDE,
                           im.csize->as<uint32_t>() + cb, im.ccrc->as<uint32_t>() + cb,
                           d_foff[i & 1].as<uint64_t>(), d_gat[i & 1].as<uint8_t>(), m,
                           SLOT_STRIDE);
        int slot = (int)(i % NSLOTS);
        double tq1 = wallm();
        if (wfut[slot].valid()) wfut[slot].get();  // pinned buffer free again
        tw_wfut += wallm() - tq1;
        uint8_t* hbuf = h_slab0 + (uint64_t)slot * worst_slab;
        HIP_CHECK(hipMemcpyAsync(hbuf, d_gat[i & 1].p, slab_bytes, hipMemcpyDeviceToHost, cstream));
        double tq2 = wallm();
        HIP_CHECK(hipStreamSynchronize(cstream));
        tw_d2h += wallm() - tq2;
        uint64_t off0 = file_off;
        wfut[slot] = std::async(std::launch::async, [=]() {
            pwrite_range(data_path, hbuf, slab_bytes, off0, 4);
        });
        file_off += slab_bytes;
    }
    {
        double tq3 = wallm();
        for (int sfin = 0; sfin < NSLOTS; sfin++)
            if (wfut[sfin].valid()) wfut[sfin].get();
        tw_wfut += wallm() - tq3;
    }
    if (g_trace)
        fprintf(stderr, "[drain] slabs=%u wait_compress=%.0fms wait_d2h=%.0fms wait_write=%.0fms\n",
                n_slabs, tw_comp, tw_d2h, tw_wfut);
    {
        struct timespec tsd; clock_gettime(CLOCK_MONOTONIC, &tsd);
        t_drain1 = tsd.tv_sec * 1e3 + tsd.tv_nsec / 1e6;
    }
    w.compressed_len = file_off;
    TR("wsd: drain done");
    if (im.index_late) {
        // segmented mode: the index image drains AFTER the data drain — an
        // earlier enqueue would gate the whole in-order cstream on ev2 (the
        // LAST serialize segment) and collapse the drain to a tail
        HIP_CHECK(hipStreamWaitEvent(cstream, ev2, 0));
        HIP_CHECK(hipMemcpyAsync(h_index, im.out_index->p, total_idx, hipMemcpyDeviceToHost, cstream));
        HIP_CHECK(hipStreamSynchronize(cstream));
    }
    HIP_CHECK(hipEventRecord(ev4, stream));

    // ==== stage 4: component tail (bytes decided in sstable_out.h) ====
    {
        std::vector<uint8_t> h_bloom(words * 8);
        std::vector<uint32_t> h_crc(n_chunks);
        TR("wsd: tail vectors");
        HIP_CHECK(hipMemcpy(h_bloom.data(), im.bloom->p, words * 8, hipMemcpyDeviceToHost));
        TR("wsd: bloom d2h");
        if (n_chunks)
            HIP_CHECK(hipMemcpy(h_crc.data(), im.ccrc->p, (uint64_t)n_chunks * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipStreamSynchronize(cstream));
        TR("wsd: tail synced");
        // digest fold and the Summary.db index walk are independent of the
        // meta build: run all three concurrently (tail was serial: ~145 ms)
        std::future<uint32_t> fut_digest =
            std::async(std::launch::async, [&]() { return fold_digest(h_crc, cs); });
        std::future<bytes> fut_summary;
        if (!bti_out)
            fut_summary = std::async(std::launch::async,
                                     [&]() { return summary_db(h_index, total_idx); });

        std::vector<uint32_t> tombs;
        if (hst.tomb_count) {
            uint64_t nt = std::min<uint64_t>(hst.tomb_count, tomb_cap);
            tombs.resize(nt);
            HIP_CHECK(hipMemcpy(tombs.data(), d_tomb.p, nt * 4, hipMemcpyDeviceToHost));
            if (hst.tomb_count > tomb_cap)
                throw std::runtime_error("tombstone list overflow (internal cap)");
        }
        OutMeta m{};
        {
            // per-partition key hashes for the COMPACTION HLL (device-hashed,
            // filtered to kept partitions on host)
            const uint64_t n_groups = im.g1 - im.g0;
            DevBuf d_kh;
            d_kh.alloc(n_groups * 8 + 8);
            uint32_t blocks = (uint32_t)((n_groups + 255) / 256);
            if (n_groups)
                hipLaunchKernelGGL(k_key_hash2, dim3(blocks), dim3(256), 0, stream, op,
                                   im.g1, d_kh.as<uint64_t>(), im.g0);
            std::vector<uint64_t> kh(n_groups);
            std::vector<uint8_t> keep(n_groups);
            if (n_groups) {
                HIP_CHECK(hipStreamSynchronize(stream));
                HIP_CHECK(hipMemcpy(kh.data(), d_kh.p, n_groups * 8, hipMemcpyDeviceToHost));
                HIP_CHECK(hipMemcpy(keep.data(), op.keep + im.g0, n_groups, hipMemcpyDeviceToHost));
            }
            m.key_hashes.reserve(n_groups);
            for (uint64_t g2 = 0; g2 < n_groups; g2++)
                if (keep[g2]) m.key_hashes.push_back(kh[g2]);
        }
        fill_meta_from_stats(m, hst, sp.hs, types);
        for (uint32_t tv : tombs) m.tomb_hist[tv]++;
        m.compression_ratio = total_unc ? (double)(w.compressed_len - (uint64_t)n_chunks * 4) / (double)total_unc : -1.0;
        if (hst.partitions_out) {
            uint64_t fg = hst.first_group, lg = hst.last_group;
            for (int which = 0; which < 2; which++) {
                uint64_t g = which ? lg : fg;
                uint64_t ka;
                uint16_t kl;
                HIP_CHECK(hipMemcpy(&ka, op.key_addr + g, 8, hipMemcpyDeviceToHost));
                HIP_CHECK(hipMemcpy(&kl, op.klen + g, 2, hipMemcpyDeviceToHost));
                bytes kb(kl);
                HIP_CHECK(hipMemcpy(kb.data(), (const void*)ka, kl, hipMemcpyDeviceToHost));
                (which ? m.last_key : m.first_key) = kb;
            }
        }
        TR("wsd: meta built");
        // Digest = CRC of the whole Data.db, folded from per-chunk CRCs in
        // the async above (CRC concatenation is associative over (crc, len))
        uint32_t digest = fut_digest.get();

        TR("wsd: digest done");
        struct timespec ts0, ts1;
        clock_gettime(CLOCK_MONOTONIC, &ts0);
        if (bti_out) {
            bti::bytes parts_img, rows_img;
            std::vector<int32_t> ckw;
            for (auto& t : types.clustering_types) ckw.push_back(type_width(t));
            build_bti_from_index_image(h_index, total_idx, total_unc, ckw, &parts_img, &rows_img);
            write_file(out_base + "-Partitions.db", parts_img);
            write_file(out_base + "-Rows.db", rows_img);
        } else {
            write_file_parallel(out_base + "-Index.db", h_index, total_idx, 4);
        }
        write_file(out_base + "-Filter.db", filter_db(bs.k, h_bloom));
        write_file(out_base + "-CompressionInfo.db",
                   compression_info_db(snappy_out, OCL, total_unc, cs));
        write_file(out_base + "-Digest.crc32", digest_text(digest));
        write_file(out_base + "-Statistics.db", serialize_statistics_out(m));
        if (!bti_out) write_file(out_base + "-Summary.db", fut_summary.get());
        write_file(out_base + "-TOC.txt", toc_text(bti_out));
        clock_gettime(CLOCK_MONOTONIC, &ts1);
        TR("wsd: components written");
        // residual (non-overlapped) component writes + the Data.db drain tail
        w.ms_io = (ts1.tv_sec - ts0.tv_sec) * 1e3 + (ts1.tv_nsec - ts0.tv_nsec) / 1e6;
        w.ms_d2h = t_drain1 - t_drain0;  // slab drain wall (overlaps compress)
    }
}

static WriteDeviceOut write_sstable_device(const OutParts& op, const UnfColsBuf& rows,
                                           uint64_t n_groups, SerParams2 sp, DevBuf& d_stats,
                                           DevBuf& d_tomb, uint32_t tomb_cap,
                                           const TableTypes& types, const OutputOptions& opt,
                                           hipStream_t stream) {
    WriteDeviceOut w;
    if (!chunk_len_supported(opt.chunk_len))
        throw unsupported_error("unsupported output chunk_length " + std::to_string(opt.chunk_len) +
                                CHUNK_LEN_WHY);
    const std::string& out_base = opt.base;
    const bool snappy_out = opt.snappy, bti_out = opt.bti;
    const int wslot = opt.wslot;
    const uint32_t OCL = opt.chunk_len;
    const uint32_t SLOT_STRIDE = snappy_out ? snp_slot_stride(OCL) : lz4_slot_stride(OCL);
    TR("wsd: enter");
    static const std::vector<int64_t> ps_off_h = est_hist_offsets(155);
    static const std::vector<int64_t> ch_off_h = est_hist_offsets(118);
    DevBuf d_ps_off, d_ch_off;
    d_ps_off.alloc(ps_off_h.size() * 8);
    d_ch_off.alloc(ch_off_h.size() * 8);
    HIP_CHECK(hipMemcpyAsync(d_ps_off.p, ps_off_h.data(), ps_off_h.size() * 8, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_ch_off.p, ch_off_h.data(), ch_off_h.size() * 8, hipMemcpyHostToDevice, stream));

    // cstream drains finished output (below); declared ahead of the buffers it reads
    Stream cstream;
    Event ev0, ev1, ev2, ev3, ev4;

    // ==== stage 1: size and scan ====
    // ---- collect stats (needed before bloom sizing) ----
    {
        uint64_t blocks = (n_groups + 255) / 256;
        hipLaunchKernelGGL(k_collect_rows, dim3((uint32_t)blocks), dim3(256), 0, stream, op,
                           rows.uc, n_groups, sp.sch.n_cols, sp.sch.n_cpx, d_stats.as<OutStats>(),
                           d_tomb.as<uint32_t>(), tomb_cap);
    }

    // ---- sizes + scans ----
    HIP_CHECK(hipEventRecord(ev0, stream));
    DevBuf d_psize, d_isize, d_nblocks, d_infsz;
    d_psize.alloc(n_groups * 8);
    d_isize.alloc(n_groups * 8);
    d_nblocks.alloc(n_groups * 4);
    d_infsz.alloc(n_groups * 8);
    {
        uint64_t blocks = (n_groups + 255) / 256;
        hipLaunchKernelGGL(k_sizes_rows, dim3((uint32_t)blocks), dim3(256), 0, stream, op,
                           rows.uc, n_groups, sp, d_psize.as<uint64_t>(), d_isize.as<uint64_t>(),
                           d_nblocks.as<uint32_t>(), d_infsz.as<uint64_t>(),
                           d_stats.as<OutStats>(), d_ps_off.as<int64_t>(), (int32_t)ps_off_h.size(),
                           d_ch_off.as<int64_t>(), (int32_t)ch_off_h.size());
    }
    uint64_t total_unc = exscan_u64(d_psize.as<uint64_t>(), n_groups, stream);
    {
        uint64_t blocks = (n_groups + 255) / 256;
        hipLaunchKernelGGL(k_index_sizes_rows, dim3((uint32_t)blocks), dim3(256), 0, stream,
                           op, n_groups, sp, d_psize.as<uint64_t>(), d_nblocks.as<uint32_t>(),
                           d_infsz.as<uint64_t>(), d_isize.as<uint64_t>());
    }
    uint64_t total_idx = exscan_u64(d_isize.as<uint64_t>(), n_groups, stream);

    OutStats hst;
    HIP_CHECK(hipStreamSynchronize(stream));
    TR("wsd: sizes synced");
    HIP_CHECK(hipMemcpy(&hst, d_stats.p, sizeof(OutStats), hipMemcpyDeviceToHost));
    w.partitions = hst.partitions_out;
    w.rows = hst.rows_out;
    w.cells = hst.total_cells;

    // ==== stage 2: serialize (+ index + bloom) interleaved with compress ====
    HBloomSpec bs = bloom_spec_001();
    uint64_t num_bits = w.partitions * (uint64_t)bs.buckets + 20;
    uint64_t words = num_bits ? ((num_bits - 1) >> 6) + 1 : 1;
    DevBuf d_out_data, d_out_index, d_bloom;
    d_out_data.alloc(total_unc);
    d_out_index.alloc(total_idx);
    d_bloom.alloc(words * 8);
    HIP_CHECK(hipMemsetAsync(d_bloom.p, 0, words * 8, stream));
    // ev1 AFTER the bloom memset: segmented serialize (cstream) gates on it
    HIP_CHECK(hipEventRecord(ev1, stream));
    // serialize in SEGMENTS INTERLEAVED with the compress slabs on the MAIN
    // stream (in-order launches are the only synchronization): compress of a
    // byte range starts once the segment covering it has been issued ahead
    // of it, so the drain receives early slabs ~7/8 of a serialize earlier.
    // NEVER a third stream, and nothing ahead of the drain ops on cstream:
    // both alternatives measured -30% whole-step
    // (profiles/r02_drain_regression.md).
    int NSEG = n_groups >= 4096 && total_unc > (256ull << 20) ? 8 : 1;
    if (const char* e = getenv("GPUC_NSEG")) NSEG = std::max(1, std::min(64, atoi(e)));
    if (n_groups < 4096) NSEG = 1;
    std::vector<uint64_t> seg_g(NSEG + 1), seg_end_byte(NSEG);
    if (NSEG > 1) {
        // equal-GROUP segments; only the NSEG-1 boundary byte offsets come
        // back from d_psize (not the whole offset array)
        seg_g[0] = 0;
        seg_g[NSEG] = n_groups;
        for (int j = 1; j < NSEG; j++) seg_g[j] = n_groups * (uint64_t)j / NSEG;
        for (int j = 0; j < NSEG - 1; j++)
            HIP_CHECK(hipMemcpy(&seg_end_byte[j], d_psize.as<uint64_t>() + seg_g[j + 1], 8,
                                hipMemcpyDeviceToHost));
        seg_end_byte[NSEG - 1] = total_unc;
    } else {
        seg_g[0] = 0;
        seg_g[NSEG] = n_groups;
        seg_end_byte[NSEG - 1] = total_unc;
    }
    auto launch_serialize_seg = [&](int j) {
        uint32_t waves_per_block = 4;
        uint64_t gs = seg_g[j], ge = seg_g[j + 1];
        uint64_t blocks = (std::max<uint64_t>(ge - gs, 1) + waves_per_block - 1) / waves_per_block;
        if (ge > gs)
            hipLaunchKernelGGL(k_serialize_rows, dim3((uint32_t)blocks),
                               dim3(WAVE * waves_per_block), 0, stream, op, rows.uc, ge,
                               sp, d_psize.as<uint64_t>(), d_isize.as<uint64_t>(),
                               d_nblocks.as<uint32_t>(), d_infsz.as<uint64_t>(),
                               d_out_data.as<uint8_t>(), d_out_index.as<uint8_t>(),
                               d_bloom.as<uint32_t>(), words * 64, bs.k, gs);
    };
    int seg_issued = 0;
    if (NSEG == 1) {
        launch_serialize_seg(0);
        seg_issued = 1;
        HIP_CHECK(hipEventRecord(ev2, stream));
    }

    // ---- compress + gather + D2H + write: slab-pipelined ----
    // Compress launches for all slabs are enqueued on `stream` back to back;
    // a second stream drains finished slabs (sizes -> local offsets -> gather
    // -> D2H into rotating pinned buffers) while later slabs still compress,
    // and host writer threads pwrite each drained slab into Data.db at its
    // final offset. Output I/O therefore rides under the compress kernel
    // instead of following it.
    if ((total_unc + OCL - 1) / OCL > 0xFFFFFFFFull)
        throw std::runtime_error("output too large for this chunk_length");
    uint32_t n_chunks = (uint32_t)((total_unc + OCL - 1) / OCL);
    const uint32_t SLAB = (512u << 20) / OCL;  // 512 MiB uncompressed per slab (32768 x 16 KiB)
    uint32_t n_slabs = n_chunks ? (n_chunks + SLAB - 1) / SLAB : 0;
    DevBuf d_slots, d_csize, d_ccrc;
    d_slots.alloc((uint64_t)n_chunks * SLOT_STRIDE + 16);
    d_csize.alloc((uint64_t)n_chunks * 4 + 16);
    d_ccrc.alloc((uint64_t)n_chunks * 4 + 16);
    // Index.db image is final right after serialize: drain it early on
    // cstream (NSEG == 1; segmented mode enqueues it after ev2 exists, below)
    uint8_t* h_index = (uint8_t*)g_pin_out[wslot][1].get(total_idx ? total_idx : 1);
    if (!h_index) throw std::runtime_error("pinned out alloc failed");
    if (NSEG == 1) {
        HIP_CHECK(hipStreamWaitEvent(cstream, ev2, 0));
        HIP_CHECK(hipMemcpyAsync(h_index, d_out_index.p, total_idx, hipMemcpyDeviceToHost, cstream));
    }

    std::vector<Event> ev_c(n_slabs);
    for (uint32_t i = 0; i < n_slabs; i++) {
        uint32_t cb = i * SLAB, m = std::min(SLAB, n_chunks - cb);
        if (NSEG > 1) {
            // issue the serialize segments covering this slab's bytes AHEAD
            // of it on the same in-order stream (ordering IS the dependency)
            uint64_t slab_end = std::min<uint64_t>((uint64_t)(cb + m) * OCL, total_unc);
            while (seg_issued < NSEG && (seg_issued ? seg_end_byte[seg_issued - 1] : 0) < slab_end)
                launch_serialize_seg(seg_issued++);
            if (seg_issued == NSEG) {
                HIP_CHECK(hipEventRecord(ev2, stream));
                seg_issued++;  // record ev2 once
            }
        }
        // all kernel arguments shift uniformly per chunk, so a slab launch is
        // just base-offset pointers with a local chunk count
        launch_chunk_compress(snappy_out, d_out_data.as<uint8_t>() + (uint64_t)cb * OCL,
                              total_unc - (uint64_t)cb * OCL,
                              d_slots.as<uint8_t>() + (uint64_t)cb * SLOT_STRIDE,
                              d_csize.as<uint32_t>() + cb, d_ccrc.as<uint32_t>() + cb, m, OCL,
                              SLOT_STRIDE, stream);
        HIP_CHECK(hipEventRecord(ev_c[i], stream));
    }
    if (NSEG > 1 && seg_issued <= NSEG) {
        while (seg_issued < NSEG) launch_serialize_seg(seg_issued++);
        HIP_CHECK(hipEventRecord(ev2, stream));
    }
    HIP_CHECK(hipEventRecord(ev3, stream));  // ev2..ev3: compress (+interleaved serialize) GPU time
    TR("wsd: compress issued");

    OutputImage im;
    im.g0 = 0;
    im.g1 = n_groups;
    im.total_unc = total_unc;
    im.total_idx = total_idx;
    im.n_chunks = n_chunks;
    im.slots = &d_slots;
    im.csize = &d_csize;
    im.ccrc = &d_ccrc;
    im.out_index = &d_out_index;
    im.bloom = &d_bloom;
    im.h_index = h_index;
    im.words = words;
    im.bs = bs;
    im.hst = hst;
    im.ev_c = &ev_c;
    im.index_late = NSEG > 1;
    drain_and_finish(im, op, sp, d_tomb, tomb_cap, types, opt, stream, cstream, ev2, ev4, w);
    w.uncompressed_len = total_unc;
    float t01, t12, t23;
    HIP_CHECK(hipEventElapsedTime(&t01, ev0, ev1));
    HIP_CHECK(hipEventElapsedTime(&t12, ev1, ev2));
    HIP_CHECK(hipEventElapsedTime(&t23, ev2, ev3));
    w.ms_sizes = t01;
    w.ms_serialize = t12;
    w.ms_compress = t23;
    return w;
}

// the writer reads only the OutParts view; a routed output passes a view whose
// keep points at that output's mask, everyone else their buffer's own
static WriteDeviceOut write_sstable_device(const OutPartsBuf& opb, const UnfColsBuf& rows,
                                           uint64_t n_groups, SerParams2 sp, DevBuf& d_stats,
                                           DevBuf& d_tomb, uint32_t tomb_cap,
                                           const TableTypes& types, const OutputOptions& opt,
                                           hipStream_t stream) {
    return write_sstable_device(opb.op, rows, n_groups, sp, d_stats, d_tomb, tomb_cap, types, opt,
                                stream);
}

// ---------------------------------------------------------------------------
// size-capped outputs (gpuc_job.max_output_bytes; MaxSSTableSizeWriter).
// The rule is stated once, next to k_size_cut. The host only chooses how far
// ahead of the unknown cut to serialize and compress (the speculative
// window) and reads one SizeCutResult per window.
// ---------------------------------------------------------------------------
// Window = (cap / ratio) * (1 + margin) + 2 chunks of uncompressed bytes,
// ratio = compressed/uncompressed of the inputs. The default margin is the
// smallest of {0, 0.01, 0.02, 0.05, 0.1} that needed no second window on the
// recorded C2-shaped run (profiles/size_split_bench_ab.json: 0.9% of the
// compressed chunks were past a cut); everything past the cut is waste, and
// a window that falls short is extended, never wrong.
static double size_split_margin() {
    if (const char* e = getenv("GPUC_SPLIT_MARGIN")) return std::max(0.0, atof(e));
    return 0.01;
}

// compressed chunks of the output being planned; reused from one output to
// the next (chunks restart at every output's first byte)
struct CutPlan {
    DevBuf slots, csize, ccrc, disk, res;
    uint32_t cap_chunks = 0;   // allocated chunk slots
    uint32_t chunks_done = 0;  // complete chunks compressed and scanned
    uint64_t disk_done = 0;    // their on-disk bytes (payload + CRC)
    uint64_t gw = 0;           // groups before gw are serialized
    uint32_t windows = 0;      // of the current output
    uint64_t chunks_compressed = 0;  // all outputs, for GPUC_TRACE
    double ms_compress = 0;
    // room for `chunks` slots; finished chunks are kept
    void reserve(uint32_t chunks, uint32_t stride, hipStream_t stream) {
        if (!res.p) res.alloc(sizeof(SizeCutResult));
        if (chunks <= cap_chunks) return;
        uint64_t want = (uint64_t)chunks + chunks / 4 + 1;
        if (want > 0xFFFFFFFFull) throw std::runtime_error("output too large for this chunk_length");
        DevBuf ns, nc, nr;
        ns.alloc(want * stride + 16);
        nc.alloc(want * 4 + 16);
        nr.alloc(want * 4 + 16);
        if (chunks_done) {
            HIP_CHECK(hipMemcpyAsync(ns.p, slots.p, (uint64_t)chunks_done * stride, hipMemcpyDeviceToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(nc.p, csize.p, (uint64_t)chunks_done * 4, hipMemcpyDeviceToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(nr.p, ccrc.p, (uint64_t)chunks_done * 4, hipMemcpyDeviceToDevice, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        std::swap(slots.p, ns.p); std::swap(slots.n, ns.n);
        std::swap(csize.p, nc.p); std::swap(csize.n, nc.n);
        std::swap(ccrc.p, nr.p); std::swap(ccrc.n, nr.n);
        disk.alloc((want + 1) * 8);
        cap_chunks = (uint32_t)want;
    }
};

// Where does the output that starts at group g0 end? P_h holds the n+1
// scanned offsets of the groups in the job's uncompressed stream (d_P is its
// device copy), d_keep their keep flags, d_data the device address of byte
// P_h[0]. `serialize(gb)` must issue on `stream` whatever makes the bytes of
// the groups [g0, gb) valid. Returns the output's last group. Groups after
// it may all be dropped ones (P_h[last + 1] == P_h[n]): then no partition is
// left to start another sstable, which the callers check. On return cp holds
// the output's complete chunks up to cp.chunks_done, compressed, and `stream`
// is idle.
static uint64_t plan_size_cut(CutPlan& cp, const std::vector<uint64_t>& P_h, const uint64_t* d_P,
                              const uint8_t* d_keep, uint64_t g0, const uint8_t* d_data,
                              double ratio, bool snappy, uint32_t L, uint64_t max_bytes,
                              const std::function<void(uint64_t)>& serialize,
                              hipStream_t stream) {
    const uint64_t n = P_h.size() - 1;
    const uint64_t B = P_h[g0], remaining = P_h[n] - B;
    const uint32_t stride = snappy ? snp_slot_stride(L) : lz4_slot_stride(L);
    const uint8_t* d_base = d_data + (B - P_h[0]);
    cp.chunks_done = 0;
    cp.disk_done = 0;
    cp.gw = g0;
    cp.windows = 0;
    if (!(ratio > 0.01)) ratio = 0.01;
    if (ratio > 1.5) ratio = 1.5;
    double want = (double)max_bytes / ratio * (1.0 + size_split_margin()) + 2.0 * L;
    Event eb, ee;
    for (;;) {
        const uint64_t U = want >= (double)remaining ? remaining : (uint64_t)want;
        // first group boundary at or past U bytes; P_h[n] - B >= U, so it exists
        uint64_t gb = (uint64_t)(std::lower_bound(P_h.begin() + cp.gw, P_h.end(), B + U) - P_h.begin());
        if (gb > n) gb = n;
        if (gb <= cp.gw) throw std::runtime_error("size split: window did not grow");
        serialize(gb);
        const uint64_t W = P_h[gb] - B;
        if (W / L > 0xFFFFFFFEull) throw std::runtime_error("output too large for this chunk_length");
        const uint32_t c1 = (uint32_t)(W / L);  // complete chunks of the window
        cp.reserve(c1 + 1, stride, stream);     // + the short last chunk of the finished output
        HIP_CHECK(hipEventRecord(eb, stream));
        if (c1 > cp.chunks_done) {
            const uint32_t c0 = cp.chunks_done;
            launch_chunk_compress(snappy, d_base + (uint64_t)c0 * L, W - (uint64_t)c0 * L,
                                  cp.slots.as<uint8_t>() + (uint64_t)c0 * stride,
                                  cp.csize.as<uint32_t>() + c0, cp.ccrc.as<uint32_t>() + c0,
                                  c1 - c0, L, stride, stream);
            cp.chunks_compressed += c1 - c0;
        }
        hipLaunchKernelGGL(k_size_cut, dim3(1), dim3(SIZE_CUT_BLOCK), 0, stream, d_P + 1, d_keep,
                           cp.gw, gb, B, cp.csize.as<uint32_t>(), cp.chunks_done, c1, cp.disk_done,
                           L, max_bytes, cp.disk.as<uint64_t>(), cp.res.as<SizeCutResult>());
        HIP_CHECK(hipEventRecord(ee, stream));
        SizeCutResult r;
        HIP_CHECK(hipMemcpyAsync(&r, cp.res.p, sizeof(r), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        float ms;
        HIP_CHECK(hipEventElapsedTime(&ms, eb, ee));
        cp.ms_compress += ms;
        cp.windows++;
        cp.chunks_done = c1;
        cp.disk_done = r.disk;
        cp.gw = gb;
        if (r.cut != SIZE_CUT_NONE) {
            if (r.cut < g0 || r.cut >= gb) throw std::runtime_error("size split: cut outside its window");
            return r.cut;
        }
        if (W == remaining) return gb - 1;  // no cut before the job's last byte
        want = std::max(want * 2.0, (double)W + 2.0 * L);
    }
}

// "<dir>/<version>-<generation>-<format>" with the generation advanced by i
static std::string output_base_plus(const std::string& ob, uint64_t i) {
    if (!i) return ob;
    size_t sl = ob.rfind('/');
    std::string dir = sl == std::string::npos ? std::string() : ob.substr(0, sl + 1);
    std::string name = sl == std::string::npos ? ob : ob.substr(sl + 1);
    size_t a = name.find('-'), b2 = a == std::string::npos ? a : name.find('-', a + 1);
    if (b2 == std::string::npos) throw unsupported_error("output_base has no generation to advance");
    uint64_t gen0 = std::stoull(name.substr(a + 1, b2 - a - 1));
    return dir + name.substr(0, a + 1) + std::to_string(gen0 + i) + name.substr(b2);
}

// The size-split writer: stage 1 (sizes) once for all groups, then per
// output a speculative window (serialize + compress + k_size_cut, extended
// until the cut is inside it), and the ordinary drain and tail over the
// output's own groups. `ratio` is the inputs' compressed/uncompressed ratio;
// `poll` is called between outputs (cancellation). opt.base names the first
// output, the following ones advance its generation.
static WriteDeviceOut write_sstables_size_split(const OutPartsBuf& opb, const UnfColsBuf& rows,
                                                uint64_t n_groups, SerParams2 sp, DevBuf& d_stats,
                                                DevBuf& d_tomb, uint32_t tomb_cap,
                                                const TableTypes& types, const OutputOptions& opt,
                                                uint64_t max_bytes, double ratio,
                                                const std::function<void()>& poll,
                                                hipStream_t stream) {
    if (!chunk_len_supported(opt.chunk_len))
        throw unsupported_error("unsupported output chunk_length " + std::to_string(opt.chunk_len) +
                                CHUNK_LEN_WHY);
    const uint32_t OCL = opt.chunk_len;
    const uint32_t SLOT_STRIDE = opt.snappy ? snp_slot_stride(OCL) : lz4_slot_stride(OCL);
    static const std::vector<int64_t> ps_off_h = est_hist_offsets(155);
    static const std::vector<int64_t> ch_off_h = est_hist_offsets(118);
    DevBuf d_ps_off, d_ch_off;
    d_ps_off.alloc(ps_off_h.size() * 8);
    d_ch_off.alloc(ch_off_h.size() * 8);
    HIP_CHECK(hipMemcpyAsync(d_ps_off.p, ps_off_h.data(), ps_off_h.size() * 8, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_ch_off.p, ch_off_h.data(), ch_off_h.size() * 8, hipMemcpyHostToDevice, stream));

    // ==== stage 1, once: partition sizes are position-independent ====
    DevBuf d_psize, d_poff, d_rel, d_isize, d_nblocks, d_infsz, d_cells;
    d_psize.alloc((n_groups + 1) * 8);
    d_poff.alloc((n_groups + 1) * 8);
    d_rel.alloc((n_groups + 1) * 8);  // offsets relative to the current output's first byte
    d_isize.alloc((n_groups + 1) * 8);
    d_nblocks.alloc(n_groups * 4);
    d_infsz.alloc(n_groups * 8);
    d_cells.alloc(n_groups * 8);
    uint64_t total_unc = 0;
    float ms_sizes = 0;
    if (n_groups) {
        Event es0, es1;
        HIP_CHECK(hipEventRecord(es0, stream));
        hipLaunchKernelGGL(k_sizes_rows, dim3((uint32_t)((n_groups + 255) / 256)), dim3(256), 0,
                           stream, opb.op, rows.uc, n_groups, sp, d_psize.as<uint64_t>(),
                           d_isize.as<uint64_t>(), d_nblocks.as<uint32_t>(),
                           d_infsz.as<uint64_t>(), (OutStats*)nullptr, d_ps_off.as<int64_t>(),
                           (int32_t)ps_off_h.size(), d_ch_off.as<int64_t>(),
                           (int32_t)ch_off_h.size(), d_cells.as<uint64_t>());
        HIP_CHECK(hipEventRecord(es1, stream));
        HIP_CHECK(hipMemsetAsync(d_psize.as<uint64_t>() + n_groups, 0, 8, stream));
        HIP_CHECK(hipMemcpyAsync(d_poff.p, d_psize.p, (n_groups + 1) * 8, hipMemcpyDeviceToDevice, stream));
        total_unc = exscan_u64(d_poff.as<uint64_t>(), n_groups + 1, stream);
        HIP_CHECK(hipEventElapsedTime(&ms_sizes, es0, es1));
    }
    // nothing kept: the one empty sstable the unsplit writer produces
    if (!total_unc)
        return write_sstable_device(opb, rows, n_groups, sp, d_stats, d_tomb, tomb_cap, types, opt,
                                    stream);
    std::vector<uint64_t> P_h(n_groups + 1);
    HIP_CHECK(hipMemcpy(P_h.data(), d_poff.p, (n_groups + 1) * 8, hipMemcpyDeviceToHost));

    WriteDeviceOut tot;
    tot.n_outputs = 0;
    tot.ms_sizes = ms_sizes;
    DevBuf d_out_data, d_out_index, d_bloom, d_stats_k;
    d_out_data.alloc(total_unc);
    d_stats_k.alloc(sizeof(OutStats));
    Stream cstream;
    Event ev2, ev4, evs0, evs1;
    CutPlan cp;
    uint64_t chunks_written = 0, windows_total = 0, unc_serialized = 0;
    const HBloomSpec bs = bloom_spec_001();
    for (uint64_t g0 = 0; g0 < n_groups && P_h[g0] < total_unc;) {
        poll();
        const uint64_t B = P_h[g0];
        uint64_t idx_n = 0;  // groups covered by the window's Index.db offsets
        bool timed = false;
        auto add_serialize_ms = [&]() {
            if (!timed) return;
            float ms;
            HIP_CHECK(hipEventElapsedTime(&ms, evs0, evs1));
            tot.ms_serialize += ms;
            timed = false;
        };
        // Index.db entry sizes depend on positions inside THIS output, so the
        // window's sizes, offsets and image are redone from g0 when it grows;
        // Data bytes come out the same and finished chunks are kept
        auto serialize = [&](uint64_t gb) {
            add_serialize_ms();  // an earlier window of this output; stream is idle
            const uint64_t ng = gb - g0;
            HIP_CHECK(hipEventRecord(evs0, stream));
            hipLaunchKernelGGL(k_index_sizes_rows, dim3((uint32_t)((ng + 255) / 256)), dim3(256), 0,
                               stream, opb.op, gb, sp, d_poff.as<uint64_t>(),
                               d_nblocks.as<uint32_t>(), d_infsz.as<uint64_t>(),
                               d_isize.as<uint64_t>(), g0, B, d_rel.as<uint64_t>());
            HIP_CHECK(hipMemsetAsync(d_isize.as<uint64_t>() + gb, 0, 8, stream));
            uint64_t idx_w = exscan_u64(d_isize.as<uint64_t>() + g0, ng + 1, stream);
            d_out_index.alloc(idx_w);
            const uint32_t waves_per_block = 4;
            hipLaunchKernelGGL(k_serialize_rows, dim3((uint32_t)((ng + waves_per_block - 1) / waves_per_block)),
                               dim3(WAVE * waves_per_block), 0, stream, opb.op, rows.uc, gb, sp,
                               d_rel.as<uint64_t>(), d_isize.as<uint64_t>(),
                               d_nblocks.as<uint32_t>(), d_infsz.as<uint64_t>(),
                               d_out_data.as<uint8_t>() + B, d_out_index.as<uint8_t>(),
                               (uint32_t*)nullptr, (uint64_t)0, 0, g0);
            HIP_CHECK(hipEventRecord(evs1, stream));
            timed = true;
            idx_n = ng;
            unc_serialized += P_h[gb] - B;
        };
        const uint64_t g_last = plan_size_cut(cp, P_h, d_poff.as<uint64_t>(), opb.op.keep, g0,
                                              d_out_data.as<uint8_t>(), ratio, opt.snappy, OCL,
                                              max_bytes, serialize, stream);
        add_serialize_ms();
        const uint64_t g1 = g_last + 1;
        if (g1 - g0 > idx_n) throw std::runtime_error("size split: cut past the serialized window");

        // ==== finish output over [g0, g1): chunks before the cut are final ====
        OutputImage im;
        im.g0 = g0;
        im.g1 = g1;
        im.total_unc = P_h[g1] - B;
        im.n_chunks = (uint32_t)((im.total_unc + OCL - 1) / OCL);
        const uint32_t full = (uint32_t)(im.total_unc / OCL);
        if (full > cp.chunks_done || im.n_chunks > cp.cap_chunks)
            throw std::runtime_error("size split: chunk bookkeeping");
        if (im.n_chunks > full) {
            // only the last, now shorter, chunk is compressed again
            launch_chunk_compress(opt.snappy, d_out_data.as<uint8_t>() + B + (uint64_t)full * OCL,
                                  im.total_unc - (uint64_t)full * OCL,
                                  cp.slots.as<uint8_t>() + (uint64_t)full * SLOT_STRIDE,
                                  cp.csize.as<uint32_t>() + full, cp.ccrc.as<uint32_t>() + full, 1,
                                  OCL, SLOT_STRIDE, stream);
            cp.chunks_compressed++;
        }
        const uint32_t SLAB = (512u << 20) / OCL;
        std::vector<Event> ev_c((im.n_chunks + SLAB - 1) / SLAB);
        for (auto& e : ev_c) HIP_CHECK(hipEventRecord(e, stream));
        HIP_CHECK(hipMemcpyAsync(&im.total_idx, d_isize.as<uint64_t>() + g1, 8, hipMemcpyDeviceToHost, stream));
        // stats, tombstone list and histograms of the output's own groups
        init_outstats(d_stats_k, stream);
        {
            const uint32_t blocks = (uint32_t)((g1 - g0 + 255) / 256);
            hipLaunchKernelGGL(k_collect_rows, dim3(blocks), dim3(256), 0, stream, opb.op, rows.uc,
                               g1, sp.sch.n_cols, sp.sch.n_cpx, d_stats_k.as<OutStats>(),
                               d_tomb.as<uint32_t>(), tomb_cap, g0);
            hipLaunchKernelGGL(k_part_hists, dim3(blocks), dim3(256), 0, stream,
                               d_psize.as<uint64_t>(), d_cells.as<uint64_t>(), g1,
                               d_stats_k.as<OutStats>(), d_ps_off.as<int64_t>(),
                               (int32_t)ps_off_h.size(), d_ch_off.as<int64_t>(),
                               (int32_t)ch_off_h.size(), g0);
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipMemcpy(&im.hst, d_stats_k.p, sizeof(OutStats), hipMemcpyDeviceToHost));
        const uint64_t num_bits = im.hst.partitions_out * (uint64_t)bs.buckets + 20;
        im.words = ((num_bits - 1) >> 6) + 1;
        im.bs = bs;
        d_bloom.alloc(im.words * 8);
        HIP_CHECK(hipMemsetAsync(d_bloom.p, 0, im.words * 8, stream));
        hipLaunchKernelGGL(k_bloom_rows, dim3((uint32_t)((g1 - g0 + 255) / 256)), dim3(256), 0,
                           stream, opb.op, g1, d_bloom.as<uint32_t>(), im.words * 64, bs.k, g0);
        HIP_CHECK(hipEventRecord(ev2, stream));
        im.slots = &cp.slots;
        im.csize = &cp.csize;
        im.ccrc = &cp.ccrc;
        im.out_index = &d_out_index;
        im.bloom = &d_bloom;
        im.h_index = (uint8_t*)g_pin_out[opt.wslot][1].get(im.total_idx ? im.total_idx : 1);
        if (!im.h_index) throw std::runtime_error("pinned out alloc failed");
        im.ev_c = &ev_c;
        im.index_late = true;
        OutputOptions opt_k = opt;
        opt_k.base = output_base_plus(opt.base, tot.n_outputs);
        WriteDeviceOut w;
        drain_and_finish(im, opb.op, sp, d_tomb, tomb_cap, types, opt_k, stream, cstream, ev2, ev4, w);
        if (g_trace)
            fprintf(stderr, "[split] output %u groups=[%llu,%llu) unc=%llu comp=%llu windows=%u\n",
                    tot.n_outputs, (unsigned long long)g0, (unsigned long long)g1,
                    (unsigned long long)im.total_unc, (unsigned long long)w.compressed_len,
                    cp.windows);
        tot.n_outputs++;
        tot.partitions += im.hst.partitions_out;
        tot.rows += im.hst.rows_out;
        tot.cells += im.hst.total_cells;
        tot.uncompressed_len += im.total_unc;
        tot.compressed_len += w.compressed_len;
        tot.ms_d2h += w.ms_d2h;
        tot.ms_io += w.ms_io;
        chunks_written += im.n_chunks;
        windows_total += cp.windows;
        g0 = g1;
    }
    tot.ms_compress = cp.ms_compress;
    if (g_trace)
        fprintf(stderr,
                "[split] outputs=%u windows=%llu chunks_compressed=%llu chunks_written=%llu "
                "bytes_serialized=%llu bytes_written=%llu margin=%.3f ratio=%.3f\n",
                tot.n_outputs, (unsigned long long)windows_total,
                (unsigned long long)cp.chunks_compressed, (unsigned long long)chunks_written,
                (unsigned long long)unc_serialized, (unsigned long long)total_unc,
                size_split_margin(), ratio);
    return tot;
}

}  // namespace gpuc

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace gpuc;

extern "C" const char* gpuc_version(void) { return "cassandra_gpucompact 0.1 (gfx950)"; }

extern "C" int gpuc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static void set_err(char* dst, size_t cap, const std::string& msg) {
    if (!dst || !cap) return;
    snprintf(dst, cap, "%s", msg.c_str());
}
// The exception-to-code ladder of the entry points that report through an
// error buffer. run_compaction (cancellation, timing), gpuc_verify and
// gpuc_compress_buffer map differently and spell their own.
template <class F> static int abi_guard(char* err, size_t cap, F&& body) {
    try {
        return body();
    } catch (const unsupported_error& e) {
        set_err(err, cap, e.what());
        return GPUC_ERR_UNSUPPORTED;
    } catch (const format_error& e) {
        set_err(err, cap, e.what());
        return GPUC_ERR_FORMAT;
    } catch (const std::exception& e) {
        set_err(err, cap, e.what());
        return GPUC_ERR_INTERNAL;
    }
}

struct CompactSetup {
    int k = 0;        // total ingested sstables (data + tombstone sources)
    int k_data = 0;   // first k_data are the compacted data inputs
    std::vector<std::string> in_bases;
    std::vector<bytes> index_data;
    std::vector<HCompressionInfo> cinfos;
    uint32_t out_chunk_len = CHUNK_LEN;  // resolved from the job / cinfos[0]
    std::vector<HStatistics> stats;
    std::vector<std::vector<uint64_t>> positions;   // n_parts+1 absolute offsets
    std::vector<std::vector<uint64_t>> entry_offs;  // Index.db entry byte offsets
    std::vector<std::vector<bti::bytes>> bti_prefixes;  // da: trie separator per partition
    std::vector<size_t> comp_file_sz;
    // one schema for the job: the union of the compacting inputs' headers
    // (the output header), and every source's own columns mapped into it
    JobSchema js;
    bool bti = false;                    // inputs are `da` (trie-indexed)
    // unsharded fast path: whole-file Data.db reads started during index
    // parse as ordered STRIPES per source (compact_one adopts them when its
    // window covers the full file and overlaps H2D with the remaining reads)
    struct StripeRead {
        mutable std::vector<std::future<void>> th;  // one per stripe, in file order
        std::vector<uint64_t> off, len;
    };
    mutable std::vector<StripeRead> full_stripes;
    // file-ordered reader pool: stripes are queued (file 0 first) so the
    // FIRST sstable's bytes land early and its H2D+decompress pipeline
    // starts ~1/k into the read instead of after all files finish together
    mutable std::vector<std::thread> read_pool;
    std::vector<uint8_t*> full_pin;
    ~CompactSetup() {
        for (auto& sr : full_stripes)
            for (auto& t : sr.th)
                if (t.valid()) t.wait();
        for (auto& t : read_pool)
            if (t.joinable()) t.join();
    }
};

struct cancelled_error : std::runtime_error {
    cancelled_error() : std::runtime_error("compaction cancelled (cancel_flag set)") {}
};
// cooperative cancellation poll (CompactionIterator.isStopRequested):
// called between pipeline phases of a task
static inline void check_cancel(const gpuc_job* job) {
    if (job->cancel_flag && *job->cancel_flag) throw cancelled_error();
}

// k_validate_digest's parameters: the output header's column names, packed
// regular then static, on the device. Holds the host staging of its async
// copies, so it lives until the stream is next synchronised.
struct ValidateNames {
    bytes names;
    std::vector<uint32_t> noff;
    DevBuf d_names, d_noff;
    ValidateParams upload(const TableTypes& header, const SchemaParams& sch, hipStream_t stream) {
        for (auto& [nm, t2] : header.regular_cols) {
            (void)t2;
            noff.push_back((uint32_t)names.size());
            names.insert(names.end(), nm.begin(), nm.end());
        }
        for (auto& [nm, t2] : header.static_cols) {
            (void)t2;
            noff.push_back((uint32_t)names.size());
            names.insert(names.end(), nm.begin(), nm.end());
        }
        noff.push_back((uint32_t)names.size());
        ValidateParams vpar{};
        vpar.names = gpuc::upload(d_names, names.data(), names.size(), stream, 8);
        vpar.name_off = gpuc::upload(d_noff, noff.data(), noff.size(), stream);
        vpar.n_reg = (uint32_t)header.regular_cols.size();
        vpar.n_static = (uint32_t)header.static_cols.size();
        vpar.counters = sch.counters;
        vpar.n_cpx = sch.n_cpx;
        vpar.n_ck = sch.n_ck;
        vpar.ck_w = sch.ck_w;
        return vpar;
    }
};

// k_validate_digest over the reconciled groups (Validator.rowHash): 32 bytes
// per group into d_hash. Both validation epilogues launch it here.
static void launch_validate_digest(const OutParts& op, const UnfColsBuf& rows, uint64_t n_groups,
                                   const ValidateParams& vpar, DevBuf& d_hash,
                                   hipStream_t stream) {
    d_hash.alloc(n_groups * 32 + 32);
    if (!n_groups) return;
    hipLaunchKernelGGL(k_validate_digest, dim3((uint32_t)((n_groups + 255) / 256)), dim3(256), 0,
                       stream, op, rows.uc, n_groups, vpar, d_hash.as<uint8_t>());
}

// ---------------------------------------------------------------------------
// The stages of compact_one. Each struct owns its device buffers AND the host
// staging that its async copies read. compact_one declares them in its own
// scope, after its Stream, so all of it outlives every synchronise of the run
// and is released before the stream is destroyed.
// ---------------------------------------------------------------------------

// What one compact_one call covers and where its output goes: the partition
// window pr[s] = [blo, bhi) per input (the full range in the unsharded case),
// the output base and the pinned-arena set. Shards run two at a time so
// front-phase kernels of one shard overlap the other shard's LDS-bound
// compress (they use disjoint CU resources).
struct ShardWindow {
    std::vector<std::pair<uint32_t, uint32_t>> pr;
    std::string out_base;
    int wslot = 0;
    // da internal shards: trie-separator windows are one partition wide of
    // exact; this token filter (on GPU-computed tokens) is the exact boundary
    bool exact = false;
    int64_t tok_lo = 0, tok_hi = 0;
};

// Window ingest: partition window -> chunk range -> compressed range per
// input, the Data.db bytes (own reader threads, or the stripes compact_setup
// pre-read), H2D on the copy stream and the per-source decompress on the main
// stream, which waits on ev_h2d[s] first. Synchronises nothing: the caller
// reads d_error next. The merge compares keys inside the decompressed bytes
// and the writer copies values out of them, so this lives for the whole run.
struct WindowIngest {
    std::vector<uint32_t> win_blo, win_n;
    std::vector<ChunkWindow> win;
    std::vector<uint64_t> win_comp_lo;
    std::vector<size_t> comp_sz;  // compressed bytes in window
    std::vector<uint8_t*> comp_pin;
    bool adopt = false;           // setup pre-read the whole files
    std::vector<std::thread> readers;
    std::optional<Stream> copy_stream;  // created by issue(); ahead of its buffers
    std::vector<DevBuf> d_comp, d_data, d_pos, d_chunks;
    std::vector<std::vector<ChunkDesc>> chunks;
    std::vector<Event> ev_h2d;          // one per input: its uploads are done
    std::vector<const uint8_t*> vbase;  // virtual decompressed origin
    ~WindowIngest() {
        // an error between resolve() and issue() must not leave a reader running
        for (auto& t : readers)
            if (t.joinable()) t.join();
    }
    // windows, pinned arenas, and the reads started
    void resolve(const CompactSetup& su, const ShardWindow& sw) {
        const int k = su.k;
        win_blo.resize(k);
        win_n.resize(k);
        win.resize(k);
        win_comp_lo.resize(k);
        comp_sz.assign(k, 0);
        comp_pin.assign(k, nullptr);
        for (int s = 0; s < k; s++) {
            win_blo[s] = sw.pr[s].first;
            win_n[s] = sw.pr[s].second - sw.pr[s].first;
            win[s] = chunk_window(su.cinfos[s], su.comp_file_sz[s], su.positions[s],
                                  sw.pr[s].first, sw.pr[s].second);
            win_comp_lo[s] = win[s].comp_lo;
            comp_sz[s] = win[s].comp_hi - win[s].comp_lo;
        }
        adopt = !su.full_pin.empty();
        readers.resize(adopt ? 0 : k);
        for (int s = 0; s < k; s++) {
            if (adopt) {
                // setup already reads the whole file into the slot-0 arenas
                comp_pin[s] = su.full_pin[s] + win_comp_lo[s];
            } else {
                comp_pin[s] = (uint8_t*)g_pin_in[sw.wslot][s].get(comp_sz[s] ? comp_sz[s] : 1);
                if (!comp_pin[s]) throw std::runtime_error("pinned alloc failed");
                readers[s] = std::thread([this, &su, s] {
                    if (comp_sz[s])
                        read_file_range(su.in_bases[s] + "-Data.db", comp_pin[s], win_comp_lo[s],
                                        comp_sz[s], 3);
                });
            }
        }
    }
    // H2D + decompress, pipelined per sstable. Returns the residual read wait
    // (ms) that the pipeline did not hide.
    double issue(const CompactSetup& su, const DevBuf& d_error, hipStream_t stream) {
        const int k = su.k;
        copy_stream.emplace();
        d_comp = std::vector<DevBuf>(k);
        d_data = std::vector<DevBuf>(k);
        d_pos = std::vector<DevBuf>(k);
        d_chunks = std::vector<DevBuf>(k);
        ev_h2d = std::vector<Event>(k);
        chunks.resize(k);
        vbase.assign(k, nullptr);
        double ms_read_data = 0;
        for (int s = 0; s < k; s++) {
            double tr = wall_ms();
            auto& ci = su.cinfos[s];
            const uint64_t icl = ci.chunk_len;  // inputs of one job may differ
            const uint64_t c_lo = win[s].c_lo, n_wchunks = win[s].c_hi - c_lo;
            d_comp[s].alloc(comp_sz[s] ? comp_sz[s] : 1);
            if (adopt && win_comp_lo[s] == 0 && comp_sz[s] == su.comp_file_sz[s]) {
                // stripe-progressive H2D: copy each stripe as its read lands
                // (whole-file window only; stripe offsets are file-absolute)
                auto& sr = su.full_stripes[s];
                for (size_t t = 0; t < sr.th.size(); t++) {
                    if (sr.th[t].valid()) sr.th[t].wait();
                    if (sr.len[t])
                        HIP_CHECK(hipMemcpyAsync(d_comp[s].as<uint8_t>() + sr.off[t],
                                                 comp_pin[s] + sr.off[t], sr.len[t],
                                                 hipMemcpyHostToDevice, *copy_stream));
                }
            } else if (adopt) {
                // token-restricted window over a preread file: wait for all
                // stripes, then one window-sized copy
                auto& sr = su.full_stripes[s];
                for (auto& t : sr.th)
                    if (t.valid()) t.wait();
                if (comp_sz[s])
                    HIP_CHECK(hipMemcpyAsync(d_comp[s].p, comp_pin[s], comp_sz[s],
                                             hipMemcpyHostToDevice, *copy_stream));
            } else {
                readers[s].join();  // in-order wait; all reads run concurrently
                if (comp_sz[s])
                    HIP_CHECK(hipMemcpyAsync(d_comp[s].p, comp_pin[s], comp_sz[s],
                                             hipMemcpyHostToDevice, *copy_stream));
            }
            ms_read_data = wall_ms() - tr + ms_read_data;
            d_data[s].alloc(n_wchunks * icl + 16);
            // positions stay ABSOLUTE: the decompressed window is addressed
            // through a virtual origin so partition offsets need no rewrite
            vbase[s] = d_data[s].as<uint8_t>() - c_lo * icl;
            upload(d_pos[s], su.positions[s].data() + win_blo[s], (size_t)win_n[s] + 1,
                   *copy_stream);
            chunks[s] = chunk_descs(chunk_frames(ci, su.comp_file_sz[s], c_lo, win[s].c_hi),
                                    d_comp[s].as<uint8_t>(), win_comp_lo[s],
                                    d_data[s].as<uint8_t>(), ci.chunk_len);
            upload(d_chunks[s], chunks[s].data(), chunks[s].size(), *copy_stream, 16);
            HIP_CHECK(hipEventRecord(ev_h2d[s], *copy_stream));
            HIP_CHECK(hipStreamWaitEvent(stream, ev_h2d[s], 0));
            launch_chunk_decompress(ci, d_chunks[s], chunks[s].size(), d_error, nullptr, stream);
        }
        return ms_read_data;
    }
    // the parse's source descriptors over the window; returns total partitions
    uint64_t source_descs(const CompactSetup& su, std::vector<SrcDesc2>& srcs) const {
        uint64_t total_parts = 0;
        srcs.resize(su.k);
        for (int s = 0; s < su.k; s++) {
            srcs[s].data = vbase[s];
            srcs[s].part_pos = d_pos[s].as<uint64_t>();
            srcs[s].n_parts = win_n[s];
            srcs[s].min_ts = su.stats[s].hdr_min_ts;
            srcs[s].min_ldt = su.stats[s].hdr_min_ldt;
            srcs[s].min_ttl = su.stats[s].hdr_min_ttl;
            srcs[s].rec_base = (uint32_t)total_parts;
            set_src_columns(srcs[s], su.js.src[s]);
            total_parts += srcs[s].n_parts;
        }
        if (total_parts > 0xFFFFFFFFull) throw std::runtime_error("too many partitions for one job");
        return total_parts;
    }
    // exact-key comparator fallback: point the merge kernels at the
    // decompressed inputs (keys > 8 bytes tie-break by byte walk)
    KeyLut key_lut() const {
        KeyLut lut{};
        for (size_t s = 0; s < vbase.size(); s++) {
            lut.base[s] = vbase[s];
            lut.pos[s] = d_pos[s].as<uint64_t>();
        }
        lut.enabled = 1;
        return lut;
    }
};

// the event pairs behind gpuc_result's phase times, all on the main stream
struct PhaseEvents {
    Event e0, e1, e2, e3, e4, er0, er1;
};

// Purge inputs: the job's purge options, keep ranges, overlaps (with their
// bloom bit arrays packed into one buffer) and the shard's exact token bounds
// as a PurgeParams2. The async copies read the host vectors here.
struct PurgeInputs {
    std::vector<int64_t> klo, khi, ov_lo, ov_hi, ov_ts;
    std::vector<uint32_t> ov_bw;
    std::vector<uint64_t> ov_boff, ov_bbits;
    std::vector<int32_t> ov_bk;
    DevBuf d_kr_lo, d_kr_hi, d_ov_lo, d_ov_hi, d_ov_ts, d_ov_bw, d_ov_boff, d_ov_bbits, d_ov_bk;
    PurgeParams2 build(const gpuc_job* job, const ShardWindow& sw, hipStream_t stream) {
        PurgeParams2 pp{};
        pp.now_sec = job->now_sec;
        pp.gc_before = job->gc_before;
        pp.never_purge = job->never_purge;
        pp.enforce_strict_liveness = job->enforce_strict_liveness;
        pp.n_overlaps = job->n_overlaps;
        pp.has_shard = job->has_token_range;
        pp.shard_lo = job->token_lo;
        pp.shard_hi = job->token_hi;
        if (sw.exact) {
            // intersected with any job-level range
            if (pp.has_shard) {
                pp.shard_lo = std::max(pp.shard_lo, sw.tok_lo);
                pp.shard_hi = std::min(pp.shard_hi, sw.tok_hi);
            } else {
                pp.has_shard = 1;
                pp.shard_lo = sw.tok_lo;
                pp.shard_hi = sw.tok_hi;
            }
        }
        if (job->n_keep_ranges > 0) {
            for (int i = 0; i < job->n_keep_ranges; i++) {
                klo.push_back(job->keep_ranges[i].token_lo);
                khi.push_back(job->keep_ranges[i].token_hi);
            }
            pp.kr_lo = upload(d_kr_lo, klo.data(), klo.size(), stream);
            pp.kr_hi = upload(d_kr_hi, khi.data(), khi.size(), stream);
            pp.n_keep_ranges = job->n_keep_ranges;
            pp.invert_ranges = job->invert_ranges;
        }
        if (job->n_overlaps > 0) {
            bool any_bloom = false;
            for (int i = 0; i < job->n_overlaps; i++) {
                ov_lo.push_back(job->overlaps[i].token_lo);
                ov_hi.push_back(job->overlaps[i].token_hi);
                ov_ts.push_back(job->overlaps[i].min_timestamp);
                any_bloom |= job->overlaps[i].bloom_bits != nullptr;
            }
            pp.ov_lo = upload(d_ov_lo, ov_lo.data(), ov_lo.size(), stream);
            pp.ov_hi = upload(d_ov_hi, ov_hi.data(), ov_hi.size(), stream);
            pp.ov_min_ts = upload(d_ov_ts, ov_ts.data(), ov_ts.size(), stream);
            if (any_bloom) {
                // word offsets per entry; bit_len 0 = no bloom
                for (int i = 0; i < job->n_overlaps; i++) {
                    const auto& ov = job->overlaps[i];
                    ov_boff.push_back(ov_bw.size());
                    if (ov.bloom_bits && ov.bloom_bit_len) {
                        uint64_t words32 = (ov.bloom_bit_len + 31) / 32;
                        ov_bw.insert(ov_bw.end(), ov.bloom_bits, ov.bloom_bits + words32);
                        ov_bbits.push_back(ov.bloom_bit_len);
                        ov_bk.push_back(ov.bloom_hash_count);
                    } else {
                        ov_bbits.push_back(0);
                        ov_bk.push_back(0);
                    }
                }
                pp.ov_bloom_words = upload(d_ov_bw, ov_bw.data(), ov_bw.size(), stream, 8);
                pp.ov_bloom_off = upload(d_ov_boff, ov_boff.data(), ov_boff.size(), stream);
                pp.ov_bloom_bits = upload(d_ov_bbits, ov_bbits.data(), ov_bbits.size(), stream);
                pp.ov_bloom_k = upload(d_ov_bk, ov_bk.data(), ov_bk.size(), stream);
                pp.ov_has_bloom = 1;
            }
        }
        return pp;
    }
};

// Merkle device side. assign() gives every group its leaf BEFORE reconcile,
// which then drops the partitions of no tree instead of merging them;
// reduce() XORs the digests into their leaves after it, so that only the
// leaves travel to the host. The spec's arrays are the caller's.
struct MerkleLeaves {
    DevBuf d_left, d_begin, d_right, d_group_leaf;
    uint32_t n_leaves = 0;
    const int32_t* assign(const gpuc_merkle_spec& ms, const Groups& groups, hipStream_t stream) {
        n_leaves = ms.leaf_begin[ms.n_trees];
        MerkleParams mp{upload(d_left, ms.tree_left, (size_t)ms.n_trees, stream),
                        upload(d_begin, ms.leaf_begin, (size_t)ms.n_trees + 1, stream),
                        upload(d_right, ms.leaf_right, (size_t)n_leaves, stream), ms.n_trees};
        d_group_leaf.alloc(groups.n * 4 + 4);
        if (groups.n)
            hipLaunchKernelGGL(k_merkle_assign, dim3((uint32_t)((groups.n + 255) / 256)),
                               dim3(256), 0, stream, groups.sorted,
                               groups.start.as<uint64_t>(), groups.n, mp,
                               d_group_leaf.as<int32_t>());
        return d_group_leaf.as<int32_t>();
    }
    // the MERKLE epilogue; synchronises. Returns the partitions digested.
    uint64_t reduce(MerkleRun& run, const TableTypes& header, const SchemaParams& sch,
                    const OutParts& op, const UnfColsBuf& rows, uint64_t n_groups,
                    hipStream_t stream) {
        ValidateNames vnames;
        ValidateParams vpar = vnames.upload(header, sch, stream);
        DevBuf d_hash, d_leaves;
        // n_leaves x 4 hash words, then n_leaves counts
        d_leaves.alloc((uint64_t)n_leaves * 40);
        HIP_CHECK(hipMemsetAsync(d_leaves.p, 0, (uint64_t)n_leaves * 40, stream));
        unsigned long long* d_lh = d_leaves.as<unsigned long long>();
        unsigned long long* d_lc = d_lh + (uint64_t)n_leaves * 4;
        launch_validate_digest(op, rows, n_groups, vpar, d_hash, stream);
        if (n_groups)
            hipLaunchKernelGGL(k_merkle_leaf_xor, dim3((uint32_t)((n_groups + 255) / 256)),
                               dim3(256), 0, stream, op.keep, d_group_leaf.as<int32_t>(),
                               d_hash.as<uint64_t>(), n_groups, d_lh, d_lc);
        std::vector<uint64_t> h_cnt(n_leaves);
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipMemcpy(run.leaf_hash, d_lh, (uint64_t)n_leaves * 32, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(h_cnt.data(), d_lc, (uint64_t)n_leaves * 8, hipMemcpyDeviceToHost));
        uint64_t cnt = 0;
        for (uint32_t i = 0; i < n_leaves; i++) cnt += h_cnt[i];
        if (run.leaf_partitions) memcpy(run.leaf_partitions, h_cnt.data(), (uint64_t)n_leaves * 8);
        run.n_partitions = cnt;
        return cnt;
    }
};

// The VALIDATION epilogue: per-partition repair digests of the kept groups
// (8-byte BE token + 32-byte hash each) written to `path` instead of an
// sstable. Synchronises. Returns the partitions digested.
static uint64_t write_digest_file(const char* path, const TableTypes& header,
                                  const SchemaParams& sch, const OutParts& op,
                                  const UnfColsBuf& rows, uint64_t n_groups, hipStream_t stream) {
    ValidateNames vnames;
    ValidateParams vpar = vnames.upload(header, sch, stream);
    DevBuf d_hash;
    launch_validate_digest(op, rows, n_groups, vpar, d_hash, stream);
    std::vector<uint8_t> h_hash(n_groups * 32);
    std::vector<int64_t> h_tok(n_groups);
    std::vector<uint8_t> h_keep(n_groups);
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipMemcpy(h_hash.data(), d_hash.p, n_groups * 32, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h_tok.data(), op.token, n_groups * 8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h_keep.data(), op.keep, n_groups, hipMemcpyDeviceToHost));
    bytes outb;
    uint64_t cnt = 0;
    for (uint64_t g2 = 0; g2 < n_groups; g2++) {
        if (!h_keep[g2]) continue;
        for (int b2 = 7; b2 >= 0; b2--) outb.push_back((uint8_t)((uint64_t)h_tok[g2] >> (8 * b2)));
        outb.insert(outb.end(), h_hash.begin() + g2 * 32, h_hash.begin() + g2 * 32 + 32);
        cnt++;
    }
    write_file(path, outb.data(), outb.size());
    return cnt;
}

// Garbage-collect pass (kd < k): the tombstone sources are merged and
// reconciled among themselves, matched against the data groups, the shadowed
// data is filtered out into `rows`, and the purge that the data pass deferred
// runs last (GarbageSkipper runs before the Purger in CompactionIterator).
// Synchronises to read d_error. `rows` replaces the data pass's rows for the
// writer and shares their complex-cell arena.
struct GarbageCollect {
    UnfColsBuf rows;
    Groups groups_t;  // tombstone sources, reconciled among themselves
    Reconciled rec_t;
    DevBuf d_ctr_arena_t;
    void run(const gpuc_job* job, const std::vector<uint64_t>& runs_t, MRec* d_recs_a,
             MRec* d_recs_b, const KeyLut& lut, const DevBuf& d_srcbases,
             const ParsedInput& parsed, const SchemaParams& sch, uint64_t ctr_arena_cap,
             const PurgeParams2& pp, const PurgeParams2& pp_data, Reconciled& rec,
             uint64_t n_groups, const DevBuf& d_error, hipStream_t stream) {
        const OutParts& op = rec.parts.op;
        const uint64_t src_parts = runs_t.back();
        if (src_parts > 0) {
            MRec* d_sorted_t = merge_sorted_runs(d_recs_a, d_recs_b, runs_t, stream, lut);
            find_groups(groups_t, d_sorted_t, src_parts, lut, stream);
            scan_group_rows(groups_t, d_srcbases, parsed.pc, stream);
            rec_t.alloc(groups_t, sch, parsed.total_cpx, stream);
            // the source pass bump-allocates merged counter contexts from
            // its own arena (the main pass's bump counter lives in the
            // OTHER OutStats, so sharing one arena would overlap)
            SchemaParams sch_t = sch;
            if (sch.counters) {
                d_ctr_arena_t.alloc(ctr_arena_cap);
                sch_t.ctr_arena = d_ctr_arena_t.as<uint8_t>();
            }
            PurgeParams2 pp_src = pp_data;
            pp_src.has_shard = 0;  // sources shadow regardless of the shard
            pp_src.group_leaf = nullptr;  // indexed by the data groups, not these
            launch_reconcile(groups_t, (int)runs_t.size() - 1, d_srcbases, parsed, rec_t, sch_t,
                             pp_src, d_error, stream);
        }
        // match + capacity scan + filter
        const dim3 grid((uint32_t)((n_groups + 255) / 256)), block(256);
        DevBuf d_tidx, d_cap;
        d_tidx.alloc(n_groups * 8);
        d_cap.alloc(n_groups * 8);
        hipLaunchKernelGGL(k_gc_match, grid, block, 0, stream, op, n_groups, rec_t.parts.op,
                           groups_t.n, d_tidx.as<int64_t>(), d_cap.as<uint64_t>());
        uint64_t gc_total = exscan_u64(d_cap.as<uint64_t>(), n_groups, stream);
        rows.alloc(gc_total, sch.n_cols, sch.n_ck, sch.n_cpx);
        // the cpx CELL arena is shared: the filter compacts each row's
        // own [start,count) segment of the data rows' arena in place
        if (sch.n_cpx) rows.uc.cpx = rec.rows.uc.cpx;
        hipLaunchKernelGGL(k_garbage_filter, grid, block, 0, stream, op, n_groups, rec_t.parts.op,
                           rec.rows.uc, rec_t.rows.uc, rows.uc, d_tidx.as<int64_t>(),
                           d_cap.as<uint64_t>(), sch, parsed.cx, job->cell_level_gc ? 1 : 0);
        // reset first/last group, then the deferred purge pass
        HIP_CHECK(hipMemsetAsync((uint8_t*)rec.stats.p + offsetof(OutStats, first_group), 0xFF, 8, stream));
        HIP_CHECK(hipMemsetAsync((uint8_t*)rec.stats.p + offsetof(OutStats, last_group), 0x00, 8, stream));
        hipLaunchKernelGGL(k_purge_parts, grid, block, 0, stream, op, rows.uc, n_groups, sch, pp,
                           rec.stats.as<OutStats>());
        if (unsigned long long err = read_dev_error(d_error, stream))
            throw std::runtime_error("GPU gc filter error code " + std::to_string(err));
    }
};

// the output header's minima (SerializationHeader.make merges the compacted
// inputs' EncodingStats; a minimum does not depend on their order)
static HeaderStats merged_header_stats(const std::vector<HStatistics>& stats, int kd) {
    int64_t min_ts = INT64_MAX, min_ldt = INT64_MAX;
    int32_t min_ttl = INT32_MAX;
    for (int s = 0; s < kd; s++) {
        min_ts = std::min(min_ts, stats[s].min_timestamp);
        min_ldt = std::min(min_ldt, stats[s].min_ldt);
        min_ttl = std::min(min_ttl, stats[s].min_ttl);
    }
    HeaderStats hs;
    hs.min_ts = min_ts == NO_TIMESTAMP ? TIMESTAMP_EPOCH : min_ts;
    hs.min_ldt = min_ldt == NO_DELETION_TIME ? DELETION_TIME_EPOCH : min_ldt;
    hs.min_ttl = min_ttl == INT32_MAX ? 0 : min_ttl;
    return hs;
}

// What the writing epilogues consume: the reconciled partitions, the rows
// that survived (the garbage-collect pass's, when it ran), the header, and
// the stats and tombstone list that reconcile filled.
struct MergedOutput {
    const OutPartsBuf& parts;
    const UnfColsBuf& rows;
    uint64_t n_groups;
    SerParams2 sp;
    DevBuf& stats;
    DevBuf& tomb;
    uint32_t tomb_cap;
};

// ROUTED outputs: classify the kept partitions by token once, then run the
// writer once per output under that output's keep mask. Synchronises to read
// the per-output counts; polls for cancellation between outputs.
static WriteDeviceOut write_routed_outputs(const gpuc_job* job, RouteRun& run,
                                           const MergedOutput& m, const TableTypes& header,
                                           const OutputOptions& oopt, hipStream_t stream) {
    const gpuc_route_spec& rs = *run.spec;
    const uint32_t n_out = rs.n_outputs;
    const uint64_t n_groups = m.n_groups;
    DevBuf d_rlo, d_rhi, d_rout, d_cls, d_mask, d_cnt, d_stats_o;
    RouteParams rp{upload(d_rlo, rs.range_lo, (size_t)rs.n_ranges, stream, 8),
                   upload(d_rhi, rs.range_hi, (size_t)rs.n_ranges, stream, 8),
                   upload(d_rout, rs.range_output, (size_t)rs.n_ranges, stream, 4),
                   rs.n_ranges, rs.default_output, n_out};
    d_cls.alloc(n_groups + 1);
    d_mask.alloc(n_groups + 1);
    d_cnt.alloc((uint64_t)n_out * 8);
    d_stats_o.alloc(sizeof(OutStats));
    HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, (uint64_t)n_out * 8, stream));
    const dim3 grid((uint32_t)((n_groups + 255) / 256)), block(256);
    if (n_groups)
        hipLaunchKernelGGL(k_route_parts, grid, block, 0, stream, m.parts.op.token,
                           m.parts.op.keep, n_groups, rp, d_cls.as<uint8_t>(),
                           d_cnt.as<unsigned long long>());
    std::vector<uint64_t> h_cnt(n_out);
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipMemcpy(h_cnt.data(), d_cnt.p, (uint64_t)n_out * 8, hipMemcpyDeviceToHost));
    WriteDeviceOut w;
    w.n_outputs = 0;
    OutParts view = m.parts.op;
    view.keep = d_mask.as<uint8_t>();
    for (uint32_t o = 0; o < n_out; o++) {
        gpuc_route_output ro{};
        if (h_cnt[o]) {
            check_cancel(job);
            hipLaunchKernelGGL(k_route_mask, grid, block, 0, stream, d_cls.as<uint8_t>(), n_groups,
                               (uint8_t)o, d_mask.as<uint8_t>());
            init_outstats(d_stats_o, stream);
            OutputOptions oopt_o = oopt;
            oopt_o.base = rs.output_bases[o];
            WriteDeviceOut wo = write_sstable_device(view, m.rows, n_groups, m.sp, d_stats_o,
                                                     m.tomb, m.tomb_cap, header, oopt_o, stream);
            if (wo.partitions != h_cnt[o])
                throw std::runtime_error("routed output " + std::to_string(o) +
                                         ": writer and router disagree on partitions");
            ro.written = 1;
            ro.partitions = wo.partitions;
            ro.rows = wo.rows;
            ro.uncompressed_bytes = wo.uncompressed_len;
            ro.compressed_bytes = wo.compressed_len;
            w.add(wo);
        }
        if (run.outputs) run.outputs[o] = ro;
    }
    return w;
}

// one sstable, or several cut at job->max_output_bytes
static WriteDeviceOut write_plain_or_split(const gpuc_job* job, const CompactSetup& su, int kd,
                                           const MergedOutput& m, const OutputOptions& oopt,
                                           hipStream_t stream) {
    if (!job->max_output_bytes)
        return write_sstable_device(m.parts, m.rows, m.n_groups, m.sp, m.stats, m.tomb,
                                    m.tomb_cap, su.js.header, oopt, stream);
    // r of the speculative window: the inputs' own compressed/uncompressed ratio
    uint64_t in_comp = 0, in_unc = 0;
    for (int s = 0; s < kd; s++) {
        in_comp += su.comp_file_sz[s];
        in_unc += su.cinfos[s].data_len;
    }
    return write_sstables_size_split(m.parts, m.rows, m.n_groups, m.sp, m.stats, m.tomb,
                                     m.tomb_cap, su.js.header, oopt, job->max_output_bytes,
                                     in_unc ? (double)in_comp / (double)in_unc : 1.0,
                                     [&]() { check_cancel(job); }, stream);
}

// Result accounting of a writing run: phase times from the events (all long
// complete: the writer has drained), the writer's totals, and merged_counts
// from RECONCILE's stats (a routed run's per-output stats never hold them).
static void account_result(gpuc_result* res, std::mutex& res_mu, const PhaseEvents& ev,
                           const WriteDeviceOut& w, const DevBuf& d_stats) {
    OutStats hst;
    HIP_CHECK(hipMemcpy(&hst, d_stats.p, sizeof(OutStats), hipMemcpyDeviceToHost));
    float th2d, tdec, tparse, tmerge, trec;
    HIP_CHECK(hipEventElapsedTime(&th2d, ev.e0, ev.e1));
    HIP_CHECK(hipEventElapsedTime(&tdec, ev.e1, ev.e2));
    HIP_CHECK(hipEventElapsedTime(&tparse, ev.e2, ev.e3));
    HIP_CHECK(hipEventElapsedTime(&tmerge, ev.e3, ev.e4));
    HIP_CHECK(hipEventElapsedTime(&trec, ev.er0, ev.er1));
    std::lock_guard<std::mutex> g(res_mu);
    res->n_outputs += w.n_outputs;
    res->partitions_out += w.partitions;
    res->rows_out += w.rows;
    res->output_uncompressed_bytes += w.uncompressed_len;
    res->output_compressed_bytes += w.compressed_len;
    for (int i = 0; i < 64; i++) res->merged_counts[i] += hst.merged_counts[i];
    res->ms_h2d = 0;         // overlapped into the ingest pipeline (e0..e1)
    res->ms_decompress += th2d + tdec;  // read/H2D/decompress pipeline, GPU side
    res->ms_parse += tparse;
    res->ms_reconcile += trec;
    res->ms_merge += tmerge - trec;  // merge rounds + grouping
    res->ms_serialize += w.ms_sizes + w.ms_serialize;
    res->ms_compress += w.ms_compress;
    res->ms_d2h += w.ms_d2h;
    res->ms_write_io += w.ms_io;
    // dominant kernel estimate
    struct { const char* n; double ms; } ks[] = {
        {"k_lz4_decompress", (double)th2d + tdec}, {"k_parse", (double)tparse},
        {"merge+reconcile", (double)tmerge},
        {"k_serialize", w.ms_serialize}, {"k_lz4_compress", w.ms_compress}};
    for (auto& kk : ks)
        if (kk.ms > res->dominant_kernel_ms) {
            res->dominant_kernel_ms = kk.ms;
            snprintf(res->dominant_kernel, sizeof(res->dominant_kernel), "%s", kk.n);
        }
    res->dominant_kernel_launches = 1;
}

// Everything from data read through component write for ONE shard window:
// the pipeline, top to bottom. `mode` says what comes out at the end.
static void compact_one(const gpuc_job* job, const CompactSetup& su, const ShardWindow& sw,
                        const CompactMode& mode, gpuc_result* res, std::mutex& res_mu) {
    HIP_CHECK(hipSetDevice(job->device));
    Stream stream;  // ahead of every buffer used on it
    const int k = su.k;

    // ---- window ingest: read, H2D + decompress (pipelined per sstable) ----
    double t0 = wall_ms();
    WindowIngest ingest;
    ingest.resolve(su, sw);
    {
        std::lock_guard<std::mutex> g(res_mu);
        res->ms_read_io += wall_ms() - t0;
    }
    TR("window resolved");
    check_cancel(job);
    PhaseEvents ev;
    HIP_CHECK(hipEventRecord(ev.e0, stream));
    DevBuf d_error;
    d_error.alloc(8);
    HIP_CHECK(hipMemsetAsync(d_error.p, 0, 8, stream));
    {
        double ms_read_data = ingest.issue(su, d_error, stream);
        std::lock_guard<std::mutex> g(res_mu);
        res->ms_read_io += ms_read_data;  // residual read wait not hidden by the pipeline
    }
    TR("ingest issued");
    HIP_CHECK(hipEventRecord(ev.e1, stream));  // e0..e1: H2D+decompress pipeline (overlapped)
    HIP_CHECK(hipEventRecord(ev.e2, stream));
    // corrupt inputs must fail cleanly, not fault the GPU: the parse
    // walk trusts decompressed bytes, so the chunk-CRC verdict is checked
    // BEFORE any parse kernel touches them
    if (unsigned long long err = read_dev_error(d_error, stream))
        throw std::runtime_error("input chunk decompress/CRC failed, code " + std::to_string(err));

    // ---- parse (pass A: count + partition meta; pass B: row decode) ----
    std::vector<SrcDesc2> srcs;  // read by an async copy: lives past the parse sync
    const uint64_t total_parts = ingest.source_descs(su, srcs);
    DevSchema dsch;
    SchemaParams sch = dsch.upload(su.js.schema, stream);
    DevBuf d_srcs, d_recs_a, d_recs_b, d_rows_in;
    upload(d_srcs, srcs.data(), srcs.size(), stream);
    d_recs_a.alloc(total_parts * sizeof(MRec));
    d_recs_b.alloc(total_parts * sizeof(MRec));
    d_rows_in.alloc(8);
    HIP_CHECK(hipMemsetAsync(d_rows_in.p, 0, 8, stream));
    ParsedInput parsed;
    parsed.cx = cpx_types(su.js.schema);
    parse_input(parsed, d_srcs, (uint32_t)k, total_parts, d_recs_a, sch, d_error, d_rows_in, false,
                stream);
    HIP_CHECK(hipEventRecord(ev.e3, stream));
    {
        unsigned long long err = read_dev_error(d_error, stream);
        TR("parse synced");
        check_cancel(job);  // a set cancel flag takes precedence over a parse error
        throw_if_collection_parse_error(err);
        if (err) throw std::runtime_error("GPU decode/parse error code " + std::to_string(err));
        uint64_t rows_in_local = 0;
        HIP_CHECK(hipMemcpy(&rows_in_local, d_rows_in.p, 8, hipMemcpyDeviceToHost));
        std::lock_guard<std::mutex> g(res_mu);
        res->rows_in += rows_in_local;
    }

    // ---- merge (pairwise rounds over pre-sorted source runs) ----
    // In garbage-collect mode the first k_data inputs are the compacted
    // data; the rest are tombstone sources merged in a second pass.
    const KeyLut lut = ingest.key_lut();
    const int kd = su.k_data > 0 ? su.k_data : k;
    const bool gc_mode = kd < k;
    std::vector<uint64_t> runs{0}, runs_t{0};
    for (int s = 0; s < kd; s++) runs.push_back(runs.back() + srcs[s].n_parts);
    for (int s = kd; s < k; s++) runs_t.push_back(runs_t.back() + srcs[s].n_parts);
    const uint64_t data_parts = runs.back();
    MRec* d_sorted = merge_sorted_runs(d_recs_a.as<MRec>(), d_recs_b.as<MRec>(), runs, stream, lut);
    TR("merge issued");

    // ---- group heads + starts ----
    Groups groups;
    find_groups(groups, d_sorted, data_parts, lut, stream);
    const uint64_t n_groups = groups.n;
    TR("groups known");
    check_cancel(job);

    // ---- reconcile + purge ----
    std::vector<uint32_t> bases(k);  // read by an async copy: lives past the next sync
    for (int s = 0; s < k; s++) bases[s] = srcs[s].rec_base;
    DevBuf d_srcbases;
    upload(d_srcbases, bases.data(), bases.size(), stream);
    scan_group_rows(groups, d_srcbases, parsed.pc, stream);
    TR("out rows scanned");
    Reconciled rec;
    rec.alloc(groups, sch, parsed.total_cpx, stream);
    DevBuf d_tomb, d_ctr_arena;
    uint64_t ctr_arena_cap = 0;
    if (sch.counters) {
        ctr_arena_cap = counter_arena_cap(parsed, sch.n_cols, stream);
        d_ctr_arena.alloc(ctr_arena_cap);
        sch.ctr_arena = d_ctr_arena.as<uint8_t>();
    }
    const uint32_t tomb_cap = tomb_list_cap(groups.total_rows, parsed.total_cpx, n_groups, sch);
    d_tomb.alloc((uint64_t)tomb_cap * 4);
    MerkleLeaves merkle;
    PurgeInputs purge;
    const int32_t* group_leaf =
        mode.merkle ? merkle.assign(*mode.merkle->spec, groups, stream) : nullptr;
    PurgeParams2 pp = purge.build(job, sw, stream);
    pp.group_leaf = group_leaf;
    HIP_CHECK(hipEventRecord(ev.er0, stream));
    // GC mode: purge is DEFERRED until after the garbage filter
    PurgeParams2 pp_data = pp;
    if (gc_mode) {
        pp_data.gc_before = INT64_MIN;
        pp_data.never_purge = 1;
        pp_data.enforce_strict_liveness = 0;
    }
    launch_reconcile(groups, kd, d_srcbases, parsed, rec, sch, pp_data, d_error, stream);
    HIP_CHECK(hipEventRecord(ev.er1, stream));
    HIP_CHECK(hipEventRecord(ev.e4, stream));
    TR("reconcile issued");
    if (unsigned long long err = read_dev_error(d_error, stream))
        throw std::runtime_error("GPU reconcile error code " + std::to_string(err));

    // ---- garbage collect: merge the tombstone sources, filter, purge ----
    GarbageCollect gc;
    const bool gc_ran = gc_mode && n_groups > 0;
    if (gc_ran) {
        gc.run(job, runs_t, d_recs_a.as<MRec>() + data_parts, d_recs_b.as<MRec>() + data_parts, lut,
               d_srcbases, parsed, sch, ctr_arena_cap, pp, pp_data, rec, n_groups, d_error, stream);
        TR("garbage filtered");
    }

    // ---- output header, then the mode's epilogue ----
    const MergedOutput out{rec.parts, gc_ran ? gc.rows : rec.rows, n_groups,
                           SerParams2{merged_header_stats(su.stats, kd), sch},
                           rec.stats, d_tomb, tomb_cap};
    restore_ck_ascending(out.parts.op, out.rows, n_groups, sch, stream);
    if (mode.digest_path || mode.merkle) {
        // digests instead of a written sstable: no writer, so no phase times
        // and no merged_counts either
        uint64_t cnt;
        if (mode.merkle) {
            cnt = merkle.reduce(*mode.merkle, su.js.header, sch, out.parts.op, out.rows, n_groups,
                                stream);
        } else {
            cnt = write_digest_file(mode.digest_path, su.js.header, sch, out.parts.op, out.rows,
                                    n_groups, stream);
            if (mode.digest_count) *mode.digest_count = cnt;
        }
        std::lock_guard<std::mutex> gl(res_mu);
        res->partitions_out += cnt;
        return;
    }
    const OutputOptions oopt{sw.out_base, su.cinfos[0].snappy, su.bti, su.out_chunk_len, sw.wslot};
    const WriteDeviceOut w = mode.route
        ? write_routed_outputs(job, *mode.route, out, su.js.header, oopt, stream)
        : write_plain_or_split(job, su, kd, out, oopt, stream);
    TR("writer done");
    account_result(res, res_mu, ev, w, rec.stats);
}


// ---------------------------------------------------------------------------
// compaction setup (host metadata shared by all shards) + sharded driver
// ---------------------------------------------------------------------------

static void compact_setup(const gpuc_job* job, CompactSetup& su, bool preread_full) {
    int k = job->n_inputs + (job->n_tomb_sources > 0 ? job->n_tomb_sources : 0);
    su.k = k;
    {
        std::string b0 = job->input_bases[0];
        su.bti = file_exists(b0 + "-Partitions.db") && !file_exists(b0 + "-Index.db");
    }
    su.k_data = job->n_inputs;
    su.in_bases.resize(k);
    su.index_data.resize(k);
    su.cinfos.resize(k);
    su.stats.resize(k);
    su.positions.resize(k);
    su.entry_offs.resize(k);
    su.bti_prefixes.resize(k);
    su.comp_file_sz.resize(k);
    // Data.db reads start FIRST (they are the long pole); metadata parse and
    // index decode run while they stream into the pinned arenas
    if (preread_full) {
        su.full_pin.resize(k, nullptr);
        su.full_stripes.resize(k);
        struct RTask { int s; uint64_t off, len; std::promise<void> done; };
        auto tasks = std::make_shared<std::vector<RTask>>();
        for (int s = 0; s < k; s++) {
            su.in_bases[s] = s < su.k_data ? job->input_bases[s]
                                           : job->tombstone_source_bases[s - su.k_data];
            su.comp_file_sz[s] = file_size_of(su.in_bases[s] + "-Data.db");
            su.full_pin[s] = (uint8_t*)g_pin_in[0][s].get(su.comp_file_sz[s] ? su.comp_file_sz[s] : 1);
            if (!su.full_pin[s]) throw std::runtime_error("pinned alloc failed");
            auto& sr = su.full_stripes[s];
            const int NS_STRIPE = 6;
            uint64_t per = (su.comp_file_sz[s] + NS_STRIPE - 1) / NS_STRIPE;
            for (int t = 0; t < NS_STRIPE; t++) {
                uint64_t o = (uint64_t)t * per;
                if (o >= su.comp_file_sz[s]) break;
                uint64_t len = std::min<uint64_t>(per, su.comp_file_sz[s] - o);
                sr.off.push_back(o);
                sr.len.push_back(len);
                tasks->push_back(RTask{s, o, len, std::promise<void>()});
                sr.th.push_back(tasks->back().done.get_future());
            }
        }
        // pool drains tasks in queue order (file-major): early files complete
        // first and the consumer's per-stripe waits overlap the later reads
        auto next = std::make_shared<std::atomic<size_t>>(0);
        int nworkers = (int)std::min<size_t>(12, tasks->size());
        for (int wkr = 0; wkr < nworkers; wkr++) {
            su.read_pool.emplace_back([&su, tasks, next] {
                for (;;) {
                    size_t i = next->fetch_add(1);
                    if (i >= tasks->size()) return;
                    RTask& rt = (*tasks)[i];
                    read_file_range(su.in_bases[rt.s] + "-Data.db", su.full_pin[rt.s] + rt.off,
                                    rt.off, rt.len, 1);
                    rt.done.set_value();
                }
            });
        }
    }
    {
        std::vector<std::thread> mth;
        std::vector<std::exception_ptr> merr(k);  // rethrown as thrown: keeps the ABI code
        for (int s = 0; s < k; s++) {
            su.in_bases[s] = s < su.k_data ? job->input_bases[s]
                                           : job->tombstone_source_bases[s - su.k_data];
            mth.emplace_back([&, s, preread_full]() {
                try {
                    const std::string& base = su.in_bases[s];
                    if (su.bti) {
                        // `da` inputs: partition positions come from the
                        // Partitions.db trie (payload < 0 == ~data_pos;
                        // >= 0 == Rows.db TrieIndexEntry footer, whose
                        // dataStartPosition leads). DFS order == key order
                        // == data order.
                        bytes pf = read_file(base + "-Partitions.db");
                        bytes rf = read_file(base + "-Rows.db");
                        bti::bytes pfb(pf.begin(), pf.end());
                        bti::bytes rfb(rf.begin(), rf.end());
                        auto bp = bti::read_bti_partitions(pfb);
                        auto& pos = su.positions[s];
                        pos.reserve(bp.entries.size() + 1);
                        auto& pfx = su.bti_prefixes[s];
                        pfx.reserve(bp.entries.size());
                        for (auto& e : bp.entries) {
                            pos.push_back(e.idxpos < 0 ? (uint64_t)~e.idxpos
                                                       : bti::row_index_data_pos(rfb, (uint64_t)e.idxpos));
                            pfx.push_back(std::move(e.prefix));
                        }
                    } else {
                        su.index_data[s] = read_file(base + "-Index.db");
                    }
                    su.cinfos[s] = parse_compression_info(read_file(base + "-CompressionInfo.db"));
                    su.stats[s] = parse_statistics(read_file(base + "-Statistics.db"));
                    if (!preread_full) su.comp_file_sz[s] = file_size_of(base + "-Data.db");
                } catch (const std::exception&) { merr[s] = std::current_exception(); }
            });
        }
        for (auto& t : mth) t.join();
        for (int s = 0; s < k; s++)
            if (merr[s]) std::rethrow_exception(merr[s]);
    }
    for (int s = 0; s < k; s++) {
        auto& st = su.stats[s];
        if (!st.partitioner.empty() && st.partitioner.find("Murmur3") == std::string::npos)
            throw std::runtime_error("Murmur3Partitioner required");
    }
    su.js = resolve_job_schema(su.stats, su.k_data);
    if (su.bti) refuse_bti_desc(su.js.header.clustering_types, "a `da` (BTI) input");
    if (su.bti) {
        // positions collected from the tries above; append the end sentinel
        for (int s = 0; s < k; s++) su.positions[s].push_back(su.cinfos[s].data_len);
    } else {
        std::vector<std::thread> th;
        std::vector<std::string> perr(k);
        for (int s = 0; s < k; s++)
            th.emplace_back(parse_index_positions, std::cref(su.index_data[s]),
                            su.cinfos[s].data_len, std::ref(su.positions[s]),
                            preread_full ? nullptr : &su.entry_offs[s], std::ref(perr[s]));
        for (auto& t : th) t.join();
        for (int s = 0; s < k; s++)
            if (!perr[s].empty()) throw std::runtime_error("Index.db parse: " + perr[s]);
    }
    for (int s = 1; s < k; s++)
        if (su.cinfos[s].snappy != su.cinfos[0].snappy)
            throw std::runtime_error("mixed compressors across inputs unsupported");
}

// Murmur3 token of the key in Index.db entry at byte offset `off`
static int64_t index_entry_token(const bytes& ib, uint64_t off) {
    uint32_t klen = ((uint32_t)ib[off] << 8) | ib[off + 1];
    return murmur3_token(ib.data() + off + 2, klen);
}

// The run behind gpuc_compact, gpuc_validate, gpuc_validate_merkle and
// gpuc_compact_routed: `mode` says what it produces. The mode entry points
// reject the job options they cannot be combined with before calling this.
static int run_compaction(const gpuc_job* job, gpuc_result* res, const CompactMode& mode) {
    memset(res, 0, sizeof(*res));
    const double t_start_all = wall_ms();
    if (g_trace) g_trace_t0 = wall_ms();
    auto failed = [&](int code, const std::exception& e) {
        set_err(res->error, sizeof(res->error), e.what());
        res->ms_total = wall_ms() - t_start_all;
        return code;
    };
    try {
        int ndev = gpuc_device_count();
        if (ndev <= 0) { set_err(res->error, sizeof(res->error), "no HIP device (no CPU fallback)"); return GPUC_ERR_NO_GPU; }
        HIP_CHECK(hipSetDevice(job->device));
        {
            Stream s0;
            ensure_crc_tables(s0);
        }
        if (job->n_inputs < 1 || job->n_inputs + (job->n_tomb_sources > 0 ? job->n_tomb_sources : 0) > 64) {
            set_err(res->error, sizeof(res->error), "n_inputs (+ tombstone sources) must be 1..64");
            return GPUC_ERR_UNSUPPORTED;
        }
        // argument checks first: a bad output length or mode never reads a byte
        (void)checked_chunk_len_arg(job->output_chunk_length, CHUNK_LEN);
        if (job->max_output_bytes && job->n_output_shards > 1)
            throw unsupported_error("max_output_bytes + n_output_shards unsupported");
        double t0 = wall_ms();
        int S_pre = job->n_output_shards > 1 ? job->n_output_shards : 1;
        CompactSetup su;
        compact_setup(job, su, S_pre == 1);
        // 0 == the chunk length of input_bases[0] (what the reference
        // compactor does when the table params are unchanged)
        su.out_chunk_len = checked_chunk_len_arg(job->output_chunk_length, su.cinfos[0].chunk_len);
        res->ms_read_io = wall_ms() - t0;
        TR("meta+index parsed");
        for (int s = 0; s < su.k_data; s++)
            res->input_uncompressed_bytes += su.cinfos[s].data_len;
        for (int s = 0; s < su.k_data; s++)
            res->partitions_in += su.positions[s].size() - 1;

        int S = S_pre;
        if (S > 1024) throw std::runtime_error("n_output_shards must be <= 1024");
        std::mutex res_mu;
        if (S == 1) {
            ShardWindow sw;
            for (int s = 0; s < su.k; s++)
                sw.pr.push_back({0u, (uint32_t)(su.positions[s].size() - 1)});
            sw.out_base = job->output_base;
            compact_one(job, su, sw, mode, res, res_mu);
        } else {
            if (job->has_token_range)
                throw std::runtime_error("token_range + n_output_shards unsupported");
            // output bases: generation g, g+1, ... (a compaction may emit
            // several sstables — UCS shard model / SplittingCompactionWriter)
            std::string ob = job->output_base;
            size_t sl = ob.rfind('/');
            std::string dir = sl == std::string::npos ? std::string(".") : ob.substr(0, sl);
            std::string name = sl == std::string::npos ? ob : ob.substr(sl + 1);
            size_t a = name.find('-'), b2 = name.find('-', a + 1);
            uint64_t gen0 = std::stoull(name.substr(a + 1, b2 - a - 1));
            std::string pre = name.substr(0, a + 1), post = name.substr(b2);
            // equal token-range split (cassandra_amd/sharding.py contract)
            std::vector<int64_t> lo_tok(S + 1);
            for (int i = 0; i < S; i++) {
                uint64_t lo_u = (uint64_t)(((unsigned __int128)i << 64) / (unsigned)S);
                lo_tok[i] = (int64_t)(lo_u + 0x8000000000000000ULL);
            }
            // per input: shard boundary partition = first with token >= lo_tok[i]
            std::vector<std::vector<uint32_t>> bounds(su.k, std::vector<uint32_t>(S + 1));
            std::vector<std::vector<uint32_t>> boundsR(su.k, std::vector<uint32_t>(S + 1));
            for (int s = 0; s < su.k; s++) {
                uint32_t n = (uint32_t)(su.positions[s].size() - 1);
                bounds[s][0] = boundsR[s][0] = 0;
                bounds[s][S] = boundsR[s][S] = n;
                for (int i = 1; i < S; i++) {
                    if (!su.bti) {
                        uint32_t lo = 0, hi = n;  // lower_bound(token >= lo_tok[i])
                        while (lo < hi) {
                            uint32_t mid = (lo + hi) >> 1;
                            if (index_entry_token(su.index_data[s], su.entry_offs[s][mid]) < lo_tok[i])
                                lo = mid + 1;
                            else hi = mid;
                        }
                        bounds[s][i] = lo;
                    } else {
                        // da inputs: Partitions.db stores CUT byte-comparable
                        // separators S_j with key_{j-1} < S_j <= key_j, whose
                        // leading bytes are the sign-flipped BE token
                        // (bti_byte_comparable_m3). A cut separator can be a
                        // strict PREFIX of the boundary string B, which makes
                        // its side ambiguous — so each boundary gets a
                        // left-biased lower bound (prefix-of-B counts as > B;
                        // first hit is provably <= j0+1, where j0 = first
                        // partition with token >= the boundary, because
                        // S_{j0+1} > key_{j0} >= B is never a prefix of B)
                        // and a right-biased upper bound (prefix counts as
                        // <= B; every separator before j0 is < B, so the
                        // first hit is >= j0 and <= j0+1). Window i =
                        // [L[i]-1, R[i+1]) then OVERLAPS its neighbours by at
                        // most two partitions; compact_one's per-shard token
                        // filter (exact, on GPU-computed tokens) assigns each
                        // partition to exactly one shard.
                        // boundary string: NEXT_COMPONENT then the
                        // sign-flipped BE token (bti_byte_comparable_m3)
                        uint8_t B[9];
                        B[0] = 0x40;
                        uint64_t tb = (uint64_t)lo_tok[i] ^ (1ull << 63);
                        for (int b3 = 0; b3 < 8; b3++) B[1 + b3] = (uint8_t)(tb >> (8 * (7 - b3)));
                        auto search = [&](bool prefix_is_gt) {
                            uint32_t lo = 0, hi = n;
                            while (lo < hi) {
                                uint32_t mid = (lo + hi) >> 1;
                                const bti::bytes& p2 = su.bti_prefixes[s][mid];
                                size_t m2 = p2.size() < 9 ? p2.size() : 9;
                                int c2 = m2 ? memcmp(p2.data(), B, m2) : 0;
                                bool gt = c2 ? c2 > 0 : (p2.size() >= 9 ? false : prefix_is_gt);
                                if (gt) hi = mid;
                                else lo = mid + 1;
                            }
                            return lo;
                        };
                        uint32_t L = search(true);
                        boundsR[s][i] = search(false);
                        bounds[s][i] = L > 0 ? L - 1 : 0;
                    }
                }
            }
            // two workers: front-phase kernels of one shard overlap the
            // other shard's compress
            std::atomic<int> next{0};
            // a worker's failure: a cancellation keeps its type; any other
            // error is rethrown by message as a plain runtime error
            std::vector<std::string> werr(2);
            bool wcancelled[2] = {false, false};
            auto workfn = [&](int w) {
                for (;;) {
                    int i = next.fetch_add(1);
                    if (i >= S) break;
                    ShardWindow sw;
                    for (int s = 0; s < su.k; s++) {
                        // bti: window = [left-biased start, right-biased end)
                        uint32_t e2 = su.bti ? boundsR[s][i + 1] : bounds[s][i + 1];
                        sw.pr.push_back({std::min(bounds[s][i], e2), e2});
                    }
                    sw.out_base = dir + "/" + pre + std::to_string(gen0 + i) + post;
                    sw.wslot = w;
                    sw.exact = su.bti;
                    sw.tok_lo = lo_tok[i];
                    sw.tok_hi = i + 1 < S ? lo_tok[i + 1] - 1 : INT64_MAX;
                    try {
                        compact_one(job, su, sw, mode, res, res_mu);
                    } catch (const cancelled_error&) {
                        wcancelled[w] = true;
                        break;
                    } catch (const std::exception& e) {
                        werr[w] = e.what();
                        break;
                    }
                }
            };
            std::thread w0(workfn, 0), w1(workfn, 1);
            w0.join();
            w1.join();
            for (int w = 0; w < 2; w++) {
                if (wcancelled[w]) throw cancelled_error();
                if (!werr[w].empty()) throw std::runtime_error(werr[w]);
            }
        }
        res->ms_total = wall_ms() - t_start_all;
        return GPUC_OK;
    } catch (const cancelled_error& e) { return failed(GPUC_ERR_CANCELLED, e);
    } catch (const unsupported_error& e) { return failed(GPUC_ERR_UNSUPPORTED, e);
    } catch (const format_error& e) { return failed(GPUC_ERR_FORMAT, e);
    } catch (const std::exception& e) { return failed(GPUC_ERR_INTERNAL, e);
    }
}

extern "C" int gpuc_compact(const gpuc_job* job, gpuc_result* res) {
    return run_compaction(job, res, CompactMode{});
}

// One-sstable verification (Verifier.java / `nodetool verify --extended`
// semantics): CompressionInfo + per-chunk CRC32 (verified inside the
// decompress kernel), full row-format walk (parse pass A validates structure
// and sizes), strict DecoratedKey order, Digest.crc32 recomputed from the
// chunk frames, and the bloom filter rebuilt from the keys and compared with
// Filter.db. Runs the same GPU ingest path as compaction.
extern "C" int gpuc_verify(const char* input_base, int32_t device, char* error,
                           size_t error_len) {
    try {
        if (gpuc_device_count() <= 0) { set_err(error, error_len, "no HIP device"); return GPUC_ERR_NO_GPU; }
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        ensure_crc_tables(stream);
        std::string base = input_base;
        const bool da = file_exists(base + "-Partitions.db") && !file_exists(base + "-Index.db");
        HCompressionInfo ci = parse_compression_info(read_file(base + "-CompressionInfo.db"));
        HStatistics st = parse_statistics(read_file(base + "-Statistics.db"));
        if (da) refuse_bti_desc(st.clustering_types, "a `da` (BTI) input");
        bytes comp = read_file(base + "-Data.db");
        std::vector<uint64_t> positions;
        if (da) {
            // `da` sstables: positions from the Partitions.db trie, as the
            // compaction front end reads them (DFS order == data order),
            // held to the same bounds parse_index_positions enforces
            bytes pf = read_file(base + "-Partitions.db");
            bytes rf = read_file(base + "-Rows.db");
            bti::bytes pfb(pf.begin(), pf.end());
            bti::bytes rfb(rf.begin(), rf.end());
            auto bp = bti::read_bti_partitions(pfb);
            for (auto& e : bp.entries) {
                uint64_t pos = e.idxpos < 0 ? (uint64_t)~e.idxpos
                                            : bti::row_index_data_pos(rfb, (uint64_t)e.idxpos);
                if (pos >= ci.data_len || (!positions.empty() && pos <= positions.back()))
                    throw std::runtime_error("Partitions.db positions not increasing/in range");
                positions.push_back(pos);
            }
            positions.push_back(ci.data_len);
        } else {
            bytes index_data = read_file(base + "-Index.db");
            std::string perr;
            parse_index_positions(index_data, ci.data_len, positions, nullptr, perr);
            if (!perr.empty()) throw std::runtime_error("Index.db: " + perr);
        }
        uint64_t n_parts = positions.size() - 1;
        const std::vector<ChunkFrame> frames = chunk_frames(ci, comp.size(), 0, ci.offsets.size());

        // digest from the chunk frames (CRC fields validated against bytes below)
        {
            std::vector<uint32_t> crcs, sizes;
            for (const ChunkFrame& fr : frames) {
                const uint8_t* p = comp.data() + fr.off + fr.comp_len;
                crcs.push_back(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
                               ((uint32_t)p[2] << 8) | p[3]);
                sizes.push_back(fr.comp_len);
            }
            bytes dg = read_file(base + "-Digest.crc32");
            std::string want(dg.begin(), dg.end());
            if (want != digest_text(fold_digest(crcs, sizes)))
                throw std::runtime_error("Digest.crc32 mismatch");
        }

        // GPU: decompress (chunk CRC verify) + structural walk + order + bloom
        DevBuf d_pos, d_error, d_recs;
        upload(d_pos, positions.data(), positions.size(), stream);
        d_error.alloc(8);
        HIP_CHECK(hipMemsetAsync(d_error.p, 0, 8, stream));
        DecodedFile dec;
        dec.issue(ci, frames, comp, d_error, nullptr, stream);
        const DevBuf& d_data = dec.data;
        {
            unsigned long long e = read_dev_error(d_error, stream);
            if (e == 1) throw std::runtime_error("chunk CRC mismatch");
            if (e) throw std::runtime_error("chunk decompress failed, code " + std::to_string(e));
        }
        HostSchema hsch = resolve_schema(st);
        if (hsch.col_fixed.empty() && !hsch.n_cpx) hsch.col_fixed.push_back(-1);
        DevSchema dsch;
        SchemaParams sch = dsch.upload(hsch, stream);
        if (!sch.n_cols && !sch.n_cpx) sch.n_cols = 1;
        SrcDesc2 src{};
        src.data = d_data.as<uint8_t>();
        src.part_pos = d_pos.as<uint64_t>();
        src.n_parts = (uint32_t)n_parts;
        src.min_ts = st.hdr_min_ts;
        src.min_ldt = st.hdr_min_ldt;
        src.min_ttl = st.hdr_min_ttl;
        src.rec_base = 0;
        set_src_identity(src, sch);
        DevBuf d_src;
        d_src.alloc(sizeof(src));
        HIP_CHECK(hipMemcpyAsync(d_src.p, &src, sizeof(src), hipMemcpyHostToDevice, stream));
        d_recs.alloc((n_parts + 1) * sizeof(MRec));
        // pass A only: it walks every row's structure; nothing here needs the
        // rows. A set column or a collection with int, bigint or timestamp
        // keys adds checks that only the cell walk of pass B makes (path
        // widths, no value in a set cell): such a table gets the full parse.
        const CpxTypes cx = cpx_types(hsch);
        const bool cell_checks = cx.key_signed || cx.is_set;
        DevBuf d_rows_in;
        if (cell_checks) {
            d_rows_in.alloc(8);
            HIP_CHECK(hipMemsetAsync(d_rows_in.p, 0, 8, stream));
        }
        ParsedInput parsed;
        parsed.cx = cx;
        parse_input(parsed, d_src, 1u, n_parts, d_recs, sch, d_error, d_rows_in, !cell_checks,
                    stream);
        if (cell_checks) throw_if_collection_parse_error(read_dev_error(d_error, stream));
        const ParsedCols& pc = parsed.pc;
        uint32_t blocks = (uint32_t)((n_parts + 255) / 256);
        if (n_parts) {
            KeyLut lut{};
            lut.base[0] = d_data.as<uint8_t>();
            lut.pos[0] = d_pos.as<uint64_t>();
            lut.enabled = 1;
            hipLaunchKernelGGL(k_verify_order, dim3(blocks), dim3(256), 0, stream,
                               d_recs.as<MRec>(), n_parts, lut, d_error.as<unsigned long long>());
        }
        // bloom recheck
        {
            bytes f = read_file(base + "-Filter.db");
            HReader r(f);
            uint32_t bk = r.be32();
            uint32_t words = r.be32();
            DevBuf d_bloom;
            d_bloom.alloc((uint64_t)words * 8 + 8);
            HIP_CHECK(hipMemsetAsync(d_bloom.p, 0, (uint64_t)words * 8, stream));
            if (n_parts)
                hipLaunchKernelGGL(k_verify_bloom, dim3(blocks), dim3(256), 0, stream, pc,
                                   d_recs.as<MRec>(), n_parts, d_bloom.as<uint32_t>(),
                                   (uint64_t)words * 64, (int32_t)bk);
            std::vector<uint8_t> got(words * 8);
            HIP_CHECK(hipStreamSynchronize(stream));
            HIP_CHECK(hipMemcpy(got.data(), d_bloom.p, words * 8, hipMemcpyDeviceToHost));
            unsigned long long gerr = 0;
            HIP_CHECK(hipMemcpy(&gerr, d_error.p, 8, hipMemcpyDeviceToHost));
            if (gerr == 1) throw std::runtime_error("chunk CRC mismatch");
            if (gerr == 30) throw std::runtime_error("partitions out of order");
            if (gerr) throw std::runtime_error("row format walk failed, code " + std::to_string(gerr));
            if (memcmp(got.data(), f.data() + 8, std::min<size_t>(got.size(), f.size() - 8)) != 0)
                throw std::runtime_error("Filter.db does not match keys");
        }
        return GPUC_OK;
    } catch (const unsupported_error& e) {
        set_err(error, error_len, e.what());
        return GPUC_ERR_UNSUPPORTED;
    } catch (const std::exception& e) {
        set_err(error, error_len, e.what());
        return GPUC_ERR_FORMAT;
    }
}

// Scrub (SortedTableScrubber semantics, this implementation's recovery
// granularity — mirrored by oracle::scrub_sstable): salvage partitions whose
// byte range touches only CRC/decode-clean chunks, rewrite them through the
// standard writer; report kept/dropped counts.
extern "C" int gpuc_scrub(const char* input_base, const char* output_base, int32_t device,
                          uint64_t* kept, uint64_t* dropped, char* error, size_t error_len) {
    return abi_guard(error, error_len, [&]() -> int {
        if (gpuc_device_count() <= 0) { set_err(error, error_len, "no HIP device"); return GPUC_ERR_NO_GPU; }
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        ensure_crc_tables(stream);
        std::string base = input_base;
        bytes index_data = read_file(base + "-Index.db");
        HCompressionInfo ci = parse_compression_info(read_file(base + "-CompressionInfo.db"));
        HStatistics st = parse_statistics(read_file(base + "-Statistics.db"));
        bytes comp = read_file(base + "-Data.db");
        std::vector<uint64_t> positions;
        std::string perr;
        parse_index_positions(index_data, ci.data_len, positions, nullptr, perr);
        if (!perr.empty()) throw std::runtime_error("Index.db: " + perr);
        uint64_t n_parts = positions.size() - 1;
        size_t n_chunks = ci.offsets.size();
        const std::vector<ChunkFrame> frames = chunk_frames(ci, comp.size(), 0, n_chunks);

        // decompress with per-chunk bad flags
        DevBuf d_error, d_bad;
        d_bad.alloc(n_chunks + 8);
        HIP_CHECK(hipMemsetAsync(d_bad.p, 0, n_chunks + 8, stream));
        d_error.alloc(8);
        HIP_CHECK(hipMemsetAsync(d_error.p, 0, 8, stream));
        DecodedFile dec;
        dec.issue(ci, frames, comp, d_error, d_bad.as<uint8_t>(), stream);
        const DevBuf& d_data = dec.data;
        std::vector<uint8_t> bad(n_chunks);
        HIP_CHECK(hipStreamSynchronize(stream));
        if (n_chunks)
            HIP_CHECK(hipMemcpy(bad.data(), d_bad.p, n_chunks, hipMemcpyDeviceToHost));

        // kept partitions: all overlapped chunks clean
        std::vector<uint64_t> kpos, kend;
        for (uint64_t i = 0; i < n_parts; i++) {
            uint64_t c0 = positions[i] / ci.chunk_len;
            uint64_t c1 = (positions[i + 1] + ci.chunk_len - 1) / ci.chunk_len;
            bool ok = true;
            for (uint64_t c = c0; c < c1 && c < n_chunks; c++)
                if (bad[c]) ok = false;
            if (ok) {
                kpos.push_back(positions[i]);
                kend.push_back(positions[i + 1]);
            }
        }
        uint64_t n_kept = kpos.size();
        if (kept) *kept = n_kept;
        if (dropped) *dropped = n_parts - n_kept;

        const HostSchema hsch = resolve_schema(st);
        DevSchema dsch;
        SchemaParams sch = dsch.upload(hsch, stream);

        // parse kept partitions (explicit ends: gaps where partitions dropped)
        DevBuf d_kpos, d_kend, d_recs, d_rows_in;
        d_kpos.alloc(n_kept * 8 + 8);
        d_kend.alloc(n_kept * 8 + 8);
        if (n_kept) {
            HIP_CHECK(hipMemcpyAsync(d_kpos.p, kpos.data(), n_kept * 8, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(d_kend.p, kend.data(), n_kept * 8, hipMemcpyHostToDevice, stream));
        }
        SrcDesc2 src{};
        src.data = d_data.as<uint8_t>();
        src.part_pos = d_kpos.as<uint64_t>();
        src.part_end = d_kend.as<uint64_t>();
        src.n_parts = (uint32_t)n_kept;
        src.min_ts = st.hdr_min_ts;
        src.min_ldt = st.hdr_min_ldt;
        src.min_ttl = st.hdr_min_ttl;
        src.rec_base = 0;
        set_src_identity(src, sch);
        DevBuf d_src;
        d_src.alloc(sizeof(src));
        HIP_CHECK(hipMemcpyAsync(d_src.p, &src, sizeof(src), hipMemcpyHostToDevice, stream));
        d_recs.alloc(n_kept * sizeof(MRec) + 32);
        d_rows_in.alloc(8);
        HIP_CHECK(hipMemsetAsync(d_rows_in.p, 0, 8, stream));
        ParsedInput parsed;
        parsed.cx = cpx_types(hsch);
        parse_input(parsed, d_src, 1u, n_kept, d_recs, sch, d_error, d_rows_in, false, stream);
        if (unsigned long long e = read_dev_error(d_error, stream)) {
            throw_if_collection_parse_error(e);
            throw std::runtime_error("scrub parse failed, code " + std::to_string(e));
        }
        // single source: records are already in DecoratedKey order
        KeyLut lut{};
        lut.base[0] = d_data.as<uint8_t>();
        lut.pos[0] = d_kpos.as<uint64_t>();
        lut.enabled = 1;
        Groups groups;
        find_groups(groups, d_recs.as<MRec>(), n_kept, lut, stream);
        DevBuf d_srcbases, d_tomb;
        uint32_t zero = 0;
        d_srcbases.alloc(8);
        HIP_CHECK(hipMemcpyAsync(d_srcbases.p, &zero, 4, hipMemcpyHostToDevice, stream));
        scan_group_rows(groups, d_srcbases, parsed.pc, stream);
        Reconciled rec;
        rec.alloc(groups, sch, parsed.total_cpx, stream);
        DevBuf d_ctr_arena;
        if (sch.counters) {
            // arity-1 reconcile still routes counter cells through the context branch
            d_ctr_arena.alloc(counter_arena_cap(parsed, sch.n_cols, stream));
            sch.ctr_arena = d_ctr_arena.as<uint8_t>();
        }
        uint32_t tomb_cap = tomb_list_cap(groups.total_rows, parsed.total_cpx, groups.n, sch);
        d_tomb.alloc((uint64_t)tomb_cap * 4);
        PurgeParams2 pp{};
        pp.gc_before = INT64_MIN;
        pp.never_purge = 1;
        launch_reconcile(groups, 1, d_srcbases, parsed, rec, sch, pp, d_error, stream);
        if (unsigned long long e = read_dev_error(d_error, stream))
            throw std::runtime_error("scrub reconcile failed, code " + std::to_string(e));
        SerParams2 sp2{};
        sp2.sch = sch;
        sp2.hs.min_ts = st.min_timestamp == NO_TIMESTAMP ? TIMESTAMP_EPOCH : st.min_timestamp;
        sp2.hs.min_ldt = st.min_ldt == NO_DELETION_TIME ? DELETION_TIME_EPOCH : st.min_ldt;
        sp2.hs.min_ttl = st.min_ttl == INT32_MAX ? 0 : st.min_ttl;
        restore_ck_ascending(rec.parts.op, rec.rows, groups.n, sch, stream);
        write_sstable_device(rec.parts, rec.rows, groups.n, sp2, rec.stats, d_tomb, tomb_cap, st,
                             OutputOptions{output_base, ci.snappy, false, ci.chunk_len, 0}, stream);
        return GPUC_OK;
    });
}

// Memtable flush: unsorted unique-key rows from the host ->
// token sort on device -> the shared serialize/compress/index/bloom kernels
// -> one complete `oa` sstable. Schema: `pk blob PRIMARY KEY, val blob`
// (one regular column; row tombstones via del_ldt != UINT32_MAX).
extern "C" int gpuc_flush(const gpuc_flush_rows* rows, const char* output_base,
                          int32_t device, char* error, size_t error_len) {
    return abi_guard(error, error_len, [&]() -> int {
        if (gpuc_device_count() <= 0) { set_err(error, error_len, "no HIP device"); return GPUC_ERR_NO_GPU; }
        if (!rows || rows->n_rows == 0) { set_err(error, error_len, "no rows"); return GPUC_ERR_UNSUPPORTED; }
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        ensure_crc_tables(stream);
        uint64_t n = rows->n_rows;
        // flatten to arenas
        std::vector<uint64_t> koff(n + 1, 0), voff(n + 1, 0);
        for (uint64_t i = 0; i < n; i++) {
            if (rows->key_lens[i] == 0) throw std::runtime_error("empty key");
            koff[i + 1] = koff[i] + rows->key_lens[i];
            voff[i + 1] = voff[i] + (rows->values[i] ? rows->value_lens[i] : 0);
        }
        std::vector<uint8_t> kbuf(koff[n]), vbuf(voff[n] ? voff[n] : 1);
        std::vector<uint32_t> dldt(n);
        for (uint64_t i = 0; i < n; i++) {
            memcpy(kbuf.data() + koff[i], rows->keys[i], rows->key_lens[i]);
            if (rows->values[i]) {
                memcpy(vbuf.data() + voff[i], rows->values[i], rows->value_lens[i]);
                dldt[i] = LDT_NONE_U32;
            } else {
                dldt[i] = rows->del_ldts[i];
                if (dldt[i] == LDT_NONE_U32)
                    throw std::runtime_error("row without value needs del_ldt");
            }
        }
        DevBuf d_k, d_koff, d_v, d_voff, d_ts, d_dldt, d_a, d_b, d_err;
        d_k.alloc(kbuf.size()); d_koff.alloc((n + 1) * 8);
        d_v.alloc(vbuf.size()); d_voff.alloc((n + 1) * 8);
        d_ts.alloc(n * 8); d_dldt.alloc(n * 4);
        HIP_CHECK(hipMemcpyAsync(d_k.p, kbuf.data(), kbuf.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_koff.p, koff.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_v.p, vbuf.data(), vbuf.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_voff.p, voff.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_ts.p, rows->timestamps, n * 8, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_dldt.p, dldt.data(), n * 4, hipMemcpyHostToDevice, stream));
        FlushParams fp{};
        fp.keys = d_k.as<uint8_t>();
        fp.key_off = d_koff.as<uint64_t>();
        fp.ts = d_ts.as<int64_t>();
        fp.vals = d_v.as<uint8_t>();
        fp.val_off = d_voff.as<uint64_t>();
        fp.del_ldt = d_dldt.as<uint32_t>();
        fp.n = n;
        d_a.alloc(n * sizeof(MRec));
        d_b.alloc(n * sizeof(MRec));
        uint32_t blocks = (uint32_t)((n + 255) / 256);
        hipLaunchKernelGGL(k_flush_recs, dim3(blocks), dim3(256), 0, stream, fp, d_a.as<MRec>());
        // exact-key comparator over the key arena (offsets pre-shifted by -2
        // to cancel the short-length skip in mrec_key_bytes)
        std::vector<uint64_t> koff_adj(n);
        for (uint64_t i = 0; i < n; i++) koff_adj[i] = koff[i] - 2;
        DevBuf d_koff_adj;
        d_koff_adj.alloc(n * 8);
        HIP_CHECK(hipMemcpyAsync(d_koff_adj.p, koff_adj.data(), n * 8, hipMemcpyHostToDevice, stream));
        KeyLut lut{};
        lut.base[0] = d_k.as<uint8_t>();
        lut.pos[0] = d_koff_adj.as<uint64_t>();
        lut.enabled = 1;
        MRec* d_sorted = merge_sort_recs(d_a.as<MRec>(), d_b.as<MRec>(), n, stream, lut);
        d_err.alloc(8);
        HIP_CHECK(hipMemsetAsync(d_err.p, 0, 8, stream));
        hipLaunchKernelGGL(k_flush_dupcheck, dim3(blocks), dim3(256), 0, stream, fp, d_sorted,
                           d_err.as<unsigned long long>());
        OutPartsBuf opb;
        opb.alloc(n);
        UnfColsBuf urows;
        urows.alloc(n, 1, 0);
        hipLaunchKernelGGL(k_flush_fill, dim3(blocks), dim3(256), 0, stream, fp, d_sorted,
                           opb.op, urows.uc);
        {
            unsigned long long e = 0;
            HIP_CHECK(hipStreamSynchronize(stream));
            HIP_CHECK(hipMemcpy(&e, d_err.p, 8, hipMemcpyDeviceToHost));
            if (e == 40) throw std::runtime_error("duplicate partition keys in flush input");
        }
        // header mins (SerializationHeader.make at flush: collect, then write).
        // k_flush_fill writes no TTL (live_ttl and every cell_ttl are 0), so
        // the collected min_ttl is never folded into and decodes to 0.
        DevBuf d_stats, d_tomb;
        uint32_t tomb_cap = (uint32_t)std::min<uint64_t>(n * 3 + 1024, 400000000ull);
        SerParams2 sp{};
        sp.hs = fresh_rows_header(opb, urows, n, 1u, 0u, d_stats, d_tomb, tomb_cap, stream);
        HostSchema hsch;
        hsch.col_fixed = {-1};  // val blob
        DevSchema dsch;
        sp.sch = dsch.upload(hsch, stream);
        TableTypes types;
        types.key_type = "org.apache.cassandra.db.marshal.BytesType";
        types.regular_cols = {{bytes{'v', 'a', 'l'}, "org.apache.cassandra.db.marshal.BytesType"}};
        OutputOptions opt;
        opt.base = output_base;
        write_sstable_device(opb, urows, n, sp, d_stats, d_tomb, tomb_cap, types, opt, stream);
        return GPUC_OK;
    });
}


// ---- full-schema memtable flush (gpuc_flush_table) -----------------------
// Memtable.FlushablePartitionSet -> SortedTablePartitionWriter: the caller
// hands partitions with within-partition clustering order already
// established (memtables are sorted maps); the engine token-sorts the
// partitions on device, validates order/uniqueness, marshals rows into the
// same OutParts/UnfCols layout the generator and parse kernels produce, and
// runs the shared writer kernels (serialize/compress/index/bloom/stats).
namespace flushv2 {

// host mirrors of the device ck encodings (kernels_rows.hip ck_sortable /
// ck_prefix_var)
static uint64_t h_ck_sortable(const uint8_t* p, int width) {
    uint64_t v = 0;
    for (int b = 0; b < width; b++) v = (v << 8) | p[b];
    return v ^ (1ULL << (8 * width - 1));
}
static uint64_t h_ck_prefix_var(const uint8_t* p, uint32_t len) {
    uint64_t v = 0;
    uint32_t n = len < 8 ? len : 8;
    for (uint32_t b = 0; b < n; b++) v |= (uint64_t)p[b] << (8 * (7 - b));
    return v;
}
static int h_bk_cmp_to_clustering(uint8_t kk) {
    static const int tbl[8] = {-1, -1, -1, -1, 0, 1, 1, 1};
    return tbl[kk];
}
static int h_bk_comparison(uint8_t k) {
    static const int tbl[8] = {0, 0, 0, 1, 2, 3, 3, 3};
    return tbl[k];
}

// ClusteringComparator.compare over two ABI unfiltereds (mirrors pos_cmp)
static int h_unf_cmp(const gpuc_unfiltered& a, const gpuc_unfiltered& b,
                     const std::vector<int32_t>& ckw, uint32_t ck_desc) {
    uint32_t mn = a.ck_count < b.ck_count ? a.ck_count : b.ck_count;
    for (uint32_t c = 0; c < mn; c++) {
        int32_t w = ckw[c];
        const uint8_t* pa = a.ck[c];
        const uint8_t* pb = b.ck[c];
        uint32_t la = a.ck_lens[c], lb = b.ck_lens[c];
        uint64_t sa, sb;
        if (w > 0) { sa = h_ck_sortable(pa, w); sb = h_ck_sortable(pb, w); }
        else { sa = h_ck_prefix_var(pa, la); sb = h_ck_prefix_var(pb, lb); }
        // a descending component: every value comparison negated (kinds are not)
        const int lt = (ck_desc >> c) & 1u ? 1 : -1;
        if (sa != sb) return sa < sb ? lt : -lt;
        if (w < 0) {
            uint32_t n = la < lb ? la : lb;
            for (uint32_t i = 8; i < n; i++)
                if (pa[i] != pb[i]) return pa[i] < pb[i] ? lt : -lt;
            if (la != lb) return la < lb ? lt : -lt;
        }
    }
    if (a.ck_count != b.ck_count)
        return a.ck_count < b.ck_count ? h_bk_cmp_to_clustering(a.kind)
                                       : -h_bk_cmp_to_clustering(b.kind);
    return h_bk_comparison(a.kind) - h_bk_comparison(b.kind);
}

// complex column x of a row: cpx_cols[x] when the caller gave the per-column
// array, else the legacy single-column fields stand for column 0
static gpuc_cpx_col cpx_col_of(const gpuc_unfiltered& U, uint32_t x) {
    if (U.cpx_cols) return U.cpx_cols[x];
    if (x == 0 && U.has_cpx)
        return gpuc_cpx_col{1, U.cpx_del_mfda, U.cpx_del_ldt, U.n_cpx_cells, U.cpx_cells};
    return gpuc_cpx_col{0, INT64_MIN, LDT_NONE_U32, 0, nullptr};
}
// CellPath order of the column's key type: the function the kernels run (cell_path.h)
static int h_path_cmp(const gpuc_cpx_cell& a, const gpuc_cpx_cell& b, bool key_signed) {
    return cell_path_cmp(a.path, a.path_len, b.path, b.path_len, key_signed);
}

}  // namespace flushv2

extern "C" int gpuc_flush_table(const gpuc_flush_schema* schema, const gpuc_flush_part* parts,
                                uint64_t n_parts, const char* output_base, int32_t device,
                                char* error, size_t error_len) {
    using namespace flushv2;
    return abi_guard(error, error_len, [&]() -> int {
        if (gpuc_device_count() <= 0) { set_err(error, error_len, "no HIP device"); return GPUC_ERR_NO_GPU; }
        if (!schema || !parts || n_parts == 0) throw std::runtime_error("no partitions");
        const gpuc_flush_schema& S = *schema;
        (void)checked_chunk_len_arg(S.chunk_length, CHUNK_LEN);  // before any work
        if (S.n_cols == 0 || S.n_cols + S.n_static > 63)
            throw std::runtime_error("1..63 columns supported");
        if (S.n_cpx > S.n_cols) throw std::runtime_error("n_cpx exceeds n_cols");
        if (S.n_ck > 32) throw std::runtime_error("at most 32 clustering columns");
        const std::string CTRT = "org.apache.cassandra.db.marshal.CounterColumnType";
        // the types go to the Statistics.db header as given; the widths the
        // kernels walk with: clustering types must be known (ck_type
        // throws), an unknown regular or static type is variable width
        TableTypes types;
        HostSchema hsch;
        types.key_type = S.key_type ? S.key_type : "org.apache.cassandra.db.marshal.BytesType";
        for (uint32_t i = 0; i < S.n_ck; i++) {
            types.clustering_types.emplace_back(S.ck_types[i]);
            hsch.add_ck(types.clustering_types.back());
        }
        const uint32_t ck_desc_h = hsch.ck_desc_mask();
        if (S.bti) refuse_bti_desc(types.clustering_types, "`bti` output");
        const std::vector<int32_t>& ckw_h = hsch.ck_widths;
        // n_cols in the ABI counts ALL regular columns; SchemaParams.n_cols
        // counts the SIMPLE ones (the n_cpx complex ones last, excluded)
        const uint32_t NSIMPLE = S.n_cols - S.n_cpx;
        const uint32_t NX = S.n_cpx;
        for (uint32_t i = 0; i < S.n_cols; i++) {
            std::string t(S.col_types[i]);
            if (multicell_type(t) != (i >= NSIMPLE))
                throw std::runtime_error(
                    "the complex (set, map) columns must be the last n_cpx regular columns");
            if (t == CTRT) hsch.counters = true;
            types.regular_cols.emplace_back(
                bytes(S.col_names[i], S.col_names[i] + S.col_name_lens[i]), t);
            if (i < NSIMPLE) hsch.col_fixed.push_back(type_width(t));
            else hsch.add_cpx(collection_type(t));  // throws for the refused types
        }
        // complex column x, by name, for the messages of the checks below
        auto cpx_label = [&](uint32_t x) { return column_label(types.regular_cols[NSIMPLE + x].first); };
        for (uint32_t i = 0; i < S.n_static; i++) {
            std::string t(S.static_types[i]);
            types.static_cols.emplace_back(
                bytes(S.static_names[i], S.static_names[i] + S.static_name_lens[i]), t);
            hsch.static_fixed.push_back(type_width(t));
        }
        // ---- pass 0: totals + validation ----
        uint64_t key_bytes = 0, n_unf = 0, val_bytes = 0, cpx_total = 0;
        for (uint64_t p = 0; p < n_parts; p++) {
            const gpuc_flush_part& P = parts[p];
            if (P.key_len == 0) throw std::runtime_error("empty partition key");
            key_bytes += P.key_len;
            n_unf += P.n_unf;
            if (P.static_flags && S.n_static)
                for (uint32_t c = 0; c < S.n_static; c++)
                    if (P.static_cells[c].flags & GPUC_CELLF_PRESENT)
                        val_bytes += P.static_cells[c].value_len;
            const gpuc_unfiltered* prev = nullptr;
            for (uint64_t r = 0; r < P.n_unf; r++) {
                const gpuc_unfiltered& U = P.unf[r];
                if (U.kind > 7 || U.kind == 3) throw std::runtime_error("bad unfiltered kind");
                bool is_row = U.kind == 4;
                if (is_row && U.ck_count != S.n_ck)
                    throw std::runtime_error("rows must have all clustering components");
                if (U.ck_count > S.n_ck) throw std::runtime_error("ck_count exceeds schema");
                for (uint32_t c = 0; c < U.ck_count; c++) {
                    int32_t w = ckw_h[c];
                    if (w > 0 && U.ck_lens[c] != (uint32_t)w)
                        throw std::runtime_error("fixed clustering component width mismatch");
                    if (w < 0) val_bytes += U.ck_lens[c];
                }
                if (is_row) {
                    for (uint32_t c = 0; c < NSIMPLE; c++)
                        if (U.cells[c].flags & GPUC_CELLF_PRESENT) val_bytes += U.cells[c].value_len;
                    if ((U.has_cpx || U.cpx_cols) && !S.n_cpx)
                        throw std::runtime_error("complex data on a schema without a complex column");
                    if (S.n_cpx >= 2 && U.has_cpx && !U.cpx_cols)
                        throw std::runtime_error(
                            "a row with complex data needs cpx_cols when the schema has "
                            "several complex columns");
                    for (uint32_t x = 0; x < S.n_cpx; x++) {
                        const gpuc_cpx_col X = cpx_col_of(U, x);
                        if (!X.present) continue;
                        cpx_total += X.n_cells;
                        for (uint32_t e = 0; e < X.n_cells; e++) {
                            const gpuc_cpx_cell& C = X.cells[e];
                            val_bytes += C.path_len + C.cell.value_len;
                            if (hsch.cpx_key_w[x] && C.path_len != hsch.cpx_key_w[x])
                                throw std::runtime_error(
                                    "cell path of " + std::to_string(C.path_len) +
                                    " bytes in column " + cpx_label(x) + ", whose key type is " +
                                    std::to_string(hsch.cpx_key_w[x]) + " bytes wide, in partition " +
                                    std::to_string(p));
                            // the writer sets the empty-value flag by length
                            if (hsch.cpx_set[x] && C.cell.value_len)
                                throw std::runtime_error("cell with a value in set column " +
                                                         cpx_label(x) + ", in partition " +
                                                         std::to_string(p));
                            if (e && h_path_cmp(X.cells[e - 1], C, hsch.cpx_key_w[x] != 0) >= 0)
                                throw std::runtime_error(
                                    "complex cells out of CellPath order in partition " +
                                    std::to_string(p) + ", complex column " + std::to_string(x) +
                                    " " + cpx_label(x));
                        }
                    }
                }
                if (prev && h_unf_cmp(*prev, U, ckw_h, ck_desc_h) >= 0)
                    throw std::runtime_error("unfiltereds out of clustering order in partition " +
                                             std::to_string(p));
                prev = &U;
            }
        }
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        ensure_crc_tables(stream);
        // ---- key arena + device partition sort (token, key bytes) ----
        std::vector<uint8_t> kbuf(key_bytes);
        std::vector<uint64_t> koff(n_parts + 1, 0);
        for (uint64_t p = 0; p < n_parts; p++) {
            memcpy(kbuf.data() + koff[p], parts[p].key, parts[p].key_len);
            koff[p + 1] = koff[p] + parts[p].key_len;
        }
        DevBuf d_keys, d_koff, d_a, d_b, d_koff_adj, d_err;
        d_keys.alloc(kbuf.size());
        d_koff.alloc((n_parts + 1) * 8);
        HIP_CHECK(hipMemcpyAsync(d_keys.p, kbuf.data(), kbuf.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(d_koff.p, koff.data(), (n_parts + 1) * 8, hipMemcpyHostToDevice, stream));
        FlushParams fp{};
        fp.keys = d_keys.as<uint8_t>();
        fp.key_off = d_koff.as<uint64_t>();
        fp.n = n_parts;
        d_a.alloc(n_parts * sizeof(MRec));
        d_b.alloc(n_parts * sizeof(MRec));
        uint32_t pblocks = (uint32_t)((n_parts + 255) / 256);
        hipLaunchKernelGGL(k_flush_recs, dim3(pblocks), dim3(256), 0, stream, fp, d_a.as<MRec>());
        std::vector<uint64_t> koff_adj(n_parts);
        for (uint64_t p = 0; p < n_parts; p++) koff_adj[p] = koff[p] - 2;
        d_koff_adj.alloc(n_parts * 8);
        HIP_CHECK(hipMemcpyAsync(d_koff_adj.p, koff_adj.data(), n_parts * 8, hipMemcpyHostToDevice, stream));
        KeyLut lut{};
        lut.base[0] = d_keys.as<uint8_t>();
        lut.pos[0] = d_koff_adj.as<uint64_t>();
        lut.enabled = 1;
        MRec* d_sorted = merge_sort_recs(d_a.as<MRec>(), d_b.as<MRec>(), n_parts, stream, lut);
        d_err.alloc(8);
        HIP_CHECK(hipMemsetAsync(d_err.p, 0, 8, stream));
        hipLaunchKernelGGL(k_flush_dupcheck, dim3(pblocks), dim3(256), 0, stream, fp, d_sorted,
                           d_err.as<unsigned long long>());
        std::vector<MRec> sorted(n_parts);
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipMemcpy(sorted.data(), d_sorted, n_parts * sizeof(MRec), hipMemcpyDeviceToHost));
        {
            unsigned long long e = 0;
            HIP_CHECK(hipMemcpy(&e, d_err.p, 8, hipMemcpyDeviceToHost));
            if (e) throw std::runtime_error("duplicate partition keys in flush input");
        }
        // ---- device layout + host mirrors (filled in sorted order) ----
        OutPartsBuf opb;
        opb.alloc(n_parts, S.n_static);
        UnfColsBuf urows;
        urows.alloc(n_unf, NSIMPLE ? NSIMPLE : 1, S.n_ck, S.n_cpx);
        if (S.n_cpx) urows.alloc_cpx_arena(cpx_total);
        DevBuf d_vals;
        d_vals.alloc(val_bytes ? val_bytes : 1);
        uint8_t* const VBASE = d_vals.as<uint8_t>();
        std::vector<uint8_t> h_vals(val_bytes ? val_bytes : 1);
        uint64_t vcur = 0;
        auto stash = [&](const uint8_t* src, uint32_t len) -> uint64_t {
            uint64_t at = (uint64_t)(VBASE + vcur);
            if (len) memcpy(h_vals.data() + vcur, src, len);
            vcur += len;
            return at;
        };
        const uint32_t NCK = S.n_ck ? S.n_ck : 1;
        const uint32_t NCV = NSIMPLE ? NSIMPLE : 1;
        const uint32_t NST = S.n_static ? S.n_static : 1;
        // OutParts host
        std::vector<uint64_t> h_keypfx(n_parts), h_keyaddr(n_parts), h_rowbase(n_parts);
        std::vector<int64_t> h_token(n_parts), h_pdelm(n_parts);
        std::vector<uint16_t> h_klen(n_parts);
        std::vector<uint32_t> h_pdell(n_parts), h_rowcnt(n_parts);
        std::vector<uint8_t> h_keep(n_parts, 1);
        // statics host
        std::vector<uint8_t> h_sflags(n_parts, 0), h_scf(n_parts * NST, 0);
        std::vector<int64_t> h_sts(n_parts, NO_TIMESTAMP), h_slet(n_parts, NO_DELETION_TIME),
            h_sdm(n_parts, INT64_MIN), h_scts(n_parts * NST, 0);
        std::vector<int32_t> h_sttl(n_parts, 0), h_scttl(n_parts * NST, 0);
        std::vector<uint32_t> h_sdl(n_parts, LDT_NONE_U32), h_scldt(n_parts * NST, 0),
            h_scvl(n_parts * NST, 0);
        std::vector<uint64_t> h_scva(n_parts * NST, 0);
        // UnfCols host
        std::vector<uint64_t> h_ck(n_unf * NCK, 0), h_ckaddr(n_unf * NCK, 0);
        std::vector<uint32_t> h_cklen(n_unf * NCK, 0);
        std::vector<uint8_t> h_ckcnt(n_unf, 0), h_rkind(n_unf), h_flags(n_unf, 0),
            h_cf(n_unf * NCV, 0);
        std::vector<int64_t> h_lts(n_unf, NO_TIMESTAMP), h_llet(n_unf, NO_DELETION_TIME),
            h_rdm(n_unf, INT64_MIN), h_sm(n_unf, INT64_MIN), h_cts(n_unf * NCV, 0);
        std::vector<int32_t> h_lttl(n_unf, 0), h_cttl(n_unf * NCV, 0);
        std::vector<uint32_t> h_rdl(n_unf, LDT_NONE_U32), h_sl(n_unf, LDT_NONE_U32),
            h_cldt(n_unf * NCV, 0), h_cvl(n_unf * NCV, 0);
        std::vector<uint64_t> h_cva(n_unf * NCV, 0);
        // per (unfiltered, complex column), strided by NX
        std::vector<uint8_t> h_xp(n_unf * NX, 0);
        std::vector<int64_t> h_xdm(n_unf * NX, INT64_MIN);
        std::vector<uint32_t> h_xdl(n_unf * NX, LDT_NONE_U32), h_xcnt(n_unf * NX, 0);
        std::vector<uint64_t> h_xstart(n_unf * NX, 0);
        std::vector<int64_t> h_xts(cpx_total);
        std::vector<uint32_t> h_xldt(cpx_total), h_xpl(cpx_total), h_xvl(cpx_total);
        std::vector<int32_t> h_xttl(cpx_total);
        std::vector<uint8_t> h_xf(cpx_total);
        std::vector<uint64_t> h_xpa(cpx_total), h_xva(cpx_total);
        auto conv_cell = [&](const gpuc_cell& C, int64_t* ts, uint32_t* ldt, int32_t* ttl,
                             uint64_t* va, uint32_t* vl, uint8_t* cf) {
            if (!(C.flags & GPUC_CELLF_PRESENT)) { *cf = 0; return; }
            uint8_t f = CELLF_PRESENT;
            if (C.flags & GPUC_CELLF_HAS_VALUE) f |= CELLF_HAS_VALUE;
            if (C.ttl != 0) f |= CELLF_EXPIRING;
            *cf = f;
            *ts = C.ts;
            *ldt = C.ldt;
            *ttl = C.ttl;
            *vl = C.value_len;
            *va = (C.flags & GPUC_CELLF_HAS_VALUE) ? stash(C.value, C.value_len)
                                                   : (uint64_t)VBASE;
        };
        uint64_t ob = 0, xcur = 0;
        for (uint64_t si = 0; si < n_parts; si++) {
            const uint64_t p = sorted[si].idx;
            const gpuc_flush_part& P = parts[p];
            h_keypfx[si] = sorted[si].pfx;
            h_token[si] = (int64_t)(sorted[si].tok ^ 0x8000000000000000ULL);
            h_keyaddr[si] = (uint64_t)(d_keys.as<uint8_t>() + koff[p]);
            h_klen[si] = P.key_len;
            h_pdelm[si] = P.pdel_mfda;
            h_pdell[si] = P.pdel_ldt;
            h_rowbase[si] = ob;
            h_rowcnt[si] = (uint32_t)P.n_unf;
            if (S.n_static && P.static_flags) {
                h_sflags[si] = P.static_flags & 7;  // PF_HAS_ROW|PF_LIVE_TS|PF_ROW_DEL
                h_sts[si] = P.static_live_ts;
                h_sttl[si] = P.static_live_ttl;
                h_slet[si] = P.static_live_let;
                h_sdm[si] = P.static_del_mfda;
                h_sdl[si] = P.static_del_ldt;
                for (uint32_t c = 0; c < S.n_static; c++)
                    conv_cell(P.static_cells[c], &h_scts[si * NST + c], &h_scldt[si * NST + c],
                              &h_scttl[si * NST + c], &h_scva[si * NST + c], &h_scvl[si * NST + c],
                              &h_scf[si * NST + c]);
            }
            for (uint64_t r = 0; r < P.n_unf; r++, ob++) {
                const gpuc_unfiltered& U = P.unf[r];
                h_rkind[ob] = U.kind;
                h_ckcnt[ob] = U.ck_count;
                // ascending encodings whatever the direction: the order was
                // checked on the host (h_unf_cmp) and the device only writes
                for (uint32_t c = 0; c < U.ck_count; c++) {
                    uint64_t oc = ob * NCK + c;
                    int32_t w = ckw_h[c];
                    if (w > 0) {
                        h_ck[oc] = h_ck_sortable(U.ck[c], w);
                        h_ckaddr[oc] = 0;
                        h_cklen[oc] = (uint32_t)w;
                    } else {
                        h_ck[oc] = h_ck_prefix_var(U.ck[c], U.ck_lens[c]);
                        h_ckaddr[oc] = stash(U.ck[c], U.ck_lens[c]);
                        h_cklen[oc] = U.ck_lens[c];
                    }
                }
                if (U.kind == 4) {
                    uint8_t f = PF_HAS_ROW;
                    if (U.row_flags & GPUC_ROWF_LIVE_TS) {
                        f |= PF_LIVE_TS;
                        h_lts[ob] = U.live_ts;
                        h_lttl[ob] = U.live_ttl;
                        h_llet[ob] = U.live_let;
                    }
                    if (U.row_flags & GPUC_ROWF_DELETED) {
                        f |= PF_ROW_DEL;
                        h_rdm[ob] = U.del_mfda;
                        h_rdl[ob] = U.del_ldt;
                    }
                    for (uint32_t c = 0; c < NSIMPLE; c++)
                        conv_cell(U.cells[c], &h_cts[ob * NCV + c], &h_cldt[ob * NCV + c],
                                  &h_cttl[ob * NCV + c], &h_cva[ob * NCV + c],
                                  &h_cvl[ob * NCV + c], &h_cf[ob * NCV + c]);
                    // a row's segments lie end to end in header order
                    for (uint32_t x = 0; x < NX; x++) {
                        const uint64_t ox = ob * NX + x;
                        const gpuc_cpx_col X = cpx_col_of(U, x);
                        h_xstart[ox] = xcur;
                        if (!X.present) continue;
                        f |= PF_HAS_CPX;
                        h_xp[ox] = 1;
                        h_xdm[ox] = X.del_mfda;
                        h_xdl[ox] = X.del_ldt;
                        h_xcnt[ox] = X.n_cells;
                        for (uint32_t e = 0; e < X.n_cells; e++, xcur++) {
                            const gpuc_cpx_cell& C = X.cells[e];
                            conv_cell(C.cell, &h_xts[xcur], &h_xldt[xcur], &h_xttl[xcur],
                                      &h_xva[xcur], &h_xvl[xcur], &h_xf[xcur]);
                            h_xpa[xcur] = stash(C.path, C.path_len);
                            h_xpl[xcur] = C.path_len;
                        }
                    }
                    h_flags[ob] = f;
                } else {
                    h_flags[ob] = 0;
                    h_rdm[ob] = U.del_mfda;
                    h_rdl[ob] = U.del_ldt;
                    if (U.kind == 2 || U.kind == 5) {  // boundary: open deletion
                        h_sm[ob] = U.open_mfda;
                        h_sl[ob] = U.open_ldt;
                    }
                    for (uint32_t x = 0; x < NX; x++) h_xstart[ob * NX + x] = xcur;
                }
            }
        }
        // ---- upload ----
        auto up = [&](const DevBuf& d, const void* src, size_t len) {
            if (len) HIP_CHECK(hipMemcpyAsync(d.p, src, len, hipMemcpyHostToDevice, stream));
        };
        up(d_vals, h_vals.data(), vcur);
        up(opb.keypfx, h_keypfx.data(), n_parts * 8);
        up(opb.key_addr, h_keyaddr.data(), n_parts * 8);
        up(opb.token, h_token.data(), n_parts * 8);
        up(opb.klen, h_klen.data(), n_parts * 2);
        up(opb.pdel_mfda, h_pdelm.data(), n_parts * 8);
        up(opb.pdel_ldt, h_pdell.data(), n_parts * 4);
        up(opb.row_base, h_rowbase.data(), n_parts * 8);
        up(opb.row_count, h_rowcnt.data(), n_parts * 4);
        up(opb.keep, h_keep.data(), n_parts);
        if (S.n_static) {
            up(opb.stb.flags, h_sflags.data(), n_parts);
            up(opb.stb.live_ts, h_sts.data(), n_parts * 8);
            up(opb.stb.live_ttl, h_sttl.data(), n_parts * 4);
            up(opb.stb.live_let, h_slet.data(), n_parts * 8);
            up(opb.stb.rdel_mfda, h_sdm.data(), n_parts * 8);
            up(opb.stb.rdel_ldt, h_sdl.data(), n_parts * 4);
            up(opb.stb.cell_flags, h_scf.data(), n_parts * NST);
            up(opb.stb.cell_ts, h_scts.data(), n_parts * NST * 8);
            up(opb.stb.cell_ldt, h_scldt.data(), n_parts * NST * 4);
            up(opb.stb.cell_ttl, h_scttl.data(), n_parts * NST * 4);
            up(opb.stb.val_addr, h_scva.data(), n_parts * NST * 8);
            up(opb.stb.val_len, h_scvl.data(), n_parts * NST * 4);
        }
        up(urows.ck, h_ck.data(), n_unf * NCK * 8);
        up(urows.ck_addr, h_ckaddr.data(), n_unf * NCK * 8);
        up(urows.ck_len, h_cklen.data(), n_unf * NCK * 4);
        up(urows.ck_count, h_ckcnt.data(), n_unf);
        up(urows.rkind, h_rkind.data(), n_unf);
        up(urows.flags, h_flags.data(), n_unf);
        up(urows.live_ts, h_lts.data(), n_unf * 8);
        up(urows.live_ttl, h_lttl.data(), n_unf * 4);
        up(urows.live_let, h_llet.data(), n_unf * 8);
        up(urows.rdel_mfda, h_rdm.data(), n_unf * 8);
        up(urows.rdel_ldt, h_rdl.data(), n_unf * 4);
        up(urows.start_mfda, h_sm.data(), n_unf * 8);
        up(urows.start_ldt, h_sl.data(), n_unf * 4);
        up(urows.cell_ts, h_cts.data(), n_unf * NCV * 8);
        up(urows.cell_ldt, h_cldt.data(), n_unf * NCV * 4);
        up(urows.cell_ttl, h_cttl.data(), n_unf * NCV * 4);
        up(urows.val_addr, h_cva.data(), n_unf * NCV * 8);
        up(urows.val_len, h_cvl.data(), n_unf * NCV * 4);
        up(urows.cell_flags, h_cf.data(), n_unf * NCV);
        if (S.n_cpx) {
            up(urows.cpx_present, h_xp.data(), n_unf * NX);
            up(urows.cpx_del_mfda, h_xdm.data(), n_unf * NX * 8);
            up(urows.cpx_del_ldt, h_xdl.data(), n_unf * NX * 4);
            up(urows.cpx_start, h_xstart.data(), n_unf * NX * 8);
            up(urows.cpx_count, h_xcnt.data(), n_unf * NX * 4);
            if (cpx_total) {
                up(urows.cx_ts, h_xts.data(), cpx_total * 8);
                up(urows.cx_ldt, h_xldt.data(), cpx_total * 4);
                up(urows.cx_ttl, h_xttl.data(), cpx_total * 4);
                up(urows.cx_flags, h_xf.data(), cpx_total);
                up(urows.cx_pa, h_xpa.data(), cpx_total * 8);
                up(urows.cx_pl, h_xpl.data(), cpx_total * 4);
                up(urows.cx_va, h_xva.data(), cpx_total * 8);
                up(urows.cx_vl, h_xvl.data(), cpx_total * 4);
            }
        }
        // ---- header mins from a pre-collect (gpuc_generate's recipe) ----
        DevSchema dsch;
        SerParams2 sp{};
        sp.sch = dsch.upload(hsch, stream,
                             S.column_index_size ? S.column_index_size : 64 * 1024);
        DevBuf d_stats, d_tomb;
        uint32_t tomb_cap = tomb_list_cap(n_unf, cpx_total, n_parts, sp.sch);
        sp.hs = fresh_rows_header(opb, urows, n_parts, NCV, NX, d_stats, d_tomb, tomb_cap, stream);
        if (S.has_stats) {
            // caller-provided EncodingStats (Memtable -> SerializationHeader.make)
            sp.hs.min_ts = S.stats_min_ts;
            sp.hs.min_ldt = S.stats_min_ldt;
            sp.hs.min_ttl = S.stats_min_ttl;
        }
        write_sstable_device(opb, urows, n_parts, sp, d_stats, d_tomb, tomb_cap, types,
                             OutputOptions{output_base, S.snappy != 0, S.bti != 0,
                                           checked_chunk_len_arg(S.chunk_length, CHUNK_LEN), 0},
                             stream);
        return GPUC_OK;
    });
}

// job modes neither validation entry point takes
static bool validate_mode_rejected(const gpuc_job* job, char* error, size_t error_len) {
    if (job->n_output_shards > 1 || job->max_output_bytes || job->n_tomb_sources > 0 ||
        job->n_keep_ranges > 0) {
        set_err(error, error_len,
                "validation: sharding/size-split/tomb-source/keep-range modes unsupported");
        return true;
    }
    return false;
}

extern "C" int gpuc_validate_merkle(const gpuc_job* job, const gpuc_merkle_spec* spec,
                                    uint8_t* leaf_hash, uint64_t* leaf_partitions,
                                    uint64_t* n_partitions, char* error, size_t error_len) {
    // argument checks first: no device is probed and no input byte read
    if (validate_mode_rejected(job, error, error_len)) return GPUC_ERR_UNSUPPORTED;
    std::string bad = merkle_spec_error(spec);
    if (bad.empty() && !leaf_hash) bad = "merkle: leaf_hash is NULL";
    if (!bad.empty()) {
        set_err(error, error_len, bad);
        return GPUC_ERR_UNSUPPORTED;
    }
    gpuc_result res{};
    MerkleRun run{spec, leaf_hash, leaf_partitions, 0};
    gpuc_job vjob = *job;
    if (!vjob.output_base) vjob.output_base = "/unused";  // nothing is written
    CompactMode mode;
    mode.merkle = &run;
    int rc = run_compaction(&vjob, &res, mode);
    if (rc == GPUC_OK && n_partitions) *n_partitions = run.n_partitions;
    if (rc != GPUC_OK) set_err(error, error_len, res.error);
    return rc;
}

extern "C" int gpuc_compact_routed(const gpuc_job* job, const gpuc_route_spec* spec,
                                   gpuc_result* res, gpuc_route_output* outputs) {
    // argument checks first: no device is probed and no input byte read
    std::string bad;
    if (job->n_keep_ranges > 0) bad = "routed outputs: keep_ranges unsupported (route by the spec)";
    else if (job->n_output_shards > 1) bad = "routed outputs: n_output_shards unsupported";
    else if (job->max_output_bytes) bad = "routed outputs: max_output_bytes unsupported";
    else bad = route_spec_error(spec);
    if (!bad.empty()) {
        memset(res, 0, sizeof(*res));
        set_err(res->error, sizeof(res->error), bad);
        return GPUC_ERR_UNSUPPORTED;
    }
    if (outputs) memset(outputs, 0, sizeof(*outputs) * spec->n_outputs);
    RouteRun run{spec, outputs};
    gpuc_job rjob = *job;
    rjob.output_base = spec->output_bases[0];  // unused: every output has its own base
    CompactMode mode;
    mode.route = &run;
    return run_compaction(&rjob, res, mode);
}

extern "C" int gpuc_validate(const gpuc_job* job, const char* out_path, uint64_t* n_partitions,
                             char* error, size_t error_len) {
    if (validate_mode_rejected(job, error, error_len)) return GPUC_ERR_UNSUPPORTED;
    gpuc_result res{};
    uint64_t count = 0;
    CompactMode mode;
    mode.digest_path = out_path;
    mode.digest_count = &count;
    int rc = run_compaction(job, &res, mode);
    if (rc == GPUC_OK && n_partitions) *n_partitions = count;
    if (rc != GPUC_OK) set_err(error, error_len, res.error);
    return rc;
}

extern "C" int gpuc_generate(const gpuc_gen_spec* spec, const char* dir, char* error, size_t error_len) {
    return abi_guard(error, error_len, [&]() -> int {
        if (gpuc_device_count() <= 0) { set_err(error, error_len, "no HIP device"); return GPUC_ERR_NO_GPU; }
        (void)checked_chunk_len_arg(spec->chunk_length, CHUNK_LEN);  // before any work
        HIP_CHECK(hipSetDevice(spec->device));
        Stream stream;
        ensure_crc_tables(stream);
        uint64_t R = spec->rows_per_sstable;
        uint64_t stride = R * (100 - spec->overlap_pct) / 100;
        uint64_t universe = std::max<uint64_t>(stride * spec->n_sstables, R);
        for (uint32_t s = 0; s < spec->n_sstables; s++) {
            GenParams2 gp{};
            gp.seed = spec->seed;
            gp.universe = universe;
            gp.stride = stride;
            gp.rows = R;
            gp.sst = s;
            gp.value_len = spec->value_len;
            gp.value_repeat_pct = spec->value_repeat_pct;
            gp.tombstone_pct = spec->tombstone_pct;
            gp.partition_del_pct = spec->partition_del_pct;
            gp.clustering_rows = spec->clustering_rows;
            gp.range_tomb_pct = spec->range_tomb_pct;
            gp.base_ts = spec->base_ts;
            gp.base_ldt = spec->base_ldt;
            gp.key_len = spec->key_len ? spec->key_len : 8;
            gp.ck_text = spec->ck_text;
            gp.n_value_cols = spec->n_value_cols ? spec->n_value_cols : 1;
            gp.ck_cols = spec->ck_cols;
            gp.static_pct = spec->static_pct;
            if (gp.ck_cols > 2) throw std::runtime_error("ck_cols must be 0..2");
            if (gp.ck_cols == 2 && gp.ck_text) throw std::runtime_error("ck_cols=2 with ck_text unsupported");
            gp.col_missing_pct = spec->col_missing_pct;
            gp.ttl_pct = spec->ttl_pct;
            gp.complex_pct = spec->complex_pct;
            gp.complex_del_pct = spec->complex_del_pct;
            gp.counter = spec->counter;
            if (gp.counter) {
                if (gp.complex_pct || spec->static_pct || spec->ttl_pct || gp.n_value_cols > 1)
                    throw std::runtime_error("counter mode: single counter column only");
                gp.value_len = 274;  // context arena stride (8-shard worst case)
                // sorted CounterId pool (oracle gen.h gen_counter_id)
                struct P { uint8_t id[16]; uint8_t idx; };
                std::vector<P> pool(8);
                for (uint32_t i = 0; i < 8; i++) {
                    uint64_t a = splitmix64(0xC0C0C0C0ULL + i), b = splitmix64(0xF00DF00DULL + i);
                    for (int x = 0; x < 8; x++) pool[i].id[x] = (uint8_t)(a >> (8 * (7 - x)));
                    for (int x = 0; x < 8; x++) pool[i].id[8 + x] = (uint8_t)(b >> (8 * (7 - x)));
                    pool[i].idx = (uint8_t)i;
                }
                std::sort(pool.begin(), pool.end(), [](const P& x, const P& y) {
                    return memcmp(x.id, y.id, 16) < 0;
                });
                for (int i = 0; i < 8; i++) {
                    memcpy(gp.ctr_pool[i], pool[i].id, 16);
                    gp.ctr_pool_idx[i] = pool[i].idx;
                }
            }
            if (gp.n_value_cols > 63) throw std::runtime_error("n_value_cols must be 1..63");
            if (gp.ck_text && (uint64_t)gp.clustering_rows * 16 >= 100000000ull)
                throw std::runtime_error("ck_text needs clustering_rows*16 < 1e8 (8-digit order)");
            if (gp.key_len < 8 || gp.key_len > 255)
                throw std::runtime_error("key_len must be 8..255 (generator contract)");
            KeyLut lut{};  // generated 8-byte prefixes are unique: prefix compare is exact
            DevBuf d_a, d_b, d_ids, d_keys, d_vals, d_stats, d_tomb, d_prows;
            d_a.alloc(R * sizeof(MRec));
            d_b.alloc(R * sizeof(MRec));
            d_ids.alloc(R * 8);
            d_keys.alloc(R * (uint64_t)gp.key_len);
            uint32_t blocks = (uint32_t)((R + 255) / 256);
            hipLaunchKernelGGL(k_gen_recs2, dim3(blocks), dim3(256), 0, stream, gp,
                               d_a.as<MRec>(), d_ids.as<uint64_t>(), d_keys.as<uint8_t>());
            MRec* d_sorted = merge_sort_recs(d_a.as<MRec>(), d_b.as<MRec>(), R, stream, lut);
            OutPartsBuf opb;
            opb.alloc(R, gp.static_pct ? 1 : 0);
            d_prows.alloc(R * 8);
            DevBuf d_cpxcnt, d_cpxbytes;
            if (gp.complex_pct) d_cpxcnt.alloc(R * 8 + 8);
            hipLaunchKernelGGL(k_gen_count, dim3(blocks), dim3(256), 0, stream, gp, d_sorted,
                               d_ids.as<uint64_t>(), R, opb.op, d_prows.as<uint64_t>(),
                               d_keys.as<uint8_t>(),
                               gp.complex_pct ? d_cpxcnt.as<uint64_t>() : nullptr);
            uint64_t total_cpx = gp.complex_pct ? exscan_u64(d_cpxcnt.as<uint64_t>(), R, stream) : 0;
            uint64_t total_rows = exscan_u64(d_prows.as<uint64_t>(), R, stream);
            UnfColsBuf rows;
            uint32_t gen_nck = gp.clustering_rows ? (gp.ck_cols ? gp.ck_cols : 1) : 0;
            rows.alloc(total_rows, gp.n_value_cols, gen_nck, gp.complex_pct ? 1 : 0);
            if (gp.complex_pct) {
                rows.alloc_cpx_arena(total_cpx);
                d_cpxbytes.alloc(total_cpx * 12 + 16);  // 4B path + 8B value per cell
            }
            d_vals.alloc(total_rows * (uint64_t)gp.n_value_cols * spec->value_len);
            DevBuf d_ckarena, d_svals;
            if (gp.ck_text) d_ckarena.alloc(total_rows * 16 + 16);
            if (gp.static_pct) d_svals.alloc(R * (uint64_t)spec->value_len + 16);
            hipLaunchKernelGGL(k_gen_fill2, dim3(blocks), dim3(256), 0, stream, gp, d_sorted,
                               d_ids.as<uint64_t>(), R, opb.op, rows.uc, d_prows.as<uint64_t>(),
                               d_vals.as<uint8_t>(), gp.ck_text ? d_ckarena.as<uint8_t>() : nullptr,
                               gp.static_pct ? d_svals.as<uint8_t>() : nullptr,
                               gp.complex_pct ? d_cpxbytes.as<uint8_t>() : nullptr,
                               gp.complex_pct ? d_cpxcnt.as<uint64_t>() : nullptr);
            hipLaunchKernelGGL(k_gen_values2, dim3(blocks), dim3(256), 0, stream, gp, d_sorted,
                               d_ids.as<uint64_t>(), opb.op, rows.uc, R, d_vals.as<uint8_t>(),
                               d_prows.as<uint64_t>());
            // the generator's own bound: at most 7 cells per complex column
            uint32_t tomb_cap = (uint32_t)std::min<uint64_t>(
                total_rows * ((uint64_t)gp.n_value_cols + (gp.complex_pct ? 7 : 0) + 2) +
                    R * 3 + 1024,
                400000000ull);
            SerParams2 sp{};
            sp.hs = fresh_rows_header(opb, rows, R, gp.n_value_cols, gp.complex_pct ? 1u : 0u,
                                      d_stats, d_tomb, tomb_cap, stream);
            HostSchema hsch;
            hsch.ck_widths.assign(gen_nck, gp.ck_text ? -1 : 8);
            hsch.col_fixed.assign(gp.n_value_cols, -1);          // val blobs
            hsch.static_fixed.assign(gp.static_pct ? 1 : 0, -1);  // blob
            hsch.n_cpx = gp.complex_pct ? 1 : 0;
            DevSchema dsch;
            sp.sch = dsch.upload(hsch, stream);
            TableTypes types;
            std::vector<std::pair<bytes, std::string>>& cols = types.regular_cols;
            if (gp.counter) {
                cols.push_back({bytes{'c', 'n', 't'}, "org.apache.cassandra.db.marshal.CounterColumnType"});
            } else if (gp.n_value_cols == 1) {
                cols.push_back({bytes{'v', 'a', 'l'}, "org.apache.cassandra.db.marshal.BytesType"});
            } else {
                for (uint32_t c = 0; c < gp.n_value_cols; c++) {
                    std::string nm = "val" + std::to_string(c);
                    cols.push_back({bytes(nm.begin(), nm.end()),
                                    "org.apache.cassandra.db.marshal.BytesType"});
                }
            }
            if (gp.complex_pct)
                cols.push_back({bytes{'z', 'm'}, "org.apache.cassandra.db.marshal.MapType(org.apache.cassandra.db.marshal.BytesType,org.apache.cassandra.db.marshal.BytesType)"});
            if (gp.static_pct)
                types.static_cols.push_back({bytes{'s', '0'}, "org.apache.cassandra.db.marshal.BytesType"});
            types.key_type = gp.key_len > 8 ? "org.apache.cassandra.db.marshal.BytesType"
                                            : "org.apache.cassandra.db.marshal.LongType";
            types.clustering_types.assign(gen_nck, gp.ck_text
                                                       ? "org.apache.cassandra.db.marshal.UTF8Type"
                                                       : "org.apache.cassandra.db.marshal.LongType");
            OutputOptions opt;
            opt.base = std::string(dir) + (spec->bti ? "/da-" : "/oa-") +
                       std::to_string(spec->first_generation + s) + (spec->bti ? "-bti" : "-big");
            opt.snappy = spec->snappy != 0;
            opt.bti = spec->bti != 0;
            opt.chunk_len = checked_chunk_len_arg(spec->chunk_length, CHUNK_LEN);
            write_sstable_device(opb, rows, R, sp, d_stats, d_tomb, tomb_cap, types, opt, stream);
        }
        return GPUC_OK;
    });
}


// Diagnostic: chunk-compress a host buffer with the writer's own launch
// (launch_chunk_compress + k_chunk_gather) and hand back the Data.db image.
extern "C" int gpuc_compress_buffer(const uint8_t* data, uint64_t len, uint32_t chunk_length,
                                    int32_t snappy, int32_t device, uint8_t* out,
                                    uint64_t out_cap, uint64_t* out_len, uint64_t* offsets,
                                    uint32_t offsets_cap, uint32_t* n_chunks_out, char* error,
                                    size_t error_len) {
    try {
        if (gpuc_device_count() <= 0) { set_err(error, error_len, "no HIP device"); return GPUC_ERR_NO_GPU; }
        const uint32_t cl = checked_chunk_len_arg(chunk_length, CHUNK_LEN);
        if (!data && len) throw unsupported_error("null data");
        if ((len + cl - 1) / cl > 0x7FFFFFFFull) throw unsupported_error("buffer too large");
        const uint32_t n_chunks = (uint32_t)((len + cl - 1) / cl);
        if (n_chunks > offsets_cap) throw unsupported_error("offsets_cap too small");
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        ensure_crc_tables(stream);
        const uint32_t stride = snappy ? snp_slot_stride(cl) : lz4_slot_stride(cl);
        uint64_t total = 0;
        if (n_chunks) {
            DevBuf d_in, d_slots, d_csize, d_ccrc, d_foff, d_gat;
            d_in.alloc(len);
            d_slots.alloc((uint64_t)n_chunks * stride + 16);
            d_csize.alloc((uint64_t)n_chunks * 4 + 16);
            d_ccrc.alloc((uint64_t)n_chunks * 4 + 16);
            HIP_CHECK(hipMemcpyAsync(d_in.p, data, len, hipMemcpyHostToDevice, stream));
            launch_chunk_compress(snappy != 0, d_in.as<uint8_t>(), len, d_slots.as<uint8_t>(),
                                  d_csize.as<uint32_t>(), d_ccrc.as<uint32_t>(), n_chunks, cl,
                                  stride, stream);
            std::vector<uint32_t> cs(n_chunks);
            HIP_CHECK(hipMemcpyAsync(cs.data(), d_csize.p, (uint64_t)n_chunks * 4,
                                     hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            std::vector<uint64_t> fo(n_chunks);
            uint64_t acc = 0;
            for (uint32_t c = 0; c < n_chunks; c++) {
                if (cs[c] > stride) throw std::runtime_error("compressed chunk exceeds its slot");
                fo[c] = acc;
                offsets[c] = acc + (uint64_t)c * 4;  // CompressionInfo.db offsets
                acc += cs[c];
            }
            total = acc + (uint64_t)n_chunks * 4;
            if (total > out_cap) throw unsupported_error("out_cap too small");
            d_foff.alloc((uint64_t)n_chunks * 8);
            d_gat.alloc(total);
            HIP_CHECK(hipMemcpyAsync(d_foff.p, fo.data(), (uint64_t)n_chunks * 8,
                                     hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(k_chunk_gather, dim3(n_chunks), dim3(WAVE), 0, stream,
                               d_slots.as<uint8_t>(), d_csize.as<uint32_t>(),
                               d_ccrc.as<uint32_t>(), d_foff.as<uint64_t>(), d_gat.as<uint8_t>(),
                               n_chunks, stride);
            HIP_CHECK(hipMemcpyAsync(out, d_gat.p, total, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        if (out_len) *out_len = total;
        if (n_chunks_out) *n_chunks_out = n_chunks;
        return GPUC_OK;
    } catch (const unsupported_error& e) {
        set_err(error, error_len, e.what());
        return GPUC_ERR_UNSUPPORTED;
    } catch (const std::exception& e) {
        set_err(error, error_len, e.what());
        return GPUC_ERR_INTERNAL;
    }
}

// Diagnostic: the cut points of the size-split writer over a host buffer,
// through plan_size_cut (the writer's own launches: launch_chunk_compress and
// k_size_cut), with part_ends standing in for the serialized partitions.
extern "C" int gpuc_plan_size_cuts(const uint8_t* data, uint64_t len, const uint64_t* part_ends,
                                   uint64_t n_parts, uint32_t chunk_length, int32_t snappy,
                                   uint64_t max_output_bytes, int32_t device, uint64_t* cut_after,
                                   uint64_t cut_cap, uint64_t* n_cuts, char* error,
                                   size_t error_len) {
    try {
        if (gpuc_device_count() <= 0) { set_err(error, error_len, "no HIP device"); return GPUC_ERR_NO_GPU; }
        const uint32_t cl = checked_chunk_len_arg(chunk_length, CHUNK_LEN);
        if (!max_output_bytes) throw unsupported_error("max_output_bytes must be above 0");
        if ((!data && len) || (!part_ends && n_parts)) throw unsupported_error("null data");
        std::vector<uint64_t> P_h(n_parts + 1, 0);
        std::vector<uint8_t> keep(n_parts ? n_parts : 1, 0);
        for (uint64_t i = 0; i < n_parts; i++) {
            if (part_ends[i] < P_h[i] || part_ends[i] > len)
                throw unsupported_error("part_ends must be non-decreasing and within the buffer");
            P_h[i + 1] = part_ends[i];
            keep[i] = part_ends[i] > P_h[i];
        }
        uint64_t cuts = 0;
        const uint64_t total = P_h[n_parts];
        if (total) {
            HIP_CHECK(hipSetDevice(device));
            Stream stream;
            ensure_crc_tables(stream);
            DevBuf d_in, d_P, d_keep;
            d_in.alloc(total);
            d_P.alloc((n_parts + 1) * 8);
            d_keep.alloc(n_parts);
            HIP_CHECK(hipMemcpyAsync(d_in.p, data, total, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(d_P.p, P_h.data(), (n_parts + 1) * 8, hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(d_keep.p, keep.data(), n_parts, hipMemcpyHostToDevice, stream));
            CutPlan cp;
            for (uint64_t g0 = 0; g0 < n_parts && P_h[g0] < total;) {
                uint64_t g_last = plan_size_cut(cp, P_h, d_P.as<uint64_t>(), d_keep.as<uint8_t>(), g0,
                                                d_in.as<uint8_t>(), 1.0, snappy != 0, cl,
                                                max_output_bytes, [](uint64_t) {}, stream);
                if (g_last + 1 < n_parts && P_h[g_last + 1] < total) {
                    if (cuts >= cut_cap) throw unsupported_error("cut_cap too small");
                    cut_after[cuts++] = g_last;
                }
                g0 = g_last + 1;
            }
        }
        if (n_cuts) *n_cuts = cuts;
        return GPUC_OK;
    } catch (const unsupported_error& e) {
        set_err(error, error_len, e.what());
        return GPUC_ERR_UNSUPPORTED;
    } catch (const std::exception& e) {
        set_err(error, error_len, e.what());
        return GPUC_ERR_INTERNAL;
    }
}
