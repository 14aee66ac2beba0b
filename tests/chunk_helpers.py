"""CPU-only helpers for the chunk-length tests: re-chunk an LZ4 sstable to
another chunk length with the system liblz4 (the library the oracle links),
then have the oracle rewrite it, so inputs at any chunk length never depend
on GPU code. Also the eight content modes of tests/native/lz4_wave_sim.cpp
and CPU reference images for the direct codec test."""
import ctypes
import ctypes.util
import os
import shutil
import struct
import subprocess
import zlib

from conftest import ORACLE

OA_COMPONENTS = ["Data.db", "Index.db", "CompressionInfo.db", "Filter.db",
                 "Digest.crc32", "Statistics.db", "Summary.db", "TOC.txt"]
DA_COMPONENTS = ["Data.db", "Partitions.db", "Rows.db", "CompressionInfo.db", "Filter.db",
                 "Digest.crc32", "Statistics.db", "TOC.txt"]

_lz4 = None


def lz4():
    global _lz4
    if _lz4 is None:
        lib = ctypes.CDLL("liblz4.so.1")
        lib.LZ4_compress_default.argtypes = [ctypes.c_char_p, ctypes.c_char_p,
                                             ctypes.c_int, ctypes.c_int]
        lib.LZ4_compress_default.restype = ctypes.c_int
        lib.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p,
                                            ctypes.c_int, ctypes.c_int]
        lib.LZ4_decompress_safe.restype = ctypes.c_int
        lib.LZ4_compressBound.argtypes = [ctypes.c_int]
        lib.LZ4_compressBound.restype = ctypes.c_int
        _lz4 = lib
    return _lz4


def snappy():
    """libsnappy's C API, or None where the library is absent."""
    for name in ("libsnappy.so.1", "/opt/conda/lib/libsnappy.so.1",
                 "/usr/lib/x86_64-linux-gnu/libsnappy.so.1"):
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        lib.snappy_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                        ctypes.POINTER(ctypes.c_size_t)]
        lib.snappy_compress.restype = ctypes.c_int
        lib.snappy_max_compressed_length.argtypes = [ctypes.c_size_t]
        lib.snappy_max_compressed_length.restype = ctypes.c_size_t
        return lib
    return None


def lz4_payload(chunk):
    """LZ4Compressor chunk payload: 4-byte LE length + LZ4 block."""
    lib = lz4()
    cap = lib.LZ4_compressBound(len(chunk))
    buf = ctypes.create_string_buffer(cap)
    n = lib.LZ4_compress_default(bytes(chunk), buf, len(chunk), cap)
    assert n > 0
    return struct.pack("<I", len(chunk)) + buf.raw[:n]


def snappy_payload(chunk, lib):
    cap = lib.snappy_max_compressed_length(len(chunk))
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(cap)
    assert lib.snappy_compress(bytes(chunk), len(chunk), buf, ctypes.byref(n)) == 0
    return buf.raw[:n.value]


def chunk_image(raw, chunk_len, payload_fn):
    """Data.db image (per chunk: payload, BE CRC32 of the payload) + offsets."""
    out, offsets = bytearray(), []
    for o in range(0, len(raw), chunk_len):
        p = payload_fn(raw[o:o + chunk_len])
        offsets.append(len(out))
        out += p + struct.pack(">I", zlib.crc32(p))
    return bytes(out), offsets


def parse_compression_info(b):
    """-> (name, options-bytes, chunk_len, max_compressed, data_len, offsets)"""
    o = 0
    (nl,) = struct.unpack_from(">H", b, o); o += 2
    name = b[o:o + nl]; o += nl
    opt0 = o
    (nopt,) = struct.unpack_from(">I", b, o); o += 4
    for _ in range(nopt):
        for _kv in range(2):
            (l,) = struct.unpack_from(">H", b, o); o += 2 + l
    opts = b[opt0:o]
    chunk_len, max_comp, data_len, n = struct.unpack_from(">IIQI", b, o); o += 20
    offsets = list(struct.unpack_from(f">{n}Q", b, o))
    return name, opts, chunk_len, max_comp, data_len, offsets


def make_compression_info(name, opts, chunk_len, max_comp, data_len, offsets):
    return (struct.pack(">H", len(name)) + name + opts +
            struct.pack(">IIQI", chunk_len, max_comp, data_len, len(offsets)) +
            struct.pack(f">{len(offsets)}Q", *offsets))


def read_uncompressed(base):
    """Decode an LZ4 sstable's Data.db through its CompressionInfo.db."""
    with open(base + "-CompressionInfo.db", "rb") as f:
        name, _opts, chunk_len, _mc, data_len, offsets = parse_compression_info(f.read())
    assert name == b"LZ4Compressor", name
    with open(base + "-Data.db", "rb") as f:
        data = f.read()
    lib = lz4()
    out = bytearray()
    for i, off in enumerate(offsets):
        end = offsets[i + 1] if i + 1 < len(offsets) else len(data)
        payload = data[off:end - 4]
        assert zlib.crc32(payload) == struct.unpack(">I", data[end - 4:end])[0]
        (ulen,) = struct.unpack_from("<I", payload, 0)
        buf = ctypes.create_string_buffer(max(ulen, 1))
        got = lib.LZ4_decompress_safe(payload[4:], buf, len(payload) - 4, ulen)
        assert got == ulen, (got, ulen)
        out += buf.raw[:ulen]
    assert len(out) == data_len
    return bytes(out)


def write_chunked(src_base, dst_base, raw, chunk_len, image=None, offsets=None, name=None):
    """Copy src_base's components to dst_base with Data.db / CompressionInfo.db
    / Digest.crc32 replaced by the given (or liblz4-built) chunk image."""
    with open(src_base + "-CompressionInfo.db", "rb") as f:
        sname, opts, _cl, max_comp, _dl, _offs = parse_compression_info(f.read())
    if image is None:
        image, offsets = chunk_image(raw, chunk_len, lz4_payload)
    os.makedirs(os.path.dirname(dst_base), exist_ok=True)
    prefix = os.path.basename(src_base) + "-"
    for fn in os.listdir(os.path.dirname(src_base)):
        if fn.startswith(prefix) and not fn.endswith(".memdump"):
            shutil.copyfile(os.path.join(os.path.dirname(src_base), fn),
                            dst_base + "-" + fn[len(prefix):])
    with open(dst_base + "-Data.db", "wb") as f:
        f.write(image)
    with open(dst_base + "-CompressionInfo.db", "wb") as f:
        f.write(make_compression_info(name or sname, opts, chunk_len, max_comp, len(raw),
                                      offsets))
    with open(dst_base + "-Digest.crc32", "wb") as f:
        f.write(str(zlib.crc32(image)).encode())


def rechunk(src_base, dst_base, chunk_len, scratch_dir):
    """Oracle-written copy of the LZ4 sstable src_base at chunk_len: re-chunk
    with liblz4 into scratch_dir, then `oracle_tool rewrite` to dst_base (so
    Statistics.db's compression ratio matches the new chunking)."""
    raw = read_uncompressed(src_base)
    tmp = os.path.join(scratch_dir, os.path.basename(src_base))
    write_chunked(src_base, tmp, raw, chunk_len)
    os.makedirs(os.path.dirname(dst_base), exist_ok=True)
    subprocess.run([ORACLE, "rewrite", tmp, dst_base], check=True, capture_output=True)
    return dst_base


def chunk_length_of(base):
    with open(base + "-CompressionInfo.db", "rb") as f:
        return parse_compression_info(f.read())[2]


def _sm(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def content(mode, n, seed=1):
    """The eight content modes of tests/native/lz4_wave_sim.cpp (same shapes;
    the byte streams need not match the C++ ones, references are computed
    from these bytes)."""
    import numpy as np
    i = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(seed * 1000 + mode)
    rnd = rng.integers(0, 256, n, dtype=np.uint8)
    if mode == 0:
        b = rnd
    elif mode == 1:
        b = np.zeros(n, np.uint8)
    elif mode == 2:
        q = rng.integers(0, 256, (n + 7) // 8, dtype=np.uint8)
        b = np.repeat(q, 8)[:n] ^ (i % 8).astype(np.uint8)
    elif mode == 3:
        b = np.where(i % 3 != 0, (97 + i % 17).astype(np.uint8), rnd)
    elif mode == 4:
        q = rng.integers(0, 26, (n + 3) // 4, dtype=np.uint8)
        b = (97 + np.repeat(q, 4)[:n]).astype(np.uint8)
    elif mode == 5:
        b = np.where(i % 512 == 0, rnd, np.uint8(0x42))
    elif mode == 6:
        b = ((i // 100) & 0xFF).astype(np.uint8)
    else:
        b = rnd % 4
    return np.asarray(b, dtype=np.uint8).tobytes()
