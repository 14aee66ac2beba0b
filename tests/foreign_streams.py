"""CPU-only helpers for the foreign-stream tests: LZ4 blocks and Snappy
fragments as OTHER encoders write them (LZ4HC, LZ4 fast, hand-transcoded
streams with split matches, demoted match heads, widened Snappy literal
fields, copy-4 tags, 1..3-byte copies), over plaintext whose bytes are chosen
so that short periodic offsets and far offsets occur.

An op is ("lit", bytes) or ("copy", offset, length). For each codec there is
a wire parser, a plain reference decoder (run_ops) and an emitter; a variant
is a function chunk -> payload usable as payload_fn of
chunk_helpers.chunk_image. census() reports what a set of streams contains,
so that the tests can require the shapes they are about. No GPU code here."""
import ctypes
import os
import random
import struct
import subprocess
import zlib

import chunk_helpers as ch
from conftest import ORACLE

SNAPPY_NAME = b"SnappyCompressor"
CHUNK_LENGTHS = (1024, 16384, 65536)


# the decoders' frame bounds (codec.h: lz4_max_comp / snp_max_comp)
def lz4_bound(n):
    return 4 + n + n // 255 + 16


def snappy_bound(n):
    return 32 + n + n // 6


def frame_bound(codec, n):
    return lz4_bound(n) if codec == "lz4" else snappy_bound(n)


# ---- plaintext --------------------------------------------------------------
VALUE_LEN = 1800
PERIODS = (1, 2, 3, 4, 5, 6, 7)


def periodic(p, n, salt):
    """n bytes of exact minimal period p (p distinct non-zero bytes)."""
    pat = bytes((37 * salt + 11 * j) % 251 + 1 for j in range(p))
    return (pat * (n // p + 1))[:n]


def rows():
    """~80 rows of ~1800-byte values: the eight content modes, periods 1..7,
    one run of 3000 zero bytes, one value whose tail repeats its head 2047
    bytes back (Snappy copy-1's largest offset), and one random value shared
    by every 16th row (far offsets inside a 64 KiB chunk)."""
    shared = ch.content(0, VALUE_LEN, seed=99)
    far = ch.content(0, 2047, seed=98)
    specials = [bytes(3000), far + far[:64]]
    specials += [periodic(p, VALUE_LEN, 3 * p + k) for k in range(3) for p in PERIODS]
    out = []
    for i in range(80):
        key = struct.pack(">Q", 0x1000 + i)
        if i % 16 == 0:
            val = shared
        elif i % 3 == 1 and specials:
            val = specials.pop(0)
        else:
            val = ch.content(i % 8, VALUE_LEN, seed=i)
        out.append((key, 1700000000000000 + i, val))
    assert not specials
    return out


def tiny_rows():
    """3 rows that fit one 1 KiB chunk: periods 3 and 7, and random bytes
    followed by their own repeat."""
    r = ch.content(0, 60, seed=97)
    vals = [periodic(3, 200, 1), periodic(7, 260, 2), r + r + bytes(40) + r[:30]]
    return [(struct.pack(">Q", 0x2000 + i), 1700000000000000 + i, v)
            for i, v in enumerate(vals)]


def flush_rows(row_list, base):
    """`oracle_tool flush` of (key, ts, value) rows -> one LZ4 sstable."""
    os.makedirs(os.path.dirname(base), exist_ok=True)
    with open(base + ".rows.txt", "w") as f:
        for key, ts, val in row_list:
            f.write(f"{key.hex()} {ts} {val.hex()}\n")
    subprocess.run([ORACLE, "flush", base, base + ".rows.txt"], check=True,
                   capture_output=True)
    os.remove(base + ".rows.txt")
    return base


def read_payloads(base):
    """-> (codec name, chunk_len, data_len, [payload per chunk]); every chunk
    CRC is checked."""
    with open(base + "-CompressionInfo.db", "rb") as f:
        name, _o, chunk_len, _mc, data_len, offsets = ch.parse_compression_info(f.read())
    with open(base + "-Data.db", "rb") as f:
        data = f.read()
    out = []
    for i, off in enumerate(offsets):
        end = offsets[i + 1] if i + 1 < len(offsets) else len(data)
        p = data[off:end - 4]
        assert zlib.crc32(p) == struct.unpack(">I", data[end - 4:end])[0]
        out.append(p)
    return name, chunk_len, data_len, out


def split_chunks(raw, chunk_len):
    return [raw[o:o + chunk_len] for o in range(0, len(raw), chunk_len)]


def canonical(plain_base, dst_base, chunk_len, codec, scratch_dir):
    """The oracle-written sstable of plain_base's bytes at chunk_len: LZ4 via
    chunk_helpers.rechunk; Snappy by wrapping a literal-only Snappy image and
    having the oracle rewrite it (no libsnappy involved)."""
    if codec == "lz4":
        return ch.rechunk(plain_base, dst_base, chunk_len, scratch_dir)
    raw = ch.read_uncompressed(plain_base)
    tmp = os.path.join(scratch_dir, os.path.basename(plain_base))
    image, offs = ch.chunk_image(raw, chunk_len, snappy_literal)
    ch.write_chunked(plain_base, tmp, raw, chunk_len, image, offs, name=SNAPPY_NAME)
    os.makedirs(os.path.dirname(dst_base), exist_ok=True)
    subprocess.run([ORACLE, "rewrite", tmp, dst_base], check=True, capture_output=True)
    return dst_base


def write_variant(canon_base, dst_base, raw, chunk_len, payload_fn):
    """canon_base with its chunk payloads replaced by payload_fn's."""
    image, offs = ch.chunk_image(raw, chunk_len, payload_fn)
    ch.write_chunked(canon_base, dst_base, raw, chunk_len, image, offs)
    return dst_base


def run_ops(ops):
    """Plain reference decoder: literals appended, copies byte by byte (so an
    overlapped copy repeats the bytes it has just written)."""
    out = bytearray()
    for op in ops:
        if op[0] == "lit":
            out += op[1]
        else:
            _, off, n = op
            assert 0 < off <= len(out), (off, len(out))
            for _ in range(n):
                out.append(out[-off])
    return bytes(out)


# ---- LZ4 block wire format --------------------------------------------------
def lz4_walk(payload):
    """Yield (literal bytes, literal extension bytes, offset, match length,
    match extension bytes) per sequence of a 4-byte-length-prefixed LZ4 block;
    offset is None in the last sequence."""
    b, ip, end = payload, 4, len(payload)
    while ip < end:
        token = b[ip]; ip += 1
        lit, lext = token >> 4, b""
        if lit == 15:
            s0 = ip
            while b[ip] == 255:
                ip += 1
            ip += 1
            lext = b[s0:ip]
            lit += sum(lext)
        lits = b[ip:ip + lit]
        assert len(lits) == lit
        ip += lit
        if ip >= end:
            yield lits, lext, None, 0, b""
            return
        off = b[ip] | (b[ip + 1] << 8); ip += 2
        ml, mext = (token & 15) + 4, b""
        if ml == 19:
            s0 = ip
            while b[ip] == 255:
                ip += 1
            ip += 1
            mext = b[s0:ip]
            ml += sum(mext)
        yield lits, lext, off, ml, mext
    raise AssertionError("LZ4 block does not end in a literal-only sequence")


def lz4_parse(payload):
    ops = []
    for lits, _le, off, ml, _me in lz4_walk(payload):
        if lits:
            ops.append(("lit", bytes(lits)))
        if off is not None:
            ops.append(("copy", off, ml))
    return ops


def _lz4_ext(n):
    return b"\xff" * (n // 255) + bytes([n % 255])


def lz4_emit(ops, knobs=None):
    """ops -> payload. Adjacent literals merge (LZ4 cannot split a literal
    run); adjacent copies become zero-literal sequences. The ops must end in a
    literal: the format's last sequence has no match."""
    seqs, lit = [], b""
    for op in ops:
        if op[0] == "lit":
            lit += op[1]
        else:
            seqs.append((lit, op[1], op[2]))
            lit = b""
    assert lit, "an LZ4 block ends with literals"
    seqs.append((lit, None, 0))
    out = bytearray(struct.pack("<I", sum(len(s[0]) + s[2] for s in seqs)))
    for lits, off, ml in seqs:
        ll = len(lits)
        mcode = 0 if off is None else ml - 4
        assert off is None or (ml >= 4 and 0 < off < 65536)
        out.append((min(ll, 15) << 4) | min(mcode, 15))
        if ll >= 15:
            out += _lz4_ext(ll - 15)
        out += lits
        if off is not None:
            out += struct.pack("<H", off)
            if mcode >= 15:
                out += _lz4_ext(mcode - 15)
    return bytes(out)


# piece lengths of a split match: the shortest match, both sides of the
# disjoint/overlapped copy boundary (ml == off, ml == off+1), and both sides
# of the one- and two-byte length extensions
SPLIT_TARGETS = (4, "off", "off+1", 19, 20, 18, 273, 274, 275)
# literal run lengths a demoted match head lands on
LITERAL_TARGETS = (14, 15, 16, 269, 270, 271)
# liblz4 refuses a match that starts in the last 12 bytes of a block
LZ4_MFLIMIT = 12


def lz4_split_matches(ops, n):
    """Every match of length >= 8 cut into back-to-back pieces at the same
    offset (a periodic copy can be cut anywhere): zero-literal sequences."""
    out, pos, rot = [], 0, 0
    for op in ops:
        if op[0] == "lit":
            out.append(op)
            pos += len(op[1])
            continue
        _, off, ml = op
        p, rem, misses = pos, ml, 0
        while rem >= 8 and misses < len(SPLIT_TARGETS):
            t = SPLIT_TARGETS[rot % len(SPLIT_TARGETS)]
            rot += 1
            t = off if t == "off" else off + 1 if t == "off+1" else t
            if t >= 4 and rem - t >= 4 and p + t <= n - LZ4_MFLIMIT:
                out.append(("copy", off, t))
                p, rem, misses = p + t, rem - t, 0
            else:
                misses += 1
        out.append(("copy", off, rem))
        pos += ml
    return out


def lz4_demote_heads(ops, chunk):
    """The first bytes of a match written as literals instead, so that the
    literal run before it takes one of LITERAL_TARGETS."""
    n, out, pos, rot, run = len(chunk), [], 0, 0, 0
    for op in ops:
        if op[0] == "lit":
            out.append(op)
            pos += len(op[1])
            run += len(op[1])
            continue
        _, off, ml = op
        k = 0
        for j in range(len(LITERAL_TARGETS)):
            d = LITERAL_TARGETS[(rot + j) % len(LITERAL_TARGETS)] - run
            if 0 < d <= ml - 4 and pos + d <= n - LZ4_MFLIMIT:
                k, rot = d, rot + j + 1
                break
        if k:
            out.append(("lit", chunk[pos:pos + k]))
        out.append(("copy", off, ml - k))
        pos += ml
        run = 0
    return out


def _lz4_lib():
    lib = ch.lz4()
    if not getattr(lib, "_foreign", False):
        for fn in (lib.LZ4_compress_HC, lib.LZ4_compress_fast):
            fn.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                           ctypes.c_int]
            fn.restype = ctypes.c_int
        lib._foreign = True
    return lib


def _lz4_library(fn_name, arg):
    def payload(chunk):
        lib = _lz4_lib()
        cap = lib.LZ4_compressBound(len(chunk))
        buf = ctypes.create_string_buffer(cap)
        n = getattr(lib, fn_name)(bytes(chunk), buf, len(chunk), cap, arg)
        assert n > 0
        return struct.pack("<I", len(chunk)) + buf.raw[:n]
    return payload


def lz4_split(chunk):
    return lz4_emit(lz4_split_matches(lz4_parse(ch.lz4_payload(chunk)), len(chunk)))


def lz4_demote(chunk):
    return lz4_emit(lz4_demote_heads(lz4_parse(ch.lz4_payload(chunk)), chunk))


def lz4_literal(chunk):
    return lz4_emit([("lit", bytes(chunk))])


def lz4_decompress_safe(payload):
    """The system liblz4's verdict on a payload: the bytes, or None."""
    lib = ch.lz4()
    (ulen,) = struct.unpack_from("<I", payload, 0)
    buf = ctypes.create_string_buffer(max(ulen, 1))
    got = lib.LZ4_decompress_safe(payload[4:], buf, len(payload) - 4, ulen)
    return buf.raw[:ulen] if got == ulen else None


# ---- Snappy fragment wire format -------------------------------------------
def _varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def snappy_walk(payload):
    """-> (uncompressed length, elements). An element is ("lit", bytes, width)
    with width = number of extra length bytes (0..4), or ("copy", offset,
    length, kind) with kind = the tag's low two bits (1, 2 or 3)."""
    b, ip, ulen, sh = payload, 0, 0, 0
    while True:
        c = b[ip]; ip += 1
        ulen |= (c & 0x7F) << sh
        if not c & 0x80:
            break
        sh += 7
    els, end = [], len(b)
    while ip < end:
        tag = b[ip]; ip += 1
        kind = tag & 3
        if kind == 0:
            n, w = (tag >> 2) + 1, 0
            if n > 60:
                w = n - 60
                n = int.from_bytes(b[ip:ip + w], "little") + 1
                ip += w
            lits = b[ip:ip + n]
            assert len(lits) == n
            ip += n
            els.append(("lit", bytes(lits), w))
        elif kind == 1:
            els.append(("copy", ((tag >> 5) << 8) | b[ip], ((tag >> 2) & 7) + 4, 1))
            ip += 1
        else:
            w = 2 if kind == 2 else 4
            els.append(("copy", int.from_bytes(b[ip:ip + w], "little"), (tag >> 2) + 1, kind))
            ip += w
    assert ip == end
    return ulen, els


def snappy_parse(payload):
    return [e[:2] if e[0] == "lit" else e[:3] for e in snappy_walk(payload)[1]]


def _min_width(n):
    return 0 if n <= 60 else 1 if n <= 1 << 8 else 2 if n <= 1 << 16 else 3 if n <= 1 << 24 else 4


def _auto_kind(off, n):
    return 1 if 4 <= n <= 11 and off < 2048 else 2


def snappy_lower(ops):
    """ops -> wire elements in the minimal encoding: literal fields at their
    narrowest, copies cut into <= 64 bytes the way the reference encoder does
    and tagged copy-1 where that fits."""
    els = []
    for op in ops:
        if op[0] == "lit":
            els.append(("lit", op[1], 0))
            continue
        _, off, n = op
        while n >= 68:
            els.append(("copy", off, 64, 2))
            n -= 64
        if n > 64:
            els.append(("copy", off, 60, 2))
            n -= 60
        els.append(("copy", off, n, _auto_kind(off, n)))
    return els


def _el_cost(e):
    if e[0] == "lit":
        return 1 + max(e[2], _min_width(len(e[1]))) + len(e[1])
    return {1: 2, 2: 3, 3: 5}[e[3]]


def snappy_encode(els):
    body, total = bytearray(), 0
    for e in els:
        if e[0] == "lit":
            n = len(e[1])
            assert n > 0
            w = max(e[2], _min_width(n))
            if w == 0:
                body.append((n - 1) << 2)
            else:
                body.append((59 + w) << 2)
                body += (n - 1).to_bytes(w, "little")
            body += e[1]
        else:
            _, off, n, kind = e
            assert off > 0
            if kind == 1:
                assert 4 <= n <= 11 and off < 2048
                body.append(1 | ((n - 4) << 2) | ((off >> 8) << 5))
                body.append(off & 0xFF)
            else:
                assert 1 <= n <= 64 and off < (1 << 16 if kind == 2 else 1 << 32)
                body.append(kind | ((n - 1) << 2))
                body += off.to_bytes(2 if kind == 2 else 4, "little")
        total += n
    return _varint(total) + bytes(body)


def snappy_emit(ops, knobs=None):
    """ops -> payload. knobs: lit_width (extra length bytes of every literal,
    never below the minimal width) and copy_kind (2 or 3 for every copy)."""
    knobs = knobs or {}
    els = []
    for e in snappy_lower(ops):
        if e[0] == "lit":
            els.append(("lit", e[1], knobs.get("lit_width", 0)))
        else:
            els.append(e[:3] + (knobs.get("copy_kind", e[3]),))
    return snappy_encode(els)


def _within_bound(els, transform, n):
    """Apply transform (element -> list of elements) to each element while the
    fragment stays inside the decoder's frame bound for an n-byte chunk."""
    slack = snappy_bound(n) - len(_varint(n)) - sum(_el_cost(e) for e in els)
    assert slack >= 0
    out = []
    for e in els:
        alt = transform(e)
        delta = sum(_el_cost(a) for a in alt) - _el_cost(e)
        if delta <= slack:
            out += alt
            slack -= delta
        else:
            out.append(e)
    return out


def snappy_literal(chunk):
    return snappy_encode([("lit", bytes(chunk), 0)])


# piece lengths of a split copy: the three lengths only copy-2 and copy-4 can
# carry, then copy-1's shortest and longest
COPY_PIECES = (1, 2, 3, 4, 11)


class SnappyVariants:
    """Variants of the oracle's canonical fragments. canon maps a chunk's
    bytes to its canonical payload (read from the oracle-written sstable)."""

    def __init__(self, canon):
        self.canon = canon

    def _els(self, chunk):
        return snappy_lower(snappy_parse(self.canon[bytes(chunk)]))

    def widen(self, w):
        def payload(chunk):
            return snappy_encode(_within_bound(
                self._els(chunk),
                lambda e: [("lit", e[1], max(w, e[2]))] if e[0] == "lit" else [e], len(chunk)))
        return payload

    def split_literals(self, chunk):
        rng = random.Random(zlib.crc32(bytes(chunk)))

        def cut(e):
            if e[0] != "lit" or len(e[1]) < 2:
                return [e]
            b, out = e[1], []
            while b:
                k = rng.choice((1, 2, 3, 59, 60, 61, 255, 256, 257, len(b)))
                out.append(("lit", b[:k], 0))
                b = b[k:]
            return out
        return snappy_encode(_within_bound(self._els(chunk), cut, len(chunk)))

    def copy_kind(self, kind):
        def payload(chunk):
            return snappy_encode(_within_bound(
                self._els(chunk),
                lambda e: [e[:3] + (kind,)] if e[0] == "copy" else [e], len(chunk)))
        return payload

    def short_copies(self, chunk):
        rot = [0]

        def cut(e):
            if e[0] != "copy":
                return [e]
            _, off, rem, _k = e
            out = []
            while rem:
                t = min(COPY_PIECES[rot[0] % len(COPY_PIECES)], rem)
                rot[0] += 1
                out.append(("copy", off, t, _auto_kind(off, t)))
                rem -= t
            return out
        return snappy_encode(_within_bound(self._els(chunk), cut, len(chunk)))


def alternating(even_fn, odd_fn):
    """payload_fn for chunk_image: chunk 2k through even_fn, 2k+1 through
    odd_fn (the two chunks one decode wave takes). Fresh per image."""
    idx = [0]

    def payload(chunk):
        fn = odd_fn if idx[0] & 1 else even_fn
        idx[0] += 1
        return fn(chunk)
    return payload


def lz4_variants():
    """name -> factory of payload_fn. 'split' is the most heavily split."""
    v = {f"hc{lvl}": (lambda lvl=lvl: _lz4_library("LZ4_compress_HC", lvl)) for lvl in (3, 9, 12)}
    v.update({f"fast{a}": (lambda a=a: _lz4_library("LZ4_compress_fast", a))
              for a in (8, 65537)})
    v["split"] = lambda: lz4_split
    v["demote"] = lambda: lz4_demote
    v["literal"] = lambda: lz4_literal
    v["alternating"] = lambda: alternating(lz4_literal, lz4_split)
    return v


def snappy_variants(canon):
    """name -> factory of payload_fn. 'short' is the most heavily split;
    'lib' (libsnappy's own output) is present only where the library is."""
    sv = SnappyVariants(canon)
    v = {f"width{w}": (lambda w=w: sv.widen(w)) for w in (1, 2, 3, 4)}
    v["litsplit"] = lambda: sv.split_literals
    v["copy2"] = lambda: sv.copy_kind(2)
    v["copy4"] = lambda: sv.copy_kind(3)
    v["short"] = lambda: sv.short_copies
    v["literal"] = lambda: snappy_literal
    v["alternating"] = lambda: alternating(snappy_literal, sv.short_copies)
    lib = ch.snappy()
    if lib is not None:
        v["lib"] = lambda: (lambda chunk: ch.snappy_payload(chunk, lib))
    return v


LZ4_VARIANT_NAMES = ("hc3", "hc9", "hc12", "fast8", "fast65537", "split", "demote", "literal",
                     "alternating")
SNAPPY_VARIANT_NAMES = ("width1", "width2", "width3", "width4", "litsplit", "copy2", "copy4",
                        "short", "literal", "alternating", "lib")
HEAVIEST = {"lz4": "split", "snappy": "short"}


def variant_names(codec):
    return LZ4_VARIANT_NAMES if codec == "lz4" else SNAPPY_VARIANT_NAMES


def variants(codec, canon_base, raw, chunk_len):
    """name -> factory of payload_fn for the chunks of raw at chunk_len;
    canon_base is the canonical sstable of that codec and chunk length."""
    if codec == "lz4":
        return lz4_variants()
    _n, _cl, _dl, payloads = read_payloads(canon_base)
    chunks = split_chunks(raw, chunk_len)
    assert len(chunks) == len(payloads)
    return snappy_variants(dict(zip(chunks, payloads)))


def parse(payload, codec):
    return lz4_parse(payload) if codec == "lz4" else snappy_parse(payload)


# ---- census -----------------------------------------------------------------
LIT_EDGES = (14, 15, 16, 269, 270, 271)
MATCH_EDGES = (18, 19, 20, 273, 274, 275)


def census(payloads, codec):
    """What a set of streams contains (JSON-friendly). Small offsets are those
    up to 9; overlapped means length > offset."""
    if codec == "lz4":
        c = dict(sequences=0, small_offsets=set(), overlapped_offsets=set(),
                 len_eq_off=set(), len_eq_off_plus_1=set(), zero_literal_sequences=0,
                 lit_ext_ends_in_0=0, match_ext_ends_in_0=0, lit_ext_255x2=0,
                 match_ext_255x2=0, literal_edges=set(), match_edges=set(), max_offset=0)
        for p in payloads:
            first = True
            for lits, lext, off, ml, mext in lz4_walk(p):
                c["sequences"] += 1
                if len(lits) in LIT_EDGES:
                    c["literal_edges"].add(len(lits))
                c["lit_ext_ends_in_0"] += lext[-1:] == b"\0"
                c["lit_ext_255x2"] += lext.count(255) >= 2
                if off is None:
                    break
                # the first sequence of a block always has literals
                c["zero_literal_sequences"] += not lits and not first
                first = False
                c["match_ext_ends_in_0"] += mext[-1:] == b"\0"
                c["match_ext_255x2"] += mext.count(255) >= 2
                if ml in MATCH_EDGES:
                    c["match_edges"].add(ml)
                c["max_offset"] = max(c["max_offset"], off)
                if off <= 9:
                    c["small_offsets"].add(off)
                    if ml > off:
                        c["overlapped_offsets"].add(off)
                if off >= 2 and ml == off:
                    c["len_eq_off"].add(off)
                if off >= 2 and ml == off + 1:
                    c["len_eq_off_plus_1"].add(off)
    else:
        c = dict(elements=0, kinds=set(), literal_widths=set(), nonminimal_literals=0,
                 copy2_short_lengths=set(), copy4_short_lengths=set(), copy1_lengths=set(),
                 copy1_max_offset=0, small_offsets=set(), overlapped_offsets=set(),
                 max_offset=0)
        for p in payloads:
            for e in snappy_walk(p)[1]:
                c["elements"] += 1
                if e[0] == "lit":
                    c["kinds"].add(0)
                    c["literal_widths"].add(e[2])
                    c["nonminimal_literals"] += e[2] > _min_width(len(e[1]))
                    continue
                _, off, n, kind = e
                c["kinds"].add(kind)
                c["max_offset"] = max(c["max_offset"], off)
                if kind == 1:
                    c["copy1_lengths"].add(n)
                    c["copy1_max_offset"] = max(c["copy1_max_offset"], off)
                elif n <= 3:
                    c["copy2_short_lengths" if kind == 2 else "copy4_short_lengths"].add(n)
                if off <= 9:
                    c["small_offsets"].add(off)
                    if n > off:
                        c["overlapped_offsets"].add(off)
    return {k: sorted(v) if isinstance(v, set) else int(v) for k, v in c.items()}


def merge_census(a, b):
    """Union of two census dicts of one codec."""
    out = {}
    for k in a:
        if isinstance(a[k], list):
            out[k] = sorted(set(a[k]) | set(b[k]))
        elif k.startswith(("max_", "copy1_max")):
            out[k] = max(a[k], b[k])
        else:
            out[k] = a[k] + b[k]
    return out


# ---- the shared corpus ------------------------------------------------------
def _snappy_lib_uncompress(payload, lib):
    lib.snappy_uncompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                      ctypes.POINTER(ctypes.c_size_t)]
    lib.snappy_uncompress.restype = ctypes.c_int
    cap = snappy_walk(payload)[0]
    buf = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_size_t(cap)
    if lib.snappy_uncompress(payload, len(payload), buf, ctypes.byref(n)) != 0:
        return None
    return buf.raw[:n.value]


def snappy_lib_uncompress(payload):
    """libsnappy's verdict on a payload (the bytes, or None); the string
    "absent" where the library is not installed."""
    lib = ch.snappy()
    return "absent" if lib is None else _snappy_lib_uncompress(payload, lib)


def oracle_compact(out_base, *in_bases):
    os.makedirs(os.path.dirname(out_base), exist_ok=True)
    subprocess.run([ORACLE, "compact", out_base, *in_bases], check=True, capture_output=True)
    return out_base


class Corpus:
    """The chosen-bytes sstable ("main", 3 chunks at 64 KiB) and the
    single-chunk one ("tiny"), their canonical copies per codec and chunk
    length, the variant sstables and the oracle's compaction of each
    canonical copy; everything is built on first use under `root` and then
    left unchanged."""

    def __init__(self, root):
        self.root = str(root)
        self.plain = {"main": flush_rows(rows(), f"{self.root}/plain/main/oa-1-big"),
                      "tiny": flush_rows(tiny_rows(), f"{self.root}/plain/tiny/oa-1-big")}
        self.raw = {k: ch.read_uncompressed(b) for k, b in self.plain.items()}
        assert len(self.raw["tiny"]) <= min(CHUNK_LENGTHS)
        assert len(split_chunks(self.raw["main"], 65536)) == 3
        self._canon, self._compacted, self._variant = {}, {}, {}

    def chunks(self, chunk_len, which="main"):
        return split_chunks(self.raw[which], chunk_len)

    def canon(self, codec, chunk_len, which="main"):
        k = (codec, chunk_len, which)
        if k not in self._canon:
            d = f"{self.root}/canon/{which}-{codec}-{chunk_len}"
            self._canon[k] = canonical(self.plain[which], f"{d}/oa-1-big", chunk_len, codec,
                                       f"{d}/tmp")
        return self._canon[k]

    def canon_compacted(self, codec, chunk_len, which="main"):
        k = (codec, chunk_len, which)
        if k not in self._compacted:
            self._compacted[k] = oracle_compact(
                f"{self.root}/compacted/{which}-{codec}-{chunk_len}/oa-2-big",
                self.canon(codec, chunk_len, which))
        return self._compacted[k]

    def payload_fn(self, codec, chunk_len, name, which="main"):
        """A fresh payload_fn of the named variant; None where the variant
        needs a library that is absent."""
        fac = variants(codec, self.canon(codec, chunk_len, which), self.raw[which],
                       chunk_len).get(name)
        return fac() if fac else None

    def payloads(self, codec, chunk_len, name, which="main"):
        fn = self.payload_fn(codec, chunk_len, name, which)
        return None if fn is None else [fn(c) for c in self.chunks(chunk_len, which)]

    def variant(self, codec, chunk_len, name, which="main"):
        """The variant sstable's base path, or None (see payload_fn)."""
        k = (codec, chunk_len, name, which)
        if k not in self._variant:
            fn = self.payload_fn(codec, chunk_len, name, which)
            self._variant[k] = fn and write_variant(
                self.canon(codec, chunk_len, which),
                f"{self.root}/variant/{which}-{codec}-{chunk_len}-{name}/oa-1-big",
                self.raw[which], chunk_len, fn)
        return self._variant[k]
