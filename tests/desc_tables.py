"""Authored tables with descending clustering columns (ReversedType).

The oracle knows no ReversedType. It is still the reference, through an
equivalence: map every descending clustering component to an order-reversed
value (the MIRROR) and a table written in its own descending order becomes a
legal ascending table of the oracle's.

  fixed width      m(v) = ~v            reverses signed order, MIN <-> MAX
  variable width   m(s) = ~s + b"\\xff"  for s without a 0x00 byte; reverses
                                        prefix pairs too: a < ab, m(ab) < m(a).
                                        The mirror's type is BytesType.

Ascending components are left alone. Cases are authored IN MIRROR SPACE, as
authored_tables.Matrix over the mirror schema, so Matrix's own checks (items
sorted, ranges open and close in turn) hold for the mirror; the descending
table is the un-mirrored one, its items in the same sequence.

  engine inputs    the descending table under its BASE types (items in
                   descending order; `oracle_tool fromdump` sorts partitions
                   only and writes unfiltereds as given), then Statistics.db
                   rewritten so that HEADER and STATS carry the ReversedType /
                   TimestampType strings.
  expected bytes   the oracle's compaction of the mirrors, read back with
                   `dumpsst`, clusterings mapped back, written with `fromdump`
                   under the header stats dumpsst reported, same rewrite.

Paths handed to oracle_tool must not contain '=' (it reads key=value).

Plain helper module: no fixtures, not a conftest.
"""
import os
import random
import struct
import subprocess
import zlib
from dataclasses import dataclass, replace

import authored_tables as at
from authored_tables import (BYTES, DT, INT32, L, LONG, T, UTF8, Case, Cell, Live, Marker, Matrix,
                             Partition, Row, Schema)

MARSHAL = b"org.apache.cassandra.db.marshal."
TYPE_NAMES = {at.BYTES: MARSHAL + b"BytesType", at.UTF8: MARSHAL + b"UTF8Type",
              at.ASCII: MARSHAL + b"AsciiType", at.LONG: MARSHAL + b"LongType",
              at.INT32: MARSHAL + b"Int32Type"}
TIMESTAMP = MARSHAL + b"TimestampType"
FIXED = {at.LONG: 8, at.INT32: 4}


def reversed_type(inner):
    return MARSHAL + b"ReversedType(" + inner + b")"


# --------------------------------------------------------------------------
# schema and mirror
# --------------------------------------------------------------------------
@dataclass
class DescSchema:
    base: Schema                    # the descending table under its base types
    desc: tuple                     # per clustering column: descending?
    timestamp_ck: tuple = ()        # clustering columns (LONG) whose type is TimestampType
    timestamp_cols: tuple = ()      # regular/static column names (LONG) that are TimestampType

    def __post_init__(self):
        assert len(self.desc) == len(self.base.ck_types)

    @property
    def mirror(self):
        """The oracle's twin schema: a descending variable-width column is BytesType."""
        cks = tuple(BYTES if d and t not in FIXED else t
                    for t, d in zip(self.base.ck_types, self.desc))
        return replace(self.base, ck_types=cks)

    def ck_strings(self):
        """The clustering type strings of the real table."""
        out = []
        for i, (t, d) in enumerate(zip(self.base.ck_types, self.desc)):
            inner = TIMESTAMP if i in self.timestamp_ck else TYPE_NAMES[t]
            out.append(reversed_type(inner) if d else inner)
        return out

    def base_ck_strings(self):
        return [TYPE_NAMES[t] for t in self.base.ck_types]

    def col_strings(self, to_real=True):
        """{column name: (from type, to type)} of the columns the rewrite renames."""
        a, b = TYPE_NAMES[LONG], TIMESTAMP
        return {nm: (a, b) if to_real else (b, a) for nm in self.timestamp_cols}


def _mirror_value(t, v):
    assert v is not None
    inv = bytes(b ^ 0xFF for b in v)
    if t in FIXED:
        assert len(v) == FIXED[t]
        return inv
    assert 0 not in v, "the variable-width mirror needs values without a 0x00 byte"
    return inv + b"\xff"


def _unmirror_value(t, v):
    if t in FIXED:
        return bytes(b ^ 0xFF for b in v)
    assert v[-1:] == b"\xff", v
    return bytes(b ^ 0xFF for b in v[:-1])


def mirror_ck(ds, ck):
    return tuple(_mirror_value(t, v) if d else v
                 for v, t, d in zip(ck, ds.base.ck_types, ds.desc))


def unmirror_ck(ds, ck):
    return tuple(_unmirror_value(t, v) if d else v
                 for v, t, d in zip(ck, ds.base.ck_types, ds.desc))


def map_clusterings(parts, fn):
    """The same partitions, every clustering prefix mapped through fn."""
    out = []
    for p in parts:
        items = [replace(it, ck=fn(it.ck)) for it in p.items]
        out.append(Partition(p.key, p.del_, p.static, items))
    return out


def mirror_parts(ds, parts):
    return map_clusterings(parts, lambda ck: mirror_ck(ds, ck))


def unmirror_parts(ds, parts):
    return map_clusterings(parts, lambda ck: unmirror_ck(ds, ck))


def desc_compare_prefix(ds, ka, a, kb, b):
    """The ClusteringComparator of the real table: every descending component's
    comparison negated, sizes and kinds untouched."""
    for i in range(min(len(a), len(b))):
        c = at._cmp_component(ds.base.ck_types[i], a[i], b[i])
        if ds.base.ck_types[i] == INT32:
            c = at._cmp(struct.unpack(">i", a[i])[0], struct.unpack(">i", b[i])[0])
        if c:
            return -c if ds.desc[i] else c
    if len(a) == len(b):
        return at._cmp(at._KIND_COMPARISON[ka], at._KIND_COMPARISON[kb])
    return at._KIND_VS_CLUSTERING[ka] if len(a) < len(b) else -at._KIND_VS_CLUSTERING[kb]


def mirror_compare_prefix(ds, ka, a, kb, b):
    """at.compare_prefix over the mirror schema (INT32 as a signed int)."""
    ts = ds.mirror.ck_types
    for i in range(min(len(a), len(b))):
        if ts[i] == INT32:
            c = at._cmp(struct.unpack(">i", a[i])[0], struct.unpack(">i", b[i])[0])
            if c:
                return c
            continue
        c = at._cmp_component(ts[i], a[i], b[i])
        if c:
            return c
    return at.compare_prefix(ts, ka, (), kb, ()) if len(a) == len(b) else \
        (at._KIND_VS_CLUSTERING[ka] if len(a) < len(b) else -at._KIND_VS_CLUSTERING[kb])


# --------------------------------------------------------------------------
# Statistics.db rewrite
# --------------------------------------------------------------------------
def _uvint_get(b, pos):
    first = b[pos]
    extra = 0
    while extra < 8 and first & (0x80 >> extra):
        extra += 1
    v = first & (0xFF >> extra) if extra < 8 else 0
    for i in range(extra):
        v = (v << 8) | b[pos + 1 + i]
    return v, pos + 1 + extra


def _uvint_put(v):
    if v < 0x80:
        return bytes([v])
    size = 2
    while size < 9 and v >= 1 << (7 * size):
        size += 1
    extra = size - 1
    body = v.to_bytes(size, "big") if size < 9 else b"\0" + v.to_bytes(8, "big")
    return bytes([body[0] | ((0xFF << (8 - extra)) & 0xFF)]) + body[1:]


def _crc_be32(crc, v):
    return zlib.crc32(struct.pack(">I", v), crc)


def split_statistics(data):
    """Statistics.db -> [(component type, body)], every checksum verified."""
    count, crc0 = struct.unpack_from(">II", data, 0)
    crc = _crc_be32(0, count)
    assert crc == crc0, "Statistics.db: count checksum"
    toc = []
    for i in range(count):
        t, off = struct.unpack_from(">II", data, 8 + 8 * i)
        crc = _crc_be32(_crc_be32(crc, t), off)
        toc.append((t, off))
    assert struct.unpack_from(">I", data, 8 + 8 * count)[0] == crc, "Statistics.db: TOC checksum"
    assert toc[0][1] == 8 + 8 * count + 4 and [o for _, o in toc] == sorted(o for _, o in toc)
    comps = []
    for i, (t, off) in enumerate(toc):
        end = toc[i + 1][1] if i + 1 < count else len(data)
        body = data[off:end - 4]
        assert struct.unpack_from(">I", data, end - 4)[0] == zlib.crc32(body), \
            f"Statistics.db: component {t} checksum"
        comps.append((t, body))
    return comps


def join_statistics(comps):
    """[(type, body)] -> Statistics.db with offsets and checksums recomputed."""
    count = len(comps)
    o = bytearray(struct.pack(">I", count))
    crc = _crc_be32(0, count)
    o += struct.pack(">I", crc)
    pos = 8 + 8 * count + 4
    for t, body in comps:
        o += struct.pack(">II", t, pos)
        crc = _crc_be32(_crc_be32(crc, t), pos)
        pos += len(body) + 4
    o += struct.pack(">I", crc)
    for _, body in comps:
        o += body + struct.pack(">I", zlib.crc32(body))
    return bytes(o)


def _type_list(b, pos):
    """uvint count + count x (uvint length + bytes) at pos -> (strings, end)."""
    n, pos = _uvint_get(b, pos)
    out = []
    for _ in range(n):
        ln, pos = _uvint_get(b, pos)
        out.append(bytes(b[pos:pos + ln]))
        pos += ln
    return out, pos


def _put_type_list(types):
    return _uvint_put(len(types)) + b"".join(_uvint_put(len(t)) + t for t in types)


def _stats_types_at(body):
    """Offset of the clustering type list in the STATS component."""
    pos = 0
    for _ in range(2):                              # two estimated histograms
        pos += 4 + 16 * struct.unpack_from(">I", body, pos)[0]
    pos += 12 + 32 + 8                              # commit log bound, min/max, ratio
    pos += 4                                        # tombstone histogram: max bin size
    pos += 4 + 12 * struct.unpack_from(">I", body, pos)[0]
    return pos + 4 + 8                              # level, repairedAt


def statistics_types(data):
    """-> (HEADER clustering types, STATS clustering types, {column: type})."""
    comps = dict(split_statistics(data))
    stats_ck, _ = _type_list(comps[2], _stats_types_at(comps[2]))
    h = comps[3]
    pos = 0
    for _ in range(3):
        _, pos = _uvint_get(h, pos)
    ln, pos = _uvint_get(h, pos)
    pos += ln
    hdr_ck, pos = _type_list(h, pos)
    cols = {}
    for _ in range(2):
        n, pos = _uvint_get(h, pos)
        for _ in range(n):
            ln, pos = _uvint_get(h, pos)
            nm = bytes(h[pos:pos + ln])
            pos += ln
            ln, pos = _uvint_get(h, pos)
            cols[nm] = bytes(h[pos:pos + ln])
            pos += ln
    assert pos == len(h)
    return hdr_ck, stats_ck, cols


def rewrite_statistics(data, old_ck, new_ck, col_types=None):
    """Replaces the clustering type strings (HEADER and STATS) and the types of
    the named columns; offsets and checksums recomputed. The strings found
    must be old_ck / the column's `from` type."""
    col_types = col_types or {}
    out = []
    for t, body in split_statistics(data):
        if t == 2:
            at_ = _stats_types_at(body)
            found, end = _type_list(body, at_)
            assert found == list(old_ck), (found, old_ck)
            body = body[:at_] + _put_type_list(new_ck) + body[end:]
        elif t == 3:
            pos = 0
            for _ in range(3):
                _, pos = _uvint_get(body, pos)
            ln, pos = _uvint_get(body, pos)
            pos += ln
            found, end = _type_list(body, pos)
            assert found == list(old_ck), (found, old_ck)
            nb = bytearray(body[:pos] + _put_type_list(new_ck))
            pos = end
            seen = set()
            for _ in range(2):
                n, pos = _uvint_get(body, pos)
                nb += _uvint_put(n)
                for _ in range(n):
                    ln, pos = _uvint_get(body, pos)
                    nm = bytes(body[pos:pos + ln])
                    pos += ln
                    ln, pos = _uvint_get(body, pos)
                    ty = bytes(body[pos:pos + ln])
                    pos += ln
                    if nm in col_types:
                        assert ty == col_types[nm][0], (nm, ty)
                        ty = col_types[nm][1]
                        seen.add(nm)
                    nb += _uvint_put(len(nm)) + nm + _uvint_put(len(ty)) + ty
            assert pos == len(body) and seen == set(col_types)
            body = bytes(nb)
        out.append((t, body))
    return join_statistics(out)


def to_real(ds, base):
    """Rewrites <base>-Statistics.db from the base types to the real ones."""
    p = base + "-Statistics.db"
    data = open(p, "rb").read()
    with open(p, "wb") as f:
        f.write(rewrite_statistics(data, ds.base_ck_strings(), ds.ck_strings(), ds.col_strings()))


def to_base(ds, base, out_base):
    """A copy of the sstable <base> as <out_base> under the base types."""
    import shutil
    stem = os.path.basename(base)
    for fn in os.listdir(os.path.dirname(base)):
        if fn.startswith(stem + "-"):
            shutil.copy(os.path.join(os.path.dirname(base), fn), out_base + fn[len(stem):])
    p = out_base + "-Statistics.db"
    data = open(p, "rb").read()
    with open(p, "wb") as f:
        f.write(rewrite_statistics(data, ds.ck_strings(), ds.base_ck_strings(),
                                   ds.col_strings(to_real=False)))


# --------------------------------------------------------------------------
# writing inputs and expected outputs
# --------------------------------------------------------------------------
def _fromdump(oracle, gmd2, md, base):
    assert "=" not in md and "=" not in base
    os.makedirs(os.path.dirname(base), exist_ok=True)
    with open(md, "wb") as f:
        f.write(gmd2)
    subprocess.run([oracle, "fromdump", md, base], check=True, capture_output=True)


def gmd2_with_stats(schema, parts, stats):
    """at.to_gmd2 with the given (min ts, min ldt, min ttl) header stats in
    place of recomputed ones."""
    g = bytearray(at.to_gmd2(schema, parts))
    at_ = len(at.to_gmd2(schema, [])) - 8 - 20
    assert bytes(g[at_ + 20:at_ + 28]) == struct.pack("<Q", len(parts))
    g[at_:at_ + 20] = struct.pack("<qqi", *stats)
    return bytes(g)


def write_real(oracle, ds, parts, base, gmd2=None):
    """The descending table `parts` (real clusterings, descending order) as
    the sstable <base>."""
    _fromdump(oracle, gmd2 or at.to_gmd2(ds.base, parts), base + ".memdump", base)
    to_real(ds, base)


def expected_from_mirror(oracle, ds, mirror_out, want_base):
    """The oracle's output over the mirrors -> the expected real sstable."""
    md = want_base + ".mirror.memdump"
    os.makedirs(os.path.dirname(want_base), exist_ok=True)
    subprocess.run([oracle, "dumpsst", mirror_out, md], check=True, capture_output=True)
    with open(md, "rb") as f:
        schema, stats, parts = at.parse_gmd2(f.read())
    assert schema.ck_types == ds.mirror.ck_types
    real = replace(schema, ck_types=ds.base.ck_types)
    write_real(oracle, ds, None, want_base,
               gmd2_with_stats(real, unmirror_parts(ds, parts), stats))


@dataclass
class DescCase:
    ds: DescSchema
    matrix: Matrix                  # in MIRROR space, over ds.mirror

    @property
    def name(self):
        return self.matrix.name

    def mirror_inputs(self):
        ins, tomb = self.matrix.tables()
        return ins + ([tomb] if self.matrix.has_tomb_source else [])

    def real_inputs(self):
        return [unmirror_parts(self.ds, p) for p in self.mirror_inputs()]

    def write(self, oracle, d, real_stem="oa-%d-big"):
        """-> (real bases, mirror bases); a tombstone source is the last of each."""
        real, mirror = [], []
        for i, mp in enumerate(self.mirror_inputs()):
            mb = f"{d}/mirror/oa-{i + 1}-big"
            _fromdump(oracle, at.to_gmd2(self.ds.mirror, mp), mb + ".memdump", mb)
            rb = f"{d}/real/" + real_stem % (i + 1)
            write_real(oracle, self.ds, unmirror_parts(self.ds, mp), rb)
            real.append(rb)
            mirror.append(mb)
        return real, mirror


def all_prefixes(parts_lists):
    """Every distinct (kind, clustering prefix) of the given tables."""
    seen = {}
    for parts in parts_lists:
        for p in parts:
            for it in p.items:
                seen[(at._item_kind(it), it.ck)] = None
    return list(seen)


# --------------------------------------------------------------------------
# the cases. m8/m4 mirror a long/int: the REAL value is the argument.
# --------------------------------------------------------------------------
def m8(v):
    return struct.pack(">q", ~v)


def m4(v):
    return struct.pack(">i", ~v)


def mv(s):
    return _mirror_value(BYTES, s)


def _with_schema(mk, name, schema):
    """A matrix of authored_tables with its name and schema replaced (the
    items are re-sorted and re-checked under the new schema)."""
    m = mk()
    return Matrix(name, schema, m.n_inputs, m.cases, m.jobs, m.has_tomb_source)


def bigint_desc():
    """matrix_c_bigint's shape: its clusterings 10/20/30 ARE the mirrors, the
    real rows are ~10 > ~20 > ~30."""
    ds = DescSchema(at.ROWLEVEL, (True,))
    return DescCase(ds, _with_schema(at.matrix_c_bigint, "DESC_bigint", ds.mirror))


def composite(desc, snappy=0):
    s = Schema(ck_types=(LONG, LONG), regular_cols=((b"v", BYTES),), snappy=snappy)
    ds = DescSchema(s, desc)
    name = "DESC_composite_" + "".join("d" if d else "a" for d in desc) + ("_snappy" * snappy)
    return DescCase(ds, _with_schema(at.matrix_c_composite, name, ds.mirror))


def text_desc():
    """matrix_c_text's shape over the prefix pairs a / ab / b: in mirror space
    m(b) < m(ab) < m(a), so b stands where the ascending matrix has a. Then
    the long values: four rows and the same four as range bounds, sharing
    their first 8 bytes."""
    ds = DescSchema(Schema(ck_types=(UTF8,), regular_cols=((b"v", BYTES),)), (True,))
    k = lambda v: (mv(v),)
    lo, mid, hi = k(b"b"), k(b"ab"), k(b"a")
    assert lo < mid < hi
    ranges = [("[b,ab]", lo, True, mid, True), ("(b,ab)", lo, False, mid, False),
              ("[b,ab)", lo, True, mid, False), ("(b,ab]", lo, False, mid, True),
              ("[ab,a]", mid, True, hi, True), ("(ab,a]", mid, False, hi, True),
              ("[-inf,ab]", at.NEG_INF, True, mid, True), ("[ab,+inf]", mid, True, at.POS_INF, True)]
    m = at._marker_matrix("DESC_text", ds.mirror, [lo, mid, hi], ranges, mid)
    # real descending order: 12345678b, 12345678ab, 12345678a, 12345678
    longs = [k(b"12345678b"), k(b"12345678ab"), k(b"12345678a"), k(b"12345678")]
    assert longs == sorted(longs)
    d1, d2 = DT(T, L), DT(T + 1, L)
    rows = lambda tag, ts: [Row(c, Live(ts), cells={0: Cell(ts, tag)}) for c in longs]
    cases = list(m.cases)
    for i in range(3):
        cases.append(Case(f"long values, range [{i},{i + 1}] over rows", [
            Partition(b"", items=rows(b"r1", T)),
            Partition(b"", items=at._range(longs[i], True, longs[i + 1], True, d2)),
            Partition(b"", items=rows(b"r3", T)[i:i + 2])]))
    cases.append(Case("long values, exclusive bounds and a boundary", [
        Partition(b"", items=rows(b"r1", T + 2)),
        Partition(b"", items=[Marker(at.EXCL_START, longs[0], d1),
                              Marker(at.EXCL_END_INCL_START, longs[1], d1, d2),
                              Marker(at.INCL_END_EXCL_START, longs[2], d2, d1),
                              Marker(at.EXCL_END, longs[3], d1)]),
        Partition(b"", items=at._range(longs[0], True, longs[3], True, d2))]))
    return DescCase(ds, Matrix("DESC_text", ds.mirror, 3, cases))


class PresortedMatrix(Matrix):
    """A Matrix whose items stay as authored. authored_tables orders INT32
    clusterings as unsigned bytes, which is wrong at the sign edges; the
    author sorts with mirror_compare_prefix instead."""

    def __post_init__(self):
        for n, c in enumerate(self.cases):
            c.inputs = list(c.inputs) + [None] * (self.n_inputs - len(c.inputs))
            for p in c.inputs + [c.tomb]:
                if p is not None:
                    p.key = at.case_key(n)


def sign_edges(t):
    """MIN, -1, 0, 1, MAX of int / bigint: each a row in two inputs with a
    timestamp tie, one range spanning MIN..MAX."""
    import functools
    bits, mk = (32, m4) if t == INT32 else (64, m8)
    vals = [-2 ** (bits - 1), -1, 0, 1, 2 ** (bits - 1) - 1]
    ds = DescSchema(Schema(ck_types=(t,), regular_cols=((b"v", BYTES),)), (True,))
    k = lambda v: (mk(v),)
    row = lambda v, tag: Row(k(v), Live(T), cells={0: Cell(T, tag)})
    # descending: the range starts at MAX and ends at MIN
    span = lambda d: at._range(k(vals[-1]), True, k(vals[0]), True, d)
    rows = lambda tag: [row(v, tag) for v in vals]
    order = lambda items: sorted(items, key=functools.cmp_to_key(
        lambda a, b: mirror_compare_prefix(ds, at._item_kind(a), a.ck, at._item_kind(b), b.ck)))
    part = lambda items: Partition(b"", items=order(items))
    cases = [
        Case("tie on every edge value", [part(rows(b"l")), part(rows(b"r"))]),
        Case("range MAX..MIN under the rows", [part(rows(b"l")), part(span(DT(T - 1, L)))]),
        Case("range MAX..MIN over the rows", [part(rows(b"l") + span(DT(T, L))),
                                              part(rows(b"r")[1:4])]),
    ]
    for c in cases:
        for p in c.inputs:
            # MAX first ... MIN last, a range's start before MAX's row
            real = [struct.unpack(">i" if t == INT32 else ">q", _unmirror_value(t, it.ck[0]))[0]
                    for it in p.items if isinstance(it, Row)]
            assert real == sorted(real, reverse=True)
            assert not isinstance(p.items[0], Marker) or p.items[0].kind == at.INCL_START
    return DescCase(ds, PresortedMatrix("DESC_edges_" + ("int" if t == INT32 else "bigint"),
                                        ds.mirror, 2, cases))


def blocks_desc():
    ds = DescSchema(Schema(ck_types=(LONG,)), (True,))
    return DescCase(ds, _with_schema(at.matrix_c_blocks, "DESC_blocks", ds.mirror))


def timestamp_desc():
    """timestamp DESC clustering, a timestamp regular and a timestamp static
    column: TimestampType in the header, LONG for the oracle."""
    s = Schema(ck_types=(LONG,), static_cols=((b"st", LONG),),
               regular_cols=((b"v", BYTES), (b"w", LONG)))
    ds = DescSchema(s, (True,), timestamp_ck=(0,), timestamp_cols=(b"st", b"w"))
    k = lambda v: (m8(v),)
    ms = 1_700_000_000_000
    lng = lambda v: struct.pack(">q", v)
    P = lambda *items, **kw: Partition(b"", items=list(items), **kw)
    cases = [
        Case("newest first, ties", [
            P(Row(k(ms + 2), Live(T), cells={0: Cell(T, b"a"), 1: Cell(T, lng(ms))}),
              Row(k(ms + 1), cells={1: Cell(T, lng(-1))}), Row(k(ms), Live(T)),
              static=Row((), cells={0: Cell(T, lng(ms))})),
            P(Row(k(ms + 2), cells={1: Cell(T, lng(ms + 1))}),
              Row(k(ms - 1), cells={0: Cell(T, b"z")}),
              static=Row((), cells={0: Cell(T, lng(ms + 5))}))]),
        Case("range over a time window", [
            P(*[Row(k(ms + i), Live(T), cells={1: Cell(T, lng(i))}) for i in range(5, -1, -1)]),
            P(*at._range(k(ms + 4), True, k(ms + 1), False, DT(T + 1, L)))]),
        Case("static only", [None, P(static=Row((), cells={0: Cell(T + 1, b"", L)}))]),
    ]
    return DescCase(ds, Matrix("DESC_timestamp", ds.mirror, 2, cases))


MANY_SIZES = (300, 70, 130)


def many_desc():
    """300/70/130 partitions, 1-4 rows each, random ties: a source boundary
    inside a 256-thread block of the parse kernels."""
    rnd = random.Random(90210)
    keys = [list(range(300)),
            sorted(rnd.sample(range(300), 35) + rnd.sample(range(300, 400), 35)),
            sorted(rnd.sample(range(300), 65) + rnd.sample(range(300, 400), 65))]
    ds = DescSchema(Schema(ck_types=(LONG,), regular_cols=((b"a", BYTES), (b"b", LONG))), (True,))
    parts = [dict(), dict(), dict()]
    for i in range(3):
        for key in keys[i]:
            p = Partition(b"")
            if rnd.random() < 0.1:
                p.del_ = DT(T + rnd.randint(-1, 0), L)
            for ck in sorted(rnd.sample(range(-3, 3), rnd.randint(1, 4)), reverse=True):
                r = Row((m8(ck),))
                if rnd.random() < 0.4:
                    r.live = Live(T + rnd.randint(-1, 1))
                if rnd.random() < 0.15:
                    r.del_ = DT(T + rnd.randint(-1, 1), L)
                if rnd.random() < 0.6:
                    r.cells[0] = Cell(T + rnd.randint(-1, 1), rnd.choice([b"", b"p", b"q", b"pq"]))
                if rnd.random() < 0.5:
                    r.cells[1] = Cell(T + rnd.randint(-1, 1), struct.pack(">q", rnd.randint(-2, 2)))
                if r.is_empty():
                    r.live = Live(T)
                p.items.append(r)
            if rnd.random() < 0.2:
                lo, hi = sorted(rnd.sample(range(-3, 3), 2))
                p.items += at._range((m8(hi),), True, (m8(lo),), rnd.random() < 0.5,
                                     DT(T + rnd.randint(-1, 1), L))
            parts[i][key] = p
    cases = [Case(f"key {k}", [parts[i].get(k) for i in range(3)]) for k in range(400)]
    return DescCase(ds, Matrix("DESC_many", ds.mirror, 3, cases))


def purge_desc():
    """matrix_d's cases and jobs (row and range tombstones at the purge
    bounds) under a descending bigint."""
    ds = DescSchema(at.ROWLEVEL, (True,))
    return DescCase(ds, _with_schema(at.matrix_d, "DESC_purge", ds.mirror))


def gc_desc():
    """header_union_tables.gc_case's shape (bigint clustering, a tombstone
    source), every input under the full header."""
    import header_union_tables as hu
    m = hu.gc_case().matrix
    ds = DescSchema(m.schema, (True,))
    return DescCase(ds, Matrix("DESC_gc", ds.mirror, m.n_inputs, m.cases, m.jobs, True))


ALL_CASES = {
    "bigint": bigint_desc,
    "composite_ad": lambda: composite((False, True)),
    "composite_da": lambda: composite((True, False)),
    "text": text_desc,
    "edges_int": lambda: sign_edges(INT32),
    "edges_bigint": lambda: sign_edges(LONG),
    "blocks": blocks_desc,
    "timestamp": timestamp_desc,
    "many": many_desc,
    "purge": purge_desc,
    "gc": gc_desc,
}
