"""Authored tables with set and typed-key map columns, and frozen columns.

The oracle knows one collection type, map<blob,blob>, and orders cell paths
as unsigned bytes. It is still the reference, through the devices of
desc_tables.py (rewrite_statistics, dumpsst, fromdump, gmd2_with_stats):

  engine inputs    every table is authored over MAP_BB columns (a frozen column
                   over a BYTES one) with its cells in the REAL type's path
                   order. `oracle_tool fromdump` sorts partitions only and
                   writes cells as given; then the HEADER of Statistics.db is
                   rewritten to the real type strings.
  expected bytes   byte-ordered keys (blob, text, ascii): the oracle's
                   compaction of the un-rewritten inputs, then the same
                   rewrite. A set<text> is a map<blob,blob> whose values are
                   empty.
                   signed keys (int, bigint, timestamp): the oracle compacts
                   the MIRROR, every path with its first byte XOR 0x80, which
                   keeps the length and turns signed order into unsigned
                   order. Its output is read back with `dumpsst`, the paths
                   mapped back, written with `fromdump` under the stats dumpsst
                   reported, and rewritten.
  digests          `oracle_tool validate` of the single expected sstable under
                   its base types: one input has no path merge and purge is
                   idempotent. The digest covers path bytes, so the mirror's
                   digests would not do.

Inputs of one job may list different columns (header_union_tables.project):
the engine compacts the narrow real tables, the oracle the wide mirrors.

at.to_gmd2 keeps authored values at 16 bytes. A longer value is authored as a
16-byte token (`long_value`) and widened in the memdump by `gmd2`.

Paths handed to oracle_tool must not contain '='.
Plain helper module: no fixtures, not a conftest.
"""
import os
import random
import shutil
import struct
import subprocess
from dataclasses import dataclass, replace
from typing import Optional

import authored_tables as at
import desc_tables as dt
import header_union_tables as hu
from authored_tables import (BYTES, DT, DT_LIVE, L, LONG, MAP_BB, T, Case, Cell, Live, Matrix,
                             Partition, Row, Schema)

M = dt.MARSHAL
BYTES_T, UTF8_T, ASCII_T = M + b"BytesType", M + b"UTF8Type", M + b"AsciiType"
INT32_T, LONG_T, TIMESTAMP_T = M + b"Int32Type", M + b"LongType", M + b"TimestampType"
MAP_BB_T = M + b"MapType(" + BYTES_T + b"," + BYTES_T + b")"
SIGNED_WIDTH = {INT32_T: 4, LONG_T: 8, TIMESTAMP_T: 8}
G = at.G                        # a local deletion time the purge bounds stand on
PURGE_NOW = 2000000000          # after every authored local deletion time


def set_of(k):
    return M + b"SetType(" + k + b")"


def map_of(k, v):
    return M + b"MapType(" + k + b"," + v + b")"


def frozen(inner):
    return M + b"FrozenType(" + inner + b")"


def i4(v):
    return struct.pack(">i", v)


def i8(v):
    return struct.pack(">q", v)


def edges(width):
    bits = 8 * width
    return [-2 ** (bits - 1), -1, 0, 1, 2 ** (bits - 1) - 1]


def key_type_of(t):
    """The K of SetType(K) / MapType(K,V); K is never nested here."""
    assert t.startswith(M + b"SetType(") or t.startswith(M + b"MapType("), t
    inner = t[t.index(b"(") + 1:-1]
    return inner.split(b",")[0]


def real_path_key(t):
    """Sort key of a cell path under the collection type string t: signed
    keys as the integer, every other key as its bytes (shorter first)."""
    w = SIGNED_WIDTH.get(key_type_of(t))
    if w is None:
        return lambda p: p

    def key(p):
        assert len(p) == w, f"path {p!r} is not {w} bytes"
        return int.from_bytes(p, "big", signed=True)
    return key


def mirror_path(p):
    """First byte XOR 0x80: its own inverse, keeps the length."""
    return bytes([p[0] ^ 0x80]) + p[1:]


# --------------------------------------------------------------------------
# long values
# --------------------------------------------------------------------------
_LONG = {}


def long_value(n, fill):
    """A 16-byte token that `gmd2` widens to n bytes of `fill`."""
    tok = b"\x01LONGVALU%02x%04x\x02" % (fill, n)
    assert len(tok) == 16
    _LONG[tok] = bytes([fill]) * n
    return tok


def gmd2(schema, parts, stats=None):
    g = dt.gmd2_with_stats(schema, parts, stats) if stats else at.to_gmd2(schema, parts)
    for tok, v in _LONG.items():
        g = g.replace(struct.pack("<I", 16) + tok, struct.pack("<I", len(v)) + v)
    return g


def narrow_values(parts):
    """Partitions read back from a dump, long values as their tokens again."""
    back = {v: k for k, v in _LONG.items()}
    fix = lambda c: replace(c, value=back.get(c.value, c.value))
    return map_cells(parts, None, fix)


def map_cells(parts, complex_fn, cell_fn=None):
    """The same partitions with complex_fn(col index, cell) over every complex
    cell (cell_fn over every simple and complex cell when given)."""
    cf = cell_fn or (lambda c: c)
    xf = (lambda i, c: cf(complex_fn(i, c))) if complex_fn else (lambda i, c: cf(c))

    def row(r):
        if r is None:
            return None
        return Row(r.ck, r.live, r.del_, {i: cf(c) for i, c in r.cells.items()},
                   {i: (d, [xf(i, c) for c in cs]) for i, (d, cs) in r.complex.items()})
    return [Partition(p.key, p.del_, row(p.static),
                      [row(it) if isinstance(it, Row) else it for it in p.items]) for p in parts]


# --------------------------------------------------------------------------
# a case
# --------------------------------------------------------------------------
@dataclass
class CollCase:
    matrix: Matrix                  # REAL paths in real order, over the oracle's (union) schema
    types: dict                     # column name -> real type string, the renamed columns
    headers: Optional[list] = None  # per input (regular names, static names); None == all

    @property
    def name(self):
        return self.matrix.name

    @property
    def schema(self):
        return self.matrix.schema

    def signed_cols(self):
        """Regular column indices whose paths compare signed."""
        return {i for i, (nm, _) in enumerate(self.schema.regular_cols)
                if nm in self.types and self.types[nm].startswith((M + b"SetType(", M + b"MapType("))
                and key_type_of(self.types[nm]) in SIGNED_WIDTH}

    def mirror(self, parts):
        s = self.signed_cols()
        return map_cells(parts, lambda i, c: replace(c, path=mirror_path(c.path)) if i in s else c)

    unmirror = mirror               # an involution

    def mirror_matrix(self):
        """The oracle's twin of the matrix, for the Python model's path order."""
        m = self.matrix
        mp = lambda p: None if p is None else self.mirror([p])[0]
        cases = [Case(c.label, [mp(p) for p in c.inputs], mp(c.tomb)) for c in m.cases]
        return Matrix(m.name, m.schema, m.n_inputs, cases, m.jobs, m.has_tomb_source)

    def inputs(self):
        ins, tomb = self.matrix.tables()
        return ins + ([tomb] if self.matrix.has_tomb_source else [])

    def header_of(self, i):
        if self.headers and self.headers[i] is not None:
            return self.headers[i]
        return ([nm for nm, _ in self.schema.regular_cols], [nm for nm, _ in self.schema.static_cols])

    def base_type(self, nm):
        t = dict(self.schema.regular_cols + self.schema.static_cols)[nm]
        return MAP_BB_T if t == MAP_BB else dt.TYPE_NAMES[t]

    def renames(self, names, to_real=True):
        """{name: (from, to)} for rewrite_statistics over a header with `names`."""
        out = {}
        for nm in names:
            if nm in self.types:
                a, b = self.base_type(nm), self.types[nm]
                out[nm] = (a, b) if to_real else (b, a)
        return out

    def all_names(self):
        return [nm for nm, _ in self.schema.regular_cols + self.schema.static_cols]

    def stem(self, gen):
        return f"da-{gen}-bti" if self.schema.bti else f"oa-{gen}-big"

    def write(self, oracle, d):
        """-> (real bases, mirror bases); a tombstone source is the last of each."""
        real, mirror = [], []
        for i, parts in enumerate(self.inputs()):
            hdr = self.header_of(i)
            ns, nparts = hu.project(self.schema, parts, *hdr)
            rb = f"{d}/real/{self.stem(i + 1)}"
            mb = f"{d}/mirror/{self.stem(i + 1)}"
            fromdump(oracle, gmd2(ns, nparts), rb)
            rewrite(rb, ns, self.renames(hdr[0] + hdr[1]))
            fromdump(oracle, gmd2(self.schema, self.mirror(parts)), mb)
            real.append(rb)
            mirror.append(mb)
        return real, mirror


def fromdump(oracle, g, base):
    assert "=" not in base
    os.makedirs(os.path.dirname(base), exist_ok=True)
    with open(base + ".memdump", "wb") as f:
        f.write(g)
    subprocess.run([oracle, "fromdump", base + ".memdump", base], check=True, capture_output=True)


def rewrite(base, schema, renames):
    """Rewrites the column types of <base>-Statistics.db in place."""
    ck = [dt.TYPE_NAMES[t] for t in schema.ck_types]
    p = base + "-Statistics.db"
    data = open(p, "rb").read()
    with open(p, "wb") as f:
        f.write(dt.rewrite_statistics(data, ck, ck, renames))


def copy_sstable(base, out_base):
    os.makedirs(os.path.dirname(out_base), exist_ok=True)
    stem = os.path.basename(base)
    for fn in os.listdir(os.path.dirname(base)):
        if fn.startswith(stem + "-"):
            shutil.copy(os.path.join(os.path.dirname(base), fn), out_base + fn[len(stem):])


def to_base(case, base, out_base):
    """A copy of the real sstable <base> (full header) under the oracle's types."""
    copy_sstable(base, out_base)
    rewrite(out_base, case.schema, case.renames(case.all_names(), to_real=False))


def read_dump(oracle, base, md):
    subprocess.run([oracle, "dumpsst", base, md], check=True, capture_output=True)
    with open(md, "rb") as f:
        return at.parse_gmd2(f.read())


def expected(oracle, case, mirror_out, want_base):
    """The oracle's output over the mirrors -> the expected real sstable."""
    os.makedirs(os.path.dirname(want_base), exist_ok=True)
    if not case.signed_cols():
        copy_sstable(mirror_out, want_base)
    else:
        schema, stats, parts = read_dump(oracle, mirror_out, want_base + ".mirror.memdump")
        assert schema.regular_cols == case.schema.regular_cols
        fromdump(oracle, gmd2(schema, narrow_values(case.unmirror(parts)), stats), want_base)
    rewrite(want_base, case.schema, case.renames(case.all_names()))


def paths_in_real_order(case, parts):
    """Every complex column's cells ascend strictly under its real type."""
    for p in parts:
        for it in p.items:
            if not isinstance(it, Row):
                continue
            for i, (_, cs) in it.complex.items():
                nm = case.schema.regular_cols[i][0]
                key = real_path_key(case.types.get(nm, MAP_BB_T))
                ks = [key(c.path) for c in cs]
                assert all(a < b for a, b in zip(ks, ks[1:])), (case.name, nm, ks)


# --------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------
def P(*items, **kw):
    return Partition(b"", items=list(items), **kw)


def K(v):
    return (at.ck_long(v),)


LIVE = lambda p, v=b"", ts=T: Cell(ts, v, path=p)
TOMB = lambda p, ts=T, ldt=L: Cell(ts, b"", ldt, path=p)
EXP = lambda p, v=b"", ts=T: Cell(ts, v, L, 60, path=p)


def set_text():
    """The same element in two inputs at one timestamp (live against
    tombstone, live against expiring), a complexDeletion at the timestamp of
    a cell, prefix pairs a / ab / b and the empty element."""
    s = Schema(regular_cols=((b"v", BYTES), (b"zs", MAP_BB)))
    X = 1
    row = lambda d, *cs, **kw: P(Row((), complex={X: (d, list(cs))}, **kw))
    cases = [
        Case("live | tombstone | expiring on one element", [
            row(DT_LIVE, LIVE(b"a"), LIVE(b"ab"), LIVE(b"b")),
            row(DT_LIVE, TOMB(b"a"), LIVE(b"b", ts=T + 1)),
            row(DT_LIVE, EXP(b"ab"), EXP(b"c"))]),
        Case("live | expiring, reversed input order", [
            row(DT_LIVE, EXP(b"a")), row(DT_LIVE, LIVE(b"a")), row(DT_LIVE, TOMB(b"a", ts=T - 1))]),
        Case("complexDeletion at the timestamp of a cell", [
            row(DT_LIVE, LIVE(b""), LIVE(b"k"), LIVE(b"l", ts=T + 1)),
            row(DT(T, L)),
            row(DT(T - 1, L), LIVE(b"k", ts=T - 1), LIVE(b"m", ts=T))]),
        Case("complexDeletion and cells in one input, simple column beside", [
            P(Row((), Live(T), cells={0: Cell(T, b"x")}, complex={X: (DT(T, G), [LIVE(b"q", ts=T + 1)])})),
            row(DT_LIVE, LIVE(b"p"), TOMB(b"q", ts=T + 1, ldt=G)), None]),
        Case("disjoint elements interleave", [
            row(DT_LIVE, LIVE(b"a"), LIVE(b"c"), LIVE(b"e")),
            row(DT_LIVE, LIVE(b"b"), LIVE(b"d")),
            row(DT_LIVE, LIVE(b"aa"), LIVE(b"\xc3\xa9"))]),
        Case("one input only", [None, None, row(DT_LIVE, LIVE(b"only"))]),
    ]
    return CollCase(Matrix("COLL_set_text", s, 3, cases), {b"zs": set_of(UTF8_T)})


def _edge_cases(pk, val, X, extra_cols=None):
    """MIN, -1, 0, 1, MAX spread so that every adjacent pair straddles two
    inputs; -1 in all three inputs with a timestamp tie. pk packs a key, val
    gives the value of a live cell (b"" in a set)."""
    e = [pk(v) for v in edges(len(pk(0)))]
    mn, m1, z, p1, mx = e
    row = lambda d, *cs: P(Row((), complex={X: (d, list(cs))}))
    cases = []
    for rot in range(3):
        ins = [row(DT_LIVE, LIVE(mn, val(0)), LIVE(m1, val(1)), LIVE(z, val(2)), LIVE(mx, val(3))),
               row(DT_LIVE, TOMB(m1), LIVE(p1, val(4))),
               row(DT_LIVE, EXP(m1, val(5)), LIVE(mx, val(6)))]
        cases.append(Case(f"edges, -1 tied in all three (rotation {rot})", ins[rot:] + ins[:rot]))
    cases += [
        Case("negative against positive, one element an input", [
            row(DT_LIVE, LIVE(p1, val(1))), row(DT_LIVE, LIVE(m1, val(2))), row(DT_LIVE, LIVE(mn, val(3)))]),
        Case("value tie-break on a negative key", [
            row(DT_LIVE, LIVE(m1, val(7))), row(DT_LIVE, LIVE(m1, val(8))), row(DT_LIVE, LIVE(z, val(0)))]),
        Case("complexDeletion at the timestamp of MIN's cell", [
            row(DT_LIVE, LIVE(mn, val(0)), LIVE(mx, val(0), ts=T + 1)),
            row(DT(T, G)),
            row(DT_LIVE, LIVE(m1, val(2), ts=T - 1), LIVE(z, val(2), ts=T + 2))]),
        Case("purgeable tombstones at the edges", [
            row(DT_LIVE, TOMB(mn, ldt=G), TOMB(mx, ldt=G + 1)),
            row(DT(T - 5, G), LIVE(m1, val(1), ts=T - 5), LIVE(p1, val(1))),
            row(DT_LIVE, EXP(mn, val(4), ts=T - 1), LIVE(z, val(3)))]),
        Case("every edge in every input, newest wins", [
            row(DT_LIVE, *[LIVE(k, val(1), ts=T + (i % 3)) for i, k in enumerate(e)]),
            row(DT_LIVE, *[LIVE(k, val(2), ts=T + ((i + 1) % 3)) for i, k in enumerate(e)]),
            row(DT_LIVE, *[LIVE(k, val(3), ts=T + ((i + 2) % 3)) for i, k in enumerate(e)])]),
        Case("one input only", [None, row(DT_LIVE, LIVE(m1, val(0)), LIVE(z, val(1))), None]),
    ]
    # more partitions, so that shards, routed outputs and kept ranges all hold some
    rnd = random.Random(4711)
    for n in range(12):
        ins = []
        for i in range(3):
            ks = sorted(rnd.sample(range(5), rnd.randint(1, 4)))
            mk = lambda k: rnd.choice([LIVE(e[k], val(rnd.randint(0, 8)), ts=T + rnd.randint(-1, 1)),
                                       TOMB(e[k], ts=T + rnd.randint(-1, 1), ldt=rnd.choice([G, L])),
                                       EXP(e[k], val(rnd.randint(0, 8)), ts=T + rnd.randint(-1, 1))])
            d = DT(T + rnd.randint(-2, 0), rnd.choice([G, L])) if rnd.random() < 0.3 else DT_LIVE
            ins.append(row(d, *[mk(k) for k in ks]) if rnd.random() < 0.8 else None)
        if all(x is None for x in ins):
            ins[0] = row(DT_LIVE, LIVE(z, val(0)))
        cases.append(Case(f"random edges {n}", ins))
    return cases


PURGE_JOBS = [("default", at.Job()),
              ("purge everything", at.Job(now=PURGE_NOW, gc_before=PURGE_NOW)),
              ("gc_before=G", at.Job(gc_before=G)), ("gc_before=G+1", at.Job(gc_before=G + 1)),
              ("gc_before=G+1 overlap min_ts=T", at.Job(gc_before=G + 1, overlap_min_ts=T))]


def set_int_edges(**schema_kw):
    """The smallest shape where an unsigned path compare emits out-of-order
    and duplicate cells."""
    s = Schema(regular_cols=((b"zs", MAP_BB),), **schema_kw)
    name = "COLL_set_int_edges" + ("_da" if schema_kw.get("bti") else "") + \
        ("_snappy" if schema_kw.get("snappy") else "")
    return CollCase(Matrix(name, s, 3, _edge_cases(i4, lambda n: b"", 0), jobs=PURGE_JOBS),
                    {b"zs": set_of(INT32_T)})


def _map_values():
    vs = [b"", b"a", b"b", long_value(300, 0x61), long_value(300, 0x62), b"ab", b"\x80", b"\x7f",
          b"0123456789abcdef"]
    return lambda n: vs[n]


def map_bigint_text():
    s = Schema(regular_cols=((b"zm", MAP_BB),))
    return CollCase(Matrix("COLL_map_bigint_text", s, 3, _edge_cases(i8, _map_values(), 0)),
                    {b"zm": map_of(LONG_T, UTF8_T)})


def map_timestamp_blob():
    s = Schema(regular_cols=((b"zm", MAP_BB),))
    return CollCase(Matrix("COLL_map_timestamp_blob", s, 3, _edge_cases(i8, _map_values(), 0)),
                    {b"zm": map_of(TIMESTAMP_T, BYTES_T)})


def map_bigint_wide():
    """40 partitions of five 300-byte values at the edge keys in two inputs:
    about 60 KB, so the output spans several 16 KiB chunks and a size cap
    cuts it."""
    s = Schema(regular_cols=((b"zm", MAP_BB),))
    e = [i8(v) for v in edges(8)]
    va, vb = long_value(300, 0x61), long_value(300, 0x62)
    row = lambda *cs: P(Row((), complex={0: (DT_LIVE, list(cs))}))
    cases = [Case(f"wide {n}", [row(*[LIVE(k, va if (n + i) % 2 else vb) for i, k in enumerate(e)]),
                                row(*[LIVE(k, vb if (n + i) % 3 else va, ts=T + (i + n) % 2)
                                      for i, k in enumerate(e) if (i + n) % 4])])
             for n in range(40)]
    return CollCase(Matrix("COLL_map_bigint_wide", s, 2, cases), {b"zm": map_of(LONG_T, UTF8_T)})


MIXED_SCHEMA = Schema(ck_types=(LONG,), static_cols=((b"s", BYTES),),
                      regular_cols=((b"a", BYTES), (b"f", BYTES), (b"zs", MAP_BB), (b"zt", MAP_BB),
                                    (b"zu", MAP_BB)))
MIXED_TYPES = {b"f": frozen(M + b"ListType(" + INT32_T + b")"), b"zs": set_of(INT32_T),
               b"zt": map_of(UTF8_T, UTF8_T)}
A, F, ZS, ZT, ZU = range(5)


def _mixed_row(rnd, ck, cols):
    r = Row(K(ck))
    if rnd.random() < 0.4:
        r.live = Live(T + rnd.randint(-1, 1))
    if rnd.random() < 0.15:
        r.del_ = DT(T + rnd.randint(-1, 1), rnd.choice([G, L]))
    ts = lambda: T + rnd.randint(-1, 1)

    def cell(v, path=None):
        k = rnd.random()
        if k < 0.15:
            return Cell(ts(), b"", rnd.choice([G, L]), path=path)
        if k < 0.3:
            return Cell(ts(), v, L, 60, path=path)
        return Cell(ts(), v, path=path)
    pools = {ZS: [i4(v) for v in edges(4)] + [i4(-7), i4(7)],
             ZT: [b"", b"a", b"ab", b"b", b"k"], ZU: [b"\x00", b"\x7f", b"\x80", b"\xff\x01", b"\xff"]}
    keys = {ZS: real_path_key(MIXED_TYPES[b"zs"]), ZT: None, ZU: None}
    for c in cols:
        if rnd.random() < 0.4:
            continue
        if c in (A, F):
            r.cells[c] = cell(rnd.choice([b"", b"p", b"q", b"\x00\x00\x00\x01"]))
            continue
        d = DT(T + rnd.randint(-2, 0), rnd.choice([G, L])) if rnd.random() < 0.3 else DT_LIVE
        paths = sorted(rnd.sample(pools[c], rnd.randint(0, 4)), key=keys[c])
        if d.live and not paths:
            continue
        r.complex[c] = (d, [cell(b"" if c == ZS else rnd.choice([b"", b"x", b"yz"]), p) for p in paths])
    if r.is_empty():
        r.live = Live(T)
    return r


def _mixed_matrix(name, schema, n_inputs, n_keys, cols_of, seed):
    rnd = random.Random(seed)
    cases = []
    for k in range(n_keys):
        ins = []
        for i in range(n_inputs):
            if rnd.random() < 0.55 and not (i == n_inputs - 1 and not any(ins)):
                ins.append(None)
                continue
            p = Partition(b"")
            if rnd.random() < 0.1:
                p.del_ = DT(T + rnd.randint(-1, 0), rnd.choice([G, L]))
            if schema.static_cols and rnd.random() < 0.4:
                p.static = Row((), cells={0: Cell(T + rnd.randint(-1, 1), rnd.choice([b"s", b"t"]))})
            p.items = [_mixed_row(rnd, ck, cols_of(i))
                       for ck in sorted(rnd.sample(range(5), rnd.randint(1, 3)))]
            if rnd.random() < 0.3:      # a range tombstone over rows with collections
                lo, hi = sorted(rnd.sample(range(5), 2))
                p.items += at._range(K(lo), rnd.random() < 0.5, K(hi), True,
                                     DT(T + rnd.randint(-1, 1), rnd.choice([G, L])))
            ins.append(p)
        cases.append(Case(f"key {k}", ins))
    return Matrix(name, schema, n_inputs, cases, jobs=PURGE_JOBS)


def mixed():
    """simple a, a frozen list, set<int>, map<text,text> and map<blob,blob>
    under a clustering column, a static column and range tombstones: 8 inputs."""
    return CollCase(_mixed_matrix("COLL_mixed", MIXED_SCHEMA, 8, 24, lambda i: (A, F, ZS, ZT, ZU), 31),
                    MIXED_TYPES)


UNION_SCHEMA = Schema(ck_types=(LONG,), regular_cols=((b"a", BYTES), (b"f", BYTES), (b"zs", MAP_BB)))
UNION_TYPES = {b"f": frozen(map_of(UTF8_T, INT32_T)), b"zs": set_of(INT32_T)}
UNION_HEADERS = [([b"a", b"f"], []), ([b"a", b"zs"], []), ([b"a", b"f", b"zs"], [])]


def union():
    """Input 0 lacks the set column, input 1 the frozen one. The frozen type
    string holds "MapType(": it must still sort among the simple columns."""
    cols = [(A, F), (A, ZS), (A, F, ZS)]
    return CollCase(_mixed_matrix("COLL_union", UNION_SCHEMA, 3, 16, lambda i: cols[i], 57),
                    UNION_TYPES, UNION_HEADERS)


def gc():
    """Two data inputs and a tombstone source that holds a cell tombstone at
    a negative key and a complexDeletion."""
    s = Schema(ck_types=(LONG,), regular_cols=((b"a", BYTES), (b"zs", MAP_BB)))
    X = 1
    mn, m1, z, p1, mx = [i4(v) for v in edges(4)]
    row = lambda ck, d, *cs, **kw: Row(K(ck), complex={X: (d, list(cs))}, **kw)
    cases = [
        Case("source tombstone at -1, newer and older", [
            P(row(1, DT_LIVE, LIVE(mn), LIVE(m1), LIVE(z), LIVE(mx)),
              row(2, DT_LIVE, LIVE(m1, ts=T + 5), LIVE(p1))),
            P(row(1, DT_LIVE, LIVE(m1, ts=T - 1), LIVE(p1)))],
            P(row(1, DT_LIVE, TOMB(m1, ts=T + 1)), row(2, DT_LIVE, TOMB(m1, ts=T + 1)))),
        Case("source complexDeletion", [
            P(row(1, DT_LIVE, LIVE(mn), LIVE(m1, ts=T + 3), LIVE(mx), cells={0: Cell(T, b"a")})),
            P(row(1, DT(T - 2, L), LIVE(z, ts=T + 2)))],
            P(row(1, DT(T + 1, L)))),
        Case("source tombstones at MIN and MAX around the data", [
            P(row(1, DT_LIVE, LIVE(m1), LIVE(z), LIVE(p1))), None],
            P(row(1, DT_LIVE, TOMB(mn, ts=T + 1), TOMB(z, ts=T), TOMB(mx, ts=T + 1)))),
        Case("source cell at a negative key ties with the data", [
            P(row(1, DT_LIVE, EXP(mn), LIVE(m1))), P(row(1, DT_LIVE, TOMB(m1)))],
            P(row(1, DT_LIVE, TOMB(mn), TOMB(m1)))),
        Case("no source partition", [P(row(1, DT_LIVE, LIVE(m1), LIVE(z))), P(row(1, DT_LIVE, LIVE(mn)))]),
    ]
    return CollCase(Matrix("COLL_gc", s, 2, cases, has_tomb_source=True), {b"zs": set_of(INT32_T)})


ALL_CASES = {"set_text": set_text, "set_int_edges": set_int_edges, "map_bigint_text": map_bigint_text,
             "map_timestamp_blob": map_timestamp_blob, "map_bigint_wide": map_bigint_wide,
             "mixed": mixed, "union": union, "gc": gc}
# the Python model (authored_tables) has no garbage collection over complex columns
PREDICTED = ("set_text", "set_int_edges", "map_bigint_text", "map_timestamp_blob", "map_bigint_wide",
             "mixed", "union")
