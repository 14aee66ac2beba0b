"""Authored inputs whose serialization headers list different columns.

The oracle merges cells by column index, so it cannot compact such inputs
itself. It is still the reference, through an equivalence: an sstable written
with a narrow header is logically the same table as one written with the full
(union) header in which the missing columns never occur. Every input here is
therefore written twice through `oracle_tool fromdump`: the NARROW twin under
its own header, which the engine compacts, and the WIDE twin under the union
header, which the oracle compacts. The expected bytes are always the oracle's
compaction of the wide twins.

Each case is an authored_tables.Matrix over the UNION schema (one partition
per case number, so a failure names its cases) plus one header per input.
Every complex column is named zm..., after every simple column, so that the
oracle's name-only sort and Columns order (simple, then complex) agree.

Plain helper module: no fixtures, not a conftest.
"""
import os
import random
import struct
import subprocess
from dataclasses import dataclass, replace
from typing import Optional

import authored_tables as at
from authored_tables import (BYTES, COUNTER, DT, DT_LIVE, INT32, L, LONG, MAP_BB, T, Case, Cell,
                             Live, Marker, Matrix, Partition, Row, Schema, ck_long)

PURGE_NOW = 2000000000          # gcbefore == now of the purging runs


def K(v):
    return (ck_long(v),)


def lng(v):
    return struct.pack(">q", v)


def i32(v):
    return struct.pack(">i", v)


# --------------------------------------------------------------------------
# projection and the twins
# --------------------------------------------------------------------------
def _rows(parts):
    for p in parts:
        for it in p.items:
            if isinstance(it, Row):
                yield it


def used_columns(schema, parts):
    """(regular names, static names) that occur in the partitions, header order."""
    reg, st = set(), set()
    for r in _rows(parts):
        reg.update(r.cells)
        reg.update(r.complex)
    for p in parts:
        if p.static is not None:
            st.update(p.static.cells)
    return ([nm for i, (nm, _) in enumerate(schema.regular_cols) if i in reg],
            [nm for i, (nm, _) in enumerate(schema.static_cols) if i in st])


def project(schema, parts, keep_regular, keep_static):
    """The same partitions under a header with only the kept columns (given
    by name): cell and complex indices renumbered. A cell of a column that is
    not kept is a mistake of the caller."""
    keep_regular, keep_static = set(keep_regular), set(keep_static)
    rmap, smap = {}, {}
    for i, (nm, _) in enumerate(schema.regular_cols):
        if nm in keep_regular:
            rmap[i] = len(rmap)
    for i, (nm, _) in enumerate(schema.static_cols):
        if nm in keep_static:
            smap[i] = len(smap)
    assert len(rmap) == len(keep_regular) and len(smap) == len(keep_static), "unknown column kept"
    narrow = replace(schema,
                     regular_cols=tuple(c for c in schema.regular_cols if c[0] in keep_regular),
                     static_cols=tuple(c for c in schema.static_cols if c[0] in keep_static))

    def row(r, m):
        return Row(r.ck, r.live, r.del_, {m[i]: c for i, c in r.cells.items()},
                   {m[i]: (d, list(cs)) for i, (d, cs) in r.complex.items()})

    out = []
    for p in parts:
        st = None
        if p.static is not None and not p.static.is_empty():
            assert smap or not p.static.cells, "static cells under a header without statics"
            st = row(p.static, smap)
            if not smap:
                # a header without static columns has no static slot at all
                assert st.is_empty(), "a static row needs a static column"
                st = None
        out.append(Partition(p.key, p.del_, st,
                             [row(it, rmap) if isinstance(it, Row) else it for it in p.items]))
    return narrow, out


def _fromdump(oracle, schema, parts, md, base):
    with open(md, "wb") as f:
        f.write(at.to_gmd2(schema, parts))
    subprocess.run([oracle, "fromdump", md, base], check=True, capture_output=True)


def write_twins(oracle, d, schema, inputs, headers=None, first_gen=1):
    """Per input i (its partitions under the union schema): the wide sstable
    <d>/wide/oa-<gen>-big (union header) and the narrow one
    <d>/narrow/oa-<gen>-big (headers[i] == (regular names, static names), or
    the columns that occur in input i). -> (narrow bases, wide bases, narrow
    schemas)."""
    os.makedirs(f"{d}/narrow", exist_ok=True)
    os.makedirs(f"{d}/wide", exist_ok=True)
    stem = "da-%d-bti" if schema.bti else "oa-%d-big"
    narrow, wide, schemas = [], [], []
    for i, parts in enumerate(inputs):
        hdr = headers[i] if headers and headers[i] is not None else used_columns(schema, parts)
        ns, nparts = project(schema, parts, *hdr)
        name = stem % (first_gen + i)
        _fromdump(oracle, schema, parts, f"{d}/wide/in{i}.memdump", f"{d}/wide/{name}")
        _fromdump(oracle, ns, nparts, f"{d}/narrow/in{i}.memdump", f"{d}/narrow/{name}")
        narrow.append(f"{d}/narrow/{name}")
        wide.append(f"{d}/wide/{name}")
        schemas.append(ns)
    return narrow, wide, schemas


@dataclass
class UnionCase:
    matrix: Matrix                  # over the union schema
    headers: Optional[list] = None  # per input (regular names, static names); None == derived
    # every union column is missing from one input header and present in another
    all_columns_partial: bool = False
    # an explicit header may hold a column its input happens not to use
    may_hold_unused: bool = False

    @property
    def name(self):
        return self.matrix.name

    def inputs(self):
        ins, tomb = self.matrix.tables()
        return ins + ([tomb] if self.matrix.has_tomb_source else [])

    def header_of(self, i):
        if self.headers and self.headers[i] is not None:
            return self.headers[i]
        return used_columns(self.matrix.schema, self.inputs()[i])

    def write(self, oracle, d):
        """-> (narrow bases, wide bases, narrow schemas); a tombstone source
        is the last entry of each."""
        return write_twins(oracle, d, self.matrix.schema, self.inputs(),
                           [self.header_of(i) for i in range(len(self.inputs()))])


def P(*items, **kw):
    return Partition(b"", items=list(items), **kw)


# --------------------------------------------------------------------------
# U1: disjoint headers
# --------------------------------------------------------------------------
U1_SCHEMA = Schema(ck_types=(LONG,), static_cols=((b"s1", BYTES), (b"s2", LONG)),
                   regular_cols=((b"a", BYTES), (b"b", LONG), (b"c", BYTES), (b"zm", MAP_BB)))
A, B, C, ZM = 0, 1, 2, 3
S1, S2 = 0, 1


def u1(**schema_kw):
    """Inputs 1-3 are {a,c}; {b,zm}+{s2}; an empty regular header. A union
    column exists only if some input's header has it, so a fourth input
    {a,zm}+{s1} brings s1 (and ties with inputs 1 and 2 on a and zm)."""
    cases = [
        Case("common to all", [
            P(Row(K(10), Live(T), cells={A: Cell(T, b"a1"), C: Cell(T, b"c1")}),
              Row(K(20), cells={A: Cell(T + 1, b"a2")})),
            P(Row(K(10), cells={B: Cell(T, lng(1))},
                  complex={ZM: (DT_LIVE, [Cell(T, b"m", path=b"k")])}),
              Row(K(20), cells={B: Cell(T, lng(2))}),
              Row(K(30), complex={ZM: (DT(T - 1, L), [Cell(T, b"n", path=b"k2")])}),
              static=Row((), cells={S2: Cell(T, lng(7))})),
            P(Row(K(10), Live(T + 2)), Row(K(20), del_=DT(T, L)), Row(K(30), Live(T))),
            P(Row(K(10), cells={A: Cell(T, b"a0")},
                  complex={ZM: (DT_LIVE, [Cell(T, b"p", path=b"k"), Cell(T, b"q", path=b"k3")])}),
              static=Row((), cells={S1: Cell(T, b"s")}))]),
        Case("partition deletion from the empty header over {a,c}", [
            P(Row(K(10), cells={C: Cell(T, b"x")}), Row(K(11), cells={A: Cell(T + 9, b"y")})),
            None,
            Partition(b"", del_=DT(T + 5, L)),
            None]),
        Case("only {b,zm}+{s2}", [
            None,
            P(Row(K(1), Live(T), cells={B: Cell(T, lng(-1))}),
              static=Row((), cells={S2: Cell(T, lng(9))})),
            None, None]),
        Case("only the empty header", [None, None, P(Row(K(1), Live(T)), Row(K(2), del_=DT(T, L))),
                                       None]),
        Case("only {a,zm}+{s1}", [
            None, None, None,
            P(Row(K(1), complex={ZM: (DT(T, L), [])}), static=Row((), cells={S1: Cell(T, b"")}))]),
        Case("every regular column on one row", [
            P(Row(K(10), cells={A: Cell(T, b"a"), C: Cell(T, b"c")})),
            P(Row(K(10), cells={B: Cell(T, lng(5))},
                  complex={ZM: (DT_LIVE, [Cell(T, b"v", path=b"k")])})),
            None, None]),
        Case("row deletion from the empty header under newer cells", [
            P(Row(K(10), cells={A: Cell(T + 1, b"new"), C: Cell(T - 1, b"old")})),
            P(Row(K(10), cells={B: Cell(T, lng(3))})),
            P(Row(K(10), del_=DT(T, L))),
            P(Row(K(10), complex={ZM: (DT_LIVE, [Cell(T - 1, b"o", path=b"k"),
                                                  Cell(T + 1, b"n", path=b"l")])}))]),
    ]
    return UnionCase(Matrix("U1_disjoint", replace(U1_SCHEMA, **schema_kw), 4, cases),
                     all_columns_partial=True)


# --------------------------------------------------------------------------
# U2: a column added between two generations
# --------------------------------------------------------------------------
def u2(swapped=False):
    s = Schema(ck_types=(LONG,), regular_cols=((b"a", BYTES), (b"b", LONG)))
    pairs = [
        ("tie on a, b only in the wider", P(Row(K(1), Live(T), cells={0: Cell(T, b"x")})),
         P(Row(K(1), Live(T), cells={0: Cell(T, b"y"), 1: Cell(T, lng(4))}))),
        ("narrow newer on a", P(Row(K(1), cells={0: Cell(T + 1, b"n")})),
         P(Row(K(1), cells={0: Cell(T, b"o"), 1: Cell(T, lng(4))}))),
        ("narrow row deletion over b", P(Row(K(1), del_=DT(T, L)), Row(K(2), cells={0: Cell(T, b"k")})),
         P(Row(K(1), cells={1: Cell(T, lng(4))}), Row(K(2), cells={1: Cell(T, b"", L)}))),
        ("only the narrow", P(Row(K(1), cells={0: Cell(T, b"a")})), None),
        ("only the wider", None, P(Row(K(1), cells={1: Cell(T, lng(0))}),
                                   Row(K(2), cells={0: Cell(T, b"a")}))),
    ]
    cases = [Case(label, [w, n] if swapped else [n, w]) for label, n, w in pairs]
    return UnionCase(Matrix("U2_added_swapped" if swapped else "U2_added", s, 2, cases))


# --------------------------------------------------------------------------
# U3: static sets {}, {s1}, {s2}, {s1,s2}
# --------------------------------------------------------------------------
def u3():
    s = Schema(ck_types=(LONG,), static_cols=((b"s1", BYTES), (b"s2", LONG)),
               regular_cols=((b"v", BYTES),))
    row = lambda n: Row(K(n), cells={0: Cell(T, b"r%d" % n)})
    cases = [
        Case("all four, ties on s1", [
            P(row(1)),
            P(row(2), static=Row((), cells={0: Cell(T, b"x")})),
            P(row(3), static=Row((), cells={1: Cell(T, lng(1))})),
            P(row(1), static=Row((), cells={0: Cell(T, b"y"), 1: Cell(T + 1, lng(2))}))]),
        Case("no static row under headers that have statics", [P(row(1)), P(row(1)), P(row(2)),
                                                               P(row(3))]),
        Case("static row deleted in one input, set in another", [
            None,
            P(static=Row((), cells={0: Cell(T, b"set")})),
            P(static=Row((), cells={1: Cell(T, lng(5))})),
            P(static=Row((), cells={0: Cell(T + 1, b"", L), 1: Cell(T + 1, b"", L)}))]),
        Case("partition deletion without statics over a static row", [
            Partition(b"", del_=DT(T, L)),
            P(static=Row((), cells={0: Cell(T, b"gone")})),
            P(static=Row((), cells={1: Cell(T + 1, lng(6))})),
            None]),
        Case("a static row under the widest header alone", [
            P(row(1)), None, None, P(row(2), static=Row((), cells={1: Cell(T, lng(1))}))]),
    ]
    return UnionCase(Matrix("U3_statics", s, 4, cases))


# --------------------------------------------------------------------------
# U4: complex columns
# --------------------------------------------------------------------------
U4_SCHEMA = Schema(ck_types=(LONG,),
                   regular_cols=((b"a", BYTES), (b"zm1", MAP_BB), (b"zm2", MAP_BB)))


def u4():
    """{a,zm1}, {zm1,zm2} (no simple column), {a,zm2}."""
    c = lambda ts, v, p: Cell(ts, v, path=p)
    cases = [
        Case("deletions next to live columns, path ties", [
            P(Row(K(10), cells={0: Cell(T, b"a1")},
                  complex={1: (DT(T - 1, L), [c(T, b"x", b"k1"), c(T, b"y", b"k2")])})),
            # zm1 live next to a deleted zm2 (row flag 0x40); zm2 ends with a
            # deletion and no cells
            P(Row(K(10), complex={1: (DT_LIVE, [c(T, b"z", b"k1")]), 2: (DT(T, L), [])})),
            P(Row(K(10), cells={0: Cell(T + 1, b"a3")},
                  complex={2: (DT_LIVE, [c(T - 1, b"dead", b"q"), c(T + 1, b"live", b"q2")])}))]),
        Case("only the header without a simple column", [
            None,
            P(Row(K(1), complex={2: (DT_LIVE, [c(T, b"v", b"p")])}),
              Row(K(2), complex={1: (DT(T, L), []), 2: (DT(T, L + 1), [c(T + 1, b"w", b"p")])})),
            None]),
        Case("tie on a between the outer headers", [
            P(Row(K(1), cells={0: Cell(T, b"l")})), None, P(Row(K(1), cells={0: Cell(T, b"r")}))]),
        Case("zm2 path ties, zm1 from one side", [
            P(Row(K(1), Live(T), complex={1: (DT_LIVE, [c(T, b"1", b"a"), c(T, b"2", b"b")])})),
            P(Row(K(1), complex={2: (DT_LIVE, [c(T, b"m", b"p"), c(T, b"n", b"pq")])})),
            P(Row(K(1), complex={2: (DT_LIVE, [c(T, b"n", b"p"), c(T, b"m", b"pq"),
                                                c(T, b"", b"r", )])}))]),
        Case("complex deletion across headers", [
            P(Row(K(1), complex={1: (DT_LIVE, [c(T, b"old", b"k")])})),
            P(Row(K(1), complex={1: (DT(T, L), [])})),
            P(Row(K(1), cells={0: Cell(T, b"a")}))]),
    ]
    return UnionCase(Matrix("U4_complex", U4_SCHEMA, 3, cases), all_columns_partial=True)


# --------------------------------------------------------------------------
# U5: markers in a narrow-header input
# --------------------------------------------------------------------------
def u5():
    s = Schema(ck_types=(LONG,), regular_cols=((b"a", BYTES), (b"b", BYTES)))
    d1, d2 = DT(T, L), DT(T + 1, L)
    ranges = lambda: [Marker(at.INCL_START, K(10), d1),
                      Marker(at.INCL_END_EXCL_START, K(20), d1, d2),
                      Marker(at.INCL_END, K(30), d2)]
    brow = lambda n, ts: Row(K(n), cells={1: Cell(ts, b"b%d" % n)})
    cases = [
        Case("ranges of {a} over cells of {b}", [
            P(Row(K(5), cells={0: Cell(T, b"a5")}), *ranges()),
            P(brow(10, T), brow(15, T + 1), brow(20, T), brow(25, T + 1), brow(30, T + 2),
              brow(35, T)),
            P(Row(K(15), cells={0: Cell(T + 5, b"a"), 1: Cell(T + 5, b"b")}),
              Row(K(40), Live(T), cells={0: Cell(T, b"a"), 1: Cell(T, b"b")}))]),
        Case("open-ended range of {b} over {a}", [
            P(Row(K(1), Live(T), cells={0: Cell(T, b"x")}), Row(K(50), cells={0: Cell(T + 3, b"y")})),
            P(Marker(at.INCL_START, (), d2), Row(K(7), cells={1: Cell(T + 2, b"k")}),
              Marker(at.INCL_END, K(60), d2)),
            None]),
        Case("every union column on one row from two headers", [
            P(Row(K(1), cells={0: Cell(T, b"a")})), P(Row(K(1), cells={1: Cell(T, b"b")})), None]),
    ]
    return UnionCase(Matrix("U5_markers", s, 3, cases))


# --------------------------------------------------------------------------
# U6: fixed widths through the map
# --------------------------------------------------------------------------
def u6():
    """b is source column 0 under {b} and column 1 under {a,b,i}."""
    s = Schema(ck_types=(LONG,), regular_cols=((b"a", BYTES), (b"b", LONG), (b"i", INT32)))
    cases = [
        Case("tie on b", [P(Row(K(1), cells={1: Cell(T, lng(10))})),
                          P(Row(K(1), cells={0: Cell(T, b"abc"), 1: Cell(T, lng(11)),
                                             2: Cell(T, i32(-3))}))]),
        Case("narrow b newer", [P(Row(K(1), cells={1: Cell(T + 1, lng(2 ** 62))}),
                                  Row(K(2), cells={1: Cell(T, b"", L)})),
                                P(Row(K(1), cells={1: Cell(T, lng(0)), 2: Cell(T, i32(7))}),
                                  Row(K(2), cells={0: Cell(T, b""), 1: Cell(T, lng(1))}))]),
        Case("only {b}", [P(Row(K(1), Live(T), cells={1: Cell(T, lng(-1))})), None]),
        Case("only {a,b,i}", [None, P(Row(K(1), cells={2: Cell(T, i32(1))}),
                                      Row(K(2), cells={0: Cell(T, b"z"), 2: Cell(T, i32(2))}))]),
    ]
    return UnionCase(Matrix("U6_fixed", s, 2, cases))


# --------------------------------------------------------------------------
# U7: counters
# --------------------------------------------------------------------------
def u7():
    """{c1} against {c1,c2}: the tombstone/context pairs of matrix_a_counter
    on c1, a context on c2."""
    s = Schema(regular_cols=((b"c1", COUNTER), (b"c2", COUNTER)))
    cases = []
    for (ln, lc), (rn, rc) in ((a, b) for a in at.COUNTER_KINDS for b in at.COUNTER_KINDS):
        if lc.ldt == at.LDT_NONE and rc.ldt == at.LDT_NONE:
            continue
        cases.append(Case(f"counter {ln} | {rn}", [
            P(Row((), cells={0: lc})),
            P(Row((), cells={0: rc, 1: Cell(T, at.COUNTER_CTX)}))]))
    return UnionCase(Matrix("U7_counters", s, 2, cases))


# --------------------------------------------------------------------------
# U8: many partitions
# --------------------------------------------------------------------------
U8_HEADERS = [([b"a", b"c"], []), ([b"b", b"zm"], [b"s2"]),
              ([b"a", b"b", b"c", b"zm"], [b"s1", b"s2"])]
U8_SIZES = (300, 70, 130)


def u8():
    """300, 70 and 130 partitions, about half of the smaller inputs' keys
    shared with the first; 1-4 rows each, so the first input alone holds more
    than 256 unfiltereds. The smallest sizes that put a source boundary inside
    a 256-thread block of the parse kernels and make the complex-arena scan
    cross blocks."""
    rnd = random.Random(20250)
    keys = [list(range(300)),
            sorted(rnd.sample(range(300), 35) + rnd.sample(range(300, 400), 35)),
            sorted(rnd.sample(range(300), 65) + rnd.sample(range(300, 400), 65))]
    types = dict((nm, t) for nm, t in U1_SCHEMA.regular_cols + U1_SCHEMA.static_cols)
    ridx = {nm: i for i, (nm, _) in enumerate(U1_SCHEMA.regular_cols)}
    sidx = {nm: i for i, (nm, _) in enumerate(U1_SCHEMA.static_cols)}

    def cell(nm, path=None):
        ts = T + rnd.randint(-1, 1)     # few timestamps: many ties
        k = rnd.random()
        if k < 0.15:
            return Cell(ts, b"", L + rnd.randint(0, 1), path=path)
        v = lng(rnd.randint(-2, 2)) if types[nm] == LONG else rnd.choice([b"", b"p", b"q", b"pq"])
        if k < 0.3:
            return Cell(ts, v, L, 60, path=path)
        return Cell(ts, v, path=path)

    def row(ck, regular):
        r = Row(K(ck))
        if rnd.random() < 0.4:
            r.live = Live(T + rnd.randint(-1, 1))
        if rnd.random() < 0.15:
            r.del_ = DT(T + rnd.randint(-1, 1), L)
        for nm in regular:
            if rnd.random() < 0.4:
                continue
            if types[nm] == MAP_BB:
                d = DT(T + rnd.randint(-2, 0), L) if rnd.random() < 0.3 else DT_LIVE
                paths = sorted(rnd.sample([b"k1", b"k2", b"k3", b"k4"], rnd.randint(0, 3)))
                if d.live and not paths:
                    continue
                r.complex[ridx[nm]] = (d, [cell(nm, p) for p in paths])
            else:
                r.cells[ridx[nm]] = cell(nm)
        if r.is_empty():
            r.live = Live(T)
        return r

    parts = [dict(), dict(), dict()]
    for i, (regular, static) in enumerate(U8_HEADERS):
        for k in keys[i]:
            p = Partition(b"")
            if rnd.random() < 0.1:
                p.del_ = DT(T + rnd.randint(-1, 0), L)
            if static and rnd.random() < 0.6:
                p.static = Row((), cells={sidx[nm]: cell(nm) for nm in static
                                          if rnd.random() < 0.7})
            p.items = [row(ck, regular) for ck in sorted(rnd.sample(range(6), rnd.randint(1, 4)))]
            parts[i][k] = p
    cases = [Case(f"key {k}", [parts[i].get(k) for i in range(3)]) for k in range(400)]
    return UnionCase(Matrix("U8_many", U1_SCHEMA, 3, cases), headers=U8_HEADERS,
                     all_columns_partial=True, may_hold_unused=True)


# --------------------------------------------------------------------------
# garbage collection: the tombstone source's header is {b} only
# --------------------------------------------------------------------------
def gc_case():
    """Data inputs {a,b} and {a}; the tombstone source knows b alone."""
    s = Schema(ck_types=(LONG,), regular_cols=((b"a", BYTES), (b"b", BYTES)))
    cases = [
        Case("source tombstone over b", [
            P(Row(K(1), cells={0: Cell(T, b"a"), 1: Cell(T, b"b")})),
            P(Row(K(1), cells={0: Cell(T + 1, b"a2")}))],
            P(Row(K(1), cells={1: Cell(T + 1, b"", L)}))),
        Case("source tombstone older than b", [
            P(Row(K(1), cells={0: Cell(T, b"a"), 1: Cell(T, b"b")})),
            None],
            P(Row(K(1), cells={1: Cell(T - 1, b"", L)}))),
        Case("source row deletion next to its b", [
            P(Row(K(1), Live(T), cells={1: Cell(T + 2, b"b")}), Row(K(2), cells={1: Cell(T, b"k")})),
            P(Row(K(1), cells={0: Cell(T, b"a")}), Row(K(3), cells={0: Cell(T, b"z")}))],
            P(Row(K(1), del_=DT(T + 1, L)), Row(K(2), cells={1: Cell(T, b"", L)}))),
        Case("source partition deletion", [
            P(Row(K(1), cells={0: Cell(T, b"a"), 1: Cell(T + 5, b"b")})),
            P(Row(K(1), cells={0: Cell(T + 5, b"a")}))],
            Partition(b"", del_=DT(T + 1, L),
                      items=[Row(K(9), cells={1: Cell(T, b"", L)})])),
        Case("no source partition", [
            P(Row(K(1), cells={1: Cell(T, b"b")})), P(Row(K(1), cells={0: Cell(T, b"a")}))]),
    ]
    return UnionCase(Matrix("GC_narrow_source", s, 2, cases, has_tomb_source=True))


ALL_CASES = {"U1": u1, "U2": u2, "U2s": lambda: u2(True), "U3": u3, "U4": u4, "U5": u5, "U6": u6,
             "U7": u7, "U8": u8}
PREDICTED = ("U1", "U2", "U2s", "U3", "U4", "U5", "U6")     # inside the Python model
