"""Hand-authored sstables for the merge, reconcile and purge edge cases.

The shared generator never produces a timestamp tie, a range bound on a
row's clustering, a deletion at the timestamp of the data it covers, or a
purge parameter on a stored value. This module authors exactly those:

  * a builder from small Python descriptions to the GMD2 memdump, which
    `oracle_tool fromdump` writes as an sstable and `flush_table` flushes;
  * a Python model of the reference merge rules, written from the Java
    sources (Cells.reconcile, LivenessInfo.supersedes, DeletionTime,
    Row.Merger, RangeTombstoneMarker.Merger, PurgeFunction, AbstractCell
    .purge, Rows.removeShadowedCells). Every rule reports the line that
    decided, into a census;
  * the case matrices: one partition per case, keyed by its case number;
  * a reporter that names the differing cases of two sstables.

Plain helper module: no fixtures, not a conftest.
"""
import itertools
import os
import struct
import subprocess
from dataclasses import dataclass, field, replace
from typing import Optional

NO_TS = -2 ** 63
LDT_NONE = 0xFFFFFFFF
NO_DELETION_TIME = 2 ** 63 - 1          # long form of "no local deletion time"
NO_TTL = 0
EXPIRED_TTL = 2 ** 31 - 1               # LivenessInfo.EXPIRED_LIVENESS_TTL
NO_EXPIRATION = 2 ** 63 - 1
TIMESTAMP_EPOCH = 1442880000000000      # EncodingStats epochs
DELETION_TIME_EPOCH = 1442880000

# ClusteringPrefix.Kind ordinals
EXCL_END, INCL_START, EXCL_END_INCL_START = 0, 1, 2
CLUSTERING = 4
INCL_END_EXCL_START, INCL_END, EXCL_START = 5, 6, 7
BOUNDARY_KINDS = (EXCL_END_INCL_START, INCL_END_EXCL_START)
KIND_NAMES = {0: "EXCL_END", 1: "INCL_START", 2: "EXCL_END_INCL_START",
              5: "INCL_END_EXCL_START", 6: "INCL_END", 7: "EXCL_START"}

# memdump type ordinals (oracle CqlType)
BYTES, UTF8, ASCII, LONG, INT32, MAP_BB, COUNTER = range(7)

# fixed points of every matrix. L lies after the default `now` so that
# expiring cells stay expiring (and keep their ttl) unless a job says otherwise.
T = 1_700_000_000_000_000
L = 1_900_000_000
NOW = 1_800_000_000


# --------------------------------------------------------------------------
# logical model
# --------------------------------------------------------------------------
@dataclass(frozen=True)
class DT:
    mfda: int = NO_TS
    ldt: int = LDT_NONE

    @property
    def live(self):
        return self.mfda == NO_TS and self.ldt == LDT_NONE


DT_LIVE = DT()


@dataclass(frozen=True)
class Live:
    ts: int = NO_TS
    ttl: int = NO_TTL
    let: int = NO_EXPIRATION

    @property
    def empty(self):
        return self.ts == NO_TS


LIVE_EMPTY = Live()


@dataclass(frozen=True)
class Cell:
    ts: int
    value: bytes = b""
    ldt: int = LDT_NONE
    ttl: int = NO_TTL
    path: Optional[bytes] = None


@dataclass
class Row:
    ck: tuple = ()
    live: Live = LIVE_EMPTY
    del_: DT = DT_LIVE
    cells: dict = field(default_factory=dict)      # column index -> Cell
    complex: dict = field(default_factory=dict)    # column index -> (DT, [Cell])

    def is_empty(self):
        return self.live.empty and self.del_.live and not self.cells and not self.complex


@dataclass
class Marker:
    kind: int
    ck: tuple
    end_dt: DT
    start_dt: DT = DT_LIVE

    @property
    def boundary(self):
        return self.kind in BOUNDARY_KINDS

    @property
    def opens(self):
        return self.kind in (INCL_START, EXCL_START) or self.boundary

    @property
    def open_dt(self):
        return self.start_dt if self.boundary else self.end_dt


@dataclass
class Partition:
    key: bytes
    del_: DT = DT_LIVE
    static: Optional[Row] = None
    items: list = field(default_factory=list)      # Row | Marker, clustering order


@dataclass
class Schema:
    ck_types: tuple = ()
    static_cols: tuple = ()        # ((name, type), ...), sorted by name
    regular_cols: tuple = ((b"v", BYTES),)
    key_type: int = LONG
    snappy: int = 0
    bti: int = 0
    column_index_size: int = 65536


def case_key(n):
    return struct.pack(">q", n)


def key_case(key):
    return struct.unpack(">q", key)[0]


def ck_long(v):
    return struct.pack(">q", v)


# --------------------------------------------------------------------------
# GMD2 writer / reader
# --------------------------------------------------------------------------
def header_stats(parts):
    """min timestamp / local deletion time / ttl over the content, with the
    EncodingStats epoch defaults, as the oracle's generator collects them."""
    tss, ldts, ttls = [], [], []

    def dt(d):
        if not d.live:
            tss.append(d.mfda)
            ldts.append(d.ldt)

    def cell(c):
        tss.append(c.ts)
        if c.ldt != LDT_NONE:
            ldts.append(c.ldt)
        if c.ttl != NO_TTL:
            ttls.append(c.ttl)

    def row(r):
        if not r.live.empty:
            tss.append(r.live.ts)
            if r.live.ttl != NO_TTL:
                ttls.append(r.live.ttl)
                ldts.append(r.live.let)
        dt(r.del_)
        for c in r.cells.values():
            cell(c)
        for d, cs in r.complex.values():
            dt(d)
            for c in cs:
                cell(c)

    for p in parts:
        dt(p.del_)
        if p.static is not None:
            row(p.static)
        for it in p.items:
            if isinstance(it, Row):
                row(it)
            else:
                dt(it.end_dt)
                if it.boundary:
                    dt(it.start_dt)
    return (min(tss) if tss else TIMESTAMP_EPOCH,
            min(ldts) if ldts else DELETION_TIME_EPOCH,
            min(ttls) if ttls else 0)


def to_gmd2(schema, parts):
    o = bytearray(b"GMD2")
    # authored values stay tiny; a counter context cannot (34 bytes a shard)
    max_value = 64 if any(t == COUNTER for _, t in schema.regular_cols) else 16
    u8 = lambda v: o.append(v)
    u32 = lambda v: o.extend(struct.pack("<I", v))
    i32 = lambda v: o.extend(struct.pack("<i", v))
    i64 = lambda v: o.extend(struct.pack("<q", v))

    def blob(b):
        u32(len(b))
        o.extend(b)

    def dt(d):
        i64(d.mfda)
        u32(d.ldt)

    def cell(c):
        if c is None:
            u8(0)
            return
        assert len(c.value) <= max_value
        tomb = c.ldt != LDT_NONE and c.ttl == NO_TTL
        assert not (tomb and c.value)
        u8(1 | (0 if tomb else 2) | (4 if c.ttl != NO_TTL else 0))
        i64(c.ts)
        u32(c.ldt)
        i32(c.ttl)
        blob(c.value)

    def clustering(ck):
        u8(len(ck))
        for v in ck:
            u8(2 if v is None else 0)      # None == a null component
            blob(v or b"")

    def row_head(r):
        u8(1 | (0 if r.live.empty else 2) | (0 if r.del_.live else 4))
        i64(r.live.ts)
        i32(r.live.ttl)
        i64(r.live.let)
        dt(r.del_)

    u8(schema.key_type)
    u32(len(schema.ck_types))
    for t in schema.ck_types:
        u8(t)
    for cols in (schema.static_cols, schema.regular_cols):
        assert list(cols) == sorted(cols), "columns go in name order"
        u32(len(cols))
        for nm, t in cols:
            blob(nm)
            u8(t)
    u8(schema.snappy)
    u8(schema.bti)
    u32(schema.column_index_size)
    mts, mldt, mttl = header_stats(parts)
    i64(mts)
    i64(mldt)
    i32(mttl)
    o.extend(struct.pack("<Q", len(parts)))
    for p in parts:
        blob(p.key)
        dt(p.del_)
        if schema.static_cols:
            if p.static is None or p.static.is_empty():
                u8(0)
            else:
                row_head(p.static)
                for i in range(len(schema.static_cols)):
                    cell(p.static.cells.get(i))
        u32(len(p.items))
        for it in p.items:
            if isinstance(it, Row):
                u8(0)
                clustering(it.ck)
                row_head(it)
                for i, (_, t) in enumerate(schema.regular_cols):
                    if t == MAP_BB:
                        if i not in it.complex:
                            u8(0)
                            continue
                        d, cs = it.complex[i]
                        u8(1)
                        dt(d)
                        u32(len(cs))
                        for c in cs:
                            cell(c)
                            blob(c.path)
                    else:
                        cell(it.cells.get(i))
            else:
                u8(1)
                u8(it.kind)
                clustering(it.ck)
                dt(it.end_dt)
                dt(it.start_dt)
    return bytes(o)


def parse_gmd2(data):
    """GMD2 bytes -> (Schema, (min_ts, min_ldt, min_ttl), [Partition])."""
    assert data[:4] == b"GMD2", "bad memdump magic"
    pos = [4]

    def take(fmt):
        v = struct.unpack_from(fmt, data, pos[0])[0]
        pos[0] += struct.calcsize(fmt)
        return v

    u8 = lambda: take("<B")
    u32 = lambda: take("<I")
    i32 = lambda: take("<i")
    i64 = lambda: take("<q")

    def blob():
        n = u32()
        b = bytes(data[pos[0]:pos[0] + n])
        assert len(b) == n, "memdump truncated"
        pos[0] += n
        return b

    def dt():
        m = i64()
        return DT(m, u32())

    def cell(with_path=False):
        if not u8():
            return None
        ts, ldt, ttl, v = i64(), u32(), i32(), blob()
        return Cell(ts, v, ldt, ttl, blob() if with_path else None)

    def clustering():
        out = []
        for _ in range(u8()):
            state, v = u8(), blob()
            out.append(None if state == 2 else v)
        return tuple(out)

    def row_head(r):
        ts, ttl, let = i64(), i32(), i64()
        r.live = Live(ts, ttl, let)
        r.del_ = dt()

    s = Schema()
    s.key_type = u8()
    s.ck_types = tuple(u8() for _ in range(u32()))
    s.static_cols = tuple((blob(), u8()) for _ in range(u32()))
    s.regular_cols = tuple((blob(), u8()) for _ in range(u32()))
    s.snappy, s.bti, s.column_index_size = u8(), u8(), u32()
    stats = (i64(), i64(), i32())
    parts = []
    for _ in range(take("<Q")):
        p = Partition(blob())
        p.del_ = dt()
        if s.static_cols and u8():
            p.static = Row()
            row_head(p.static)
            for i in range(len(s.static_cols)):
                c = cell()
                if c is not None:
                    p.static.cells[i] = c
        for _ in range(u32()):
            if u8() == 0:
                r = Row(clustering())
                u8()
                row_head(r)
                for i, (_, t) in enumerate(s.regular_cols):
                    if t == MAP_BB:
                        if u8():
                            d = dt()
                            r.complex[i] = (d, [cell(True) for _ in range(u32())])
                    else:
                        c = cell()
                        if c is not None:
                            r.cells[i] = c
                p.items.append(r)
            else:
                k = u8()
                ck = clustering()
                e = dt()
                p.items.append(Marker(k, ck, e, dt()))
        parts.append(p)
    assert pos[0] == len(data), "memdump trailing bytes"
    return s, stats, parts


# --------------------------------------------------------------------------
# the reference rules. Each returns its decision and records the rule line
# that made it in `census`, a dict (rule, line, outcome) -> count.
# --------------------------------------------------------------------------
class Census(dict):
    def hit(self, rule, line, outcome):
        k = (rule, line, outcome)
        self[k] = self.get(k, 0) + 1


def _ldt_long(ldt):
    return NO_DELETION_TIME if ldt == LDT_NONE else ldt


def reconcile(left, right, census=None):
    """Cells.reconcile / resolveRegular. Returns (winner, line)."""
    def done(w, line):
        if census is not None:
            census.hit("reconcile", line, "left" if w is left else "right")
        return w, line

    if left.ts != right.ts:
        return done(left if left.ts > right.ts else right, "timestamp")
    l_dt, r_dt = left.ldt != LDT_NONE, right.ldt != LDT_NONE
    if l_dt or r_dt:
        # a tombstone or expiring cell beats a live cell of the same timestamp
        if l_dt != r_dt:
            return done(left if l_dt else right, "has_deletion_time")
        # then a tombstone beats an expiring cell
        l_tomb, r_tomb = left.ttl == NO_TTL, right.ttl == NO_TTL
        if l_tomb != r_tomb:
            return done(left if l_tomb else right, "tombstone_vs_expiring")
        if left.ldt != right.ldt:
            return done(left if left.ldt > right.ldt else right, "local_deletion_time")
    # compareValues: unsigned lexicographic (bytes compare that way); left on a tie
    if left.value == right.value:
        return done(left, "full_tie")
    return done(left if left.value > right.value else right, "value")


def reconcile_column(col_type, left, right, census=None):
    """Cells.reconcile for a column of the given type: the winner."""
    if col_type == COUNTER:
        # Cells.resolveCounter: a tombstone beats a live counter whatever the
        # timestamps; two tombstones reconcile as regular cells
        l_tomb, r_tomb = left.ldt != LDT_NONE, right.ldt != LDT_NONE
        assert l_tomb or r_tomb, "context merges are outside this model"
        if l_tomb != r_tomb:
            if census is not None:
                census.hit("counter", "tombstone_vs_live", "left" if l_tomb else "right")
            return left if l_tomb else right
    return reconcile(left, right, census)[0]


def liveness_supersedes(a, b, census=None):
    """LivenessInfo.supersedes: does a supersede b?"""
    def done(v, line):
        if census is not None and not a.empty and not b.empty:
            census.hit("liveness", line, v)
        return v

    if a.ts != b.ts:
        return done(a.ts > b.ts, "timestamp")
    a_expired, b_expired = a.ttl == EXPIRED_TTL, b.ttl == EXPIRED_TTL
    if a_expired != b_expired:
        return done(a_expired, "expired")
    a_exp, b_exp = a.ttl != NO_TTL, b.ttl != NO_TTL
    if a_exp == b_exp:
        return done(a.let > b.let, "expiration_time")
    return done(a_exp, "expiring")


def dt_supersedes(a, b, census=None):
    """DeletionTime.supersedes."""
    if a.mfda != b.mfda:
        v, line = a.mfda > b.mfda, "marked_for_delete_at"
    else:
        v, line = _ldt_long(a.ldt) > _ldt_long(b.ldt), "local_deletion_time"
    if census is not None and not a.live and not b.live:
        census.hit("dt_supersedes", line, v)
    return v


def dt_deletes(d, ts, census=None):
    """DeletionTime.deletes(timestamp)."""
    if census is not None and not d.live and ts != NO_TS:
        census.hit("deletes", "<" if ts < d.mfda else "==" if ts == d.mfda else ">", ts <= d.mfda)
    return ts <= d.mfda


def cell_is_live(c, now):
    return c.ldt == LDT_NONE or (c.ttl != NO_TTL and now < c.ldt)


# --- clustering order (ClusteringComparator + ClusteringPrefix.Kind) ---
_KIND_COMPARISON = {0: 0, 1: 0, 2: 0, 3: 1, 4: 2, 5: 3, 6: 3, 7: 3}
_KIND_VS_CLUSTERING = {0: -1, 1: -1, 2: -1, 3: -1, 4: 0, 5: 1, 6: 1, 7: 1}


def _cmp(a, b):
    return (a > b) - (a < b)


def _cmp_component(t, a, b):
    if t == LONG:
        return _cmp(struct.unpack(">q", a)[0], struct.unpack(">q", b)[0])
    return _cmp(a, b)


def compare_prefix(ck_types, ka, a, kb, b):
    for i in range(min(len(a), len(b))):
        c = _cmp_component(ck_types[i], a[i], b[i])
        if c:
            return c
    if len(a) == len(b):
        return _cmp(_KIND_COMPARISON[ka], _KIND_COMPARISON[kb])
    return _KIND_VS_CLUSTERING[ka] if len(a) < len(b) else -_KIND_VS_CLUSTERING[kb]


def _item_kind(it):
    return CLUSTERING if isinstance(it, Row) else it.kind


def compare_items(ck_types, a, b):
    return compare_prefix(ck_types, _item_kind(a), a.ck, _item_kind(b), b.ck)


def sort_items(ck_types, items):
    import functools
    return sorted(items, key=functools.cmp_to_key(lambda a, b: compare_items(ck_types, a, b)))


# --- Row.Merger ---
def merge_rows(versions, active, cols, census):
    """versions: Row or None per source, in source order. None == no row."""
    present = [r for r in versions if r is not None]
    if len(present) == 1 and active.live:
        return present[0]
    info, row_del = LIVE_EMPTY, DT_LIVE
    for r in present:
        if liveness_supersedes(r.live, info, census):
            info = r.live
        if dt_supersedes(r.del_, row_del, census):
            row_del = r.del_
    if dt_supersedes(row_del, active, census):
        active = row_del
    else:
        row_del = DT_LIVE
    if dt_deletes(active, info.ts, census):
        info = LIVE_EMPTY
    out = Row(present[-1].ck, info, row_del)
    for ci, (_, t) in enumerate(cols):
        if t == MAP_BB:
            cds = [r.complex[ci] for r in present if ci in r.complex]
            if not cds:
                continue
            cdel = DT_LIVE
            for d, _ in cds:
                if dt_supersedes(d, cdel, census):
                    cdel = d
            cell_active, out_del = active, DT_LIVE
            if dt_supersedes(cdel, active, census):
                cell_active = out_del = cdel
            merged = {}
            for _, cs in cds:          # source order per path
                for c in cs:
                    if dt_deletes(cell_active, c.ts, census):
                        continue
                    merged[c.path] = c if c.path not in merged else \
                        reconcile(merged[c.path], c, census)[0]
            if out_del.live and not merged:
                continue
            out.complex[ci] = (out_del, [merged[k] for k in sorted(merged)])
            continue
        m = None
        for r in present:
            c = r.cells.get(ci)
            if c is None or dt_deletes(active, c.ts, census):
                continue
            m = c if m is None else reconcile_column(t, m, c, census)
        if m is not None:
            out.cells[ci] = m
    return None if out.is_empty() else out


# --- RangeTombstoneMarker.Merger ---
class MarkerMerger:
    def __init__(self, n, partition_del, census):
        self.pdel, self.open, self.biggest, self.census = partition_del, [None] * n, -1, census

    def open_in_merged(self):
        if self.biggest < 0:
            return DT_LIVE
        d = self.open[self.biggest]
        return d if dt_supersedes(d, self.pdel, self.census) else DT_LIVE

    def active(self):
        d = self.open_in_merged()
        return self.pdel if d.live else d

    def merge(self, versions):
        prev = self.open_in_merged()
        bound = None
        for i, m in enumerate(versions):
            if m is None:
                continue
            bound = m
            self.open[i] = m.open_dt if m.opens else None
        self.biggest = -1
        for i, d in enumerate(self.open):
            if d is not None and (self.biggest < 0 or
                                  dt_supersedes(d, self.open[self.biggest], self.census)):
                self.biggest = i
        nxt = self.open_in_merged()
        if prev == nxt:
            return None
        before = _KIND_VS_CLUSTERING[bound.kind] < 0
        if prev.live:
            out = Marker(INCL_START if before else EXCL_START, bound.ck, nxt)
        elif nxt.live:
            out = Marker(EXCL_END if before else INCL_END, bound.ck, prev)
        else:
            out = Marker(EXCL_END_INCL_START if before else INCL_END_EXCL_START,
                         bound.ck, prev, nxt)
        self.census.hit("marker_emitted", KIND_NAMES[out.kind], True)
        return out


def merge_partitions(versions, schema, census):
    """UnfilteredRowIterators.merge over the versions of one partition."""
    if len(versions) == 1:
        return versions[0]
    out = Partition(versions[0].key)
    pdel = DT_LIVE
    for p in versions:
        if not dt_supersedes(pdel, p.del_, census):
            pdel = p.del_
    out.del_ = pdel
    statics = [p.static for p in versions if p.static is not None and not p.static.is_empty()]
    if statics:
        out.static = merge_rows(statics, pdel, schema.static_cols, census)
    pos = [0] * len(versions)
    mm = MarkerMerger(len(versions), pdel, census)
    while True:
        heads = [(i, p.items[pos[i]]) for i, p in enumerate(versions) if pos[i] < len(p.items)]
        if not heads:
            break
        first = heads[0][1]
        for _, it in heads[1:]:
            if compare_items(schema.ck_types, it, first) < 0:
                first = it
        rows, markers = [None] * len(versions), [None] * len(versions)
        for i, it in heads:
            if compare_items(schema.ck_types, it, first) == 0:
                (rows if isinstance(it, Row) else markers)[i] = it
                pos[i] += 1
        if isinstance(first, Row):
            r = merge_rows(rows, mm.active(), schema.regular_cols, census)
        else:
            r = mm.merge(markers)
        if r is not None:
            out.items.append(r)
    return out


# --- purge (PurgeFunction, BTreeRow.purge, AbstractCell.purge) ---
@dataclass
class Job:
    now: int = NOW
    gc_before: int = NO_TS
    never_purge: bool = False
    overlap_min_ts: Optional[int] = None    # one overlap entry covering every token
    cell_level_gc: bool = False

    def oracle_args(self):
        a = [f"now={self.now}", f"gcbefore={self.gc_before}"]
        if self.never_purge:
            a.append("nevergc=1")
        if self.cell_level_gc:
            a.append("cellgc=1")
        if self.overlap_min_ts is not None:
            a.append(f"ov={NO_TS}:{2 ** 63 - 1}:{self.overlap_min_ts}")
        return a

    def gpu_kwargs(self):
        kw = dict(now_sec=self.now, gc_before=self.gc_before, never_purge=self.never_purge,
                  cell_level_gc=self.cell_level_gc)
        if self.overlap_min_ts is not None:
            kw["overlaps"] = [(NO_TS, 2 ** 63 - 1, self.overlap_min_ts)]
        return kw


def should_purge(job, ts, ldt, census):
    """The DeletionPurger of a compaction: strictly before gc_before, and
    strictly older than every overlapping sstable's minimum timestamp."""
    if job.never_purge:
        census.hit("purge", "never_purge", False)
        return False
    if not ldt < job.gc_before:
        census.hit("purge", "gc_before==" if ldt == job.gc_before else "gc_before>", False)
        return False
    if job.overlap_min_ts is not None and not ts < job.overlap_min_ts:
        census.hit("purge", "overlap==" if ts == job.overlap_min_ts else "overlap>", False)
        return False
    census.hit("purge", "purged", True)
    return True


def purge_dt(job, d, census):
    return not d.live and should_purge(job, d.mfda, _ldt_long(d.ldt), census)


def purge_cell(job, c, census):
    if cell_is_live(c, job.now):
        if c.ttl != NO_TTL:
            census.hit("expiry", "now<let", False)
        return c
    if c.ttl != NO_TTL:
        census.hit("expiry", "now==let" if job.now == c.ldt else "now>let", True)
    if should_purge(job, c.ts, _ldt_long(c.ldt), census):
        return None
    if c.ttl != NO_TTL:
        # an expired cell becomes a tombstone dated when it was written
        return purge_cell(job, Cell(c.ts, b"", c.ldt - c.ttl, NO_TTL, c.path), census)
    return c


def purge_row(job, r, census):
    live = r.live
    is_live = not live.empty and live.ttl != EXPIRED_TTL and \
        (live.ttl == NO_TTL or job.now < live.let)
    if not live.empty and live.ttl not in (NO_TTL, EXPIRED_TTL):
        census.hit("expiry", "liveness now<let" if is_live else
                   "liveness now==let" if job.now == live.let else "liveness now>let", not is_live)
    out = Row(r.ck, live, r.del_)
    if not live.empty and not is_live and should_purge(job, live.ts, live.let, census):
        out.live = LIVE_EMPTY
    if purge_dt(job, r.del_, census):
        out.del_ = DT_LIVE
    for ci, c in r.cells.items():
        c = purge_cell(job, c, census)
        if c is not None:
            out.cells[ci] = c
    for ci, (d, cs) in r.complex.items():
        if purge_dt(job, d, census):
            d = DT_LIVE
        cs = [c for c in (purge_cell(job, c, census) for c in cs) if c is not None]
        if not d.live or cs:
            out.complex[ci] = (d, cs)
    return None if out.is_empty() else out


def purge_partition(job, p, census):
    out = Partition(p.key, DT_LIVE if purge_dt(job, p.del_, census) else p.del_)
    if p.static is not None and not p.static.is_empty():
        out.static = purge_row(job, p.static, census)
    for it in p.items:
        if isinstance(it, Row):
            it = purge_row(job, it, census)
        elif it.boundary:
            pc, po = purge_dt(job, it.end_dt, census), purge_dt(job, it.start_dt, census)
            incl_start = it.kind == EXCL_END_INCL_START
            if pc and po:
                it = None
            elif pc:
                it = Marker(INCL_START if incl_start else EXCL_START, it.ck, it.start_dt)
            elif po:
                it = Marker(EXCL_END if incl_start else INCL_END, it.ck, it.end_dt)
        elif purge_dt(job, it.end_dt, census):
            it = None
        if it is not None:
            out.items.append(it)
    if out.del_.live and not out.items and out.static is None:
        return None
    return out


# --- garbage skipping against a tombstone source (rows only) ---
def _gc_row(data, tomb, active, cell_level, census, cols=((b"v", BYTES),)):
    tomb_del = tomb.del_ if tomb is not None else DT_LIVE
    deletion = tomb_del if dt_supersedes(tomb_del, active, census) else active
    out = Row(data.ck)
    if not cell_level:
        # BTreeRow.filter(all, activeDeletion, setActiveDeletionToRow=false)
        if deletion.live or dt_supersedes(data.del_, deletion, census):
            return data
        if not dt_deletes(deletion, data.live.ts, census):
            out.live = data.live
        for ci, c in data.cells.items():
            if not dt_deletes(deletion, c.ts, census):
                out.cells[ci] = c
        assert not data.complex
        return None if out.is_empty() else out
    # Rows.removeShadowedCells
    if not dt_deletes(deletion, data.live.ts, census):
        out.live = data.live
    if not dt_supersedes(deletion, data.del_, census):
        out.del_ = data.del_
    for ci, c in data.cells.items():
        if dt_deletes(deletion, c.ts, census):
            continue
        upd = tomb.cells.get(ci) if tomb is not None else None
        # dropped iff reconcile(existing, update) hands back the update
        if upd is not None and reconcile_column(cols[ci][1], c, upd, census) is not c:
            continue
        out.cells[ci] = c
    assert not data.complex
    return None if out.is_empty() else out


def gc_partition(data, tomb, cell_level, census, schema=None):
    assert all(isinstance(i, Row) for i in data.items + tomb.items), "rows only"
    out = Partition(data.key)
    out.del_ = data.del_ if dt_supersedes(data.del_, tomb.del_, census) else DT_LIVE
    active = tomb.del_
    if data.static is not None:
        out.static = _gc_row(data.static, tomb.static, active, cell_level, census,
                             schema.static_cols if schema else ())
    trows = {r.ck: r for r in tomb.items}
    for r in data.items:
        t = trows.get(r.ck)
        if t is None:
            # no row in the source at this clustering: only the partition deletion applies
            r = _gc_row(r, None, active, False, census)
        else:
            r = _gc_row(r, t, active, cell_level, census, schema.regular_cols if schema else ((b"v", BYTES),))
        if r is not None:
            out.items.append(r)
    return out


# --------------------------------------------------------------------------
# matrices
# --------------------------------------------------------------------------
@dataclass
class Case:
    label: str
    inputs: list                 # Partition or None per input; keys filled in by Matrix
    tomb: Optional[Partition] = None


@dataclass
class Matrix:
    name: str
    schema: Schema
    n_inputs: int
    cases: list
    jobs: list = field(default_factory=lambda: [("default", Job())])
    has_tomb_source: bool = False

    def __post_init__(self):
        # a case's partitions take its number as their key
        for n, c in enumerate(self.cases):
            c.inputs = list(c.inputs) + [None] * (self.n_inputs - len(c.inputs))
            assert len(c.inputs) == self.n_inputs, c.label
            for p in c.inputs + [c.tomb]:
                if p is not None:
                    p.key = case_key(n)
                    p.items = sort_items(self.schema.ck_types, p.items)
                    # an authored input is a legal stream: ranges open and close in turn
                    is_open = False
                    for it in p.items:
                        if isinstance(it, Marker):
                            assert it.boundary == (is_open and it.opens) and \
                                (is_open or it.opens), f"{self.name}: {c.label}: marker order"
                            is_open = it.opens
                    assert not is_open, f"{self.name}: {c.label}: range left open"

    @property
    def labels(self):
        return [c.label for c in self.cases]

    def tables(self):
        """[partitions of input i], tombstone-source partitions."""
        ins = [[p for p in (c.inputs[i] for c in self.cases) if p is not None]
               for i in range(self.n_inputs)]
        return ins, [c.tomb for c in self.cases if c.tomb is not None]

    def write(self, oracle, d):
        """Writes <d>/in<i>.memdump and the sstable <d>/oa-<i+1>-big per
        input (and `tomb`); returns (input bases, tomb base or None)."""
        os.makedirs(d, exist_ok=True)
        ins, tomb = self.tables()
        stem = "da-%d-bti" if self.schema.bti else "oa-%d-big"
        bases = []
        for i, parts in enumerate(ins):
            md = os.path.join(d, f"in{i + 1}.memdump")
            with open(md, "wb") as f:
                f.write(to_gmd2(self.schema, parts))
            bases.append(os.path.join(d, stem % (i + 1)))
            subprocess.run([oracle, "fromdump", md, bases[-1]], check=True, capture_output=True)
        tbase = None
        if self.has_tomb_source:
            md = os.path.join(d, "tomb.memdump")
            with open(md, "wb") as f:
                f.write(to_gmd2(self.schema, tomb))
            tbase = os.path.join(d, stem % 99)
            subprocess.run([oracle, "fromdump", md, tbase], check=True, capture_output=True)
        return bases, tbase

    def predict(self, job, census=None):
        """case number -> Partition the compaction must hold (absent == dropped)."""
        census = Census() if census is None else census
        out = {}
        for n, c in enumerate(self.cases):
            vs = [p for p in c.inputs if p is not None]
            if not vs:
                continue
            m = merge_partitions(vs, self.schema, census)
            if c.tomb is not None:
                m = gc_partition(m, c.tomb, job.cell_level_gc, census, self.schema)
            m = purge_partition(job, m, census)
            if m is not None:
                out[n] = m
        return out


def canonical(p):
    """Partition -> comparable nested tuples (a static row that is empty is absent)."""
    def row(r):
        return ("row", r.ck, r.live, r.del_, tuple(sorted(r.cells.items())),
                tuple((ci, d, tuple(cs)) for ci, (d, cs) in sorted(r.complex.items())))

    def item(it):
        if isinstance(it, Row):
            return row(it)
        return ("marker", KIND_NAMES[it.kind], it.ck, it.end_dt,
                it.start_dt if it.boundary else DT_LIVE)
    st = None if p.static is None or p.static.is_empty() else row(p.static)
    return (p.del_, st, tuple(item(i) for i in p.items))


# cell kinds of matrix A, all at timestamp T unless named otherwise
V16 = b"0123456789abcde"
CELL_KINDS = [
    ("live_a", Cell(T, b"a")),
    ("live_b", Cell(T, b"b")),
    ("live_ab", Cell(T, b"ab")),
    ("live_empty", Cell(T, b"")),
    ("live_7f", Cell(T, b"\x7f")),
    ("live_80", Cell(T, b"\x80")),
    ("live_16x", Cell(T, V16 + b"x")),
    ("live_16y", Cell(T, V16 + b"y")),
    ("exp60_L", Cell(T, b"e", L, 60)),
    ("exp60_L1", Cell(T, b"e", L + 1, 60)),
    ("exp61_L", Cell(T, b"e", L, 61)),
    ("tomb_L", Cell(T, b"", L)),
    ("tomb_L1", Cell(T, b"", L + 1)),
    ("live_a_T-1", Cell(T - 1, b"a")),
    ("live_a_T+1", Cell(T + 1, b"a")),
]
OLD_CELL = Cell(T - 100, b"old")


def _cell_groups():
    """(label, [cell or None per input]) over 2 and 3 inputs."""
    out = []
    for (ln, lc), (rn, rc) in itertools.product(CELL_KINDS, repeat=2):
        out.append((f"pair {ln} | {rn}", [lc, rc, None]))
    n = len(CELL_KINDS)
    for i in range(n):
        a, b, c = CELL_KINDS[i], CELL_KINDS[(i + 1) % n], CELL_KINDS[(i + 2) % n]
        out.append((f"triple {a[0]} | {b[0]} | {c[0]}", [a[1], b[1], c[1]]))
    # fold order: the third input decides after the first two tied
    for (xn, x), (yn, y) in itertools.permutations(CELL_KINDS[:13], 2):
        if (CELL_KINDS.index((xn, x)) + CELL_KINDS.index((yn, y))) % 5 == 0:
            out.append((f"fold {xn} | {yn} | {xn}@T+1", [x, y, replace(x, ts=T + 1)]))
            out.append((f"fold {xn}@T-1 | {yn} | {xn}", [replace(x, ts=T - 1), y, x]))
    return out


SKINNY = Schema()
WIDE = Schema(ck_types=(LONG,), static_cols=((b"s", BYTES),),
              regular_cols=((b"a", BYTES), (b"b", BYTES), (b"c", BYTES)))
MAPPED = Schema(regular_cols=((b"m", MAP_BB),))
# simple columns go first: the engine takes complex columns only after them
ROWLEVEL = Schema(ck_types=(LONG,), regular_cols=((b"v", BYTES), (b"w", MAP_BB)))
VCOL, MCOL = 0, 1


def matrix_a_skinny():
    cases = []
    for label, cells in _cell_groups():
        cases.append(Case(label, [None if c is None else Partition(b"", items=[Row((), cells={0: c})])
                                  for c in cells]))
    return Matrix("A_i_skinny", SKINNY, 3, cases)


def matrix_a_wide():
    cases = []
    for n, (label, cells) in enumerate(_cell_groups()):
        col = n % 3
        others = [c for c in range(3) if c != col]
        ins = []
        for i, c in enumerate(cells):
            if c is None:
                ins.append(None)
                continue
            r = Row((ck_long(10),), cells={col: c})
            if i < 2:       # each other column lives in one input only
                r.cells[others[i]] = Cell(T - 7, b"only%d" % i)
            ins.append(Partition(b"", static=Row((), cells={0: c}), items=[r]))
        cases.append(Case(f"{label} [col {'abc'[col]}]", ins))
    return Matrix("A_ii_wide", WIDE, 3, cases)


def matrix_a_map():
    cases = []
    for label, cells in _cell_groups():
        cases.append(Case(label, [
            None if c is None else
            Partition(b"", items=[Row((), complex={0: (DT_LIVE, [replace(c, path=b"k")])})])
            for c in cells]))
    # tie pairs on two paths of one row: the winners come from different inputs
    for (an, a), (bn, b) in itertools.product(CELL_KINDS[:6] + CELL_KINDS[8:13], repeat=2):
        l = Row((), complex={0: (DT_LIVE, [replace(a, path=b"k1"), replace(b, path=b"k2")])})
        r = Row((), complex={0: (DT_LIVE, [replace(b, path=b"k1"), replace(a, path=b"k2")])})
        cases.append(Case(f"two paths {an},{bn} | {bn},{an}",
                          [Partition(b"", items=[l]), Partition(b"", items=[r]), None]))
    # path order p < pq < q, spread over the inputs
    for perm in itertools.permutations([b"p", b"pq", b"q"]):
        ins = [Partition(b"", items=[Row((), complex={0: (DT_LIVE, sorted(
            [Cell(T, b"x%d" % i, path=perm[i]), Cell(T, b"y%d" % i, path=perm[(i + 1) % 3])],
            key=lambda c: c.path))})]) for i in range(3)]
        cases.append(Case("path order " + b",".join(perm).decode(), ins))
    return Matrix("A_iii_map", MAPPED, 3, cases)


def matrix_a_eight():
    """8 inputs; the tie is between inputs 3 and 7, the rest older or absent."""
    cases = []
    for n, ((ln, lc), (rn, rc)) in enumerate(itertools.product(CELL_KINDS, repeat=2)):
        cells = [None] * 8
        cells[2], cells[6] = lc, rc
        for i in (0, 1, 3, 4, 5, 7):
            if (n >> i) & 1:
                cells[i] = replace(OLD_CELL, value=b"old%d" % i)
        cases.append(Case(f"8-input {ln} | {rn}", [
            None if c is None else Partition(b"", items=[Row((), cells={0: c})]) for c in cells]))
    return Matrix("A_eight", SKINNY, 8, cases)


# one remote shard: no flagged elements, (id, clock, count)
COUNTER_CTX = b"\0\0" + bytes(range(16)) + struct.pack(">qq", 3, 7)
COUNTER_KINDS = [
    ("tomb_L", Cell(T, b"", L)), ("tomb_L1", Cell(T, b"", L + 1)),
    ("tomb_T-1", Cell(T - 1, b"", L)), ("tomb_T+1", Cell(T + 1, b"", L)),
    ("ctx", Cell(T, COUNTER_CTX)), ("ctx_T-1", Cell(T - 1, COUNTER_CTX)),
    ("ctx_T+1", Cell(T + 1, COUNTER_CTX)),
]


def matrix_a_counter():
    """Counter table: tombstone against tombstone and against a live context."""
    cases = []
    for (ln, lc), (rn, rc) in itertools.product(COUNTER_KINDS, repeat=2):
        if lc.ldt == LDT_NONE and rc.ldt == LDT_NONE:
            continue
        cases.append(Case(f"counter {ln} | {rn}", [Partition(b"", items=[Row((), cells={0: lc})]),
                                                    Partition(b"", items=[Row((), cells={0: rc})])]))
    return Matrix("A_counter", Schema(regular_cols=((b"v", COUNTER),)), 2, cases)


def matrix_a_counter_gc():
    """The same counter pairs with the right cell in the tombstone source."""
    cases = []
    for (ln, lc), (rn, rc) in itertools.product(COUNTER_KINDS, repeat=2):
        if lc.ldt == LDT_NONE and rc.ldt == LDT_NONE:
            continue
        cases.append(Case(f"gc counter {ln} | {rn}", [Partition(b"", items=[Row((), cells={0: lc})])],
                          Partition(b"", items=[Row((), cells={0: rc})])))
    return Matrix("A_counter_gc", Schema(regular_cols=((b"v", COUNTER),)), 1, cases,
                  jobs=[("rowgc", Job()), ("cellgc", Job(cell_level_gc=True))], has_tomb_source=True)


def matrix_a_gc():
    """Left cell in the data input, right cell in the tombstone source; plus
    row and partition deletions in the source at the data's timestamp."""
    cases = []
    for (ln, lc), (rn, rc) in itertools.product(CELL_KINDS, repeat=2):
        cases.append(Case(f"gc {ln} | {rn}", [Partition(b"", items=[Row((), cells={0: lc})])],
                          Partition(b"", items=[Row((), cells={0: rc})])))
    data = lambda: Partition(b"", items=[Row((), Live(T), cells={0: Cell(T, b"d")})])
    for d in (-1, 0, 1):
        cases.append(Case(f"gc row deletion mfda=T{d:+d}", [data()],
                          Partition(b"", items=[Row((), del_=DT(T + d, L))])))
        cases.append(Case(f"gc partition deletion mfda=T{d:+d}", [data()],
                          Partition(b"", del_=DT(T + d, L))))
        p = data()
        p.items[0].del_ = DT(T - 50, L)
        cases.append(Case(f"gc own row deletion under source mfda=T-50{d:+d}", [p],
                          Partition(b"", items=[Row((), del_=DT(T - 50 + d, L))])))
    return Matrix("A_iv_gc", SKINNY, 1, cases,
                  jobs=[("rowgc", Job()), ("cellgc", Job(cell_level_gc=True))],
                  has_tomb_source=True)


LIVENESS_KINDS = [
    ("plain", Live(T)),
    ("exp_L", Live(T, 60, L)),
    ("exp_L1", Live(T, 60, L + 1)),
    ("expired", Live(T, EXPIRED_TTL, L)),
    ("plain_T-1", Live(T - 1)),
    ("plain_T+1", Live(T + 1)),
]
CK = (ck_long(10),)


def matrix_b():
    cases = []
    part = lambda r, **kw: Partition(b"", items=[r], **kw)
    for (an, a), (bn, b) in itertools.product(LIVENESS_KINDS, repeat=2):
        cases.append(Case(f"liveness {an} | {bn}", [part(Row(CK, a)), part(Row(CK, b))]))
    dts = [("T,L", DT(T, L)), ("T,L+1", DT(T, L + 1)), ("T+1,L", DT(T + 1, L))]
    for (an, a), (bn, b) in itertools.permutations(dts, 2):
        cases.append(Case(f"row deletion {an} | {bn}", [part(Row(CK, del_=a)), part(Row(CK, del_=b))]))
        cases.append(Case(f"partition deletion {an} | {bn}",
                          [Partition(b"", del_=a), Partition(b"", del_=b)]))
    cpx = lambda d, cells: {MCOL: (d, cells)}
    data_kinds = [
        ("liveness", lambda: Row(CK, Live(T))),
        ("simple cell", lambda: Row(CK, cells={VCOL: Cell(T, b"d")})),
        ("complex cell", lambda: Row(CK, complex=cpx(DT_LIVE, [Cell(T, b"d", path=b"k")]))),
        ("complex deletion", lambda: Row(CK, complex=cpx(DT(T, L), []))),
    ]
    for d in (-1, 0, 1):
        for dn, mk in data_kinds:
            for order in (0, 1):
                rd = [part(mk()), part(Row(CK, del_=DT(T + d, L + 1)))]
                pd = [part(mk()), Partition(b"", del_=DT(T + d, L + 1))]
                if order:
                    rd.reverse()
                    pd.reverse()
                cases.append(Case(f"row deletion mfda=ts{d:+d} over {dn} (order {order})", rd))
                cases.append(Case(f"partition deletion mfda=ts{d:+d} over {dn} (order {order})", pd))
        # a complex deletion over cells of its own column, across and within inputs
        cell = Cell(T, b"d", path=b"k")
        cases.append(Case(f"complex deletion mfda=ts{d:+d} over its cell, other input",
                          [part(Row(CK, complex=cpx(DT_LIVE, [cell]))),
                           part(Row(CK, complex=cpx(DT(T + d, L), [])))]))
        cases.append(Case(f"complex deletion mfda=ts{d:+d} over its cell, same input",
                          [part(Row(CK, complex=cpx(DT(T + d, L), [cell]))),
                           part(Row(CK, cells={VCOL: Cell(T - 9, b"z")}))]))
    for rl, pl in ((L, L + 1), (L + 1, L)):
        for order in (0, 1):
            ins = [part(Row(CK, Live(T + 5), del_=DT(T, rl))), Partition(b"", del_=DT(T, pl))]
            if order:
                ins.reverse()
            cases.append(Case(f"row deletion (T,{rl - L:+d}) under partition deletion "
                              f"(T,{pl - L:+d}) (order {order})", ins))
        cases.append(Case(f"row deletion (T,{rl - L:+d}) and partition deletion (T,{pl - L:+d}) "
                          "in one input, merged with a row",
                          [part(Row(CK, Live(T + 5), del_=DT(T, rl)), del_=DT(T, pl)),
                           part(Row(CK, cells={VCOL: Cell(T + 5, b"n")}))]))
    return Matrix("B_rowlevel", ROWLEVEL, 2, cases)


# ---- C: markers and rows in one partition ----
NEG_INF, POS_INF = "-inf", "+inf"


def _range(lo, lo_incl, hi, hi_incl, dt):
    """Two bound markers; lo/hi are clustering prefixes (tuples) or +-inf.
    The open ends are the reference's BOTTOM and TOP: inclusive bounds
    without values (an exclusive one would sort at the other end)."""
    assert (lo != NEG_INF or lo_incl) and (hi != POS_INF or hi_incl)
    s = Marker(INCL_START if lo_incl else EXCL_START, () if lo == NEG_INF else lo, dt)
    e = Marker(INCL_END if hi_incl else EXCL_END, () if hi == POS_INF else hi, dt)
    return [s, e]


def _marker_matrix(name, schema, rows_cks, ranges, tie_ck):
    """ranges: (label, lo, lo_incl, hi, hi_incl). Rows at rows_cks with
    liveness and a cell at T in input 1; a second version of the row at
    tie_ck in input 2."""
    A, B, C, D = DT(T, L), DT(T, L + 1), DT(T + 1, L), DT(T - 1, L)
    combos = [("equal", A, A), ("ldt<", A, B), ("ldt>", B, A), ("mfda over|under", C, D),
              ("mfda under|over", D, C)]
    vcol = 0        # every schema here has its blob column first
    rows1 = lambda: [Row(ck, Live(T), cells={vcol: Cell(T, b"r1")}) for ck in rows_cks]
    row2 = lambda: [Row(tie_ck, Live(T), cells={vcol: Cell(T, b"r2")})]
    cases = []
    for (an, *a), (bn, *b) in itertools.product(ranges, repeat=2):
        for cn, da, db in combos:
            cases.append(Case(f"{an} | {bn} dts {cn}", [
                Partition(b"", items=rows1() + _range(*a, da)),
                Partition(b"", items=row2() + _range(*b, db)), None]))
    n = len(ranges)
    for i in range(n):
        (an, *a), (bn, *b), (cn, *c) = ranges[i], ranges[(i + 3) % n], ranges[(i + 5) % n]
        for dn, da, db, dc in (("A,B,C", A, B, C), ("C,A,A", C, A, A), ("A,A,A", A, A, A)):
            cases.append(Case(f"three inputs {an} | {bn} | {cn} dts {dn}", [
                Partition(b"", items=rows1() + _range(*a, da)),
                Partition(b"", items=row2() + _range(*b, db)),
                Partition(b"", items=_range(*c, dc))]))
    # an input that already holds a boundary marker at tie_ck, of either kind
    lo, hi = ranges[0][1], ranges[4][3]
    for kind in BOUNDARY_KINDS:
        held = [Marker(INCL_START, lo, A), Marker(kind, tie_ck, A, B), Marker(INCL_END, hi, B)]
        for (bn, *b) in ranges:
            for cn, dd in (("A", A), ("B", B), ("C", C), ("D", D)):
                cases.append(Case(f"held {KIND_NAMES[kind]} | {bn} dt {cn}", [
                    Partition(b"", items=rows1() + list(held)),
                    Partition(b"", items=row2() + _range(*b, dd)), None]))
    return Matrix(name, schema, 3, cases)


def matrix_c_bigint():
    k = lambda v: (ck_long(v),)
    ranges = [("[10,20]", k(10), True, k(20), True), ("(10,20)", k(10), False, k(20), False),
              ("[10,20)", k(10), True, k(20), False), ("(10,20]", k(10), False, k(20), True),
              ("[20,30]", k(20), True, k(30), True), ("(20,30]", k(20), False, k(30), True),
              ("[-inf,20]", NEG_INF, True, k(20), True), ("[20,+inf]", k(20), True, POS_INF, True)]
    return _marker_matrix("C_bigint", ROWLEVEL, [k(10), k(20), k(30)], ranges, k(20))


def matrix_c_composite():
    s = Schema(ck_types=(LONG, LONG), regular_cols=((b"v", BYTES),))
    k = lambda *v: tuple(ck_long(x) for x in v)
    ranges = [("[20,20]", k(20), True, k(20), True),              # start and end on one prefix
              ("(10,20)", k(10), False, k(20), False),
              ("[20:1,20:2]", k(20, 1), True, k(20, 2), True),
              ("(20:1,20]", k(20, 1), False, k(20), True),
              ("[20,30:1]", k(20), True, k(30, 1), True),
              ("(20,30]", k(20), False, k(30), True),
              ("[-inf,20:1)", NEG_INF, True, k(20, 1), False),
              ("[20:2,+inf]", k(20, 2), True, POS_INF, True)]
    return _marker_matrix("C_composite", s, [k(10, 1), k(20, 1), k(20, 2), k(30, 1)], ranges, k(20, 1))


def matrix_c_text():
    s = Schema(ck_types=(UTF8,), regular_cols=((b"v", BYTES),))
    k = lambda v: (v,)
    ranges = [("[a,ab]", k(b"a"), True, k(b"ab"), True), ("(a,ab)", k(b"a"), False, k(b"ab"), False),
              ("[a,ab)", k(b"a"), True, k(b"ab"), False), ("(a,ab]", k(b"a"), False, k(b"ab"), True),
              ("[ab,b]", k(b"ab"), True, k(b"b"), True), ("(ab,b]", k(b"ab"), False, k(b"b"), True),
              ("[-inf,ab]", NEG_INF, True, k(b"ab"), True), ("[ab,+inf]", k(b"ab"), True, POS_INF, True)]
    return _marker_matrix("C_text", s, [k(b"a"), k(b"ab"), k(b"b")], ranges, k(b"ab"))


def matrix_c_blocks():
    """Open-ended ranges over partitions wide enough for several index
    blocks, so that a bound without values is a block's first or last entry
    and a range stays open across block ends."""
    k = lambda v: (ck_long(v),)
    n = 4000
    rows = lambda: [Row(k(i), Live(T), cells={0: Cell(T, b"%016d" % i)}) for i in range(n)]
    under, at = DT(T - 1, L), DT(T, L)
    ends = lambda d: _range(NEG_INF, True, k(1000), True, d) + _range(k(3000), True, POS_INF, True, d)
    cases = [
        Case("open ends under the rows, other input",
             [Partition(b"", items=rows()), Partition(b"", items=ends(under))]),
        Case("open ends under the rows, same input", [Partition(b"", items=rows() + ends(under)), None]),
        Case("open ends over the rows", [Partition(b"", items=rows()), Partition(b"", items=ends(at))]),
        Case("whole partition under the rows",
             [Partition(b"", items=rows()), Partition(b"", items=_range(NEG_INF, True, POS_INF, True, under))]),
        Case("whole partition over the rows",
             [Partition(b"", items=rows()), Partition(b"", items=_range(NEG_INF, True, POS_INF, True, at))]),
    ]
    return Matrix("C_blocks", Schema(ck_types=(LONG,)), 2, cases)


# ---- D: job parameters on stored values ----
G = 1_750_000_000            # local deletion time of D's tombstones
E = 1_760_000_000            # expiration time of D's expiring data


def matrix_d():
    part = lambda *items, **kw: Partition(b"", items=list(items), **kw)
    k = lambda v: (ck_long(v),)
    cases = [
        Case("cell tombstone", [part(Row(CK, cells={VCOL: Cell(T, b"", G)})), None]),
        Case("cell tombstone over older cell",
             [part(Row(CK, cells={VCOL: Cell(T, b"", G)})), part(Row(CK, cells={VCOL: Cell(T - 1, b"o")}))]),
        Case("complex cell tombstone and complex deletion",
             [part(Row(CK, complex={MCOL: (DT(T, G), [Cell(T + 1, b"", G, path=b"k")])})), None]),
        Case("row deletion", [part(Row(CK, del_=DT(T, G))), None]),
        Case("row deletion over older row",
             [part(Row(CK, del_=DT(T, G))), part(Row(CK, Live(T - 1), cells={VCOL: Cell(T - 1, b"o")}))]),
        Case("partition deletion", [Partition(b"", del_=DT(T, G)), None]),
        Case("partition deletion and newer row",
             [Partition(b"", del_=DT(T, G)), part(Row(CK, Live(T + 1)))]),
        Case("range tombstone", [part(*_range(k(10), True, k(20), True, DT(T, G))), None]),
        Case("boundary, close side at G",
             [part(Marker(INCL_START, k(10), DT(T, G)),
                   Marker(EXCL_END_INCL_START, k(20), DT(T, G), DT(T, G + 1)),
                   Marker(INCL_END, k(30), DT(T, G + 1))), None]),
        Case("boundary, open side at G",
             [part(Marker(INCL_START, k(10), DT(T, G + 1)),
                   Marker(INCL_END_EXCL_START, k(20), DT(T, G + 1), DT(T, G)),
                   Marker(INCL_END, k(30), DT(T, G))), None]),
        Case("expiring cell", [part(Row(CK, cells={VCOL: Cell(T, b"e", E, 60)})), None]),
        Case("expiring complex cell",
             [part(Row(CK, complex={MCOL: (DT_LIVE, [Cell(T, b"e", E, 60, path=b"k")])})), None]),
        Case("expiring liveness", [part(Row(CK, Live(T, 60, E))), None]),
        Case("expiring liveness and cell", [part(Row(CK, Live(T, 60, E), cells={VCOL: Cell(T, b"e", E, 60)})),
                                            part(Row(CK, cells={VCOL: Cell(T - 1, b"o")}))]),
        Case("expired liveness", [part(Row(CK, Live(T, EXPIRED_TTL, G))), None]),
        Case("plain live row", [part(Row(CK, Live(T), cells={VCOL: Cell(T, b"p")})), None]),
    ]
    jobs = []
    for g in (G, G + 1):
        jobs.append((f"gc_before=G{g - G:+d}", Job(gc_before=g)))
    for ov in (T, T + 1):
        jobs.append((f"gc_before=G+1 overlap min_ts=T{ov - T:+d}", Job(gc_before=G + 1, overlap_min_ts=ov)))
    for now in (E - 1, E, E + 1):
        jobs.append((f"now=E{now - E:+d}", Job(now=now)))
    # the tombstone made from a cell that expired at E is dated E-60
    for g in (E - 60, E - 59):
        jobs.append((f"now=E gc_before=E-60{g - (E - 60):+d}", Job(now=E, gc_before=g)))
    jobs.append(("now=E gc_before=E+1", Job(now=E, gc_before=E + 1)))
    jobs.append(("never_purge", Job(now=E + 1, gc_before=E + 1, never_purge=True)))
    return Matrix("D_jobs", ROWLEVEL, 2, cases, jobs=jobs)


# ---- E: timestamp range ----
def matrix_e():
    tss = [-5, 0, 1, 2 ** 62]
    part = lambda *items, **kw: Partition(b"", items=list(items), **kw)
    cases = []
    for a, b in itertools.product(tss, repeat=2):
        cases.append(Case(f"cells {a} | {b}", [
            part(Row(CK, Live(a), cells={VCOL: Cell(a, b"l")}), Row((ck_long(20),), cells={VCOL: Cell(b, b"m")})),
            part(Row(CK, Live(b), cells={VCOL: Cell(b, b"r")}))]))
        cases.append(Case(f"row deletion {a} over cell {b}", [
            part(Row(CK, del_=DT(a, L))), part(Row(CK, cells={VCOL: Cell(b, b"r")}))]))
        # the partition-level deletion is stored as a raw long whose sign bit
        # is the format's "live" flag, so it cannot be negative; row, range
        # and complex deletions are stored as deltas and can
        cases.append(Case(f"partition deletion {max(a, 0)}, range {b}", [
            Partition(b"", del_=DT(max(a, 0), L)),
            part(Row(CK, Live(b)), *_range((ck_long(5),), True, (ck_long(15),), True, DT(b, L + 1)))]))
    for (ln, lc), (rn, rc) in itertools.product(CELL_KINDS[:13], repeat=2):
        cases.append(Case(f"tie at ts=-5 {ln} | {rn}", [
            part(Row(CK, cells={VCOL: replace(lc, ts=-5)})), part(Row(CK, cells={VCOL: replace(rc, ts=-5)}))]))
    return Matrix("E_timestamps", ROWLEVEL, 2, cases)


ALL_MATRICES = [matrix_a_skinny, matrix_a_wide, matrix_a_map, matrix_a_eight, matrix_a_counter,
                matrix_a_counter_gc, matrix_a_gc, matrix_b, matrix_c_bigint, matrix_c_composite,
                matrix_c_text, matrix_c_blocks, matrix_d, matrix_e]


# --------------------------------------------------------------------------
# reading an sstable back, and the failure reporter
# --------------------------------------------------------------------------
def read_sstable(oracle, base, scratch):
    """sstable -> {case number: Partition} through `dumpsst`. The dump is
    read with parse_gmd2: the engine's _parse_memdump builds the ctypes graph
    of a flush call, not values to compare (test_merge_edges_cpu.py checks
    that it accepts every authored table)."""
    subprocess.run([oracle, "dumpsst", base, scratch], check=True, capture_output=True)
    with open(scratch, "rb") as f:
        _, _, parts = parse_gmd2(f.read())
    return {key_case(p.key): p for p in parts}


def differing_cases(oracle, base_a, base_b, labels, scratch_dir):
    """Names the cases whose partitions differ between two sstables."""
    a = read_sstable(oracle, base_a, os.path.join(scratch_dir, "_a.memdump"))
    b = read_sstable(oracle, base_b, os.path.join(scratch_dir, "_b.memdump"))
    out = []
    for n in sorted(set(a) | set(b)):
        ca = canonical(a[n]) if n in a else None
        cb = canonical(b[n]) if n in b else None
        if ca != cb:
            lab = labels[n] if 0 <= n < len(labels) else "?"
            out.append(f"case {n} [{lab}]:\n    {base_a}: {ca}\n    {base_b}: {cb}")
    return out
