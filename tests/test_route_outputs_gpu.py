"""Routed outputs (gpuc_compact_routed): one compaction written into several
sstables chosen by token range.

The reference of every output is the oracle's compaction of the same inputs
restricted to that output's ranges (`ranges=`; the default output is
`invertranges=1` over the ranges of all other outputs), one oracle run per
output, compared byte for byte in every component file. An output the oracle
leaves empty must not be written at all. The check itself is in
route_helpers.route_and_check."""
import ctypes
import glob
import os

import pytest

import chunk_helpers as ch
import header_union_tables as hu
from multi_cpx_helpers import COMPONENTS, assert_same_components
from route_helpers import gen as _gen, kept_tokens as _kept_tokens
from route_helpers import oracle_compact as _oracle_compact, route_and_check as _route_and_check
from route_helpers import rs as _rs

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
CANCELLED = 7


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


@pytest.fixture(scope="module")
def three(oracle_bin, tmp_path_factory):
    """The anticompaction inputs, their kept tokens and the unrouted oracle
    compaction; written once, never modified."""
    d = str(tmp_path_factory.mktemp("route_three"))
    ins = _gen(d, "seed=141 n=3 rows=2000 vlen=250 overlap=30 tomb=10")
    whole = _oracle_compact(f"{d}/whole/oa-90-big", ins)
    return ins, _kept_tokens(ins), whole, f"{d}/whole/oa-90-big"


# ---- 1. three-way anticompaction ------------------------------------------------
def test_three_way_anticompaction(ca, three, tmp_path):
    ins, _, whole, _ = three
    d = str(tmp_path)
    full = [(-2 ** 62, -2 ** 61), (0, 2 ** 60)]
    trans = [(2 ** 61, 2 ** 62)]
    bases = [f"{d}/oa-{g}-big" for g in (10, 11, 12)]
    r = ca.anticompact(ins, *bases, full, trans)
    cpu = [f"{d}/cpu/oa-{g}-big" for g in (10, 11, 12)]
    want = [_oracle_compact(cpu[0], ins, _rs(full)),
            _oracle_compact(cpu[1], ins, _rs(trans)),
            _oracle_compact(cpu[2], ins, _rs(sorted(full + trans)), "invertranges=1")]
    assert [w["partitions_out"] for w in want] == [819, 552, 2829]
    assert whole["partitions_out"] == 4200
    assert r["n_outputs"] == 3
    assert [o["partitions"] for o in r["outputs"]] == [819, 552, 2829]
    assert sum(o["partitions"] for o in r["outputs"]) == r["partitions_out"] == 4200
    assert r["partitions_in"] == whole["partitions_in"]
    for g, c in zip(bases, cpu):
        assert_same_components(g, c, COMPONENTS + ["TOC.txt"])


# ---- 2. bounds -----------------------------------------------------------------
def test_bounds(ca, three, tmp_path):
    """About 700 ranges whose ends ARE partition tokens, with the neighbouring
    tokens one step outside; single-token ranges; both extremes; one range
    that no token falls in."""
    ins, T, whole, _ = three
    assert len(T) == whole["partitions_out"]  # no two partitions share a token here
    ranges = []
    for i in range(len(T) // 12):
        ranges.append((T[12 * i + 2], T[12 * i + 7], i % 2))
        ranges.append((T[12 * i + 9], T[12 * i + 9], 2))
    ranges[0] = (INT64_MIN, ranges[0][1], ranges[0][2])
    ranges[-1] = (ranges[-1][0], INT64_MAX, ranges[-1][2])
    # a range strictly between two adjacent tokens that no other range covers
    i = next(i for i in range(5, len(T) // 12 - 1) if T[12 * i + 11] - T[12 * i + 10] >= 2)
    ranges.append((T[12 * i + 10] + 1, T[12 * i + 11] - 1, 4))
    ranges.sort()
    assert 690 <= len(ranges) <= 710
    r, want = _route_and_check(ca, ins, str(tmp_path), ranges, 3, 5)
    assert want[4] == 0 and r["outputs"][4]["written"] == 0
    assert all(w > 0 for w in want[:4]) and sum(want) == whole["partitions_out"]
    assert r["n_outputs"] == 4


# ---- 3. drop -------------------------------------------------------------------
def test_drop(ca, three, tmp_path):
    ins, T, whole, _ = three
    ranges = [(T[100], T[400], 0), (T[401], T[500], -1), (T[2000], T[2000], 0),
              (T[3000] + 1, T[3500], 0)]
    r, want = _route_and_check(ca, ins, str(tmp_path), ranges, -1, 1)
    assert want == [301 + 1 + 500]
    assert r["partitions_out"] == want[0] and r["n_outputs"] == 1
    assert r["partitions_in"] == whole["partitions_in"]


def test_everything_dropped(ca, three, tmp_path):
    """No output receives anything: nothing is written, and that is no error."""
    ins, T, _, _ = three
    d = str(tmp_path)
    r = ca.compact_routed(ins, [f"{d}/oa-10-big", f"{d}/oa-11-big"],
                          [(T[0] + 1, T[1] - 1, 0)], -1)
    assert r["n_outputs"] == 0 and r["partitions_out"] == 0
    assert [o["written"] for o in r["outputs"]] == [0, 0]
    assert not glob.glob(f"{d}/oa-1*")


# ---- 4. degenerate -------------------------------------------------------------
def test_one_output_no_ranges(ca, three, tmp_path):
    ins, _, whole, whole_base = three
    d = str(tmp_path)
    r, want = _route_and_check(ca, ins, d, [], 0, 1)
    assert want == [whole["partitions_out"]]
    os.makedirs(f"{d}/plain")
    rc = ca.compact(ins, f"{d}/plain/oa-10-big")
    assert_same_components(f"{d}/gpu/oa-10-big", f"{d}/plain/oa-10-big", COMPONENTS + ["TOC.txt"])
    assert_same_components(f"{d}/gpu/oa-10-big", whole_base, COMPONENTS + ["TOC.txt"])
    for k in ("partitions_in", "partitions_out", "rows_in", "rows_out", "merged_counts",
              "output_compressed_bytes", "output_uncompressed_bytes", "n_outputs"):
        assert r[k] == rc[k], k


# ---- 5. after purge ------------------------------------------------------------
def test_after_purge(ca, oracle_bin, tmp_path):
    """Partitions that the purge removes entirely appear in neither output."""
    d = str(tmp_path)
    ins = _gen(d, "seed=77 n=3 rows=150 crows=4 vlen=120 overlap=40 tomb=55 rtomb=40 "
                  "statics=30 pdel=25 ttl=30")
    now = 2000000000
    ov = (-2 ** 62, 0, 1)
    oargs = [f"now={now}", f"gcbefore={now}", f"ov={ov[0]}:{ov[1]}:{ov[2]}"]
    unpurged = _oracle_compact(f"{d}/ref/oa-80-big", ins)
    purged = _oracle_compact(f"{d}/ref/oa-81-big", ins, *oargs)
    assert 0 < purged["partitions_out"] < unpurged["partitions_out"]
    T = _kept_tokens(ins)  # purged partitions included: they must not come back
    q = len(T) // 4
    ranges = [(INT64_MIN, T[q], 0), (T[q + 1], T[2 * q], 1), (T[3 * q], T[3 * q + 20], 0)]
    r, want = _route_and_check(ca, ins, d, ranges, 1, 2, oracle_args=oargs,
                               now_sec=now, gc_before=now, overlaps=[ov])
    assert sum(want) == purged["partitions_out"] and min(want) > 0
    assert r["rows_out"] == purged["rows_out"]


# ---- 6. one small case per mode --------------------------------------------------
SMALL = "n=2 rows=400 vlen=120 overlap=30 tomb=10"


def _thirds(T):
    a, b = len(T) // 3, 2 * len(T) // 3
    return [(T[5], T[a], 0), (T[a + 1], T[a + 1], 1), (T[b], INT64_MAX, 1)]


@pytest.mark.parametrize("extra", ["bti=1", "snappy=1", "cpx=30 cpxdel=10", "counter=1"],
                         ids=["da", "snappy", "complex", "counter"])
def test_generated_shapes(ca, oracle_bin, tmp_path, extra):
    d = str(tmp_path)
    ins = _gen(d, f"seed=151 {SMALL} {extra}")
    r, want = _route_and_check(ca, ins, d, _thirds(_kept_tokens(ins)), 2, 3,
                               bti=extra == "bti=1")
    assert min(want) > 0 and r["n_outputs"] == 3


def test_output_chunk_length(ca, oracle_bin, tmp_path):
    """The oracle writes at the chunk length of its first input."""
    d = str(tmp_path)
    ins = _gen(d, f"seed=152 {SMALL}")
    os.makedirs(f"{d}/tmp4k")
    first4k = ch.rechunk(ins[0], f"{d}/in4k/oa-1-big", 4096, f"{d}/tmp4k")
    r, want = _route_and_check(ca, ins, d, _thirds(_kept_tokens(ins)), 2, 3,
                               oracle_ins=[first4k, ins[1]], output_chunk_length=4096)
    assert min(want) > 0
    assert ch.chunk_length_of(f"{d}/gpu/oa-11-big") == 4096


def test_token_range_intersects(ca, oracle_bin, tmp_path):
    d = str(tmp_path)
    ins = _gen(d, f"seed=153 {SMALL}")
    T = _kept_tokens(ins)
    a, b = len(T) // 3, 2 * len(T) // 3
    tr = (T[a - 40], T[b + 40])  # cuts into the first and the last range
    r, want = _route_and_check(ca, ins, d, _thirds(T), 2, 3,
                               oracle_args=[f"shard={tr[0]}:{tr[1]}"], token_range=tr)
    # output 0: T[a-40..a]; output 1: T[a+1] and T[b..b+40]; default: T[a+2..b-1]
    assert want == [41, 42, b - a - 2]


def test_tombstone_sources_cell_gc(ca, oracle_bin, tmp_path):
    d = str(tmp_path)
    ins = _gen(d, f"seed=154 {SMALL}")
    srcs = _gen(f"{d}/src", "seed=154 n=2 rows=300 vlen=100 overlap=40 tomb=40 pdel=10 "
                            "ts0=1700000500000000")
    r, want = _route_and_check(ca, ins, d, _thirds(_kept_tokens(ins)), 2, 3,
                               oracle_args=["tombsrc=" + ",".join(srcs), "cellgc=1"],
                               tombstone_sources=srcs, cell_level_gc=True)
    assert min(want) > 0


def test_header_union_pair(ca, oracle_bin, tmp_path):
    """Inputs with different headers: the engine routes the narrow inputs, the
    oracle compacts their wide twins."""
    d = str(tmp_path)
    uc = hu.u8()
    narrow, wide, _ = uc.write(oracle_bin, f"{d}/in")
    T = _kept_tokens(wide)
    assert len(T) >= 3
    m = len(T) // 2
    ranges = [(INT64_MIN, T[m - 1], 0), (T[m], T[m], 1)]
    r, want = _route_and_check(ca, narrow, d, ranges, 2, 3, oracle_ins=wide,
                               bti=bool(uc.matrix.schema.bti))
    assert want[0] > 0 and want[1] > 0 and sum(want) == r["partitions_out"]


# ---- 7. cancel -------------------------------------------------------------------
def test_cancel(ca, three, tmp_path):
    ins, T, _, _ = three
    d = str(tmp_path)
    flag = ctypes.c_int32(1)
    with pytest.raises(ca.GpuCompactError, match=rf"rc={CANCELLED}\b"):
        ca.compact_routed(ins, [f"{d}/oa-10-big", f"{d}/oa-11-big"], [(T[0], T[2000], 0)], 1,
                          cancel_flag=flag)
