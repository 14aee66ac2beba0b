"""GPU tests for compact(max_output_bytes=...): a compaction whose output is
cut into several sstables at an on-disk size, the way MaxSSTableSizeWriter
cuts it. Every output is compared byte for byte, every component, with the
oracle's own sstable of that output's token range; the cut points come from
tests/native/size_split_ref.cpp (size_split_helpers.split_ref), and those of
plan_size_cuts from liblz4 / libsnappy in Python."""
import ctypes
import glob
import os

import pytest

import chunk_helpers as ch
from multi_cpx_helpers import widen_tool, widened  # noqa: F401  (fixtures)
from size_split_helpers import CASES, size_split_tool, split_ref  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


def _assert_equal(got_base, want_base, comps):
    for c in comps:
        with open(f"{got_base}-{c}", "rb") as f:
            got = f.read()
        with open(f"{want_base}-{c}", "rb") as f:
            want = f.read()
        if got != want:
            n = min(len(got), len(want))
            i = next((j for j in range(n) if got[j] != want[j]), n)
            raise AssertionError(f"{os.path.basename(got_base)} {c}: got {len(got)} bytes, "
                                 f"want {len(want)}, first diff at {i}")


def _out_base(d, ref, k):
    return f"{d}/{ref['name'][0]}-{500 + k}-{ref['name'][2]}"


# ---- (a)-(g): every output equals the oracle's sstable of its token range ----
@pytest.mark.parametrize("case", sorted(CASES))
def test_outputs_match_oracle(ca, split_ref, tmp_path, case):
    ref = split_ref[case]
    d = str(tmp_path)
    r = ca.compact(ref["inputs"], _out_base(d, ref, 0), max_output_bytes=ref["cap"], **ref["gpu"])
    want = ref["outputs"]
    print(case, "outputs", r["n_outputs"], "want", len(want))
    assert r["n_outputs"] == len(want)
    assert r["partitions_out"] == ref["r"]["partitions_out"]
    assert r["rows_out"] == ref["r"]["rows_out"]
    for k, o in enumerate(want):
        _assert_equal(_out_base(d, ref, k), o["base"], ref["comps"])
        ca.verify(_out_base(d, ref, k))
    # nothing past the last output
    assert not glob.glob(_out_base(d, ref, len(want)) + "-*")


def test_cap_above_everything_is_the_unsplit_run(ca, split_ref, tmp_path):
    ref = split_ref["a_nocut"]
    d = str(tmp_path)
    os.makedirs(d + "/s"), os.makedirs(d + "/u")
    rs = ca.compact(ref["inputs"], _out_base(d + "/s", ref, 0), max_output_bytes=ref["cap"])
    ru = ca.compact(ref["inputs"], _out_base(d + "/u", ref, 0))
    assert rs["n_outputs"] == 1 and ru["n_outputs"] == 1
    _assert_equal(_out_base(d + "/s", ref, 0), _out_base(d + "/u", ref, 0), ref["comps"])
    assert rs["merged_counts"] == ru["merged_counts"]
    assert rs["output_compressed_bytes"] == ru["output_compressed_bytes"]


def test_n_outputs_of_the_existing_modes(ca, split_ref, tmp_path):
    ref = split_ref["a"]
    r = ca.compact(ref["inputs"], _out_base(str(tmp_path), ref, 0), n_output_shards=3)
    assert r["n_outputs"] == 3


# ---- (h) refusals -------------------------------------------------------------
def test_refused_with_shards_and_by_validate(ca, split_ref, tmp_path):
    ref = split_ref["a"]
    d = str(tmp_path)
    with pytest.raises(ca.GpuCompactError, match=r"rc=3.*max_output_bytes"):
        ca.compact(ref["inputs"], _out_base(d, ref, 0), max_output_bytes=6000, n_output_shards=2)
    with pytest.raises(ca.GpuCompactError, match=r"rc=3"):
        ca.validate(ref["inputs"], d + "/digests", max_output_bytes=6000)
    # refused before any input byte is read: missing inputs are not even opened
    with pytest.raises(ca.GpuCompactError, match=r"rc=3.*max_output_bytes"):
        ca.compact([d + "/missing/oa-1-big"], _out_base(d, ref, 0), max_output_bytes=6000,
                   n_output_shards=2)
    assert os.listdir(d) == []


# ---- (i) cancellation ---------------------------------------------------------
def test_cancelled_before_the_call(ca, split_ref, tmp_path):
    ref = split_ref["a"]
    flag = ctypes.c_int32(1)
    with pytest.raises(ca.GpuCompactError, match=r"rc=7.*cancel"):
        ca.compact(ref["inputs"], _out_base(str(tmp_path), ref, 0), max_output_bytes=6000,
                   cancel_flag=ctypes.pointer(flag))


# ---- (j) plan_size_cuts against liblz4 / libsnappy ---------------------------
def _sizes(L):
    """40 chunks of partitions: ends on exact multiples of L, on k*L - 1 and
    k*L + 1, runs of equal ends (dropped partitions), one partition spanning
    five chunks, a final partial chunk and dropped partitions after it. Sizes
    of exactly L keep producing
    exact multiples after every cut, wherever the cut moved the origin."""
    s = [L // 2, L - L // 2, 0, 1, L - 1, 0, 0, L + 1, L - 1, 5 * L, L, L, L - 1, 1, 2 * L,
         L + 1, L - 1, 0, L, L, L, L, 2 * L - 1, 1, L, L]
    total = 39 * L + L // 3
    while sum(s) + L <= 39 * L:
        s.append(L)
    s.append(total - sum(s))
    s += [0, 0]  # dropped partitions after the last byte
    assert all(x >= 0 for x in s) and sum(s) == total
    return s


def _ref_cuts(data, ends, L, payload, cap, lazy=True):
    """the rule, over CPU-library chunk payloads"""
    cuts, start, held, count, last = [], 0, 0, 0, None
    cache = {}

    def est(e):
        flushed = ((e - 1) // L if e else 0) if lazy else e // L
        tot = 0
        for c in range(flushed):
            if (start, c) not in cache:
                cache[(start, c)] = len(payload(data[start + c * L:start + (c + 1) * L])) + 4
            tot += cache[(start, c)]
        return tot

    prev = 0
    for i, e in enumerate(ends):
        size, prev = e - prev, e
        if size == 0:
            continue  # dropped: no bytes, never carries a cut
        if count > 0 and est(held) > cap:
            cuts.append(last)
            start, held, count = e - size, 0, 0
        held += size
        count += 1
        last = i
    return cuts


@pytest.mark.parametrize("L", [1024, 16384])
@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_plan_size_cuts(ca, codec, L):
    if codec == "snappy":
        lib = ch.snappy()
        if lib is None:
            pytest.skip("libsnappy not present (case (c) still covers the Snappy writer)")
        payload = lambda c: ch.snappy_payload(c, lib)  # noqa: E731
    else:
        payload = ch.lz4_payload
    sizes = _sizes(L)
    ends, acc = [], 0
    for s in sizes:
        acc += s
        ends.append(acc)
    for mode in (0, 1, 3):
        data = ch.content(mode, acc)
        c0 = len(payload(data[:L])) + 4
        caps = [1, c0, 2 * c0 + 2, 5 * c0, 1 << 40]
        want = {cap: _ref_cuts(data, ends, L, payload, cap) for cap in caps}
        # the lazy flush must matter somewhere, or (E-1)/L is not under test
        assert any(want[cap] != _ref_cuts(data, ends, L, payload, cap, lazy=False)
                   for cap in caps), (codec, L, mode)
        assert want[1 << 40] == [] and len(want[1]) >= 10
        for cap in caps:
            got = ca.plan_size_cuts(data, ends, L, codec == "snappy", cap)
            assert got == want[cap], (codec, L, mode, cap, got[:8], want[cap][:8])
        assert ca.plan_size_cuts(data[:ends[0]], ends[:1], L, codec == "snappy", 1) == []
    assert ca.plan_size_cuts(b"", [], L, codec == "snappy", 1) == []
    assert ca.plan_size_cuts(b"", [0, 0], L, codec == "snappy", 1) == []
