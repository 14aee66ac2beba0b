"""gpuc_validate_merkle on the GPU: the leaf hashes, leaf counts and partition
total must equal, exactly, the oracle's `validate` records for the same inputs
and parameters XORed and counted per leaf in Python (merkle_helpers). The tree
layouts are cut from the sorted record tokens T, so what each one exercises
holds by construction: one leaf for everything, thousands of mostly empty
leaves, runs that end on wave and block edges, bounds that sit on tokens,
trees with gaps between them, a token window across the trees."""
import os
import subprocess

import pytest

import merkle_helpers as mh
from conftest import ORACLE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    if mod.device_count() < 1:
        pytest.skip("no GPU")
    return mod


class Case:
    def __init__(self, d, gen, n, **params):
        os.makedirs(d)
        subprocess.run([ORACLE, "gen", d, *[f"{k}={v}" for k, v in gen.items()]],
                       check=True, capture_output=True)
        self.ins = [f"{d}/oa-{g}-big" for g in range(1, n + 1)]
        self.params = params  # now_sec / gc_before of the GPU calls
        self.vfile = f"{d}/v_cpu.bin"
        oargs = [f"now={params['now_sec']}"]
        if "gc_before" in params:
            oargs.append(f"gcbefore={params['gc_before']}")
        subprocess.run([ORACLE, "validate", self.vfile, *self.ins, *oargs],
                       check=True, capture_output=True)
        self.records = mh.read_records(self.vfile)
        self.T = [t for t, _ in self.records]

    def check(self, ca, trees, token_range=None):
        want = mh.reduce_leaves(self.records, trees, token_range)
        got = ca.validate_merkle(self.ins, trees, token_range=token_range, **self.params)
        assert got[2] == want[2], (got[2], want[2])
        assert got[1] == want[1], [(i, g, w) for i, (g, w) in
                                   enumerate(zip(got[1], want[1])) if g != w][:8]
        bad = [i for i, (g, w) in enumerate(zip(got[0], want[0])) if g != w]
        assert not bad, (len(bad), bad[:8], want[1][bad[0]])
        assert len(got[0]) == len(want[0])
        return got


@pytest.fixture(scope="module")
def S(oracle_bin, tmp_path_factory):
    """2025 merged partitions of which 329 are purged entirely: keep == 0
    groups sit inside the leaves."""
    c = Case(str(tmp_path_factory.mktemp("merkle") / "s"),
             dict(seed=5, n=3, rows=900, vlen=100, overlap=25, tomb=15, pdel=2), 3,
             now_sec=1900000000, gc_before=1900000000)
    assert len(c.T) == 1696
    assert all(a < b for a, b in zip(c.T, c.T[1:]))
    assert c.T[0] < 0 < c.T[-1]
    return c


@pytest.fixture(scope="module")
def W(oracle_bin, tmp_path_factory):
    """Wide partitions, few of them: leaves outnumber partitions."""
    c = Case(str(tmp_path_factory.mktemp("merkle") / "w"),
             dict(seed=6, n=2, rows=40, crows=60, vlen=120, rtomb=25, tomb=10, overlap=20,
                  statics=40, cktext=1), 2, now_sec=1800000000)
    assert 0 < len(c.T) < 4096
    return c


def test_one_leaf(ca, S):
    """(INT64_MIN, INT64_MAX]: every digest meets in one leaf."""
    hashes, counts, n = S.check(ca, [(mh.INT64_MIN, [mh.INT64_MAX])])
    x = 0
    for _, h in S.records:
        x ^= int.from_bytes(h, "big")
    assert hashes == [x.to_bytes(32, "big")] and counts == [1696] and n == 1696


@pytest.mark.parametrize("which", ["S", "W"])
def test_full_ring_4096_leaves(ca, S, W, which):
    """Most leaves empty, many with one partition, a split at 0 (an unsigned
    compare would misplace every negative token)."""
    c = S if which == "S" else W
    trees = mh.even_split(4096)
    assert trees[0][1][2047] in (-1, 0)
    hashes, counts, _ = c.check(ca, trees)
    assert counts.count(0) > 2048
    assert all(h == mh.ZERO for h, k in zip(hashes, counts) if k == 0)


def test_runs_cross_waves_and_blocks(ca, S):
    """Runs of 1, 63, 1, 1, 190, 1, 744 and the rest."""
    T = S.T
    rights = [T[0], T[63], T[64], T[65], T[255], T[256], T[1000], T[-1]]
    _, counts, _ = S.check(ca, [(mh.INT64_MIN, rights)])
    assert counts == [1, 63, 1, 1, 190, 1, 744, len(T) - 1001]


def test_boundary_inclusion(ca, S):
    """The tree's left token is excluded, a leaf's right token is included,
    and a leaf between two adjacent tokens is empty."""
    T = S.T
    assert T[21] > T[20] + 1
    hashes, counts, n = S.check(ca, [(T[10], [T[20], T[20] + 1, T[30]])])
    assert counts == [10, 0, 10] and n == 20
    assert hashes[1] == mh.ZERO


def _gapped_trees(T):
    return [(T[99], [T[120], T[150], T[151], T[200], T[250], T[298], T[299]]),
            (T[499], [T[501]]),
            (T[1499], [T[1600], T[-1], mh.INT64_MAX])]


def test_trees_with_gaps(ca, S):
    """Partitions before, between and after the trees are in no leaf and not
    in n_partitions."""
    T = S.T
    _, counts, n = S.check(ca, _gapped_trees(T))
    assert n == 200 + 2 + (len(T) - 1500)
    assert counts[7] == 2 and counts[-1] == 0


def test_token_range_intersects(ca, S):
    T = S.T
    _, _, n = S.check(ca, mh.even_split(4096), token_range=(T[300], T[1200]))
    assert n == 901
    trees = _gapped_trees(T)
    hull = (trees[0][0] + 1, trees[-1][1][-1])
    assert S.check(ca, trees, token_range=hull) == S.check(ca, trees)


def test_null_outputs(ca, S):
    trees = _gapped_trees(S.T)
    want = mh.reduce_leaves(S.records, trees)
    for kw in (dict(want_leaf_partitions=False), dict(want_n_partitions=False),
               dict(want_leaf_partitions=False, want_n_partitions=False)):
        hashes, counts, n = ca.validate_merkle(S.ins, trees, **S.params, **kw)
        assert hashes == want[0]
        assert counts == (None if "want_leaf_partitions" in kw else want[1])
        assert n == (None if "want_n_partitions" in kw else want[2])


def test_validate_unchanged_after_merkle(ca, S, tmp_path):
    """gpuc_validate still writes the oracle's file, right after a Merkle call
    on the same thread."""
    S.check(ca, _gapped_trees(S.T))
    out = str(tmp_path / "v_gpu.bin")
    n = ca.validate(S.ins, out, **S.params)
    assert n == 1696
    assert open(out, "rb").read() == open(S.vfile, "rb").read()
    S.check(ca, [(mh.INT64_MIN, [mh.INT64_MAX])])
