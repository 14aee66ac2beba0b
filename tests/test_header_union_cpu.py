"""CPU side of the header-union tests (header_union_tables.py): the authored
cases are what they claim to be, the narrow and wide twins hold the same
table, the oracle's compaction of the wide twins is a sound reference (it
round-trips them, and its output is what the reference rules predict), and
resolve_job_schema maps and rejects headers as documented."""
import os
import subprocess

import pytest

import authored_tables as at
import header_union_tables as hu
from conftest import REPO

PURGING = at.Job(now=hu.PURGE_NOW, gc_before=hu.PURGE_NOW)


@pytest.fixture(scope="module")
def twins(oracle_bin, tmp_path_factory):
    """case -> (UnionCase, narrow bases, wide bases, narrow schemas), written once."""
    root = tmp_path_factory.mktemp("header_union")
    out = {}
    for name, mk in list(hu.ALL_CASES.items()) + [("GC", hu.gc_case)]:
        uc = mk()
        out[name] = (uc, *uc.write(oracle_bin, str(root / name)))
    return out


@pytest.mark.parametrize("name", sorted(hu.ALL_CASES) + ["GC"])
def test_preconditions(name):
    uc = (hu.gc_case if name == "GC" else hu.ALL_CASES[name])()
    schema, inputs = uc.matrix.schema, uc.inputs()
    headers = [tuple(map(tuple, uc.header_of(i))) for i in range(len(inputs))]
    assert len(set(headers)) >= 2, "at least two inputs have different headers"
    n_data = uc.matrix.n_inputs
    for what, sel, cols in (("regular", 0, schema.regular_cols), ("static", 1, schema.static_cols)):
        for nm, _ in cols:
            # a union column comes from a compacting input's header
            have = [nm in h[sel] for h in headers[:n_data]]
            assert any(have), f"{what} column {nm} is in no input header"
            if uc.all_columns_partial:
                assert not all(have), f"{what} column {nm} is in every input header"
    for i, parts in enumerate(inputs):
        used = tuple(map(tuple, hu.used_columns(schema, parts)))
        for sel in (0, 1):
            assert set(used[sel]) <= set(headers[i][sel]), f"input {i} uses a column outside its header"
            if not uc.may_hold_unused:
                assert used[sel] == headers[i][sel], f"input {i}: header holds an unused column"


def test_u8_sizes():
    uc = hu.u8()
    ins = uc.inputs()
    assert tuple(len(p) for p in ins) == hu.U8_SIZES
    counts = [sum(len(p.items) for p in parts) for parts in ins]
    assert max(counts) > 256, counts
    assert all(1 <= len(p.items) <= 4 for parts in ins for p in parts)
    keys = [set(p.key for p in parts) for parts in ins]
    for other in keys[1:]:
        shared = len(other & keys[0]) / len(other)
        assert 0.4 <= shared <= 0.6, shared
    # a source boundary inside a 256-thread block of the parse kernels
    assert len(ins[0]) % 256 and (len(ins[0]) + len(ins[1])) % 256


def _dump(oracle, base, scratch):
    subprocess.run([oracle, "dumpsst", base, scratch], check=True, capture_output=True)
    with open(scratch, "rb") as f:
        return at.parse_gmd2(f.read())


@pytest.mark.parametrize("name", sorted(hu.ALL_CASES) + ["GC"])
def test_twins_hold_the_same_table(twins, oracle_bin, tmp_path, name):
    uc, narrow, wide, schemas = twins[name]
    assert len({tuple(s.regular_cols) + tuple(s.static_cols) for s in schemas}) >= 2
    for i, (nb, wb) in enumerate(zip(narrow, wide)):
        ns, _, nparts = _dump(oracle_bin, nb, str(tmp_path / "n.memdump"))
        ws, _, wparts = _dump(oracle_bin, wb, str(tmp_path / "w.memdump"))
        assert ns.regular_cols == schemas[i].regular_cols and ns.static_cols == schemas[i].static_cols
        assert ws.regular_cols == uc.matrix.schema.regular_cols
        assert ws.static_cols == uc.matrix.schema.static_cols
        _, projected = hu.project(ws, wparts, [nm for nm, _ in ns.regular_cols],
                                  [nm for nm, _ in ns.static_cols])
        assert [p.key for p in nparts] == [p.key for p in projected]
        assert len(nparts) == len(uc.inputs()[i])
        for a, b in zip(nparts, projected):
            assert at.canonical(a) == at.canonical(b), f"{name} input {i} case {at.key_case(a.key)}"


@pytest.mark.parametrize("name", sorted(hu.ALL_CASES))
def test_oracle_is_the_reference(twins, oracle_bin, tmp_path, name):
    """The oracle reads each wide twin back as written, compacts them plain
    and purging, and for the cases inside the Python model its output is what
    the reference rules predict on the union schema. It cannot compact the
    narrow inputs (it merges cells by column index, and rows of different
    widths are outside what it was written for: what it does with them is
    not defined, so no test runs it on them), which is why the wide twins
    are the reference."""
    uc, narrow, wide, _ = twins[name]
    for wb in wide:
        subprocess.run([oracle_bin, "roundtrip", wb], check=True, capture_output=True)
    for tag, job in (("plain", at.Job()), ("purge", PURGING)):
        out = str(tmp_path / tag / "oa-50-big")
        os.makedirs(os.path.dirname(out))
        subprocess.run([oracle_bin, "compact", out, *wide, *job.oracle_args()], check=True,
                       capture_output=True)
        if name not in hu.PREDICTED:
            continue
        got = at.read_sstable(oracle_bin, out, str(tmp_path / "out.memdump"))
        want = uc.matrix.predict(job)
        assert sorted(got) == sorted(want), f"{name} [{tag}]: partitions"
        for n in want:
            assert at.canonical(got[n]) == at.canonical(want[n]), \
                f"{name} [{tag}] case {n} [{uc.matrix.labels[n]}]"


def test_resolve_job_schema_native(twins, tmp_path):
    """tests/native/header_union_test.cpp over the Statistics.db files of the
    U1 and U4 narrow inputs: union order, every map entry and per-source
    count, the identity case and each rejection. Built with the address and
    undefined-behaviour sanitizers."""
    exe = str(tmp_path / "header_union_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tests/native/header_union_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    stats = [b + "-Statistics.db" for b in twins["U1"][1] + twins["U4"][1]]
    r = subprocess.run([exe, *stats], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
