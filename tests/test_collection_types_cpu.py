"""Set and typed-key map columns: the host-side parser, resolver and path
comparator, and the soundness of the reference route of
test_collection_types_gpu.py (collection_tables.py). Runs without a GPU."""
import itertools
import json
import os
import subprocess

import pytest

import authored_tables as at
import collection_tables as ct
import desc_tables as dt
from conftest import REPO
from multi_cpx_helpers import BTI_COMPONENTS, COMPONENTS, assert_same_components

NATIVE = os.path.join(REPO, "tests", "native", "collection_types_test.cpp")
CASES = dict(ct.ALL_CASES, set_int_edges_da=lambda: ct.set_int_edges(bti=1))


def _all8(case):
    return (BTI_COMPONENTS if case.schema.bti else COMPONENTS) + ["TOC.txt"]


@pytest.fixture(scope="module")
def tables(oracle_bin, tmp_path_factory):
    """case -> (CollCase, real bases, mirror bases), written once."""
    root = tmp_path_factory.mktemp("coll_cpu")
    out = {}
    for name, mk in CASES.items():
        c = mk()
        real, mirror = c.write(oracle_bin, str(root / name))
        out[name] = (c, real, mirror)
    return out


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]],
                         ids=["plain", "sanitized"])
def test_native(tmp_path, flags):
    """Parser on every accepted and refused string, masks and widths from
    resolve_schema, the union order, and cell_path_cmp (the function the
    kernels call) against plain integer compares; once more as its own
    sanitized executable."""
    exe = str(tmp_path / "collection_types_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, NATIVE, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "collection_types_test OK" in r.stdout


@pytest.mark.parametrize("pack,width", [(ct.i4, 4), (ct.i8, 8)])
def test_mirror_preserves_order(pack, width):
    """Signed order of MIN, -1, 0, 1, MAX == unsigned byte order of their
    mirrors; the mirror keeps the length and is its own inverse."""
    vals = ct.edges(width)
    for a, b in itertools.product(vals, repeat=2):
        ma, mb = ct.mirror_path(pack(a)), ct.mirror_path(pack(b))
        assert (ma < mb) == (a < b) and (ma == mb) == (a == b)
        assert len(ma) == width and ct.mirror_path(ma) == pack(a)
    # and the unsigned order of the real bytes is NOT the signed order
    assert sorted(vals, key=pack) != vals


@pytest.mark.parametrize("name", sorted(CASES))
def test_real_tables_are_in_real_path_order(name):
    c = CASES[name]()
    for parts in c.inputs():
        ct.paths_in_real_order(c, parts)
    # the mirror is in the oracle's (unsigned) order
    for parts in c.inputs():
        for p in c.mirror(parts):
            for it in p.items:
                for _, cs in getattr(it, "complex", {}).values():
                    ps = [x.path for x in cs]
                    assert ps == sorted(ps) and len(set(ps)) == len(ps)


def test_signed_cases_differ_from_byte_order():
    """set_int_edges holds rows whose real order is not the byte order: a
    build that keeps the byte compare cannot pass it."""
    c = ct.set_int_edges()
    n = 0
    for parts in c.inputs():
        for p in parts:
            for it in p.items:
                for _, cs in it.complex.values():
                    ps = [x.path for x in cs]
                    n += ps != sorted(ps)
    assert n >= 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_rewrite_round_trip(tables, oracle_bin, tmp_path, name):
    """The rewrite puts the real strings into the header, and rewriting back
    restores the bytes fromdump wrote."""
    c, real, _ = tables[name]
    for i, parts in enumerate(c.inputs()):
        hdr = c.header_of(i)
        ns, nparts = ct.hu.project(c.schema, parts, *hdr)
        base = str(tmp_path / f"b{i}" / c.stem(1))
        ct.fromdump(oracle_bin, ct.gmd2(ns, nparts), base)
        data = open(real[i] + "-Statistics.db", "rb").read()
        cols = dt.statistics_types(data)[2]
        for nm in hdr[0] + hdr[1]:
            assert cols[nm] == c.types.get(nm, c.base_type(nm))
        ck = [dt.TYPE_NAMES[t] for t in ns.ck_types]
        back = dt.rewrite_statistics(data, ck, ck, c.renames(hdr[0] + hdr[1], to_real=False))
        assert back == open(base + "-Statistics.db", "rb").read()
        for comp in _all8(c):
            if comp != "Statistics.db":
                assert open(f"{real[i]}-{comp}", "rb").read() == open(f"{base}-{comp}", "rb").read()


def _compact(oracle, out, inputs, *args):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([oracle, "compact", out, *inputs, *args], check=True, capture_output=True,
                       text=True)
    return json.loads(r.stdout.splitlines()[-1])


def _oracle_outputs(c, mirror, oracle, d):
    """(label, job, output base or None) per job of the case, over the mirrors."""
    n_data = c.matrix.n_inputs
    for j, (label, job) in enumerate(c.matrix.jobs):
        out = f"{d}/o{j}/{c.stem(50)}"
        args = list(job.oracle_args())
        if c.matrix.has_tomb_source:
            args.append(f"tombsrc={mirror[n_data]}")
        res = _compact(oracle, out, mirror[:n_data], *args)
        yield j, label, job, out if res["partitions_out"] else None


@pytest.mark.parametrize("name", sorted(CASES))
def test_fromdump_of_dumpsst_reproduces_the_oracle_output(tables, oracle_bin, tmp_path, name):
    """fromdump(dumpsst(O)) == O in all eight components for the oracle's
    compaction O of the mirrors under every job: the route that carries the
    expected bytes back adds nothing of its own (long values included)."""
    c, _, mirror = tables[name]
    d = str(tmp_path)
    seen = 0
    for j, label, job, out in _oracle_outputs(c, mirror, oracle_bin, d):
        if out is None:
            continue
        schema, stats, parts = ct.read_dump(oracle_bin, out, f"{d}/o{j}/dump.memdump")
        back = f"{d}/b{j}/{c.stem(50)}"
        ct.fromdump(oracle_bin, ct.gmd2(schema, ct.narrow_values(parts), stats), back)
        assert_same_components(back, out, _all8(c))
        seen += 1
    assert seen


@pytest.mark.parametrize("name", ct.PREDICTED)
def test_python_model_agrees_with_the_expected_content(tables, oracle_bin, tmp_path, name):
    """authored_tables' merge and purge rules, run over the mirror (where its
    path sort is the real comparator's) and mapped back, give the content of
    the expected real sstable, case by case and job by job."""
    c, _, mirror = tables[name]
    d = str(tmp_path)
    mm = c.mirror_matrix()
    for j, label, job, out in _oracle_outputs(c, mirror, oracle_bin, d):
        predicted = mm.predict(job)
        if out is None:
            assert not predicted, label
            continue
        want = f"{d}/want{j}/{c.stem(50)}"
        ct.expected(oracle_bin, c, out, want)
        ct.to_base(c, want, f"{d}/wantb{j}/{c.stem(50)}")
        _, _, parts = ct.read_dump(oracle_bin, f"{d}/wantb{j}/{c.stem(50)}", f"{d}/want{j}.memdump")
        got = {at.key_case(p.key): p for p in ct.narrow_values(parts)}
        assert sorted(got) == sorted(predicted), label
        for n in got:
            ct.paths_in_real_order(c, [got[n]])
            model = c.unmirror([predicted[n]])[0]
            assert at.canonical(got[n]) == at.canonical(model), (label, c.matrix.labels[n])
