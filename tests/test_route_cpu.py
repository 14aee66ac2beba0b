"""CPU tests of the routed-output entry point (gpuc_compact_routed): the
host-only spec code of cassandra_amd/csrc/route_spec.h in a native test built
with plain g++ (no HIP), every refusal the real library makes before it probes
a device (malformed routing tables and the job modes routing does not take),
the Python anticompact() range check, and the pure-C command line tool."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "native", "route_spec_test.cpp")
CLI = os.path.join(REPO, "tools", "gpuc_cli.c")
UNSUPPORTED, NO_GPU = 3, 4
INS = ["/nonexistent/oa-1-big"]


def test_route_spec_native(tmp_path):
    """Lookup against a linear scan on tables of 0, 1, 2 and about 1000
    ranges, and the spec check on every malformed spec."""
    binp = str(tmp_path / "route_spec_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", binp, SRC],
                   check=True)
    r = subprocess.run([binp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith("OK route_spec"), r.stdout
    sizes = [int(m) for m in re.findall(r"^table \S+: (\d+) ranges", r.stdout, re.M)]
    assert sorted(set(sizes))[:3] == [0, 1, 2] and max(sizes) >= 1000, r.stdout
    assert "17 malformed specs refused" in r.stdout, r.stdout


@pytest.fixture(scope="module")
def ca(product_lib):
    import cassandra_amd as mod
    return mod


def _refused(ca, match, raw_spec=None, **kw):
    """The call must fail with GPUC_ERR_UNSUPPORTED and name `match`."""
    with pytest.raises(ca.GpuCompactError) as ei:
        if raw_spec is None:
            ca.compact_routed(INS, ["/o/a", "/o/b"], [(0, 10, 0), (20, 30, 1)], 1, **kw)
        else:
            ca.compact_routed(INS, None, None, None, raw_spec=raw_spec, **kw)
    msg = str(ei.value)
    assert f"rc={UNSUPPORTED}:" in msg, msg
    assert match in msg, msg


B3 = ["/o/a", "/o/b", "/o/c"]
LO, HI, OUT = [0, 20, 40], [10, 30, 50], [0, 1, -1]
# (n_outputs, output_bases, n_ranges, range_lo, range_hi, range_output,
# default_output) handed over unchecked, and what the message must name
BAD_SPECS = {
    "null_bases": ((3, None, 3, LO, HI, OUT, 2), "output_bases"),
    "null_range_lo": ((3, B3, 3, None, HI, OUT, 2), "range_lo"),
    "null_range_hi": ((3, B3, 3, LO, None, OUT, 2), "range_hi"),
    "null_range_output": ((3, B3, 3, LO, HI, None, 2), "range_output"),
    "no_outputs": ((0, B3, 3, LO, HI, OUT, 2), "n_outputs"),
    "too_many_outputs": ((33, B3, 3, LO, HI, OUT, 2), "33"),
    "null_base": ((3, ["/o/a", None, "/o/c"], 3, LO, HI, OUT, 2), "base 1"),
    "empty_base": ((3, ["/o/a", "/o/b", ""], 3, LO, HI, OUT, 2), "base 2"),
    "equal_bases": ((3, ["/o/a", "/o/b", "/o/a"], 3, LO, HI, OUT, 2), "0 and 2"),
    "lo_above_hi": ((3, B3, 3, [0, 31, 40], HI, OUT, 2), "range 1"),
    "touching_ranges": ((3, B3, 3, [0, 20, 30], HI, OUT, 2), "range 2"),
    "overlapping_ranges": ((3, B3, 3, [0, 5, 40], HI, OUT, 2), "range 1"),
    "range_output_too_high": ((3, B3, 3, LO, HI, [0, 3, -1], 2), "range 1"),
    "range_output_too_low": ((3, B3, 3, LO, HI, [0, 1, -2], 2), "range 2"),
    "default_too_high": ((3, B3, 3, LO, HI, OUT, 3), "default_output"),
    "default_too_low": ((3, B3, 3, LO, HI, OUT, -2), "default_output"),
}


@pytest.mark.parametrize("name", sorted(BAD_SPECS))
def test_malformed_spec_refused(ca, name):
    raw, match = BAD_SPECS[name]
    _refused(ca, match, raw_spec=raw)


def test_null_spec_refused(ca):
    _refused(ca, "NULL", raw_spec="null")


@pytest.mark.parametrize("mode", [
    dict(keep_ranges=[(0, 100)]),
    dict(n_output_shards=2),
    dict(max_output_bytes=1 << 20),
], ids=["keep_ranges", "shards", "size_split"])
def test_rejected_job_modes(ca, mode):
    _refused(ca, "unsupported", **mode)


def test_well_formed_call_needs_a_gpu(ca):
    if ca.device_count() > 0:
        pytest.skip("GPU present; the no-GPU refusal is exercised on CPU boxes")
    with pytest.raises(ca.GpuCompactError, match=f"rc={NO_GPU}:"):
        ca.compact_routed(INS, ["/o/a", "/o/b"], [(0, 10, 0), (20, 30, 1)], 1)
    # no ranges at all is well formed too (NULL arrays with a zero count)
    with pytest.raises(ca.GpuCompactError, match=f"rc={NO_GPU}:"):
        ca.compact_routed(INS, None, None, None, raw_spec=(1, ["/o/a"], 0, None, None, None, 0))


def test_anticompact_refuses_overlapping_classes(ca):
    with pytest.raises(ValueError, match="overlap"):
        ca.anticompact(INS, "/o/a", "/o/b", "/o/c", [(0, 100)], [(100, 200)])
    with pytest.raises(ValueError, match="overlap"):
        ca.anticompact(INS, "/o/a", "/o/b", "/o/c", [(0, 100), (300, 400)], [(-5, 0)])


def test_anticompact_builds_one_sorted_table(ca, monkeypatch):
    seen = {}

    def fake(input_bases, output_bases, ranges, default_output, **kw):
        seen.update(bases=output_bases, ranges=ranges, default=default_output, kw=kw)
        return {}

    monkeypatch.setattr(ca, "compact_routed", fake)
    ca.anticompact(INS, "/o/a", "/o/b", "/o/c", [(300, 400), (0, 100)], [(101, 200)],
                   now_sec=5)
    assert seen["bases"] == ["/o/a", "/o/b", "/o/c"]
    assert seen["ranges"] == [(0, 100, 0), (101, 200, 1), (300, 400, 0)]
    assert seen["default"] == 2
    assert seen["kw"] == {"now_sec": 5, "never_purge": True}


def test_declared_and_exported(product_lib):
    hdr = open(os.path.join(REPO, "include", "gpucompact.h")).read()
    assert re.search(r"^int gpuc_compact_routed\(const gpuc_job\* job, "
                     r"const gpuc_route_spec\* spec,", hdr, re.M)
    assert "typedef struct gpuc_route_spec {" in hdr
    assert "typedef struct gpuc_route_output {" in hdr
    lib = ctypes.CDLL(product_lib)
    assert hasattr(lib, "gpuc_compact_routed")


def test_route_structs_match_the_header(tmp_path, ca):
    """The ctypes mirrors have the C structs' sizes and field offsets."""
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n'
        f'#include "{REPO}/include/gpucompact.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(gpuc_route_spec),\n'
        '  offsetof(gpuc_route_spec, default_output), sizeof(gpuc_route_output),\n'
        '  offsetof(gpuc_route_output, partitions),\n'
        '  offsetof(gpuc_route_output, compressed_bytes)); return 0; }\n')
    binp = str(tmp_path / "sz")
    subprocess.run(["gcc", "-o", binp, str(src)], check=True)
    got = [int(x) for x in subprocess.run([binp], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [ctypes.sizeof(ca.GpucRouteSpec), ca.GpucRouteSpec.default_output.offset,
                   ctypes.sizeof(ca.GpucRouteOutput), ca.GpucRouteOutput.partitions.offset,
                   ca.GpucRouteOutput.compressed_bytes.offset]


def test_cli_builds_with_plain_gcc(tmp_path, product_lib):
    """gpuc_cli.c, anticompact command included, stays a gcc-only build."""
    binp = str(tmp_path / "gpuc_cli")
    subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-o", binp, CLI,
                    f"-L{os.path.dirname(product_lib)}", "-lcassandra_gpucompact",
                    f"-Wl,-rpath,{os.path.dirname(product_lib)}"], check=True)
    assert "anticompact" in open(CLI).read()
    r = subprocess.run([binp, "anticompact", "/o/a", "/o/b", "/o/c", "full=1:x", "/i/oa-1-big"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "bad range list" in r.stderr, r.stdout + r.stderr
