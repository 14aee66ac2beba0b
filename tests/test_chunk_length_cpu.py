"""CPU pins for chunk lengths from 1 byte to one 64 KiB chunk: the LZ4 and
Snappy scalar models and the wave-window decompositions the HIP kernels
transcribe, against the system codecs, byte for byte; plus a self-test of the
re-chunking helper the GPU tests build their inputs with."""
import os
import subprocess

import pytest

import chunk_helpers as ch
from conftest import ORACLE, REPO

NATIVE = os.path.join(REPO, "tests", "native")


def _build_run(binp, src, libs, args=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", binp, src, *libs], check=True)
    r = subprocess.run([binp, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout, r.stdout
    return r.stdout


def test_lz4_model_and_wave_sim_to_64k(tmp_path):
    _build_run(str(tmp_path / "cl_lz4"), os.path.join(NATIVE, "chunklen_lz4_fuzz.cpp"),
               ["-l:liblz4.so.1"])


def test_snappy_model_and_wave_mirror_to_64k(tmp_path):
    have = ch.snappy() is not None
    out = _build_run(str(tmp_path / "cl_snp"), os.path.join(NATIVE, "chunklen_snappy_fuzz.cpp"),
                     ["-ldl"], () if have else ("nolib",))
    assert have == ("skipped" not in out)


@pytest.mark.parametrize("chunk_len", [4096, 65536])
def test_rechunk_helper_roundtrips(oracle_bin, tmp_path, chunk_len):
    """A re-chunked, oracle-rewritten sstable is a genuine sstable at that
    chunk length: `oracle_tool roundtrip` reproduces every component."""
    d = str(tmp_path)
    subprocess.run([ORACLE, "gen", d, "seed=31", "n=1", "rows=600", "vlen=700", "tomb=10"],
                   check=True, capture_output=True)
    out = ch.rechunk(f"{d}/oa-1-big", f"{d}/r/oa-1-big", chunk_len, f"{d}/tmp")
    assert ch.chunk_length_of(out) == chunk_len
    assert ch.read_uncompressed(out) == ch.read_uncompressed(f"{d}/oa-1-big")
    r = subprocess.run([ORACLE, "roundtrip", out], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0 and lines, r.stdout + r.stderr
    assert all(l.startswith("OK") for l in lines), r.stdout
