"""Shared reference for the size-split (max_output_bytes) tests, all of it on
the CPU: oracle-generated inputs, the oracle's single-output result R of each
job, the cut points that tests/native/size_split_ref.cpp finds in R, and the
oracle's own `shard=first:last` output for every range. Built once per
session and never modified by the tests that use it."""
import json
import os
import struct
import subprocess

import pytest

import chunk_helpers as ch
import multi_cpx_helpers as mc
from conftest import ORACLE, REPO

KB1 = 1024
GC_NOW = 2000000000
# (g): two kept ranges inside a token range
G_RANGES = [(-3 * 2**61, -2**61), (-2**60, 2**62)]
G_TOKENS = (-2**62, 3 * 2**61)

# case -> what differs from "three LZ4 inputs re-chunked to 1 KiB, no job
# arguments". gen: oracle generator spec; cap: max_output_bytes; oracle: the
# job's own oracle_tool arguments; gpu: the same job as compact() keywords.
CASES = {
    "a": dict(gen="seed=11 rows=300 vlen=120 overlap=50 tomb=15", cap=6000),
    "a_cap1": dict(like="a", cap=1),
    "a_nocut": dict(like="a", cap=1 << 40, min_outputs=1),
    "b": dict(gen="seed=12 rows=8 crows=200 vlen=400 rtomb=30 statics=40", cap=20000),
    "c": dict(gen="seed=13 bti=1 snappy=1 rows=400 vlen=300", cap=40000, rechunk=0, bti=True),
    "d": dict(gen="seed=14 rows=600 vlen=700 overlap=30 tomb=10", cap=30000, rechunk=0,
              out_chunk=4096),
    "e_purge": dict(like="a", cap=6000, oracle=[f"now={GC_NOW}", f"gcbefore={GC_NOW}"],
                    gpu=dict(now_sec=GC_NOW, gc_before=GC_NOW)),
    "e_gc": dict(like="a", cap=4000, tombsrc=True, oracle=["cellgc=1"],
                 gpu=dict(cell_level_gc=True)),
    # the widened inputs are small (about 30 KB in all): 8000 gives two
    # outputs, so the same inputs also run at a cap that gives three or more
    "f": dict(widened="a", cap=8000, min_outputs=2),
    "f_cap3000": dict(like="f", cap=3000),
    "g": dict(like="a", cap=3000,
              oracle=["ranges=" + ",".join(f"{lo}:{hi}" for lo, hi in G_RANGES)],
              shard=G_TOKENS, gpu=dict(keep_ranges=G_RANGES, token_range=G_TOKENS)),
}


def components(case):
    return ch.DA_COMPONENTS if CASES[case].get("bti") else ch.OA_COMPONENTS


def oracle(*args):
    return subprocess.run([ORACLE, *[str(a) for a in args]], check=True, capture_output=True,
                          text=True)


def oracle_compact(out_base, inputs, args):
    r = oracle("compact", out_base, *inputs, *args)
    return json.loads(r.stdout.splitlines()[-1])


@pytest.fixture(scope="session")
def size_split_tool(oracle_bin, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("size_split_tool") / "size_split_ref")
    src = [os.path.join(REPO, "tests/native/size_split_ref.cpp")] + [
        os.path.join(REPO, "oracle/src", f)
        for f in ("sstable.cpp", "compact.cpp", "gen.cpp", "bti.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", *src, "-o", exe, "-l:liblz4.so.1", "-ldl"],
                   check=True, capture_output=True)
    return exe


def cut_ranges(tool, r_base, cap):
    r = subprocess.run([tool, r_base, str(cap)], check=True, capture_output=True, text=True)
    return [json.loads(l) for l in r.stdout.splitlines() if l.strip()]


def _inputs(case, spec, d, widened):
    """-> (gpu inputs, oracle inputs) of a case that owns its inputs"""
    if "widened" in spec:
        raw = widened[spec["widened"]]["bases"]
    else:
        os.makedirs(d + "/raw")
        oracle("gen", d + "/raw", "n=3", *spec["gen"].split())
        name = "da-{}-bti" if spec.get("bti") else "oa-{}-big"
        raw = [f"{d}/raw/" + name.format(i) for i in (1, 2, 3)]
    cl = spec.get("rechunk", KB1)
    ins = [ch.rechunk(b, f"{d}/in/" + os.path.basename(b), cl, f"{d}/tmp") for b in raw] \
        if cl else list(raw)
    ins_oracle = list(ins)
    if spec.get("out_chunk"):
        # the oracle's output follows its first input's chunk length
        ins_oracle[0] = ch.rechunk(ins[0], f"{d}/oc/" + os.path.basename(ins[0]),
                                   spec["out_chunk"], f"{d}/tmpoc")
    return ins, ins_oracle


@pytest.fixture(scope="session")
def split_ref(size_split_tool, widened, tmp_path_factory):
    """case -> dict(inputs, gpu, cap, comps, r: the oracle's JSON of the
    single-output job, r_base, outputs: [dict(first_token, last_token,
    partitions, base: the oracle's sstable of that range, oracle: its JSON)])"""
    own, out = {}, {}
    for case, spec in CASES.items():
        d = str(tmp_path_factory.mktemp(f"ssplit_{case}"))
        src = spec.get("like", case)
        if src not in own:
            own[src] = _inputs(src, CASES[src], str(tmp_path_factory.mktemp(f"ssplit_in_{src}")),
                               widened)
        ins, ins_oracle = own[src]
        args = list(spec.get("oracle", []))
        gpu = dict(spec.get("gpu", {}))
        if spec.get("tombsrc"):
            args.append(f"tombsrc={ins_oracle[2]}")
            gpu["tombstone_sources"] = [ins[2]]
            ins, ins_oracle = ins[:2], ins_oracle[:2]
        if spec.get("out_chunk"):
            gpu["output_chunk_length"] = spec["out_chunk"]
        name = os.path.basename(ins[0]).split("-")
        r_base = f"{d}/{name[0]}-900-{name[2]}"
        shard = [f"shard={spec['shard'][0]}:{spec['shard'][1]}"] if spec.get("shard") else []
        r = oracle_compact(r_base, ins_oracle, args + shard)
        outputs = []
        for k, o in enumerate(cut_ranges(size_split_tool, r_base, spec["cap"])):
            o["base"] = f"{d}/{name[0]}-{1000 + k}-{name[2]}"
            # the range lies inside the job's own token range, so it replaces it
            o["oracle"] = oracle_compact(o["base"], ins_oracle,
                                         args + [f"shard={o['first_token']}:{o['last_token']}"])
            outputs.append(o)
        out[case] = dict(inputs=ins, gpu=gpu, cap=spec["cap"], comps=components(case), r=r,
                         r_base=r_base, outputs=outputs, name=name,
                         min_outputs=spec.get("min_outputs", 3))
    return out


def last_partition_offset(base):
    """Uncompressed offset of the last partition of a big-format sstable, from
    its Index.db (u16 key length, key, position vint, promoted-index vint size
    + bytes)."""
    with open(base + "-Index.db", "rb") as f:
        b = f.read()

    def uvint(o):
        first = b[o]
        extra = 0
        while extra < 8 and first & (0x80 >> extra):
            extra += 1
        v = first & (0xFF >> extra) if extra < 8 else 0
        for i in range(extra):
            v = (v << 8) | b[o + 1 + i]
        return v, o + 1 + extra

    o, pos = 0, None
    while o < len(b):
        (kl,) = struct.unpack_from(">H", b, o)
        o += 2 + kl
        pos, o = uvint(o)
        psz, o = uvint(o)
        o += psz
    assert o == len(b)
    return pos


def est_on_disk(offsets, chunk_len, e):
    """the rule: on-disk bytes of the chunks flushed once e bytes are held"""
    flushed = (e - 1) // chunk_len if e else 0
    return offsets[flushed] if flushed else 0
