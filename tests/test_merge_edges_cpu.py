"""Merge, reconcile and purge edge cases, CPU half (no GPU).

Pins the reference before the GPU is compared with it:
  * `fromdump` is the exact inverse of `dumpsst` / `gen dump=1`;
  * each authored matrix reaches every rule line it is there for, with each
    side winning (the census), so removing a kind from a matrix fails here;
  * `oracle compact` on every matrix and job holds, case by case, exactly
    what the Python model of the reference rules predicts.
"""
import filecmp
import os
import subprocess

import pytest

import authored_tables as at

COMPONENTS = ["Data.db", "Index.db", "CompressionInfo.db", "Filter.db",
              "Digest.crc32", "Statistics.db", "Summary.db", "TOC.txt"]
BTI_COMPONENTS = ["Data.db", "CompressionInfo.db", "Filter.db", "Digest.crc32",
                  "Statistics.db", "Partitions.db", "Rows.db", "TOC.txt"]

# the gen dump=1 shapes of test_flush_table_full_schema
GEN_SHAPES = {
    "simple": dict(seed=21, rows=800, vlen=90, tomb=15, pdel=3),
    "wide": dict(seed=22, rows=40, crows=50, vlen=120, rtomb=40, tomb=10,
                 statics=40, cktext=1, ttl=30),
    "cpx": dict(seed=23, rows=500, vlen=60, cpx=45, cpxdel=25),
    "counter": dict(seed=24, rows=500, counter=1),
    "multicol": dict(seed=25, rows=60, crows=12, ckcols=2, ncols=5, colmiss=30, snappy=1),
    "bti": dict(seed=26, rows=30, crows=40, vlen=200, rtomb=30, bti=1),
}


def _run(oracle, *args):
    return subprocess.run([oracle, *[str(a) for a in args]], capture_output=True, text=True)


@pytest.mark.parametrize("shape", sorted(GEN_SHAPES))
def test_fromdump_round_trips(oracle_bin, tmp_path, shape):
    """A: fromdump(gen's memdump) == gen's sstable in every component.
    B: dumpsst(fromdump(x)) == x."""
    kw = GEN_SHAPES[shape]
    d = str(tmp_path)
    assert _run(oracle_bin, "gen", d, "n=1", "dump=1", *[f"{k}={v}" for k, v in kw.items()]).returncode == 0
    stem = "da-1-bti" if kw.get("bti") else "oa-1-big"
    r = _run(oracle_bin, "fromdump", f"{d}/{stem}.memdump", f"{d}/back")
    assert r.returncode == 0, r.stderr
    for c in BTI_COMPONENTS if kw.get("bti") else COMPONENTS:
        assert filecmp.cmp(f"{d}/{stem}-{c}", f"{d}/back-{c}", shallow=False), f"{shape}: {c} differs"
    assert _run(oracle_bin, "dumpsst", f"{d}/back", f"{d}/back.memdump").returncode == 0
    assert open(f"{d}/back.memdump", "rb").read() == open(f"{d}/{stem}.memdump", "rb").read()
    # the Python reader and writer agree with the oracle's on the same bytes
    data = open(f"{d}/{stem}.memdump", "rb").read()
    if shape != "counter":      # counter contexts exceed the authored 16-byte value limit
        schema, stats, parts = at.parse_gmd2(data)
        assert at.header_stats(parts) == stats, "header stats rule differs from the generator's"
        if all(len(c.value) <= 16 for p in parts for it in p.items if isinstance(it, at.Row)
               for c in it.cells.values()):
            assert at.to_gmd2(schema, parts) == data


def test_fromdump_rejects_malformed(oracle_bin, tmp_path):
    m = at.matrix_b()
    good = at.to_gmd2(m.schema, m.tables()[0][0])
    bad = {
        "bad magic": b"GMD1" + good[4:],
        "trailing bytes": good + b"\0",
        "truncated": good[:-3],
        "truncated in header": good[:9],
        "cell flags": None,
    }
    # a present cell whose flag byte disagrees with its fields
    sk = at.matrix_a_skinny()
    one = at.to_gmd2(sk.schema, sk.tables()[0][0][:1])
    i = one.rindex(b"\x03" + at.struct.pack("<q", at.T))
    bad["cell flags"] = one[:i] + b"\x07" + one[i + 1:]
    for what, data in bad.items():
        p = tmp_path / "bad.memdump"
        p.write_bytes(data)
        r = _run(oracle_bin, "fromdump", p, tmp_path / "out")
        assert r.returncode != 0 and "memdump" in r.stderr, (what, r.stderr)
        assert not os.path.exists(f"{tmp_path}/out-Data.db"), what
    # a partition deletion before the epoch has no encoding in the format
    neg = at.to_gmd2(at.SKINNY, [at.Partition(at.case_key(1), del_=at.DT(-5, at.L))])
    (tmp_path / "neg.memdump").write_bytes(neg)
    r = _run(oracle_bin, "fromdump", tmp_path / "neg.memdump", tmp_path / "out")
    assert r.returncode != 0 and "negative markedForDeleteAt" in r.stderr
    p = tmp_path / "good.memdump"
    p.write_bytes(good)
    assert _run(oracle_bin, "fromdump", p, tmp_path / "out").returncode == 0


def test_builder_is_accepted_by_the_flush_parser():
    """The engine's own memdump parser takes every authored table."""
    from cassandra_amd import _parse_memdump
    for mk in at.ALL_MATRICES:
        m = mk()
        ins, tomb = m.tables()
        for parts in ins + [tomb]:
            data = at.to_gmd2(m.schema, parts)
            _, _, n, _ = _parse_memdump(data)
            assert n == len(parts)
            s2, stats, p2 = at.parse_gmd2(data)
            assert [at.canonical(p) for p in p2] == [at.canonical(p) for p in parts]
            assert stats == at.header_stats(parts)


def test_header_stats_epoch_defaults():
    p = at.Partition(at.case_key(0), items=[at.Row((), cells={0: at.Cell(5, b"x")})])
    assert at.header_stats([p]) == (5, at.DELETION_TIME_EPOCH, 0)
    assert at.header_stats([]) == (at.TIMESTAMP_EPOCH, at.DELETION_TIME_EPOCH, 0)


# ---- census -----------------------------------------------------------------
RECONCILE_LINES = {("reconcile", line, side)
                   for line in ("timestamp", "has_deletion_time", "tombstone_vs_expiring",
                                "local_deletion_time", "value")
                   for side in ("left", "right")} | {("reconcile", "full_tie", "left")}
LIVENESS_LINES = {("liveness", line, v) for line in ("timestamp", "expired", "expiration_time", "expiring")
                  for v in (True, False)}
DT_LINES = {("dt_supersedes", line, v) for line in ("marked_for_delete_at", "local_deletion_time")
            for v in (True, False)}
DELETES_LINES = {("deletes", "<", True), ("deletes", "==", True), ("deletes", ">", False)}
MARKER_KINDS = {("marker_emitted", k, True) for k in at.KIND_NAMES.values()}
PURGE_LINES = {("purge", line, False) for line in ("gc_before==", "gc_before>", "overlap==", "overlap>",
                                                   "never_purge")} | {("purge", "purged", True)}
EXPIRY_LINES = {("expiry", f"{p}now{op}let", op != "<") for p in ("", "liveness ") for op in ("<", "==", ">")}

CENSUS = {
    "A_i_skinny": RECONCILE_LINES,
    "A_ii_wide": RECONCILE_LINES,
    "A_iii_map": RECONCILE_LINES,
    "A_eight": RECONCILE_LINES,
    "A_counter": {("counter", "tombstone_vs_live", "left"), ("counter", "tombstone_vs_live", "right"),
                  ("reconcile", "timestamp", "left"), ("reconcile", "timestamp", "right"),
                  ("reconcile", "local_deletion_time", "left"),
                  ("reconcile", "local_deletion_time", "right"), ("reconcile", "full_tie", "left")},
    "A_counter_gc": {("counter", "tombstone_vs_live", "left"), ("counter", "tombstone_vs_live", "right"),
                     ("reconcile", "timestamp", "left"), ("reconcile", "timestamp", "right"),
                     ("reconcile", "local_deletion_time", "left"),
                     ("reconcile", "local_deletion_time", "right"), ("reconcile", "full_tie", "left")},
    "A_iv_gc": RECONCILE_LINES | DELETES_LINES,
    "B_rowlevel": LIVENESS_LINES | DT_LINES | DELETES_LINES,
    "C_bigint": MARKER_KINDS | DT_LINES | DELETES_LINES,
    "C_composite": MARKER_KINDS | DT_LINES | DELETES_LINES,
    "C_text": MARKER_KINDS | DT_LINES | DELETES_LINES,
    "C_blocks": {("marker_emitted", k, True) for k in ("INCL_START", "INCL_END")} |
                {("deletes", "==", True), ("deletes", ">", False)},
    "D_jobs": PURGE_LINES | EXPIRY_LINES,
    "E_timestamps": RECONCILE_LINES | DELETES_LINES,
}
MATRICES = {mk().name: mk for mk in at.ALL_MATRICES}


def test_every_matrix_has_a_census():
    assert set(CENSUS) == set(MATRICES)


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_census(name):
    """The model reaches every rule line the matrix is there for, with each
    side winning. Take a kind out of a matrix and this fails."""
    m = MATRICES[name]()
    census = at.Census()
    for _, job in m.jobs:
        m.predict(job, census)
    missing = CENSUS[name] - set(census)
    assert not missing, f"{name}: rule lines never reached: {sorted(missing, key=str)}"
    print(name, len(m.cases), "cases", {k: census[k] for k in sorted(CENSUS[name], key=str)})


def test_census_notices_a_removed_kind(monkeypatch):
    monkeypatch.setattr(at, "CELL_KINDS", [k for k in at.CELL_KINDS if k[0] != "exp61_L"])
    census = at.Census()
    at.matrix_a_skinny().predict(at.Job(), census)
    # without the all-fields-tie pair of expiring cells only equal cells tie fully
    assert census[("reconcile", "full_tie", "left")] < 17
    monkeypatch.setattr(at, "CELL_KINDS", [k for k in at.CELL_KINDS if not k[0].startswith("tomb")])
    census = at.Census()
    at.matrix_a_skinny().predict(at.Job(), census)
    assert RECONCILE_LINES - set(census)


def test_a_eight_ties_inputs_three_and_seven():
    for c in at.matrix_a_eight().cases:
        newest = sorted(range(8), key=lambda i: -(c.inputs[i].items[0].cells[0].ts
                                                  if c.inputs[i] else at.NO_TS))[:2]
        assert sorted(newest) == [2, 6], c.label


# ---- oracle against model ---------------------------------------------------
def compare_with_model(oracle, m, d, model=at):
    """Runs every job of the matrix through `oracle compact` and returns the
    disagreements with the model, as readable lines."""
    bases, tbase = m.write(oracle, d)
    bad = []
    for jn, job in m.jobs:
        out = os.path.join(d, "out-" + str(m.jobs.index((jn, job))))
        args = job.oracle_args() + ([f"tombsrc={tbase}"] if tbase else [])
        r = _run(oracle, "compact", out, *bases, *args)
        assert r.returncode == 0, f"{m.name} [{jn}]: {r.stderr}"
        got = at.read_sstable(oracle, out, out + ".memdump")
        want = m.predict(job)
        for n in range(len(m.cases)):
            g = at.canonical(got[n]) if n in got else None
            w = at.canonical(want[n]) if n in want else None
            if g != w:
                bad.append(f"{m.name} [{jn}] case {n} [{m.cases[n].label}]:\n"
                           f"    oracle: {g}\n    model:  {w}")
        assert set(got) <= set(range(len(m.cases)))
    return bad


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_oracle_matches_model(oracle_bin, tmp_path, name):
    bad = compare_with_model(oracle_bin, MATRICES[name](), str(tmp_path))
    assert not bad, f"{len(bad)} cases differ:\n" + "\n".join(bad[:20])


# Proof that the comparison can fail: each mutation of one rule line of the
# model must make it disagree with the oracle somewhere.
def _mut_value_strict(left, right, census=None):
    w, line = at_reconcile(left, right, census)
    if line == "full_tie":
        return right, line
    return w, line


def _signed(b):
    return [x - 256 if x > 127 else x for x in b]


def _mut_signed_compare(left, right, census=None):
    w, line = at_reconcile(left, right, census)
    if line == "value":
        return (left if _signed(left.value) > _signed(right.value) else right), line
    return w, line


def _mut_expiring_over_tombstone(left, right, census=None):
    w, line = at_reconcile(left, right, census)
    if line == "tombstone_vs_expiring":
        return (right if w is left else left), line
    return w, line


at_reconcile = at.reconcile
MUTATIONS = {
    # final value compare `>=` -> `>`: the right cell wins a full tie
    "value_tie_goes_right": ("reconcile", _mut_value_strict),
    "signed_byte_compare": ("reconcile", _mut_signed_compare),
    "expiring_beats_tombstone": ("reconcile", _mut_expiring_over_tombstone),
    # deletes `<=` -> `<`
    "deletes_strict": ("dt_deletes", lambda d, ts, census=None: ts < d.mfda),
    # purge `ldt < gc_before` -> `<=`
    "purge_at_gc_before": ("should_purge", lambda job, ts, ldt, census:
                           not job.never_purge and ldt <= job.gc_before and
                           (job.overlap_min_ts is None or ts < job.overlap_min_ts)),
    # purge `ts < min_ts` -> `<=`
    "purge_at_overlap_min_ts": ("should_purge", lambda job, ts, ldt, census:
                                not job.never_purge and ldt < job.gc_before and
                                (job.overlap_min_ts is None or ts <= job.overlap_min_ts)),
    # expiry `now < let` -> `now <= let`
    "live_at_expiration": ("cell_is_live", lambda c, now:
                           c.ldt == at.LDT_NONE or (c.ttl != at.NO_TTL and now <= c.ldt)),
    # DeletionTime.supersedes ignoring the local deletion time
    "dt_supersedes_mfda_only": ("dt_supersedes", lambda a, b, census=None: a.mfda > b.mfda),
    # LivenessInfo.supersedes: the expired line dropped
    "liveness_ignores_expired": ("liveness_supersedes", lambda a, b, census=None:
                                 a.ts > b.ts if a.ts != b.ts else
                                 a.let > b.let if (a.ttl != 0) == (b.ttl != 0) else a.ttl != 0),
}
MUTATION_MATRICES = {
    "value_tie_goes_right": "A_i_skinny", "signed_byte_compare": "A_i_skinny",
    "expiring_beats_tombstone": "A_iii_map", "deletes_strict": "B_rowlevel",
    "purge_at_gc_before": "D_jobs", "purge_at_overlap_min_ts": "D_jobs",
    "live_at_expiration": "D_jobs", "dt_supersedes_mfda_only": "C_bigint",
    "liveness_ignores_expired": "B_rowlevel",
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutated_model_disagrees_with_oracle(oracle_bin, tmp_path, monkeypatch, mutation):
    attr, fn = MUTATIONS[mutation]
    monkeypatch.setattr(at, attr, fn)
    bad = compare_with_model(oracle_bin, MATRICES[MUTATION_MATRICES[mutation]](), str(tmp_path))
    print(f"mutation {mutation}: {len(bad)} failing cases in {MUTATION_MATRICES[mutation]}")
    assert bad, f"mutation {mutation} goes unnoticed"
