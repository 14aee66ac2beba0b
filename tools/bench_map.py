"""A map<blob,blob> workload against a given engine .so (A/B regression probe;
bench.py has no complex-column workload): generate(complex_pct=50) once into
/tmp/gpuc_map_bench, then 1 warm-up + 3 timed compactions of the 8 inputs.
Prints one JSON line: MB/s, ms per step and the library's phase timings of
the last step.
Usage: python tools/bench_map.py <path-to-so>"""
import json
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cassandra_amd as ca

ca.load_library(sys.argv[1])
D = "/tmp/gpuc_map_bench"
N, ROWS = 8, 400_000
if not os.path.exists(f"{D}/in/oa-{N}-big-Data.db"):
    shutil.rmtree(D, ignore_errors=True)
    os.makedirs(f"{D}/in")
    ca.generate(f"{D}/in", seed=77, n_sstables=N, rows_per_sstable=ROWS, overlap_pct=30,
                value_len=128, complex_pct=50, complex_del_pct=10, tombstone_pct=5)
bases = [f"{D}/in/oa-{g}-big" for g in range(1, N + 1)]
last, t0 = None, None
for i in range(4):
    if i == 1:
        t0 = time.time()
    out = f"{D}/out{i}"
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    last = ca.compact(bases, f"{out}/oa-100-big")
    shutil.rmtree(out, ignore_errors=True)
el = time.time() - t0
print(json.dumps({"value": round(last["input_uncompressed_bytes"] * 3 / el / 1e6, 2),
                  "ms_per_step": round(el * 1000 / 3, 2),
                  "config": {"phase_ms": last["ms"], "partitions_out": last["partitions_out"],
                             "input_uncompressed_bytes": last["input_uncompressed_bytes"]}}))
