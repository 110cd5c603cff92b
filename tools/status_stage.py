"""The status write-back stage (kdtn_epoch_status_encode) on one config-2 epoch.

    python tools/status_stage.py [--pods N] [--reps R] [--cache DIR] [--out FILE]
Times the stage with the engine's HIP events (mean over reps after a warm-up epoch), reports
ms, arena bytes and GB/s beside the HBM write bound for those bytes, and the same epoch's
LinksBatchQuery encode (kdtn_epoch_encode) from the same build as context. Every Topology is
committed (an all-ones mask), so the arena holds every Link of the desired store. Writes the
record as JSON (default profiles/status_stage_cfg2.json). Needs an MI355X: no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (one HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-dtn_amd"))
from kdtn import Engine, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak

ap = argparse.ArgumentParser()
ap.add_argument("--pods", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cache", default="/tmp/kdtn_cache")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "status_stage_cfg2.json"))
a = ap.parse_args()
inp = synth.make(2, pods_per_shard=a.pods, cache_dir=a.cache or None)
eng = Engine(device=0)
eng.upload(inp)
mask = np.ones(inp.topos.n, np.uint8)
acc = {"status": {}, "encode": {}}
info = (0, 0)
wire_bytes = 0
for rep in range(a.reps + 1):                 # epoch 0 warms up (code objects, buffers, tables)
    if rep == 1:
        acc = {"status": {}, "encode": {}}
    eng.run()
    eng.sync()
    wire_bytes = eng.encode()
    for k, v in eng.kernel_times().items():
        acc["encode"][k] = acc["encode"].get(k, 0.0) + v / a.reps
    info = eng.status_encode(mask)
    for k, v in eng.kernel_times().items():
        acc["status"][k] = acc["status"].get(k, 0.0) + v / a.reps
n_written, n_bytes = info
ms = sum(acc["status"].values())
gpu_ms = ms - acc["status"].get("status_host_sync", 0.0)
rec = {"config": 2, "pods": a.pods, "topologies": int(inp.topos.n), "links": int(inp.desired.n), "reps": a.reps,
       "timer": "HIP events of the stage's stream marks, mean over reps after one warm-up epoch",
       "status_ms": {k: round(v, 4) for k, v in acc["status"].items()},
       "status_total_ms": round(ms, 4), "status_gpu_ms": round(gpu_ms, 4),
       "n_written": n_written, "arena_bytes": n_bytes,
       "arena_GBps_over_gpu_ms": round(n_bytes / gpu_ms / 1e6, 1) if gpu_ms else None,
       "hbm_write_bound_ms": round(n_bytes / HBM_PEAK_GBS / 1e6, 4),
       "wire_encode_ms": {k: round(v, 4) for k, v in acc["encode"].items()},
       "wire_encode_total_ms": round(sum(acc["encode"].values()), 4), "wire_bytes": wire_bytes}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
