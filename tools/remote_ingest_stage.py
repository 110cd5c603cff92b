"""The RemotePod planning stage (kdtn_remote_ingest) on the config-2 RemotePod stream.

    python tools/remote_ingest_stage.py [--pods N] [--reps R] [--cache DIR] [--out FILE]
Runs one config-2 epoch, marshals its RemotePod messages (kdtn_epoch_remote_encode), strips each
length varint on the host and plans the bodies, against a VxlanManager snapshot holding every
eighth message's VNI. Times the stage with the engine's HIP events (rp_vni_build, rp_plan; mean
over reps after a warm-up call) and reports ms, the bytes read and written and GB/s beside the HBM
bound for those bytes, with the encoder's time for the same messages as context. Writes the
record as JSON (default profiles/remote_ingest_stage_cfg2.json). Needs an MI355X: no fallback.
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cache", default="/tmp/kdtn_cache")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remote_ingest_stage_cfg2.json"))
a = ap.parse_args()
inp = synth.make(2, pods_per_shard=a.pods, cache_dir=a.cache or None)
eng = Engine(device=0)
out = eng.reconcile(inp)
arena, off, entry, n_remote, _, _ = eng.remote_pods()
encode_ms = {k: v for k, v in eng.kernel_times().items() if k.startswith("remote_")}
total = np.diff(off.astype(np.int64))
live = np.flatnonzero(total > 0)                         # an empty slot: the message failed to marshal
hdr = 1 + (total[live] > 128) + (total[live] > 16385)    # bytes of the length varint in front of a body
start = (off[live].astype(np.int64) + hdr).astype(np.uint64)
size = (total[live] - hdr).astype(np.uint32)
vni = out.add_res["vni"][entry[live]][::8]
stream = arena.tobytes()
acc, rep_plan = {}, None
for rep in range(a.reps + 1):                            # call 0 warms up (code objects, buffers)
    if rep == 1:
        acc = {}
    plan, qd = eng.remote_ingest(stream, start, size, vni, [b"/run/netns/snapshot"] * len(vni))
    for k, v in eng.kernel_times().items():
        acc[k] = acc.get(k, 0.0) + v / a.reps
    rep_plan = eng.remote_plan()
ms = sum(acc.values())
read_b, written_b = int(size.sum()), len(size) * (64 + 72)
rec = {"config": 2, "pods": a.pods, "messages": int(len(size)), "body_bytes": read_b, "snapshot_entries": int(len(vni)),
       "reps": a.reps, "timer": "HIP events of the stage's stream marks, mean over reps after one warm-up call",
       "stage_ms": {k: round(v, 4) for k, v in acc.items()}, "stage_total_ms": round(ms, 4),
       "read_GBps": round(read_b / ms / 1e6, 1) if ms else None,
       "hbm_bound_ms": round((read_b + written_b) / HBM_PEAK_GBS / 1e6, 4),
       "n_direct": rep_plan.n_direct, "n_rejected": rep_plan.n_rejected, "n_conflict": rep_plan.n_conflict,
       "errs": {str(k): int(v) for k, v in zip(*np.unique(plan["err"], return_counts=True))},
       "remote_encode_ms": {k: round(v, 4) for k, v in encode_ms.items()}}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
