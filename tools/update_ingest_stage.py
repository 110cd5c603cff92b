"""The UpdateLinks planning stage (kdtn_update_ingest) on the config-2-shaped UPD stream.

    python tools/update_ingest_stage.py [--pods N] [--reps R] [--cache DIR] [--out FILE]
Runs one config-2 epoch and encodes its add batches (kdtn_epoch_encode): the same bytes are valid
UpdateLinks bodies. Plans them with the new stage and, alternating in the same process, with the
route a caller had before it: kdtn_wire_ingest (kind UPD) + kdtn_ingest_download + kdtn_make_qdiscs
over the downloaded property columns (MakeVeth and the cut are not in that route at all). The
stages' passes are timed with the engine's HIP events, each whole call with a host clock around
it (every call ends in a stream synchronise; the stream's upload is in both); mean over reps after
a warm-up round. Checks that both routes give the same qdisc records. Writes the record as JSON
(default profiles/update_ingest_stage_cfg2.json). Needs an MI355X: no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-dtn_amd"))
from kdtn import Engine, abi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pods", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cache", default="/tmp/kdtn_cache")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_ingest_stage_cfg2.json"))
a = ap.parse_args()
inp = synth.make(2, pods_per_shard=a.pods, cache_dir=a.cache or None)
T = inp.topos.n
eng = Engine(device=0)
eng.reconcile(inp)
eng.encode()
arena, off, _ = eng.download_wire()
lo = int(off[T])                                         # the ADD region: messages [T, 2T)
stream, moff = arena[lo:int(off[2 * T])].tobytes(), off[T:2 * T + 1] - np.uint64(lo)
encode_ms = {k: v for k, v in eng.kernel_times().items() if k.startswith("wire")}
del arena, inp


def timed(acc, name, fn):
    t0 = time.perf_counter()
    r = fn()
    acc[name] = acc.get(name, 0.0) + (time.perf_counter() - t0) * 1e3 / a.reps
    return r


new_ev, old_ev, wall = {}, {}, {}
for rep in range(a.reps + 1):                            # round 0 warms up (code objects, buffers)
    if rep == 1:
        new_ev, old_ev, wall = {}, {}, {}
    msgs, links, qd = timed(wall, "update_ingest", lambda: eng.update_ingest(stream, moff))
    for k, v in eng.kernel_times().items():
        new_ev[k] = new_ev.get(k, 0.0) + v / a.reps
    report = eng.update_plan()
    timed(wall, "wire_ingest", lambda: eng.wire_ingest(stream, moff, np.full(T, abi.BATCH_UPD, np.uint8)))
    for k, v in eng.kernel_times().items():
        old_ev[k] = old_ev.get(k, 0.0) + v / a.reps
    tab = timed(wall, "ingest_download", eng.ingest_tables)
    old_qd = timed(wall, "make_qdiscs", lambda: eng.make_qdiscs(tab.pdict, tab.desired.prop, tab.desired.gap))
assert qd.tobytes() == old_qd.tobytes(), "the two routes disagree on the qdisc records"
r4 = lambda d: {k: round(v, 4) for k, v in d.items()}    # noqa: E731
rec = {"config": 2, "pods": a.pods, "messages": T, "stream_bytes": len(stream), "links": int(len(links)), "reps": a.reps,
       "timer": "HIP events of each stage's stream marks; host clock around each whole call (upload and downloads "
                "included); mean over reps after one warm-up round, the two routes alternating",
       "update_ingest_ms": r4(new_ev), "update_ingest_total_ms": round(sum(new_ev.values()), 4),
       "wire_ingest_ms": r4(old_ev), "wire_ingest_total_ms": round(sum(old_ev.values()), 4),
       "host_wall_ms": r4(wall), "previous_route_wall_ms": round(sum(v for k, v in wall.items() if k != "update_ingest"), 4),
       "n_long": report.n_long, "n_direct": report.n_direct, "n_rejected": report.n_rejected, "n_cut": report.n_cut,
       "errs": {str(k): int(v) for k, v in zip(*np.unique(links["err"], return_counts=True))},
       "wire_encode_ms": r4(encode_ms)}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
