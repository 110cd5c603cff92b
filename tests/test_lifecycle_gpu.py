"""Context lifetime: every device buffer a context allocated goes back with kdtn_destroy.
Three create / use / close cycles in one process, each touching the ingest (sharded and
plain), the epoch, every output stage, the VXLAN apply and a resident delta upload; free
device memory after the later cycles must stay where it was after the first."""
import numpy as np
import pytest
import torch

from kdtn import Engine, synth
from kdtn.delta import build_delta
from kdtn.tables import Vnis

pytestmark = pytest.mark.gpu
TICK = 15.625


def _cycle(doc):
    eng = Engine(device=0, tick_in_usec=TICK)
    try:
        eng.ingest(doc, shard=(2, 1))
        info = eng.ingest(doc)
        eng.run()
        counts = eng.sync()
        eng.encode()
        eng.fanout()
        eng.remote_encode()
        eng.tc_argv(counts.n_add, counts.n_upd)
        eng.status_encode(np.ones(info.n_topos, np.uint8))
        eng.vni_apply()
        st = eng.tables()
        # the smallest delta: no Topology changed, no string added, the resident VXLAN map kept
        d = build_delta(st, st, st.kdict.n, st.pdict.n, vnis=Vnis.keep_resident())
        assert d.n_changed == 0
        eng.upload_delta(d)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
    finally:
        eng.close()
    return before, torch.cuda.mem_get_info()[0]


def test_destroy_returns_every_buffer():
    # synth.make(1)'s document (a 0.49 GB footprint) is too small a workload here: the runtime
    # itself keeps 112 MiB more after the process's first create / close cycle, on the parent
    # commit as well: 23 % of that footprint. The cap stays and the workload grows
    doc = synth.topology_list_json(synth.make(2, pods_per_shard=60000))
    torch.cuda.init()
    before, after = zip(*[_cycle(doc) for _ in range(3)])
    foot = [a - b for a, b in zip(after, before)]
    print("free before close", before, "after close", after, "footprint", foot)
    assert all(f > 0 for f in foot), foot
    # a tenth of a cycle's footprint: a cap, not a measurement (a context that kept its buffers
    # would drift by a whole footprint per cycle)
    for k in (1, 2):
        assert after[0] - after[k] <= foot[0] // 10, (k, after, foot)
