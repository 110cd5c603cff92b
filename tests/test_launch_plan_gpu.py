"""GPU: every launch plan of kdtn_epoch_run on adversarial epochs, bit for bit vs the oracle.

kdtn_epoch_run chooses its kernels from the upload's sizes (fused or serial front, comparison
or look-back build of k_reconcile, 1-4 workgroups per chunk, wave-per-chunk or parts-per-chunk
placement). tests/plan_epochs.py composes one adversarial epoch per plan; each test here
compares every output field with the CPU oracle and then asserts from Engine.plan() that the
epoch ran the branch it was built for — an epoch that silently ran another plan fails.

Running time (MI355X, whole `-m gpu` suite, --durations=0): this file 4.96 s for its 42 tests,
of which 1.9 s generate the 70k-Topology epoch and its oracle once and about 1.5 s compose,
pack and reconcile the eight named epochs once; the 24 test_random_epochs seeds take 0.31 s
together. The file is therefore above that yardstick: what it spends is the one-off generation
(shared by all tests through the caches below), not the GPU runs or the comparisons, which
take 10-100 ms per test.
"""
import functools

import numpy as np
import pytest

import oracle as O
import plan_epochs as PE
from helpers import trim, with_rows
from kdtn import abi

pytestmark = pytest.mark.gpu
TICK = 15.625
MID = "place_wave_adversarial"
EPOCHS = PE.NAMED + [MID]
LISTS = ("action", "del_off", "add_off", "upd_off", "del_idx", "add_idx", "upd_idx")


def _epoch(name) -> PE.PlanEpoch:
    return PE.place_wave_adversarial() if name == MID else PE.named(name)


def _reference(name, inp):
    return (O.reconcile_parallel if name == MID else O.reconcile)(inp, tick=TICK)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's epoch, computed once and shared (no test writes to it)."""
    return _reference(name, _epoch(name).inp)


def _late_row(inp) -> np.ndarray:
    """One pod row that no link names: Topology 0's namespace, and for its name the first
    record's interface string, which is no Topology's name and no record's peer_pod."""
    L0 = inp.desired if inp.desired.n else inp.realised
    ns, name = int(inp.topos.ns[0]), int(L0.key[abi.KEY_COLS.index("local_intf"), 0])
    assert not (inp.topos.name == name).any()
    for L in (inp.realised, inp.desired):
        assert not (L.key[abi.KEY_COLS.index("peer_pod")] == name).any()
    return np.array([[ns, name, 0, 0]], np.uint32)


def assert_same(got, want, ctx):
    bad = got.mismatches(want)
    if bad:
        f = bad[0]
        a, b = getattr(got, f), getattr(want, f)
        diff = [i for i in range(min(len(a), len(b))) if a[i].tobytes() != b[i].tobytes()][:5]
        raise AssertionError(f"{ctx}: fields {bad} differ; {f} len {len(a)} vs {len(b)}; first idx {diff}: "
                             f"{[a[i] for i in diff]} vs {[b[i] for i in diff]}")


def assert_plan(plan, ep, front, ctx):
    """The branch the epoch was built for, field by field (no formula over n_cus: a chip on
    which the shape does not reach its branch fails)."""
    exp = dict(ep.expect)
    split_min = exp.pop("split_min", None)
    for f, v in exp.items():
        assert v is None or plan[f] == v, (ctx, f, plan)
    if split_min is not None:
        assert plan["split"] >= split_min, (ctx, plan)
    assert plan["front"] == front, (ctx, plan)
    assert plan["nwg"] == (ep.inp.topos.n + PE.TPW - 1) // PE.TPW and plan["n_cus"] > 0, (ctx, plan)
    assert (plan["place_parts"] >= 1) == (plan["place"] != abi.PLACE_NONE), (ctx, plan)


def _run(engine, stages=abi.STAGE_ALL):
    engine.run(stages)
    engine.sync()
    return engine.download()


@pytest.mark.parametrize("name", EPOCHS)
def test_base_run_matches_oracle_and_runs_its_plan(engine, name):
    ep = _epoch(name)
    want = _oracle(name)
    got = engine.reconcile(ep.inp)
    plan = engine.plan()
    print(f"plan[{name}] = {plan}")
    assert_same(got, want, name)
    assert_plan(plan, ep, abi.FRONT_FUSED, name)
    assert plan["first_partial_chunk"] == PE.first_partial_chunk(ep.inp, want), plan
    assert plan["kstrings_parsed"] == ep.inp.kdict.n and plan["pstrings_parsed"] == ep.inp.pdict.n, plan


@pytest.mark.parametrize("name", EPOCHS)
def test_serial_front_gives_the_fused_fronts_bytes(engine, name):
    """One late pod row takes the run off the fused front (k_kdict_flags, launch_pdict,
    k_epoch_begin, k_pod_direct_scatter, k_pod_verify_prefix): the same plan otherwise, the
    oracle's outputs over the table with that list-less Topology, the fused run's bytes."""
    ep = _epoch(name)
    inp = ep.inp
    fused = engine.reconcile(inp)
    assert engine.plan()["front"] == abi.FRONT_FUSED
    rows = _late_row(inp)
    engine.late_pods(rows)
    got = _run(engine)
    assert_plan(engine.plan(), ep, abi.FRONT_SERIAL, name)
    want = _reference(name, with_rows(inp, inp.kdict, rows, np.array([False])))
    assert_same(got, trim(want, inp.topos.n), f"{name}: serial front")
    assert not got.mismatches(fused), got.mismatches(fused)


@pytest.mark.parametrize("name", EPOCHS)
def test_stage_masks(engine, name):
    ep = _epoch(name)
    want = _oracle(name)
    got = engine.reconcile(ep.inp, abi.STAGE_DIFF)
    for f in LISTS:
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), (name, "DIFF", f)
    assert_plan(engine.plan(), ep, abi.FRONT_SERIAL, name)      # (no pod tables without resolve)
    got = engine.reconcile(ep.inp, abi.STAGE_DIFF | abi.STAGE_RESOLVE)
    for f in LISTS + ("del_res", "add_res", "upd_res"):
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), (name, "DIFF | RESOLVE", f)
    assert_plan(engine.plan(), ep, abi.FRONT_FUSED, name)


@pytest.mark.parametrize("name", EPOCHS)
def test_repeat_on_the_resident_tables(engine, name):
    ep = _epoch(name)
    engine.upload(ep.inp)
    a, pa = _run(engine), engine.plan()
    b, pb = _run(engine), engine.plan()
    assert not a.mismatches(b), a.mismatches(b)
    assert pa == pb
    assert_plan(pb, ep, abi.FRONT_FUSED, name)
    assert_same(b, _oracle(name), f"{name}: second run")


@pytest.mark.parametrize("x", PE.SWEEP)
def test_split_sweep(engine, x):
    """A bulk chunk of x records shared by 4 parts, x around 4*64 and 4*256: the parts' record
    ranges (ceil(x / 4) each, the last one ragged) and the partial waves of the qdisc store."""
    ep = PE.sweep(x)
    want = O.reconcile(ep.inp, tick=TICK)
    got = engine.reconcile(ep.inp)
    assert_plan(engine.plan(), ep, abi.FRONT_FUSED, ep.name)
    for f in ("add_idx", "add_off", "add_res", "add_qdisc"):
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), (x, f)
    assert_same(got, want, ep.name)
