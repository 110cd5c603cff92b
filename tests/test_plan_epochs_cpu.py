"""CPU: the plan-shaped epochs of tests/plan_epochs.py have the shape their plan depends on.

Conditions on the inputs alone, from the packed tables and the oracle's output: which chunks are
bulk, where the full prefix ends, the share of realised records, the records per chunk, the
sizes of the window and hub chunks, and that every epoch carries the adversarial content (errors,
ghost peers, duplicate keys, CREATED and SKIP rows). The engine is not involved: that the GPU ran
the plan these shapes ask for is tests/test_launch_plan_gpu.py's assertion.
"""
import functools

import numpy as np
import pytest

import oracle as O
import plan_epochs as PE
from kdtn import abi

TICK = 15.625
BULK = {"add", "dele", "mixed"}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return O.reconcile(PE.named(name).inp, tick=TICK)


def _chunks(inp):
    return [(c * PE.TPW, min((c + 1) * PE.TPW, inp.topos.n)) for c in range((inp.topos.n + PE.TPW - 1) // PE.TPW)]


def _has_duplicate_key(inp, L, off):
    t = np.repeat(np.arange(inp.topos.n), np.diff(off.astype(np.int64)))
    rows = np.vstack([t, L.key]).T
    return len(np.unique(rows, axis=0)) < len(rows)


@pytest.mark.parametrize("name", PE.NAMED)
def test_chunk_classes_sit_where_intended(name):
    ep = PE.named(name)
    inp, T, ora = ep.inp, ep.inp.topos, _oracle(name)
    assert T.n <= 1024 and inp.realised.n + inp.desired.n <= 26_000
    cmp_ = PE.needs_comparison(inp)
    ko, kn = np.diff(T.real_off.astype(np.int64)), np.diff(T.des_off.astype(np.int64))
    recs = PE.chunk_records(inp)
    assert len(ep.classes) == len(recs)
    for c, ((a, b), cls) in enumerate(zip(_chunks(inp), ep.classes)):
        assert (not cmp_[a:b].any()) == (cls in BULK), (c, cls)
        act = ora.action[a:b]
        if cls == "add":
            assert ko[a:b].sum() == 0 and (T.flags[a:b] == 0).all(), c
        elif cls == "dele":
            assert kn[a:b].sum() == 0 and ko[a:b].sum() > 0, c
        elif cls == "mixed":
            assert (act == abi.ACT_CREATED).any() and (act == abi.ACT_SKIP).any() and kn[a:b].sum() > 0, c
            assert ((T.flags[a:b] & abi.TOPO_SPEC_NIL) != 0).any(), c
        elif cls == "fast":
            assert recs[c] <= PE.CAP, (c, recs[c])
        elif cls == "windows":
            assert b - a == 64 and recs[c] > PE.CAP and (ko[a:b] + kn[a:b]).max() <= PE.CAP, (c, recs[c])
        elif cls == "hub":
            assert ((ko[a:b] > PE.CAP) & (kn[a:b] > PE.CAP)).sum() == 1, c


@pytest.mark.parametrize("name", PE.NAMED)
def test_full_prefix_ends_where_the_plan_says(name):
    ep = PE.named(name)
    assert PE.first_partial_chunk(ep.inp, _oracle(name)) == ep.expect["first_partial_chunk"]


@pytest.mark.parametrize("name", PE.NAMED)
def test_record_shares_and_records_per_chunk(name):
    ep = PE.named(name)
    M, N = ep.inp.realised.n, ep.inp.desired.n
    nwg = len(ep.classes)
    if name == "teardown":
        assert N == 0 and M > 0
    elif name == "split4_default":
        assert M == 0
    else:
        assert M > 0 and M * 4 <= N, (M, N)
    assert bool(ep.expect["diff_build"]) == (M > 0 and N > 0)
    if ep.per_chunk:
        lo, hi = ep.per_chunk
        assert lo <= (M + N) // nwg < hi, ((M + N) // nwg, ep.per_chunk)
    if name == "all_prefix_diff":
        assert not PE.needs_comparison(ep.inp).any()
    if name == "split4_ragged":
        recs = PE.chunk_records(ep.inp)
        assert [int(recs[c]) for c in (1, 3, 4)] == [2, PE.RAGGED_ODD, 4 * PE.BLOCK]
        assert PE.RAGGED_ODD % 2 == 1 and PE.RAGGED_ODD % 64 != 0
        assert max(1, 3, 4) < ep.expect["first_partial_chunk"]


@pytest.mark.parametrize("name", PE.NAMED)
def test_adversarial_content(name):
    ep = PE.named(name)
    inp, ora = ep.inp, _oracle(name)
    compares = bool(PE.needs_comparison(inp).any())
    assert (len(ora.del_idx) > 0) == (inp.realised.n > 0)
    assert (len(ora.add_idx) > 0) == (inp.desired.n > 0)
    assert (len(ora.upd_idx) > 0) == compares
    if inp.desired.n:                                   # (a teardown adds nothing)
        assert (ora.add_qdisc["err"] != 0).any()
        assert (ora.add_res["err"] == abi.E_PEER_LOOKUP).any()
    assert _has_duplicate_key(inp, inp.desired, inp.topos.des_off) or \
        _has_duplicate_key(inp, inp.realised, inp.topos.real_off)
    assert (ora.action == abi.ACT_CREATED).any() and (ora.action == abi.ACT_SKIP).any()
    assert inp.vnis.n > 0
    assert ((inp.topos.flags & abi.TOPO_STATUS_NIL) != 0).any()


@pytest.mark.parametrize("x", PE.SWEEP)
def test_split_sweep_shapes(x):
    ep = PE.sweep(x)
    inp = ep.inp
    recs = PE.chunk_records(inp)
    assert int(recs[1]) == x and len(recs) == 4
    assert not PE.needs_comparison(inp)[:3 * PE.TPW].any() and PE.needs_comparison(inp)[3 * PE.TPW]
    assert inp.realised.n * 4 <= inp.desired.n and (inp.realised.n + inp.desired.n) // 4 >= 1200
    assert PE.first_partial_chunk(inp, O.reconcile(inp, tick=TICK)) == 3


def test_sweep_totals_straddle_the_part_boundaries():
    assert PE.SWEEP == [255, 256, 257, 1023, 1024, 1025]


def test_place_wave_epoch_is_perturbed_and_large_enough():
    ep = PE.place_wave_adversarial()
    inp = ep.inp
    assert (inp.topos.n + PE.TPW - 1) // PE.TPW >= 4 * 256
    assert inp.realised.n * 4 > inp.desired.n > 0              # comparison-heavy: split 1
    des, off = inp.desired, inp.topos.des_off.astype(np.int64)
    same = (des.key[:, 1:] == des.key[:, :-1]).all(axis=0)     # a record with its neighbour's key ...
    same[off[1:-1] - 1] = False                                # ... in the same Topology's list
    assert same.any()
    n_err = len([s for s in dict.fromkeys(PE.PCTS + PE.DURS + PE.RATES) if s])
    assert (des.prop >= inp.pdict.n - n_err).any()             # property ids of the appended error strings
    # (no Topology of this workload has an empty list, so the nil-flag edit finds nothing to set)
