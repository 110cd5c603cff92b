"""GPU: the four output stages (kdtn_epoch_encode, kdtn_epoch_fanout, kdtn_epoch_remote_encode,
kdtn_epoch_tc) on the adversarial epochs of tests/stage_epochs.py, byte for byte against the
oracle (pinned on the same epochs by tests/test_output_stages_cpu.py), in two stage orders, with
a plain short epoch on the same context before and after each one."""
import numpy as np
import pytest

import stage_epochs as S
from helpers import golden_epoch
from kdtn import abi
from kdtn.abi import EINVAL
from kdtn.engine import KdtnError
from kdtn.model import pack
from test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu

NAMES = [n for n in S.COMPOSERS if n != "fan_nodes8193"]


def _same_arena(what, got, goff, want, woff):
    """Arena and offsets equal; else the first differing message / batch / slot index and a
    64-byte hex window of both sides around the first differing byte."""
    goff, woff = np.asarray(goff).astype(np.int64), np.asarray(woff).astype(np.int64)
    assert len(goff) == len(woff), (what, "offsets", len(goff), len(woff))
    bad = np.flatnonzero(goff != woff)
    assert not len(bad), f"{what}: offset {bad[0]} is {goff[bad[0]]}, the oracle's {woff[bad[0]]}"
    g, w = np.asarray(got), np.asarray(want)
    assert len(g) == len(w), (what, "bytes", len(g), len(w))
    diff = np.flatnonzero(g != w)
    if len(diff):
        d = int(diff[0])
        m = int(np.searchsorted(woff, d, side="right")) - 1
        a = max(d - 16, 0)
        raise AssertionError(f"{what}: index {m} (bytes {woff[m]}..{woff[m + 1]}) differs at byte {d} "
                             f"(+{d - woff[m]}); {len(diff)} bytes differ\n  got  {g[a:a + 64].tobytes().hex()}\n"
                             f"  want {w[a:a + 64].tobytes().hex()}")


def _fanout_same(engine, ref, ctx):
    node, off, idx = engine.fanout()
    for name, g, w in zip(("node", "off", "idx"), (node, off, idx), ref.fan):
        assert np.array_equal(g, w), (ctx, "fanout", name)


def _remote_same(engine, ref, ctx):
    arena, off, entry, nr, tc, tc_off = engine.remote_pods()
    wa, wo, we, wnr, wtc, wtco = ref.remote
    assert nr == wnr and np.array_equal(entry, we), (ctx, "remote entries", nr, wnr)
    _same_arena(f"{ctx}: RemotePod message", arena, off, wa, wo)
    _same_arena(f"{ctx}: remote tc argv", tc, tc_off, wtc, wtco)


def _tc_same(engine, ref, ctx):
    arena, off = engine.tc_argv(len(ref.out.add_idx), len(ref.out.upd_idx))
    _same_arena(f"{ctx}: tc slot", arena, off, *ref.tc)


def _wire_same(engine, ref, ctx):
    n = engine.encode()
    arena, off, err = engine.download_wire()
    wa, wo, werr = ref.wire
    assert n == len(wa) and np.array_equal(err, werr.astype(np.uint32)), (ctx, "wire err bits")
    _same_arena(f"{ctx}: batch (list * T + topology)", arena, off, wa, wo)


def _order_a(engine, inp, ref, ctx, fan=True):
    """inp None: the epoch is uploaded and run already (another entry point)."""
    if inp is not None:
        engine.upload(inp)
        engine.run()
        engine.sync()
    assert_same(engine.download(), ref.out, ctx)
    if fan:
        _fanout_same(engine, ref, ctx)
        _remote_same(engine, ref, ctx + " (strings)")
    _tc_same(engine, ref, ctx)
    _wire_same(engine, ref, ctx)
    if fan:
        _remote_same(engine, ref, ctx + " (properties copied from the wire arena)")


def _order_b(engine, inp, ref, ctx):
    if inp is not None:
        engine.upload(inp)
        engine.run()
        engine.sync()
    assert_same(engine.download(), ref.out, ctx)
    _wire_same(engine, ref, ctx)
    _tc_same(engine, ref, ctx)
    _remote_same(engine, ref, ctx + " (after encode)")
    _fanout_same(engine, ref, ctx)


_PLAIN = {}                     # the plain epoch and its reference, computed once


def _plain_epoch(golden):
    if "ep" not in _PLAIN:
        inp = pack(golden_epoch(golden, golden["transitions"][1]))
        _PLAIN["ep"] = (inp, S.reference(inp))
    return _PLAIN["ep"]


@pytest.mark.parametrize("name", NAMES)
def test_stage_epoch_both_orders(engine, golden, name):
    ep = S.COMPOSERS[name]()
    pin, pref = _plain_epoch(golden)
    _order_a(engine, pin, pref, "plain epoch before")
    _order_a(engine, ep.inp, ep.ref, f"{name}, order A")
    _order_b(engine, pin, pref, "plain epoch between")
    _order_b(engine, ep.inp, ep.ref, f"{name}, order B")
    _order_a(engine, pin, pref, "plain epoch after")


def test_fanout_over_the_node_cap_is_refused(engine, golden):
    """FAN_NODE_CAP + 1 destination daemons: kdtn_epoch_fanout and kdtn_epoch_remote_encode return
    KDTN_EINVAL naming the count, the run's other stages stay exact, and so does the next epoch."""
    ep = S.fan_nodes(S.FAN_NODE_CAP + 1)
    assert ep.expect["refused"]
    assert_same(engine.reconcile(ep.inp), ep.ref.out, "over the cap")
    def refused(stage):
        # KdtnError's text is kdtn_strerror(code), which returns the thread's last error message
        # (g_last_error, "fan-out over <n> daemons (cap 8192)") for KDTN_EINVAL
        with pytest.raises(KdtnError) as e:
            stage()
        assert e.value.code == EINVAL and f"{S.FAN_NODE_CAP + 1} daemons" in str(e.value), str(e.value)
    refused(engine.fanout)
    refused(engine.remote_pods)
    _tc_same(engine, ep.ref, "over the cap")
    _wire_same(engine, ep.ref, "over the cap")
    refused(engine.fanout)
    _order_a(engine, ep.inp, ep.ref, "over the cap, again", fan=False)
    pin, pref = _plain_epoch(golden)
    _order_a(engine, pin, pref, "plain epoch after the refusal")
    _order_b(engine, pin, pref, "plain epoch after the refusal")
    at_cap = S.fan_nodes(S.FAN_NODE_CAP)
    _order_a(engine, at_cap.inp, at_cap.ref, "at the cap after the refusal")


@pytest.mark.parametrize("order", ["A", "B"])
def test_string_lengths_as_append_only_suffix(engine, order):
    """kdict_keep / pdict_keep: the inline string tables of the kept prefix are built by an
    earlier epoch's output stage, those of the suffix from the keep index rounded down to 64,
    with long strings before, between and after."""
    ep = S.string_lengths()
    prefix, kk, pk = S.keep_suffix(ep)
    engine.upload(prefix)
    engine.run()
    engine.sync()
    engine.encode()                              # builds the prefix's string tables
    engine.tc_argv(0, 0)
    engine.upload(ep.inp, kk, pk)
    engine.run()
    engine.sync()
    (_order_a if order == "A" else _order_b)(engine, None, ep.ref, f"string_lengths kept {kk}/{pk}, order {order}")


@pytest.mark.parametrize("order", ["A", "B"])
def test_varints_after_a_late_pod_row(engine, order):
    """kdtn_epoch_late_pods: every peer of the varints epoch misses the table, the late row makes
    it resolve, and each RemotePod's net_ns is the row's (a pod index past the table)."""
    grown, rows, ref = S.varints_late()
    first = engine.reconcile(grown)
    assert (first.add_res["err"] == abi.E_PEER_LOOKUP).all()
    engine.remote_pods()                         # the stages of the run without the row: no message
    engine.late_pods(rows)
    engine.run()
    engine.sync()
    (_order_a if order == "A" else _order_b)(engine, None, ref, f"varints after a late row, order {order}")
    want_ns = b"/run/ns/late-vb"
    assert want_ns in ref.remote[0].tobytes()
