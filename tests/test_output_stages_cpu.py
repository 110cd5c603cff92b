"""CPU: the oracle itself on the adversarial epochs of tests/stage_epochs.py, so that
tests/test_output_stages_gpu.py does not compare the engine with an oracle that is wrong at
these edges. Building an epoch runs its branch-coverage assertions (oracle outputs only); the
oracle's bytes are then checked against the Python protobuf runtime (tests/wire_pb.py) and
against plain restatements of the tc argv and of the fan-out grouping."""
import numpy as np
import pytest

import stage_epochs as S
from kdtn import abi
from test_wire_cpu import _check_epoch, _check_remote

SMALL = [n for n in S.COMPOSERS if n not in ("fan_nodes8192", "fan_nodes8193")]


@pytest.mark.parametrize("name", list(S.COMPOSERS))
def test_epoch_reaches_its_branch(name):
    ep = S.COMPOSERS[name]()             # the composer asserts its coverage
    assert ep.expect and ep.inp.topos.n > 0


@pytest.mark.parametrize("name", SMALL)
def test_wire_and_remote_match_protobuf_runtime(name):
    ep = S.COMPOSERS[name]()
    _check_epoch(ep.inp, ep.ref.out)
    _check_remote(ep.inp, ep.ref.out)


def _reached(out, T):
    """Per add / update entry: no earlier failing entry in the Topology's Del, Add, Update order."""
    ra, ru = np.zeros(len(out.add_idx), bool), np.zeros(len(out.upd_idx), bool)
    for t in range(T):
        ok = not (out.del_res["err"][out.del_off[t]:out.del_off[t + 1]] != 0).any()
        for e in range(out.add_off[t], out.add_off[t + 1]):
            if not ok:
                break
            ra[e] = True
            r, q = out.add_res[e], out.add_qdisc[e]
            builds = r["kind"] in (abi.KIND_SAME_NODE, abi.KIND_CROSS_NODE, abi.KIND_PHYSICAL)
            if r["err"] or (builds and q["err"]) or r["remote_err"]:
                ok = False
        for e in range(out.upd_off[t], out.upd_off[t + 1]):
            if not ok:
                break
            ru[e] = True
            if out.upd_res["err"][e]:
                ok = False
    return ra, ru


def _argv(intf: bytes, q) -> bytes:
    """common/qdisc.go:252-266: exec("tc", ...)'s arguments, each NUL-terminated."""
    return b"\0".join([b"qdisc", b"add", b"dev", intf, b"parent", b"1:1", b"handle", b"10:0", b"tbf", b"rate",
                       str(int(q["tbf_rate"])).encode(), b"burst", str(int(q["tbf_buffer"])).encode(),
                       b"latency", b"50ms", b"minburst", str(int(q["tbf_minburst"])).encode()]) + b"\0"


@pytest.mark.parametrize("name", SMALL)
def test_tc_argv_matches_restatement(name):
    ep = S.COMPOSERS[name]()
    inp, out = ep.inp, ep.ref.out
    arena, off = ep.ref.tc
    ra, ru = _reached(out, inp.topos.n)
    key = lambda col, j: inp.kdict.get(int(inp.desired.key[abi.KEY_COLS.index(col), j]))
    want = []
    for e in range(len(out.add_idx)):
        r, q, j = out.add_res[e], out.add_qdisc[e], int(out.add_idx[e])
        on = (ra[e] and q["has_tbf"] and not q["err"] and not r["err"] and
              r["kind"] in (abi.KIND_SAME_NODE, abi.KIND_CROSS_NODE, abi.KIND_PHYSICAL))
        want.append(_argv(key("local_intf", j), q) if on else b"")
        want.append(_argv(key("peer_intf", j), q) if on and r["kind"] == abi.KIND_SAME_NODE else b"")
    for e in range(len(out.upd_idx)):
        r, q, j = out.upd_res[e], out.upd_qdisc[e], int(out.upd_idx[e])
        on = ru[e] and q["has_tbf"] and not q["err"] and not r["err"]
        want.append(_argv(key("local_intf", j), q) if on else b"")
    assert len(off) == len(want) + 1
    for g, w in enumerate(want):
        assert arena[int(off[g]):int(off[g + 1])].tobytes() == w, g
    assert int(off[-1]) == len(arena)


@pytest.mark.parametrize("name", list(S.COMPOSERS))
def test_fanout_matches_dict_grouping(name):
    ep = S.COMPOSERS[name]()
    out = ep.ref.out
    node, off, idx = ep.ref.fan
    ra, _ = _reached(out, ep.inp.topos.n)
    groups: dict[int, list[int]] = {}
    for e in range(len(out.add_idx)):
        r, q = out.add_res[e], out.add_qdisc[e]
        if ra[e] and r["kind"] == abi.KIND_CROSS_NODE and not r["err"] and not q["err"]:
            groups.setdefault(int(r["vtep"]), []).append(e)
    assert node.tolist() == sorted(groups)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(groups[n]) for n in sorted(groups)])]).tolist()
    assert idx.tolist() == [e for n in sorted(groups) for e in groups[n]]


def test_entry_point_variants():
    """The keep-suffix split of string_lengths and the late-row variant of varints assert their
    own shape (long strings on both sides of the rounded keep index; every peer resolved by the
    late row) from the dictionaries and the oracle."""
    ep = S.string_lengths()
    prefix, kk, pk = S.keep_suffix(ep)
    assert prefix.kdict.n == kk and prefix.pdict.n == pk and kk % 64 and pk % 64
    assert prefix.kdict.bytes_.tobytes() == ep.inp.kdict.bytes_[:len(prefix.kdict.bytes_)].tobytes()
    grown, rows, ref = S.varints_late()
    assert len(rows) == 1 and len(ref.wire[1]) == 3 * grown.topos.n + 1 and len(ref.out.action) == grown.topos.n
