"""kdtn_remote_ingest on the GPU: RemotePod request bodies decoded and planned, against the Python
protobuf runtime over the descriptor of tests/wire_pb.py (ParseFromString of every body),
oracle.parse_cidr, oracle.make_qdisc (tick 15.625) and a Python dict for the VxlanManager map.
Every comparison is exact. Two expectations are literals because that runtime does not pin them:
the 10th-byte rule of a varint and the refusal of groups (include/kdtn.h)."""
import numpy as np
import pytest

import oracle as O
import stage_epochs as S
from kdtn import abi
from kdtn.engine import Engine
from test_wire_ingest_gpu import fld
from wire_pb import _C, _varint

pytestmark = pytest.mark.gpu
WINDOW = 16384                                      # k_rp_plan's LDS window
STRS = ("net_ns", "intf_name", "intf_ip", "peer_vtep", "kube_ns", "name")     # abi.RP_* order
V0, NS0 = 7000, b"/run/netns/cni-0"


@pytest.fixture(scope="module")
def eng():
    with Engine(device=0, tick_in_usec=15.625) as e:
        yield e


def body(m: int, props=(), **kw) -> bytes:
    """An ordinary RemotePod; props None: no properties field; a dict overrides the varying ones."""
    p = _C["RemotePod"](net_ns=f"/run/netns/cni-{m}", intf_name=f"eth{m % 9}", intf_ip=f"10.{m % 250}.0.2/24",
                        peer_vtep=f"192.168.1.{m % 250}", kube_ns="default", vni=5000 + m, name=f"pod-{m}")
    if props is not None:
        p.properties.SetInParent()
        for k, v in {"latency": f"{m % 40}ms", "loss": ("", "0.5", "12")[m % 3], "rate": ("", "1Gbit", "10mbit")[m % 3],
                     "gap": m % 4, **dict(props)}.items():
            setattr(p.properties, k, v)
    for k, v in kw.items():
        setattr(p, k, v)
    return p.SerializeToString()


def sized(size: int) -> bytes:
    """A body of exactly `size` bytes: the name stretched to fit."""
    pad = size - len(body(1, name=""))
    for _ in range(4):
        b = body(1, name="z" * pad)
        if len(b) == size:
            return b
        pad += size - len(b)
    raise AssertionError("no body of that size")


def lay(bodies, first=0):
    """Starts of the bodies in a receive buffer: 5 bytes (a gRPC frame header) before each."""
    return [int(s) for s in first + 5 + np.cumsum([0] + [len(b) + 5 for b in bodies])[:-1]]


def check(eng, bodies, starts=None, snap=(), rejected=()):
    """Every body against ParseFromString / parse_cidr / make_qdisc / the dict; returns the plans."""
    starts = lay(bodies) if starts is None else starts
    buf = bytearray(b"\xaa" * max([s + len(b) for s, b in zip(starts, bodies)] + [1]))
    for s, b in zip(starts, bodies):
        buf[s:s + len(b)] = b
    first = {}
    for i, (v, ns) in enumerate(snap):
        first.setdefault(v, (i, ns))                 # a key listed twice: its lowest entry
    plan, qd = eng.remote_ingest(bytes(buf), starts, [len(b) for b in bodies], [v for v, _ in snap], [ns for _, ns in snap])
    assert len(plan) == len(qd) == len(bodies)
    n_conf = 0
    for m, b in enumerate(bodies):
        g = plan[m]
        if m in rejected:
            assert g["wire_err"] == rejected[m], (m, g["wire_err"])
            zero = np.zeros(1, abi.REMOTE_PLAN_DTYPE)[0]
            zero["wire_err"] = g["wire_err"]
            assert g.tobytes() == zero.tobytes() and not qd[m].tobytes().strip(b"\0"), m
            continue
        p = _C["RemotePod"]()
        p.ParseFromString(b)
        assert g["wire_err"] == 0, (m, g["wire_err"])
        got = [bytes(buf[o:o + n]) for o, n in g["str"]]
        assert got == [getattr(p, f).encode() for f in STRS], m
        assert all(o == 0 for o, n in g["str"] if n == 0), m
        q = O.make_qdisc({**{c: getattr(p.properties, c) for c in abi.PROP_COLS}, "gap": p.properties.gap})
        assert qd[m].tobytes() == q.tobytes(), (m, qd[m], q)
        err = abi.E_REMOTE_CIDR if p.intf_ip and not O.parse_cidr(p.intf_ip) else int(q["err"])
        ent, ns = first.get(p.vni, (abi.RP_NO_ENTRY, None))
        conflict = ns is not None and ns != p.net_ns.encode()
        n_conf += conflict
        assert (g["vni"], g["err"], g["has_props"], g["vni_entry"], g["vni_conflict"]) == \
               (p.vni, err, p.HasField("properties"), ent, conflict), (m, g)
    rep = eng.remote_plan()
    assert (rep.window_bytes, rep.n_rejected, rep.n_conflict) == (WINDOW, len(rejected), n_conf)
    return plan


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_message_counts(eng, n):
    check(eng, [body(m) for m in range(n)], snap=[(5000 + m, f"/run/netns/cni-{m + m % 2}".encode()) for m in range(0, n, 3)])
    assert eng.remote_plan().n_direct == 0


def _staging():
    step = [next(b for b in (body(i, name="q" * k) for k in range(1, 40)) if (len(b) + 5) % 16 == 1) for i in range(17)]
    mod16 = [b"", body(0, props=None)] + step
    big = [body(0), sized(WINDOW), sized(WINDOW + 1), body(3), sized(3 * WINDOW), body(5)]
    at = lay(big, first=(-10 - len(big[0])) % 16)                      # the window-sized body starts 16-aligned
    many = [body(m) for m in range(65)]
    return {   # name: (bodies, starts, lanes read from memory)
        "every_start_mod_16": (mod16, lay(mod16), 0),
        "two_runs_per_wave": ([body(m, name="r" * 200) for m in range(64)], None, 0),
        "window_sizes": (big, at, 2),                                  # window + 1 and 3 windows do not fit
        "descending_wave": (many, lay(many)[63::-1] + lay(many)[64:], 64),
        "gap_over_a_window": ([body(0), body(1), body(2)], [0, 200, 400 + WINDOW + 1], 3),
    }


@pytest.mark.parametrize("case", ["every_start_mod_16", "two_runs_per_wave", "window_sizes", "descending_wave", "gap_over_a_window"])
def test_staging(eng, case):
    bodies, starts, n_direct = _staging()[case]
    starts = lay(bodies) if starts is None else starts
    if case == "every_start_mod_16":
        assert set(s % 16 for s in starts) == set(range(16))
    if case == "two_runs_per_wave":
        assert starts[-1] + len(bodies[-1]) - (starts[0] & ~15) > WINDOW
    if case == "window_sizes":
        assert starts[1] % 16 == 0 and len(bodies[1]) == WINDOW
    if case == "descending_wave":                                       # the same buffer, the first wave listed backwards
        bodies = bodies[63::-1] + bodies[64:]
    check(eng, bodies, starts)
    assert eng.remote_plan().n_direct == n_direct


UNK = fld(15, 0, _varint(300)) + fld(16, 1, b"\1" * 8) + fld(17, 2, b"\xffxyz") + fld(18, 5, b"\2" * 4)
P0 = _C["RemotePod"].FromString(body(3))
STRUCTURE = {
    "reverse": b"".join(reversed([fld(1, 2, b"/ns"), fld(2, 2, b"eth0"), fld(3, 2, b"10.0.0.1/24"), fld(4, 2, b"10.9.9.9"),
                                  fld(5, 2, b"kns"), fld(6, 0, _varint(5007)), fld(7, 2, P0.properties.SerializeToString()), fld(8, 2, b"pod")])),
    "repeated": fld(1, 2, b"first") + fld(6, 0, _varint(7)) + fld(3, 2, b"junk") + fld(1, 2, b"last") + fld(6, 0, _varint(9))
                + fld(3, 2, b"10.0.0.1/8") + fld(8, 2, b"gone") + fld(8, 2, b""),
    "split_props": fld(7, 2, fld(1, 2, b"1ms") + fld(7, 0, b"\5")) + fld(2, 2, b"eth1") + fld(7, 2, fld(6, 2, b"2Mbit") + fld(1, 2, b"3ms")),
    "unknown": UNK + fld(1, 2, b"/ns") + UNK + fld(7, 2, fld(1, 2, b"1ms") + UNK + fld(13, 2, b"2")) + fld(8, 2, b"n") + UNK,
    "wrong_type": fld(1, 0, b"\7") + fld(6, 2, b"xy") + fld(2, 5, b"abcd") + fld(7, 1, b"\0" * 8) + fld(3, 2, b"1.2.3.4/5")
                  + fld(7, 2, fld(7, 2, b"g") + fld(1, 0, b"\1") + fld(4, 2, b"5")) + fld(8, 1, b"\0" * 8),
    **{f"vni_{i}": fld(6, 0, v) + fld(1, 2, b"/ns") for i, v in enumerate(
        (b"\0", _varint(2 ** 31 - 1), b"\xff" * 9 + b"\1", _varint(2 ** 32 + 7), b"\x85\x80\x80\0"))},
}


@pytest.mark.parametrize("case", sorted(STRUCTURE))
def test_field_structure(eng, case):
    plan = check(eng, [body(0), STRUCTURE[case], body(2)], snap=[(-1, b"/other"), (7, b"/ns")])
    if case.startswith("vni_"):
        assert plan[1]["vni"] == (0, 2 ** 31 - 1, -1, 7, 5)[int(case[4:])]


BAD_PROPS = [({"latency": "1xs"}, abi.E_LATENCY), ({"latency_corr": "x"}, abi.E_LATENCY_CORR), ({"jitter": "5"}, abi.E_JITTER),
             ({"loss": "1%"}, abi.E_LOSS), ({"loss_corr": "-"}, abi.E_LOSS_CORR), ({"duplicate": "a"}, abi.E_DUPLICATE),
             ({"duplicate_corr": "1e"}, abi.E_DUPLICATE_CORR), ({"reorder_prob": "."}, abi.E_REORDER_PROB),
             ({"reorder_corr": "0x"}, abi.E_REORDER_CORR), ({"corrupt_prob": "p"}, abi.E_CORRUPT_PROB),
             ({"corrupt_corr": " 1"}, abi.E_CORRUPT_CORR), ({"rate": "fast"}, abi.E_RATE),
             ({"rate": "1Qbit", "jitter": "ms"}, abi.E_JITTER), ({"corrupt_corr": "z", "loss": "z"}, abi.E_LOSS)]
GOOD_PROPS = [{"latency": "", "loss": "", "rate": "", "gap": 0}, None, {"rate": "100kbit"}, {"rate": "1Gibps", "latency": "2ms", "jitter": "1ms"},
              {"rate": "18446744073709551615", "reorder_prob": "25", "gap": 0}, {"latency": "1h", "latency_corr": "50", "jitter": "10us"}]


@pytest.mark.parametrize("ip", ["", "10.0.0.1/24", "10.0.0.1", "junk"])
def test_plans(eng, ip):
    table = BAD_PROPS + [(p, 0) for p in GOOD_PROPS]
    plan = check(eng, [body(m, props=p, intf_ip=ip) for m, (p, _) in enumerate(table)])
    cidr_bad = ip in ("10.0.0.1", "junk")
    assert [int(e) for e in plan["err"]] == [abi.E_REMOTE_CIDR if cidr_bad else code for _, code in table]


BAD = [  # (body, kdtn_wire_err, the Python runtime rejects it too)
    (body(1)[:-1], abi.WIRE_TRUNCATED, True),
    (fld(7, 2, b"\x0a\x05abc"), abi.WIRE_TRUNCATED, True),                # nested length past properties
    (b"\x30" + b"\xff" * 10 + b"\1", abi.WIRE_VARINT, True),              # 11 bytes
    (b"\x30" + b"\xff" * 9 + b"\2", abi.WIRE_VARINT, None),               # literal: the 10th byte above 1
    (fld(1, 2, b"/ns") + b"\x00\x00", abi.WIRE_TAG, True),                # field number 0
    (b"\x0e\x00", abi.WIRE_TAG, True),                                    # wire type 6
    (fld(1, 2, b"\xff"), abi.WIRE_UTF8, True),
    (fld(2, 2, b"\xc3") + fld(2, 2, b"eth0"), abi.WIRE_UTF8, True),       # overridden, still checked
    (fld(7, 2, fld(6, 2, b"1\xffGbit")), abi.WIRE_UTF8, True),
    (fld(8, 2, b"\xed\xa0\x80") + body(1)[:-1], abi.WIRE_UTF8, True),     # the first fault in stream order
    (body(1) + b"\x9b\x01\x9c\x01", abi.WIRE_GROUP, None),                # literal: a well-formed unknown group
]


def test_refusals(eng):
    """One rejected body of each kind between good ones, the neighbours planned in full."""
    bodies, rejected = [body(0)], {}
    for m, (b, code, py) in enumerate(BAD, 1):
        if py:
            with pytest.raises(Exception):
                _C["RemotePod"]().ParseFromString(b)
        rejected[len(bodies)] = code
        bodies += [b, body(m)]
    check(eng, bodies, rejected=rejected)
    assert eng.remote_plan().n_rejected == len(BAD)


def _home(v: int, n: int) -> int:
    """Home slot of a vni in k_rp_vni_build's table of n entries (restated from kdtn_remote.hip)."""
    bits = max(6, (2 * n - 1).bit_length())
    return ((v & 0xFFFFFFFF) * 0x9E3779B1 & 0xFFFFFFFF) >> (32 - bits)


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_conflicts(eng, n):
    crowd = [v for v in range(8000, 400000) if _home(v, n) == _home(V0, n)][:40] if n else []
    assert n == 0 or len(crowd) == 40                                  # forty keys probing from V0's home slot
    snap = ([(V0, NS0)] + [(v, b"/crowd") for v in crowd] + [(-5, b"/neg"), (crowd[3], b"/later"), (V0, b"/later")] if n else [])
    snap = (snap + [(20000 + i, f"/fill/{i}".encode()) for i in range(n)])[:n]
    probe = [(V0, NS0), (V0, NS0[:-1] + b"1"), (V0, NS0[:-1]), (V0, NS0 + b"x"), (V0, b""), (4999, NS0), (-5, b"/neg"), (-5, b"/pos"),
             (crowd[3] if crowd else 9, b"/crowd"), (crowd[39] if crowd else 10, b"/later"), (20000 + n - 1, b"/fill/0")]
    plan = check(eng, [body(m, vni=v, net_ns=ns.decode()) for m, (v, ns) in enumerate(probe)], snap=snap)
    if n == 1000:
        assert list(plan["vni_entry"][:5]) == [0] * 5 and list(plan["vni_conflict"][:5]) == [0, 1, 1, 1, 1]
        assert plan["vni_entry"][8] == 4 and eng.remote_plan().n_conflict == 6


@pytest.mark.parametrize("name,n_msgs", [("segments_rounds", 204), ("props_copy", 228), ("varints", 191)])
def test_round_trip(eng, name, n_msgs):
    """reconcile → encode → remote_encode → download: every marshalled RemotePod, its length varint
    stripped, plans as the sender predicted it."""
    ep = getattr(S, name)()
    inp, out = ep.inp, eng.reconcile(ep.inp)
    eng.encode()
    arena, off, entry, _, _, _ = eng.remote_pods()
    assert len(entry) == n_msgs
    slots = [m for m in range(n_msgs) if off[m + 1] > off[m]]           # an empty slot: the message failed to marshal
    sizes = [S._varint_at(arena, int(off[m])) for m in slots]
    starts = [int(off[m + 1]) - n for m, n in zip(slots, sizes)]
    assert all(s - int(off[m]) == len(_varint(n)) for m, s, n in zip(slots, starts, sizes))
    plan, qd = eng.remote_ingest(arena.tobytes(), starts, sizes)
    compared = 0
    for k, m in enumerate(slots):
        e = int(entry[m])
        r, g = out.add_res[e], plan[k]
        assert (g["wire_err"], g["vni"], g["err"] == abi.E_REMOTE_CIDR) == (0, r["vni"], r["remote_err"] != 0), (m, g, r)
        assert qd[k].tobytes() == out.add_qdisc[e].tobytes(), m
        o, n = g["str"][abi.RP_NAME]
        assert arena[o:o + n].tobytes() == bytes(inp.kdict.get(inp.desired.key[abi.KEY_COLS.index("peer_pod"), out.add_idx[e]])), m
        compared += 1
    assert compared == len(slots) > 0 and min(sizes) >= 0 and max(sizes) <= 16455
