"""kdtn_update_ingest on the GPU: Local.UpdateLinks request bodies decoded and planned per link, against
the Python protobuf runtime over the descriptor of tests/wire_pb.py (ParseFromString of every
message), oracle.parse_cidr, oracle.parse_mac, oracle.make_qdisc (tick 15.625) and a loop for the
cut. Every comparison is exact. As in test_wire_ingest_gpu.py, whose message tables are reused, the
10th-byte rule of a varint and the refusal of groups are literals."""
import numpy as np
import pytest

import oracle as O
import stage_epochs as S
import test_wire_ingest_gpu as W
from kdtn import abi
from kdtn.engine import Engine
from test_remote_ingest_gpu import BAD_PROPS, GOOD_PROPS
from wire_pb import _C, _varint

pytestmark = pytest.mark.gpu
fld = W.fld
WINDOW = 16384                                      # k_ul_plan's LDS window
MAC = "00:00:5e:00:53:01"


@pytest.fixture(scope="module")
def eng():
    with Engine(device=0, tick_in_usec=15.625) as e:
        yield e


def lk(i: int, props=(), **kw):
    """An ordinary Link; props None: no properties field; a dict overrides the varying ones."""
    l = _C["Link"](peer_pod=f"p{i}", local_intf=f"eth{i}", local_ip=f"10.0.{i % 200}.1/24", local_mac=MAC, uid=i)
    if props is not None:
        l.properties.SetInParent()
        for k, v in {"latency": f"{i % 40}ms", "rate": ("", "1Gbit")[i % 2], "gap": i % 4, **dict(props)}.items():
            setattr(l.properties, k, v)
    for k, v in kw.items():
        setattr(l, k, v)
    return l


def batch(links, m: int = 0, pods: int = 1) -> bytes:
    """A LinksBatchQuery: `pods` local_pod occurrences (the second, behind the links, merges into the first)."""
    pod = [_C["Pod"](name=f"pod{m}", net_ns=f"/run/ns/{m}", kube_ns="default"), _C["Pod"](net_ns=f"/run/ns/{m}b", src_ip="10.1.0.1")]
    pod = [fld(1, 2, p.SerializeToString()) for p in pod[:pods]]
    return b"".join(pod[:1]) + b"".join(fld(2, 2, l if isinstance(l, bytes) else l.SerializeToString()) for l in links) + b"".join(pod[1:])


def sized(size: int) -> bytes:
    """A Link of exactly `size` bytes: the peer_pod stretched to fit."""
    pad = size - len(lk(1, peer_pod="").SerializeToString())
    for _ in range(4):
        b = lk(1, peer_pod="z" * pad).SerializeToString()
        if len(b) == size:
            return b
        pad += size - len(b)
    raise AssertionError("no link of that size")


def check(eng, msgs, rejected=()):
    """Every message against ParseFromString / parse_cidr / parse_mac / make_qdisc; returns (msgs, links)."""
    buf = b"".join(msgs)
    M, L, Q = eng.update_ingest(buf, np.cumsum([0] + [len(b) for b in msgs]))
    base = n_cut = 0
    for m, b in enumerate(msgs):
        g = M[m]
        if m in rejected:
            zero = np.zeros(1, abi.UPDATE_MSG_DTYPE)[0]
            zero["wire_err"], zero["link_base"] = rejected[m], base
            assert g.tobytes() == zero.tobytes(), (m, g)
            continue
        q = _C["LinksBatchQuery"].FromString(b)
        n = len(q.links)
        assert (g["wire_err"], g["link_base"], g["n_links"]) == (0, base, n), (m, g)
        assert [buf[o:o + k] for o, k in (g["net_ns"], g["name"])] == [q.local_pod.net_ns.encode(), q.local_pod.name.encode()], m
        cut, cut_err = n, 0
        for j, l in enumerate(q.links):
            r, p = L[base + j], l.properties
            want = O.make_qdisc({**{c: getattr(p, c) for c in abi.PROP_COLS}, "gap": p.gap})
            assert Q[base + j].tobytes() == want.tobytes(), (m, j, Q[base + j], want)
            err = abi.E_VETH_CIDR if l.local_ip and not O.parse_cidr(l.local_ip) else \
                abi.E_VETH_MAC if l.local_mac and not O.parse_mac(l.local_mac) else int(want["err"])
            o, k = r["local_intf"]
            assert buf[o:o + k] == l.local_intf.encode() and (k or not o), (m, j)
            assert (r["uid"], r["msg"], r["index"], r["err"], r["has_props"]) == (l.uid, m, j, err, l.HasField("properties")), (m, j, r)
            if err and cut == n:
                cut, cut_err = j, err
        assert (g["cut"], g["err"]) == (cut, cut_err), (m, g)
        n_cut += cut < n
        base += n
    rep = eng.update_plan()
    assert (rep.window_bytes, rep.n_rejected, rep.n_links, rep.n_cut) == (WINDOW, len(rejected), base, n_cut)
    assert len(M) == len(msgs) and len(L) == len(Q) == base
    return M, L


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_message_counts(eng, n):
    check(eng, [batch([lk(7 * m + i) for i in range(m % 3)], m, pods=m % 4 % 3) for m in range(n)])
    assert (eng.update_plan().n_long, eng.update_plan().n_direct) == (0, 0)


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 129])
def test_links_per_message(eng, k):
    """Segments that start and end inside, at and across wave boundaries; no local_pod, and two that merge."""
    M, _ = check(eng, [batch([lk(1), lk(2)], 0), batch([lk(i) for i in range(k)], 1, pods=0), batch([lk(i) for i in range(3)], 2, pods=2)])
    assert list(M["n_links"]) == [2, k, 3] and tuple(M[1]["net_ns"]) == (0, 0)


IP, MACF, RATE = {"local_ip": "junk"}, {"local_mac": "zz"}, {"props": {"rate": "fast"}}
CUTS = {  # name: ([(links of the message, {index: what fails})], the cuts)
    **{f"only_{k}": ([(130, {k: IP}), (2, {})], [k, 2]) for k in (0, 63, 64, 129)},
    "none": ([(130, {}), (2, {})], [130, 2]),
    "two_waves": ([(130, {100: IP, 10: RATE})], [10]),
    "shared_wave": ([(5, {3: MACF}), (6, {1: RATE, 4: IP})], [3, 1]),
    "between_clean": ([(3, {}), (70, {65: RATE}), (3, {})], [3, 65, 3]),
}


@pytest.mark.parametrize("case", sorted(CUTS))
def test_cut(eng, case):
    spec, cuts = CUTS[case]
    M, _ = check(eng, [batch([lk(i, **fails.get(i, {})) for i in range(n)], m) for m, (n, fails) in enumerate(spec)])
    assert list(M["cut"]) == cuts
    if case == "two_waves":
        assert M[0]["err"] == abi.E_RATE


ORDER = [(dict(local_ip="300.1.1.1/24", local_mac="zz", props={"latency": "1xs"}), abi.E_VETH_CIDR),
         (dict(local_mac="zz", props={"rate": "fast"}), abi.E_VETH_MAC), (dict(local_ip="10.0.0.1"), abi.E_VETH_CIDR),
         (dict(local_ip="", local_mac="00:11"), abi.E_VETH_MAC)] + \
        [(dict(props=p), code) for p, code in BAD_PROPS] + [(dict(props=p), 0) for p in GOOD_PROPS]


def test_error_order(eng):
    """One link per message: MakeVeth's CIDR, then its MAC, then the MakeQdiscs steps; absent and empty properties."""
    M, L = check(eng, [batch([lk(m, **kw)], m) for m, (kw, _) in enumerate(ORDER)])
    assert [int(e) for e in L["err"]] == [int(e) for e in M["err"]] == [code for _, code in ORDER]
    assert list(L["has_props"][-len(GOOD_PROPS):]) == [p is not None for p in GOOD_PROPS]


def _staging():
    aligned = next(p for p in (fld(15, 2, b"x" * k) for k in range(16)) if (len(p) + 1 + len(_varint(WINDOW))) % 16 == 0)
    return {   # name: (messages, n_long, n_direct)
        "two_runs_per_wave": ([batch([lk(32 * m + i, peer_pod="r" * 200) for i in range(32)], m) for m in (0, 1)], 0, 0),
        "window_frames": ([aligned + batch([sized(WINDOW), sized(WINDOW + 1), lk(3)], pods=0), batch([lk(4)], 1)], 1, 1),
        "long_message": ([batch([lk(1)], 0), batch([lk(i) for i in range(3 * WINDOW // 60)], 1), batch([lk(2)], 2)], 1, 0),
        "intf_16k": ([batch([lk(1), lk(2, local_intf="i" * WINDOW), lk(3)])], 1, 1),
    }


@pytest.mark.parametrize("case", ["two_runs_per_wave", "window_frames", "long_message", "intf_16k"])
def test_staging(eng, case):
    msgs, n_long, n_direct = _staging()[case]
    if case == "two_runs_per_wave":
        assert max(map(len, msgs)) < WINDOW < sum(map(len, msgs))
    if case == "long_message":
        assert len(msgs[1]) >= 3 * WINDOW
    check(eng, msgs)
    rep = eng.update_plan()
    assert (rep.n_long, rep.n_direct) == (n_long, n_direct)


STRUCTURE = {**W.STRUCTURE,
             "override": batch([fld(4, 2, b"junk") + fld(8, 2, b"zz") + fld(4, 2, b"10.0.0.1/8") + fld(2, 2, b"eth9") + fld(8, 2, b"")]),
             "uids": batch([fld(6, 0, u) + fld(7, 2, fld(7, 0, _varint(2 ** 32 + 7))) for u in (b"\0", _varint(2 ** 63 - 1), b"\xff" * 9 + b"\1")])}


@pytest.mark.parametrize("case", sorted(STRUCTURE))
def test_field_structure(eng, case):
    _, L = check(eng, [batch([lk(0)], 0), STRUCTURE[case], batch([lk(2)], 2)])
    if case == "uids":
        assert [int(u) for u in L["uid"][1:4]] == [0, 2 ** 63 - 1, -1]


BAD = W.BAD + [(batch([fld(7, 2, b"\x0a\x05abc")]), abi.WIRE_TRUNCATED, True),                  # nested length past properties
               (batch([fld(8, 2, b"\xc3") + fld(8, 2, MAC.encode())]), abi.WIRE_UTF8, True)]   # overridden, still checked


def test_refusals(eng):
    """One rejected message of each kind between good ones: the neighbours planned in full, link_base consistent."""
    msgs, rejected = [batch([lk(0), lk(1)], 0)], {}
    for m, (b, code, py) in enumerate(BAD, 1):
        if py:
            with pytest.raises(Exception):
                _C["LinksBatchQuery"]().ParseFromString(b)
        rejected[len(msgs)] = code
        msgs += [b, batch([lk(i) for i in range(1 + m % 3)], m)]
    check(eng, msgs, rejected)


def test_round_trip(eng):
    """reconcile → encode → download_wire: every Topology's UpdateLinks body plans as the epoch planned its batch."""
    inp = S.sparse_lists().inp
    T = inp.topos.n
    out = eng.reconcile(inp)
    eng.encode()
    arena, off, werr = eng.download_wire()
    assert not werr.any() and len(out.upd_idx) > 3000
    lo = int(off[2 * T])
    M, L, Q = eng.update_ingest(bytes(arena[lo:int(off[3 * T])]), off[2 * T:] - lo)
    assert not M["wire_err"].any() and list(M["link_base"]) == list(out.upd_off[:-1]) and len(Q) == len(out.upd_idx)
    assert Q.tobytes() == out.upd_qdisc.tobytes()
    local = out.upd_res["err"] < abi.E_PEER_LOOKUP                     # no peer-side error
    want = np.where(np.isin(out.upd_res["err"], (abi.E_VETH_CIDR, abi.E_VETH_MAC)), out.upd_res["err"], out.upd_qdisc["err"])
    assert local.any() and (L["err"][local] == want[local]).all()
    assert eng.update_plan().n_long >= 1                               # the hub's 3000 links
