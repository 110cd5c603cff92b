"""kdtn_wire_ingest on the GPU: streams of LinksBatchQuery messages decoded into epoch tables,
against the Python protobuf runtime over the descriptor of tests/wire_pb.py (ParseFromString of
every message, every field compared as strings through the downloaded dictionaries). Two
expectations are literals because that runtime does not pin them: the 10th-byte rule of a
varint and the refusal of groups (include/kdtn.h)."""
import numpy as np
import pytest

from helpers import random_epoch
from kdtn import abi
from kdtn.engine import Engine
from kdtn.model import pack
from wire_pb import _C, _varint

pytestmark = pytest.mark.gpu
ADD, DEL, UPD = abi.BATCH_ADD, abi.BATCH_DEL, abi.BATCH_UPD
WINDOW = 16384                                      # the frame pass's LDS window
POD_FIELDS = ("kube_ns", "name", "src_ip", "net_ns")   # the row's ns / name / src_ip / net_ns
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    with Engine() as e:
        yield e


def fld(fn: int, wt: int, payload: bytes) -> bytes:
    """One hand-assembled field: tag, then the payload (length-prefixed for wire type 2)."""
    return _varint(fn << 3 | wt) + (_varint(len(payload)) + payload if wt == 2 else payload)


def link(i: int, **kw):
    l = _C["Link"](peer_pod=f"p{i}", local_intf=f"eth{i}", peer_intf="e0", local_ip=f"10.0.{i % 200}.1/24",
                   peer_ip="", local_mac="00:00:5e:00:53:01", peer_mac="", uid=i)
    l.properties.SetInParent()
    l.properties.latency, l.properties.rate, l.properties.gap = f"{i}ms", "1Gbit", i % 7
    for k, v in kw.items():
        setattr(l.properties if k in abi.PROP_COLS else l, k, v)
    return l


def msg(n_links: int, m: int = 0, pod=True, **kw) -> bytes:
    q = _C["LinksBatchQuery"]()
    if pod:
        q.local_pod.name, q.local_pod.kube_ns = f"pod{m}", "default"
        q.local_pod.src_ip, q.local_pod.net_ns = f"10.1.0.{m % 250}", f"/run/ns/{m}"
    q.links.extend(link(m * 7 + i, **kw) for i in range(n_links))
    return q.SerializeToString()


def sized(size: int) -> bytes:
    """A message of exactly `size` bytes: 40 links, one peer_pod stretched to fit."""
    pad = size - len(msg(40, peer_pod=""))
    for _ in range(4):
        b = msg(39) + fld(2, 2, link(999, peer_pod="z" * pad).SerializeToString())
        if len(b) == size:
            return b
        pad += size - len(b)
    raise AssertionError("no message of that size")


def decode(eng, msgs, kinds):
    off = np.cumsum([0] + [len(b) for b in msgs]).astype(np.uint64)
    info, err = eng.wire_ingest(b"".join(msgs), off, kinds)
    tab = eng.ingest_tables()
    for d, n in ((tab.kdict, info.n_kdict), (tab.pdict, info.n_pdict)):     # duplicate-free, id 0 = ""
        strs = [bytes(d.get(i)) for i in range(n)]
        assert strs[0] == b"" and len(set(strs)) == n
    return info, err, tab


def check(eng, msgs, kinds, rejected=()):
    """Every message against ParseFromString; rejected ones are empty Topologies."""
    info, err, tab = decode(eng, msgs, kinds)
    T, kd, pd = tab.topos, tab.kdict, tab.pdict
    assert info.n_topos == len(msgs) and not T.flags.any()
    n_des = n_real = 0
    for m, (b, kind) in enumerate(zip(msgs, kinds)):
        q = _C["LinksBatchQuery"]()
        if m not in rejected:
            assert err[m] == 0, (m, err[m])
            q.ParseFromString(b)
        row = [bytes(kd.get(c[m])) for c in (T.ns, T.name, T.src_ip, T.net_ns)]
        assert row == [getattr(q.local_pod, f).encode() for f in POD_FIELDS], m
        side, other = (T.real_off, T.des_off) if kind == DEL else (T.des_off, T.real_off)
        L = tab.realised if kind == DEL else tab.desired
        assert (int(side[m]), int(other[m])) == ((n_real, n_des) if kind == DEL else (n_des, n_real)), m
        assert side[m + 1] - side[m] == len(q.links) and other[m + 1] == other[m], m
        for j, l in enumerate(q.links, int(side[m])):
            got = [bytes(kd.get(L.key[k, j])) for k in range(abi.NKEY)] + \
                  [bytes(pd.get(L.prop[k, j])) for k in range(abi.NPROP)]
            want = [getattr(l, c).encode() for c in abi.KEY_COLS] + \
                   [getattr(l.properties, c).encode() for c in abi.PROP_COLS]
            assert got == want, (m, j)
            assert (int(L.uid[j]), int(L.gap[j])) == (l.uid, l.properties.gap), (m, j)
        n_des, n_real = n_des + (kind != DEL) * len(q.links), n_real + (kind == DEL) * len(q.links)
    assert (info.n_desired, info.n_realised) == (n_des, n_real)
    return info, err


def rev(m) -> bytes:
    """The (singular) fields of a Link or Pod serialized one by one, in reverse order."""
    parts = []
    for d, v in m.ListFields():
        one = type(m)()
        getattr(one, d.name).CopyFrom(v) if d.type == d.TYPE_MESSAGE else setattr(one, d.name, v)
        parts.append(one.SerializeToString())
    return b"".join(reversed(parts))


UNK = fld(15, 0, _varint(300)) + fld(16, 1, b"\1" * 8) + fld(17, 2, b"\xffxyz") + fld(18, 5, b"\2" * 4)
L0, P0 = link(3), link(3).properties
STRUCTURE = {
    "reverse": fld(2, 2, rev(L0)) + fld(2, 2, rev(link(4))) + fld(1, 2, rev(_C["LinksBatchQuery"].FromString(msg(0, 5)).local_pod)),
    "scalar_repeated": fld(2, 2, fld(6, 0, _varint(7)) + fld(2, 2, b"first") + fld(6, 0, _varint(9)) + fld(2, 2, b"last")),
    "split_merge": fld(1, 2, fld(1, 2, b"n1") + fld(2, 2, b"ip1")) + fld(2, 2, fld(7, 2, fld(1, 2, b"1ms") + fld(7, 0, b"\5"))
                   + fld(1, 2, b"peer") + fld(7, 2, fld(6, 2, b"2Mbit") + fld(1, 2, b"3ms"))) + fld(1, 2, fld(2, 2, b"ip2") + fld(4, 2, b"ns")),
    "unknown": UNK + fld(1, 2, fld(1, 2, b"n") + UNK + fld(4, 2, b"k")) + UNK
               + fld(2, 2, fld(1, 2, b"a") + UNK + fld(7, 2, fld(1, 2, b"1ms") + UNK + fld(13, 2, b"2")) + fld(9, 2, b"m")) + UNK,
    "wrong_type": fld(2, 0, b"\7") + fld(1, 5, b"abcd") + fld(2, 2, fld(1, 0, b"\3") + fld(6, 2, b"xy") + fld(2, 2, b"eth") + fld(7, 1, b"\0" * 8)
                                                                 + fld(7, 2, fld(7, 2, b"g") + fld(1, 0, b"\1") + fld(2, 2, b"5"))),
    "scalars": b"".join(fld(2, 2, fld(6, 0, u) + fld(7, 2, fld(7, 0, _varint(g)))) for u, g in
                        ((b"\xff" * 9 + b"\1", 2 ** 32 + 7), (b"\x80" * 9 + b"\1", 2 ** 40), (b"\x85\x80\x80\0", 2 ** 32 - 1))),
}


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_message_counts(eng, n):
    check(eng, [msg(m % 3, m) for m in range(n)], [(ADD, DEL, UPD)[m % 3] for m in range(n)])


def test_message_sizes(eng):
    msgs = [b"", msg(2, 1, pod=False)] + [msg(n, n) for n in (0, 1, 63, 64, 65)] + \
           [next(b for b in (msg(1, i, peer_pod="q" * k) for k in range(1, 40)) if len(b) % 16 == 1) for i in range(17)]
    starts = np.cumsum([0] + [len(b) for b in msgs])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))        # a message start at every offset mod 16
    check(eng, msgs, [ADD] * len(msgs))
    assert eng.wire_plan().n_long == 0


def test_long_messages(eng):
    """Just below and just above the threshold ((start & 15) + size > window), and three windows."""
    msgs = [sized(WINDOW), sized(WINDOW + 1), msg(2, 2), sized(3 * WINDOW + 100), msg(1, 4)]
    assert len(msgs[0]) % 16 == 0                                       # message 1 starts aligned
    check(eng, msgs, [ADD, DEL, ADD, UPD, DEL])
    p = eng.wire_plan()
    assert (p.window_bytes, p.first_long, p.n_long) == (WINDOW, 1, 2)


@pytest.mark.parametrize("n", [0, 1, 24, 25, 127, 128, 16384])
def test_string_lengths(eng, n):
    s = "s" * n
    q = _C["LinksBatchQuery"].FromString(msg(2, 1, peer_pod=s, rate=s))
    for f in POD_FIELDS:
        setattr(q.local_pod, f, f[0] * n)
    check(eng, [msg(1, 0), q.SerializeToString(), msg(2, 3, peer_pod=s)], [ADD, DEL, ADD])


@pytest.mark.parametrize("case", sorted(STRUCTURE))
def test_field_structure(eng, case):
    check(eng, [msg(1, 0), STRUCTURE[case], msg(1, 2)], [ADD, ADD, DEL])


def test_scalar_values(eng):
    _, _, tab = decode(eng, [STRUCTURE["scalars"]], [ADD])
    assert [int(u) for u in tab.desired.uid] == [-1, -2 ** 63, 5]       # 10-byte and over-long varints
    assert [int(g) for g in tab.desired.gap] == [7, 0, 2 ** 32 - 1]     # the low 32 bits


BAD = [  # (message, kdtn_wire_err, the Python runtime rejects it too)
    (msg(2, 1)[:-1], abi.WIRE_TRUNCATED, True),
    (fld(2, 2, b"\x0a\x05abc"), abi.WIRE_TRUNCATED, True),               # nested length past its Link
    (fld(2, 2, b"\x30" + b"\xff" * 10 + b"\1"), abi.WIRE_VARINT, True),  # 11 bytes
    (fld(2, 2, b"\x30" + b"\xff" * 9 + b"\2"), abi.WIRE_VARINT, None),   # literal: the 10th byte above 1
    (fld(2, 2, b"\x00\x00"), abi.WIRE_TAG, True),                        # field number 0
    (b"\x0e\x00", abi.WIRE_TAG, True),                                   # wire type 6
    (fld(2, 2, fld(1, 2, b"\xff")), abi.WIRE_UTF8, True),
    (fld(2, 2, fld(2, 2, b"\xc3") + fld(2, 2, b"eth0")), abi.WIRE_UTF8, True),   # overridden, still checked
    (fld(1, 2, fld(3, 2, b"\xed\xa0\x80")), abi.WIRE_UTF8, True),
    (fld(2, 2, fld(7, 2, fld(6, 2, b"1\xffGbit"))), abi.WIRE_UTF8, True),
    (msg(1, 1) + b"\x9b\x01\x9c\x01", abi.WIRE_GROUP, None),             # literal: a well-formed unknown group
]


def test_refusals(eng):
    """One rejected message of each code between good ones, the neighbours decoded in full."""
    msgs, want = [msg(2, 0)], [0]
    for m, (b, code, py) in enumerate(BAD, 1):
        if py:
            with pytest.raises(Exception):
                _C["LinksBatchQuery"]().ParseFromString(b)
        msgs += [b, msg(1 + m % 3, m)]
        want += [code, 0]
    rejected = set(range(1, len(msgs), 2))
    _, err = check(eng, msgs, [(ADD, DEL, UPD)[m % 3] for m in range(len(msgs))], rejected)
    assert list(err) == want
    assert eng.wire_plan().n_rejected == len(BAD)


def test_dictionary_order(eng):
    """Ids rank by the lowest stream offset of a surviving value; an overridden value ranks nothing."""
    b = fld(2, 2, fld(2, 2, b"gone") + fld(1, 2, b"bb") + fld(2, 2, b"cc")) + fld(1, 2, fld(1, 2, b"aa")) + fld(2, 2, fld(1, 2, b"bb") + fld(3, 2, b"dd"))
    info, _, tab = decode(eng, [b], [ADD])
    assert [bytes(tab.kdict.get(i)) for i in range(info.n_kdict)] == [b"", b"bb", b"cc", b"aa", b"dd"]


def test_round_trip(eng):
    """encode() → download_wire() → wire_ingest(): every batch comes back as the records it was
    encoded from, and run() plans each ADD message as the epoch planned that batch."""
    topos, _ = random_epoch(11, T=96, p_err=0.1)
    inp = pack(topos, [])
    T = inp.topos.n
    out = eng.reconcile(inp)
    eng.encode()
    arena, off, werr = eng.download_wire()
    assert not werr.any()
    kinds = [DEL] * T + [ADD] * T + [UPD] * T
    info, err = eng.wire_ingest(bytes(arena[:int(off[-1])]), off, kinds)
    assert not err.any()
    tab = eng.ingest_tables()
    lists = ((out.del_off, out.del_idx, inp.realised), (out.add_off, out.add_idx, inp.desired), (out.upd_off, out.upd_idx, inp.desired))
    for lst, (boff, bidx, src) in enumerate(lists):
        L, seg = (tab.realised, tab.topos.real_off) if lst == 0 else (tab.desired, tab.topos.des_off)
        for t in range(T):
            idx, m = bidx[int(boff[t]):int(boff[t + 1])], lst * T + t
            assert seg[m + 1] - seg[m] == len(idx), (lst, t)
            for j, i in zip(range(int(seg[m]), int(seg[m + 1])), idx):
                assert [bytes(tab.kdict.get(L.key[k, j])) for k in range(abi.NKEY)] == [bytes(inp.kdict.get(src.key[k, i])) for k in range(abi.NKEY)]
                assert [bytes(tab.pdict.get(L.prop[k, j])) for k in range(abi.NPROP)] == [bytes(inp.pdict.get(src.prop[k, i])) for k in range(abi.NPROP)]
                assert (L.uid[j], L.gap[j]) == (src.uid[i], src.gap[i])
    eng.run()
    eng.sync()
    out2 = eng.download()
    sent = {t for t in range(T) if any(o[t + 1] > o[t] for o in (out.del_off, out.add_off, out.upd_off))}
    compared = 0
    for t in range(T):
        e0, e1, m = int(out.add_off[t]), int(out.add_off[t + 1]), T + t
        f0, f1 = int(out2.add_off[m]), int(out2.add_off[m + 1])
        assert f1 - f0 == e1 - e0 and out2.del_off[m + 1] == out2.del_off[m] and out2.upd_off[m + 1] == out2.upd_off[m]
        for e, f in zip(range(e0, e1), range(f0, f1)):
            r, r2 = out.add_res[e], out2.add_res[f]
            p = int(r["peer_topo"])
            if p == NONE or p not in sent or inp.topos.flags[p] & abi.TOPO_SPEC_NIL:
                continue                                             # the peer is not among the local pods
            compared += 1
            assert [r2[k] for k in ("vni", "kind", "err", "vni_hit", "remote_err")] == [r[k] for k in ("vni", "kind", "err", "vni_hit", "remote_err")]
            assert bytes(tab.kdict.get(r2["vtep"])) == bytes(inp.kdict.get(r["vtep"]))
            p2 = int(r2["peer_topo"])
            assert bytes(tab.kdict.get(tab.topos.name[p2])) == bytes(inp.kdict.get(inp.topos.name[p]))
            assert out2.add_qdisc[f].tobytes() == out.add_qdisc[e].tobytes()
    assert compared >= 10
