"""kdtn_epoch_status_encode on the GPU: the status write-back bodies, json.Marshal(status.links)
as Go 1.19 encoding/json writes them (controllers/topology_controller.go:125-138), byte for byte
against a plain restatement of the format (include/kdtn.h) that works on the uploaded
dictionaries' bytes, and against the oracle's Go-faithful JSON decoder (round trip)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from helpers import random_epoch
from kdtn import abi
from kdtn.delta import build_delta
from kdtn.engine import KdtnError, lib
from kdtn.model import Link, LinkProperties, Topology, pack
from kdtn.tables import Interner
from state import apply_delta, commit, predicted_commit

pytestmark = pytest.mark.gpu
WINDOW = 16384                      # the writer's LDS window
GAP_AFTER = abi.PROP_COLS.index("rate")


# ---- the format, restated ---------------------------------------------------------------------
def go_string(b: bytes) -> bytes:
    out, i = bytearray(b'"'), 0
    while i < len(b):
        c = b[i]
        if c < 0x80:
            if c in b'"\\':
                out += b"\\" + bytes([c])
            elif c in b"\n\r\t":
                out += {10: b"\\n", 13: b"\\r", 9: b"\\t"}[c]
            elif c < 0x20 or c in b"<>&":
                out += b"\\u00%02x" % c
            else:
                out.append(c)
            i += 1
            continue
        ch = None
        for k in (2, 3, 4):                      # the strict decoder is utf8.DecodeRune's validity
            try:
                if len(b[i:i + k].decode("utf-8")) == 1:
                    ch = b[i:i + k]
                    break
            except UnicodeDecodeError:
                pass
        if ch is None:
            out += b"\\ufffd"
            i += 1
        else:
            out += {"\u2028": b"\\u2028", "\u2029": b"\\u2029"}.get(ch.decode(), ch)
            i += len(ch)
    return bytes(out + b'"')


def ref_link(inp, j) -> bytes:
    L, kd, pd = inp.desired, inp.kdict, inp.pdict
    f = [b'"%s":%s' % (n.encode(), go_string(kd.get(L.key[k, j]))) for k, n in enumerate(abi.KEY_COLS)]
    f.append(b'"uid":%d' % int(L.uid[j]))
    p = []
    for k, n in enumerate(abi.PROP_COLS):
        if L.prop[k, j]:
            p.append(b'"%s":%s' % (n.encode(), go_string(pd.get(L.prop[k, j]))))
        if k == GAP_AFTER and L.gap[j]:
            p.append(b'"gap":%d' % int(L.gap[j]))
    return b"{" + b",".join(f) + b',"properties":{' + b",".join(p) + b"}}"


def ref_bodies(inp, written):
    T, out = inp.topos, []
    for t in range(T.n):
        a, b = int(T.des_off[t]), int(T.des_off[t + 1])
        if not written[t]:
            out.append(b"")
        elif a == b:
            out.append(b"null" if T.flags[t] & abi.TOPO_SPEC_NIL else b"[]")
        else:
            out.append(b"[" + b",".join(ref_link(inp, j) for j in range(a, b)) + b"]")
    return out


def check(eng, inp, action, mask, commit_mask=None):
    """Encode with `mask`; the bodies and offsets equal the restatement for the Topologies
    `commit_mask` (default: mask) commits and whose action is not SKIP."""
    cm = np.asarray(mask if commit_mask is None else commit_mask, bool)
    written = cm & (action != abi.ACT_SKIP)
    want = ref_bodies(inp, written)
    nw, nb = eng.status_encode(mask)
    arena, off = eng.status_json()
    assert nw == int(written.sum()) and nb == sum(map(len, want)) == len(arena)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64))
    for t, w in enumerate(want):
        assert arena[int(off[t]):int(off[t + 1])].tobytes() == w, (t, w[:200])
    return arena, off, written


def run(eng, inp):
    eng.upload(inp)
    eng.run()
    eng.sync()
    return eng.download()


def created(links):                              # status nil: CREATED, always written
    return Topology("t", "default", links, None, "10.0.0.1", "/run/ns/a")


def epoch_of(eng, topos):
    inp = pack(topos)
    out = run(eng, inp)
    return inp, out


# ---- strings, numbers, properties --------------------------------------------------------------
SPECIALS = [b'"', b"\\", b"\n", b"\r", b"\t", b"\x00", b"\x08", b"\x0c", b"\x1f", b"<", b">", b"&", b"\x7f",
            "\u2027".encode(), "\u2028".encode(), "\u2029".encode(), "\u00e9".encode(), "\u65e5".encode(),
            "\U0001f642".encode(), b"\x80", b"\xc0\x80", b"\xed\xa0\x80", b"\xf5", b"\xe2\x80"]


@pytest.mark.parametrize("s", SPECIALS, ids=[s.hex() for s in SPECIALS])
def test_special_bytes_first_middle_last_in_both_dictionaries(engine, s):
    forms = [s + b"ab", b"a" + s + b"b", b"ab" + s]          # (the truncated E2 80 is last in forms[2])
    links = [Link(local_intf=f, peer_pod=f + b"k", uid=i, properties=LinkProperties(latency=f, rate=f + b"p"))
             for i, f in enumerate(forms)]
    inp, out = epoch_of(engine, [created(links)])
    check(engine, inp, out.action, None, np.ones(1, bool))


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, WINDOW + 3000])
def test_string_lengths_plain_and_rewritten(engine, n):
    plain, esc = b"x" * n, b"y" * max(n - 1, 0) + b'"' * min(n, 1)
    links = [Link(local_intf=plain, peer_ip=esc, uid=1, properties=LinkProperties(jitter=plain, corrupt_corr=esc)),
             Link(local_intf=b"eth0", uid=2)]
    inp, out = epoch_of(engine, [created(links)])
    check(engine, inp, out.action, None, np.ones(1, bool))


ALL13 = LinkProperties(**{f: "1" + f for f in abi.PROP_COLS}, gap=7)
PROPS = [LinkProperties(), LinkProperties(gap=1), LinkProperties(corrupt_corr="5"), ALL13, LinkProperties(gap=2 ** 32 - 1)]
UIDS = [0, 9, 10, -1, 2 ** 31, 2 ** 63 - 1, -2 ** 63]


def test_numbers_and_property_sets(engine):
    links = [Link(local_intf="e", uid=u, properties=p) for u in UIDS for p in PROPS]
    inp, out = epoch_of(engine, [created(links)])
    check(engine, inp, out.action, None, np.ones(1, bool))


# ---- topology shapes ---------------------------------------------------------------------------
def _links(n, tag):
    return [Link(local_intf=f"eth{i}", local_ip="10.0.0.1/24", peer_pod=f"{tag}-{i}", uid=i + 1,
                 properties=LinkProperties(latency="10ms") if i % 3 == 0 else LinkProperties()) for i in range(n)]


def test_topology_shapes_in_one_epoch(engine):
    one = _links(1, "s")
    shapes = [("nil", None, _links(2, "a")), ("empty", [], _links(2, "b")), ("skip", one, one)]
    shapes += [(f"n{n}", _links(n, f"n{n}"), None) for n in (1, 63, 64, 65)]
    shapes += [("hole", _links(3, "h"), None), ("e2", [], _links(1, "c")), ("e3", None, _links(1, "d")),
               ("windows", _links(400, "w"), None),          # ~60 KB: several windows
               ("big", [Link(local_intf=b"z" * (WINDOW + 100), uid=5), Link(local_intf="after", uid=6)], None),
               ("tail", _links(2, "t"), _links(1, "t"))]
    topos = [Topology(n, "default", sp, st, "10.0.0.1", "/run/ns/a") for n, sp, st in shapes]
    inp, out = epoch_of(engine, topos)
    names = [n for n, _, _ in shapes]
    assert out.action[names.index("skip")] == abi.ACT_SKIP
    mask = np.array([n != "hole" for n in names], np.uint8)
    arena, off, written = check(engine, inp, out.action, mask)
    assert arena[int(off[0]):int(off[1])].tobytes() == b"null" and arena[int(off[1]):int(off[2])].tobytes() == b"[]"
    assert not written[names.index("skip")] and not written[names.index("hole")]
    assert engine.commit(mask) == int(mask.sum())


def test_no_topologies(engine):
    inp = pack([])
    run(engine, inp)
    assert engine.status_encode() == (0, 0)
    arena, off = engine.status_json()
    assert len(arena) == 0 and off.tolist() == [0]


# ---- mask parity, round trip, resident state -----------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_predicted_and_explicit_masks_then_commit(engine, seed):
    topos, vnis = random_epoch(seed, T=150, p_err=0.2)
    inp = pack(topos, vnis)
    out = run(engine, inp)
    pred = predicted_commit(inp, out)
    check(engine, inp, out.action, None, pred)
    check(engine, inp, out.action, pred.astype(np.uint8))
    mask = (np.random.default_rng(seed).random(inp.topos.n) < 0.6).astype(np.uint8)
    check(engine, inp, out.action, mask)
    assert engine.commit(mask) == int(mask.sum())


def _strings(tab, ids):
    return [tab.get(i) for i in ids]


def test_round_trip_through_the_go_faithful_decoder(engine):
    topos, vnis = random_epoch(5, T=120, p_err=0.1)
    inp = pack(topos, vnis)
    out = run(engine, inp)
    mask = np.ones(inp.topos.n, np.uint8)
    engine.status_encode(mask)
    arena, off = engine.status_json()
    body = lambda t: arena[int(off[t]):int(off[t + 1])].tobytes()
    ts = [t for t in range(inp.topos.n) if off[t + 1] > off[t]]
    assert ts == [t for t in range(inp.topos.n) if out.action[t] != abi.ACT_SKIP]
    doc = b'{"items":[' + b",".join(b'{"metadata":{"name":"t%d"},"status":{"links":%s}}' % (t, body(t))
                                    for t in ts) + b"]}"
    err, _, got = O.json_ingest(doc)
    assert err == 0 and got.topos.n == len(ts)
    for i, t in enumerate(ts):
        a, b = int(inp.topos.des_off[t]), int(inp.topos.des_off[t + 1])
        ga, gb = int(got.topos.real_off[i]), int(got.topos.real_off[i + 1])
        assert gb - ga == b - a and bool(got.topos.flags[i] & abi.TOPO_STATUS_NIL) == (body(t) == b"null")
        for j, g in zip(range(a, b), range(ga, gb)):
            L, G = inp.desired, got.realised
            assert _strings(inp.kdict, L.key[:, j]) == _strings(got.kdict, G.key[:, g])
            assert _strings(inp.pdict, L.prop[:, j]) == _strings(got.pdict, G.prop[:, g])
            assert (L.uid[j], L.gap[j]) == (G.uid[g], G.gap[g])


def test_resident_delta_appends_strings_to_both_dictionaries(engine):
    """The escape tables' watermark: strings a delta appends (one of which needs escaping, in
    each dictionary) are scanned by the next encode; the earlier words are kept."""
    kd, pd = Interner(), Interner()
    topos = [Topology(f"t{i}", "default", _links(3, f"r{i}"), None, "10.0.0.1", "/run/ns/a") for i in range(5)]
    a = pack(topos, kdict=kd, pdict=pd)
    out = run(engine, a)
    mask = np.ones(a.topos.n, bool)
    check(engine, a, out.action, mask.astype(np.uint8))
    engine.commit(mask)
    state = commit(a, mask)
    topos[2].status_links = topos[2].spec_links
    topos[2].spec_links = topos[2].spec_links + [
        Link(local_intf=b'new"intf', peer_pod="plain-new", uid=77, properties=LinkProperties(loss=b"1<2", rate="9Mbit"))]
    b = pack(topos, kdict=kd, pdict=pd)
    d = build_delta(a, b, a.kdict.n, a.pdict.n)
    assert b.kdict.n > a.kdict.n and b.pdict.n > a.pdict.n
    engine.upload_delta(d)
    want = apply_delta(state, d)
    engine.run()
    engine.sync()
    out = engine.download()
    assert out.action.tolist() == [abi.ACT_SKIP, abi.ACT_SKIP, abi.ACT_DIFF, abi.ACT_SKIP, abi.ACT_SKIP]
    check(engine, want, out.action, np.ones(5, np.uint8))


def test_errors(engine):
    inp = pack([created(_links(2, "e"))])
    engine.upload(inp)
    with pytest.raises(KdtnError) as e:                        # no run
        engine.status_encode()
    assert e.value.code == abi.EINVAL
    engine.run()
    engine.sync()
    o = abi.StatusJson()
    assert lib().kdtn_epoch_download_status(engine._ctx, C.byref(o)) == abi.EINVAL   # no encode of this run
    nw, nb = engine.status_encode()
    buf, off = np.zeros(nb, np.uint8), np.zeros(2, np.uint64)
    o = abi.StatusJson(buf.ctypes.data, nb - 1, off.ctypes.data, 0)
    assert lib().kdtn_epoch_download_status(engine._ctx, C.byref(o)) == abi.ENOSPC and o.n_bytes == nb
    engine.commit()
    with pytest.raises(KdtnError) as e:                        # after a commit the context needs a run
        engine.status_encode()
    assert e.value.code == abi.EINVAL
