"""Adversarial epochs shaped to reach the size-dependent branches of the output stages
(kdtn_epoch_encode, kdtn_epoch_fanout, kdtn_epoch_remote_encode, kdtn_epoch_tc).

Each composer returns a StageEpoch: the input, `expect` (the branch it is built to reach and
the figures that show it) and the oracle's outputs of every stage (`ref`). A composer proves
that it reaches its branch from the oracle's offsets and sizes alone (assertions inside the
composer: an epoch that misses its branch fails, on the CPU, in tests/test_output_stages_cpu.py);
tests/test_output_stages_gpu.py compares the engine with `ref` byte for byte.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import oracle as O
from kdtn import abi
from kdtn.model import Link, LinkProperties, Topology, pack
from kdtn.tables import EpochInput, Interner

# restated from kdtn_kernels.h and kdtn_encode.h
WIRE_IMG = 8192                  # bytes of a wave's LDS image (wave_image_write; k_tc_remote_write)
REMOTE_IMG = 10240               # k_remote_write's image
SEG_ONE_ROUND = REMOTE_IMG // 4 - 256        # slot dwords that fit one round of 64 lanes (2304)
SEG_HALF = REMOTE_IMG // 4 - 128             # budget of a round of 32 lanes (2432)
KEY_INLINE, KEY_ONE_LOAD, PROP_INLINE = 23, 15, 15   # inline string table entries (SI_KW / SI_PW)
FAN_CHUNK, FAN_NODE_CAP, NODE_BLOCK = 1024, 8192, 4096
TICK = 15.625

KEY_LENGTHS = [0, 1, 3, 4, 15, 16, 17, 22, 23, 24, 31, 32, 33, 36, 127, 128, 254, 255, 256, 16384]
PROP_LENGTHS = [0, 1, 14, 15, 16, 17, 31, 32, 33, 127, 128, 254, 255, 256]
FAN_SIZES = [0, 1, 2, 3, 63, 64, 65, 1000, 8192, 8193]


@dataclass
class Ref:
    """The oracle's outputs of every stage of one epoch."""
    out: object                  # BatchesOut
    wire: tuple                  # (arena, off, err)
    fan: tuple                   # (node, off, idx)
    remote: tuple                # (arena, off, entry, n_remote, tc, tc_off)
    tc: tuple                    # (arena, off)


def reference(inp: EpochInput) -> Ref:
    out = O.reconcile(inp, tick=TICK)
    return Ref(out, O.encode_epoch(inp, out), O.fanout(out, inp.topos.n), O.remote_epoch(inp, out),
               O.tc_epoch(inp, out))


@dataclass
class StageEpoch:
    name: str
    inp: EpochInput
    expect: dict
    ref: Ref
    topos: list = field(default_factory=list)


def _s(tag: str, n: int) -> str:
    """A string of n bytes that starts with tag (distinct tags keep the interner's ids apart)."""
    return ((tag + "-") * (n // (len(tag) + 1) + 1))[:n]


def _lk(k, peer, uid=None, rate="", **kw) -> Link:
    return Link(**{"local_intf": f"e{k}", "peer_intf": f"p{k}", "peer_pod": peer, "uid": k + 1 if uid is None else uid,
                   "properties": LinkProperties(rate=rate), **kw})


def _topo(name, links, status=(), src="10.0.0.1", netns="/run/ns/a", ns="default") -> Topology:
    return Topology(name, ns, None if links is None else list(links), None if status is None else list(status),
                    src, netns)


def _done(name, topos, expect, kdict=None) -> StageEpoch:
    inp = pack(topos, kdict=kdict)
    return StageEpoch(name, inp, expect, reference(inp), topos)


# ---- figures read from the oracle's outputs -------------------------------------------------
def entry_positions(inp: EpochInput, ref: Ref) -> np.ndarray:
    """Byte position of every entry of the global list (del, add, upd; n + 1 values) in the
    oracle's wire arena: a batch's first entry carries the LocalPod header, a failed batch's
    entries hold no bytes. Entry sizes come from or_encode_batch of one- and two-link batches and
    are checked against or_encode_epoch's batch offsets."""
    out, (arena, off, err) = ref.out, ref.wire
    T = inp.topos.n
    sizes = []
    for lst, (offs, idx) in enumerate(((out.del_off, out.del_idx), (out.add_off, out.add_idx),
                                       (out.upd_off, out.upd_idx))):
        for t in range(T):
            e0, e1 = int(offs[t]), int(offs[t + 1])
            if e1 == e0:
                continue
            if err[t] >> lst & 1:
                sizes += [0] * (e1 - e0)
                continue
            first = len(O.encode_batch(inp, t, lst, idx[e0:e0 + 1]))
            mine = [first] + [len(O.encode_batch(inp, t, lst, [idx[e0], idx[e]])) - first for e in range(e0 + 1, e1)]
            assert sum(mine) == int(off[lst * T + t + 1]) - int(off[lst * T + t]), (lst, t)
            sizes += mine
    pos = np.concatenate([[0], np.cumsum(np.array(sizes, np.int64))])
    assert pos[-1] == len(arena)
    return pos


def window_bytes(pos: np.ndarray) -> list[int]:
    """What wave_image_write compares with the image per aligned 64-entry window: the window's
    bytes plus the lead of its first byte."""
    n = len(pos) - 1
    return [int(pos[min(w + 64, n)] - pos[w]) + int(pos[w] & 3) if pos[min(w + 64, n)] > pos[w] else 0
            for w in range(0, n, 64)]


def segment_dwords(off, index_of, n_entries: int):
    """Per aligned 64-entry window of a segments writer: (slot dwords, first half, second half).
    index_of[e] = the entry's message index or -1."""
    res = []
    for w in range(0, n_entries, 64):
        dw = np.zeros(64, np.int64)
        for e in range(w, min(w + 64, n_entries)):
            m = index_of[e]
            if m >= 0 and off[m + 1] > off[m]:
                dw[e - w] = ((int(off[m]) & 3) + int(off[m + 1] - off[m]) + 3) >> 2
        res.append((int(dw.sum()), int(dw[:32].sum()), int(dw[32:].sum())))
    return res


def message_index(ref: Ref, n_add: int) -> np.ndarray:
    inv = np.full(n_add, -1, np.int64)
    inv[ref.remote[2]] = np.arange(len(ref.remote[2]))
    return inv


def _paths(wb) -> list[str]:
    return ["direct" if b > WIRE_IMG else "image" for b in wb]


def _digits(v: int) -> int:
    return len(str(int(v)))


# ---- the image and direct paths of wave_image_write ----------------------------------------
def _wire_windows(pad: int):
    long_ = lambda k, n: _lk(k, "localhost", peer_intf=_s(f"w{k}", n))
    dels = _topo("del0", [], [_lk(k, "localhost") for k in range(32)])
    a0 = _topo("a0", [_lk(k, "localhost") for k in range(32)])                   # window 0: 32 del + 32 add
    a1 = _topo("a1", [long_(0, pad)] + [long_(k, (130, 300, 24, 23)[k % 4]) for k in range(1, 21)]
               + [_lk(k, "localhost") for k in range(21, 30)])
    bad = _topo("bad", [_lk(0, "localhost"), _lk(1, "localhost", local_mac=b"\xff"), _lk(2, "localhost")])
    a2 = _topo("a2", [_lk(k, "localhost") for k in range(31)])                   # window 1 ends here
    a3 = _topo("a3", [long_(k, 300 if k % 3 else 5) for k in range(64)])         # window 2: direct
    a4 = _topo("a4", [long_(k, 131 + k) for k in range(64)])                     # window 3: direct again
    a5 = _topo("a5", [_lk(k, "localhost") for k in range(10)])
    st = [_lk(k, "localhost") for k in range(5)]
    upd = _topo("u0", [_lk(k, "localhost", rate="1Mbit") for k in range(5)], st)
    return [dels, a0, a1, bad, a2, a3, a4, a5, upd]


@functools.lru_cache(maxsize=None)
def image_overflow_wire() -> StageEpoch:
    """Windows 0-3 of the global entry list: 2 KB (del -> add inside it), WIRE_IMG - 64 .. WIRE_IMG
    with a failed batch of three entries in its middle, and two windows above WIRE_IMG."""
    pad = 600
    for _ in range(4):                       # the tuned string's length varint can move the total
        ep = _done("image_overflow_wire", _wire_windows(pad), {})
        wb = window_bytes(entry_positions(ep.inp, ep.ref))
        if WIRE_IMG - 64 <= wb[1] <= WIRE_IMG:
            break
        pad += WIRE_IMG - 20 - wb[1]
    out, (_, off, err) = ep.ref.out, ep.ref.wire
    n_del = len(out.del_idx)
    assert 0 < n_del % 64 and n_del < 64 and len(out.add_idx) > 64 - n_del, "window 0 straddles del -> add"
    assert 0 < wb[0] < WIRE_IMG - 64 and WIRE_IMG - 64 <= wb[1] <= WIRE_IMG and wb[2] > WIRE_IMG and wb[3] > WIRE_IMG
    assert 0 < wb[4] < WIRE_IMG and len(out.upd_idx) == 5
    t_bad = [t.name for t in ep.topos].index("bad")
    assert err[t_bad] == 2 and 64 < n_del + int(out.add_off[t_bad]) and n_del + int(out.add_off[t_bad + 1]) < 128
    ep.expect = {"window_bytes": wb[:5], "path": _paths(wb[:5]), "pad": pad}
    assert ep.expect["path"] == ["image", "image", "direct", "direct", "image"]
    return ep


def _tc_windows(pad: int):
    names = [23, 24, 130, 300]
    w0 = [_lk(k, "peer", rate="1Gbit") for k in range(32)]
    w1 = [_lk(100, "peer", rate="1Gbit", local_intf=_s("t", pad))] + \
         [_lk(100 + k, "peer", rate="20Mbit", local_intf=_s(f"l{k}", names[k % 4]), peer_intf=_s(f"q{k}", names[(k + 1) % 4]))
          for k in range(1, 7)] + [_lk(100 + k, "peer", rate="1Gbit") for k in range(7, 32)]
    w2 = [_lk(200 + k, "peer", rate="7Mibit", local_intf=_s(f"L{k}", 300 if k % 2 else 130), peer_intf=_s(f"Q{k}", 300))
          for k in range(32)]
    w3 = [_lk(300 + k, "peer", rate="1Gbit") for k in range(7)]
    st = [_lk(k, "peer") for k in range(3)]
    return [_topo("a", w0 + w1[:10]), _topo("b", w1[10:] + w2 + w3), _topo("peer", []),
            _topo("u", [_lk(k, "peer", rate="5Kbit") for k in range(3)], st)]


@functools.lru_cache(maxsize=None)
def image_overflow_tc() -> StageEpoch:
    """The tc slots (two per same-node add entry, one per update): windows below, within 64 bytes
    below and above WIRE_IMG, with interface names of 23, 24, 130 and 300 bytes on TBF entries."""
    pad = 100
    for _ in range(4):
        ep = _done("image_overflow_tc", _tc_windows(pad), {})
        wb = window_bytes(ep.ref.tc[1].astype(np.int64))
        if WIRE_IMG - 64 <= wb[1] <= WIRE_IMG:
            break
        pad += WIRE_IMG - 20 - wb[1]
    out = ep.ref.out
    assert (out.add_res["kind"] == abi.KIND_SAME_NODE).all() and out.add_qdisc["has_tbf"].all()
    assert len(ep.ref.tc[1]) - 1 == 2 * len(out.add_idx) + len(out.upd_idx) and len(out.upd_idx) == 3
    assert 0 < wb[0] < WIRE_IMG - 64 and WIRE_IMG - 64 <= wb[1] <= WIRE_IMG and wb[2] > WIRE_IMG and 0 < wb[3] < WIRE_IMG
    sizes = np.diff(ep.ref.tc[1].astype(np.int64))
    assert (sizes[-3:] > 0).all(), "the update slots run tc"
    ep.expect = {"window_bytes": wb, "path": _paths(wb), "pad": pad}
    assert ep.expect["path"] == ["image", "image", "direct", "image"]
    return ep


# ---- the rounds of wave_segments_write<REMOTE_IMG> ----------------------------------------
@functools.lru_cache(maxsize=None)
def segments_rounds() -> StageEpoch:
    """Three aligned windows of 64 add entries: one round of 64 lanes, two rounds of 32, and a
    direct first half with an image second half; entries alternate among five and between two
    destination daemons, one destination's net_ns is not valid UTF-8 (an empty message between
    two others)."""
    dests = [_topo(f"d{k}", [], src=f"10.0.1.{k}", netns=f"/run/ns/d{k}") for k in range(5)]
    dests.append(_topo("dbad", [], src="10.0.1.2", netns=b"/run/\xff"))        # on d2's node
    links = []
    for k in range(64):                                             # window 0: short, five daemons
        links.append(_lk(k, "dbad" if k in (7, 40) else f"d{k % 5}", peer_intf="p" * (1 + k % 4)))
    for k in range(64, 128):                                        # window 1: ~200 bytes, two daemons
        links.append(_lk(k, f"d{k % 2}", peer_intf=_s(f"m{k}", 180 + k % 7), rate="1Gbit"))
    for k in range(128, 192):                                       # window 2: first half ~400 bytes
        links.append(_lk(k, "dbad" if k == 150 else f"d{k % 5}",
                         peer_intf=_s(f"n{k}", 400 + k % 5) if k < 160 else "q" * (1 + k % 3)))
    links += [_lk(k, f"d{k % 3}") for k in range(192, 203)]
    # the shortest RemotePod the format allows: vni 0 (uid -5000), every other field of the link empty
    links.append(Link(peer_pod="d0", uid=-5000))
    senders = [_topo(f"s{i}", links[i:i + 48]) for i in range(0, len(links), 48)]
    ep = _done("segments_rounds", senders + dests, {})
    ref, n_add = ep.ref, len(ep.ref.out.add_idx)
    arena, off, entry, nr = ref.remote[:4]
    assert nr == n_add == len(links), "every add entry sends a RemotePod"
    dw = segment_dwords(off, message_index(ref, n_add), n_add)
    assert dw[0][0] <= SEG_ONE_ROUND
    assert SEG_ONE_ROUND < dw[1][0] <= 2 * SEG_HALF and dw[1][1] <= SEG_HALF and dw[1][2] <= SEG_HALF
    assert dw[2][1] > SEG_HALF and 0 < dw[2][2] <= SEG_HALF
    lens = np.diff(off.astype(np.int64))
    inv = message_index(ref, n_add)
    for w in range(3):
        ms = inv[64 * w:64 * w + 64]
        assert {int(off[m]) & 3 for m in ms if lens[m]} == {0, 1, 2, 3}, "every start alignment"
        assert len({int(x) for x in ref.out.add_res["vtep"][64 * w:64 * w + 64]}) >= (2 if w == 1 else 5)
    empty = [int(inv[e]) for e in (7, 40, 150)]
    assert all(lens[m] == 0 and lens[m - 1] > 0 and lens[m + 1] > 0 for m in empty), "empty between two messages"
    shortest = int(lens[lens > 0].min())
    # kube_ns "default" (9), net_ns, peer_vtep and name are set by the pods: no 1-3 byte message
    assert shortest == int(lens[inv[n_add - 1]])
    ep.expect = {"slot_dwords": dw[:3], "rounds": ["one", "two", "direct+image"], "shortest_message": shortest}
    return ep


# ---- inline string tables ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def string_lengths() -> StageEpoch:
    """Key strings of KEY_LENGTHS in every key column and in the Topology's own name, namespace,
    src_ip and net_ns (and the peer's net_ns); property strings of PROP_LENGTHS in the first, a
    middle (rate, valid: ParseRate trims the padding) and the last property column."""
    topos = [_topo("dst", [], src="10.0.2.1", netns="/run/ns/dst")]
    group, col_of = {}, {}                       # topology index -> its length, its (column, length)
    for L in KEY_LENGTHS:
        ns = _s(f"ns{L}", L)
        name = _s(f"pod{L}", L)
        topos.append(_topo(f"h{L}-dst", [], src="10.0.2.2", netns=_s(f"peer-netns{L}", L) or "/n", ns=ns))
        topos.append(_topo(name, [_lk(0, f"h{L}-dst", rate="1Gbit")], src=_s(f"src{L}", L), netns=_s(f"netns{L}", L), ns=ns))
        group[len(topos) - 1] = L
        for col in abi.KEY_COLS:
            s = _s(f"{col}{L}", L)
            peer = "dst"
            if col == "peer_pod":
                peer = s
                if L:
                    topos.append(_topo(s, [], src="10.0.2.3", netns="/run/ns/p"))
            topos.append(_topo(f"k-{col}-{L}", [_lk(0, peer, rate="1Gbit", **({} if col == "peer_pod" else {col: s}))]))
            group[len(topos) - 1] = L
            col_of[len(topos) - 1] = (col, L)
    for L in PROP_LENGTHS:
        for col in ("latency", "rate", "corrupt_corr"):
            s = " " * (L - 4) + "1000" if col == "rate" and L >= 4 else _s(f"{col}{L}", L)
            l = _lk(0, "dst")
            setattr(l.properties, col, s)
            topos.append(_topo(f"p-{col}-{L}", [l]))
    ep = _done("string_lengths", topos, {})
    kd, pd, ref = ep.inp.kdict, ep.inp.pdict, ep.ref
    klen, plen = np.diff(kd.offs.astype(np.int64)), np.diff(pd.offs.astype(np.int64))
    assert set(KEY_LENGTHS) <= set(klen.tolist()) and set(PROP_LENGTHS) <= set(plen.tolist())
    assert {int(b) & 3 for b in kd.offs[:-1][klen > KEY_INLINE]} == {0, 1, 2, 3}, "long key strings at every b & 3"
    assert {int(b) & 3 for b in pd.offs[:-1][plen > PROP_INLINE]} == {0, 1, 2, 3}
    out = ref.out
    t_of = np.searchsorted(out.add_off, ref.remote[2][:ref.remote[3]], side="right") - 1
    sent = {group[int(t)] for t in t_of if int(t) in group}
    assert sent == set(KEY_LENGTHS), "a RemotePod is sent for every key length"
    rate_sent = {int(plen[ep.inp.desired.prop[abi.PROP_COLS.index("rate"), out.add_idx[e]]])
                 for e in ref.remote[2][:ref.remote[3]]}
    assert {L for L in PROP_LENGTHS if L >= 4} <= rate_sent
    # which strings reach which writer: every Topology here marshals (err bit clear, bytes written),
    # so every length of every column and of the three property columns reaches the wire encoder;
    # a RemotePod needs a link that parses, so local_ip / local_mac strings reach it only when
    # empty, and of the property strings only the padded rates (latency and corrupt_corr strings
    # are not valid values: their links build no qdisc and send nothing)
    _, woff, werr = ref.wire
    T = ep.inp.topos.n
    assert not werr.any() and all(woff[T + t + 1] > woff[T + t] for t in col_of), "every AddLinks batch is written"
    by_col = {c: sorted({col_of[int(t)][1] for t in t_of if int(t) in col_of and col_of[int(t)][0] == c})
              for c in abi.KEY_COLS}
    for c in ("local_intf", "peer_intf", "peer_ip", "peer_mac"):
        assert by_col[c] == sorted(KEY_LENGTHS), c
    assert by_col["peer_pod"] == sorted(KEY_LENGTHS)[1:] and by_col["local_ip"] == by_col["local_mac"] == [0]
    ep.expect = {"key_lengths": KEY_LENGTHS, "prop_lengths": PROP_LENGTHS, "n_remote": ref.remote[3],
                 "remote_lengths_by_column": by_col, "remote_rate_lengths": sorted(rate_sent)}
    return ep


# ---- physical peers ------------------------------------------------------------------------
PHYSICAL = [b"physical/", b"physical/x"] + [b"physical/" + _s("vtep", n).encode() for n in (14, 15, 23, 246, 300)] + \
           [b"physical/\xff"]


@functools.lru_cache(maxsize=None)
def physical_peers() -> StageEpoch:
    """peer_vtep = the name minus "physical/": the bare prefix, names whose trimmed / whole length
    crosses the inline sizes and the one-byte length, and a name that is invalid after the prefix;
    with and without a TBF; one behind a failing link of its batch (not reached)."""
    links = [_lk(k, p, rate="1Gbit" if k % 2 else "") for k, p in enumerate(PHYSICAL)]
    topos = [_topo("phys", links, src="10.0.0.7"), _topo(_s("long-pod", 140), links[2:6], netns=_s("/run/ns/", 130)),
             _topo("cut", [_lk(0, "physical/9.9.9.9", local_ip="bad"), _lk(1, "physical/behind")])]
    ep = _done("physical_peers", topos, {})
    ref, out = ep.ref, ep.ref.out
    arena, off, entry, nr = ref.remote[:4]
    assert nr == 0 and (out.add_res["kind"][entry] == abi.KIND_PHYSICAL).all()
    n0 = len(PHYSICAL)
    lens = np.diff(off.astype(np.int64))
    assert list(entry) == list(range(n0 + 4)), "the entries of `cut` send nothing"
    assert lens[n0 - 1] == 0 and (lens[:n0 - 1] > 0).all() and (lens[n0:] > 0).all()
    assert (np.diff(ref.tc[1].astype(np.int64))[0:2 * n0:2] > 0).tolist() == [bool(k % 2) for k in range(n0)]
    ep.expect = {"n_physical": len(entry), "message_bytes": lens.tolist()}
    return ep


# ---- decimal numbers of the tc argv --------------------------------------------------------
def _rate_candidates():
    vals = set()
    for d in range(1, 21):
        vals |= {10 ** (d - 1), 10 ** d - 1}
    for p in (10 ** 4, 10 ** 8, 10 ** 12, 10 ** 16, 2 ** 32):
        vals |= {p - 1, p, p + 1}
    vals |= {2 ** 64 - 1, 2 ** 64, 250 * (2 ** 32 - 1), 250 * (2 ** 32 - 1) + 249, 250 * 2 ** 32}
    vals |= {250 * 10 ** 4 - 1, 250 * 10 ** 4, 250 * 10 ** 8 - 1, 250 * 10 ** 8, 250 * 5000, 250 * 5001}
    out = []
    for v in sorted(vals):
        out += [str(v), f"{v}bit"]
        if v % 8 == 0:
            out.append(f"{v // 8}bps")
        if v % 8192 == 0:
            out.append(f"{v // 8192}Kibps")
    return out + ["2251799813685247Kibps", "2305843009213693951bps", "18446744073709551615bit"]


@functools.lru_cache(maxsize=None)
def tc_numbers() -> StageEpoch:
    """Rates kept for what the oracle computes from them: every digit count of tbf_rate, both
    sides of the base-10000 limb boundaries and of 2^32, the largest rate; buffers on both sides
    of 10^4 and 10^8 and at their maximum."""
    kept, seen = [], set()
    for s in _rate_candidates():
        q = O.make_qdisc({"rate": s}, tick=TICK)
        if q["err"] or not q["has_tbf"]:
            continue
        key = (int(q["tbf_rate"]), int(q["tbf_buffer"]), s[-3:])
        if key not in seen:
            seen.add(key)
            kept.append(s)
    topos = [_topo("a", [_lk(k, "peer", rate=s) for k, s in enumerate(kept)]), _topo("peer", [])]
    ep = _done("tc_numbers", topos, {})
    q = ep.ref.out.add_qdisc
    assert (ep.ref.out.add_res["kind"] == abi.KIND_SAME_NODE).all() and q["has_tbf"].all() and not q["err"].any()
    rates, bufs, minb = ({int(x) for x in q[f]} for f in ("tbf_rate", "tbf_buffer", "tbf_minburst"))
    digits = sorted({_digits(r) for r in rates})
    assert max(rates) == 2 ** 64 - 1, "the largest rate ParseRate accepts"
    assert digits == list(range(1, _digits(max(rates)) + 1)) and len(digits) >= 10
    for p in (10 ** 4, 10 ** 8, 10 ** 12, 10 ** 16):
        assert {p - 1, p} <= rates, p
    assert {2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1} <= rates
    assert {9999, 10000, 10 ** 8 - 1, 10 ** 8, 2 ** 32 - 1, 5000} <= bufs, "buffer: 10^4, 10^8, its floor and maximum"
    assert minb == {1500}, "MakeQdiscs sets one minburst (qdisc.go:121): no other value exists to cover"
    assert np.diff(ep.ref.tc[1].astype(np.int64)).min() > 0
    ep.expect = {"rate_digits": digits, "n_rates": len(kept), "buffers": len(bufs), "minburst": sorted(minb)}
    return ep


# ---- fan-out -------------------------------------------------------------------------------
def _ip(i: int) -> str:
    return f"10.{1 + (i >> 16)}.{(i >> 8) & 255}.{i & 255}"


@functools.lru_cache(maxsize=None)
def fan_nodes(nn: int) -> StageEpoch:
    """RemotePods to exactly nn destination daemons. Up to 65: 3 * FAN_CHUNK + 37 add entries,
    consecutive senders to different daemons, the second chunk without a sender; above: nn + 1
    one-link Topologies on distinct nodes, destinations a permutation."""
    kd = None
    if nn <= 65:
        n_add = 3 * FAN_CHUNK + 37
        dests = [_topo(f"d{k}", [], src=_ip(k), netns="/n") for k in range(nn)]
        links = [_lk(k, f"d{k % nn}" if nn and not FAN_CHUNK - 24 <= k < 2 * FAN_CHUNK + 76 else "localhost")
                 for k in range(n_add)]
        topos = [_topo(f"s{i}", links[i:i + 97], src="10.0.0.1") for i in range(0, n_add, 97)]
        if nn == 65:                         # the node strings' ids over three NODE_BLOCK-id blocks
            kd = Interner()
            for k in range(nn):
                kd(_ip(k))
                if k in (20, 40):
                    for f in range(NODE_BLOCK + 500):
                        kd(f"filler-{k}-{f}")
        topos = dests + topos
    else:
        N = nn + 1
        d = [1 + (7919 * i) % nn for i in range(nn)] + [1]
        for i in range(N):                   # a self-peer is a same-node link: trade with a neighbour
            if d[i] == i:
                j = (i + 1) % nn
                d[i], d[j] = d[j], d[i]
        topos = [_topo(f"t{i}", [_lk(0, f"t{d[i]}", uid=i + 1)], src=_ip(i), netns="/n") for i in range(N)]
    ep = _done(f"fan_nodes{nn}", topos, {}, kdict=kd)
    node, off, idx = ep.ref.fan
    out = ep.ref.out
    n_add = len(out.add_idx)
    assert len(node) == nn, (len(node), nn)
    if nn <= 65:
        assert n_add > 2 * FAN_CHUNK and n_add % FAN_CHUNK and n_add % 64
        send = np.zeros(n_add, bool)
        send[idx] = True
        assert not send[FAN_CHUNK:2 * FAN_CHUNK].any() and (send[:FAN_CHUNK - 24].all() or nn == 0)
        if nn >= 2:
            v = out.add_res["vtep"][np.flatnonzero(send)]
            assert (v[1:] != v[:-1])[np.diff(np.flatnonzero(send)) == 1].all(), "neighbours to different daemons"
    else:
        assert n_add == nn + 1 == len(idx)
    blocks = len({int(x) // NODE_BLOCK for x in node})
    if nn in (65, 8192):
        assert blocks >= 3
    ep.expect = {"n_nodes": nn, "n_add": n_add, "n_send": len(idx), "id_blocks": blocks,
                 "refused": nn > FAN_NODE_CAP}
    return ep


# ---- UTF-8 validity per field --------------------------------------------------------------
UTF8_BAD = [b"\x80", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
            b"\xf5\x80\x80\x80", b"\xe2\x82", b"a\xff"]          # tests/test_wire_cpu.py::test_utf8_validity_edges
UTF8_OK = ["µ".encode(), "日本".encode(), "🙂".encode(), b"\xf4\x8f\xbf\xbf", b"\xef\xbf\xbf"]
UTF8_PLACES = ("key", "prop", "name", "peer_netns")


@functools.lru_cache(maxsize=None)
def utf8_edges() -> StageEpoch:
    """Every invalid form and the valid 2-, 3- and 4-byte forms, short (inline) and behind 24
    ASCII bytes (long), in a key column, a property column, the LocalPod name and the peer's
    net_ns: one such string per Topology, whose three lists each hold one entry, so the err bits
    tell the place. One Topology has the invalid string in its del list alone."""
    topos, want = [], {}                          # topology index -> (err bits, message empty or None)
    i = 0
    for form in UTF8_BAD + UTF8_OK:
        bad = form in UTF8_BAD
        for s in (form, b"x" * 24 + form):
            for place in UTF8_PLACES:
                i += 1
                peer = f"nd{i}"
                old, upd, add = _lk(0, "dst"), _lk(1, "dst"), _lk(2, peer, rate="1Gbit")
                upd2 = _lk(1, "dst", rate="1Mbit")
                if place == "key":
                    add.peer_intf = s
                elif place == "prop":
                    add.properties.latency_corr = s
                topos.append(_topo(peer, [], src="10.0.3.1", netns=s if place == "peer_netns" else "/run/ns/p"))
                topos.append(_topo(s if place == "name" else f"t{i}", [upd2, add], [old, upd]))
                err = 0 if not bad else {"key": 2, "prop": 2, "name": 7, "peer_netns": 0}[place]
                # a RemotePod carries the key string and the peer's net_ns; an invalid property
                # string builds no qdisc, so its link sends nothing
                empty = None if place == "prop" else bad and place in ("key", "peer_netns")
                want[len(topos) - 1] = (err, empty)
    topos.append(_topo("del-only", [_lk(1, "dst", rate="1Mbit"), _lk(2, "dst")],
                       [_lk(0, "dst", peer_mac=b"\xed\xa0\x80"), _lk(1, "dst")]))
    want[len(topos) - 1] = (1, False)
    topos.append(_topo("dst", [], src="10.0.3.2", netns="/run/ns/dst"))
    ep = _done("utf8_edges", topos, {})
    out, (_, woff, werr) = ep.ref.out, ep.ref.wire
    arena, off, entry, nr = ep.ref.remote[:4]
    inv, lens = message_index(ep.ref, len(out.add_idx)), np.diff(off.astype(np.int64))
    for t, (err, empty) in want.items():
        assert [int(x[t + 1] - x[t]) for x in (out.del_off, out.add_off, out.upd_off)] == [1, 1, 1], t
        assert int(werr[t]) == err, (t, int(werr[t]), err)
        m = inv[out.add_off[t + 1] - 1]
        assert (m < 0) if empty is None else (m >= 0 and (lens[m] == 0) == empty), (t, empty)
    assert all(O.utf8_valid(s) for s in UTF8_OK) and not any(O.utf8_valid(s) for s in UTF8_BAD)
    ep.expect = {"topologies_by_err": {e: sum(1 for w in want.values() if w[0] == e) for e in (0, 1, 2, 7)},
                 "empty_messages": int((lens[:nr] == 0).sum())}
    return ep


# ---- varint boundaries ---------------------------------------------------------------------
UIDS = [0, 1, 127, 128, 16383, 16384, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 35, 2 ** 63 - 1, -1, -2 ** 63,
        -5000, -5001, 2 ** 31 - 5000, 2 ** 31 - 5001, 2 ** 32 - 5000]
GAPS = [0, 1, 127, 128, 16383, 16384, 2 ** 28 - 1, 2 ** 28, 2 ** 32 - 1]
BOUNDS = [127, 128, 16383, 16384]


def _padded_rate(n: int) -> str:
    """A valid rate of n >= 1 bytes (ParseRate trims the white space)."""
    return " " * (n - 1) + "1"


def _varint_at(arena, p: int) -> int:
    v = sh = 0
    while True:
        b = int(arena[p])
        v |= (b & 0x7F) << sh
        if b < 0x80:
            return v
        sh += 7
        p += 1


def _varint_topos(peer="vb"):
    a = [_lk(k, peer, uid=u) for k, u in enumerate(UIDS)]
    for k, g in enumerate(GAPS):
        l = _lk(100 + k, peer)
        l.properties.gap = g
        a.append(l)
    # properties messages of 0 bytes (above), 2 (gap 1: the shortest that is not empty; a message
    # of 1 byte does not exist), 127, 128 and >= 16384 bytes: rate field = 1 + len varint + len
    a += [_lk(200 + k, peer, rate=_padded_rate(n)) for k, n in enumerate((125, 126, 16400))]
    sweep = [_lk(300 + n, peer, rate=_padded_rate(n)) for n in range(60, 135)]
    big = [_lk(1000 + n, peer, rate=_padded_rate(n)) for n in range(16300, 16385)]
    return [_topo(_s("varint-pod", 130), a), _topo("sweep", sweep), _topo("big", big)]


def _varint_checks(ep: StageEpoch):
    import wire_pb
    out, (warena, woff, _) = ep.ref.out, ep.ref.wire
    T = ep.inp.topos.n
    for e, u in enumerate(UIDS):
        assert int(out.add_res["vni"][e]) == O.vni_from_uid(u), u
    assert {0, -1, -2 ** 31, 2 ** 31 - 1} <= {int(v) for v in out.add_res["vni"][:len(UIDS)]}
    assert [int(v) for v in out.add_res["vni"][:len(UIDS)]].count(0) == 2, "uid -5000 and the wrap-around"
    link_sz, prop_sz, head_sz = set(), set(), set()
    for t in range(3):
        q = wire_pb._C["LinksBatchQuery"].FromString(warena[int(woff[T + t]):int(woff[T + t + 1])].tobytes())
        head_sz.add(q.local_pod.ByteSize())
        link_sz |= {l.ByteSize() for l in q.links}
        prop_sz |= {l.properties.ByteSize() for l in q.links}
    arena, off, entry, nr = ep.ref.remote[:4]
    assert nr == len(out.add_idx), "every entry sends"
    body_sz = {_varint_at(arena, int(off[m])) for m in range(nr)}
    assert set(BOUNDS) <= link_sz and set(BOUNDS) <= body_sz, "Link and RemotePod lengths at both boundaries"
    assert {0, 2, 127, 128} <= prop_sz and max(prop_sz) >= 16384 and max(head_sz) >= 128
    gaps = {int(g) for g in ep.inp.desired.gap[out.add_idx]}
    assert set(GAPS) <= gaps
    return {"uids": len(UIDS), "gaps": len(GAPS), "link_bytes": [min(link_sz), max(link_sz)],
            "properties_bytes_unreachable": [1], "local_pod_bytes": max(head_sz)}


@functools.lru_cache(maxsize=None)
def varints() -> StageEpoch:
    """uid / vni / gap values at the varint group boundaries and in the 10-byte negative form,
    vni 0 twice (field 6 dropped); properties, Link, LocalPod and RemotePod lengths on both sides
    of 127/128 and 16383/16384, read back from the oracle's bytes."""
    ep = _done("varints", _varint_topos() + [_topo("vb", [], src="10.0.4.2", netns="/run/ns/vb")], {})
    ep.expect = _varint_checks(ep)
    return ep


# ---- the properties field copied from the wire arena -------------------------------------
# field 7 of the Link = tag + length varint + the LinkProperties bytes: 2 when empty, 4 at the
# least otherwise (a gap below 128), 129 for 127 bytes and 131 for 128. Fields of 3 and of 130
# bytes do not exist in the format; 4 and 131 stand in their place.
PROP_FIELDS = [2, 4, 31, 32, 33, 34, 63, 64, 65, 66, 129, 131, 300, 700]


def _prop_link(k, peer, F: int, shift: int) -> Link:
    l = _lk(k, peer, local_intf="e" * (1 + shift))
    if F == 4:
        l.properties.gap = 1
    elif F > 4:
        n = F - 4 if F <= 129 else F - 5 if F <= 131 + 1 else F - 6     # rate: 1 + varint + n inside the message
        l.properties.rate = _padded_rate(n)
    return l


@functools.lru_cache(maxsize=None)
def props_copy() -> StageEpoch:
    """AddLinks entries that send a RemotePod, their properties field of every PROP_FIELDS size at
    every source alignment of the wire arena (a one-byte longer local_intf shifts it); a
    Topology whose batch fails to marshal (its own net_ns, and an invalid local_mac behind the
    senders) while its RemotePods are valid takes the strings instead."""
    links = [_prop_link(16 * i + n, "pb", F, sh) for i, F in enumerate(PROP_FIELDS)
             for n, sh in enumerate((0, 1, 3, 0, 2, 2, 1, 0, 0, 1, 2, 3, 4, 5, 6, 7))]
    fb = [_lk(0, "pb", rate=_padded_rate(40)), _lk(1, "pb", rate="1Gbit")]
    topos = [_topo(f"pc{i}", links[i:i + 28]) for i in range(0, len(links), 28)]
    topos += [_topo("fallback-netns", fb, netns=b"/run/\xff"),
              _topo("fallback-mac", fb + [_lk(2, "pb", local_mac=b"\xff")]),
              _topo("pb", [], src="10.0.5.2", netns="/run/ns/pb")]
    ep = _done("props_copy", topos, {})
    out, (warena, woff, werr) = ep.ref.out, ep.ref.wire
    pos = entry_positions(ep.inp, ep.ref)
    n_del = len(out.del_idx)
    arena, off, entry, nr = ep.ref.remote[:4]
    cover = {}
    for e in range(len(links)):                   # macs empty: the properties field ends the entry
        j = int(out.add_idx[e])
        g = n_del + e
        import wire_pb
        p = wire_pb._C["LinkProperties"]()
        p.rate, p.gap = ep.inp.pdict.get(int(ep.inp.desired.prop[abi.PROP_COLS.index("rate"), j])).decode(), \
            int(ep.inp.desired.gap[j])
        F = 1 + len(wire_pb._varint(p.ByteSize())) + p.ByteSize()
        psrc = int(pos[g + 1]) - F
        assert warena[psrc] == 0x3A and _varint_at(warena, psrc + 1) == p.ByteSize(), "field 7 of the oracle's Link"
        cover.setdefault(F, set()).add(psrc & 3)
    assert sorted(cover) == PROP_FIELDS, sorted(cover)
    assert all(v == {0, 1, 2, 3} for v in cover.values()), cover
    sent = set(int(x) for x in entry[:nr])
    assert set(range(len(links))) <= sent
    names = [t.name for t in ep.topos]
    lens = np.diff(off.astype(np.int64))
    inv = message_index(ep.ref, len(out.add_idx))
    for nm in ("fallback-netns", "fallback-mac"):
        t = names.index(nm)
        assert werr[t] & 2 and all(lens[inv[e]] > 0 for e in range(int(out.add_off[t]), int(out.add_off[t]) + 2)), nm
    ep.expect = {"field_bytes": PROP_FIELDS, "unreachable_field_bytes": [3, 130], "fallback_batches": 2}
    return ep


# ---- sparse lists: entry_topo_wave_c's fallback, entry_topo_wave's binary search --------------
def window_spans(off: np.ndarray) -> list[int]:
    """Topologies an aligned 64-entry window of a list reaches (first to last entry's)."""
    off = off.astype(np.int64)
    n = int(off[-1])
    first = np.searchsorted(off, np.arange(0, n, 64), side="right") - 1
    last = np.searchsorted(off, np.minimum(np.arange(0, n, 64) + 63, n - 1), side="right") - 1
    return (last - first + 1).tolist()


@functools.lru_cache(maxsize=None)
def sparse_lists() -> StageEpoch:
    """About 5000 Topologies with k del, k add and k upd entries each: k = 1 on every 70th, then
    64 and 65 in a row with one each, 200 without any inside one wave's entries, a hub of 3000
    and single entries after it."""
    counts = [1 if t % 70 == 0 else 0 for t in range(2100)]
    counts += [0] * 7 + [1] * 64 + [0] * 3 + [1] * 65
    counts += [5, 5] + [0] * 200 + [5, 5]
    counts += [3000] + [1] * 100
    counts += [1 if t % 70 == 0 else 0 for t in range(2400)]
    topos = []
    for t, k in enumerate(counts):
        st = [_lk(f"d{i}", "sp", uid=i + 1) for i in range(k)] + [_lk(f"u{i}", "sp", uid=i + 1) for i in range(k)]
        sp = [_lk(f"u{i}", "sp", uid=i + 1, rate="1Gbit") for i in range(k)] + \
             [_lk(f"a{i}", "sp", uid=i + 1, rate="5Kbit" if i % 2 else "") for i in range(k)]
        topos.append(_topo(f"s{t}", sp, st))
    topos.append(_topo("sp", [], src="10.0.6.2", netns="/run/ns/sp"))
    ep = _done("sparse_lists", topos, {})
    out = ep.ref.out
    n = sum(counts)
    assert len(out.del_idx) == len(out.add_idx) == len(out.upd_idx) == n and ep.ref.remote[3] == n
    spans = {f: window_spans(getattr(out, f)) for f in ("del_off", "add_off", "upd_off")}
    for f, sp in spans.items():
        assert max(sp) >= 129 and any(65 <= x < 129 for x in sp) and 1 in sp, (f, sorted(set(sp)))
    ep.expect = {"topologies": len(topos), "entries_per_list": n,
                 "window_spans": sorted(set(spans["add_off"]))}
    return ep


# ---- the other entry points that feed the output stages ----------------------------------
def keep_suffix(ep: StageEpoch):
    """(prefix epoch, kdict_keep, pdict_keep) for uploading ep.inp as an append-only suffix: the
    prefix holds the first strings of both dictionaries and one Topology without links. The keep
    indices are no multiples of 64, and long strings lie before the rounded-down index, between
    it and the index, and after it."""
    from kdtn.tables import Links, StrTab, Topos
    kd, pd = ep.inp.kdict, ep.inp.pdict
    keep = []
    for tab, inline in ((kd, KEY_INLINE), (pd, PROP_INLINE)):
        long_ids = np.flatnonzero(np.diff(tab.offs.astype(np.int64)) > inline)

        def ok(K):
            base = K // 64 * 64
            # (a dictionary of fewer than 64 strings has nothing before the rounded index)
            return K % 64 and ((long_ids < base).any() or tab.n < 64) and \
                ((long_ids >= base) & (long_ids < K)).any() and (long_ids >= K).any()
        K = next((K for K in range(tab.n // 2, tab.n) if ok(K)), None)
        assert K is not None, "no keep index with long strings on both sides"
        keep.append(K)
    assert kd.n >= 64
    cut = lambda tab, K: StrTab(tab.bytes_[:int(tab.offs[K])].copy(), tab.offs[:K + 1].copy())
    one = np.ones(1, np.uint32)
    prefix = EpochInput(cut(kd, keep[0]), cut(pd, keep[1]),
                        Topos(one, one, one, one, np.zeros(1, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32)),
                        Links.empty(), Links.empty())
    return prefix, keep[0], keep[1]


@functools.lru_cache(maxsize=None)
def varints_late():
    """The varints epoch with its peer missing from the table: (input, the peer's late pod row,
    Ref of the run after kdtn_epoch_late_pods in the engine's layout — the oracle over the table
    plus the row, whose Topology has no list, so the arenas are the same and the row's three
    empty batches drop out of the wire offsets)."""
    from helpers import trim, with_rows
    from kdtn.model import late_pod_rows
    kd = Interner()
    topos = _varint_topos()
    inp = pack(topos, kdict=kd)
    n0 = len(kd)
    late = [_topo("vb", [], src="10.0.4.2", netns="/run/ns/late-vb")]
    rows = late_pod_rows(late, kd)
    assert len(kd) > n0, "the row's net_ns is new to the dictionary"
    grown = EpochInput(kd.table(), inp.pdict, inp.topos, inp.realised, inp.desired, inp.vnis)
    first = O.reconcile(grown, tick=TICK)
    assert (first.add_res["err"] == abi.E_PEER_LOOKUP).all()
    full = with_rows(grown, grown.kdict, rows, np.zeros(1, bool))
    r = reference(full)
    T, T1 = grown.topos.n, full.topos.n
    assert (r.out.add_res["peer_topo"] == T).all() and r.remote[3] == len(r.out.add_idx), "resolved by the late row"
    arena, off, err = r.wire
    off = np.concatenate([off[l * T1:l * T1 + T] for l in range(3)] + [off[-1:]])
    ref = Ref(trim(r.out, T), (arena, off, err[:T]), r.fan, r.remote, r.tc)
    ep = StageEpoch("varints_late", full, {}, r, topos)
    ep.expect = _varint_checks(ep)
    return grown, rows, ref


COMPOSERS = {"image_overflow_wire": image_overflow_wire, "image_overflow_tc": image_overflow_tc,
             "segments_rounds": segments_rounds, "string_lengths": string_lengths,
             "physical_peers": physical_peers, "tc_numbers": tc_numbers, "utf8_edges": utf8_edges,
             "varints": varints, "props_copy": props_copy, "sparse_lists": sparse_lists}
COMPOSERS.update({f"fan_nodes{nn}": functools.partial(fan_nodes, nn) for nn in FAN_SIZES})
