"""Adversarial epochs shaped to reach every launch plan of kdtn_epoch_run.

kdtn_epoch_run picks its kernels from the upload's sizes: the comparison build of k_reconcile
(both lists non-empty) or the ticket + look-back build, 1-4 workgroups per chunk (`split`,
from the records per chunk and the share of realised records), and the placement kind. The
random epochs of helpers.random_epoch all land on one plan; the epochs here are composed chunk
by chunk (TPW = 64 Topologies, one k_reconcile chunk) from chunk classes, with the same
adversarial string pools (bad CIDR / MAC / property strings, ghost peers, duplicate keys,
nil vs [] lists), so that each named epoch reaches the plan `expect` states. What an epoch's
shape must satisfy is pinned on the CPU by tests/test_plan_epochs_cpu.py; that it ran the plan
is asserted on the GPU from Engine.plan() by tests/test_launch_plan_gpu.py.
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field

import numpy as np

from helpers import DURS, INTFS, IPS, MACS, PCTS, RATES, random_props
from kdtn import abi
from kdtn.model import Link, LinkProperties, Topology, pack
from kdtn.tables import EpochInput, StrTab, Topos

TPW, CAP, BLOCK = 64, 2048, 256          # kdtn_kernels.h
NONE = abi.NO_PARTIAL_CHUNK


@dataclass
class PlanEpoch:
    name: str
    inp: EpochInput
    classes: list[str]                   # chunk class per chunk ("" when not composed here)
    expect: dict                         # Engine.plan() fields; "split_min": a lower bound
    per_chunk: tuple[int, int] | None = None    # band of (real.n + des.n) // chunks
    topos: list[Topology] = field(default_factory=list)


def _copy(l: Link, **kw) -> Link:
    return Link(**{**l.__dict__, **kw})


class _Gen:
    def __init__(self, seed: int, T: int, p_err: float):
        self.rng = random.Random(seed)
        self.T, self.p_err = T, p_err
        self.names = [f"p{i}" for i in range(T)]

    def mk(self, uid_max: int = 60) -> Link:
        """helpers.random_epoch's link: peers across the whole epoch (other chunks), localhost,
        physical/..., ghosts; bad strings with probability p_err."""
        rng = self.rng
        bad = rng.random() < self.p_err
        return Link(local_intf=rng.choice(INTFS),
                    local_ip=rng.choice(IPS) if bad else rng.choice(IPS[:3]),
                    local_mac=rng.choice(MACS) if bad else rng.choice(MACS[:3]),
                    peer_intf=rng.choice(INTFS),
                    peer_ip=rng.choice(IPS) if bad else rng.choice(IPS[:3]),
                    peer_mac=rng.choice(MACS) if bad else rng.choice(MACS[:2]),
                    peer_pod=rng.choice(self.names + ["localhost", "physical/1.2.3.4", "ghost", "p0"]),
                    uid=rng.randint(1, uid_max), properties=random_props(rng, 0.35 if bad else 0.2))

    def links(self, k: int, uid_max: int = 60) -> list[Link]:
        ls = [self.mk(uid_max) for _ in range(k)]
        if k >= 2 and self.rng.random() < 0.15:         # duplicate key, the count unchanged
            i = self.rng.randrange(k - 1)
            ls[i + 1] = _copy(ls[i], uid=self.rng.randint(1, uid_max))
        return ls

    def topo(self, i: int, spec, status) -> Topology:
        rng = self.rng
        src = rng.choice(["", "10.0.0.1", "10.0.0.2", "10.0.0.3"])
        netns = "" if not src and rng.random() < 0.7 else rng.choice(["/run/ns/a", f"/run/ns/{i}"])
        return Topology(self.names[i], rng.choice(["default", "default", "other", ""]), spec, status, src, netns)

    def edit(self, old: list[Link], p_del=0.15, p_prop=0.2, p_dup=0.05, adds=(0, 0, 1, 2), p_shuffle=0.3,
             uid_max=60) -> list[Link]:
        """random_epoch's spec side of a compared Topology."""
        rng = self.rng
        new = []
        for l in old:
            r = rng.random()
            if r < p_del:
                continue
            nl = _copy(l)
            if r < p_del + p_prop:
                nl.properties = random_props(rng)
            new.append(nl)
            if rng.random() < p_dup:
                new.append(_copy(nl))
        new += [self.mk(uid_max) for _ in range(rng.choice(adds))]
        if rng.random() < p_shuffle:
            rng.shuffle(new)
        return new

    # ---- chunk classes: n Topologies from index i0 --------------------------------------
    def add(self, i0, n, k):
        """bulk-add: status [], spec of k links (k an int or one count per Topology)."""
        ks = [k] * n if isinstance(k, int) else k
        return [self.topo(i0 + i, self.links(ks[i]), []) for i in range(n)]

    def dele(self, i0, n, k, skip_every=0):
        """bulk-del: status of k links, spec nil or []; every skip_every-th row (nil, nil), and
        the row after it (nil, []): CREATED without a record."""
        out = []
        for i in range(n):
            if skip_every and i % skip_every == 1:
                out.append(self.topo(i0 + i, None, None))
            elif skip_every and i % skip_every == 2:
                out.append(self.topo(i0 + i, [], None))
            else:
                out.append(self.topo(i0 + i, None if self.rng.random() < 0.5 else [], self.links(k)))
        return out

    def mixed(self, i0, n, k, k_del=2, created_links=True):
        """bulk-mixed: add rows, del rows, CREATED rows (status nil; with links they emit none
        of their records, so the chunk is partial without a comparison) and SKIP rows."""
        out = []
        for i in range(n):
            m = i % 8
            if m == 5:
                out.append(self.topo(i0 + i, None if i % 16 == 5 else [], self.links(k_del)))
            elif m == 6:
                out.append(self.topo(i0 + i, self.links(k) if created_links else [], None))
            elif m == 7:
                out.append(self.topo(i0 + i, *((None, None) if i % 16 == 7 else ([], []))))
            else:
                out.append(self.topo(i0 + i, self.links(k), []))
        return out

    def fast(self, i0, n, sizes=(0, 1, 2, 3, 5)):
        """compare-fast: random_epoch-style Topologies; the first one holds a del, an add and
        an upd entry whatever the seed."""
        rng = self.rng
        a, b, c, d = (_copy(self.mk(), local_intf=f) for f in ("cf0", "cf1", "cf2", "cf3"))
        a.properties = LinkProperties(latency="5ms")
        out = [self.topo(i0, [_copy(a, properties=LinkProperties(latency="10ms")), b, d], [a, b, c])]
        for i in range(1, n):
            old = self.links(rng.choice(sizes))
            new = [_copy(l) for l in old] if rng.random() < 0.15 else self.edit(old)
            if rng.random() < 0.05 and old:
                old.append(_copy(old[0]))
            out.append(self.topo(i0 + i, None if rng.random() < 0.08 else new, None if rng.random() < 0.1 else old))
        return out

    def windows(self, i0, n, ko=6, kn=28):
        """compare-windows: mid-size Topologies, none above CAP, the chunk's sum above it."""
        out = []
        for i in range(n):
            old = self.links(ko)
            new = self.edit(old, adds=(0,), p_dup=0.1)
            new += [self.mk() for _ in range(max(0, kn - len(new)))]
            if self.rng.random() < 0.3:
                self.rng.shuffle(new)
            out.append(self.topo(i0 + i, new, old))
        return out

    def hub(self, i0, n, big=CAP + 8, at=5, k=3):
        """compare-hub: one Topology whose lists are both larger than CAP (global scratch)."""
        rng = self.rng
        out = self.add(i0, n, k)
        old = self.links(big, 10**6)
        new = self.edit(old, p_del=0.005, p_prop=0.02, p_dup=0.003, adds=(30,), p_shuffle=0.0, uid_max=10**6)
        for _ in range(20):                              # local reorders: positional compares differ
            j = rng.randrange(len(new) - 1)
            new[j], new[j + 1] = new[j + 1], new[j]
        out[at] = self.topo(i0 + at, new, old)
        return out

    def vnis(self):
        rng = self.rng
        return [(rng.choice(["10.0.0.1", "10.0.0.2", "10.0.0.3"]), 5000 + rng.randint(1, 60),
                 rng.choice(["/run/ns/a", f"/run/ns/{rng.randint(0, self.T)}", ""])) for _ in range(rng.randint(10, 40))]


def _spread(total: int, n: int) -> list[int]:
    return [total // n + (i < total % n) for i in range(n)]


def compose(name, seed, chunks, expect, total=None, per_chunk=None, p_err=0.15) -> PlanEpoch:
    """chunks: (class, Topologies, options) per chunk; every chunk but the last holds TPW
    Topologies. ("add", n, {}) chunks without k share what `total` records leave over."""
    assert all(n == TPW for _, n, _ in chunks[:-1]) and 0 < chunks[-1][1] <= TPW
    i0s = np.concatenate([[0], np.cumsum([n for _, n, _ in chunks])]).tolist()
    g = _Gen(seed, i0s[-1], p_err)
    built: list = [None] * len(chunks)
    fill = [c for c, (cls, n, o) in enumerate(chunks) if cls == "add" and "k" not in o]
    for c, (cls, n, o) in enumerate(chunks):
        if c not in fill:
            built[c] = getattr(g, cls)(i0s[c], n, **o)
    if fill:
        have = sum(len(t.status_links or []) + len(t.spec_links or []) for b in built if b for t in b)
        ks = _spread(total - have, sum(chunks[c][1] for c in fill))
        for c in fill:
            n = chunks[c][1]
            built[c], ks = g.add(i0s[c], n, ks[:n]), ks[n:]
    topos = [t for b in built for t in b]
    return PlanEpoch(name, pack(topos, g.vnis()), [cls for cls, _, _ in chunks], expect, per_chunk, topos)


def _plan(diff_build, split=None, split_min=None, first_partial=NONE, place=None):
    e = {"diff_build": diff_build, "first_partial_chunk": first_partial,
         "place": (abi.PLACE_PARTS if diff_build else abi.PLACE_NONE) if place is None else place}
    if split is not None:
        e["split"] = split
    if split_min is not None:
        e["split_min"] = split_min
    return e


A, F = ("add", TPW, {}), ("fast", TPW, {})
_TAIL = [F, A, ("mixed", TPW, {"k": 8}), ("windows", TPW, {}), ("hub", TPW, {})]


def _split_diff(name, seed, split, n_prefix, n_after, per, last=37):
    """prefix of bulk-add chunks, compare-fast (the first partial chunk), bulk-add, bulk-mixed,
    compare-windows, compare-hub, bulk-add chunks."""
    chunks = [A] * n_prefix + _TAIL + [A] * (n_after - 1) + [("add", last, {})]
    lo, hi = (300 * split, 300 * (split + 1) if split < 4 else 10**9)
    return compose(name, seed, chunks, _plan(1, split=split, first_partial=n_prefix),
                   total=per * len(chunks), per_chunk=(lo, hi))


def _ragged(x: int):
    return ("add", TPW, {"k": _spread(x, TPW)})


RAGGED_ODD = 777                          # odd, no multiple of 64


def _named(name: str) -> PlanEpoch:
    if name == "split2_diff":
        return _split_diff(name, 101, 2, 6, 5, 860)
    if name == "split3_diff":
        return _split_diff(name, 102, 3, 4, 3, 1110)
    if name == "split4_diff":
        return _split_diff(name, 103, 4, 3, 1, 1500)
    if name == "split4_ragged":
        chunks = [A, _ragged(2), A, _ragged(RAGGED_ODD), _ragged(4 * BLOCK), A] + _TAIL + [("add", 37, {})]
        return compose(name, 104, chunks, _plan(1, split=4, first_partial=6), total=1350 * len(chunks),
                       per_chunk=(1200, 10**9))
    if name == "split4_default":
        mid = ("mixed", TPW, {"k": 20, "k_del": 0})      # CREATED rows, spec-nil rows without records
        chunks = [A] * 4 + [mid] + [A] * 3 + [("add", 50, {})]
        return compose(name, 105, chunks, _plan(0, split=4, first_partial=4), total=1300 * len(chunks),
                       per_chunk=(1200, 10**9))
    if name == "teardown":
        chunks = [("dele", TPW, {"k": 9, "skip_every": 7})] * 5 + [("dele", 21, {"k": 4, "skip_every": 5})]
        return compose(name, 106, chunks, _plan(0, split=1), per_chunk=None)
    if name == "all_prefix_diff":
        chunks = [A, A, ("mixed", TPW, {"k": 9, "created_links": False}), A, ("dele", TPW, {"k": 2, "skip_every": 9}),
                  A, A, ("add", 11, {})]
        return compose(name, 107, chunks, _plan(1, split_min=2), total=700 * len(chunks), per_chunk=(600, 10**9))
    if name == "no_prefix":
        chunks = [F, A, A, ("mixed", TPW, {"k": 8}), A, ("dele", TPW, {"k": 1}), ("add", 64, {})]
        return compose(name, 108, chunks, _plan(1, split_min=2, first_partial=0), total=720 * len(chunks),
                       per_chunk=(600, 10**9))
    raise KeyError(name)


NAMED = ["split2_diff", "split3_diff", "split4_diff", "split4_ragged", "split4_default", "teardown",
         "all_prefix_diff", "no_prefix"]
SWEEP = [4 * k + d for k in (64, 256) for d in (-1, 0, 1)]     # chunk totals around the part boundaries


@functools.lru_cache(maxsize=None)
def named(name: str) -> PlanEpoch:
    return _named(name)


@functools.lru_cache(maxsize=None)
def sweep(x: int) -> PlanEpoch:
    """split4_ragged's prefix with a bulk chunk of x records between full ones, a compare-fast
    chunk after it (so the comparison build runs): split 4, the parts of the x-record chunk
    take ceil(x / 4) records each, the last one what is left."""
    chunks = [A, _ragged(x), A, F]
    return compose(f"sweep{x}", 200 + x, chunks, _plan(1, split=4, first_partial=3), total=1400 * len(chunks),
                   per_chunk=(1200, 10**9))


# ---- the mid-size epoch of the wave-per-chunk placement ------------------------------------
PLACE_WAVE_PODS = 70_000       # 1094 chunks >= 4 x 256 CUs


def _perturb(inp: EpochInput, seed: int, frac: float = 0.02) -> EpochInput:
    """Seeded numpy edits on about `frac` of the Topologies of a synthetic epoch: a duplicate
    key, two records of a spec list swapped, property ids pointed at error strings, nil flags
    on empty lists. An edit a Topology's lists cannot take is skipped."""
    rng = np.random.default_rng(seed)
    T = inp.topos
    real = inp.realised.take(np.arange(inp.realised.n))
    des = inp.desired.take(np.arange(inp.desired.n))
    flags = T.flags.copy()
    # the error strings, appended to the property dictionary
    errs = [s for s in dict.fromkeys(PCTS + DURS + RATES) if s]
    extra = StrTab.from_list(errs)
    P0 = inp.pdict.n
    pdict = StrTab(np.concatenate([inp.pdict.bytes_, extra.bytes_]),
                   np.concatenate([inp.pdict.offs, extra.offs[1:] + inp.pdict.offs[-1]]).astype(np.uint32))
    picks = rng.choice(T.n, size=int(T.n * frac), replace=False)
    kinds = rng.integers(0, 4, size=len(picks))
    for t, kind in zip(picks.tolist(), kinds.tolist()):
        r0, r1, d0, d1 = int(T.real_off[t]), int(T.real_off[t + 1]), int(T.des_off[t]), int(T.des_off[t + 1])
        if kind == 0:                                    # duplicate key in the spec or status list
            L, a, b = (des, d0, d1) if rng.random() < 0.5 else (real, r0, r1)
            if b - a >= 2:
                i = int(rng.integers(a, b - 1))
                L.key[:, i + 1] = L.key[:, i]
                L.uid[i + 1] = L.uid[i]
        elif kind == 1 and d1 - d0 >= 2:                 # two spec records swapped
            i, j = (int(x) for x in rng.choice(np.arange(d0, d1), size=2, replace=False))
            for col in (des.key, des.prop):
                col[:, [i, j]] = col[:, [j, i]]
            for col in (des.uid, des.gap):
                col[[i, j]] = col[[j, i]]
        elif kind == 2 and d1 > d0:                      # error strings as property values
            i = int(rng.integers(d0, d1))
            for f in rng.choice(abi.NPROP, size=2, replace=False).tolist():
                des.prop[f, i] = P0 + int(rng.integers(0, len(errs)))
        elif kind == 3:                                  # nil instead of [] where the list is empty
            if r1 == r0:
                flags[t] |= abi.TOPO_STATUS_NIL
            if d1 == d0:
                flags[t] |= abi.TOPO_SPEC_NIL
    topos = Topos(T.ns, T.name, T.src_ip, T.net_ns, flags, T.real_off, T.des_off)
    return EpochInput(inp.kdict, pdict, topos, real, des, inp.vnis, pod_slice=inp.pod_slice,
                      pod_base=inp.pod_base, owner=inp.owner)


@functools.lru_cache(maxsize=None)
def place_wave_adversarial() -> PlanEpoch:
    from kdtn import synth
    inp = _perturb(synth.make(3, pods_per_shard=PLACE_WAVE_PODS), 4242)
    return PlanEpoch("place_wave_adversarial", inp, [], _plan(1, split=1, first_partial=None, place=abi.PLACE_WAVE))


# ---- host restatement of the shape's definitions -------------------------------------------
def needs_comparison(inp: EpochInput) -> np.ndarray:
    """Per Topology: both lists non-empty."""
    T = inp.topos
    return (np.diff(T.real_off.astype(np.int64)) > 0) & (np.diff(T.des_off.astype(np.int64)) > 0)


def chunk_records(inp: EpochInput) -> np.ndarray:
    T = inp.topos
    w = T.real_off.astype(np.int64) + T.des_off.astype(np.int64)
    edges = np.append(np.arange(0, T.n, TPW), T.n)
    return w[edges[1:]] - w[edges[:-1]]


def first_partial_chunk(inp: EpochInput, ora) -> int:
    """The first chunk with a Topology not known to emit every record: one that needs a
    comparison, or — from the oracle's output — one whose entries are not all of its records
    (a Topology without records is full whatever its action)."""
    T = inp.topos
    ko, kn = np.diff(T.real_off.astype(np.int64)), np.diff(T.des_off.astype(np.int64))
    nd, na, nu = (np.diff(getattr(ora, f).astype(np.int64)) for f in ("del_off", "add_off", "upd_off"))
    full = ((ora.action == abi.ACT_DIFF) | (ko + kn == 0)) & (nd == ko) & (na == kn) & (nu == 0)
    part = np.flatnonzero(needs_comparison(inp) | ~full)
    return int(part[0]) // TPW if len(part) else NONE
