"""Replay under changing leaf data: a replay that cannot pass for a no-op.

tn_net_add_leaf_dev imports a device buffer without copying and a captured
graph reads through that pointer, so new contents in the same buffer must
give the new result whether the call walks normally, captures or replays
(include/tnc_hip.h). Every test here changes the leaves between calls.

The scheme. Two nets share the same leaf buffers (tests/devnet.py):
  T  has the 256 MiB arena ContractionEngine reserves so that capture arms;
  R  has no arena. Capture arms only with an arena, and so does the prepack,
     so every call on R is a normal walk: R.state() == (0, 0) throughout.
A step is: load a version; T.poison() (NaNs over T's final tensor); the
operation on T; the same operation on R. Labels must be equal, values equal
bit for bit with no NaN anywhere, and T's replay state
(tn_net_replay_state) what the step says. T and R run the same kernels on
the same bytes (test_gpu_prepack asserts the prepack changes no bit; split-K,
the dots and the slice accumulate use no atomics), so there is no tolerance.
T's first call is itself a normal walk and is compared the same way, which
separates "arena or not" from "replay or walk".

R against the oracle, once per (structure, dtype, version): the suite's bar,
max|got - ref| <= rtol * max|ref| with rtol 1e-10 (c128) and 2e-3 (c64).

The versions. v0 is the network's own data; v1.. are base + 0.25 * (N(0,1)
+ i N(0,1)) elementwise from a fixed seed, cast to the dtype. For every pair
of versions of a structure the oracle results differ by more than 100 times
that tolerance and max|ref| > 0: asserted below from the oracle values, so a
stale result cannot pass for a fresh one.
"""

import functools
import os
import sys

import numpy as np
import pytest

from oracle import contract_network
from oracle.core import OTensor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from devnet import NPDTYPE, NetSpec  # noqa: E402

pytestmark = pytest.mark.gpu

ARENA = 256 * 1024 * 1024
RTOL = {"c128": 1e-10, "c64": 2e-3}
NVERSIONS = 6
SEED = 20261021
# 5 bitstrings over 9 qubits, 3 open: the final tensor is 5 x 8
STRINGS = ["01*1101**", "11*0001**", "00*0000**", "10*0101**", "01*1010**"]
DTYPES = ["c128", "c64"]


class Case:
    """One structure: its flat network, the data versions and their oracle
    results. Built once per session; nothing here touches the GPU."""

    def __init__(self, name, tn, replace, slice_labels=None, nassign=0,
                 batch_labels=(), alt=None):
        self.name = name
        self.spec = NetSpec(tn, replace)
        self.pairs = self.spec.pairs
        self.alt_pairs = None if alt is None else self.spec.pairs_of(alt)
        self.slice_labels = slice_labels
        self.nassign = nassign
        self.batch_labels = list(batch_labels)
        # every version is held to the oracle: it takes milliseconds on the
        # host for each of these structures, rqc24 included
        self.oracle_versions = list(range(NVERSIONS))
        self._noise = {}
        self._refs = {}

    def version(self, dtype, v):
        """The leaves' arrays of version v, in the dtype."""
        if v == 0:
            return [a.astype(NPDTYPE[dtype]) for a in self.spec.base]
        if v not in self._noise:
            rng = np.random.default_rng([SEED, v])
            self._noise[v] = [
                rng.standard_normal(a.shape) + 1j * rng.standard_normal(a.shape)
                for a in self.spec.base
            ]
        return [(a + 0.25 * n).astype(NPDTYPE[dtype])
                for a, n in zip(self.spec.base, self._noise[v])]

    def _oracle(self, arrays):
        labels = [spec[0] for spec in self.spec.leaf_specs]
        if not self.batch_labels:
            ref = contract_network(
                [OTensor(l, a) for l, a in zip(labels, arrays)], self.pairs)
            return list(ref.legs), np.asarray(ref.data)
        # a batch label is kept, not summed: row r is the contraction of the
        # leaves with the label fixed at r
        (beta,) = self.batch_labels
        nrows = {a.shape[l.index(beta)]
                 for l, a in zip(labels, arrays) if beta in l}
        (nrows,) = nrows
        rows, legs = [], None
        for r in range(nrows):
            ts = []
            for l, a in zip(labels, arrays):
                if beta in l:
                    at = l.index(beta)
                    a = np.take(a, r, axis=at)
                    l = l[:at] + l[at + 1:]
                ts.append(OTensor(l, a))
            ref = contract_network(ts, self.pairs)
            assert legs is None or legs == list(ref.legs)
            legs = list(ref.legs)
            rows.append(np.asarray(ref.data))
        return [beta] + legs, np.stack(rows)

    def ref(self, dtype, v):
        """(labels, complex128 array): the oracle on version v as the dtype
        holds it."""
        if (dtype, v) not in self._refs:
            arrays = [a.astype(np.complex128) for a in self.version(dtype, v)]
            self._refs[(dtype, v)] = self._oracle(arrays)
        return self._refs[(dtype, v)]

    def assert_distinguishable(self, dtype):
        """Every two versions differ by more than 100 times the tolerance: a
        stale result is told from a fresh one."""
        vs = self.oracle_versions
        top = {v: float(np.max(np.abs(self.ref(dtype, v)[1]))) for v in vs}
        for v in vs:
            assert top[v] > 0, (self.name, dtype, v)
        for x, a in enumerate(vs):
            for b in vs[x + 1:]:
                gap = float(np.max(np.abs(self.ref(dtype, a)[1]
                                          - self.ref(dtype, b)[1])))
                need = 100 * RTOL[dtype] * max(top[a], top[b])
                assert gap > need, (self.name, dtype, a, b, gap, need)


@functools.lru_cache(maxsize=None)
def case(name):
    from tnc_amd import Greedy, RandomGreedy
    from tnc_amd.builders import random_circuit, sycamore_circuit
    from tnc_amd.connectivity import ConnectivityLayout
    from tnc_amd.contraction_path import ContractionPath
    from tnc_amd.fixtures import load_fixture

    if name == "rqc24":
        tn, toplevel, _ = load_fixture("rqc24")
        return Case(name, tn, ContractionPath.simple(toplevel))
    if name == "sv9":
        tn, _ = sycamore_circuit(9, 4, 7).into_statevector_network()
        p = Greedy().find_path(tn).replace_path()
        q = RandomGreedy(8, seed=5).find_path(tn).replace_path()
        c = Case(name, tn, p, alt=q)
        assert c.alt_pairs != c.pairs
        return c
    if name == "eagle16":
        from tnc_amd.slicing import _walk_sizes, find_slice_edges

        tn = random_circuit(16, 14, 0.5, 0.8, 3, ConnectivityLayout.EAGLE)
        p = Greedy().find_path(tn).replace_path()
        peak, _, _ = _walk_sizes(tn, p.toplevel)
        edges, _ = find_slice_edges(tn, p.toplevel, peak / 4, max_edges=4)
        assert len(edges) == 2
        return Case(name, tn, p, slice_labels=list(edges), nassign=4)
    if name == "three-leaf":
        from test_gpu_sliced_net import _three_leaf_network

        tn, edges, _, _ = _three_leaf_network()
        return Case(name, tn, ContractionPath.simple([(0, 1), (0, 2)]),
                    slice_labels=list(edges), nassign=6)
    if name == "amps":
        single, _ = sycamore_circuit(9, 4, 7).into_amplitude_network(
            STRINGS[0])
        p = Greedy().find_path(single).replace_path()
        tn, _, beta = sycamore_circuit(9, 4, 7).into_amplitudes_network(
            STRINGS)
        return Case(name, tn, p, batch_labels=[beta])
    raise KeyError(name)


def same_bits(got, want):
    """Equal labels, equal bytes, and no NaN on either side."""
    (gl, gd), (wl, wd) = got, want
    assert gl == wl, (gl, wl)
    assert gd.dtype == wd.dtype and gd.shape == wd.shape
    assert not np.isnan(gd).any(), "NaN in the arena net's result"
    assert not np.isnan(wd).any(), "NaN in the reference walk's result"
    assert gd.tobytes() == wd.tobytes(), (
        "max |difference|", float(np.max(np.abs(gd - wd))))


def within_oracle(c, dtype, v, got, what):
    labels, data = got
    ref_labels, ref = c.ref(dtype, v)
    if c.batch_labels:
        # the batched walk stores the batch label ahead of the other legs
        assert sorted(labels) == sorted(ref_labels) and len(set(labels)) == \
            len(labels), (what, labels, ref_labels)
        ref = np.transpose(ref, [ref_labels.index(l) for l in labels])
        ref_labels = labels
    assert labels == ref_labels, (what, labels, ref_labels)
    assert data.shape == ref.shape
    err = float(np.max(np.abs(data.astype(np.complex128) - ref)))
    bound = RTOL[dtype] * float(np.max(np.abs(ref)))
    print(f"{c.name} {dtype} v{v} {what}: max|got-ref| {err:.3e} "
          f"bound {bound:.3e}")
    assert err <= bound, (c.name, dtype, v, what, err, bound)


_ORACLE_DONE = set()


class Pair:
    """T (arena) and R (no arena) over one set of leaf buffers."""

    def __init__(self, c, dtype):
        self.c, self.dtype = c, dtype
        self.R = self.T = None
        self.R = c.spec.devnet(dtype)
        try:
            self.T = c.spec.devnet(dtype, arena_bytes=ARENA, share=self.R)
            assert self.T.cached() >= ARENA
            self._reference_walk_checked()
            self.load(0)
        except BaseException:
            self.close()
            raise

    def _reference_walk_checked(self):
        """Once per (structure, dtype): the versions are distinguishable, and
        R's walk is within the suite's bar of the oracle on each of them."""
        c, dtype, R = self.c, self.dtype, self.R
        if (c.name, dtype) in _ORACLE_DONE:
            return
        c.assert_distinguishable(dtype)
        for v in c.oracle_versions:
            R.load(c.version(dtype, v))
            if c.batch_labels:
                within_oracle(c, dtype, v,
                              R.batched(c.pairs, c.batch_labels), "batched")
            else:
                within_oracle(c, dtype, v, R.plain(c.pairs), "plain")
            if c.slice_labels:
                within_oracle(
                    c, dtype, v,
                    R.sliced(c.pairs, c.slice_labels, range(c.nassign)),
                    "sliced")
            assert R.state() == (0, 0)
        _ORACLE_DONE.add((c.name, dtype))

    def load(self, v):
        self.R.load(self.c.version(self.dtype, v))

    def step(self, v, op, *args, state=None):
        """load(v) (None: the leaves stay), poison T, op on T, op on R."""
        if v is not None:
            self.load(v)
        self.T.poison()
        got = getattr(self.T, op)(*args)
        want = getattr(self.R, op)(*args)
        same_bits(got[:2], want[:2])
        assert got[2:] == want[2:]  # profiled: the step kinds
        assert self.R.state() == (0, 0)
        if state is not None:
            assert self.T.state() == state, (op, v, self.T.state(), state)
        return got

    def close(self):
        for net in (self.T, self.R):
            if net is not None:
                net.close()


# ---- 1 ------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("structure", ["rqc24", "sv9"])
def test_plain_replay_follows_the_leaves(structure, dtype):
    c = case(structure)
    p = Pair(c, dtype)
    try:
        pointers = []
        for call, v in enumerate([0, 1, 2, 3, 4, 0], start=1):
            p.step(v, "plain", c.pairs, state=(1 if call == 1 else 2, 0))
            pointers.append(p.T.result_ptr())
        assert pointers[1] and len(set(pointers[1:])) == 1, pointers
    finally:
        p.close()


# ---- 2 ------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_profiled_between_replays(dtype):
    """A profiled walk under a captured graph releases the final block and
    allocates it again; the replays after it must find it where the graph
    writes."""
    c = case("sv9")
    p = Pair(c, dtype)
    try:
        p.step(1, "plain", c.pairs, state=(1, 0))
        p.step(2, "plain", c.pairs, state=(2, 0))
        p.step(3, "plain", c.pairs, state=(2, 0))
        got = p.step(4, "profiled", c.pairs, state=(2, 0))
        assert len(got[2]) == len(c.pairs)
        p.step(5, "plain", c.pairs, state=(2, 0))
        p.step(0, "plain", c.pairs, state=(2, 0))
    finally:
        p.close()


# ---- 3 ------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_change_and_back(dtype):
    c = case("sv9")
    P, Q = c.pairs, c.alt_pairs
    assert Q != P
    p = Pair(c, dtype)
    try:
        plan = [(P, 1), (P, 2), (P, 2),
                (Q, 1), (Q, 2), (Q, 2),  # the graph of P is dropped
                (P, 1), (P, 2), (P, 2)]
        for call, (pairs, state) in enumerate(plan):
            p.step((call + 1) % NVERSIONS, "plain", pairs, state=(state, 0))
    finally:
        p.close()


# ---- 4 ------------------------------------------------------------------


def test_reserve_after_capture():
    c = case("sv9")
    p = Pair(c, "c128")
    try:
        for call, state in enumerate([1, 2, 2]):
            p.step(call + 1, "plain", c.pairs, state=(state, 0))
        cached = p.T.cached()
        p.T.reserve(ARENA)
        assert p.T.state() == (0, 0)
        assert p.T.cached() == cached
        for call, state in enumerate([1, 2, 2]):
            p.step(call + 4, "plain", c.pairs, state=(state, 0))
    finally:
        p.close()


# ---- 5 ------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_between_replays(dtype):
    """tn_net_contract_batched under a captured graph sets the graph's final
    block aside; the next plain call replays into it."""
    c = case("sv9")
    p = Pair(c, dtype)
    try:
        p.step(1, "plain", c.pairs, state=(1, 0))
        p.step(2, "plain", c.pairs, state=(2, 0))
        p.step(3, "plain", c.pairs, state=(2, 0))
        p.step(4, "batched", c.pairs, state=(2, 0))
        p.step(5, "batched", c.pairs, state=(2, 0))
        p.step(0, "plain", c.pairs, state=(2, 0))
        p.step(1, "batched", c.pairs, state=(2, 0))
        p.step(2, "plain", c.pairs, state=(2, 0))
    finally:
        p.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_follows_the_leaves(dtype):
    """The real batch label: several leaves carry it, so only the batched
    entry is valid, and that walk never arms a capture."""
    c = case("amps")
    p = Pair(c, dtype)
    try:
        for v in (1, 2, 0, 3):
            labels, data = p.step(v, "batched", c.pairs, c.batch_labels,
                                  state=(0, 0))
            assert c.batch_labels[0] in labels
            assert sorted(data.shape) == [2, 2, 2, 5]
    finally:
        p.close()


# ---- 6 ------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("structure", ["eagle16", "three-leaf"])
def test_sliced_replay_follows_the_leaves(structure, dtype):
    """One captured graph serves every assignment through the control
    record: full sums, a share, the reversed share, and a plain call in
    between that drops it."""
    c = case(structure)
    labels, full = c.slice_labels, list(range(c.nassign))
    p = Pair(c, dtype)
    try:
        # captured inside the first call, at its second assignment
        p.step(1, "sliced", c.pairs, labels, full, state=(0, 2))
        p.step(2, "sliced", c.pairs, labels, full, state=(0, 2))
        p.step(3, "sliced", c.pairs, labels, full, state=(0, 2))
        p.step(4, "sliced", c.pairs, labels, [1, 3], state=(0, 2))
        p.step(5, "sliced", c.pairs, labels, [3, 1], state=(0, 2))
        p.step(0, "sliced", c.pairs, labels, full, state=(0, 2))
        p.step(1, "plain", c.pairs, state=(1, 0))
        p.step(2, "sliced", c.pairs, labels, full, state=(0, 2))
    finally:
        p.close()


# ---- 7 ------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_after_replay(dtype):
    c = case("sv9")
    u = np.random.default_rng(11).random(256)
    p = Pair(c, dtype)
    try:
        p.step(1, "plain", c.pairs, state=(1, 0))
        p.step(2, "plain", c.pairs, state=(2, 0))
        _, data = p.step(3, "plain", c.pairs, state=(2, 0))
        assert data.size == 512
        before = p.T.in_use()
        idx, norm = p.T.sample(u)
        idx_r, norm_r = p.R.sample(u)
        assert p.T.in_use() == before and p.T.state() == (2, 0)
        assert np.array_equal(idx, idx_r)
        assert not np.isnan(norm) and norm > 0
        assert np.float64(norm).tobytes() == np.float64(norm_r).tobytes()
        assert int(idx.max()) < 512
        p.step(4, "plain", c.pairs, state=(2, 0))
    finally:
        p.close()


# ---- 8 ------------------------------------------------------------------


def test_two_nets_interleaved():
    """Two arena nets with their own leaves, replaying in turn."""
    c = case("sv9")
    p1 = p2 = None
    try:
        p1 = Pair(c, "c128")
        p2 = Pair(c, "c128")
        for call, state in enumerate([1, 2]):
            p1.step(1 + call, "plain", c.pairs, state=(state, 0))
            p2.step(3 + call, "plain", c.pairs, state=(state, 0))
        p1.step(5, "plain", c.pairs, state=(2, 0))
        p2.step(0, "plain", c.pairs, state=(2, 0))
        p1.step(None, "plain", c.pairs, state=(2, 0))  # still version 5
        p2.step(1, "plain", c.pairs, state=(2, 0))
        p1.step(2, "plain", c.pairs, state=(2, 0))
        p2.step(None, "plain", c.pairs, state=(2, 0))  # still version 1
    finally:
        for p in (p1, p2):
            if p is not None:
                p.close()


# ---- 9 ------------------------------------------------------------------

OPS = ["load", "plain", "profiled", "batched", "sliced_full", "sliced_share",
       "sample", "poison"]
CONTRACTS = {"plain", "profiled", "batched", "sliced_full", "sliced_share"}


def draw_ops(seed, count=60, nassign=4):
    """`count` operations as (name, argument). At least every second contract
    call has a load right before it. A sample needs a result that was not
    poisoned since: where there is none the draw becomes a plain call."""
    rng = np.random.default_rng(seed)
    ops, version, loaded, unloaded_calls, clean = [], 0, False, 0, False
    while len(ops) < count:
        name = OPS[int(rng.integers(len(OPS)))]
        if name == "sample" and not clean:
            name = "plain"
        if name in CONTRACTS and not loaded and unloaded_calls >= 1:
            ops.append(("load", None))  # version filled in below
            loaded = True
            if len(ops) == count:
                break
        if name == "load":
            ops.append(("load", None))
            loaded = True
        elif name in CONTRACTS:
            arg = None
            if name == "sliced_share":
                n = int(rng.integers(1, nassign + 1))
                arg = [int(x) for x in rng.permutation(nassign)[:n]]
            ops.append((name, arg))
            unloaded_calls = 0 if loaded else unloaded_calls + 1
            loaded, clean = False, True
        elif name == "sample":
            ops.append(("sample", int(rng.integers(1 << 30))))
        else:
            ops.append(("poison", None))
            clean = False
    out = []
    for name, arg in ops:
        if name == "load":
            version = (version + 1 + int(rng.integers(NVERSIONS - 1))) \
                % NVERSIONS  # never the version already loaded
            arg = version
        out.append((name, arg))
    return out


def next_state(state, name, arg, nassign):
    """The replay states after an operation, by the rules in tnc_hip.hip:
    tn_net_contract arms, captures, replays and drops the sliced graph; a
    profiled walk arms only; a batched walk leaves the plain graph alone; a
    sliced call drops the plain graph, its first assignment arms, its second
    captures."""
    plain, sliced = state
    if name in ("plain", "profiled", "batched"):
        sliced = 0
        if name == "plain":
            plain = min(plain + 1, 2)
        elif name == "profiled":
            plain = max(plain, 1)
    elif name in ("sliced_full", "sliced_share"):
        n = nassign if name == "sliced_full" else len(arg)
        plain = 0
        sliced = min(sliced + n, 2)
    return plain, sliced


def run_ops(p, ops):
    c = p.c
    full = list(range(c.nassign))
    state = (0, 0)
    for name, arg in ops:
        if name == "load":
            p.load(arg)
        elif name == "poison":
            p.T.poison()
        elif name == "sample":
            u = np.random.default_rng(arg).random(64)
            before = p.T.in_use()
            idx, norm = p.T.sample(u)
            idx_r, norm_r = p.R.sample(u)
            assert np.array_equal(idx, idx_r)
            assert not np.isnan(norm)
            assert np.float64(norm).tobytes() == np.float64(norm_r).tobytes()
            assert p.T.in_use() == before
        else:
            state = next_state(state, name, arg, c.nassign)
            if name == "sliced_full":
                p.step(None, "sliced", c.pairs, c.slice_labels, full,
                       state=state)
            elif name == "sliced_share":
                p.step(None, "sliced", c.pairs, c.slice_labels, arg,
                       state=state)
            else:
                p.step(None, name, c.pairs, state=state)
        assert p.T.state() == state, (name, arg, p.T.state(), state)


def settle_and_compare(p, had_sliced):
    """Three plain calls on T and on a fresh arena net: both replay, and
    both hold the same bytes of the arena, so T leaked no block. The shadow
    leaves of a sliced call stay in the arena for the net's life, so the
    fresh net makes one sliced call first where T made any."""
    c = p.c
    fresh = c.spec.devnet(p.dtype, arena_bytes=ARENA, share=p.R)
    try:
        if had_sliced:
            fresh.sliced(c.pairs, c.slice_labels, range(c.nassign))
        for v in (1, 2, 3):
            p.step(v, "plain", c.pairs)
            same_bits(fresh.plain(c.pairs), p.R.result())
        assert p.T.state() == (2, 0) and fresh.state() == (2, 0)
        assert p.T.in_use() == fresh.in_use(), (p.T.in_use(), fresh.in_use())
    finally:
        fresh.close()


@pytest.mark.parametrize("seed,dtype", [(0, "c128"), (1, "c128"), (2, "c128"),
                                        (0, "c64")])
def test_random_sequences(seed, dtype):
    c = case("eagle16")
    ops = draw_ops(seed, 60, c.nassign)
    assert len(ops) == 60
    p = Pair(c, dtype)
    try:
        try:
            run_ops(p, ops)
            settle_and_compare(
                p, any(name.startswith("sliced") for name, _ in ops))
        except BaseException:
            print(f"test_random_sequences seed {seed} {dtype}, operations:")
            for x, op in enumerate(ops):
                print(f"  {x:2d} {op}")
            raise
    finally:
        p.close()
