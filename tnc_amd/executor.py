"""GPU contraction engine: the contract_tensor_network drop-in
(contraction.rs:35) running entirely on the MI355X.

Wraps the tn_net_* C ABI: leaves are uploaded once, the (flattened)
replace-left path walks on-device, intermediates never touch the host.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import hiplib
from .contraction_path import ContractionPath, flatten_network
from .cost import contract_cost_tensors
from .tensor import CompositeTensor, LeafTensor


class StepInfo:
    __slots__ = ("i", "j", "m", "n", "k", "flops", "out_legs", "out_dims",
                 "packa", "packb", "pipe_p", "plan", "ws", "batch")

    def __init__(self, i, j, m, n, k, flops, out_legs, out_dims,
                 packa=False, packb=False, pipe_p=0, plan=None):
        self.ws = 0     # batched walk: workspace bytes of the step
        self.batch = 1  # batched walk: the step batch
        self.i, self.j = i, j
        self.m, self.n, self.k = m, n, k
        self.flops = flops
        self.out_legs = out_legs
        self.out_dims = out_dims
        self.packa = packa  # A is not already in [M..][K..] order
        self.packb = packb  # B is not already in [K..][N..] order
        self.pipe_p = pipe_p  # pack-pipeline window count (0 = serial pack)
        self.plan = plan  # the step's whole hiplib.StepPlan


def plan_steps(leaves, steps, dtype="c128"):
    """Host-side metadata walk: per-step (M, N, K), metric flops
    ((8s-2)*o, contraction_cost.rs:26-32), output legs, and how the library
    will dispatch the step: which operands the TTGT route would pack, the
    pack-pipeline window count and the workspace it will ask for. All of
    that comes from tn_plan_step, the planner the dispatch itself runs."""
    views = [LeafTensor(t.legs, t.bond_dims) for t in leaves]
    infos = []
    for i, j in steps:
        a, b = views[i], views[j]
        out = a ^ b
        # the engine always has its second stream
        p = hiplib.plan_step(out.legs, out.bond_dims, a.legs, a.bond_dims,
                             b.legs, b.bond_dims, dtype=dtype,
                             has_stream2=True)
        infos.append(
            StepInfo(i, j, p.m, p.n, p.k, contract_cost_tensors(a, b),
                     out.legs, out.bond_dims, packa=bool(p.pack_a),
                     packb=bool(p.pack_b), pipe_p=p.pipe_p, plan=p)
        )
        views[i] = out
        views[j] = None
    return infos


def arena_bytes(leaves, steps, infos, esize=16, exact_dot=False):
    """Peak device-arena demand: live intermediates + this step's output and
    the workspaces its dispatch actually uses, walked over the plan. The
    pack-overlap executor allocates the NEXT step's pack buffers one step
    early (prepack on stream2), so each step's demand includes them.
    Padded 15% for fragmentation + split-K slack (a split buffer that does
    not fit only costs the step its split). exact_dot: count a dot step's
    partials as the plan states them (ws_dot), not by the 32 MiB bound."""
    def pack_ws(p):  # pack buffers, or the pipeline's window buffers
        return p.ws_pack_a + p.ws_pack_b

    live = {}  # slot -> bytes (intermediates only; leaves live outside)
    peak = 0
    for s, info in enumerate(infos):
        out_b = info.m * info.n * esize
        p = info.plan
        nxt = pack_ws(infos[s + 1].plan) if s + 1 < len(infos) else 0
        # dot partials: bounded, not exact (<= 2^21 blocks * 16 B)
        if p.ws_dot:
            ws = p.ws_dot if exact_dot else (1 << 25)
        else:
            ws = pack_ws(p) + p.ws_tmp_c + p.ws_slices
        demand = sum(live.values()) + out_b + ws + nxt
        peak = max(peak, demand)
        live.pop(info.j, None)
        live[info.i] = out_b
    return int(peak * 1.15) + (1 << 20)


def plan_steps_batched(leaves, steps, batch_edges, dtype="c128"):
    """plan_steps for a batched walk (tn_net_contract_batched). Stored
    orders, classes and workspaces come from tn_plan_batch_walk, the plan the
    executor itself walks; each StepInfo carries the step's hiplib.BatchPlan
    (`plan`, with `ws` the workspace bytes and `batch` the step batch), m/n/k
    of ONE batch element and flops = element cost times the step batch.
    Returns (infos, classes)."""
    dims = {l: d for t in leaves for l, d in zip(t.legs, t.bond_dims)}
    cls, out_labels, ws = hiplib.plan_batch_walk(
        [(t.legs, t.bond_dims) for t in leaves], steps, batch_edges, dtype)
    views = [LeafTensor(t.legs, t.bond_dims) for t in leaves]
    infos = []
    for s, (i, j) in enumerate(steps):
        a, b = views[i], views[j]
        out = LeafTensor(out_labels[s], [dims[l] for l in out_labels[s]])
        bp = hiplib.plan_step_batched(out.legs, out.bond_dims, a.legs,
                                      a.bond_dims, b.legs, b.bond_dims,
                                      batch_edges, dtype=dtype,
                                      has_stream2=True)
        assert bp.cls == cls[s]
        e = bp.elem
        flops = ((e.k - 1.0) * 2.0 + e.k * 6.0) * e.m * e.n * bp.batch
        info = StepInfo(i, j, e.m, e.n, e.k, flops, out.legs, out.bond_dims,
                        packa=bool(e.pack_a), packb=bool(e.pack_b),
                        pipe_p=e.pipe_p, plan=bp)
        info.ws = ws[s]
        info.batch = bp.batch
        infos.append(info)
        views[i] = out
        views[j] = None
    return infos, cls


def batched_arena_bytes(infos, esize=16):
    """Peak arena demand of a batched walk: live intermediates + the step's
    output + the workspace tn_plan_batch_walk states for it, padded as
    arena_bytes pads."""
    live = {}
    peak = 0
    for info in infos:
        out_b = info.batch * info.m * info.n * esize
        peak = max(peak, sum(live.values()) + out_b + info.ws)
        live.pop(info.j, None)
        live[info.i] = out_b
    return int(peak * 1.15) + (1 << 20)


def reduced_leaves(leaves, slice_edges):
    """The leaves with the sliced legs removed (legs and dims only): what
    slicing.slice_network produces for any assignment."""
    cut = set(slice_edges)
    return [
        LeafTensor([l for l in t.legs if l not in cut],
                   [d for l, d in zip(t.legs, t.bond_dims) if l not in cut])
        for t in leaves
    ]


def sliced_arena_bytes(leaves, steps, slice_edges, dtype="c128"):
    """Arena demand of a sliced contraction (tn_net_contract_sliced): the
    walk over the reduced leaves, plus the accumulator (one more final
    tensor, held for the whole call), plus the shadow leaves (the reduced
    copy of every leaf that carries a sliced leg, each rounded up to the
    arena's 256-byte granule). Needs no GPU."""
    esize = 16 if dtype == "c128" else 8
    red = reduced_leaves(leaves, slice_edges)
    infos = plan_steps(red, steps, dtype)
    cut = set(slice_edges)
    if infos:
        acc = infos[-1].m * infos[-1].n * esize
    else:
        acc = int(np.prod(red[0].bond_dims, dtype=object)) * esize
    shadows = sum(
        (int(np.prod(r.bond_dims, dtype=object)) * esize + 255) // 256 * 256
        for t, r in zip(leaves, red) if cut & set(t.legs)
    )
    # slicing is for networks that do not fit: no 32 MiB allowance for a dot
    # step's partials where the plan gives their size
    return (arena_bytes(red, steps, infos, esize, exact_dot=True)
            + acc + 256 + shadows)


class ContractionEngine:
    """Device-resident executor for one (flattened) network. With
    `slice_edges` the engine is sized and planned for contract_sliced():
    infos and total_flops describe one slice, the arena holds one sliced
    walk, the accumulator and the shadow leaves; the leaves are uploaded
    whole, once. With `batch_edges` (labels shared by several leaves that
    are kept, never summed) the engine is planned and sized for
    contract_batched() by tn_plan_batch_walk, and the other contract calls
    refuse."""

    def __init__(self, tn: CompositeTensor, replace_path: ContractionPath,
                 device=0, dtype="c128", slice_edges=None, batch_edges=None):
        if hiplib.device_count() == 0:
            raise RuntimeError("no AMD GPU present — tnc_amd has no CPU fallback")
        assert dtype in ("c128", "c64")
        self.dtype = dtype
        self.npdtype = np.complex128 if dtype == "c128" else np.complex64
        self.esize = 16 if dtype == "c128" else 8
        leaves, steps, final = flatten_network(tn, replace_path)
        self.leaves = leaves
        self.steps = steps
        self.final = final
        self.slice_edges = None if slice_edges is None else list(slice_edges)
        self.num_slices = 1
        self.batch_edges = None if batch_edges is None else list(batch_edges)
        if self.batch_edges is not None and self.slice_edges is not None:
            raise ValueError("batch_edges cannot be combined with slice_edges")
        if self.batch_edges is not None:
            # refuses what the executor would refuse, before anything uploads
            self.infos, self.batch_classes = plan_steps_batched(
                leaves, steps, self.batch_edges, dtype)
        elif self.slice_edges is None:
            self.infos = plan_steps(leaves, steps, dtype)
        else:
            # refuses what the executor would refuse, before anything uploads
            self.num_slices, _, _ = hiplib.plan_slices(
                [(t.legs, t.bond_dims) for t in leaves], steps,
                self.slice_edges, dtype)
            self.infos = plan_steps(
                reduced_leaves(leaves, self.slice_edges), steps, dtype)
        self.total_flops = sum(s.flops for s in self.infos)
        L = hiplib.lib()
        hiplib.check(L.tn_set_device(device), "tn_set_device")
        self.net = L.tn_net_create2(device, 0 if dtype == "c128" else 1)
        if not self.net:
            raise RuntimeError(f"tn_net_create failed: {hiplib.last_error()}")
        if self.batch_edges is not None:
            reserve = batched_arena_bytes(self.infos, self.esize)
        elif self.slice_edges is None:
            reserve = arena_bytes(leaves, steps, self.infos, self.esize)
        else:
            reserve = sliced_arena_bytes(leaves, steps, self.slice_edges,
                                         dtype)
        # launch-bound walks (many tiny steps) only replay as a hipGraph
        # when every workspace comes from the arena — reserve a floor so
        # replay engages (rqc24: ~2.4 ms/contraction unreserved vs
        # ~0.6 ms replayed)
        if len(steps) >= 64:
            reserve = max(reserve, 256 * 1024 * 1024)
        # arena is an optimization: if the reservation fails (tiny GPUs,
        # fragmented memory), every block falls back to plain hipMalloc
        # (the stream-ordered pool is avoided — see ws_alloc in tnc_hip.hip)
        if reserve > 64 * 1024 * 1024:
            rc = L.tn_net_reserve(self.net, reserve)
            if rc != 0:
                import warnings

                warnings.warn(
                    f"arena reservation of {reserve} bytes failed "
                    f"({hiplib.last_error()}); falling back to per-block "
                    "hipMalloc"
                )
        for t in leaves:
            data = np.ascontiguousarray(t.tensordata.into_data(), dtype=self.npdtype)
            assert list(data.shape) == list(t.bond_dims), (data.shape, t.bond_dims)
            idx = L.tn_net_add_leaf(
                self.net,
                hiplib._u64arr(t.legs),
                hiplib._u64arr(t.bond_dims),
                len(t.legs),
                data.ctypes.data_as(ctypes.c_void_p),
            )
            if idx < 0:
                raise RuntimeError(f"tn_net_add_leaf failed: {hiplib.last_error()}")
        self._pairs = hiplib._u64arr([x for p in steps for x in p])
        # sum of |amplitude|^2 over the final tensor, as the last sample() or
        # sample_flat() measured it
        self.sample_norm2 = None

    def _refuse_batched(self, what):
        if self.batch_edges is not None:
            raise RuntimeError(
                f"{what} on an engine built with batch_edges; use "
                "contract_batched()")

    def contract_batched(self) -> float:
        """One batched contraction (tn_net_contract_batched): the final
        tensor keeps the batch edges. Returns device wall ms."""
        if self.batch_edges is None:
            raise RuntimeError("engine was built without batch_edges")
        ms = ctypes.c_double()
        hiplib.check(
            hiplib.lib().tn_net_contract_batched(
                self.net, self._pairs, len(self.steps),
                hiplib._u64arr(self.batch_edges), len(self.batch_edges),
                ctypes.byref(ms)
            ),
            "tn_net_contract_batched",
        )
        return ms.value

    def contract(self) -> float:
        """One full contraction; returns device wall ms."""
        self._refuse_batched("contract()")
        ms = ctypes.c_double()
        hiplib.check(
            hiplib.lib().tn_net_contract(
                self.net, self._pairs, len(self.steps), ctypes.byref(ms)
            ),
            "tn_net_contract",
        )
        return ms.value

    def contract_sliced(self, which=None) -> float:
        """The sum over the listed slice assignments (None: all of them, in
        order) of the network with slice_edges fixed, on the device in one
        call; result() / result_dev() then give the sum. `which` holds
        assignment indices, first edge most significant: index t is
        list(slicing.iter_assignments(tn, slice_edges))[t]. Returns the
        device ms of all assignments."""
        self._refuse_batched("contract_sliced()")
        if self.slice_edges is None:
            raise RuntimeError("engine was built without slice_edges")
        if which is None:
            which = range(self.num_slices)
        which = list(which)
        ms = ctypes.c_double()
        hiplib.check(
            hiplib.lib().tn_net_contract_sliced(
                self.net, self._pairs, len(self.steps),
                hiplib._u64arr(self.slice_edges), len(self.slice_edges),
                hiplib._u64arr(which), len(which), ctypes.byref(ms)
            ),
            "tn_net_contract_sliced",
        )
        return ms.value

    def contract_profiled(self):
        """Contraction with per-step HIP-event timings.
        Returns (elapsed_ms, step_ms[], gemm_ms[], kind[])."""
        self._refuse_batched("contract_profiled()")
        n = len(self.steps)
        step_ms = (ctypes.c_double * n)()
        gemm_ms = (ctypes.c_double * n)()
        kind = (ctypes.c_int32 * n)()
        ms = ctypes.c_double()
        hiplib.check(
            hiplib.lib().tn_net_contract_profiled(
                self.net, self._pairs, n, step_ms, gemm_ms, kind, ctypes.byref(ms)
            ),
            "tn_net_contract_profiled",
        )
        return ms.value, list(step_ms), list(gemm_ms), list(kind)

    def _result_meta(self):
        """(legs, dims) of the final tensor in stored order."""
        labels = (ctypes.c_uint64 * 64)()
        dims = (ctypes.c_uint64 * 64)()
        nd = ctypes.c_size_t()
        hiplib.check(
            hiplib.lib().tn_net_result_meta(self.net, labels, dims,
                                            ctypes.byref(nd)),
            "tn_net_result_meta",
        )
        return ([labels[i] for i in range(nd.value)],
                [dims[i] for i in range(nd.value)])

    def result(self) -> "tuple[list, np.ndarray]":
        L = hiplib.lib()
        legs, dims = self._result_meta()
        shape = tuple(dims)
        out = np.empty(shape, dtype=self.npdtype)
        hiplib.check(
            L.tn_net_result_data(self.net, out.ctypes.data_as(ctypes.c_void_p)),
            "tn_net_result_data",
        )
        return legs, out

    def result_dev(self) -> int:
        """Device pointer of the final tensor (valid until next contract)."""
        ptr = hiplib.lib().tn_net_result_dev(self.net)
        if not ptr:
            raise RuntimeError("no result available")
        return ptr

    def sample_flat(self, u) -> np.ndarray:
        """Flat indices into the final tensor (stored order), one per
        uniform of u (each 0 <= u < 1), drawn on the device with probability
        |amplitude|^2 (tn_net_sample); the tensor stays where it is. Sets
        sample_norm2. An empty u measures the norm only."""
        u = np.ascontiguousarray(u, dtype=np.float64).ravel()
        idx = np.empty(u.size, dtype=np.uint64)
        norm2 = ctypes.c_double(float("nan"))
        rc = hiplib.lib().tn_net_sample(
            self.net, u.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            u.size, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            ctypes.byref(norm2))
        hiplib.check(rc, "tn_net_sample")
        self.sample_norm2 = norm2.value
        return idx

    def sample(self, u) -> "tuple[list, np.ndarray]":
        """Shots from the final tensor of the last contract(),
        contract_batched() or contract_sliced(). Returns (legs, digits):
        the legs in stored order and digits[nshots, rank], the value drawn
        on every leg for every uniform of u."""
        idx = self.sample_flat(u)
        legs, dims = self._result_meta()
        return legs, decode_digits(idx, dims)

    def close(self):
        if getattr(self, "net", None):
            hiplib.lib().tn_net_destroy(self.net)
            self.net = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def contract_tensor_network_gpu(tn: CompositeTensor, replace_path, device=0):
    """One-shot: contract and return (legs, ndarray)."""
    eng = ContractionEngine(tn, replace_path, device)
    try:
        eng.contract()
        return eng.result()
    finally:
        eng.close()


def amplitudes_gpu(tn: CompositeTensor, replace_path, batch_edge, device=0,
                   dtype="c128"):
    """All amplitudes of a Circuit.into_amplitudes_network network in one
    batched walk. Returns (legs, ndarray) with batch_edge first: row r is
    what contract_tensor_network_gpu gives for bitstring r's own network. A
    stored order with the batch edge elsewhere is transposed on the host.
    When no leaf carries batch_edge (every bitstring the same on every
    closed qubit) nothing is batched and the result has no batch axis."""
    carried = any(batch_edge in t.legs
                  for t in flatten_network(tn, replace_path)[0])
    eng = ContractionEngine(tn, replace_path, device, dtype,
                            batch_edges=[batch_edge] if carried else [])
    try:
        eng.contract_batched()
        legs, data = eng.result()
    finally:
        eng.close()
    if batch_edge in legs and legs[0] != batch_edge:
        at = legs.index(batch_edge)
        order = [at] + [x for x in range(len(legs)) if x != at]
        legs = [legs[x] for x in order]
        data = np.ascontiguousarray(np.transpose(data, order))
    return legs, data


def decode_digits(idx, dims) -> np.ndarray:
    """The mixed-radix digits of flat row-major indices over dims, last dim
    fastest: an int64 array [len(idx), len(dims)]. Pure numpy."""
    rest = np.asarray(idx).astype(np.int64).ravel()
    digits = np.empty((rest.size, len(dims)), dtype=np.int64)
    for x in range(len(dims) - 1, -1, -1):
        digits[:, x] = rest % int(dims[x])
        rest = rest // int(dims[x])
    if rest.size and np.any(rest):
        raise ValueError("index beyond the tensor")
    return digits


def decode_bitstrings(legs, digits, target_leg_order, batch_edge=None,
                      bitstrings=None):
    """One string per shot, in qubit order, from the digits drawn on the
    legs of a final tensor (ContractionEngine.sample). target_leg_order is
    the Permutor's: the open edges in qubit order. Without `bitstrings` a
    string holds the open qubits only. With it, the strings given to
    into_amplitudes_network (or the one given to into_amplitude_network), a
    string is the drawn row of `bitstrings`, the digit on batch_edge (row 0
    where no leg is batch_edge), with every '*' replaced by that qubit's
    drawn bit. Pure numpy."""
    legs = list(legs)
    digits = np.asarray(digits)
    if digits.ndim != 2 or digits.shape[1] != len(legs):
        raise ValueError("digits must be [nshots, len(legs)]")
    column = {l: x for x, l in enumerate(legs)}
    known = set(target_leg_order) | {batch_edge}
    if len(column) != len(legs) or not set(legs) <= known:
        raise ValueError("a leg is neither an open edge nor the batch edge")
    try:
        open_cols = [column[e] for e in target_leg_order]
    except KeyError as e:
        raise ValueError(f"open edge {e} is no leg of the tensor") from None
    if batch_edge in column:
        rows = digits[:, column[batch_edge]]
    else:
        rows = np.zeros(digits.shape[0], dtype=np.int64)
    if bitstrings is not None:
        bitstrings = list(bitstrings)
        for b in bitstrings:
            if b.count("*") != len(open_cols):
                raise ValueError("bitstrings must have one '*' per open edge")
        if rows.size and int(rows.max()) >= len(bitstrings):
            raise ValueError("drawn row beyond the bitstrings given")
    out = []
    for s in range(digits.shape[0]):
        bits = [str(int(d)) for d in digits[s, open_cols]]
        if bitstrings is None:
            out.append("".join(bits))
            continue
        it = iter(bits)
        out.append("".join(next(it) if c == "*" else c
                           for c in bitstrings[int(rows[s])]))
    return out


def sample_bitstrings_gpu(tn: CompositeTensor, replace_path, permutor, shots,
                          seed=0, device=0, dtype="c128", batch_edge=None,
                          bitstrings=None):
    """`shots` bitstrings drawn from a circuit network with probability
    |amplitude|^2: one contraction (batched when the network carries
    batch_edge), then the shots are drawn on the device from the final
    tensor, with uniforms from numpy.random.default_rng(seed). tn, permutor
    (and batch_edge, bitstrings) as Circuit.into_statevector_network,
    into_amplitude_network or into_amplitudes_network return and take them.
    Strings are as decode_bitstrings builds them. With several bitstrings the
    draw is over the whole [B, open...] block: a row with more mass in its
    open qubits is drawn more often."""
    u = np.random.default_rng(seed).random(int(shots))
    batch_edges = None
    if batch_edge is not None:
        carried = any(batch_edge in t.legs
                      for t in flatten_network(tn, replace_path)[0])
        batch_edges = [batch_edge] if carried else []
    eng = ContractionEngine(tn, replace_path, device, dtype,
                            batch_edges=batch_edges)
    try:
        if batch_edges is None:
            eng.contract()
        else:
            eng.contract_batched()
        legs, digits = eng.sample(u)
    finally:
        eng.close()
    return decode_bitstrings(legs, digits, permutor.target_leg_order,
                             batch_edge, bitstrings)
