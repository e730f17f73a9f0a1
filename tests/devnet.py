"""A tn_net over leaves that live in torch device buffers.

A plain helper module for tests/test_gpu_replay_data.py. The leaves are
registered with tn_net_add_leaf_dev, which imports the pointer without a
copy, so new contents written into the same buffers are what the next
contract call must read, whether it walks normally, captures a graph or
replays one (include/tnc_hip.h). Two DevNets may share one set of buffers:
the tests compare an arena net, which captures and replays, with an
arena-less one, which can only ever walk.

Every method goes to the C entry points through ctypes; nothing here goes
through ContractionEngine.
"""

import ctypes

import numpy as np

from tnc_amd import hiplib

NPDTYPE = {"c128": np.complex128, "c64": np.complex64}
REAL = {"c128": np.float64, "c64": np.float32}
ESIZE = {"c128": 16, "c64": 8}


def _elems(dims):
    n = 1
    for d in dims:
        n *= int(d)
    return n


class DevNet:
    """DevNet(leaf_specs, dtype, arena_bytes=None, share=None).

    leaf_specs: [(labels, dims), ...]. One torch buffer per leaf on cuda:0,
    (elems, 2) of float64 (c128) or float32 (c64); with `share` the buffers
    of that DevNet are used instead (same specs, same dtype). arena_bytes:
    tn_net_reserve is called with it; None leaves the net without an arena,
    and such a net never arms a capture and never prepacks."""

    def __init__(self, leaf_specs, dtype, arena_bytes=None, share=None):
        import torch

        assert dtype in NPDTYPE
        self.torch = torch
        self.dtype = dtype
        self.specs = [(list(map(int, labels)), list(map(int, dims)))
                      for labels, dims in leaf_specs]
        self.L = hiplib.lib()
        self.net = None
        if share is None:
            tdt = torch.float64 if dtype == "c128" else torch.float32
            self.buffers = [
                torch.zeros((_elems(dims), 2), dtype=tdt, device="cuda:0")
                for _, dims in self.specs
            ]
        else:
            assert share.dtype == dtype and share.specs == self.specs
            self.buffers = share.buffers
        self.pointers = [b.data_ptr() for b in self.buffers]
        hiplib.check(self.L.tn_set_device(0), "tn_set_device")
        self.net = self.L.tn_net_create2(0, 0 if dtype == "c128" else 1)
        if not self.net:
            raise RuntimeError(f"tn_net_create2: {hiplib.last_error()}")
        try:
            if arena_bytes is not None:
                self.reserve(arena_bytes)
            for (labels, dims), ptr in zip(self.specs, self.pointers):
                idx = self.L.tn_net_add_leaf_dev(
                    self.net, hiplib._u64arr(labels), hiplib._u64arr(dims),
                    len(labels), ptr)
                if idx < 0:
                    raise RuntimeError(
                        f"tn_net_add_leaf_dev: {hiplib.last_error()}")
        except Exception:
            self.close()
            raise

    # ---- data ----------------------------------------------------------

    def load(self, arrays):
        """New contents into the same buffers (every net sharing them sees
        them); the pointers must not have moved."""
        torch = self.torch
        assert len(arrays) == len(self.buffers)
        for (_, dims), buf, ptr, arr in zip(self.specs, self.buffers,
                                            self.pointers, arrays):
            arr = np.ascontiguousarray(arr, dtype=NPDTYPE[self.dtype])
            assert arr.size == _elems(dims), (arr.shape, dims)
            host = torch.from_numpy(
                arr.reshape(-1).view(REAL[self.dtype]).reshape(-1, 2))
            buf.copy_(host)
            assert buf.data_ptr() == ptr
        torch.cuda.synchronize()

    # ---- the contract calls ---------------------------------------------

    @staticmethod
    def _pairs(pairs):
        return hiplib._u64arr([x for p in pairs for x in p]), len(pairs)

    def plain(self, pairs):
        arr, n = self._pairs(pairs)
        hiplib.check(self.L.tn_net_contract(self.net, arr, n, None),
                     "tn_net_contract")
        return self.result()

    def profiled(self, pairs):
        """(labels, data, kinds): the result and the step kinds."""
        arr, n = self._pairs(pairs)
        step_ms = (ctypes.c_double * max(n, 1))()
        gemm_ms = (ctypes.c_double * max(n, 1))()
        kind = (ctypes.c_int32 * max(n, 1))()
        hiplib.check(
            self.L.tn_net_contract_profiled(self.net, arr, n, step_ms,
                                            gemm_ms, kind, None),
            "tn_net_contract_profiled")
        labels, data = self.result()
        return labels, data, [kind[s] for s in range(n)]

    def batched(self, pairs, batch_labels=()):
        arr, n = self._pairs(pairs)
        batch_labels = list(batch_labels)
        hiplib.check(
            self.L.tn_net_contract_batched(
                self.net, arr, n, hiplib._u64arr(batch_labels),
                len(batch_labels), None),
            "tn_net_contract_batched")
        return self.result()

    def sliced(self, pairs, labels, which):
        arr, n = self._pairs(pairs)
        labels, which = list(labels), list(which)
        hiplib.check(
            self.L.tn_net_contract_sliced(
                self.net, arr, n, hiplib._u64arr(labels), len(labels),
                hiplib._u64arr(which), len(which), None),
            "tn_net_contract_sliced")
        return self.result()

    def sample(self, u):
        """(indices, norm) of tn_net_sample on the current final tensor."""
        u = np.ascontiguousarray(u, dtype=np.float64).ravel()
        idx = np.empty(u.size, dtype=np.uint64)
        norm2 = ctypes.c_double(float("nan"))
        hiplib.check(
            self.L.tn_net_sample(
                self.net, u.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                u.size, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                ctypes.byref(norm2)),
            "tn_net_sample")
        return idx, norm2.value

    # ---- the result -------------------------------------------------------

    def _meta(self):
        labels = (ctypes.c_uint64 * 64)()
        dims = (ctypes.c_uint64 * 64)()
        nd = ctypes.c_size_t()
        hiplib.check(
            self.L.tn_net_result_meta(self.net, labels, dims,
                                      ctypes.byref(nd)),
            "tn_net_result_meta")
        return ([labels[x] for x in range(nd.value)],
                [dims[x] for x in range(nd.value)])

    def result(self):
        """(labels, a host copy of the final tensor)."""
        labels, dims = self._meta()
        out = np.empty(tuple(dims), dtype=NPDTYPE[self.dtype])
        hiplib.check(
            self.L.tn_net_result_data(self.net,
                                      out.ctypes.data_as(ctypes.c_void_p)),
            "tn_net_result_data")
        return labels, out

    def result_ptr(self):
        """tn_net_result_dev: 0 when there is no result."""
        return self.L.tn_net_result_dev(self.net) or 0

    def poison(self):
        """NaNs over the current final tensor, so a call that writes nothing,
        or writes elsewhere, cannot pass for one that computed it. Nothing
        when there is no result."""
        ptr = self.result_ptr()
        if not ptr:
            return
        torch = self.torch
        _, dims = self._meta()
        n = _elems(dims)
        tdt = torch.float64 if self.dtype == "c128" else torch.float32
        nan = torch.full((n, 2), float("nan"), dtype=tdt, device="cuda:0")
        torch.cuda.synchronize()
        hiplib.check(
            self.L.tn_memcpy_dtod(ptr, nan.data_ptr(), n * ESIZE[self.dtype]),
            "tn_memcpy_dtod")

    # ---- telemetry ------------------------------------------------------

    def state(self):
        """(plain, sliced) of tn_net_replay_state."""
        plain, sliced = ctypes.c_int32(-99), ctypes.c_int32(-99)
        hiplib.check(
            self.L.tn_net_replay_state(self.net, ctypes.byref(plain),
                                       ctypes.byref(sliced)),
            "tn_net_replay_state")
        return plain.value, sliced.value

    def _pool(self):
        used, cached = ctypes.c_uint64(), ctypes.c_uint64()
        hiplib.check(
            self.L.tn_net_pool_bytes(self.net, ctypes.byref(used),
                                     ctypes.byref(cached)),
            "tn_net_pool_bytes")
        return used.value, cached.value

    def in_use(self):
        return self._pool()[0]

    def cached(self):
        return self._pool()[1]

    def reserve(self, arena_bytes):
        hiplib.check(self.L.tn_net_reserve(self.net, int(arena_bytes)),
                     "tn_net_reserve")

    def close(self):
        if self.net:
            self.L.tn_net_destroy(self.net)
            self.net = None


class NetSpec:
    """What a DevNet needs from a CompositeTensor and its replace path: the
    leaves' labels and dims, their data (complex128) and the flat pair list,
    flattened as ContractionEngine flattens them."""

    def __init__(self, tn, replace_path):
        from tnc_amd.contraction_path import ContractionPath, flatten_network

        if not isinstance(replace_path, ContractionPath):
            replace_path = ContractionPath.simple(replace_path)
        leaves, steps, _ = flatten_network(tn, replace_path)
        self.tn = tn
        self.leaf_specs = [(list(t.legs), list(t.bond_dims)) for t in leaves]
        self.base = []
        for t in leaves:
            data = np.ascontiguousarray(t.tensordata.into_data(),
                                        dtype=np.complex128)
            assert list(data.shape) == list(t.bond_dims)
            self.base.append(data)
        self.pairs = [tuple(p) for p in steps]

    def pairs_of(self, replace_path):
        """The flat pairs of another replace path over the same network."""
        from tnc_amd.contraction_path import flatten_network

        return [tuple(p) for p in flatten_network(self.tn, replace_path)[1]]

    def devnet(self, dtype, arena_bytes=None, share=None):
        return DevNet(self.leaf_specs, dtype, arena_bytes, share)
