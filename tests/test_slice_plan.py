"""The slice plan (plan_slices in step_plan.hpp, exported as tn_plan_slices)
and the sizing of a sliced engine's arena. No GPU: the plan is host code.

What a sliced contraction does on the device follows from this plan: which
leaves are gathered, from which offset for assignment t, and into which
reduced shape. Each is checked against what slicing.slice_network does on
the host with numpy."""

import itertools

import numpy as np
import pytest

from tnc_amd import Greedy, hiplib
from tnc_amd.builders import random_circuit
from tnc_amd.connectivity import ConnectivityLayout
from tnc_amd.contraction_path import flatten_network
from tnc_amd.executor import (arena_bytes, plan_steps, reduced_leaves,
                              sliced_arena_bytes)
from tnc_amd.slicing import (_walk_sizes, find_slice_edges, iter_assignments,
                             slice_network)


@pytest.fixture(scope="module")
def eagle():
    tn = random_circuit(16, 14, 0.5, 0.8, 3, ConnectivityLayout.EAGLE)
    replace = Greedy().find_path(tn).replace_path()
    peak, _, _ = _walk_sizes(tn, replace.toplevel)
    edges, _ = find_slice_edges(tn, replace.toplevel, peak / 4, max_edges=4)
    leaves, steps, _ = flatten_network(tn, replace)
    return tn, replace, edges, leaves, steps


def _shapes(leaves):
    return [(list(t.legs), list(t.bond_dims)) for t in leaves]


def test_offsets_and_reduced_legs(eagle):
    tn, _, edges, leaves, steps = eagle
    assert edges == [365, 362]
    assert len(leaves) == 296
    assert [leaves[234].legs.index(e) for e in edges] == [0, 2]
    nassign, reduced_nd, strides = hiplib.plan_slices(
        _shapes(leaves), steps, edges)
    assert nassign == 4
    radices = [2, 2]
    assignments = list(iter_assignments(tn, edges))
    assert len(assignments) == nassign
    for t, assignment in enumerate(assignments):
        # first label most significant
        digits = [(t // 2) % 2, t % 2]
        assert digits == [assignment[e] for e in edges]
        stn = slice_network(tn, assignment)
        for x, (full, cut) in enumerate(zip(leaves, stn.tensors)):
            assert reduced_nd[x] == len(cut.legs)
            offset = sum(d * s for d, s in zip(digits, strides[x]))
            if not set(edges) & set(full.legs):
                assert strides[x] == [0, 0] and offset == 0
                continue
            # the flat offset numpy gives for the index slice_network applies
            flat = np.arange(int(np.prod(full.bond_dims))).reshape(
                tuple(full.bond_dims))
            index = tuple(assignment[l] if l in assignment else 0
                          for l in full.legs)
            assert offset == flat[index]
            # and every element of the slice sits at offset + a stride sum
            # that does not depend on the assignment
            picked = flat[tuple(assignment[l] if l in assignment
                                else slice(None) for l in full.legs)]
            base = flat[tuple(0 if l in assignment else slice(None)
                              for l in full.legs)]
            assert np.array_equal(picked, base + offset)
    assert radices == [dict(zip(leaves[234].legs, leaves[234].bond_dims))[e]
                       for e in edges]


def test_mixed_radix():
    # A[i, s:3, k], B[k, t:2, j], C[s:3, t:2, l]; slice (s, t)
    i, s, k, t, j, l = 1, 2, 3, 4, 5, 6
    leaves = [([i, s, k], [3, 3, 5]), ([k, t, j], [5, 2, 7]),
              ([s, t, l], [3, 2, 5])]
    steps = [(0, 1), (0, 2)]
    nassign, reduced_nd, strides = hiplib.plan_slices(leaves, steps, [s, t])
    assert nassign == 6
    assert reduced_nd == [2, 2, 1]
    assert strides == [[5, 0], [0, 7], [10, 5]]
    combos = list(itertools.product(range(3), range(2)))
    for idx, combo in enumerate(combos):
        assert divmod(idx, 2) == combo
        # digit x = (t // weight) % radix, weights (2, 1)
        assert ((idx // 2) % 3, idx % 2) == combo
    # the other order of labels: t most significant
    nassign, _, strides = hiplib.plan_slices(leaves, steps, [t, s])
    assert nassign == 6
    assert strides == [[0, 5], [7, 0], [5, 10]]


@pytest.mark.parametrize("labels, word", [
    ([99], "no leaf"),           # unknown label
    ([2, 2], "twice"),           # duplicate
    ([5], "final tensor"),       # j: an open leg of the result
    ([7], "final tensor"),       # carried by one leaf only
])
def test_refusals(labels, word):
    leaves = [([1, 2, 3], [3, 3, 5]), ([3, 4, 5], [5, 2, 7]),
              ([2, 4, 6, 7], [3, 2, 5, 1])]
    steps = [(0, 1), (0, 2)]
    L = hiplib.lib()
    rc = L.tn_plan_slices(
        0, hiplib._u64arr([l for ls, _ in leaves for l in ls]),
        hiplib._u64arr([d for _, ds in leaves for d in ds]),
        hiplib._u64arr([len(ls) for ls, _ in leaves]), len(leaves),
        hiplib._u64arr([x for p in steps for x in p]), len(steps),
        hiplib._u64arr(labels), len(labels), None, None, None)
    assert rc == 1  # TN_ERR_INVALID
    msg = hiplib.last_error()
    assert msg and word in msg, msg
    with pytest.raises(RuntimeError, match="tn_plan_slices"):
        hiplib.plan_slices(leaves, steps, labels)


def test_refuses_three_carriers_overflow_and_bad_path():
    # label 9 on three leaves: the symmetric difference keeps it open
    leaves = [([1, 9], [2, 2]), ([1, 9], [2, 2]), ([9], [2])]
    with pytest.raises(RuntimeError):
        hiplib.plan_slices(leaves, [(0, 1), (0, 2)], [9])
    # on four leaves it contracts away pairwise, but which pair a fixed
    # value belongs to is not one edge's business
    leaves = [([1, 9], [2, 2]), ([1, 9], [2, 2]), ([2, 9], [2, 2]),
              ([2, 9], [2, 2])]
    with pytest.raises(RuntimeError, match="4 leaves, not two"):
        hiplib.plan_slices(leaves, [(0, 1), (2, 3), (0, 2)], [9])
    # 2 labels of dim 2^33: 2^66 assignments
    big = 1 << 33
    leaves = [([1, 2], [big, big]), ([1, 2], [big, big])]
    with pytest.raises(RuntimeError, match="overflows"):
        hiplib.plan_slices(leaves, [(0, 1)], [1, 2])
    # a path plan_layouts refuses
    leaves = [([1], [2]), ([1], [2])]
    with pytest.raises(RuntimeError, match="invalid contraction path"):
        hiplib.plan_slices(leaves, [(0, 0)], [1])


def test_no_labels_is_the_plain_plan(eagle):
    _, _, _, leaves, steps = eagle
    nassign, reduced_nd, strides = hiplib.plan_slices(
        _shapes(leaves), steps, [])
    assert nassign == 1
    assert reduced_nd == [len(t.legs) for t in leaves]
    assert all(row == [] for row in strides)


def test_arena_sizing(eagle):
    _, _, edges, leaves, steps = eagle
    plain = arena_bytes(leaves, steps, plan_steps(leaves, steps), 16)
    sliced = sliced_arena_bytes(leaves, steps, edges)
    assert sliced < plain
    # like with like: the unsliced walk under the sliced engine's own rule
    assert sliced < arena_bytes(leaves, steps, plan_steps(leaves, steps), 16,
                                exact_dot=True)
    infos = plan_steps(reduced_leaves(leaves, edges), steps)
    peak = max(s.m * s.n for s in infos) * 16
    final = infos[-1].m * infos[-1].n * 16
    assert sliced >= peak + final
    # c64 halves the element size, the rule stays
    sliced64 = sliced_arena_bytes(leaves, steps, edges, dtype="c64")
    infos64 = plan_steps(reduced_leaves(leaves, edges), steps, "c64")
    assert sliced64 >= (max(s.m * s.n for s in infos64)
                        + infos64[-1].m * infos64[-1].n) * 8
