"""Host checks (no GPU) of the restatement tests/test_shard_phases.py uses to slice the oracle's output of the whole mesh
onto owners and interface slots (tests/shard_driver.py: ShardLayout), from partition_mesh / shard_host_plan alone, and of
the sizes that make the meshes worth running: interfaces longer than one and two trips of the interface kernels'
1024-thread stride, fixed shared dofs, ghost copies, ghost elements on both sides of a middle rank."""
import warnings

import numpy as np
import pytest

from shard_driver import measured_kept, mesh_case

CASES = [("A", 3), ("B", 2), ("C", 3), ("C", 5), ("D", 4)]


def _layout(name, world):
    case = mesh_case(name)
    with warnings.catch_warnings():
        # partition_mesh warns about an interface above 4096 floats; A and B stay below (1192, 2392): nothing to expect
        warnings.simplefilter("error", RuntimeWarning)
        return case, case.layout(world)


@pytest.mark.parametrize("name,world", CASES)
def test_owners_tile_the_global_dofs_once(name, world):
    case, L = _layout(name, world)
    count = np.zeros(case.n_dofs, dtype=int)
    for r in range(world):
        own = L.owned(r)
        assert np.unique(own).size == own.size
        count[own] += 1
    assert np.all(count == 1)
    # own elements tile the elements, and the local range [own_lo, own_hi) is exactly them
    seen = np.zeros(len(case.elements), dtype=int)
    for s in L.shards:
        seen[s.elems_global[s.own_lo:s.own_hi]] += 1
        assert np.array_equal(s.elems_global[s.own_lo:s.own_hi], np.arange(s.elem_lo, s.elem_hi))
        # local connectivity and numbering restate the global mesh
        assert np.array_equal(s.nodes_global[s.elements_local], case.elements[s.elems_global])
    assert np.all(seen == 1)


@pytest.mark.parametrize("name,world", CASES)
def test_interface_slots_and_their_holders(name, world):
    case, L = _layout(name, world)
    dim = case.dim
    assert np.all(L.slot_dof >= 0) and np.unique(L.slot_dof).size == L.n_iface     # every slot held, one dof per slot
    n_hold = L.holders.sum(axis=0)
    assert np.all(n_hold >= 1)
    # shared node: its elements live on several ranks -> at least those ranks hold it
    erank = np.empty(len(case.elements), dtype=int)
    for s in L.shards:
        erank[s.elem_lo:s.elem_hi] = s.rank
    ranks_of = [set() for _ in range(case.n_nodes)]
    for e, (a, b) in enumerate(case.elements):
        ranks_of[a].add(erank[e])
        ranks_of[b].add(erank[e])
    slot_node = L.slot_dof // dim
    shared_slot = np.array([len(ranks_of[n]) > 1 for n in slot_node])
    assert shared_slot.any()
    assert np.all(n_hold[shared_slot] >= 2)
    for k in np.flatnonzero(shared_slot):
        for r in ranks_of[slot_node[k]]:
            assert L.holders[r, k]
    for r, s in enumerate(L.shards):
        # a rank's interface dofs are exactly its local dofs that have a slot, in ascending order, each once
        assert np.all(np.diff(s.shared_dofs) > 0) and np.unique(s.shared_slot).size == s.shared_slot.size
        is_slot = np.isin(L.dofs_global[r], L.slot_dof)
        assert np.array_equal(np.flatnonzero(is_slot), s.shared_dofs)
        # the owner of every dof holds it; every ghost copy is an interface dof (its owner steps it from the same sum)
        assert np.all(is_slot[s.ghost_mask])
        # every dof of an OWN element whose other elements are not all on this rank is on the interface
        own_nodes = np.unique(case.elements[s.elem_lo:s.elem_hi])
        for n in own_nodes:
            if len(ranks_of[n]) > 1:
                assert np.all(np.isin(n * dim + np.arange(dim), L.slot_dof))


@pytest.mark.parametrize("name,world", CASES)
def test_measured_dofs_are_kept_by_their_owner_only(name, world):
    case, L = _layout(name, world)
    count = np.zeros(case.n_dofs, dtype=int)
    with_owner = with_copy = 0
    for r, s in enumerate(L.shards):
        kept = measured_kept(s, case)
        assert np.all(np.isin(kept, L.owned(r)))
        count[kept] += 1
        held = L.slot_dof[L.holders[r]]
        m_held = np.intersect1d(held, case.md)
        with_owner += np.isin(m_held, L.owned(r)).sum()
        with_copy += (~np.isin(m_held, L.owned(r))).sum()
    want = np.zeros(case.n_dofs, dtype=int)
    want[case.md] = 1
    assert np.array_equal(count, want)
    # measured interface dofs exist both with their owner and with ranks that only hold a copy
    assert with_owner > 0 and with_copy > 0


def test_sizes_the_phase_tests_rely_on():
    fixed_shared = lambda case, L: [int(np.isin(L.dofs_global[r][s.shared_dofs], case.fixed).sum())
                                    for r, s in enumerate(L.shards)]
    case = mesh_case("A")
    L = case.layout(3)
    assert len(case.elements) == 1200 and L.n_iface == 1192
    assert [s.shared_dofs.size for s in L.shards] == [1190, 1174, 1178]           # > 1024: a second trip on every rank
    assert fixed_shared(case, L) == [9, 9, 9]
    assert [int(s.ghost_mask.sum()) for s in L.shards] == [280, 958, 1112]
    assert np.array_equal(np.sort(case.md), np.setdiff1d(np.arange(1200), case.fixed))   # every free dof is measured
    case = mesh_case("B")
    L = case.layout(2)
    assert [s.shared_dofs.size for s in L.shards] == [2392, 2392]                 # > 2048: a third trip
    assert fixed_shared(case, L) == [9, 9]
    case = mesh_case("C")
    assert len(case.elements) == 1999 and case.n_dofs == 2002
    for world, n_iface in ((3, 26), (5, 48)):
        L = case.layout(world)
        assert L.n_iface == n_iface                                               # almost every dof is interior
        sizes = [s.elem_hi - s.elem_lo for s in L.shards]
        assert len(set(sizes)) == 2 and sum(sizes) == 1999                        # odd split
        for s in L.shards[1:-1]:                                                  # ghost elements on both sides
            assert s.own_lo > 0 and s.own_hi < s.elems_global.size
        assert L.shards[-1].own_lo > 0 and L.shards[0].own_hi < L.shards[0].elems_global.size
    case = mesh_case("D")
    L = case.layout(4)
    assert case.dim == 1 and len(case.elements) == 300 and L.n_iface == 9
    assert fixed_shared(case, L) == [0, 1, 1, 0] and not case.theta
    assert [s.own_lo for s in L.shards] == [0, 1, 1, 1]
