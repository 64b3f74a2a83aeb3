"""All ranks of a sharded run in ONE process, for tests/test_shard_phases.py and tests/test_shard_host.py.

`ShardWorld` holds the W HipShardBackend objects of a partition on the current device and calls the backend's own phase
methods on each rank in turn; the host adds the W collective buffers in place of the all-reduce (float32, rank order —
one of the orders a real all-reduce may use), so every intermediate of an iteration can be looked at.  Nothing here starts
torch.distributed: build_shard_backend needs no process group (broadcast_theta returns at once without one).

The second half restates, from partition_mesh alone, how a global vector of the unsharded mesh maps onto owners and
interface slots (`ShardLayout`), and builds the meshes the two test files share (`mesh_case`).
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from helpers import load_npz, orc, split_nets, theta_from  # noqa: E402
from pinn_fem_amd import _capi  # noqa: E402
from pinn_fem_amd.dist import Shard, partition_mesh, shard_host_plan  # noqa: E402

f32 = np.float32


# ---------------------------------------------------------------------------------------------------
# the layout of a partition on the host (no GPU)
# ---------------------------------------------------------------------------------------------------
@dataclass
class ShardLayout:
    """What partition_mesh gives for every rank, restated as global index sets."""
    shards: List[Shard]
    dofs_global: List[np.ndarray]      # per rank: global dof of each local dof
    n_dofs: int
    n_iface: int
    slot_dof: np.ndarray               # global dof of every interface slot (-1: no rank holds the slot)
    holders: np.ndarray                # (world, n_iface) bool: the rank holds a copy of the slot's dof

    @property
    def world(self):
        return len(self.shards)

    def owned(self, r):
        """Global dofs rank r owns (the entries global_vector takes from it)."""
        return self.dofs_global[r][~self.shards[r].ghost_mask]


def shard_layout(elements, n_nodes, dim, world) -> ShardLayout:
    shards = [partition_mesh(elements, n_nodes, dim, r, world) for r in range(world)]
    comp = np.arange(dim)
    dofs = [(s.nodes_global[:, None] * dim + comp[None, :]).reshape(-1) for s in shards]
    n_iface = shards[0].n_iface
    slot_dof = -np.ones(n_iface, dtype=np.int64)
    holders = np.zeros((world, n_iface), dtype=bool)
    for r, s in enumerate(shards):
        assert s.n_iface == n_iface
        g = dofs[r][s.shared_dofs]
        prev = slot_dof[s.shared_slot]
        assert np.all((prev < 0) | (prev == g)), "two ranks map one interface slot to different dofs"
        slot_dof[s.shared_slot] = g
        holders[r, s.shared_slot] = True
    return ShardLayout(shards=shards, dofs_global=dofs, n_dofs=n_nodes * dim, n_iface=n_iface, slot_dof=slot_dof,
                       holders=holders)


# ---------------------------------------------------------------------------------------------------
# meshes of the sharded tests
# ---------------------------------------------------------------------------------------------------
@dataclass
class MeshCase:
    name: str
    nodes: np.ndarray
    elements: np.ndarray
    loads: np.ndarray
    fixed: np.ndarray
    mv: np.ndarray
    md: np.ndarray
    dim: int
    widths: tuple
    scales: tuple
    theta: list

    @property
    def n_nodes(self):
        return self.nodes.shape[0]

    @property
    def n_dofs(self):
        return self.n_nodes * self.dim

    def make_model(self):
        """A fresh product model (an engine binds the material's parameters to its own flat buffer: one per rank)."""
        from helpers import product_model
        return product_model(self.nodes, self.elements, self.loads, self.fixed, self.dim, self.widths, self.scales,
                             [t.copy() for t in self.theta])

    def problem(self):
        """The oracle's Problem of the whole, unsharded mesh, with its own copy of theta."""
        nets = split_nets([t.copy() for t in self.theta])
        props, k = [], 0
        for w, sc in zip(self.widths, self.scales):
            if w is None:
                props.append(float(sc))
            else:
                props.append(orc.NetParams(nets[k], scale=float(sc)))
                k += 1
        return orc.Problem(nodes=self.nodes, elements=self.elements, loads=self.loads, fixed_dofs=self.fixed,
                           dimension=self.dim, young=props[0], area=props[1], density=props[2],
                           measured_vals=self.mv, measured_dofs=self.md)

    def layout(self, world):
        return shard_layout(self.elements, self.n_nodes, self.dim, world)


def mesh_case(name) -> MeshCase:
    """A / B: shuffled random trusses (the interface is most of the mesh: the single-block interface kernels make a
    second / third trip of their 1024-thread stride); C: a Warren girder (an interior; middle ranks have ghost elements
    on both sides); D: a 1-D bar with scalar E and A (DIM == 1, no net); A-E: mesh A with an E net only.
    The nets are the Warren fixture's (E 20 wide, A 15 wide)."""
    from dist_oracle_worker import random_truss
    from pinn_fem_amd.plan import warren_mesh
    rec = load_npz("step_warren_EA.npz")
    theta = theta_from(rec)
    widths, scales = (20, 15, None), (2.0, 0.5, 1.0)
    if name in ("A", "B", "A-E"):
        nodes, el, loads, fixed, md, mv = random_truss(3, 600 if name != "B" else 1200)
        if name == "A-E":
            widths, scales, theta = (20, None, None), (2.0, 0.5, 1.0), theta[:6]
        return MeshCase(name, nodes, el, loads, fixed, mv, md, 2, widths, scales, theta)
    if name == "C":
        nodes, el, loads, fixed, mv, md = warren_mesh(500)
        return MeshCase(name, nodes, el, loads, fixed, mv, md, 2, widths, scales, theta)
    assert name == "D"
    n = 300
    rng = np.random.default_rng(17)
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, n))]) * (3.0 / n)
    el = np.stack([np.arange(n), np.arange(1, n + 1)], axis=1)
    loads = rng.normal(size=n + 1) * 0.1
    fixed = np.array([0, 40, 150])                   # world 4: 40 is interior to rank 0, 150 is shared by ranks 1 and 2
    md = np.setdiff1d(np.arange(1, n + 1), fixed)[::2]
    mv = rng.normal(size=md.size) * 0.02
    return MeshCase(name, x, el, loads, fixed, mv, md, 1, (None, None, None), (3.0, 0.25, 1.0), [])


# ---------------------------------------------------------------------------------------------------
# the W ranks on one device
# ---------------------------------------------------------------------------------------------------
class ShardWorld:
    def __init__(self, make_model: Callable, mv, md, world: int, wg_mode=None, fe_mode=None, device=None):
        from pinn_fem_amd.dist import build_shard_backend
        self.world = int(world)
        self.backends = [build_shard_backend(make_model(), mv, md, r, self.world, device=device, wg_mode=wg_mode,
                                             fe_mode=fe_mode) for r in range(self.world)]
        first = self.theta_bytes(0)
        for r in range(1, self.world):
            assert self.theta_bytes(r) == first, "the ranks' theta differ: make_model must give every rank the same"
        b0 = self.backends[0]
        self.n_iface, self.n_theta_active = b0.n_iface, b0.n_theta_active
        self.n_buf = self.n_iface + self.n_theta_active + 3
        self.n_dofs = max(int(b.dofs_global.max()) for b in self.backends) + 1
        self.parts: List[np.ndarray] = []          # the W buffers as the last reduce() found them
        self.sum64: Optional[np.ndarray] = None    # their float64 sum
        self.sum32: Optional[np.ndarray] = None    # the float32 rank-order sum every rank received

    # -- access ---------------------------------------------------------------------------------------
    def _get(self, r, name):
        be = self.backends[r]
        if name in ("u", "m_u", "v_u"):
            return getattr(be.eng, name)
        n = be.eng.n_theta
        return {"theta": be.eng.theta.flat, "m_t": be.eng.m_t[:n], "v_t": be.eng.v_t[:n]}[name]

    def local(self, r, name) -> np.ndarray:
        import torch
        torch.cuda.synchronize()
        return self._get(r, name).detach().cpu().numpy().copy()

    def theta_bytes(self, r, name="theta") -> bytes:
        return self.local(r, name).tobytes()

    def buf(self, r) -> np.ndarray:
        import torch
        torch.cuda.synchronize()
        return self.backends[r].bufs[0].cpu().numpy().copy()

    def u2(self, r) -> np.float32:
        import torch
        torch.cuda.synchronize()
        return self.backends[r].bufs[1].cpu().numpy()[0]

    def fill_bufs(self, value):
        for be in self.backends:
            be.bufs[0].fill_(float(value))

    def state(self, r):
        return self.backends[r].state()

    def history(self, r, n_rows) -> np.ndarray:
        return self.backends[r].history(n_rows).copy()

    # -- phases -----------------------------------------------------------------------------------------
    def begin(self, u_global, lam, config):
        import torch
        u_global = np.asarray(u_global, dtype=f32)
        for be in self.backends:
            be.begin(torch.from_numpy(np.ascontiguousarray(u_global[be.dofs_global])), lam, config)

    def _each(self, fn):
        for be in self.backends:
            with be.eng.on_stream():
                fn(be)

    def forward(self):
        self._each(lambda be: be.forward())

    def backward(self):
        self._each(lambda be: be.backward(*be.bufs))

    def update_interior(self):
        self._each(lambda be: be.update_interior())

    def update_shared(self):
        self._each(lambda be: be.update_shared(*be.bufs))

    def _sum_to_all(self, tensors):
        """The all-reduce: float32 sum in rank order, the same bytes to every rank."""
        import torch
        torch.cuda.synchronize()
        parts = [t.cpu().numpy().copy() for t in tensors]
        s32 = parts[0].copy()
        for p in parts[1:]:
            s32 = (s32 + p).astype(f32)
        up = torch.from_numpy(s32)
        for t in tensors:
            t.copy_(up)
        return parts, s32

    def reduce(self):
        self.parts, self.sum32 = self._sum_to_all([be.bufs[0] for be in self.backends])
        self.sum64 = np.sum(np.stack(self.parts).astype(np.float64), axis=0)

    def flush(self):
        """dist._run_iterations' end of a chunk: the ranks' u2 reduced in the last slot of buf, then k_shard_flush."""
        lasts = [be.bufs[0][-1:] for be in self.backends]
        for be, last in zip(self.backends, lasts):
            last.copy_(be.bufs[1])
        self._sum_to_all(lasts)
        for be, last in zip(self.backends, lasts):
            with be.eng.on_stream():
                be.flush(last)

    def iteration(self):
        self.forward()
        self.backward()
        self.update_interior()
        self.reduce()
        self.update_shared()

    def iterate(self, n):
        """The sequence of dist._run_iterations."""
        for _ in range(int(n)):
            self.iteration()
        if n > 0:
            self.flush()

    # -- gathers ----------------------------------------------------------------------------------------
    def global_vector(self, name) -> np.ndarray:
        """u, m_u or v_u of the whole mesh: every dof from its owner."""
        out = np.full(self.n_dofs, np.nan, dtype=f32)
        for r, be in enumerate(self.backends):
            own = ~be.shard.ghost_mask
            out[be.dofs_global[own]] = self.local(r, name)[own]
        assert not np.any(np.isnan(out)), "a dof without an owner"
        return out

    def copies(self, name):
        """(values (world, n_iface) float32, held (world, n_iface) bool): what every holding rank has at every
        interface slot."""
        vals = np.zeros((self.world, self.n_iface), dtype=f32)
        held = np.zeros((self.world, self.n_iface), dtype=bool)
        for r, be in enumerate(self.backends):
            v = self.local(r, name)
            vals[r, be.shard.shared_slot] = v[be.shard.shared_dofs]
            held[r, be.shard.shared_slot] = True
        return vals, held

    def flags(self, r) -> np.ndarray:
        return self.backends[r].eng.plan.dof_flags


def measured_kept(shard: Shard, case: MeshCase) -> np.ndarray:
    """Global dofs whose data term rank `shard.rank` adds (the MEASURED flags of its shard_host_plan)."""
    hp, _ = shard_host_plan(shard, case.nodes, case.loads, case.fixed, case.mv, case.md, case.n_dofs)
    comp = np.arange(case.dim)
    dofs_g = (shard.nodes_global[:, None] * case.dim + comp[None, :]).reshape(-1)
    return dofs_g[(hp.dof_flags & _capi.PF_DOF_MEASURED) != 0]
