"""HipEngine — host-side owner of the device buffers of one FEM model and driver of the HIP kernels.

PyTorch is used for device memory and streams only; all arithmetic of the path runs in
libpinnfem_hip.so through the C ABI (include/pinnfem_hip.h).  There is no CPU fallback: without a
GPU or without the built library construction raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import time
import warnings
from typing import List, Optional

import numpy as np
import torch

from . import _capi
from . import coarse as _coarse
from ._capi import PfProblem, PfState, PinnFemHipError
from .nets import FlatTheta, NetSpec, describe_module
from .plan import HostPlan, build_host_plan


def _require_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise PinnFemHipError(
            "no ROCm GPU visible: pinn_fem_amd runs its hot path only through the HIP kernels "
            "(gfx950) and has no CPU fallback")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _on_engine_stream(fn):
    """Run a HipEngine method on the engine's own HIP stream (hipGraph capture is not allowed on the
    default stream), ordered after the caller's current stream on entry and before it on exit."""
    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        with self.on_stream():
            return fn(self, *a, **k)
    return wrapper


class DeviceCoarse:
    """A coarse.CoarseSpace on the device and the pf_coarse record that points at it."""

    def __init__(self, cs, device, max_coarse=None):
        """max_coarse: size a_inv for this many columns instead of cs.n_coarse (a space that refresh() will replace by
        one with another column count)."""
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.space = cs
        self.node_agg, self.agg_off, self.zcoef = t(cs.node_agg), t(cs.agg_off), t(cs.zcoef)
        self.agg_ptr, self.agg_nodes = t(cs.agg_ptr), t(cs.agg_nodes)
        self.a_c = None                 # host copy of Z^T K Z as the device formed it
        self.a_inv_host = None
        self.max_coarse = max(cs.n_coarse, 1) if max_coarse is None else max(int(max_coarse), cs.n_coarse, 1)
        self.a_inv = torch.zeros(self.max_coarse ** 2, dtype=torch.float64, device=device)
        R = self.record = _capi.PfCoarse()
        R.n_agg, R.n_coarse = cs.n_agg, cs.n_coarse
        R.node_agg, R.agg_off, R.zcoef = self.node_agg.data_ptr(), self.agg_off.data_ptr(), self.zcoef.data_ptr()
        R.agg_ptr, R.agg_nodes, R.a_inv = self.agg_ptr.data_ptr(), self.agg_nodes.data_ptr(), self.a_inv.data_ptr()

    def refresh(self, cs):
        """Another space on the same aggregation, in place: the record keeps its pointers; zcoef, agg_off and n_coarse
        follow cs (the column count of an aggregate may change with the configuration, coarse.update_coarse_space)."""
        if not np.array_equal(cs.node_agg, self.space.node_agg) or cs.n_coarse > self.max_coarse:
            raise ValueError("DeviceCoarse.refresh: the new space is not one on the same node -> aggregate map")
        self.zcoef.copy_(torch.from_numpy(cs.zcoef))
        self.agg_off.copy_(torch.from_numpy(cs.agg_off))
        self.space, self.record.n_coarse = cs, cs.n_coarse
        self.a_c = self.a_inv_host = None

    def set_inverse(self, a_inv):
        self.a_inv_host = np.ascontiguousarray(a_inv, dtype=np.float64)
        if self.a_inv_host.size:
            self.a_inv[: self.a_inv_host.size].copy_(torch.from_numpy(self.a_inv_host.reshape(-1)))


class HipEngine:
    """Device-resident problem: mesh plan, flat theta, Adam state, workspaces."""

    def __init__(self, model, measured_disp=None, measured_dofs=None, device=None,
                 wg_mode: Optional[int] = None, n_part_blocks: Optional[int] = None,
                 host_plan: Optional[HostPlan] = None, fe_mode: Optional[int] = None,
                 iface=None, mlp_dtype: Optional[str] = None):
        self.lib = _capi.load()
        self.device = _require_gpu(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.model = model
        hp = host_plan or build_host_plan(model.nodes, model.elements, model.loads, model.fixed_dofs,
                                          model.dimension, measured_disp, measured_dofs)
        self.plan = hp
        dev = self.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.conn, self.egeo, self.ecent = t(hp.conn), t(hp.egeo), t(hp.ecent)
        self.adj_ptr, self.adj, self.adj_other = t(hp.adj_ptr), t(hp.adj), t(hp.adj_other)
        self.f_ext, self.dof_flags, self.meas_val = t(hp.f_ext), t(hp.dof_flags), t(hp.meas_val)
        self.has_measurements = measured_disp is not None and measured_dofs is not None
        # multi-GPU shard interface: (interface dofs int32[], their slots int32[], n_iface, (own_lo, own_hi))
        self.own_range = (0, 0)
        if iface is not None:
            self.shared_dofs, self.shared_slot = t(np.asarray(iface[0], dtype=np.int32)), t(np.asarray(iface[1], dtype=np.int32))
            self.n_shared, self.n_iface = int(len(iface[0])), int(iface[2])
            if len(iface) > 3 and iface[3] is not None:
                self.own_range = (int(iface[3][0]), int(iface[3][1]))
        else:
            self.shared_dofs = self.shared_slot = None
            self.n_shared = self.n_iface = 0

        # ---- nets: young, area evaluated; density's parameters only ride along in theta ----------
        mat = model.material
        self.specs: List[NetSpec] = []
        param_lists = []
        for prop in (mat.young, mat.area):
            if prop.is_trainable():
                spec = describe_module(prop.net)
                spec.positive = bool(prop.enforce_positive)
                spec.scale = float(prop.scale)
                if spec.in_dim != model.dimension + 1:
                    # the reference feeds [load_factor, x(, y)] whatever input_dim says
                    # (properties.py:116-125) and torch then raises a shape error
                    raise RuntimeError(
                        f"mat1 and mat2 shapes cannot be multiplied: NN input has {model.dimension + 1} "
                        f"columns [load_factor, x(, y)] but the net expects {spec.in_dim}")
                param_lists.append(prop.get_torch_params())
            else:
                spec = NetSpec(enabled=False, scale=float(prop.value()))
            self.specs.append(spec)
        n_active = sum(p.numel() for lst in param_lists for p in lst)
        if mat.density.is_trainable():
            param_lists.append(mat.density.get_torch_params())
        self.theta = FlatTheta(param_lists, dev)
        self.n_theta = self.theta.n
        self.n_theta_active = n_active
        self.tensor_off = torch.tensor(self.theta.tensor_off, dtype=torch.int32, device=dev)

        lib = self.lib
        pad_off, theta_off, pad_index = 0, 0, []
        self._net_offsets = []
        for spec in self.specs:
            if not spec.enabled:
                self._net_offsets.append((0, 0))
                continue
            cnt = lib.pf_net_pad_count(spec.in_dim, spec.width, spec.n_hidden)
            _capi.check(min(cnt, 0), "pf_net_pad_count")
            self._net_offsets.append((theta_off, pad_off))
            for q in range(spec.n_params):
                pad_index.append(pad_off + lib.pf_net_pad_index(spec.in_dim, spec.width, spec.n_hidden, q))
            pad_off += cnt
            theta_off += spec.n_params
        self.pad_total = pad_off
        self.pad_index = torch.tensor(pad_index if pad_index else [0], dtype=torch.int32, device=dev)

        if wg_mode is None:
            wg_mode = int(os.environ.get("PINNFEM_WG_MODE", _capi.PF_WG_MFMA32))
        if wg_mode == _capi.PF_WG_MFMA32 and any(sp.enabled and sp.width > _capi.PF_N32_WIDTH_MAX for sp in self.specs):
            wg_mode = _capi.PF_WG_MFMA44          # widths 31, 32: the exact-f32 4x4x1 engine (another HIP engine)
        self.wg_mode = wg_mode
        # precision of the MLP matrix products: "f32" (split-f16 operands, float32-grade) or "bf16" (plain bf16 operands);
        # the reduced-precision variant exists only in the MFMA32 engine
        if mlp_dtype is None:
            mlp_dtype = getattr(model, "_pf_mlp_dtype", None) or os.environ.get("PINNFEM_MLP_DTYPE", "f32")
        if mlp_dtype not in ("f32", "bf16"):
            raise ValueError(f"mlp_dtype must be 'f32' or 'bf16', got {mlp_dtype!r}")
        if mlp_dtype == "bf16" and wg_mode != _capi.PF_WG_MFMA32:
            raise NotImplementedError("mlp_dtype='bf16' needs the MFMA32 engine (net widths <= 30)")
        self.mlp_dtype = mlp_dtype
        # MFMA32 engine: operand images of the enabled nets; scale of the coordinates in the f16 gradient products
        op_off, self._op_off = 0, [0, 0]
        if wg_mode == _capi.PF_WG_MFMA32:
            for k, spec in enumerate(self.specs):
                if spec.enabled:
                    cnt = lib.pf_net_op_count(spec.in_dim, spec.width, spec.n_hidden)
                    _capi.check(min(cnt, 0), "pf_net_op_count")
                    self._op_off[k] = op_off
                    op_off += (cnt + 63) // 64 * 64
        self.net_op = torch.zeros(max(op_off, 1), dtype=torch.float32, device=dev)
        cmax = float(np.max(np.abs(hp.ecent))) if hp.n_elems else 1.0
        self.coord_exp = 14 - int(np.ceil(np.log2(max(cmax, 1e-30)))) if cmax > 0 else 0
        self.coord_exp = int(min(max(self.coord_exp, -100), 100))
        if fe_mode is None:
            fe_mode = int(os.environ.get("PINNFEM_FE_MODE", _capi.PF_FE_REFERENCE))
        self.fe_mode = fe_mode
        if n_part_blocks is None:
            n_part_blocks = int(os.environ.get("PINNFEM_PART_BLOCKS", 1024))
        self.n_part_blocks = max(1, min(int(n_part_blocks), _capi.PF_MAX_BLOCKS))

        f32 = dict(dtype=torch.float32, device=dev)
        nd, ne = hp.n_dofs, max(hp.n_elems, 1)
        self.u = torch.zeros(nd, **f32)
        self.u_alt = torch.zeros(nd, **f32)      # the iteration graph's second displacement vector (pf_problem.u_alt)
        self.m_u = torch.zeros(nd, **f32)
        self.v_u = torch.zeros(nd, **f32)
        self.m_t = torch.zeros(max(self.n_theta, 1), **f32)
        self.v_t = torch.zeros(max(self.n_theta, 1), **f32)
        self.theta_pad = torch.zeros(max(self.pad_total, 1), **f32)
        # second half of (theta, m_t, v_t): lets the iteration graph fold the parameter update into the next forward launch
        self.theta_alt = torch.zeros(3 * max(self.n_theta, 1), **f32)
        # two halves: the iteration graph ping-pongs between them (pf_problem.prop_double); everything else
        # uses the first
        self.prop_e = torch.zeros(2 * ne, **f32)
        self.prop_a = torch.zeros(2 * ne, **f32)
        # entries of ke = s*pattern per element (s*c2, s*cs, s*s2; 1-D: s), written by the MFMA32 forward pass for the node
        # kernels (two halves, like the properties)
        self.elem_k = (torch.zeros(2 * ne * (3 if hp.dim == 2 else 1), **f32)
                       if self.wg_mode == _capi.PF_WG_MFMA32 and any(sp.enabled for sp in self.specs) else None)
        self.g_f = torch.zeros(nd, **f32)
        self.g_ea = torch.zeros(ne, **f32)
        self.grad_u = torch.zeros(nd, **f32)
        self.grad_theta = torch.zeros(max(self.n_theta, 1), **f32)
        size_probe = PfProblem()                      # the library owns the workspace layout: ask it for the size
        size_probe.n_part_blocks, size_probe.pad_total = self.n_part_blocks, max(self.pad_total, 1)
        self.partials = torch.zeros(int(self.lib.pf_partials_count(C.byref(size_probe))), **f32)
        self.state_t = torch.zeros(C.sizeof(PfState) // 4, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(1, **f32)
        self.hist_rows = 0
        self.P = PfProblem()
        self._graph = None
        self.pcg_iterations = 0         # CG iterations of every pcg_solve so far (tools/nr_scale.py reports them)
        self._coarse_cache = None       # (key, DeviceCoarse | None): coarse space of the two-level CG preconditioner
        self._coarse_updated = None     # (aggregation key, DeviceCoarse, A_c buffer) of preconditioner "two-level-updated"
        self.coarse_refresh_seconds = 0.0   # host seconds in the refreshes of that space so far, and their parts
        self.coarse_refresh_parts = dict(columns=0.0, setup=0.0, factor=0.0, upload=0.0)
        self.coarse_refreshes = 0       # updated_coarse_space refreshes so far
        self.pcg_batch_solves = 0       # pcg_solve_batch calls so far
        self._fixed_views = {}          # extra fixed dofs (tuple) -> (device dof_flags copy, PfProblem view, host fixed mask)
        self._gl = None                 # Green-Lagrange element buffers (d0, kt, fe, strain) and their pf_gl record
        self._gl_cable = None           # gl_state_cable: [device flags, slack set, counts, whether a cable state has run]
        self._gl_plastic = None         # gl_state_plastic: the committed and trial (ep, alpha), flags, counts (_gl_plastic_buffers)
        self._dyn = None                # explicit dynamics: buffers, pf_dyn record, step count and graphs of the run (dyn_begin)
        self._group_csr = None          # group_sum: (key of the group map, n_groups, device CSR pointer, device element ids)
        self._group_maps = {}           # _device_group_map: method name -> (key of its last map, n_groups, device int32 ids)
        self._configured = False
        env_k = os.environ.get("PINNFEM_GRAPH_ITERS")
        self.GRAPH_ITERS = int(env_k) if env_k else (self.GRAPH_ITERS_LARGE if hp.n_elems >= 200_000 else self.GRAPH_ITERS)
        self.configure(lam=1.0)

    # ------------------------------------------------------------------------------------------
    def _stream(self) -> int:
        return self.stream.cuda_stream

    @contextlib.contextmanager
    def on_stream(self):
        outer = torch.cuda.current_stream(self.device)
        if outer == self.stream:
            yield
            return
        self.stream.wait_stream(outer)
        with torch.cuda.stream(self.stream):
            yield
        outer.wait_stream(self.stream)

    def configure(self, lam: float, alpha_physics: float = 1.0, alpha_data: float = 100.0,
                  lr_u: float = 1e-7, lr_t: float = 1e-4, tol: float = 1e-6, max_iter: int = 0,
                  want_history: bool = True, want_grad_u: bool = False):
        """Fill the pf_problem record (scalars of SolverConfig + pointers)."""
        self._drop_graph()          # a captured graph holds the old record by value
        hp, P = self.plan, self.P
        M = P.mesh
        M.dim, M.n_nodes, M.n_elems, M.n_dofs = hp.dim, hp.n_nodes, hp.n_elems, hp.n_dofs
        M.conn, M.egeo, M.ecent = self.conn.data_ptr(), self.egeo.data_ptr(), self.ecent.data_ptr()
        M.adj_ptr, M.adj = self.adj_ptr.data_ptr(), self.adj.data_ptr()
        M.f_ext, M.dof_flags, M.meas_val = (self.f_ext.data_ptr(), self.dof_flags.data_ptr(),
                                            self.meas_val.data_ptr())
        M.n_meas = hp.n_meas
        for k, spec in enumerate(self.specs):
            n = P.net[k]
            n.enabled = int(spec.enabled)
            n.in_dim, n.width, n.n_hidden = spec.in_dim, spec.width, spec.n_hidden
            n.positive, n.scale = int(spec.positive), float(spec.scale)
            n.theta_off, n.pad_off = self._net_offsets[k]
        P.u, P.m_u, P.v_u = self.u.data_ptr(), self.m_u.data_ptr(), self.v_u.data_ptr()
        P.theta, P.m_t, P.v_t = self.theta.flat.data_ptr(), self.m_t.data_ptr(), self.v_t.data_ptr()
        P.n_theta, P.n_theta_active = self.n_theta, self.n_theta_active
        P.tensor_off, P.n_tensors = self.tensor_off.data_ptr(), len(self.theta.tensor_off) - 1
        P.wg_mode = self.wg_mode
        P.lam, P.alpha_physics, P.alpha_data = float(lam), float(alpha_physics), float(alpha_data)
        P.lr_u, P.lr_t, P.tol = float(lr_u), float(lr_t), float(tol)
        P.beta1, P.beta2, P.eps = 0.9, 0.999, 1e-8          # torch.optim.Adam defaults (solver.py:234)
        P.use_data = int(self.has_measurements and alpha_data > 0)   # solver.py:273
        P.max_iter = int(max_iter)
        P.theta_pad, P.prop_e, P.prop_a = (self.theta_pad.data_ptr(), self.prop_e.data_ptr(),
                                           self.prop_a.data_ptr())
        P.g_f, P.g_ea = self.g_f.data_ptr(), self.g_ea.data_ptr()
        P.grad_u = self.grad_u.data_ptr() if want_grad_u else None
        P.grad_theta, P.partials = self.grad_theta.data_ptr(), self.partials.data_ptr()
        if want_history and max_iter > 0:
            if self.hist_rows < max_iter:
                self.hist = torch.zeros(max_iter * _capi.PF_HIST_COLS, dtype=torch.float32,
                                        device=self.device)
                self.hist_rows = max_iter
            P.hist = self.hist.data_ptr()
        else:
            P.hist = None
        P.state = self.state_t.data_ptr()
        P.n_part_blocks, P.pad_total = self.n_part_blocks, self.pad_total
        P.pad_index = self.pad_index.data_ptr()
        P.n_meas_f = float(hp.n_meas)
        P.fe_mode = int(self.fe_mode)
        P.shared_dofs = self.shared_dofs.data_ptr() if self.n_shared else None
        P.shared_slot = self.shared_slot.data_ptr() if self.n_shared else None
        P.n_shared, P.n_iface = self.n_shared, self.n_iface
        P.own_lo, P.own_hi = self.own_range
        P.prop_double = 1
        P.net_op = self.net_op.data_ptr() if self.wg_mode == _capi.PF_WG_MFMA32 else None
        P.op_off[0], P.op_off[1] = self._op_off
        P.coord_exp = self.coord_exp
        P.mlp_dtype = _capi.PF_MLP_BF16 if self.mlp_dtype == "bf16" else _capi.PF_MLP_F32
        P.elem_k = self.elem_k.data_ptr() if self.elem_k is not None else None
        P.theta_alt = self.theta_alt.data_ptr() if self.n_theta_active > 0 else None
        P.u_alt = self.u_alt.data_ptr()
        P.adj_other = self.adj_other.data_ptr()
        self._configured = True

    def _ref(self):
        return C.byref(self.P)

    def _fixed_view(self, extra_fixed):
        """(pf_problem reference, host mask of the fixed dofs, key) with the dofs of extra_fixed constrained on top of the
        model's: a second device copy of dof_flags with PF_DOF_FIXED set on them and a PfProblem record that points at it,
        cached per dof tuple.  The plan, the engine's own flags and its record are never modified.  None or empty: the
        engine's own record."""
        hp = self.plan
        fixed = (hp.dof_flags & _capi.PF_DOF_FIXED) != 0
        if extra_fixed is None or len(extra_fixed) == 0:
            return self._ref(), fixed, ()
        key = tuple(sorted({int(d) for d in extra_fixed}))
        if key[0] < 0 or key[-1] >= hp.n_dofs:
            raise ValueError(f"extra_fixed: dofs {key} are not all in 0..{hp.n_dofs - 1}")
        if key not in self._fixed_views:
            flags = np.array(hp.dof_flags, copy=True)
            flags[list(key)] |= _capi.PF_DOF_FIXED
            mask = (flags & _capi.PF_DOF_FIXED) != 0
            self._fixed_views[key] = (torch.from_numpy(np.ascontiguousarray(flags)).to(self.device), PfProblem(), mask)
        flags_t, view, mask = self._fixed_views[key]
        C.memmove(C.byref(view), C.byref(self.P), C.sizeof(PfProblem))      # the record as configured now
        view.mesh.dof_flags = flags_t.data_ptr()
        return C.byref(view), mask, key

    def fusion_info(self) -> int:
        """Bit mask of the fused launches of this problem (_capi.PF_FUSED_*)."""
        return int(self.lib.pf_fusion_info(self._ref()))

    @_on_engine_stream
    def graph_form_info(self) -> int:
        """Bit mask of the iteration graph's form beyond fusion_info() (_capi.PF_GRAPH_FORM_*): 1 = the residual launch is
        folded into the fused backward and theta-stage-1 launches (path meshes).  Inspects the mesh on the device."""
        return int(self.lib.pf_graph_form_info(self._ref()))

    @_on_engine_stream
    def graph_light_forward(self) -> int:
        """1 where the iteration graph's path form runs with the light forward (the forward launch evaluates the E net only
        at task edges, the fused backward stores prop_e and the other stiffness records), else 0.  Inspects the mesh on
        the device."""
        return int(self.lib.pf_graph_light_forward(self._ref()))

    @_on_engine_stream
    def graph_ordered_path(self) -> int:
        """1 where the iteration graph runs its path form on a mesh whose node ids follow the path (element e joins node e
        to node e + 1), so that its node tasks address by node id instead of through the adjacency, else 0.  Inspects the
        mesh on the device."""
        return int(self.lib.pf_graph_ordered_path(self._ref()))

    # ---- solve_gd support ------------------------------------------------------------------------
    @_on_engine_stream
    def begin(self, u_initial, lam, config, max_iter: Optional[int] = None, want_history=True):
        """Start one solve_gd call: fresh Adam state (solver.py:234-238), u = warm start or 0."""
        if self.n_theta and not self.theta.still_bound():
            raise PinnFemHipError("a network parameter was re-assigned outside the engine; "
                                  "rebuild the engine for this model")
        self.configure(lam=lam, alpha_physics=config.alpha_physics, alpha_data=config.alpha_data,
                       lr_u=config.learning_rate_u, lr_t=config.learning_rate_theta,
                       tol=config.tolerance,
                       max_iter=config.max_iterations if max_iter is None else max_iter,
                       want_history=want_history)
        if u_initial is None:
            self.u.zero_()
        else:
            src = u_initial.detach() if isinstance(u_initial, torch.Tensor) else torch.as_tensor(
                np.asarray(u_initial))
            self.u.copy_(src.reshape(-1).to(device=self.device, dtype=torch.float32))
        s = self._stream()
        self._pending_tail = False          # (a new solve: nothing of the previous one is pending)
        _capi.check(self.lib.pf_reset(self._ref(), s), "pf_reset")
        _capi.check(self.lib.pf_pack_theta(self._ref(), s), "pf_pack_theta")

    # iterations per captured hipGraph.  A PLAIN replay ends with ~45 us of stand-alone kernels (parameter update, displacement
    # update, finalize) that the iterations inside it do not pay, so large meshes replay 20 at a time (the host polls the stop
    # flag every 50 anyway); small meshes keep 10 (a graph is captured per solve_gd call: capture time counts there).
    # Chained replays (iterate(defer_tail=True)) pay that tail once per solve.
    # PINNFEM_GRAPH_ITERS overrides both (even numbers: the graph ping-pongs state between two halves).
    GRAPH_ITERS = 10
    GRAPH_ITERS_LARGE = 20

    def _drop_graph(self):
        g = getattr(self, "_graph", None)
        if g:
            self.lib.pf_graph_destroy(g)
        self._graph = None
        for h in getattr(self, "_chain_graphs", {}).values():
            if h:
                self.lib.pf_graph_destroy(h)
        self._chain_graphs = {}

    graph_creates = 0        # hipGraph captures + instantiations so far (bench.py asserts none is timed)
    _pending_tail = False    # a chained replay has left its last iteration's updates / bookkeeping pending (see iterate)

    @_on_engine_stream
    def prepare_graph(self, chained: bool = False):
        """Capture and instantiate the iteration hipGraph of the current pf_problem record now (it is
        otherwise created by the first iterate() call that replays it).  Enqueues no iteration.
        chained: also the two graphs of chained replays (iterate(defer_tail=True)); returns whether the problem has them."""
        if getattr(self, "_graph", None) is None:
            g = C.c_void_p()
            _capi.check(self.lib.pf_graph_create(self._ref(), self.GRAPH_ITERS, self._stream(), C.byref(g)),
                        "pf_graph_create")
            self._graph = g
            self.graph_creates += 1
        if not chained:
            return True
        if not hasattr(self, "_chain_graphs"):
            self._chain_graphs = {}
        for flags in (_capi.PF_GRAPH_NO_TAIL, _capi.PF_GRAPH_NO_TAIL | _capi.PF_GRAPH_CONT_HEAD):
            if flags not in self._chain_graphs:
                g = C.c_void_p()
                rc = self.lib.pf_graph_create_ex(self._ref(), self.GRAPH_ITERS, flags, self._stream(), C.byref(g))
                if rc == _capi.PF_ERR_UNSUPPORTED:
                    self._chain_graphs[flags] = None        # (not the one-chain form: plain replays)
                    continue
                _capi.check(rc, "pf_graph_create_ex")
                self._chain_graphs[flags] = g
                self.graph_creates += 1
        return all(self._chain_graphs.get(f) for f in (2, 3))

    @_on_engine_stream
    def flush(self):
        """Run the pending tail of chained replays (parameter update, displacement update and bookkeeping of the last
        iteration).  iterate() calls it before anything but another chained replay; call it before reading the state."""
        if self._pending_tail:
            _capi.check(self.lib.pf_graph_tail(self._ref(), self.GRAPH_ITERS, self._stream()), "pf_graph_tail")
            self._pending_tail = False

    @_on_engine_stream
    def iterate(self, n_iter: int, use_graph: Optional[bool] = None, defer_tail: bool = False):
        """Enqueue n_iter GD iterations.  Whole multiples of GRAPH_ITERS replay a captured hipGraph
        (created lazily per begin(), or ahead of time by prepare_graph(); the graph bakes in the current
        pf_problem record), the remainder is launched eagerly.  Launches after the device-side stop are
        no-ops either way.
        defer_tail: the replays are CHAINED where the problem allows it — a replay ends behind its last gradient-row
        reduction and the next replay's first iteration carries that iteration's updates and bookkeeping, like every other
        iteration of a replay carries its predecessor's; the ~45 us of stand-alone launches a plain replay ends with are
        paid once, by flush().  state() / history() / u / theta lag by that one iteration until flush()."""
        n_iter = int(n_iter)
        if use_graph is None:
            use_graph = os.environ.get("PINNFEM_GRAPH", "1") != "0"
        s = self._stream()
        k = self.GRAPH_ITERS
        if use_graph and n_iter >= k:
            chained = defer_tail and self.prepare_graph(chained=True)
            if not chained:
                self.flush()
                self.prepare_graph()
            while n_iter >= k:
                if chained:
                    g = self._chain_graphs[3 if self._pending_tail else 2]
                    _capi.check(self.lib.pf_graph_launch(g, s), "pf_graph_launch")
                    self._pending_tail = True
                else:
                    _capi.check(self.lib.pf_graph_launch(self._graph, s), "pf_graph_launch")
                n_iter -= k
        if n_iter > 0:
            self.flush()
            _capi.check(self.lib.pf_gd_iterations(self._ref(), n_iter, s), "pf_gd_iterations")

    def __del__(self):
        try:
            self._drop_graph()
            self._drop_dyn_graphs()
        except Exception:
            pass

    @_on_engine_stream
    def iterate_timed(self, n_iter: int) -> np.ndarray:
        """Like iterate() but with HIP events around every kernel; synchronises.  Returns the average
        milliseconds of each kernel slot (_capi.KERNEL_SLOT_NAMES)."""
        out = (C.c_float * _capi.PF_KERNEL_SLOTS)()
        _capi.check(self.lib.pf_gd_iterations_timed(self._ref(), int(n_iter), self._stream(), out),
                    "pf_gd_iterations_timed")
        return np.array(list(out), dtype=np.float64)

    @_on_engine_stream
    def time_step_launch(self, what: str, reps: int = 20) -> float:
        """Average device time (ms) of `reps` back-to-back launches of one step of the current iteration state — "backward":
        the backward pass of every enabled net incl. the element adjoint, "forward": the forward pass of every enabled net —
        between two HIP events on the engine's stream (no launch gaps inside: the launches queue up behind each other).
        Idempotent steps: they read the state and rewrite workspaces only."""
        fn = {"backward": self.lib.pf_net_backward_all, "forward": self.lib.pf_net_forward_all}[what]
        s = self._stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            _capi.check(fn(self._ref(), s), what)
        e0.record(self.stream)
        for _ in range(int(reps)):
            _capi.check(fn(self._ref(), s), what)
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / float(reps)

    @_on_engine_stream
    def state(self) -> PfState:
        raw = self.state_t.cpu().numpy().tobytes()
        return PfState.from_buffer_copy(raw)

    @_on_engine_stream
    def history(self, n_rows: int) -> np.ndarray:
        if n_rows <= 0 or self.P.hist is None:
            return np.zeros((0, _capi.PF_HIST_COLS), dtype=np.float32)
        return self.hist[: n_rows * _capi.PF_HIST_COLS].cpu().numpy().reshape(n_rows, _capi.PF_HIST_COLS)

    # ---- building blocks -------------------------------------------------------------------------
    @_on_engine_stream
    def eval_properties(self, lam: Optional[float] = None):
        """young/area per element with the current theta (pf_pack_theta + pf_net_forward)."""
        if lam is not None:
            self.P.lam = float(lam)
        s = self._stream()
        self._clear_done()
        _capi.check(self.lib.pf_pack_theta(self._ref(), s), "pf_pack_theta")
        for k, spec in enumerate(self.specs):
            if spec.enabled:
                _capi.check(self.lib.pf_net_forward(self._ref(), k, s), "pf_net_forward")

    def _clear_done(self):
        # building-block calls outside a solve_gd run must not be masked by a finished run
        self.state_t[1] = 0

    @_on_engine_stream
    def internal_force(self, u: Optional[torch.Tensor] = None, lam: Optional[float] = None) -> torch.Tensor:
        """f_int = K(theta) u, re-evaluating the nets (the reference's no-grad re-assembly,
        solver.py:374-377)."""
        self.eval_properties(lam)
        uu = self.u if u is None else u.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(self.plan.n_dofs, dtype=torch.float32, device=self.device)
        _capi.check(self.lib.pf_internal_force(self._ref(), uu.data_ptr(), out.data_ptr(), self._stream()),
                    "pf_internal_force")
        return out

    @_on_engine_stream
    def loss_and_grads(self, u: torch.Tensor, lam: float, alpha_physics=1.0, alpha_data=100.0):
        """One forward+backward without optimiser step.  Returns (dict of loss terms, grad_u,
        grad_theta) as device tensors (views of engine workspaces)."""
        self.configure(lam=lam, alpha_physics=alpha_physics, alpha_data=alpha_data, want_history=False,
                       want_grad_u=True)
        self.u.copy_(u.reshape(-1).to(device=self.device, dtype=torch.float32))
        s = self._stream()
        self._clear_done()
        _capi.check(self.lib.pf_pack_theta(self._ref(), s), "pf_pack_theta")
        _capi.check(self.lib.pf_loss_and_grads(self._ref(), s), "pf_loss_and_grads")
        st = self.state()
        losses = dict(loss_total=st.loss_total, loss_physics=st.loss_physics, loss_data=st.loss_data,
                      residual_norm=st.residual_norm)
        return losses, self.grad_u, self.grad_theta[: max(self.n_theta_active, 0)]

    @_on_engine_stream
    def vjp(self, u: torch.Tensor, g_f: torch.Tensor, lam: float):
        """(K^T g_f, d(g_f . f_int)/dtheta): the backward of f_int = K(theta) u for an arbitrary
        upstream gradient (autograd.Function backward)."""
        self.configure(lam=lam, alpha_data=0.0, want_history=False, want_grad_u=True)
        self.P.use_data = 0
        self.u.copy_(u.reshape(-1).to(device=self.device, dtype=torch.float32))
        self.g_f.copy_(g_f.reshape(-1).to(device=self.device, dtype=torch.float32))
        s, lib, ref = self._stream(), self.lib, self._ref()
        self._clear_done()
        _capi.check(lib.pf_pack_theta(ref, s), "pf_pack_theta")
        any_net = False
        for k, spec in enumerate(self.specs):
            if spec.enabled:
                any_net = True
                _capi.check(lib.pf_net_forward(ref, k, s), "pf_net_forward")
        if any_net:
            _capi.check(lib.pf_elem_adjoint(ref, s), "pf_elem_adjoint")
            for k, spec in enumerate(self.specs):
                if spec.enabled:
                    _capi.check(lib.pf_net_backward(ref, k, s), "pf_net_backward")
        _capi.check(lib.pf_node_gradu(ref, 0, s), "pf_node_gradu")
        if any_net:
            _capi.check(lib.pf_theta_reduce(ref, 0, s), "pf_theta_reduce")
        return self.grad_u, self.grad_theta[: max(self.n_theta_active, 0)]

    # ---- classical Newton-Raphson support: float64 matrix-free K v and Jacobi-PCG (pf_pcg.hip) ---------
    @_on_engine_stream
    def kv_f64(self, v: torch.Tensor, zero_fixed: bool = False) -> torch.Tensor:
        """K(E, A) v in float64 (fem/assembly.py:16-75 without forming K).  NN properties, if any, must
        have been evaluated (eval_properties)."""
        vv = v.to(device=self.device, dtype=torch.float64).contiguous()
        out = torch.empty(self.plan.n_dofs, dtype=torch.float64, device=self.device)
        _capi.check(self.lib.pf_kv_f64(self._ref(), vv.data_ptr(), out.data_ptr(), int(zero_fixed), self._stream()),
                    "pf_kv_f64")
        return out

    # ---- large displacements: the Green-Lagrange element (pf_nl.hip) and its tangent operator --------------------
    def _gl_buffers(self):
        """(d0, kt, fe, strain, pf_gl record), allocated on first use.  d0 = X_j - X_i comes from the model's float64
        coordinates, not from the plan's float32 geometry."""
        if self._gl is None:
            hp = self.plan
            if len(self.model.nodes) != hp.n_nodes:
                raise ValueError("the Green-Lagrange element needs the engine's mesh to be the model's "
                                 "(no sharded form)")
            nodes = np.asarray(self.model.nodes, dtype=np.float64).reshape(hp.n_nodes, hp.dim)
            conn = np.asarray(hp.conn, dtype=np.int64).reshape(-1, 2)
            ne = max(hp.n_elems, 1)
            d0 = torch.zeros(ne * hp.dim, dtype=torch.float64, device=self.device)
            if hp.n_elems:
                d0[: hp.n_elems * hp.dim] = torch.from_numpy(
                    np.ascontiguousarray(nodes[conn[:, 1]] - nodes[conn[:, 0]]).reshape(-1)).to(self.device)
            f64 = dict(dtype=torch.float64, device=self.device)
            kt = torch.zeros(ne * (3 if hp.dim == 2 else 1), **f64)
            fe, strain = torch.zeros(ne * hp.dim, **f64), torch.zeros(ne, **f64)
            rec = _capi.PfGl()
            rec.d0, rec.kt, rec.fe, rec.strain = d0.data_ptr(), kt.data_ptr(), fe.data_ptr(), strain.data_ptr()
            self._gl = (d0, kt, fe, strain, rec)
        return self._gl

    def _f64_vector(self, who, name, v, count, what):
        vv = v.to(device=self.device, dtype=torch.float64).contiguous().reshape(-1)
        if vv.numel() != count:
            raise ValueError(f"{who}: {name} has {vv.numel()} entries, the mesh has {count} {what}")
        return vv

    def _accumulator(self, who, out, n, new):
        """(the float64 device vector [n] a kernel writes, whether it ADDS to it): out, checked, or new(n, ...) for None."""
        if out is None:
            return new(n, dtype=torch.float64, device=self.device), False
        if out.dtype != torch.float64 or out.device != self.device or not out.is_contiguous() or out.numel() != n:
            raise ValueError(f"{who}: out must be a contiguous float64 vector of {n} entries on {self.device}")
        return out, True

    def _group_ids(self, who, groups, lowest=0, bound=None):
        """A group map checked: (ids int64 [n_elems], their bytes as a cache key, number of groups).  lowest: the lowest id
        admitted, 0 or -1 (the element belongs to no group); bound: ids must stay below it."""
        ne = self.plan.n_elems
        gm = np.ascontiguousarray(np.asarray(groups).reshape(-1))
        top = int(gm.max()) if gm.size and gm.dtype.kind in "iu" else -1
        if gm.size != ne or (ne and (gm.dtype.kind not in "iu" or gm.min() < lowest or (bound is not None and top >= bound))):
            what = "non-negative group id" if lowest == 0 else f"group id >= {lowest}"
            raise ValueError(f"{who}: groups must hold one {what} for each of the {ne} elements")
        gm = gm.astype(np.int64, copy=False)         # read only from here on
        return gm, gm.tobytes(), top + 1

    def _device_group_map(self, who, groups, lowest=0):
        """(number of groups, device int32 ids) of a group map; each method keeps its last map's copy, since the joint
        identification calls gl_group_rhs and gl_prestress_rhs in turn with two maps."""
        gm, key, n_groups = self._group_ids(who, groups, lowest, bound=2 ** 31)
        if who not in self._group_maps or self._group_maps[who][0] != key:
            ids = gm.astype(np.int32) if gm.size else np.zeros(1, dtype=np.int32)
            self._group_maps[who] = (key, n_groups, torch.from_numpy(ids).to(self.device))
        return self._group_maps[who][1:]

    @staticmethod
    def _group_range(who, n_groups, g0, m):
        g0, m = int(g0), n_groups - int(g0) if m is None else int(m)
        if g0 < 0 or m < 1:
            raise ValueError(f"{who}: no groups in the range asked for (g0 = {g0}, m = {m}, {n_groups} groups)")
        return g0, m

    @_on_engine_stream
    def gl_state(self, u: torch.Tensor, ea: Optional[torch.Tensor] = None, e0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Green-Lagrange strain, element force and tangent block of every element at the displacements u (float64,
        pf_gl_state); they stay on the device for gl_fint, kt_v_f64, kt_diag and pcg_solve(tangent=True).  ea: E*A of every
        element [n_elems] in float64 in place of the model's (pf_gl_state_ea; the identification of fem/identify.py).
        e0: the initial strain of every element [n_elems] in float64 (pf_gl_state_e0: N = E*A (e - e0); prestress, thermal
        strain, lack of fit).  The engine keeps no e0 of its own: every call that wants it passes it.
        Returns the total strains e [n_elems] (the engine's buffer: the next gl_state overwrites it)."""
        uu = self._f64_vector("gl_state", "u", u, self.plan.n_dofs, "dofs")
        rec = self._gl_buffers()[4]
        ee = None if ea is None else self._f64_vector("gl_state", "ea", ea, self.plan.n_elems, "elements")
        if e0 is not None:
            zz = self._f64_vector("gl_state", "e0", e0, self.plan.n_elems, "elements")
            if self.plan.n_elems:
                _capi.check(self.lib.pf_gl_state_e0(self._ref(), C.byref(rec), None if ee is None else ee.data_ptr(),
                                                    zz.data_ptr(), uu.data_ptr(), self._stream()), "pf_gl_state_e0")
        elif ee is None:
            _capi.check(self.lib.pf_gl_state(self._ref(), C.byref(rec), uu.data_ptr(), self._stream()), "pf_gl_state")
        elif self.plan.n_elems:
            _capi.check(self.lib.pf_gl_state_ea(self._ref(), C.byref(rec), ee.data_ptr(), uu.data_ptr(), self._stream()),
                        "pf_gl_state_ea")
        return self._gl[3][: self.plan.n_elems]

    @_on_engine_stream
    def gl_state_cable(self, u: torch.Tensor, cable, ea: Optional[torch.Tensor] = None,
                       e0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gl_state with tension-only elements (pf_gl_state_cable).  cable: bool or uint8 [n_elems]; a flagged element with
        e - e0 < 0 is slack, its force and tangent block are +0.0.  ea, e0: as gl_state's.  The engine owns the slack set and
        its counts: gl_slack_counts() and gl_slack_mask() read those of the last call, gl_slack_clear() empties the set at the
        start of a solve.  Returns the total strains e [n_elems], the buffer gl_state returns.  (A method of its own:
        gl_state keeps its parameters and its calls.)"""
        who = "gl_state_cable"
        uu = self._f64_vector(who, "u", u, self.plan.n_dofs, "dofs")
        rec = self._gl_buffers()[4]
        ee = None if ea is None else self._f64_vector(who, "ea", ea, self.plan.n_elems, "elements")
        zz = None if e0 is None else self._f64_vector(who, "e0", e0, self.plan.n_elems, "elements")
        c = self._gl_cable_buffers()
        c[0] = self._cable_flags(cable, self.plan.n_elems, who)
        flags = c[0] if self.plan.n_elems else c[1]         # (an empty mesh: any non-null pointer, nothing reads it)
        _capi.check(self.lib.pf_gl_state_cable(self._ref(), C.byref(rec), None if ee is None else ee.data_ptr(),
                                               None if zz is None else zz.data_ptr(), flags.data_ptr(), c[1].data_ptr(),
                                               c[2].data_ptr(), uu.data_ptr(), self._stream()), "pf_gl_state_cable")
        c[3] = True
        return self._gl[3][: self.plan.n_elems]

    def _gl_cable_buffers(self):
        if self._gl_cable is None:
            slack = torch.zeros(max(self.plan.n_elems, 1), dtype=torch.uint8, device=self.device)
            counts = torch.zeros(_capi.PF_GL_CABLE_COUNT, dtype=torch.float64, device=self.device)
            self._gl_cable = [None, slack, counts, False]
        return self._gl_cable

    def _gl_cable_ready(self, who):
        if self._gl_cable is None or not self._gl_cable[3]:
            raise RuntimeError(f"{who}: no cable state yet; call gl_state_cable(u, cable) first")
        return self._gl_cable

    @_on_engine_stream
    def gl_slack_clear(self):
        """Empty the slack set gl_state_cable keeps: the start of a solve."""
        self._gl_cable_buffers()[1].zero_()

    @_on_engine_stream
    def gl_slack_counts(self):
        """(number of slack elements, number of elements whose flag changed against the set before) of the last
        gl_state_cable: one read of 16 bytes."""
        n = self._gl_cable_ready("gl_slack_counts")[2][:2].cpu()
        return int(n[0]), int(n[1])

    @_on_engine_stream
    def gl_slack_mask(self) -> np.ndarray:
        """The slack elements of the last gl_state_cable, bool [n_elems] on the host."""
        return self._gl_cable_ready("gl_slack_mask")[1][: self.plan.n_elems].cpu().numpy().astype(bool)

    @_on_engine_stream
    def gl_state_plastic(self, u: torch.Tensor, ey, kappa, ea: Optional[torch.Tensor] = None,
                         e0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gl_state with elastoplastic elements (pf_gl_state_plastic).  ey: the yield strain of every element
        [n_elems] (inf: never yields), kappa: the hardening ratio H / E [n_elems]; ea, e0: as gl_state's.  The engine owns the
        committed (ep, alpha), the trial pair the kernel writes, the flags and the counts.  Every call starts from the
        committed state: gl_plastic_commit() makes the last call's trial state the committed one (a swap of the buffers),
        gl_plastic_reset() sets it, gl_plastic_counts() and gl_plastic_state() read the last call's.  Returns the total
        strains e [n_elems], the buffer gl_state returns."""
        who = "gl_state_plastic"
        ne = self.plan.n_elems
        uu = self._f64_vector(who, "u", u, self.plan.n_dofs, "dofs")
        rec = self._gl_buffers()[4]
        ee = None if ea is None else self._f64_vector(who, "ea", ea, ne, "elements")
        zz = None if e0 is None else self._f64_vector(who, "e0", e0, ne, "elements")
        yy, kk = (self._f64_vector(who, name, torch.as_tensor(v), ne, "elements") for name, v in (("ey", ey), ("kappa", kappa)))
        p = self._gl_plastic_buffers()
        pl = _capi.PfGlPlastic()
        filler = p["counts"]                                 # (an empty mesh: any non-null pointer, nothing reads it)
        pl.ey, pl.kappa = (yy.data_ptr(), kk.data_ptr()) if ne else (filler.data_ptr(), filler.data_ptr())
        pl.ep_n, pl.al_n = p["committed"][0].data_ptr(), p["committed"][1].data_ptr()
        pl.ep, pl.al = p["trial"][0].data_ptr(), p["trial"][1].data_ptr()
        pl.yielding, pl.counts = p["yielding"].data_ptr(), p["counts"].data_ptr()
        _capi.check(self.lib.pf_gl_state_plastic(self._ref(), C.byref(rec), None if ee is None else ee.data_ptr(),
                                                 None if zz is None else zz.data_ptr(), C.byref(pl), uu.data_ptr(),
                                                 self._stream()), "pf_gl_state_plastic")
        p["formed"] = True
        return self._gl[3][:ne]

    def _gl_plastic_buffers(self):
        if self._gl_plastic is None:
            ne = max(self.plan.n_elems, 1)
            f64 = dict(dtype=torch.float64, device=self.device)
            self._gl_plastic = dict(committed=[torch.zeros(ne, **f64), torch.zeros(ne, **f64)],
                                    trial=[torch.zeros(ne, **f64), torch.zeros(ne, **f64)],
                                    yielding=torch.zeros(ne, dtype=torch.uint8, device=self.device),
                                    counts=torch.zeros(_capi.PF_GL_CABLE_COUNT, **f64), formed=False)
        return self._gl_plastic

    def _gl_plastic_ready(self, who):
        if self._gl_plastic is None or not self._gl_plastic["formed"]:
            raise RuntimeError(f"{who}: no plastic state formed since the last commit or reset; call "
                               "gl_state_plastic(u, ey, kappa) first")
        return self._gl_plastic

    @_on_engine_stream
    def gl_plastic_reset(self, ep=None, alpha=None):
        """Set the committed plastic state ((ep, alpha) [n_elems] each, zeros by default) and clear the flags: the start of
        a solve or of a load program."""
        p = self._gl_plastic_buffers()
        ne = self.plan.n_elems
        for buf, name, v in zip(p["committed"], ("ep", "alpha"), (ep, alpha)):
            if v is None:
                buf.zero_()
            else:
                buf[:ne].copy_(self._f64_vector("gl_plastic_reset", name, torch.as_tensor(v), ne, "elements"))
        p["yielding"].zero_()
        p["formed"] = False

    def gl_plastic_commit(self):
        """The trial (ep, alpha) of the last gl_state_plastic becomes the committed state: the two buffer pairs change
        places, nothing is launched.  Raises where no plastic state was formed since the last commit or reset."""
        p = self._gl_plastic_ready("gl_plastic_commit")
        p["committed"], p["trial"] = p["trial"], p["committed"]
        p["formed"] = False

    @_on_engine_stream
    def gl_plastic_counts(self):
        """(number of plastic elements, number of elements whose flag changed against the call before) of the last
        gl_state_plastic: one read of 16 bytes."""
        n = self._gl_plastic_ready("gl_plastic_counts")["counts"][:2].cpu()
        return int(n[0]), int(n[1])

    @_on_engine_stream
    def gl_plastic_state(self):
        """(ep, alpha, yielding) of the last gl_state_plastic on the host: float64 [n_elems] twice and bool [n_elems]."""
        p = self._gl_plastic_ready("gl_plastic_state")
        ne = self.plan.n_elems
        return (p["trial"][0][:ne].cpu().numpy(), p["trial"][1][:ne].cpu().numpy(),
                p["yielding"][:ne].cpu().numpy().astype(bool))

    @_on_engine_stream
    def gl_sensitivity(self, u: torch.Tensor, a: torch.Tensor, out: Optional[torch.Tensor] = None,
                       e0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dJ/d(E*A) of every element [n_elems] from the displacements u and the adjoint a of a misfit J (K_t(u) a =
        dJ/du on the free dofs): -(e / l0) d.(a_j - a_i) (pf_gl_sens).  out: a float64 device vector [n_elems] the result
        is ADDED to (load levels sum in call order); None: a new vector.  e0: the initial strain of gl_state
        [n_elems]: e - e0 takes e's place (pf_gl_sens_e0)."""
        uu = self._f64_vector("gl_sensitivity", "u", u, self.plan.n_dofs, "dofs")
        aa = self._f64_vector("gl_sensitivity", "a", a, self.plan.n_dofs, "dofs")
        ne = self.plan.n_elems
        zz = None if e0 is None else self._f64_vector("gl_sensitivity", "e0", e0, ne, "elements")
        out, accumulate = self._accumulator("gl_sensitivity", out, ne, torch.empty)
        if ne:
            rec = self._gl_buffers()[4]
            if zz is None:
                _capi.check(self.lib.pf_gl_sens(self._ref(), C.byref(rec), uu.data_ptr(), aa.data_ptr(), int(accumulate),
                                                out.data_ptr(), self._stream()), "pf_gl_sens")
            else:
                _capi.check(self.lib.pf_gl_sens_e0(self._ref(), C.byref(rec), zz.data_ptr(), uu.data_ptr(), aa.data_ptr(),
                                                   int(accumulate), out.data_ptr(), self._stream()), "pf_gl_sens_e0")
        return out

    @_on_engine_stream
    def group_sum(self, values: torch.Tensor, weights: Optional[torch.Tensor], groups) -> torch.Tensor:
        """out[g] = sum of values[e] * weights[e] (weights None: of values[e]) over the elements e with groups[e] == g, in
        ascending element id and a fixed order (pf_group_sum_f64: the same bits on every run).  groups: [n_elems]
        non-negative ints; the result has max(groups) + 1 entries.  The CSR of the last group map is cached."""
        ne = self.plan.n_elems
        gm, key, n_groups = self._group_ids("group_sum", groups)
        if self._group_csr is None or self._group_csr[0] != key:
            ptr = np.zeros(n_groups + 1, dtype=np.int32)
            np.cumsum(np.bincount(gm, minlength=n_groups), out=ptr[1:])
            order = np.argsort(gm, kind="stable").astype(np.int32)          # ascending element id inside a group
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self._group_csr = (key, n_groups, dev(ptr), dev(order if ne else np.zeros(1, dtype=np.int32)))
        _, n_groups, ptr, order = self._group_csr
        vv = self._f64_vector("group_sum", "values", values, ne, "elements")
        ww = None if weights is None else self._f64_vector("group_sum", "weights", weights, ne, "elements")
        out = torch.empty(n_groups, dtype=torch.float64, device=self.device)
        if n_groups:
            _capi.check(self.lib.pf_group_sum_f64(ne, vv.data_ptr(), None if ww is None else ww.data_ptr(), ptr.data_ptr(),
                                                  order.data_ptr(), n_groups, out.data_ptr(), self._stream()),
                        "pf_group_sum_f64")
        return out

    @_on_engine_stream
    def gl_group_rhs(self, groups, g0: int = 0, m: Optional[int] = None) -> torch.Tensor:
        """Right-hand sides of the sensitivity solves K_t s_g = -d f_int / d q_g of the last gl_state for the groups g0,
        ..., g0 + m - 1 (m None: every group from g0 on): row k is minus the internal force of the elements of group
        g0 + k alone, zero on fixed dofs (pf_gl_group_rhs).  groups: [n_elems] non-negative ints.  The device copy of the
        last group map is cached.  Returns [m, n_dofs]."""
        n_groups, ids = self._device_group_map("gl_group_rhs", groups)
        g0, m = self._group_range("gl_group_rhs", n_groups, g0, m)
        rec = self._gl_ready("gl_group_rhs")[4]
        out = torch.empty((m, self.plan.n_dofs), dtype=torch.float64, device=self.device)
        _capi.check(self.lib.pf_gl_group_rhs(self._ref(), C.byref(rec), ids.data_ptr(), g0, m, out.data_ptr(),
                                             self._stream()), "pf_gl_group_rhs")
        return out

    @_on_engine_stream
    def gl_prestress_rhs(self, u: torch.Tensor, ea: Optional[torch.Tensor], groups, g0: int = 0,
                         m: Optional[int] = None) -> torch.Tensor:
        """Right-hand sides of the sensitivity solves K_t s_h = -d f_int / d t_h at the displacements u for the prestress
        groups g0, ..., g0 + m - 1 (m None: every group from g0 on), t_h a strain added to the initial strain of the
        elements of group h: row k is, per dof, the sum of +-(ea_e / l0) d_e over the node's elements of group g0 + k, zero
        on fixed dofs (pf_gl_prestress_rhs).  ea: E*A of every element [n_elems] in float64; None: the model's scalar
        E*A as the device forms it (each factor rounded to float32 first), filled in on the host side.  groups: [n_elems]
        ints >= -1; -1: the element belongs to no group.  The device copy of the last group map is cached.  It reads d0
        and u only: no gl_state is needed first.  Returns [m, n_dofs]."""
        ne = self.plan.n_elems
        uu = self._f64_vector("gl_prestress_rhs", "u", u, self.plan.n_dofs, "dofs")
        n_groups, ids = self._device_group_map("gl_prestress_rhs", groups, lowest=-1)
        g0, m = self._group_range("gl_prestress_rhs", n_groups, g0, m)
        if ea is None:
            mat = self.model.material
            ee = torch.full((max(ne, 1),), float(np.float32(mat.young.value())) * float(np.float32(mat.area.value())),
                            dtype=torch.float64, device=self.device)
        else:
            ee = self._f64_vector("gl_prestress_rhs", "ea", ea, ne, "elements")
            if not ne:
                ee = torch.zeros(1, dtype=torch.float64, device=self.device)
        rec = self._gl_buffers()[4]
        out = torch.empty((m, self.plan.n_dofs), dtype=torch.float64, device=self.device)
        _capi.check(self.lib.pf_gl_prestress_rhs(self._ref(), C.byref(rec), ee.data_ptr(), uu.data_ptr(), ids.data_ptr(), g0, m,
                                                 out.data_ptr(), self._stream()), "pf_gl_prestress_rhs")
        return out

    @_on_engine_stream
    def gl_strain_rhs(self, u: torch.Tensor, coef: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """B^T coef [n_dofs] with B = d e / d u the derivative of the Green-Lagrange strains at the displacements u: per dof
        the sum of +-(coef[e] / l0^2) d_e over the node's elements, zero on fixed dofs (pf_gl_strain_rhs; the adjoint
        right-hand side of a strain misfit).  coef: [n_elems] float64, 0.0 where nothing is measured.  out: a float64 device
        vector [n_dofs] the result is ADDED to (fixed dofs stay as they are); None: a new vector.  It reads d0 and u only:
        no gl_state is needed first."""
        uu = self._f64_vector("gl_strain_rhs", "u", u, self.plan.n_dofs, "dofs")
        cc = self._f64_vector("gl_strain_rhs", "coef", coef, self.plan.n_elems, "elements")
        n = self.plan.n_dofs
        out, accumulate = self._accumulator("gl_strain_rhs", out, n, torch.zeros)
        if self.plan.n_elems:
            rec = self._gl_buffers()[4]
            _capi.check(self.lib.pf_gl_strain_rhs(self._ref(), C.byref(rec), uu.data_ptr(), cc.data_ptr(), int(accumulate),
                                                  out.data_ptr(), self._stream()), "pf_gl_strain_rhs")
        return out

    @_on_engine_stream
    def gl_strain_jvp(self, u: torch.Tensor, elements, V: torch.Tensor) -> torch.Tensor:
        """B V^T at the measured elements: [m, n_meas] with entry (k, i) = (d_e / l0^2).(V[k, j] - V[k, i]) for
        e = elements[i] (pf_gl_strain_jvp; the strain rows of the Gauss-Newton Jacobian from the sensitivity solutions).
        elements: [n_meas] ints in 0..n_elems-1; V: [m, n_dofs] float64.  It reads d0 and u only."""
        uu = self._f64_vector("gl_strain_jvp", "u", u, self.plan.n_dofs, "dofs")
        ids = np.ascontiguousarray(np.asarray(elements.cpu() if isinstance(elements, torch.Tensor) else elements).reshape(-1))
        if ids.size and (ids.dtype.kind not in "iu" or ids.min() < 0 or ids.max() >= self.plan.n_elems):
            raise ValueError(f"gl_strain_jvp: elements must be integer ids in 0..{self.plan.n_elems - 1}")
        if V.dim() != 2 or V.shape[1] != self.plan.n_dofs or not 1 <= V.shape[0] <= 65535:
            raise ValueError(f"gl_strain_jvp: V must be [m, {self.plan.n_dofs}] with 1 <= m <= 65535, got {tuple(V.shape)}")
        vv = V.to(device=self.device, dtype=torch.float64).contiguous()
        m, n_meas = int(vv.shape[0]), int(ids.size)
        out = torch.empty((m, n_meas), dtype=torch.float64, device=self.device)
        if n_meas:
            ids_t = torch.from_numpy(ids.astype(np.int32)).to(self.device)
            rec = self._gl_buffers()[4]
            _capi.check(self.lib.pf_gl_strain_jvp(self._ref(), C.byref(rec), uu.data_ptr(), ids_t.data_ptr(), n_meas,
                                                  vv.data_ptr(), m, out.data_ptr(), self._stream()), "pf_gl_strain_jvp")
        return out

    def _gl_ready(self, who):
        if self._gl is None:
            raise RuntimeError(f"{who}: no Green-Lagrange state yet; call gl_state(u) first")
        return self._gl

    @_on_engine_stream
    def gl_fint(self) -> torch.Tensor:
        """f_int(u) [n_dofs, every row] of the last gl_state (pf_gl_fint)."""
        rec = self._gl_ready("gl_fint")[4]
        out = torch.empty(self.plan.n_dofs, dtype=torch.float64, device=self.device)
        _capi.check(self.lib.pf_gl_fint(self._ref(), C.byref(rec), out.data_ptr(), self._stream()), "pf_gl_fint")
        return out

    # ---- explicit dynamics of the Green-Lagrange element (pf_gl_dyn_*) ---------------------------------
    def _drop_dyn_graphs(self):
        d = getattr(self, "_dyn", None)         # (__del__ may run on a half-built engine)
        if d:
            for g in d["graphs"].values():
                self.lib.pf_graph_destroy(g)
            d["graphs"] = {}

    @_on_engine_stream
    def dyn_begin(self, u0, v0, minv, dt, alpha, lam0, lam1, t_ramp, ea=None, e0=None, start=True, cable=None,
                  load_samples=None, support=None):
        """Begin a central-difference run at step 0 (pf_dyn).  u0, v0, minv: float64 [n_dofs] (minv = 1 / lumped mass of
        the dof's node; the loads are the model's, at load factor 1); ea, e0: as gl_state.  start: v0 is the velocity at
        t = 0 and the half kick (pf_gl_dyn_start) turns it into v_{1/2} and u_1, the run then stands at step 1; False: v0 is
        taken as v_{-1/2} and the run stands at step 0.  The buffers live on the engine; the graphs of dyn_steps are kept
        for as long as the scalars and the presence of ea / e0 / cable / histories, which they bake in, stay the same.
        cable: bool or uint8 [n_elems], True = the element is tension-only (no force and no strain energy where e - e0 < 0);
        the run then goes through the pf_gl_dyn_*_cable entry points.  None: a run of bars through pf_gl_dyn_*.
        load_samples: float64 [n], the load factor of step k in place of the ramp (lam0, lam1 and t_ramp are then not read);
        support: a pair (amp [n_dofs], samples [n]): a fixed dof with amp != 0 is held at amp * samples[k] at step k.  A step
        beyond a table reads its last sample; with both given the two tables have one length.  The engine keeps device
        copies, and the run goes through the pf_gl_dyn_*_hist entry points (with the cable flags, if any).  u0 on the moved
        dofs is the caller's.  With neither, every call is the call it was without these arguments."""
        nd, ne = self.plan.n_dofs, self.plan.n_elems
        flags = None if cable is None else self._cable_flags(cable, ne)
        hist = self._dyn_histories(load_samples, support, nd)
        vec = {name: self._f64_vector("dyn_begin", name, t, nd, "dofs") for name, t in (("u0", u0), ("v0", v0), ("minv", minv))}
        opt = {name: None if t is None else self._f64_vector("dyn_begin", name, t, ne, "elements")
               for name, t in (("ea", ea), ("e0", e0))}
        scalars = tuple(float(x) for x in (dt, alpha, lam0, lam1, t_ramp))
        key = scalars + (ea is None, e0 is None, cable is None, load_samples is not None, support is not None,
                         0 if hist is None else hist["lam" if "lam" in hist else "sup"].numel())
        d = self._dyn
        if d is None:
            f64 = dict(dtype=torch.float64, device=self.device)
            d = self._dyn = dict(graphs={}, key=None, rec=_capi.PfDyn(), n=0,
                                 f_ext=torch.from_numpy(np.ascontiguousarray(
                                     np.asarray(self.model.loads, dtype=np.float64).reshape(-1))).to(self.device),
                                 out=torch.zeros(_capi.PF_DYN_CABLE_ENERGY_COUNT, **f64),
                                 cable=torch.zeros(max(ne, 1), dtype=torch.uint8, device=self.device), with_cable=False,
                                 clock=torch.zeros(1, dtype=torch.int64, device=self.device),
                                 **{name: torch.zeros(max(nd, 1), **f64) for name in ("u0", "u1", "v", "minv")},
                                 **{name: torch.zeros(max(ne, 1), **f64) for name in ("ea", "e0")})
        if d["key"] != key:
            self._drop_dyn_graphs()
            d["key"] = key
        for name, src in (("u0", "u0"), ("v", "v0"), ("minv", "minv")):
            d[name][:nd].copy_(vec[src])
        d["u1"].zero_()
        d["clock"].zero_()
        d["slack_at"] = None
        for name, t in opt.items():
            if t is not None:
                d[name][:ne].copy_(t)
        rec = d["rec"]
        rec.minv, rec.f_ext, rec.u0, rec.u1, rec.v = (d[k].data_ptr() for k in ("minv", "f_ext", "u0", "u1", "v"))
        rec.ea = None if ea is None else d["ea"].data_ptr()
        rec.e0 = None if e0 is None else d["e0"].data_ptr()
        rec.clock = d["clock"].data_ptr()
        rec.dt, rec.alpha, rec.lam0, rec.lam1, rec.t_ramp = scalars
        d["with_cable"] = flags is not None
        if flags is not None:
            d["cable"][:ne].copy_(flags)
        # the histories: device copies that keep their place for as long as their presence and length, which are in the key
        if hist is None:
            d["hist"] = None
        else:
            old = d.get("hist") or {}
            h = d["hist"] = dict(rec=_capi.PfDynHist())
            for name, t in hist.items():
                keep = old.get(name)
                h[name] = keep.copy_(t) if keep is not None and keep.numel() == t.numel() else t.clone()
                setattr(h["rec"], name, h[name].data_ptr())
            h["rec"].n_samples = h["lam" if "lam" in h else "sup"].numel()
        d["n"] = 0
        if start:
            self._dyn_call(d, "pf_gl_dyn_start", self._stream())
            d["n"] = 1

    def _cable_flags(self, cable, ne, who="dyn_begin"):
        flags = cable if isinstance(cable, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cable))
        if flags.dtype not in (torch.bool, torch.uint8) or flags.dim() != 1 or flags.numel() != ne:
            raise ValueError(f"{who}: cable must be bool or uint8 [{ne}] (one flag for each element), got "
                             f"{flags.dtype} {tuple(flags.shape)}")
        return flags.to(device=self.device, dtype=torch.uint8)

    def _dyn_histories(self, load_samples, support, nd):
        """dyn_begin's load_samples and support, checked, as device vectors by pf_dyn_hist's names, or None."""
        if load_samples is None and support is None:
            return None

        def samples(name, t):
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
            if t.dtype != torch.float64 or t.dim() != 1 or t.numel() < 1:
                raise ValueError(f"dyn_begin: {name} must be float64 [n] with n >= 1, got {t.dtype} {tuple(t.shape)}")
            return t.to(self.device).contiguous()

        keep = {}
        if load_samples is not None:
            keep["lam"] = samples("load_samples", load_samples)
        if support is not None:
            try:
                amp, sup = support
            except (TypeError, ValueError):
                raise ValueError("dyn_begin: support must be a pair (amp [n_dofs], samples [n])") from None
            keep["sup_amp"] = self._f64_vector("dyn_begin", "support amp", amp if isinstance(amp, torch.Tensor)
                                               else torch.from_numpy(np.ascontiguousarray(amp)), nd, "dofs")
            keep["sup"] = samples("support samples", sup)
        if "lam" in keep and "sup" in keep and keep["lam"].numel() != keep["sup"].numel():
            raise ValueError(f"dyn_begin: load_samples has {keep['lam'].numel()} samples and support {keep['sup'].numel()}: "
                             "both are sampled at the same steps")
        return keep

    def _dyn_call(self, d, name, *args):
        """lib.<name>(problem, element record, pf_dyn, *args), or its _cable namesake with the run's flags behind pf_dyn; with
        histories its _hist namesake, where the histories' record and the flags (or null) ride behind pf_dyn.  The energies
        know no histories."""
        head = (self._ref(), C.byref(self._gl_buffers()[4]), C.byref(d["rec"]))
        if d.get("hist") is not None and name != "pf_gl_dyn_energy":
            name = name + "_hist"
            head = head + (C.byref(d["hist"]["rec"]), d["cable"].data_ptr() if d["with_cable"] else None)
        elif d["with_cable"]:
            name, head = name + "_cable", head + (d["cable"].data_ptr(),)
        _capi.check(getattr(self.lib, name)(*head, *args), name)

    def _dyn_ready(self, who):
        d = self._dyn
        if d is None:
            raise RuntimeError(f"{who}: no dynamic run yet; call dyn_begin first")
        return d

    @_on_engine_stream
    def dyn_steps(self, n: int, use_graph: bool = True):
        """n time steps, one launch each (pf_gl_dyn_steps), or one replay of their hipGraph (pf_gl_dyn_graph_create, cached
        for each n until dyn_begin changes what it bakes in).  Enqueues only."""
        d, n = self._dyn_ready("dyn_steps"), int(n)
        if n < 1:
            raise ValueError(f"dyn_steps: n must be at least 1, got {n}")
        if use_graph and os.environ.get("PINNFEM_GRAPH", "1") != "0":
            if n not in d["graphs"]:
                g = C.c_void_p()
                self._dyn_call(d, "pf_gl_dyn_graph_create", n, self._stream(), C.byref(g))
                d["graphs"][n] = g
            _capi.check(self.lib.pf_graph_launch(d["graphs"][n], self._stream()), "pf_graph_launch")
        else:
            self._dyn_call(d, "pf_gl_dyn_steps", n, self._stream())
        d["n"] += n

    @_on_engine_stream
    def dyn_state(self):
        """(u_n, v_{n-1/2}, n) of the run: copies, float64 [n_dofs] on the device."""
        d, nd = self._dyn_ready("dyn_state"), self.plan.n_dofs
        return d["u1" if d["n"] & 1 else "u0"][:nd].clone(), d["v"][:nd].clone(), d["n"]

    @_on_engine_stream
    def dyn_energy(self):
        """(kinetic energy sum m v^2 / 2, strain energy sum E*A l0 (e - e0)^2 / 2, f_ext.u at load factor 1, max |v|) at
        the run's state (pf_gl_dyn_energy), on the host: it synchronises.  With cable flags the strain energy leaves the
        slack elements out (pf_gl_dyn_energy_cable), and dyn_slack_count() reads their number."""
        d = self._dyn_ready("dyn_energy")
        self._dyn_call(d, "pf_gl_dyn_energy", d["out"].data_ptr(), self._stream())
        d["slack_at"] = d["n"]
        return tuple(float(x) for x in d["out"][:4].cpu())

    @_on_engine_stream
    def dyn_slack_count(self) -> int:
        """The number of slack elements at the state of the last dyn_energy(), read from its buffer without another
        launch; 0 in a run without cable flags."""
        d = self._dyn_ready("dyn_slack_count")
        if d.get("slack_at") != d["n"]:
            raise RuntimeError("dyn_slack_count: call dyn_energy() at this state first")
        return int(d["out"][4].cpu()) if d["with_cable"] else 0

    @_on_engine_stream
    def kt_v_f64(self, v: torch.Tensor, zero_fixed: bool = False, extra_fixed=None) -> torch.Tensor:
        """K_t(u) v in float64 with the tangent blocks of the last gl_state (pf_kt_v_f64).  extra_fixed: dofs that
        zero_fixed treats as fixed on top of the model's (_fixed_view)."""
        kt = self._gl_ready("kt_v_f64")[1]
        vv = v.to(device=self.device, dtype=torch.float64).contiguous()
        out = torch.empty(self.plan.n_dofs, dtype=torch.float64, device=self.device)
        _capi.check(self.lib.pf_kt_v_f64(self._fixed_view(extra_fixed)[0], kt.data_ptr(), vv.data_ptr(), out.data_ptr(), int(zero_fixed),
                                         self._stream()), "pf_kt_v_f64")
        return out

    @_on_engine_stream
    def kt_diag(self) -> torch.Tensor:
        """diag(K_t) [n_dofs] of the last gl_state, 0.0 on fixed dofs (pf_kt_diag_f64): what the Jacobi preconditioner of
        pcg_solve(tangent=True) inverts."""
        kt = self._gl_ready("kt_diag")[1]
        out = torch.empty(self.plan.n_dofs, dtype=torch.float64, device=self.device)
        _capi.check(self.lib.pf_kt_diag_f64(self._ref(), kt.data_ptr(), out.data_ptr(), self._stream()), "pf_kt_diag_f64")
        return out

    def _pcg_setup(self, who, tangent, preconditioner, n_aggregates, aggregates, u, extra_fixed):
        """What pcg_solve and pcg_solve_batch share before the solve: the preconditioner's checks and coarse space (one
        refresh per call), the pf_problem reference (the view of extra_fixed) and the tangent blocks.
        Returns (ref, coarse | None, kt pointer | None)."""
        coarse = None
        name = _coarse.check_preconditioner(preconditioner)
        if extra_fixed is not None and len(extra_fixed) and not tangent:
            raise ValueError(f"{who}: extra_fixed belongs to the tangent solve (tangent=True)")
        if name == "two-level":
            if tangent:
                raise ValueError("the two-level preconditioner of the linear operator has no tangent form: with "
                                 "tangent=True use preconditioner='two-level-updated' (or 'jacobi')")
            coarse = self.coarse_space(n_aggregates, aggregates)        # None: the coarse matrix could not be factored
        elif name == "two-level-updated":
            if not tangent:
                raise ValueError("preconditioner='two-level-updated' belongs to the tangent solve (tangent=True): the "
                                 "linear operator has nothing to update; use 'two-level'")
            if u is None:
                raise ValueError("preconditioner='two-level-updated' needs u, the displacements of the last gl_state")
            coarse = self.updated_coarse_space(u, n_aggregates, aggregates, extra_fixed)    # None: Jacobi on the tangent
        kt = self._gl_ready(f"{who}(tangent=True)")[1].data_ptr() if tangent else None
        return self._fixed_view(extra_fixed)[0], coarse, kt

    def _pcg_run(self, fam, head, state_head, m, bb, two_level, rtol, max_iter, poll):
        """begin, then `poll` iterations at a time (one graph replay, or eager launches for a shorter tail) until every
        one of the m right-hand sides has stopped or max_iter is reached.  Returns (x [m * n_dofs], state [m][4])."""
        lib, s, n = self.lib, self._stream(), self.plan.n_dofs
        x = torch.zeros(m * n, dtype=torch.float64, device=self.device)
        ws_count = lib.pf_pcg2_workspace_count if two_level else lib.pf_pcg_workspace_count
        ws = torch.zeros(m * int(ws_count(self._ref())), dtype=torch.float64, device=self.device)
        _capi.check(getattr(lib, fam + "_begin")(*head, bb.data_ptr(), x.data_ptr(), ws.data_ptr(), float(rtol), s),
                    fam + "_begin")
        if max_iter is None:
            max_iter = 40 * n + 2000            # slender trusses are beam-like: CG needs far more than n steps
        st = (C.c_double * (4 * m))()
        done_it = 0
        graph = C.c_void_p()
        use_graph = os.environ.get("PINNFEM_GRAPH", "1") != "0" and max_iter >= poll
        if use_graph:
            _capi.check(getattr(lib, fam + "_graph_create")(*head, x.data_ptr(), ws.data_ptr(), int(poll), s,
                                                            C.byref(graph)), fam + "_graph_create")
        try:
            while True:
                k = min(poll, max_iter - done_it)
                if use_graph and k == poll:
                    _capi.check(lib.pf_graph_launch(graph, s), "pf_graph_launch")
                    _capi.check(getattr(lib, fam + "_state")(*state_head, ws.data_ptr(), st, s),
                                fam + "_state")
                else:
                    _capi.check(getattr(lib, fam + "_iterations")(*head, x.data_ptr(), ws.data_ptr(), int(max(k, 0)), st, s),
                                fam + "_iterations")
                done_it += max(k, 0)
                if all(st[4 * j + 1] != 0.0 for j in range(m)) or done_it >= max_iter:
                    break
        finally:
            if graph:
                lib.pf_graph_destroy(graph)
        return x, [tuple(st[4 * j: 4 * j + 4]) for j in range(m)]

    @staticmethod
    def _pcg_report(st, rtol):
        converged = st[2] <= (rtol * rtol) * st[3] * 4.0 or st[3] == 0.0     # |r| <= 2 rtol |b|
        return int(st[0]), bool(converged), float(st[2]), float(st[3])

    @_on_engine_stream
    def pcg_solve(self, b: torch.Tensor, rtol: float = 1e-13, max_iter: Optional[int] = None, poll: int = 64,
                  preconditioner: str = "jacobi", n_aggregates: Optional[int] = None, aggregates=None,
                  tangent: bool = False, u=None, extra_fixed=None):
        """K_ff x = b by conjugate gradients, float64, on the device.  preconditioner: "jacobi" (diag(K_ff), the
        default) or "two-level" (Jacobi plus a coarse space of per-aggregate rigid-body modes, coarse.py;
        n_aggregates strips along the longest axis, or the caller's own node -> aggregate map).  tangent: K is the
        tangent K_t(u) of the last gl_state, which must be positive definite: pf_pcgt_* with "jacobi", pf_pcg2t_* with
        "two-level-updated", whose coarse space is rebuilt on X + u at every call (updated_coarse_space; u: the
        displacements the last gl_state was given).  extra_fixed (tangent only): dofs constrained on top of the model's
        for this solve, so K_ff loses their rows and columns as well (_fixed_view).
        Returns (x with zeros on fixed dofs, iterations, converged, |r|^2, |b|^2)."""
        ref, coarse, kt = self._pcg_setup("pcg_solve", tangent, preconditioner, n_aggregates, aggregates, u, extra_fixed)
        if tangent:
            fam = "pf_pcgt" if coarse is None else "pf_pcg2t"
            head = (ref, kt) if coarse is None else (ref, C.byref(coarse.record), kt)
            state_head = (ref, kt)
        else:
            fam = "pf_pcg" if coarse is None else "pf_pcg2"
            head = (ref,) if coarse is None else (ref, C.byref(coarse.record))
            state_head = (ref,)
        bb = b.to(device=self.device, dtype=torch.float64).contiguous()
        x, (st,) = self._pcg_run(fam, head, state_head, 1, bb, coarse is not None, rtol, max_iter, poll)
        self.pcg_iterations += int(st[0])
        return (x,) + self._pcg_report(st, rtol)

    @_on_engine_stream
    def pcg_solve_batch(self, B: torch.Tensor, tangent: bool = True, preconditioner: str = "jacobi",
                        n_aggregates: Optional[int] = None, aggregates=None, u=None, extra_fixed=None,
                        rtol: float = 1e-13, max_iter: Optional[int] = None, poll: int = 64):
        """K_t x_k = B[k] for the m rows of B [m, n_dofs] through the launches of ONE solve (pf_pcgtm_* with "jacobi",
        pf_pcg2tm_* with "two-level-updated"): every launch carries the m right-hand sides, each with its own workspace,
        stop test and iteration count, and each computes what its own pcg_solve would, bit for bit.  The coarse space is
        refreshed once per call and shared.  Polls until every right-hand side has stopped.  The tangent operator only.
        Returns (x [m, n_dofs], [(iterations, converged, |r|^2, |b|^2) per right-hand side])."""
        if not tangent:
            raise ValueError("pcg_solve_batch: only the tangent operator has a batched solve (tangent=True)")
        if B.dim() != 2 or B.shape[1] != self.plan.n_dofs or not 1 <= B.shape[0] <= _capi.PF_PCG_MAX_RHS:
            raise ValueError(f"pcg_solve_batch: B must be [m, {self.plan.n_dofs}] with 1 <= m <= {_capi.PF_PCG_MAX_RHS}, "
                             f"got {tuple(B.shape)}")
        m = int(B.shape[0])
        ref, coarse, kt = self._pcg_setup("pcg_solve_batch", True, preconditioner, n_aggregates, aggregates, u,
                                          extra_fixed)
        fam = "pf_pcgtm" if coarse is None else "pf_pcg2tm"
        head = (ref, kt, m) if coarse is None else (ref, C.byref(coarse.record), kt, m)
        bb = B.to(device=self.device, dtype=torch.float64).contiguous()
        x, states = self._pcg_run(fam, head, (ref, kt, m), m, bb, coarse is not None, rtol, max_iter, poll)
        self.pcg_iterations += sum(int(st[0]) for st in states)
        self.pcg_batch_solves += 1
        return x.reshape(m, -1), [self._pcg_report(st, rtol) for st in states]

    @_on_engine_stream
    def pcg_solve_many(self, B: torch.Tensor, preconditioner: str = "jacobi", n_aggregates: Optional[int] = None,
                       aggregates=None, u=None, rtol: float = 1e-13, max_iter: Optional[int] = None, poll: int = 64):
        """K_t x_k = B[k] for the G rows of B [G, n_dofs] on the tangent of the last gl_state, behind ONE setup: the
        coarse space of "two-level-updated" is refreshed once and serves every row.  The rows go through the batched
        family (pf_pcgtm_* with "jacobi", pf_pcg2tm_* with "two-level-updated") in row order, PF_PCG_MAX_RHS at a time;
        a last odd row goes alone through the same family with m = 1.  Each row computes what its own pcg_solve would,
        bit for bit.  The tangent operator only.
        Returns (x [G, n_dofs], [(iterations, converged, |r|^2, |b|^2) per row])."""
        if B.dim() != 2 or B.shape[1] != self.plan.n_dofs or B.shape[0] < 1:
            raise ValueError(f"pcg_solve_many: B must be [G, {self.plan.n_dofs}] with G >= 1, got {tuple(B.shape)}")
        ref, coarse, kt = self._pcg_setup("pcg_solve_many", True, preconditioner, n_aggregates, aggregates, u, None)
        fam = "pf_pcgtm" if coarse is None else "pf_pcg2tm"
        bb = B.to(device=self.device, dtype=torch.float64).contiguous()
        G = int(bb.shape[0])
        x = torch.empty_like(bb)
        reports = []
        for r0 in range(0, G, _capi.PF_PCG_MAX_RHS):
            m = min(_capi.PF_PCG_MAX_RHS, G - r0)
            head = (ref, kt, m) if coarse is None else (ref, C.byref(coarse.record), kt, m)
            xm, states = self._pcg_run(fam, head, (ref, kt, m), m, bb[r0:r0 + m], coarse is not None, rtol, max_iter, poll)
            x[r0:r0 + m] = xm.reshape(m, -1)
            self.pcg_iterations += sum(int(st[0]) for st in states)
            reports += [self._pcg_report(st, rtol) for st in states]
        return x, reports

    def _stiffness_signature(self):
        """What the coarse matrix Z^T K Z was built from: the E and A that elem_s64 reads."""
        sig = []
        ne = max(self.plan.n_elems, 0)
        for spec, buf in zip(self.specs, (self.prop_e, self.prop_a)):
            sig.append(buf[:ne].cpu().numpy().tobytes() if spec.enabled else float(np.float32(spec.scale)))
        return tuple(sig)

    @_on_engine_stream
    def coarse_space(self, n_aggregates: Optional[int] = None, aggregates=None):
        """The two-level preconditioner's coarse space on the device (a DeviceCoarse), cached per engine and rebuilt
        when the aggregation asked for or the element stiffness changes.  The device forms A_c = Z^T K Z
        (pf_coarse_setup); the host factors it (Cholesky, float64) and uploads the explicit inverse.  Returns None,
        with a RuntimeWarning, when A_c is not positive definite: the solve then runs with Jacobi alone."""
        agg_key = None if aggregates is None else np.asarray(aggregates).astype(np.int64).tobytes()
        key = (None if n_aggregates is None else int(n_aggregates), agg_key, self._stiffness_signature())
        if self._coarse_cache is not None and self._coarse_cache[0] == key:
            return self._coarse_cache[1]
        hp = self.plan
        if len(self.model.nodes) != hp.n_nodes:
            raise NotImplementedError("the two-level preconditioner needs the engine's mesh to be the model's "
                                      "(no sharded form)")
        cs = _coarse.build_coarse_space(np.asarray(self.model.nodes, dtype=np.float64), hp.dim,
                                        (hp.dof_flags & _capi.PF_DOF_FIXED) != 0, n_aggregates, aggregates)
        dc = DeviceCoarse(cs, self.device)
        a_c = torch.zeros(max(cs.n_coarse, 1) ** 2, dtype=torch.float64, device=self.device)
        _capi.check(self.lib.pf_coarse_setup(self._ref(), C.byref(dc.record), a_c.data_ptr(), self._stream()),
                    "pf_coarse_setup")
        dc.a_c = a_c[: cs.n_coarse ** 2].cpu().numpy().reshape(cs.n_coarse, cs.n_coarse)
        try:
            dc.set_inverse(_coarse.coarse_inverse(dc.a_c))
        except np.linalg.LinAlgError as e:
            warnings.warn(f"two-level preconditioner: the coarse matrix Z^T K Z ({cs.n_coarse} x {cs.n_coarse}) could "
                          f"not be factored ({e}); falling back to the Jacobi preconditioner", RuntimeWarning)
            dc = None
        self._coarse_cache = (key, dc)
        return dc

    @_on_engine_stream
    def updated_coarse_space(self, u, n_aggregates: Optional[int] = None, aggregates=None, extra_fixed=None):
        """The coarse space of preconditioner "two-level-updated" for the tangent of the last gl_state: the rigid-body
        modes of every aggregate at the current configuration X + u (X: the model's float64 coordinates), on the
        aggregation of the reference configuration.  One engine-owned DeviceCoarse is refreshed in place at every call:
        host columns, pf_coarse_setup_t with the engine's kt, read-back, host Cholesky, upload.  There is no cache: K_t
        and X + u change with every Newton iteration.  Returns None, with a RuntimeWarning, when Z^T K_t Z is not positive
        definite: the caller then runs Jacobi on the tangent.  extra_fixed: dofs constrained on top of the model's
        (_fixed_view): the columns are zero on them too, so Z^T K_t Z is that of the smaller K_ff."""
        t0 = time.perf_counter()
        hp = self.plan
        if len(self.model.nodes) != hp.n_nodes:
            raise NotImplementedError("the two-level preconditioner needs the engine's mesh to be the model's "
                                      "(no sharded form)")
        kt = self._gl_ready("updated_coarse_space")[1]
        X = np.asarray(self.model.nodes, dtype=np.float64).reshape(hp.n_nodes, hp.dim)
        uu = u.detach().cpu().numpy() if isinstance(u, torch.Tensor) else np.asarray(u)
        uu = np.asarray(uu, dtype=np.float64).reshape(-1)
        if uu.size != hp.n_dofs:
            raise ValueError(f"updated_coarse_space: u has {uu.size} entries, the mesh has {hp.n_dofs} dofs")
        ref, fixed, fixed_key = self._fixed_view(extra_fixed)
        agg_key = None if aggregates is None else np.asarray(aggregates).astype(np.int64).tobytes()
        key = (None if n_aggregates is None else int(n_aggregates), agg_key, fixed_key)
        if self._coarse_updated is None or self._coarse_updated[0] != key:
            # the node -> aggregate map: once, on the reference configuration
            first = _coarse.build_coarse_space(X, hp.dim, fixed, n_aggregates, aggregates)
            cap = _capi.PF_COARSE_MODES * first.n_agg
            dc = DeviceCoarse(first, self.device, max_coarse=cap)
            self._coarse_updated = (key, dc, torch.zeros(cap * cap, dtype=torch.float64, device=self.device))
        _, dc, a_c = self._coarse_updated
        cs = _coarse.update_coarse_space(X + uu.reshape(hp.n_nodes, hp.dim), hp.dim, fixed, dc.space.node_agg)
        dc.refresh(cs)
        t1 = time.perf_counter()
        _capi.check(self.lib.pf_coarse_setup_t(ref, C.byref(dc.record), kt.data_ptr(), a_c.data_ptr(),
                                               self._stream()), "pf_coarse_setup_t")
        dc.a_c = a_c[: cs.n_coarse ** 2].cpu().numpy().reshape(cs.n_coarse, cs.n_coarse)
        t2 = time.perf_counter()
        try:
            inv = _coarse.coarse_inverse(dc.a_c)
        except np.linalg.LinAlgError as e:
            warnings.warn(f"two-level-updated preconditioner: the coarse matrix Z^T K_t Z ({cs.n_coarse} x {cs.n_coarse}) "
                          f"could not be factored ({e}); this step falls back to the Jacobi preconditioner on the tangent",
                          RuntimeWarning)
            inv = None
        t3 = time.perf_counter()
        if inv is not None:
            dc.set_inverse(inv)
        t4 = time.perf_counter()
        parts = self.coarse_refresh_parts
        parts["columns"] += t1 - t0; parts["setup"] += t2 - t1; parts["factor"] += t3 - t2; parts["upload"] += t4 - t3
        self.coarse_refresh_seconds += t4 - t0
        self.coarse_refreshes += 1
        return dc if inv is not None else None

    @_on_engine_stream
    def diag_k(self, lam: Optional[float] = None) -> torch.Tensor:
        self.eval_properties(lam)
        out = torch.empty(self.plan.n_dofs, dtype=torch.float32, device=self.device)
        _capi.check(self.lib.pf_diag_k(self._ref(), out.data_ptr(), self._stream()), "pf_diag_k")
        return out

    @_on_engine_stream
    def sparse_k(self, lam: Optional[float] = None) -> torch.Tensor:
        """k_global as a coalesced torch sparse COO tensor (any mesh size; pf_coo_k)."""
        self.eval_properties(lam)
        n, nd = self.plan.n_dofs, 2 * self.plan.dim
        nnz = max(self.plan.n_elems, 0) * nd * nd
        idx = torch.empty((2, max(nnz, 1)), dtype=torch.int64, device=self.device)
        vals = torch.empty(max(nnz, 1), dtype=torch.float32, device=self.device)
        if nnz:
            _capi.check(self.lib.pf_coo_k(self._ref(), idx[0].data_ptr(), idx[1].data_ptr(), vals.data_ptr(), self._stream()),
                        "pf_coo_k")
        return torch.sparse_coo_tensor(idx[:, :nnz], vals[:nnz], (n, n)).coalesce()

    @_on_engine_stream
    def dense_k(self, lam: Optional[float] = None) -> torch.Tensor:
        self.eval_properties(lam)
        n = self.plan.n_dofs
        out = torch.zeros((n, n), dtype=torch.float32, device=self.device)
        _capi.check(self.lib.pf_dense_k(self._ref(), out.data_ptr(), self._stream()), "pf_dense_k")
        return out
