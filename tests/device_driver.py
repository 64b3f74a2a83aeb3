"""What the float64 device tests share: the one raw-ABI driver of the six exported CG families (CgRun); one truss on the
device (DeviceTruss) with LinearTruss for the linear operator and GlTruss, which owns the Green-Lagrange element buffers
and wraps every raw pf_gl_* entry point that more than one file calls (state, fint, kt_v, kt_diag, sens, group_rhs,
prestress_rhs, strain_rhs, strain_jvp), each on an output filled with 7.0; device_ids, group_maps and check_state beside
it; the Green-Lagrange solver configuration and models of the solve and identification tests (gl_config, truss_model,
case_model) and the CLI run on a copy of a tests/nl_inputs file (run_cli); and the seeded meshes, fields and constants
those files have in common.  The round-off bounds stay in the test files, beside the tests that derive and use them.  A
plain support module like helpers.py: no fixtures, no tests.
"""
import ctypes as C
import json
import math
import os
import shutil

import numpy as np
import torch

import f64_reference as ref
import gl_reference as gl
from helpers import _random_truss

U53, U24 = 2.0 ** -53, 2.0 ** -24
RTOL = 1e-13
ST_COUNT = 16                                   # doubles of CG state per right-hand side (the enum in pf_pcg.hip)
YOUNG, AREA = 2000.0, 0.5                       # the Green-Lagrange tests' material: E*A = 1000, exact in float32
EA = YOUNG * AREA


def same_bits(a, b):
    """Two (x, workspace) pairs as CgRun.read() returns them, bit for bit (compared as bytes: NaN-safe, and -0.0 is
    not 0.0)."""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the CG families through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
class CgRun:
    """One begin of pf_pcg{,2}{,t}{,m}_* with driver-owned x / ws, both filled with 7.0 first: what the library does not
    write stays visible.  S: anything with .eng, .n and .dev().  B: one right-hand side [n], or [m, n] when batched.
    kt: device pointer of the tangent blocks (None: the linear operator).  dc: a DeviceCoarse (None: Jacobi).
    iterate / state / replay return one (iterations, done, |r|^2, |b|^2) when unbatched and a list of m when batched;
    read() likewise (x, ws) or [(x_k, ws_k)]."""

    def __init__(self, S, B, kt=None, dc=None, batched=False, rtol=RTOL):
        from pinn_fem_amd import _capi
        self.S, self.capi, self.dc, self.batched = S, _capi, dc, batched
        eng, n = S.eng, S.n
        B = np.atleast_2d(np.asarray(B, dtype=np.float64))
        self.m = m = len(B)
        assert B.shape[1] == n and (batched or m == 1)
        self.fam = "pf_pcg" + ("2" if dc is not None else "") + ("t" if kt is not None else "") + ("m" if batched else "")
        count = eng.lib.pf_pcg2_workspace_count if dc is not None else eng.lib.pf_pcg_workspace_count
        self.stride = int(count(eng._ref()))
        # the order pcg_layout states in pf_pcg.hip: r | z | p | ap | dinv | partials | state | w | y
        sizes = [("r", n), ("z", n), ("p", n), ("ap", n), ("dinv", n), ("partials", 2 * _capi.PF_NODE_SLOTS), ("state", ST_COUNT)]
        if dc is not None:
            sizes += [("w", _capi.PF_COARSE_MAX), ("y", _capi.PF_COARSE_MAX)]
        self.offsets, at = {}, 0
        for name, size in sizes:
            self.offsets[name] = (at, at + size)
            at += size
        assert at == self.stride, (self.fam, at, self.stride)          # a layout drift fails here, not in a slice
        self.b = S.dev(B.reshape(-1))
        self.x = torch.full((m * n,), 7.0, dtype=torch.float64, device=eng.device)
        self.ws = torch.full((m * self.stride,), 7.0, dtype=torch.float64, device=eng.device)
        coarse = () if dc is None else (C.byref(dc.record),)
        tangent = () if kt is None else (kt,)
        many = (m,) if batched else ()
        self.head = (eng._ref(),) + coarse + tangent + many
        self.state_head = (eng._ref(),) + tangent + many               # the state entry points take no coarse record
        self._call("_begin", self.head, self.b.data_ptr(), self.x.data_ptr(), self.ws.data_ptr(), float(rtol), eng._stream())

    def _call(self, suffix, head, *args):
        eng = self.S.eng
        with eng.on_stream():
            self.capi.check(getattr(eng.lib, self.fam + suffix)(*head, *args), self.fam + suffix)

    def _states(self, st):
        out = [tuple(st[4 * k: 4 * k + 4]) for k in range(self.m)]
        return out if self.batched else out[0]

    def iterate(self, k):
        st = (C.c_double * (4 * self.m))()
        self._call("_iterations", self.head, self.x.data_ptr(), self.ws.data_ptr(), int(k), st, self.S.eng._stream())
        return self._states(st)

    def state(self):
        st = (C.c_double * (4 * self.m))()
        self._call("_state", self.state_head, self.ws.data_ptr(), st, self.S.eng._stream())
        return self._states(st)

    def graph(self, n_iter):
        g = C.c_void_p()
        self._call("_graph_create", self.head, self.x.data_ptr(), self.ws.data_ptr(), int(n_iter), self.S.eng._stream(),
                   C.byref(g))
        return g

    def replay(self, g):
        eng = self.S.eng
        with eng.on_stream():
            self.capi.check(eng.lib.pf_graph_launch(g, eng._stream()), "pf_graph_launch")
        return self.state()

    def read(self):
        """x and the whole workspace on the host."""
        torch.cuda.synchronize()
        x, ws = self.x.cpu().numpy().reshape(self.m, -1), self.ws.cpu().numpy().reshape(self.m, -1)
        out = [(x[k], ws[k]) for k in range(self.m)]
        return out if self.batched else out[0]

    def parts(self, k=0):
        """The named parts of right-hand side k's workspace on the host: r, z, p, ap, dinv, state, and w, y with a dc."""
        torch.cuda.synchronize()
        ws = self.ws[k * self.stride:(k + 1) * self.stride].cpu().numpy()
        return {name: ws[lo:hi] for name, (lo, hi) in self.offsets.items() if name != "partials"}


# ---------------------------------------------------------------------------------------------------------------------
# one truss on the device
# ---------------------------------------------------------------------------------------------------------------------
class DeviceTruss:
    """FEMModel + HipEngine of one truss, and what every device test reads off it.  nodes [n_nodes, dim]; mask / free: the
    fixed / free dofs; degree: per dof, the number of elements at its node.  young, area: scalars or net properties."""

    def __init__(self, nodes, el, fixed, dim, young, area, loads=None):
        from pinn_fem_amd import _capi
        from pinn_fem_amd.engine import HipEngine
        from pinn_fem_amd.fem.model import FEMModel, Material
        self.capi, self.dim = _capi, dim
        self.nodes = np.asarray(nodes, dtype=np.float64).reshape(-1, dim)
        self.el, self.fixed = np.asarray(el), np.asarray(fixed, dtype=int)
        self.n_nodes, self.ne = len(self.nodes), len(self.el)
        self.n = self.n_nodes * dim
        self.free = gl.free_mask(self.n, self.fixed)
        self.mask = ~self.free
        self.degree = np.repeat(np.bincount(self.el.reshape(-1), minlength=self.n_nodes), dim)
        self.max_degree = int(self.degree.max())
        self.model = FEMModel(nodes=self.nodes if dim == 2 else self.nodes.reshape(-1), elements=self.el,
                              material=Material(young, area, 1.0), loads=np.zeros(self.n) if loads is None else loads,
                              fixed_dofs=self.fixed, dimension=dim)
        self.eng = HipEngine(self.model)
        self.lib = self.eng.lib

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.eng.device)


class LinearTruss(DeviceTruss):
    """A truss and its CPU float64 matrices (tests of the linear operator: test_pcg_f64.py, test_pcg_two_level.py).  `K`,
    `Kabs` are built from the plan's own float32 geometry widened to float64 (the inputs the kernel reads) with
    s = (E*A)/l0 as the kernel forms it; from_f64_coordinates() builds them from the float64 node coordinates."""

    def __init__(self, nodes, el, fixed, dim, young=3.0, area=0.25, net_widths=(None, None), seed=0):
        from pinn_fem_amd.fem.properties import NNProperty
        from pinn_fem_amd.nets import SimpleNN
        torch.manual_seed(seed)
        props = []
        for w, scale in zip(net_widths, (young, area)):
            props.append(scale if w is None else
                         NNProperty(net=SimpleNN(hidden_layers=2, neurons_per_layer=w, input_dim=dim + 1),
                                    input_dim=dim + 1, enforce_positive=True, scale=scale))
        super().__init__(nodes, el, fixed, dim, props[0], props[1])
        ea = []
        if any(w is not None for w in net_widths):
            self.eng.eval_properties(1.0)
            torch.cuda.synchronize()
        for w, scale, buf in zip(net_widths, (young, area), (self.eng.prop_e, self.eng.prop_a)):
            # the nets are not under test: their float32 outputs are read back and fed to the reference
            ea.append(np.full(self.ne, np.float32(scale), dtype=np.float64) if w is None
                      else buf[:self.ne].cpu().numpy().astype(np.float64))
        self.E, self.A = ea
        assert np.all(np.isfinite(self.E * self.A)) and np.all(self.E * self.A > 0)
        self._cache = {}

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    @property
    def geo(self):
        return self.eng.plan.egeo.astype(np.float64)

    @property
    def s(self):
        return (self.E * self.A) / self.geo[:, 3]

    K = property(lambda self: self._get("K", lambda: ref.k_csr(self.geo, self.el, self.s, self.dim, self.n_nodes)))
    Kabs = property(lambda self: self._get("Kabs", lambda: ref.abs_k_csr(self.geo, self.el, self.s, self.dim, self.n_nodes)))
    Kff = property(lambda self: self._get("Kff", lambda: ref.restrict_ff(self.K, self.mask)))
    dinv = property(lambda self: self._get("dinv", lambda: ref.jacobi_dinv(self.K, self.mask)))

    def from_f64_coordinates(self):
        g = ref.geo_f64(self.nodes if self.dim == 2 else self.nodes[:, 0], self.el, self.dim)
        s = (self.E * self.A) / g[:, 3]
        return (ref.k_csr(g, self.el, s, self.dim, self.n_nodes), ref.abs_k_csr(g, self.el, s, self.dim, self.n_nodes))

    def kv(self, v, zero_fixed):
        out = self.eng.kv_f64(self.dev(v), zero_fixed=zero_fixed)
        torch.cuda.synchronize()
        return out.cpu().numpy()


class GlTruss(DeviceTruss):
    """A truss with test-owned Green-Lagrange element buffers (d0, kt, fe, strain) and the raw entry points on them, each
    with its output filled with 7.0 first: what the kernel does not write stays visible."""

    def __init__(self, nodes, el, fixed, dim):
        super().__init__(nodes, el, fixed, dim, YOUNG, AREA)
        d0 = self.nodes[self.el[:, 1]] - self.nodes[self.el[:, 0]]
        self.d0 = self.dev(d0.reshape(-1))
        self.kt, self.fe, self.strain = (self._sevens(k) for k in (self.ne * (3 if dim == 2 else 1), self.ne * dim, self.ne))
        self.rec = self.capi.PfGl()
        self.rec.d0, self.rec.kt, self.rec.fe, self.rec.strain = (t.data_ptr() for t in (self.d0, self.kt, self.fe, self.strain))

    def _sevens(self, *shape):
        return torch.full(shape, 7.0, dtype=torch.float64, device=self.eng.device)

    def _call(self, name, *args, record=True):
        """lib.<name>(engine, [the element record,] *args, stream) on the engine's stream, checked and waited for."""
        eng = self.eng
        head = (eng._ref(), C.byref(self.rec)) if record else (eng._ref(),)
        with eng.on_stream():
            self.capi.check(getattr(self.lib, name)(*head, *args, eng._stream()), name)
        torch.cuda.synchronize()

    def refill(self):
        for t in (self.kt, self.fe, self.strain):
            t.fill_(7.0)

    def state(self, u, e0=None, ea=None):
        """pf_gl_state at u, pf_gl_state_ea with a per-element ea, pf_gl_state_e0 with an initial strain (ea then given
        too or NULL) -> (strain, fe [ne, dim], kt [ne, 3 or 1]) on the host."""
        uu, ee, zz = self.dev(u), (None if ea is None else self.dev(ea)), (None if e0 is None else self.dev(e0))
        ep = None if ee is None else ee.data_ptr()
        self.refill()
        if zz is not None:
            self._call("pf_gl_state_e0", ep, zz.data_ptr(), uu.data_ptr())
        elif ee is not None:
            self._call("pf_gl_state_ea", ep, uu.data_ptr())
        else:
            self._call("pf_gl_state", uu.data_ptr())
        return (self.strain.cpu().numpy(), self.fe.cpu().numpy().reshape(self.ne, self.dim),
                self.kt.cpu().numpy().reshape(self.ne, -1))

    def fint(self):
        out = self._sevens(self.n)
        self._call("pf_gl_fint", out.data_ptr())
        return out.cpu().numpy()

    def kt_v(self, v, zero_fixed=False):
        vv, out = self.dev(v), self._sevens(self.n)
        self._call("pf_kt_v_f64", self.kt.data_ptr(), vv.data_ptr(), out.data_ptr(), int(zero_fixed), record=False)
        return out.cpu().numpy()

    def kt_diag(self):
        out = self._sevens(self.n)
        self._call("pf_kt_diag_f64", self.kt.data_ptr(), out.data_ptr(), record=False)
        return out.cpu().numpy()

    def kv_linear(self, v):
        out = self.eng.kv_f64(self.dev(v))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def sens(self, u, a, e0=None, accumulate=0, out=None):
        """pf_gl_sens (e0 given: pf_gl_sens_e0) -> the device tensor [ne], `out` if given."""
        uu, aa, zz = self.dev(u), self.dev(a), (None if e0 is None else self.dev(e0))
        out = self._sevens(self.ne) if out is None else out
        if zz is None:
            self._call("pf_gl_sens", uu.data_ptr(), aa.data_ptr(), int(accumulate), out.data_ptr())
        else:
            self._call("pf_gl_sens_e0", zz.data_ptr(), uu.data_ptr(), aa.data_ptr(), int(accumulate), out.data_ptr())
        return out

    def group_rhs(self, ids, g0, m):
        """pf_gl_group_rhs on the element buffers as the last state() left them, ids a device group map -> [m, n] on the host."""
        out = self._sevens(m, self.n)
        self._call("pf_gl_group_rhs", ids.data_ptr(), g0, m, out.data_ptr())
        return out.cpu().numpy()

    def prestress_rhs(self, u, ea, ids, g0, m):
        uu, ee, out = self.dev(u), self.dev(ea), self._sevens(m, self.n)
        self._call("pf_gl_prestress_rhs", ee.data_ptr(), uu.data_ptr(), ids.data_ptr(), g0, m, out.data_ptr())
        return out.cpu().numpy()

    def strain_rhs(self, u, coef, accumulate=0, out=None):
        uu, cc = self.dev(u), self.dev(coef)
        out = self._sevens(self.n) if out is None else out
        self._call("pf_gl_strain_rhs", uu.data_ptr(), cc.data_ptr(), int(accumulate), out.data_ptr())
        return out.cpu().numpy()

    def strain_jvp(self, u, elems, V):
        """pf_gl_strain_jvp for the rows of V [m, n_dofs] -> [m, len(elems)] on the host."""
        uu, vv, ids = self.dev(u), self.dev(np.asarray(V).reshape(-1)), device_ids(self, elems)
        out = self._sevens(len(V), len(elems))
        self._call("pf_gl_strain_jvp", uu.data_ptr(), ids.data_ptr(), len(elems), vv.data_ptr(), len(V), out.data_ptr())
        return out.cpu().numpy()


def device_ids(S, groups):
    return torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(S.eng.device)


def group_maps(S, rng, n_groups):
    """name -> [n_elems] group ids: random in 0..n_groups - 1; group 3 empty; some elements at -1 and some at G + 3."""
    random = rng.integers(0, n_groups, S.ne)
    hole = np.where(random == 3, 1, random)
    stray = random.copy()
    pick = rng.permutation(S.ne)
    stray[pick[: max(1, S.ne // 7)]] = -1
    stray[pick[max(1, S.ne // 7): max(1, S.ne // 7) + S.ne // 9]] = n_groups + 3
    return {"random": random, "one empty group": hole, "ids -1 and G + 3": stray}


def check_state(got, bounds, label):
    """(strain, fe, kt) as GlTruss.state returns them against [(want, bound)] in that order, entry by entry."""
    for what, g, (want, bound) in zip(("strain", "fe", "kt"), got, bounds):
        g = g.reshape(want.shape)
        assert np.all(np.isfinite(g)), what
        err = np.abs(g - want)
        print(f"{label} {what}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
              f"relative {np.max(err) / np.max(np.abs(want)):.2e}")
        assert np.all(err <= bound), what


# ---------------------------------------------------------------------------------------------------------------------
# the Green-Lagrange Newton solve and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def gl_config(**kw):
    from pinn_fem_amd.fem.solver import SolverConfig
    return SolverConfig(**{**dict(max_iterations=50, tolerance=1e-10, kinematics="green-lagrange"), **kw})


def truss_model(nodes, el, loads, fixed, dim=2):
    from pinn_fem_amd.fem.model import FEMModel, Material
    return FEMModel(nodes=nodes, elements=el, material=Material(YOUNG, AREA, 1.0), loads=loads, fixed_dofs=fixed, dimension=dim)


def case_model(case):
    """The model of an identification case of the restatements (identify_reference.Case and its kin)."""
    return truss_model(case.nodes, case.el, case.loads, case.fixed)


def run_cli(tmp_path, input_name, as_name=None, parse=False):
    """Copy tests/nl_inputs/<input_name>.json to tmp_path (as <as_name>.json) and run the generic CLI on it -> the parsed
    .res.json; parse: (that, the CLI's own parse of the input)."""
    from pinn_fem_amd.cli import generic as g
    copy = tmp_path / ((as_name or input_name) + ".json")
    shutil.copy(os.path.join(os.path.dirname(os.path.abspath(__file__)), "nl_inputs", input_name + ".json"), copy)
    g.main(["generic.py", str(copy)])
    out = json.loads(copy.with_suffix(".res.json").read_text())
    return (out, g.parse_problem(str(copy))) if parse else out


def system_cache(make):
    """The body of a module-scoped `systems` fixture: name -> make(name), built once per module and dropped with it."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make(name)
        return cache[name]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# meshes, fields, right-hand sides
# ---------------------------------------------------------------------------------------------------------------------
def irregular_truss_with_supports(n_elems, rng):
    """gl.irregular_truss with node 0 and ux of node 1 fixed, and a random 10 % of the dofs on top."""
    nodes, el = gl.irregular_truss(n_elems, rng)
    fixed = np.unique(np.concatenate([[0, 1, 2], rng.choice(nodes.size, size=max(1, nodes.size // 10), replace=False)]))
    return nodes, el, fixed


def flipped_chain_1d(n_elems, rng):
    """1-D chain of uneven elements held at node 0: random element orientation, shuffled element order."""
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(n_elems))])
    e = np.arange(n_elems)
    el = np.stack([e, e + 1], axis=1)
    flip = rng.random(n_elems) < 0.5
    el[flip] = el[flip][:, ::-1]
    return x, el[rng.permutation(n_elems)], np.array([0])


def gl_system(name):
    """"truss_<n>" or "chain_<n>": the n-element GlTruss of the Green-Lagrange and the identification tests."""
    kind, count = name.split("_")
    n = int(count)
    if kind == "truss":
        return GlTruss(*irregular_truss_with_supports(n, np.random.default_rng(1000 + n)), 2)
    return GlTruss(*flipped_chain_1d(n, np.random.default_rng(2000 + n)), 1)


def gl_field(S, kind, rng):
    """Displacements with |du| / l0 about 0.3 ("large") or 1e-9 ("tiny": where (l^2 - l0^2) would lose every digit)."""
    mean_l0 = float(np.mean(np.linalg.norm(S.nodes[S.el[:, 1]] - S.nodes[S.el[:, 0]], axis=1)))
    amp = {"large": 0.3, "tiny": 1e-9}[kind] * mean_l0 / math.sqrt(2.0 * S.dim)
    return amp * rng.standard_normal(S.n)


def bar1d(n_nodes, rng):
    x, el, _ = ref.pinned_bar(n_nodes, rng)
    flip = rng.random(len(el)) < 0.5
    el[flip] = el[flip][:, ::-1]
    fixed = np.unique(np.concatenate([[0], rng.choice(n_nodes, size=max(1, n_nodes // 9), replace=False)]))
    return x, el, fixed


def hub_truss(rng):
    nodes, el = _random_truss(2500, rng, 300)
    fixed = np.unique(rng.choice(5000, size=250, replace=False))
    return nodes, el, fixed


def wide_vector(rng, n):
    """random signs, magnitudes spread over 2^-20 .. 2^20"""
    return rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-20.0, 20.0, n))


def manufactured(S, rng):
    xs = np.where(S.mask, 0.0, rng.standard_normal(S.n))
    return xs, S.Kff @ xs
