"""The raw pf_gl_state_plastic wrapper of tests/test_gl_plastic_f64.py on a device_driver.GlTruss: test-owned yield strains,
hardening ratios, committed and trial (ep, alpha), flags and counts, the outputs filled with 7.0 first so that what the kernel
does not write stays visible.  A plain support module like device_driver.py: no fixtures, no tests.
"""
import ctypes as C

import numpy as np
import torch

import gl_plastic_reference as gp

EA = 1000.0
# the seeds of the device test's yielding fields (tests/test_gl_plastic_host.py asserts the margin condition for them): (mesh, seed)
FIELD_SEEDS = {"truss_257": 4257, "truss_1000": 5000, "chain_257": 4258, "chain_1000": 5001}
KAPPAS = ("0", "0.05", "per-element")


def field_case(name, kappa_name, with_e0_ea):
    """The seeded yielding field of the device test on mesh `name`: (nodes, el, fixed, dim, u, u_other, kappa, ep_n, al_n,
    e0, ea).  Built from the seeds alone, so the host test can assert the margin condition for what the device test runs."""
    from device_driver import flipped_chain_1d, irregular_truss_with_supports
    kind, count = name.split("_")
    n = int(count)
    if kind == "truss":
        nodes, el, fixed = irregular_truss_with_supports(n, np.random.default_rng(1000 + n))
        dim = 2
    else:
        nodes, el, fixed = flipped_chain_1d(n, np.random.default_rng(2000 + n))
        dim = 1
    rng = np.random.default_rng(FIELD_SEEDS[name] + 17 * KAPPAS.index(kappa_name) + (7 if with_e0_ea else 0))
    u, other = gp.seeded_field(nodes, el, dim, rng), gp.seeded_field(nodes, el, dim, rng)
    kappa = gp.kappa_case(kappa_name, n, rng)
    ep_n, al_n = gp.seeded_state(n, rng)
    e0 = rng.uniform(-3e-4, 3e-4, n) if with_e0_ea else None
    ea = EA * rng.uniform(0.5, 2.0, n) if with_e0_ea else None
    return nodes, el, fixed, dim, u, other, kappa, ep_n, al_n, e0, ea


def wrap_case():
    """The chain of PF_MAX_NODE_BLOCKS * 256 + 37 elements of the grid-stride test and its seeded yielding field (kappa
    0.05, a virgin state): (x, el, fixed, u).  The first 37 threads of the launch take a second element."""
    from device_driver import flipped_chain_1d
    from pinn_fem_amd import _capi
    ne = _capi.PF_MAX_NODE_BLOCKS * 256 + 37
    x, el, fixed = flipped_chain_1d(ne, np.random.default_rng(ne))
    # (among a million elements the nearest one lies about 1e-6 ey from its branch point; seeds ne + 1 .. ne + 6 leave it
    # under the margin, this one keeps it)
    return x, el, fixed, gp.seeded_field(x, el, 1, np.random.default_rng(ne + 7))


class PlasticState:
    """pf_gl_state_plastic on S (a GlTruss).  yielding is in/out: clear() empties it, every state() leaves the current flags."""

    def __init__(self, S):
        self.S = S
        dev, ne = S.eng.device, max(S.ne, 1)
        f64 = dict(dtype=torch.float64, device=dev)
        self.ey, self.kappa, self.ep_n, self.al_n = (torch.zeros(ne, **f64) for _ in range(4))
        self.ep, self.al = torch.full((ne,), 7.0, **f64), torch.full((ne,), 7.0, **f64)
        self.yielding = torch.zeros(ne, dtype=torch.uint8, device=dev)
        self.counts = torch.full((S.capi.PF_GL_CABLE_COUNT,), 7.0, **f64)
        self.blocks = min((S.ne + 255) // 256, S.capi.PF_MAX_NODE_BLOCKS)

    def clear(self):
        self.yielding.zero_()

    def record(self, **swap):
        """The pf_gl_plastic of the buffers, with any pointer replaced by name (None: a null pointer)."""
        pl = self.S.capi.PfGlPlastic()
        for name in ("ey", "kappa", "ep_n", "al_n", "ep", "al", "yielding", "counts"):
            t = swap.get(name, getattr(self, name))
            setattr(pl, name, None if t is None else t.data_ptr())
        return pl

    def set(self, ey, kappa, ep_n=0.0, al_n=0.0):
        ne = self.S.ne
        for t, v in ((self.ey, ey), (self.kappa, kappa), (self.ep_n, ep_n), (self.al_n, al_n)):
            t[:ne] = torch.from_numpy(np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (ne,)))).to(t.device)

    def state(self, u, ey, kappa, ep_n=0.0, al_n=0.0, e0=None, ea=None):
        """-> (strain, fe [ne, dim], kt [ne, 3 or 1], ep, al, yielding bool [ne], (n_plastic, n_changed) as the doubles the
        device wrote)."""
        S = self.S
        self.set(ey, kappa, ep_n, al_n)
        uu, ee, zz = S.dev(u), (None if ea is None else S.dev(ea)), (None if e0 is None else S.dev(e0))
        S.refill()
        for t in (self.ep, self.al, self.counts):
            t.fill_(7.0)
        pl = self.record()
        S._call("pf_gl_state_plastic", None if ee is None else ee.data_ptr(), None if zz is None else zz.data_ptr(),
                C.byref(pl), uu.data_ptr())
        counts = self.counts.cpu().numpy()
        return (S.strain.cpu().numpy(), S.fe.cpu().numpy().reshape(S.ne, S.dim), S.kt.cpu().numpy().reshape(S.ne, -1),
                self.ep[: S.ne].cpu().numpy(), self.al[: S.ne].cpu().numpy(),
                self.yielding[: S.ne].cpu().numpy().astype(bool), (counts[0], counts[1]))

    def inputs(self):
        """The bytes of the four input arrays."""
        torch.cuda.synchronize()
        return b"".join(t.cpu().numpy().tobytes() for t in (self.ey, self.kappa, self.ep_n, self.al_n))

    def everything(self):
        """Every byte the entry point may read or write: the element record, the eight buffers of the plastic record."""
        S = self.S
        torch.cuda.synchronize()
        return b"".join(t.cpu().numpy().tobytes() for t in (S.strain, S.fe, S.kt, self.ey, self.kappa, self.ep_n, self.al_n,
                                                            self.ep, self.al, self.yielding, self.counts))
