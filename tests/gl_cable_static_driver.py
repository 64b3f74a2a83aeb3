"""The raw pf_gl_state_cable wrapper of tests/test_gl_cable_static_f64.py on a device_driver.GlTruss: test-owned flags,
slack set and counts, the outputs filled with 7.0 first so that what the kernel does not write stays visible.  A plain
support module like device_driver.py: no fixtures, no tests.
"""
import numpy as np
import torch


class CableState:
    """pf_gl_state_cable on S (a GlTruss).  slack is in/out: clear() empties it, every state() leaves the current set."""

    def __init__(self, S):
        self.S = S
        dev = S.eng.device
        self.cable = torch.zeros(max(S.ne, 1), dtype=torch.uint8, device=dev)
        self.slack = torch.zeros(max(S.ne, 1), dtype=torch.uint8, device=dev)
        self.counts = torch.full((S.capi.PF_GL_CABLE_COUNT,), 7.0, dtype=torch.float64, device=dev)
        self.blocks = min((S.ne + 255) // 256, S.capi.PF_MAX_NODE_BLOCKS)

    def clear(self):
        self.slack.zero_()

    def state(self, u, cable, e0=None, ea=None):
        """-> (strain, fe [ne, dim], kt [ne, 3 or 1], slack bool [ne], (n_slack, n_changed) as the doubles the device wrote)."""
        S = self.S
        self.cable[: S.ne] = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(cable, (S.ne,)), dtype=np.uint8)).to(S.eng.device)
        uu, ee, zz = S.dev(u), (None if ea is None else S.dev(ea)), (None if e0 is None else S.dev(e0))
        S.refill()
        self.counts.fill_(7.0)
        S._call("pf_gl_state_cable", None if ee is None else ee.data_ptr(), None if zz is None else zz.data_ptr(),
                self.cable.data_ptr(), self.slack.data_ptr(), self.counts.data_ptr(), uu.data_ptr())
        counts = self.counts.cpu().numpy()
        return (S.strain.cpu().numpy(), S.fe.cpu().numpy().reshape(S.ne, S.dim), S.kt.cpu().numpy().reshape(S.ne, -1),
                self.slack[: S.ne].cpu().numpy().astype(bool), (counts[0], counts[1]))

    def everything(self):
        """Every byte the entry point may write: the element record, the slack set and the whole counts buffer."""
        S = self.S
        torch.cuda.synchronize()
        return b"".join(t.cpu().numpy().tobytes() for t in (S.strain, S.fe, S.kt, self.slack, self.counts))


def host_slack(cable, strain, e0):
    """The rule on the device's own strains, with the kernel's subtraction: e - e0, or e - 0.0 without an e0."""
    return np.asarray(cable, dtype=bool) & ((strain - (0.0 if e0 is None else e0)) < 0.0)
