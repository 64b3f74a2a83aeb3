// pf_nl.hip — the geometrically nonlinear (total-Lagrangian, Green-Lagrange strain) truss element in float64: element state
// and internal force for the Newton-Raphson solve on large displacements.
//
// Per element with nodes i, j:  d0 = X_j - X_i (float64, from the caller: pf_gl.d0),  du = u_j - u_i,  d = d0 + du,
//   e  = (2 d0.du + du.du) / (2 l0^2)          the difference of squares written out: (l^2 - l0^2) cancels at small strain
//   N  = E*A * e                               E*A as pf_pcg.hip forms it (elem_ea64)
//   fe = (N / l0) d                            f_int[j] += fe, f_int[i] -= fe
//   B  = (E*A / l0^3) d d^T + (N / l0) I       K_t v: row j += B (v_j - v_i), row i -= B (v_j - v_i)
// B is what pf_pcg.hip's gather64 reads as `kt`.  The reference's truss2d_element_state (fem/element.py:105-133) is NOT
// this element: its force has the other sign and lacks 1/l0, and its "nonlinear" stiffness is e d d^T, not (N/l0) I.
//
// k_gl_state: one element per thread (grid-stride), coalesced records out, two gathered node vectors in.
// k_gl_fint:  one node per thread, +-fe of the node's elements in ascending element id, no atomics; the adjacency codes
//             and the records of two incidences are loaded together (selects, not branches), as the node kernels of
//             pf_node.h issue theirs.
#include <stdio.h>
#include "pf_common.h"

namespace {

template <int DIM>
__global__ __launch_bounds__(256) void k_gl_state(pf_problem P, pf_gl G, const double* __restrict__ u) {
  const pf_mesh& M = P.mesh;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < M.n_elems; e += gridDim.x * blockDim.x) {
    const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
    double d0[DIM], du[DIM];
    if (DIM == 2) {
      const double2 a = reinterpret_cast<const double2*>(G.d0)[e];
      const double2 ui = reinterpret_cast<const double2*>(u)[nn.x], uj = reinterpret_cast<const double2*>(u)[nn.y];
      d0[0] = a.x; d0[DIM - 1] = a.y;
      du[0] = uj.x - ui.x; du[DIM - 1] = uj.y - ui.y;
    } else {
      d0[0] = G.d0[e];
      du[0] = u[nn.y] - u[nn.x];
    }
    const double ea = elem_ea64(P, e);
    double l02 = 0.0, d0du = 0.0, dudu = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) { l02 += d0[c] * d0[c]; d0du += d0[c] * du[c]; dudu += du[c] * du[c]; }
    const double l0 = sqrt(l02);
    const double strain = (2.0 * d0du + dudu) / (2.0 * l02);
    const double n_l0 = (ea * strain) / l0;          // N / l0
    const double k = ea / (l02 * l0);                // E*A / l0^3
    double d[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) d[c] = d0[c] + du[c];
    G.strain[e] = strain;
    if (DIM == 2) {
      reinterpret_cast<double2*>(G.fe)[e] = make_double2(n_l0 * d[0], n_l0 * d[DIM - 1]);
      double* __restrict__ b = G.kt + 3 * (size_t)e;
      b[0] = k * (d[0] * d[0]) + n_l0;
      b[1] = k * (d[0] * d[DIM - 1]);
      b[2] = k * (d[DIM - 1] * d[DIM - 1]) + n_l0;
    } else {
      G.fe[e] = n_l0 * d[0];
      G.kt[e] = k * (d[0] * d[0]) + n_l0;
    }
  }
}

// +fe at the element's second node (end 1), -fe at its first
template <int DIM>
__device__ __forceinline__ void load_fe(const double* __restrict__ fe, int code, double* out) {
  const int e = code >> 1;
  const double sg = (code & 1) ? 1.0 : -1.0;
  if (DIM == 2) {
    const double2 f = reinterpret_cast<const double2*>(fe)[e];
    out[0] = sg * f.x; out[DIM - 1] = sg * f.y;
  } else {
    out[0] = sg * fe[e];
  }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_gl_fint(pf_problem P, const double* __restrict__ fe, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    const int b = M.adj_ptr[node], e_ = M.adj_ptr[node + 1];
    double acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
    for (int idx = b; idx < e_; idx += 2) {
      const bool two = idx + 1 < e_;
      const int code0 = M.adj[idx], code1 = M.adj[two ? idx + 1 : idx];
      double f0[DIM], f1[DIM];
      load_fe<DIM>(fe, code0, f0);
      load_fe<DIM>(fe, code1, f1);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        acc[c] += f0[c];
        const double t = acc[c] + f1[c];
        acc[c] = two ? t : acc[c];
      }
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) out[node * DIM + c] = acc[c];
  }
}

int gl_fail(int code, const char* who, const char* what) {
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  pf_set_error(buf);
  return code;
}

bool mesh_ok(const pf_problem* p) { return p && (p->mesh.dim == 1 || p->mesh.dim == 2) && p->mesh.n_elems >= 0; }

}  // namespace

extern "C" {

int pf_gl_state(const pf_problem* p, const pf_gl* g, const double* u, void* stream) {
  const char* who = "pf_gl_state";
  if (!mesh_ok(p) || !g || !g->d0 || !g->kt || !g->fe || !g->strain || !u) return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_elems == 0) return PF_OK;
  int nb = (p->mesh.n_elems + 255) / 256;
  if (nb > PF_MAX_NODE_BLOCKS) nb = PF_MAX_NODE_BLOCKS;
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_state<2>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p, *g, u);
  else hipLaunchKernelGGL(k_gl_state<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p, *g, u);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

int pf_gl_fint(const pf_problem* p, const pf_gl* g, double* f_int_out, void* stream) {
  const char* who = "pf_gl_fint";
  if (!mesh_ok(p) || !g || !g->fe || !f_int_out) return gl_fail(PF_ERR_ARG, who, "bad argument");
  const int nb = pf_node_blocks(p->mesh.n_nodes);
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_fint<2>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p, g->fe, f_int_out);
  else hipLaunchKernelGGL(k_gl_fint<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p, g->fe, f_int_out);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

}  // extern "C"
