// pf_nl.hip — the geometrically nonlinear (total-Lagrangian, Green-Lagrange strain) truss element in float64: element state
// and internal force for the Newton-Raphson solve on large displacements.
//
// Per element with nodes i, j:  d0 = X_j - X_i (float64, from the caller: pf_gl.d0),  du = u_j - u_i,  d = d0 + du,
//   e  = (2 d0.du + du.du) / (2 l0^2)          the difference of squares written out: (l^2 - l0^2) cancels at small strain
//   N  = E*A * e                               E*A as pf_pcg.hip forms it (elem_ea64); with an initial strain e0
//                                              (pf_gl_state_e0: prestress, thermal, lack of fit) N = E*A * (e - e0)
//   fe = (N / l0) d                            f_int[j] += fe, f_int[i] -= fe
//   B  = (E*A / l0^3) d d^T + (N / l0) I       K_t v: row j += B (v_j - v_i), row i -= B (v_j - v_i)
// B is what pf_pcg.hip's gather64 reads as `kt`.  The reference's truss2d_element_state (fem/element.py:105-133) is NOT
// this element: its force has the other sign and lacks 1/l0, and its "nonlinear" stiffness is e d d^T, not (N/l0) I.
//
// k_gl_state: one element per thread (grid-stride), coalesced records out, two gathered node vectors in.  E*A is
//             elem_ea64, or the caller's per-element float64 array (pf_gl_state_ea: the identification of DESIGN.md §7).
//             e0 (nullable, the same decision in every thread as ea): e - e0[e] is formed once, after e as above, and
//             takes e's place in N; the strain written out stays e.  e - 0.0 is e to the bit.
// k_gl_fint:  one node per thread, +-fe of the node's elements in ascending element id, no atomics; the adjacency codes
//             and the records of two incidences are loaded together (selects, not branches), as the node kernels of
//             pf_node.h issue theirs.
// k_gl_sens:  dJ/d(E*A) of an element from the state u and an adjoint a: -(e / l0) d.(a_j - a_i); k_gl_state's loads
//             and its strain (less e0[e] when e0 is given, as k_gl_state), one store (or one load and one store when
//             it accumulates), no atomics.
// k_group_sum: out[g] = sum of values[e] * weights[e] over the elements of group g (CSR, ascending element id): one
//             workgroup per group, thread t adds elements t, t + 256, ... in that order, then the fixed-order block
//             sum of pf_pcg.hip's block_sum64.  No atomics: the same bits on every run.
// k_gl_group_rhs: k_gl_fint restricted to the elements of one group and negated: the right-hand side of the sensitivity
//             solve K_t s = -d f_int / d q_g (f_int is linear in E*A, so that derivative is the group's own internal
//             force).  One node per thread, the group in blockIdx.y; the group ids of two incidences are loaded with
//             their codes and records, and an incidence of another group adds +0.0 by a select, so the matching terms
//             are summed in k_gl_fint's order.  Fixed dofs get 0.0.  No atomics.
// k_gl_strain_rhs: B^T c, the transpose of the strain's derivative d e / d u applied to per-element coefficients (the
//             adjoint right-hand side of a strain misfit): one node per thread, +-(c_e / l0^2) d_e of the node's elements
//             in ascending incidence order, two incidences per round with selects as k_gl_fint takes them; d is formed
//             from d0 and u as k_gl_sens forms it.  Fixed dofs get 0.0, or stay untouched when it accumulates.  No atomics.
// k_gl_strain_jvp: B v, that derivative applied to vectors, at the measured elements only: (d_e / l0^2).(v_j - v_i), one
//             (gauge, row) pair per thread with the row in blockIdx.y; an element id outside the mesh writes 0.0 and
//             reads nothing, k_group_sum's rule.
// k_gl_prestress_rhs: the right-hand side of the sensitivity solve K_t s = -d f_int / d t_h for an additive initial strain
//             t_h on the elements of group h: f_int is affine in e0 with d fe / d e0 = -(E*A / l0) d, so the row is the
//             node gather of +-(ea_e / l0) d_e over the group's elements.  k_gl_group_rhs's shape: one node per thread, the
//             group in blockIdx.y, two incidences per round whose codes, group ids, conn, d0 records and ea are loaded
//             together, and an incidence of another group adds +0.0 by a select.  d is formed from d0 and u as
//             k_gl_strain_rhs forms it, so it reads no record of pf_gl_state.  Fixed dofs get 0.0.  No atomics.
#include <limits.h>
#include <stdio.h>
#include "pf_common.h"

namespace {

template <int DIM>
__global__ __launch_bounds__(256) void k_gl_state(pf_problem P, pf_gl G, const double* __restrict__ u,
                                                  const double* __restrict__ ea_in, const double* __restrict__ e0_in) {
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
    const double ea = ea_in ? ea_in[e] : elem_ea64(P, e);
    double l02 = 0.0, d0du = 0.0, dudu = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) { l02 += d0[c] * d0[c]; d0du += d0[c] * du[c]; dudu += du[c] * du[c]; }
    const double l0 = sqrt(l02);
    const double strain = (2.0 * d0du + dudu) / (2.0 * l02);
    const double se = e0_in ? strain - e0_in[e] : strain;     // the strain that carries stress
    const double n_l0 = (ea * se) / l0;              // N / l0
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

template <int DIM>
__global__ __launch_bounds__(256) void k_gl_sens(pf_problem P, const double* __restrict__ d0_in, const double* __restrict__ u,
                                                 const double* __restrict__ a, const double* __restrict__ e0_in, int accumulate,
                                                 double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < M.n_elems; e += gridDim.x * blockDim.x) {
    const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
    double d0[DIM], du[DIM], da[DIM];
    if (DIM == 2) {
      const double2 g = reinterpret_cast<const double2*>(d0_in)[e];
      const double2 ui = reinterpret_cast<const double2*>(u)[nn.x], uj = reinterpret_cast<const double2*>(u)[nn.y];
      const double2 ai = reinterpret_cast<const double2*>(a)[nn.x], aj = reinterpret_cast<const double2*>(a)[nn.y];
      d0[0] = g.x; d0[DIM - 1] = g.y;
      du[0] = uj.x - ui.x; du[DIM - 1] = uj.y - ui.y;
      da[0] = aj.x - ai.x; da[DIM - 1] = aj.y - ai.y;
    } else {
      d0[0] = d0_in[e];
      du[0] = u[nn.y] - u[nn.x];
      da[0] = a[nn.y] - a[nn.x];
    }
    double l02 = 0.0, d0du = 0.0, dudu = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) { l02 += d0[c] * d0[c]; d0du += d0[c] * du[c]; dudu += du[c] * du[c]; }
    const double strain = (2.0 * d0du + dudu) / (2.0 * l02);     // as k_gl_state forms it
    double dda = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) dda += (d0[c] + du[c]) * da[c];
    const double se = e0_in ? strain - e0_in[e] : strain;
    const double s = -(se / sqrt(l02)) * dda;
    out[e] = accumulate ? __dadd_rn(out[e], s) : s;      // s rounded first: the sum of two single calls, to the bit
  }
}

// the sum of v over the block's threads, the same on every thread: the order of pf_pcg.hip's block_sum64
__device__ __forceinline__ double block_sum(double v, double* smem) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) smem[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t += smem[i];
  return t;
}

// an element id outside 0..n_elems-1 in group_elems adds nothing (and reads nothing)
__global__ __launch_bounds__(256) void k_group_sum(int n_elems, const double* __restrict__ values,
                                                   const double* __restrict__ weights, const int* __restrict__ group_ptr,
                                                   const int* __restrict__ group_elems, int n_groups,
                                                   double* __restrict__ out) {
  __shared__ double red[8];
  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {        // uniform over the block: the barriers are safe
    const int b = group_ptr[g], e_ = group_ptr[g + 1];
    double acc = 0.0;
    for (int idx = b + (int)threadIdx.x; idx < e_; idx += (int)blockDim.x) {
      const int e = group_elems[idx];
      if ((unsigned)e < (unsigned)n_elems) acc += weights ? values[e] * weights[e] : values[e];
    }
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) out[g] = t;
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

// out[k][dof] = -(sum of +-fe over the node's elements e with elem_group[e] == g0 + k), k = blockIdx.y; 0.0 on fixed dofs
template <int DIM>
__global__ __launch_bounds__(256) void k_gl_group_rhs(pf_problem P, const double* __restrict__ fe,
                                                      const int* __restrict__ elem_group, int g0, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  const int group = g0 + (int)blockIdx.y;
  double* __restrict__ row = out + (size_t)blockIdx.y * (size_t)M.n_dofs;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    const int b = M.adj_ptr[node], e_ = M.adj_ptr[node + 1];
    double acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
    for (int idx = b; idx < e_; idx += 2) {
      const bool two = idx + 1 < e_;
      const int code0 = M.adj[idx], code1 = M.adj[two ? idx + 1 : idx];
      const bool in0 = elem_group[code0 >> 1] == group, in1 = two && elem_group[code1 >> 1] == group;
      double f0[DIM], f1[DIM];
      load_fe<DIM>(fe, code0, f0);
      load_fe<DIM>(fe, code1, f1);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        acc[c] += in0 ? f0[c] : 0.0;
        acc[c] += in1 ? f1[c] : 0.0;
      }
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node * DIM + c;
      row[dof] = (M.dof_flags[dof] & PF_DOF_FIXED) ? 0.0 : -acc[c];
    }
  }
}

// +-(coef[e] / l0^2) d of one incidence: + at the element's second node (end 1), - at its first; d as k_gl_sens forms it
template <int DIM>
__device__ __forceinline__ void load_strain_term(const pf_mesh& M, const double* __restrict__ d0_in, const double* __restrict__ u,
                                                 const double* __restrict__ coef, int code, double* out) {
  const int e = code >> 1;
  const double sg = (code & 1) ? 1.0 : -1.0;
  const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
  double d0[DIM], du[DIM];
  if (DIM == 2) {
    const double2 g = reinterpret_cast<const double2*>(d0_in)[e];
    const double2 ui = reinterpret_cast<const double2*>(u)[nn.x], uj = reinterpret_cast<const double2*>(u)[nn.y];
    d0[0] = g.x; d0[DIM - 1] = g.y;
    du[0] = uj.x - ui.x; du[DIM - 1] = uj.y - ui.y;
  } else {
    d0[0] = d0_in[e];
    du[0] = u[nn.y] - u[nn.x];
  }
  double l02 = 0.0;
#pragma unroll
  for (int c = 0; c < DIM; ++c) l02 += d0[c] * d0[c];
  const double w = coef[e] / l02;
#pragma unroll
  for (int c = 0; c < DIM; ++c) out[c] = sg * (w * (d0[c] + du[c]));
}

// +-(ea[e] / l0) d of one incidence, load_strain_term's loads, signs and d; `in` false: +0.0 (the loads are issued all the same)
template <int DIM>
__device__ __forceinline__ void load_prestress_term(const pf_mesh& M, const double* __restrict__ d0_in, const double* __restrict__ u,
                                                    const double* __restrict__ ea, int code, bool in, double* out) {
  const int e = code >> 1;
  const double sg = (code & 1) ? 1.0 : -1.0;
  const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
  double d0[DIM], du[DIM];
  if (DIM == 2) {
    const double2 g = reinterpret_cast<const double2*>(d0_in)[e];
    const double2 ui = reinterpret_cast<const double2*>(u)[nn.x], uj = reinterpret_cast<const double2*>(u)[nn.y];
    d0[0] = g.x; d0[DIM - 1] = g.y;
    du[0] = uj.x - ui.x; du[DIM - 1] = uj.y - ui.y;
  } else {
    d0[0] = d0_in[e];
    du[0] = u[nn.y] - u[nn.x];
  }
  double l02 = 0.0;
#pragma unroll
  for (int c = 0; c < DIM; ++c) l02 += d0[c] * d0[c];
  const double w = ea[e] / sqrt(l02);
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    const double t = sg * (w * (d0[c] + du[c]));
    out[c] = in ? t : 0.0;
  }
}

// out[k][dof] = sum of +-(ea[e] / l0) d_e over the node's elements e with elem_group[e] == g0 + k, k = blockIdx.y; 0.0 on
// fixed dofs
template <int DIM>
__global__ __launch_bounds__(256) void k_gl_prestress_rhs(pf_problem P, const double* __restrict__ d0_in,
                                                          const double* __restrict__ ea, const double* __restrict__ u,
                                                          const int* __restrict__ elem_group, int g0, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  const int group = g0 + (int)blockIdx.y;
  double* __restrict__ row = out + (size_t)blockIdx.y * (size_t)M.n_dofs;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    const int b = M.adj_ptr[node], e_ = M.adj_ptr[node + 1];
    double acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
    for (int idx = b; idx < e_; idx += 2) {
      const bool two = idx + 1 < e_;
      const int code0 = M.adj[idx], code1 = M.adj[two ? idx + 1 : idx];
      const bool in0 = elem_group[code0 >> 1] == group, in1 = two && elem_group[code1 >> 1] == group;
      double t0[DIM], t1[DIM];
      load_prestress_term<DIM>(M, d0_in, u, ea, code0, in0, t0);
      load_prestress_term<DIM>(M, d0_in, u, ea, code1, in1, t1);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        acc[c] += t0[c];
        acc[c] += t1[c];
      }
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node * DIM + c;
      row[dof] = (M.dof_flags[dof] & PF_DOF_FIXED) ? 0.0 : acc[c];
    }
  }
}

// out[dof] = sum over the node's incidences of +-(coef[e] / l0^2) d_e; accumulate: out += that sum, rounded first
template <int DIM>
__global__ __launch_bounds__(256) void k_gl_strain_rhs(pf_problem P, const double* __restrict__ d0_in,
                                                       const double* __restrict__ u, const double* __restrict__ coef,
                                                       int accumulate, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    const int b = M.adj_ptr[node], e_ = M.adj_ptr[node + 1];
    double acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
    for (int idx = b; idx < e_; idx += 2) {
      const bool two = idx + 1 < e_;
      const int code0 = M.adj[idx], code1 = M.adj[two ? idx + 1 : idx];
      double t0[DIM], t1[DIM];
      load_strain_term<DIM>(M, d0_in, u, coef, code0, t0);
      load_strain_term<DIM>(M, d0_in, u, coef, code1, t1);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        acc[c] += t0[c];
        const double t = acc[c] + t1[c];
        acc[c] = two ? t : acc[c];
      }
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node * DIM + c;
      const bool fixed = M.dof_flags[dof] & PF_DOF_FIXED;
      if (accumulate) {
        if (!fixed) out[dof] = __dadd_rn(out[dof], acc[c]);      // acc rounded first: the sum of two single calls, to the bit
      } else {
        out[dof] = fixed ? 0.0 : acc[c];
      }
    }
  }
}

// out[k][i] = (d_e / l0^2).(v_k[j] - v_k[i]) for e = elems[i], k = blockIdx.y; an id outside 0..n_elems-1 gives 0.0
template <int DIM>
__global__ __launch_bounds__(256) void k_gl_strain_jvp(pf_problem P, const double* __restrict__ d0_in,
                                                       const double* __restrict__ u, const int* __restrict__ elems, int n_meas,
                                                       const double* __restrict__ v, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  const double* __restrict__ vk = v + (size_t)blockIdx.y * (size_t)M.n_dofs;
  double* __restrict__ row = out + (size_t)blockIdx.y * (size_t)n_meas;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_meas; i += gridDim.x * blockDim.x) {
    const int e = elems[i];
    double r = 0.0;
    if ((unsigned)e < (unsigned)M.n_elems) {
      const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
      double d0[DIM], du[DIM], dv[DIM];
      if (DIM == 2) {
        const double2 g = reinterpret_cast<const double2*>(d0_in)[e];
        const double2 ui = reinterpret_cast<const double2*>(u)[nn.x], uj = reinterpret_cast<const double2*>(u)[nn.y];
        const double2 vi = reinterpret_cast<const double2*>(vk)[nn.x], vj = reinterpret_cast<const double2*>(vk)[nn.y];
        d0[0] = g.x; d0[DIM - 1] = g.y;
        du[0] = uj.x - ui.x; du[DIM - 1] = uj.y - ui.y;
        dv[0] = vj.x - vi.x; dv[DIM - 1] = vj.y - vi.y;
      } else {
        d0[0] = d0_in[e];
        du[0] = u[nn.y] - u[nn.x];
        dv[0] = vk[nn.y] - vk[nn.x];
      }
      double l02 = 0.0, ddv = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) { l02 += d0[c] * d0[c]; ddv += (d0[c] + du[c]) * dv[c]; }
      r = ddv / l02;
    }
    row[i] = r;
  }
}

int gl_fail(int code, const char* who, const char* what) {
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  pf_set_error(buf);
  return code;
}

bool mesh_ok(const pf_problem* p) { return p && (p->mesh.dim == 1 || p->mesh.dim == 2) && p->mesh.n_elems >= 0; }

int elem_blocks(int n_elems) {
  const int nb = (n_elems + 255) / 256;
  return nb > PF_MAX_NODE_BLOCKS ? PF_MAX_NODE_BLOCKS : nb;
}

int gl_state(const char* who, const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const double* u,
             void* stream) {
  if (!mesh_ok(p) || !g || !g->d0 || !g->kt || !g->fe || !g->strain || !u) return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_elems == 0) return PF_OK;
  const int nb = elem_blocks(p->mesh.n_elems);
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_state<2>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p, *g, u, ea, e0);
  else hipLaunchKernelGGL(k_gl_state<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p, *g, u, ea, e0);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

int gl_sens(const char* who, const pf_problem* p, const pf_gl* g, const double* e0, const double* u, const double* a,
            int accumulate, double* out, void* stream) {
  if (!mesh_ok(p) || !g || !g->d0 || !u || !a || !out || (accumulate != 0 && accumulate != 1))
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_elems == 0) return PF_OK;
  const int nb = elem_blocks(p->mesh.n_elems);
  const hipStream_t s = (hipStream_t)stream;
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_sens<2>, dim3(nb), dim3(256), 0, s, *p, g->d0, u, a, e0, accumulate, out);
  else hipLaunchKernelGGL(k_gl_sens<1>, dim3(nb), dim3(256), 0, s, *p, g->d0, u, a, e0, accumulate, out);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

}  // namespace

extern "C" {

int pf_gl_state(const pf_problem* p, const pf_gl* g, const double* u, void* stream) {
  return gl_state("pf_gl_state", p, g, nullptr, nullptr, u, stream);
}

int pf_gl_state_ea(const pf_problem* p, const pf_gl* g, const double* ea, const double* u, void* stream) {
  if (!ea) return gl_fail(PF_ERR_ARG, "pf_gl_state_ea", "null ea (pf_gl_state is the solve with the problem's own E*A)");
  return gl_state("pf_gl_state_ea", p, g, ea, nullptr, u, stream);
}

int pf_gl_state_e0(const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const double* u, void* stream) {
  if (!e0) return gl_fail(PF_ERR_ARG, "pf_gl_state_e0", "null e0 (pf_gl_state / pf_gl_state_ea are the unstrained solves)");
  return gl_state("pf_gl_state_e0", p, g, ea, e0, u, stream);
}

int pf_gl_sens(const pf_problem* p, const pf_gl* g, const double* u, const double* a, int accumulate, double* out,
               void* stream) {
  return gl_sens("pf_gl_sens", p, g, nullptr, u, a, accumulate, out, stream);
}

int pf_gl_sens_e0(const pf_problem* p, const pf_gl* g, const double* e0, const double* u, const double* a, int accumulate,
                  double* out, void* stream) {
  if (!e0) return gl_fail(PF_ERR_ARG, "pf_gl_sens_e0", "null e0 (pf_gl_sens is the unstrained sensitivity)");
  return gl_sens("pf_gl_sens_e0", p, g, e0, u, a, accumulate, out, stream);
}

int pf_group_sum_f64(int n_elems, const double* values, const double* weights, const int* group_ptr, const int* group_elems,
                     int n_groups, double* out, void* stream) {
  const char* who = "pf_group_sum_f64";
  if (n_elems < 0 || n_groups < 0 || !values || !group_ptr || !group_elems || !out)
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (n_groups == 0) return PF_OK;
  const int nb = n_groups < PF_MAX_NODE_BLOCKS ? n_groups : PF_MAX_NODE_BLOCKS;
  hipLaunchKernelGGL(k_group_sum, dim3(nb), dim3(256), 0, (hipStream_t)stream, n_elems, values, weights, group_ptr,
                     group_elems, n_groups, out);
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

int pf_gl_group_rhs(const pf_problem* p, const pf_gl* g, const int* elem_group, int g0, int m, double* out, void* stream) {
  const char* who = "pf_gl_group_rhs";
  if (!mesh_ok(p) || !p->mesh.adj_ptr || !p->mesh.adj || !p->mesh.dof_flags || p->mesh.n_nodes < 0 ||
      p->mesh.n_dofs != p->mesh.n_nodes * p->mesh.dim || !g || !g->fe || !elem_group || !out)
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (m < 1 || m > 65535) return gl_fail(PF_ERR_ARG, who, "bad group count (m)");
  if (g0 < 0 || g0 > INT_MAX - m) return gl_fail(PF_ERR_ARG, who, "bad first group (g0)");
  if (p->mesh.n_nodes == 0) return PF_OK;
  const dim3 grid(pf_node_blocks(p->mesh.n_nodes), m);
  const hipStream_t s = (hipStream_t)stream;
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_group_rhs<2>, grid, dim3(256), 0, s, *p, g->fe, elem_group, g0, out);
  else hipLaunchKernelGGL(k_gl_group_rhs<1>, grid, dim3(256), 0, s, *p, g->fe, elem_group, g0, out);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

int pf_gl_prestress_rhs(const pf_problem* p, const pf_gl* g, const double* ea, const double* u, const int* elem_group, int g0,
                        int m, double* out, void* stream) {
  const char* who = "pf_gl_prestress_rhs";
  if (!mesh_ok(p) || !p->mesh.conn || !p->mesh.adj_ptr || !p->mesh.adj || !p->mesh.dof_flags || p->mesh.n_nodes < 0 ||
      p->mesh.n_dofs != p->mesh.n_nodes * p->mesh.dim || !g || !g->d0 || !ea || !u || !elem_group || !out)
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (m < 1 || m > 65535) return gl_fail(PF_ERR_ARG, who, "bad group count (m)");
  if (g0 < 0 || g0 > INT_MAX - m) return gl_fail(PF_ERR_ARG, who, "bad first group (g0)");
  if (p->mesh.n_nodes == 0) return PF_OK;
  const dim3 grid(pf_node_blocks(p->mesh.n_nodes), m);
  const hipStream_t s = (hipStream_t)stream;
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_prestress_rhs<2>, grid, dim3(256), 0, s, *p, g->d0, ea, u, elem_group, g0, out);
  else hipLaunchKernelGGL(k_gl_prestress_rhs<1>, grid, dim3(256), 0, s, *p, g->d0, ea, u, elem_group, g0, out);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

int pf_gl_strain_rhs(const pf_problem* p, const pf_gl* g, const double* u, const double* coef, int accumulate, double* out,
                     void* stream) {
  const char* who = "pf_gl_strain_rhs";
  if (!mesh_ok(p) || !p->mesh.conn || !p->mesh.adj_ptr || !p->mesh.adj || !p->mesh.dof_flags || p->mesh.n_nodes < 0 ||
      p->mesh.n_dofs != p->mesh.n_nodes * p->mesh.dim || !g || !g->d0 || !u || !coef || !out ||
      (accumulate != 0 && accumulate != 1))
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_nodes == 0) return PF_OK;
  const int nb = pf_node_blocks(p->mesh.n_nodes);
  const hipStream_t s = (hipStream_t)stream;
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_strain_rhs<2>, dim3(nb), dim3(256), 0, s, *p, g->d0, u, coef, accumulate, out);
  else hipLaunchKernelGGL(k_gl_strain_rhs<1>, dim3(nb), dim3(256), 0, s, *p, g->d0, u, coef, accumulate, out);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

int pf_gl_strain_jvp(const pf_problem* p, const pf_gl* g, const double* u, const int* elems, int n_meas, const double* v,
                     int m, double* out, void* stream) {
  const char* who = "pf_gl_strain_jvp";
  if (!mesh_ok(p) || !p->mesh.conn || p->mesh.n_nodes < 0 || p->mesh.n_dofs != p->mesh.n_nodes * p->mesh.dim || !g ||
      !g->d0 || !u || !elems || !v || !out || n_meas < 0)
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (m < 1 || m > 65535) return gl_fail(PF_ERR_ARG, who, "bad row count (m)");
  if (n_meas == 0) return PF_OK;
  const dim3 grid(elem_blocks(n_meas), m);
  const hipStream_t s = (hipStream_t)stream;
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k_gl_strain_jvp<2>, grid, dim3(256), 0, s, *p, g->d0, u, elems, n_meas, v, out);
  else hipLaunchKernelGGL(k_gl_strain_jvp<1>, grid, dim3(256), 0, s, *p, g->d0, u, elems, n_meas, v, out);
  if (hipGetLastError() != hipSuccess) return gl_fail(PF_ERR_HIP, who, "HIP launch failed");
  return PF_OK;
}

}  // extern "C"
