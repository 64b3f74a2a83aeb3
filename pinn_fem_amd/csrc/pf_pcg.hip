// pf_pcg.hip — matrix-free K(E,A) v and a preconditioned conjugate-gradient solve in float64 (Jacobi, or opt-in two-level):
// the linear solve inside the classical Newton-Raphson solver for scalar materials
// (FEM/python/fem/solver.py:408-512: `du_f = np.linalg.solve(k_ff, rhs_f)` on the dense float64 tangent
// of fem/assembly.py:16-75; fem/element.py:45-102).  SURVEY.md §8(f) rank 3: the reference's dense solve
// stops at ~2*10^4 dofs; here K is never formed.  The preconditioner is diag(K_ff) — the "Jacobi/diagonal
// preconditioner" BASELINE.json's north-star names (the reference itself has none).
//
// Layout: every vector is double [n_dofs]; fixed dofs are carried as zeros (K_ff is K with the fixed rows
// and columns dropped).  The element stiffness is ((double)E*(double)A)/(double)l0 with E, A from the
// per-element property arrays when a net is enabled, else the scalar value.  Sums over a node's elements
// run in ascending element id (no atomics: the same owner-computes gather as pf_mesh.hip).
//
// The operator has a second form: with a non-null `kt` (double [n_elems][3] = B11, B12, B22; 1-D [n_elems]) the element
// block is read from it instead of being formed as s*(c2, cs, s2).  That is the tangent of the Green-Lagrange element
// (pf_nl.hip: pf_gl_state writes kt), served by the same kernels: pf_kt_v_f64, pf_pcgt_* and, with the two-level
// preconditioner, pf_coarse_setup_t and pf_pcg2t_*.  kt == NULL is the linear operator, arithmetic unchanged.
#include <stdio.h>
#include "pf_common.h"
#include "pf_graph.h"

namespace {

enum { ST_RZ = 0, ST_PAP, ST_RR, ST_BB, ST_ALPHA, ST_BETA, ST_DONE, ST_ITERS, ST_RTOL2, ST_RZ_NEW, ST_COUNT = 16 };

__device__ __forceinline__ double elem_s64(const pf_problem& P, int e, float l0) {
  return elem_ea64(P, e) / (double)l0;
}

// (K v)[node] and diag(K)[node] in one pass over the node's elements; kt != NULL: the element blocks are kt's (the same
// decision in every thread of the launch)
template <int DIM>
__device__ __forceinline__ void gather64(const pf_problem& P, const double* __restrict__ kt, const double* __restrict__ v,
                                         int node, double* kv, double* diag) {
  const pf_mesh& M = P.mesh;
#pragma unroll
  for (int c = 0; c < DIM; ++c) { kv[c] = 0.0; diag[c] = 0.0; }
  for (int idx = M.adj_ptr[node]; idx < M.adj_ptr[node + 1]; ++idx) {
    const int code = M.adj[idx];
    const int e = code >> 1, end = code & 1;
    const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
    const double sg = end ? -1.0 : 1.0;
    if (kt) {
      if (DIM == 2) {
        const double dx = v ? v[2 * nn.y] - v[2 * nn.x] : 0.0, dy = v ? v[2 * nn.y + 1] - v[2 * nn.x + 1] : 0.0;
        const double b11 = kt[3 * (size_t)e], b12 = kt[3 * (size_t)e + 1], b22 = kt[3 * (size_t)e + 2];
        kv[0] += -sg * (b11 * dx + b12 * dy);
        kv[1] += -sg * (b12 * dx + b22 * dy);
        diag[0] += b11;
        diag[1] += b22;
      } else {
        const double dx = v ? v[nn.y] - v[nn.x] : 0.0;
        kv[0] += -sg * (kt[e] * dx);
        diag[0] += kt[e];
      }
      continue;
    }
    const ElemGeo g = load_geo(M.egeo, e);
    const double s = elem_s64(P, e, g.l0);
    if (DIM == 2) {
      const double dx = v ? v[2 * nn.y] - v[2 * nn.x] : 0.0, dy = v ? v[2 * nn.y + 1] - v[2 * nn.x + 1] : 0.0;
      // rows of s*pattern @ [v_i; v_j] for this end: -(sg*s) * (c2*dx + cs*dy), -(sg*s) * (cs*dx + s2*dy)
      kv[0] += -(sg * s) * ((double)g.c2 * dx + (double)g.cs * dy);
      kv[1] += -(sg * s) * ((double)g.cs * dx + (double)g.s2 * dy);
      diag[0] += s * (double)g.c2;
      diag[1] += s * (double)g.s2;
    } else {
      const double dx = v ? v[nn.y] - v[nn.x] : 0.0;
      kv[0] += -(sg * s) * dx;
      diag[0] += s;
    }
  }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_kv64(pf_problem P, const double* __restrict__ kt, const double* __restrict__ v,
                                              double* __restrict__ out, int zero_fixed) {
  const pf_mesh& M = P.mesh;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    double kv[2], dg[2];
    gather64<DIM>(P, kt, v, node, kv, dg);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node * DIM + c;
      out[dof] = (zero_fixed && (M.dof_flags[dof] & PF_DOF_FIXED)) ? 0.0 : kv[c];
    }
  }
}

// out = diag(K_t) on the free dofs, 0.0 on the fixed ones: the dg that k_pcg_init inverts (gather64 with a null vector)
template <int DIM>
__global__ __launch_bounds__(256) void k_kt_diag64(pf_problem P, const double* __restrict__ kt, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    double kv[2], dg[2];
    gather64<DIM>(P, kt, nullptr, node, kv, dg);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node * DIM + c;
      out[dof] = (M.dof_flags[dof] & PF_DOF_FIXED) ? 0.0 : dg[c];
    }
  }
}

// ---- several right-hand sides per launch ----------------------------------------------------------------------------
// Every CG kernel below serves right-hand side k = blockIdx.y of a launch with grid (blocks, m): its b and x are rows k of
// [m][n_dofs] arrays (stride xs = n_dofs) and every part of its workspace lies wss doubles behind the same part of
// right-hand side 0 (wss = the family's workspace count, so state and partial sums are its own).  kt, the coarse space
// and a_inv are shared.  m = 1 (the four single families): blockIdx.y = 0 and every pointer is the caller's.
template <class T>
__device__ __forceinline__ T* rhs_of(T* base, long long stride) {
  return base + (size_t)blockIdx.y * (size_t)stride;
}

// x = 0, r = b (free dofs), dinv = 1/diag(K_ff), z = dinv*r, p = z; partials of r.z and b.b
template <int DIM>
__global__ __launch_bounds__(256) void k_pcg_init(pf_problem P, const double* __restrict__ kt, const double* __restrict__ b,
                                                  double* x, double* r, double* z, double* p, double* dinv, double* part,
                                                  long long wss) {
  __shared__ double red[8];
  const pf_mesh& M = P.mesh;
  b = rhs_of(b, M.n_dofs); x = rhs_of(x, M.n_dofs);
  r = rhs_of(r, wss); z = rhs_of(z, wss); p = rhs_of(p, wss); dinv = rhs_of(dinv, wss); part = rhs_of(part, wss);
  double rz = 0.0, bb = 0.0;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    double kv[2], dg[2];
    gather64<DIM>(P, kt, nullptr, node, kv, dg);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node * DIM + c;
      const bool fixed = M.dof_flags[dof] & PF_DOF_FIXED;
      const double bi = fixed ? 0.0 : b[dof];
      const double di = (fixed || dg[c] == 0.0) ? 0.0 : 1.0 / dg[c];
      x[dof] = 0.0; r[dof] = bi; dinv[dof] = di;
      const double zi = di * bi;
      z[dof] = zi; p[dof] = zi;
      rz += bi * zi; bb += bi * bi;
    }
  }
  const double t0 = pf_block_sum_d(rz, red), t1 = pf_block_sum_d(bb, red);
  if (threadIdx.x == 0) { part[blockIdx.x] = t0; part[PF_NODE_SLOTS + blockIdx.x] = t1; }
}

// ap = K p (fixed rows zero); partial p.ap
template <int DIM>
__global__ __launch_bounds__(256) void k_pcg_ap(pf_problem P, const double* __restrict__ kt, const double* __restrict__ st,
                                                const double* __restrict__ p, double* __restrict__ ap, double* part,
                                                long long wss) {
  st = rhs_of(st, wss);
  if (st[ST_DONE] != 0.0) return;
  p = rhs_of(p, wss); ap = rhs_of(ap, wss); part = rhs_of(part, wss);
  __shared__ double red[8];
  const pf_mesh& M = P.mesh;
  double pap = 0.0;
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < M.n_nodes; node += gridDim.x * blockDim.x) {
    double kv[2], dg[2];
    gather64<DIM>(P, kt, p, node, kv, dg);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node * DIM + c;
      const double a = (M.dof_flags[dof] & PF_DOF_FIXED) ? 0.0 : kv[c];
      ap[dof] = a;
      pap += p[dof] * a;
    }
  }
  const double t = pf_block_sum_d(pap, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one block: phase 0 (after init) rz, bb | phase 1 (after ap) pAp -> alpha | phase 2 (after update) rz_new, rr ->
// beta, stop test.  rtol2 is read in phase 0 only (it is stored in the state for the stop tests that follow)
__global__ __launch_bounds__(1024) void k_pcg_scalars(double* st, const double* __restrict__ part, int nb, int phase,
                                                      double rtol2, long long wss) {
  st = rhs_of(st, wss); part = rhs_of(part, wss);
  if (phase != 0 && st[ST_DONE] != 0.0) return;
  __shared__ double red[16];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) { a += part[i]; b += part[PF_NODE_SLOTS + i]; }
  const double ta = pf_block_sum_d(a, red), tb = pf_block_sum_d(b, red);
  if (threadIdx.x != 0) return;
  if (phase == 0) {
    st[ST_RZ] = ta; st[ST_BB] = tb; st[ST_RR] = tb; st[ST_ITERS] = 0.0; st[ST_RTOL2] = rtol2;
    st[ST_DONE] = (tb == 0.0) ? 1.0 : 0.0;        // b = 0: x = 0 is the solution
  } else if (phase == 1) {
    st[ST_PAP] = ta;
    st[ST_ALPHA] = ta != 0.0 ? st[ST_RZ] / ta : 0.0;
  } else {
    st[ST_BETA] = st[ST_RZ] != 0.0 ? ta / st[ST_RZ] : 0.0;
    st[ST_RZ] = ta; st[ST_RR] = tb; st[ST_ITERS] += 1.0;
    if (tb <= st[ST_RTOL2] * st[ST_BB] || ta == 0.0) st[ST_DONE] = 1.0;
  }
}

// x += alpha p; r -= alpha ap; z = dinv r; partials r.z, r.r
__global__ __launch_bounds__(256) void k_pcg_update(const double* __restrict__ st, int n, double* x, double* r, double* z,
                                                    const double* __restrict__ p, const double* __restrict__ ap,
                                                    const double* __restrict__ dinv, double* part, long long wss) {
  st = rhs_of(st, wss);
  if (st[ST_DONE] != 0.0) return;
  x = rhs_of(x, n); r = rhs_of(r, wss); z = rhs_of(z, wss); p = rhs_of(p, wss); ap = rhs_of(ap, wss);
  dinv = rhs_of(dinv, wss); part = rhs_of(part, wss);
  __shared__ double red[8];
  const double alpha = st[ST_ALPHA];
  double rz = 0.0, rr = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * ap[i];
    r[i] = ri;
    const double zi = dinv[i] * ri;
    z[i] = zi;
    rz += ri * zi; rr += ri * ri;
  }
  const double t0 = pf_block_sum_d(rz, red), t1 = pf_block_sum_d(rr, red);
  if (threadIdx.x == 0) { part[blockIdx.x] = t0; part[PF_NODE_SLOTS + blockIdx.x] = t1; }
}

// p = z + beta p
__global__ __launch_bounds__(256) void k_pcg_dir(const double* __restrict__ st, int n, const double* __restrict__ z, double* p,
                                                 long long wss) {
  st = rhs_of(st, wss);
  if (st[ST_DONE] != 0.0) return;
  z = rhs_of(z, wss); p = rhs_of(p, wss);
  const double beta = st[ST_BETA];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = z[i] + beta * p[i];
}

// ---- two-level preconditioner: M^-1 r = dinv r + Z (Z^T K Z)^-1 Z^T r -------------------------------------------------
// Z is held as per-dof coefficients: column agg_off[a] + k of Z has zcoef[dof][k] on the dofs of aggregate a's nodes and
// zeros elsewhere (pinnfem_hip.h: pf_coarse).  Every sum over an aggregate runs over its node list (ascending node
// id) strided over the block's threads and then through pf_block_sum_d: a fixed order, no atomics.

// columns of aggregate J at one node: the node's coefficient rows if it belongs to J, zeros otherwise
template <int DIM>
__device__ __forceinline__ void coarse_cols(const pf_coarse& C, int node, int J, double (*z)[PF_COARSE_MODES]) {
  const bool in = C.node_agg[node] == J;
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int k = 0; k < PF_COARSE_MODES; ++k)
      z[c][k] = in ? C.zcoef[((size_t)node * DIM + c) * PF_COARSE_MODES + k] : 0.0;
}

// (K z_j)[node] for the (up to 3) columns j of aggregate J: gather64 with z_j evaluated from the coefficients; kt != NULL:
// the element blocks are kt's, as in gather64 (the same decision in every thread of the launch)
template <int DIM>
__device__ __forceinline__ void gather_kz(const pf_problem& P, const double* __restrict__ kt, const pf_coarse& C, int J,
                                          int node, double (*kz)[PF_COARSE_MODES]) {
  const pf_mesh& M = P.mesh;
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int k = 0; k < PF_COARSE_MODES; ++k) kz[c][k] = 0.0;
  for (int idx = M.adj_ptr[node]; idx < M.adj_ptr[node + 1]; ++idx) {
    const int code = M.adj[idx];
    const int e = code >> 1, end = code & 1;
    const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
    const double sg = end ? -1.0 : 1.0;
    double zi[DIM][PF_COARSE_MODES], zj[DIM][PF_COARSE_MODES];
    coarse_cols<DIM>(C, nn.x, J, zi);
    coarse_cols<DIM>(C, nn.y, J, zj);
    if (kt) {
      if (DIM == 2) {
        const double b11 = kt[3 * (size_t)e], b12 = kt[3 * (size_t)e + 1], b22 = kt[3 * (size_t)e + 2];
#pragma unroll
        for (int k = 0; k < PF_COARSE_MODES; ++k) {
          const double dx = zj[0][k] - zi[0][k], dy = zj[1][k] - zi[1][k];
          kz[0][k] += -sg * (b11 * dx + b12 * dy);
          kz[1][k] += -sg * (b12 * dx + b22 * dy);
        }
      } else {
#pragma unroll
        for (int k = 0; k < PF_COARSE_MODES; ++k) kz[0][k] += -sg * (kt[e] * (zj[0][k] - zi[0][k]));
      }
      continue;
    }
    const ElemGeo g = load_geo(M.egeo, e);
    const double s = elem_s64(P, e, g.l0);
#pragma unroll
    for (int k = 0; k < PF_COARSE_MODES; ++k) {
      if (DIM == 2) {
        const double dx = zj[0][k] - zi[0][k], dy = zj[1][k] - zi[1][k];
        kz[0][k] += -(sg * s) * ((double)g.c2 * dx + (double)g.cs * dy);
        kz[1][k] += -(sg * s) * ((double)g.cs * dx + (double)g.s2 * dy);
      } else {
        kz[0][k] += -(sg * s) * (zj[0][k] - zi[0][k]);
      }
    }
  }
}

// A_c = Z^T K Z.  Block I owns the rows of aggregate I: entry (I,ki | J,kj) = sum over the nodes of I of
// z_(I,ki)[node] . (K z_(J,kj))[node], which is non-zero only when J is I or holds a neighbour of a node of I
// (nbr[] marks those).  The caller zeroed ac.  kt != NULL: K is the tangent K_t of those element blocks (pf_coarse_setup_t).
template <int DIM>
__global__ __launch_bounds__(256) void k_coarse_setup(pf_problem P, const double* __restrict__ kt, pf_coarse C,
                                                      double* __restrict__ ac) {
  __shared__ int nbr[PF_COARSE_MAX_AGG];
  __shared__ double red[8];
  const pf_mesh& M = P.mesh;
  const int I = blockIdx.x, lo = C.agg_ptr[I], hi = C.agg_ptr[I + 1];
  const int offI = C.agg_off[I], nI = C.agg_off[I + 1] - offI, nc = C.n_coarse;
  if (nI == 0) return;
  for (int t = threadIdx.x; t < C.n_agg; t += blockDim.x) nbr[t] = 0;
  __syncthreads();
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int node = C.agg_nodes[i];
    nbr[I] = 1;
    for (int idx = M.adj_ptr[node]; idx < M.adj_ptr[node + 1]; ++idx) {
      const int code = M.adj[idx];
      const int2 nn = reinterpret_cast<const int2*>(M.conn)[code >> 1];
      nbr[C.node_agg[(code & 1) ? nn.x : nn.y]] = 1;       // every writer stores the same value
    }
  }
  __syncthreads();
  for (int J = 0; J < C.n_agg; ++J) {
    const int offJ = C.agg_off[J], nJ = C.agg_off[J + 1] - offJ;
    if (!nbr[J] || nJ == 0) continue;                       // the same decision in every thread of the block
    double acc[PF_COARSE_MODES][PF_COARSE_MODES];
#pragma unroll
    for (int ki = 0; ki < PF_COARSE_MODES; ++ki)
#pragma unroll
      for (int kj = 0; kj < PF_COARSE_MODES; ++kj) acc[ki][kj] = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const int node = C.agg_nodes[i];
      double kz[DIM][PF_COARSE_MODES];
      gather_kz<DIM>(P, kt, C, J, node, kz);
#pragma unroll
      for (int c = 0; c < DIM; ++c)
#pragma unroll
        for (int ki = 0; ki < PF_COARSE_MODES; ++ki) {
          const double zi = C.zcoef[((size_t)node * DIM + c) * PF_COARSE_MODES + ki];
#pragma unroll
          for (int kj = 0; kj < PF_COARSE_MODES; ++kj) acc[ki][kj] += zi * kz[c][kj];
        }
    }
#pragma unroll
    for (int ki = 0; ki < PF_COARSE_MODES; ++ki)
#pragma unroll
      for (int kj = 0; kj < PF_COARSE_MODES; ++kj) {
        const double t = pf_block_sum_d(acc[ki][kj], red);
        if (threadIdx.x == 0 && ki < nI && kj < nJ) ac[(size_t)(offI + ki) * nc + offJ + kj] = t;
      }
  }
}

// one workgroup per aggregate (every node belongs to exactly one): x += alpha p, r -= alpha ap on its dofs (update != 0;
// pf_pcg2_begin restricts the r that k_pcg_init wrote), w = Z^T r for its columns, partial r.r
template <int DIM>
__global__ __launch_bounds__(256) void k_pcg2_restrict(pf_coarse C, const double* __restrict__ st, int update, double* x,
                                                       double* r, const double* __restrict__ p,
                                                       const double* __restrict__ ap, double* __restrict__ w, double* part,
                                                       long long xs, long long wss) {
  st = rhs_of(st, wss);
  if (st[ST_DONE] != 0.0) return;
  x = rhs_of(x, xs); r = rhs_of(r, wss); p = rhs_of(p, wss); ap = rhs_of(ap, wss); w = rhs_of(w, wss);
  part = rhs_of(part, wss);
  __shared__ double red[8];
  const int a = blockIdx.x, lo = C.agg_ptr[a], hi = C.agg_ptr[a + 1];
  const int off = C.agg_off[a], nk = C.agg_off[a + 1] - off;
  const double alpha = update ? st[ST_ALPHA] : 0.0;
  double acc[PF_COARSE_MODES] = {0.0, 0.0, 0.0}, rr = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int node = C.agg_nodes[i];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const size_t dof = (size_t)node * DIM + c;
      double ri = r[dof];
      if (update) {
        x[dof] += alpha * p[dof];
        ri -= alpha * ap[dof];
        r[dof] = ri;
      }
      rr += ri * ri;
#pragma unroll
      for (int k = 0; k < PF_COARSE_MODES; ++k) acc[k] += C.zcoef[dof * PF_COARSE_MODES + k] * ri;
    }
  }
#pragma unroll
  for (int k = 0; k < PF_COARSE_MODES; ++k) {
    const double t = pf_block_sum_d(acc[k], red);
    if (threadIdx.x == 0 && k < nk) w[off + k] = t;
  }
  const double t = pf_block_sum_d(rr, red);
  if (threadIdx.x == 0) part[PF_NODE_SLOTS + a] = t;
}

// one workgroup per aggregate: y = A^-1 w for the aggregate's columns (one row per wave, wave-wide reduction), then
// z = dinv r + Z y on its dofs and the partial r.z; p_init != NULL (pf_pcg2_begin): p = z as well
template <int DIM>
__global__ __launch_bounds__(256) void k_pcg2_apply(pf_coarse C, const double* __restrict__ st, const double* __restrict__ r,
                                                    const double* __restrict__ dinv, const double* __restrict__ w,
                                                    double* __restrict__ y, double* __restrict__ z, double* p_init,
                                                    double* part, long long wss) {
  st = rhs_of(st, wss);
  if (st[ST_DONE] != 0.0) return;
  r = rhs_of(r, wss); dinv = rhs_of(dinv, wss); w = rhs_of(w, wss); y = rhs_of(y, wss); z = rhs_of(z, wss);
  if (p_init) p_init = rhs_of(p_init, wss);                  // a null p_init stays null
  part = rhs_of(part, wss);
  __shared__ double red[8];
  __shared__ double ys[PF_COARSE_MODES];
  const int a = blockIdx.x, lo = C.agg_ptr[a], hi = C.agg_ptr[a + 1];
  const int off = C.agg_off[a], nk = C.agg_off[a + 1] - off, nc = C.n_coarse;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave < PF_COARSE_MODES) {
    double s = 0.0;
    if (wave < nk) {
      const double* __restrict__ row = C.a_inv + (size_t)(off + wave) * nc;
      for (int j = lane; j < nc; j += 64) s += row[j] * w[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      ys[wave] = s;                                         // 0.0 for a column the aggregate does not have
      if (wave < nk) y[off + wave] = s;
    }
  }
  __syncthreads();
  const double y0 = ys[0], y1 = ys[1], y2 = ys[2];
  double rz = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int node = C.agg_nodes[i];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const size_t dof = (size_t)node * DIM + c;
      const double* __restrict__ zc = C.zcoef + dof * PF_COARSE_MODES;
      const double ri = r[dof];
      const double zi = dinv[dof] * ri + (zc[0] * y0 + zc[1] * y1 + zc[2] * y2);
      z[dof] = zi;
      if (p_init) p_init[dof] = zi;
      rz += ri * zi;
    }
  }
  const double t = pf_block_sum_d(rz, red);
  if (threadIdx.x == 0) part[a] = t;
}

// r.z of the start (pf_pcg2_begin): k_pcg_scalars' phase 0 stored the Jacobi value
__global__ __launch_bounds__(256) void k_pcg2_rz0(double* st, const double* __restrict__ part, int nb, long long wss) {
  st = rhs_of(st, wss); part = rhs_of(part, wss);
  if (st[ST_DONE] != 0.0) return;
  __shared__ double red[8];
  double a = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) a += part[i];
  const double t = pf_block_sum_d(a, red);
  if (threadIdx.x == 0) st[ST_RZ] = t;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
// One implementation behind six exported families: pf_pcg_* (Jacobi), pf_pcg2_* (two-level), pf_pcgt_* (Jacobi on the
// tangent operator), pf_pcg2t_* (two-level on the tangent operator) and their forms for m right-hand sides per launch,
// pf_pcgtm_* and pf_pcg2tm_*, are argument checks in front of pcg_begin_impl / pcg_iterations_impl / pcg_graph_impl /
// pcg_state_impl, which take the coarse space as a nullable `c` (NULL = Jacobi), the tangent blocks as a nullable `kt`
// (NULL = the linear operator), the number of right-hand sides `m` (1 for the four single families: grid (blocks, 1)) and
// the exported function's name as `who`, the prefix of every error message.  The workspace layout is stated once, in pcg_layout; the iteration's launch sequence
// once, in pcg_enqueue; the CG graphs are captured by the library's capture_graph (pf_graph.h) as a single chain.
#define PCG_CHECK(who) \
  if (hipGetLastError() != hipSuccess) return pcg_fail(PF_ERR_HIP, who, "HIP launch failed");

// `launches` once for the mesh's dimension, with DIM a compile-time constant
#define PCG_FOR_DIM(p, launches)                                 \
  do {                                                           \
    if ((p)->mesh.dim == 2) { constexpr int DIM = 2; launches; } \
    else { constexpr int DIM = 1; launches; }                    \
  } while (0)

static int pcg_fail(int code, const char* who, const char* what) {
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  pf_set_error(buf);
  return code;
}

// The CG workspace, in doubles: r | z | p | ap | dinv (n_dofs each) | partials (2 * PF_NODE_SLOTS) | state (ST_COUNT) |
// w = Z^T r | y = A^-1 w (PF_COARSE_MAX each).  The Jacobi solve's workspace ends at w, the two-level solve's at end.
// T = double*: the parts of a workspace; T = long long: their offsets, i.e. the counts
template <class T>
struct PcgLayout { T r, z, p, ap, dinv, part, st, w, y, end; };
using PcgWs = PcgLayout<double*>;

template <class T>
static PcgLayout<T> pcg_layout(T base, int n_dofs) {
  const long long n = n_dofs;
  PcgLayout<T> L;
  L.r = base; L.z = L.r + n; L.p = L.z + n; L.ap = L.p + n; L.dinv = L.ap + n; L.part = L.dinv + n;
  L.st = L.part + 2 * PF_NODE_SLOTS; L.w = L.st + ST_COUNT; L.y = L.w + PF_COARSE_MAX; L.end = L.y + PF_COARSE_MAX;
  return L;
}

static long long pcg_ws_count(const pf_problem* p, bool two_level) {
  if (!p) return PF_ERR_ARG;
  const PcgLayout<long long> L = pcg_layout(0LL, p->mesh.n_dofs);
  return two_level ? L.end : L.w;
}

// doubles from one right-hand side's workspace to the next (the family's workspace count)
static long long pcg_ws_stride(const pf_problem* p, bool two_level) {
  const PcgLayout<long long> L = pcg_layout(0LL, p->mesh.n_dofs);
  return two_level ? L.end : L.w;
}

extern "C" {

static int kv_impl(const pf_problem* p, const double* kt, const double* v, double* out, int zero_fixed, hipStream_t s,
                   const char* who) {
  if (!p || !v || !out) return pcg_fail(PF_ERR_ARG, who, "null argument");
  const int nb = pf_node_blocks(p->mesh.n_nodes);
  PCG_FOR_DIM(p, hipLaunchKernelGGL(k_kv64<DIM>, dim3(nb), dim3(256), 0, s, *p, kt, v, out, zero_fixed));
  PCG_CHECK(who);
  return PF_OK;
}

static void pcg2_precondition(const pf_problem* p, const pf_coarse* c, int m, double* x, const PcgWs& L, int update,
                              double* p_init, hipStream_t s);   // (with the two-level preconditioner's own code, below)

// x = 0, r = b, dinv, |b|^2 and the b = 0 exit; two-level: then z = M^-1 r, p = z and r.z over the Jacobi start
static int pcg_begin_impl(const pf_problem* p, const pf_coarse* c, const double* kt, int m, const double* b, double* x,
                          double* ws, double rtol, hipStream_t s, const char* who) {
  if (!p || !b || !x || !ws || !(rtol >= 0.0)) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  const PcgWs L = pcg_layout(ws, p->mesh.n_dofs);
  const long long wss = pcg_ws_stride(p, c != nullptr);
  const int nb = pf_node_blocks(p->mesh.n_nodes);
  for (int k = 0; k < m; ++k)
    if (hipMemsetAsync(L.st + k * wss, 0, ((c ? L.end : L.w) - L.st) * sizeof(double), s) != hipSuccess)
      return pcg_fail(PF_ERR_HIP, who, "state setup failed");
  PCG_FOR_DIM(p, hipLaunchKernelGGL(k_pcg_init<DIM>, dim3(nb, m), dim3(256), 0, s, *p, kt, b, x, L.r, L.z, L.p, L.dinv,
                                    L.part, wss));
  PCG_CHECK(who);
  hipLaunchKernelGGL(k_pcg_scalars, dim3(1, m), dim3(1024), 0, s, L.st, L.part, nb, 0, rtol * rtol, wss);   // by value: no copy, no sync
  if (c) {
    pcg2_precondition(p, c, m, x, L, 0, L.p, s);
    hipLaunchKernelGGL(k_pcg2_rz0, dim3(1, m), dim3(256), 0, s, L.st, L.part, c->n_agg, wss);
  }
  PCG_CHECK(who);
  return PF_OK;
}

// n_iter CG iterations (no-ops once the stop test |r| <= rtol |b| fired).  The preconditioner step is k_pcg_update
// (one block per 256 dofs) or restrict + apply (one block per aggregate); phase 2 sums that step's partials.  Every launch
// carries the m right-hand sides in grid.y; one that has stopped returns at kernel entry and the others go on
static int pcg_enqueue(const pf_problem* p, const pf_coarse* c, const double* kt, int m, double* x, double* ws, int n_iter,
                       hipStream_t s, const char* who) {
  const int n = p->mesh.n_dofs, nb = pf_node_blocks(p->mesh.n_nodes);
  const PcgWs L = pcg_layout(ws, n);
  const long long wss = pcg_ws_stride(p, c != nullptr);
  int nbv = (n + 255) / 256;
  if (nbv > PF_MAX_NODE_BLOCKS) nbv = PF_MAX_NODE_BLOCKS;
  for (int it = 0; it < n_iter; ++it) {
    PCG_FOR_DIM(p, hipLaunchKernelGGL(k_pcg_ap<DIM>, dim3(nb, m), dim3(256), 0, s, *p, kt, L.st, L.p, L.ap, L.part, wss));
    hipLaunchKernelGGL(k_pcg_scalars, dim3(1, m), dim3(1024), 0, s, L.st, L.part, nb, 1, 0.0, wss);
    if (c) pcg2_precondition(p, c, m, x, L, 1, nullptr, s);
    else hipLaunchKernelGGL(k_pcg_update, dim3(nbv, m), dim3(256), 0, s, L.st, n, x, L.r, L.z, L.p, L.ap, L.dinv, L.part,
                            wss);
    hipLaunchKernelGGL(k_pcg_scalars, dim3(1, m), dim3(1024), 0, s, L.st, L.part, c ? c->n_agg : nbv, 2, 0.0, wss);
    hipLaunchKernelGGL(k_pcg_dir, dim3(nbv, m), dim3(256), 0, s, L.st, n, L.z, L.p, wss);
  }
  PCG_CHECK(who);
  return PF_OK;
}

// [iterations, stopped, |r|^2, |b|^2] of the running solve, one row per right-hand side (synchronises the stream once)
static int pcg_state_impl(const pf_problem* p, bool two_level, int m, double* ws, double* state_out, hipStream_t s,
                          const char* who) {
  if (!p || !ws || !state_out) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  double h[PF_PCG_MAX_RHS][ST_COUNT];
  const double* st = pcg_layout(ws, p->mesh.n_dofs).st;
  const long long wss = pcg_ws_stride(p, two_level);
  for (int k = 0; k < m; ++k)
    if (hipMemcpyAsync(h[k], st + k * wss, sizeof(h[k]), hipMemcpyDeviceToHost, s) != hipSuccess)
      return pcg_fail(PF_ERR_HIP, who, "state read-back failed");
  if (hipStreamSynchronize(s) != hipSuccess) return pcg_fail(PF_ERR_HIP, who, "state read-back failed");
  for (int k = 0; k < m; ++k) {
    double* o = state_out + 4 * k;
    o[0] = h[k][ST_ITERS]; o[1] = h[k][ST_DONE]; o[2] = h[k][ST_RR]; o[3] = h[k][ST_BB];
  }
  return PF_OK;
}

// state_out (host, may be NULL) receives the state after a stream synchronisation
static int pcg_iterations_impl(const pf_problem* p, const pf_coarse* c, const double* kt, int m, double* x, double* ws,
                               int n_iter, double* state_out, hipStream_t s, const char* who) {
  if (!p || !x || !ws || n_iter < 0) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  const int rc = pcg_enqueue(p, c, kt, m, x, ws, n_iter, s, who);
  if (rc != PF_OK) return rc;
  return state_out ? pcg_state_impl(p, c != nullptr, m, ws, state_out, s, who) : PF_OK;
}

// the same n_iter iterations as ONE hipGraph (record and pointers baked in; handle for pf_graph_launch /
// pf_graph_destroy): 5 or 6 tiny launches per CG iteration are launch bound when issued one by one.  A single chain of
// kernel nodes, no parallel branches: no events, no side stream
static int pcg_graph_impl(const pf_problem* p, const pf_coarse* c, const double* kt, int m, double* x, double* ws, int n_iter,
                          hipStream_t s, void** graph_out, const char* who) {
  if (!p || !x || !ws || n_iter < 1 || !graph_out) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  return capture_graph(s, 0, hipStreamCaptureModeThreadLocal, graph_out,
                       [&](pf_capture& cap) { return pcg_enqueue(p, c, kt, m, x, ws, n_iter, cap.s, who); });
}

// ---- the two-level preconditioner's own code ----------------------------------------------------------------------
static bool coarse_ok(const pf_coarse* c, bool need_inverse) {
  return c && c->n_agg >= 1 && c->n_agg <= PF_COARSE_MAX_AGG && c->n_coarse >= 0 &&
         c->n_coarse <= PF_COARSE_MODES * c->n_agg && c->node_agg && c->agg_off && c->zcoef && c->agg_ptr &&
         c->agg_nodes && (!need_inverse || c->a_inv);
}

// A_c = Z^T K Z, K the linear operator (kt == NULL) or the tangent of the element blocks kt
static int coarse_setup_impl(const pf_problem* p, const pf_coarse* c, const double* kt, double* a_c_out, hipStream_t s,
                             const char* who) {
  if (!p || !coarse_ok(c, false) || !a_c_out) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  if (c->n_coarse == 0) return PF_OK;
  if (hipMemsetAsync(a_c_out, 0, (size_t)c->n_coarse * c->n_coarse * sizeof(double), s) != hipSuccess)
    return pcg_fail(PF_ERR_HIP, who, "clearing the coarse matrix failed");
  PCG_FOR_DIM(p, hipLaunchKernelGGL(k_coarse_setup<DIM>, dim3(c->n_agg), dim3(256), 0, s, *p, kt, *c, a_c_out));
  PCG_CHECK(who);
  return PF_OK;
}

// z = M^-1 r and r.z for the r in the workspace: restriction, then coarse solve + prolongation (two launches)
static void pcg2_precondition(const pf_problem* p, const pf_coarse* c, int m, double* x, const PcgWs& L, int update,
                              double* p_init, hipStream_t s) {
  const long long xs = p->mesh.n_dofs, wss = pcg_ws_stride(p, true);
  PCG_FOR_DIM(p, hipLaunchKernelGGL(k_pcg2_restrict<DIM>, dim3(c->n_agg, m), dim3(256), 0, s, *c, L.st, update, x, L.r, L.p,
                                    L.ap, L.w, L.part, xs, wss);
              hipLaunchKernelGGL(k_pcg2_apply<DIM>, dim3(c->n_agg, m), dim3(256), 0, s, *c, L.st, L.r, L.dinv, L.w, L.y, L.z,
                                 p_init, L.part, wss));
}

// ---- the exported families -----------------------------------------------------------------------------------------
// pf_pcgt_*, pf_pcg2t_*, pf_coarse_setup_t: a null kt is an error here, never a silent linear solve
#define PCGT_NEED_KT(who) \
  if (!kt) return pcg_fail(PF_ERR_ARG, who, "null tangent (kt)");
// pf_pcg2t_*: nor does a null or inconsistent coarse space become a silent Jacobi solve
#define PCG2T_NEED(who)                                                         \
  PCGT_NEED_KT(who);                                                            \
  if (!coarse_ok(c, true)) return pcg_fail(PF_ERR_ARG, who, "bad coarse space");

int pf_coarse_setup(const pf_problem* p, const pf_coarse* c, double* a_c_out, void* stream) {
  return coarse_setup_impl(p, c, nullptr, a_c_out, (hipStream_t)stream, "pf_coarse_setup");
}
int pf_coarse_setup_t(const pf_problem* p, const pf_coarse* c, const double* kt, double* a_c_out, void* stream) {
  PCGT_NEED_KT("pf_coarse_setup_t");
  return coarse_setup_impl(p, c, kt, a_c_out, (hipStream_t)stream, "pf_coarse_setup_t");
}

long long pf_pcg_workspace_count(const pf_problem* p) { return pcg_ws_count(p, false); }
long long pf_pcg2_workspace_count(const pf_problem* p) { return pcg_ws_count(p, true); }

int pf_kv_f64(const pf_problem* p, const double* v, double* out, int zero_fixed, void* stream) {
  return kv_impl(p, nullptr, v, out, zero_fixed, (hipStream_t)stream, "pf_kv_f64");
}
int pf_kt_v_f64(const pf_problem* p, const double* kt, const double* v, double* out, int zero_fixed, void* stream) {
  PCGT_NEED_KT("pf_kt_v_f64");
  return kv_impl(p, kt, v, out, zero_fixed, (hipStream_t)stream, "pf_kt_v_f64");
}
int pf_kt_diag_f64(const pf_problem* p, const double* kt, double* out, void* stream) {
  const char* who = "pf_kt_diag_f64";
  PCGT_NEED_KT(who);
  if (!p || !out) return pcg_fail(PF_ERR_ARG, who, "null argument");
  const int nb = pf_node_blocks(p->mesh.n_nodes);
  PCG_FOR_DIM(p, hipLaunchKernelGGL(k_kt_diag64<DIM>, dim3(nb), dim3(256), 0, (hipStream_t)stream, *p, kt, out));
  PCG_CHECK(who);
  return PF_OK;
}

int pf_pcg_begin(const pf_problem* p, const double* b, double* x, double* ws, double rtol, void* stream) {
  return pcg_begin_impl(p, nullptr, nullptr, 1, b, x, ws, rtol, (hipStream_t)stream, "pf_pcg_begin");
}
int pf_pcg2_begin(const pf_problem* p, const pf_coarse* c, const double* b, double* x, double* ws, double rtol,
                  void* stream) {
  const char* who = "pf_pcg2_begin";
  if (!coarse_ok(c, true)) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  return pcg_begin_impl(p, c, nullptr, 1, b, x, ws, rtol, (hipStream_t)stream, who);
}
int pf_pcgt_begin(const pf_problem* p, const double* kt, const double* b, double* x, double* ws, double rtol,
                  void* stream) {
  PCGT_NEED_KT("pf_pcgt_begin");
  return pcg_begin_impl(p, nullptr, kt, 1, b, x, ws, rtol, (hipStream_t)stream, "pf_pcgt_begin");
}

int pf_pcg2t_begin(const pf_problem* p, const pf_coarse* c, const double* kt, const double* b, double* x, double* ws,
                   double rtol, void* stream) {
  PCG2T_NEED("pf_pcg2t_begin");
  return pcg_begin_impl(p, c, kt, 1, b, x, ws, rtol, (hipStream_t)stream, "pf_pcg2t_begin");
}

int pf_pcg_iterations(const pf_problem* p, double* x, double* ws, int n_iter, double* state_out, void* stream) {
  return pcg_iterations_impl(p, nullptr, nullptr, 1, x, ws, n_iter, state_out, (hipStream_t)stream, "pf_pcg_iterations");
}
int pf_pcg2_iterations(const pf_problem* p, const pf_coarse* c, double* x, double* ws, int n_iter, double* state_out,
                       void* stream) {
  const char* who = "pf_pcg2_iterations";
  if (!coarse_ok(c, true)) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  return pcg_iterations_impl(p, c, nullptr, 1, x, ws, n_iter, state_out, (hipStream_t)stream, who);
}
int pf_pcgt_iterations(const pf_problem* p, const double* kt, double* x, double* ws, int n_iter, double* state_out,
                       void* stream) {
  PCGT_NEED_KT("pf_pcgt_iterations");
  return pcg_iterations_impl(p, nullptr, kt, 1, x, ws, n_iter, state_out, (hipStream_t)stream, "pf_pcgt_iterations");
}

int pf_pcg2t_iterations(const pf_problem* p, const pf_coarse* c, const double* kt, double* x, double* ws, int n_iter,
                        double* state_out, void* stream) {
  PCG2T_NEED("pf_pcg2t_iterations");
  return pcg_iterations_impl(p, c, kt, 1, x, ws, n_iter, state_out, (hipStream_t)stream, "pf_pcg2t_iterations");
}

int pf_pcg_graph_create(const pf_problem* p, double* x, double* ws, int n_iter, void* stream, void** graph_out) {
  return pcg_graph_impl(p, nullptr, nullptr, 1, x, ws, n_iter, (hipStream_t)stream, graph_out, "pf_pcg_graph_create");
}
int pf_pcg2_graph_create(const pf_problem* p, const pf_coarse* c, double* x, double* ws, int n_iter, void* stream,
                         void** graph_out) {
  const char* who = "pf_pcg2_graph_create";
  if (!coarse_ok(c, true)) return pcg_fail(PF_ERR_ARG, who, "bad argument");
  return pcg_graph_impl(p, c, nullptr, 1, x, ws, n_iter, (hipStream_t)stream, graph_out, who);
}
int pf_pcgt_graph_create(const pf_problem* p, const double* kt, double* x, double* ws, int n_iter, void* stream,
                         void** graph_out) {
  PCGT_NEED_KT("pf_pcgt_graph_create");
  return pcg_graph_impl(p, nullptr, kt, 1, x, ws, n_iter, (hipStream_t)stream, graph_out, "pf_pcgt_graph_create");
}

int pf_pcg2t_graph_create(const pf_problem* p, const pf_coarse* c, const double* kt, double* x, double* ws, int n_iter,
                          void* stream, void** graph_out) {
  PCG2T_NEED("pf_pcg2t_graph_create");
  return pcg_graph_impl(p, c, kt, 1, x, ws, n_iter, (hipStream_t)stream, graph_out, "pf_pcg2t_graph_create");
}

int pf_pcg_state(const pf_problem* p, double* ws, double* state_out, void* stream) {
  return pcg_state_impl(p, false, 1, ws, state_out, (hipStream_t)stream, "pf_pcg_state");
}
int pf_pcg2_state(const pf_problem* p, double* ws, double* state_out, void* stream) {
  return pcg_state_impl(p, true, 1, ws, state_out, (hipStream_t)stream, "pf_pcg2_state");
}
int pf_pcgt_state(const pf_problem* p, const double* kt, double* ws, double* state_out, void* stream) {
  PCGT_NEED_KT("pf_pcgt_state");
  return pcg_state_impl(p, false, 1, ws, state_out, (hipStream_t)stream, "pf_pcgt_state");
}
int pf_pcg2t_state(const pf_problem* p, const double* kt, double* ws, double* state_out, void* stream) {
  PCGT_NEED_KT("pf_pcg2t_state");
  return pcg_state_impl(p, true, 1, ws, state_out, (hipStream_t)stream, "pf_pcg2t_state");
}

// ---- m right-hand sides per launch on the tangent: pf_pcgtm_* (Jacobi), pf_pcg2tm_* (two-level) -----------------------
// b and x are [m][n_dofs], ws is m workspaces of the family's count, state_out is [m][4]
#define PCGTM_NEED(who)                                                                                \
  PCGT_NEED_KT(who);                                                                                   \
  if (m < 1 || m > PF_PCG_MAX_RHS) return pcg_fail(PF_ERR_ARG, who, "bad right-hand-side count (m)");
#define PCG2TM_NEED(who)                                                        \
  PCGTM_NEED(who);                                                              \
  if (!coarse_ok(c, true)) return pcg_fail(PF_ERR_ARG, who, "bad coarse space");

int pf_pcgtm_begin(const pf_problem* p, const double* kt, int m, const double* b, double* x, double* ws, double rtol,
                   void* stream) {
  PCGTM_NEED("pf_pcgtm_begin");
  return pcg_begin_impl(p, nullptr, kt, m, b, x, ws, rtol, (hipStream_t)stream, "pf_pcgtm_begin");
}
int pf_pcgtm_iterations(const pf_problem* p, const double* kt, int m, double* x, double* ws, int n_iter, double* state_out,
                        void* stream) {
  PCGTM_NEED("pf_pcgtm_iterations");
  return pcg_iterations_impl(p, nullptr, kt, m, x, ws, n_iter, state_out, (hipStream_t)stream, "pf_pcgtm_iterations");
}
int pf_pcgtm_graph_create(const pf_problem* p, const double* kt, int m, double* x, double* ws, int n_iter, void* stream,
                          void** graph_out) {
  PCGTM_NEED("pf_pcgtm_graph_create");
  return pcg_graph_impl(p, nullptr, kt, m, x, ws, n_iter, (hipStream_t)stream, graph_out, "pf_pcgtm_graph_create");
}
int pf_pcgtm_state(const pf_problem* p, const double* kt, int m, double* ws, double* state_out, void* stream) {
  PCGTM_NEED("pf_pcgtm_state");
  return pcg_state_impl(p, false, m, ws, state_out, (hipStream_t)stream, "pf_pcgtm_state");
}

int pf_pcg2tm_begin(const pf_problem* p, const pf_coarse* c, const double* kt, int m, const double* b, double* x, double* ws,
                    double rtol, void* stream) {
  PCG2TM_NEED("pf_pcg2tm_begin");
  return pcg_begin_impl(p, c, kt, m, b, x, ws, rtol, (hipStream_t)stream, "pf_pcg2tm_begin");
}
int pf_pcg2tm_iterations(const pf_problem* p, const pf_coarse* c, const double* kt, int m, double* x, double* ws, int n_iter,
                         double* state_out, void* stream) {
  PCG2TM_NEED("pf_pcg2tm_iterations");
  return pcg_iterations_impl(p, c, kt, m, x, ws, n_iter, state_out, (hipStream_t)stream, "pf_pcg2tm_iterations");
}
int pf_pcg2tm_graph_create(const pf_problem* p, const pf_coarse* c, const double* kt, int m, double* x, double* ws, int n_iter,
                           void* stream, void** graph_out) {
  PCG2TM_NEED("pf_pcg2tm_graph_create");
  return pcg_graph_impl(p, c, kt, m, x, ws, n_iter, (hipStream_t)stream, graph_out, "pf_pcg2tm_graph_create");
}
int pf_pcg2tm_state(const pf_problem* p, const double* kt, int m, double* ws, double* state_out, void* stream) {
  PCGTM_NEED("pf_pcg2tm_state");
  return pcg_state_impl(p, true, m, ws, state_out, (hipStream_t)stream, "pf_pcg2tm_state");
}

}  // extern "C"
