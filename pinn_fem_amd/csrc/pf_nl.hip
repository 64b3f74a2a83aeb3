// pf_nl.hip — the geometrically nonlinear (total-Lagrangian, Green-Lagrange strain) truss element in float64: element state
// and internal force for the Newton-Raphson solve on large displacements, and the derivatives the identification of
// E*A factors and initial strains reads.
//
// Per element with nodes i, j:  d0 = X_j - X_i (float64, from the caller: pf_gl.d0),  du = u_j - u_i,  d = d0 + du,
//   e  = (2 d0.du + du.du) / (2 l0^2)          the difference of squares written out: (l^2 - l0^2) cancels at small strain
//   N  = E*A * (e - e0)                        E*A as pf_pcg.hip forms it (elem_ea64) or the caller's per-element array;
//                                              e0 an initial strain (prestress, thermal, lack of fit) or absent
//   fe = (N / l0) d                            f_int[j] += fe, f_int[i] -= fe
//   B  = (E*A / l0^3) d d^T + (N / l0) I       K_t v: row j += B (v_j - v_i), row i -= B (v_j - v_i)
// B is what pf_pcg.hip's gather64 reads as `kt`.  The reference's truss2d_element_state (fem/element.py:105-133) is NOT
// this element: its force has the other sign and lacks 1/l0, and its "nonlinear" stiffness is e d d^T, not (N/l0) I.
//
// Two pieces are stated once.  load_gl_geo reads an element's conn, d0 and the two gathered u and returns its nodes, d0 and du;
// node_gather sums a per-incidence term over a node's elements, one node per thread, in ascending incidence order and
// without atomics, and hands each dof's sum to the kernel's store.
//
// Element kernels, one element (or gauge) per thread, grid-stride:
//   k_gl_state       strain, fe and B records out.  ea and e0 are nullable, the same decision in every thread; e - e0[e]
//                    is formed once, after e, and takes e's place in N; the strain written out stays e.
//                    The <DIM, true, gl_cable_set> instantiations apply the tension-only rule of the dynamics (below) to
//                    N / l0 and E*A / l0^3 by a select, keep the slack set (in/out) and write per-block partials of the
//                    number of slack elements and of changed flags; k_gl_cable_counts adds them in one block.
//                    The <DIM, false, gl_plastic_set> instantiations are the elastoplastic element: 1-D
//                    rate-independent plasticity with linear isotropic hardening in e and its conjugate force.  The
//                    return map (gl_return_map) starts from the committed (ep_n, al_n) of the caller, never from a
//                    previous iterate, and writes the trial (ep, al) to buffers of their own; N = E*A s with s the
//                    elastic part of e - e0, and B takes E*A kappa / (1 + kappa) in its material term where the element
//                    is plastic: the consistent tangent, since the map is exact.  Flags and counts as the cable's.
//   k_gl_sens        dJ/d(E*A) from the state u and an adjoint a: -((e - e0) / l0) d.(a_j - a_i); may accumulate.
//   k_gl_strain_jvp  (d_e / l0^2).(v_j - v_i) at the measured elements, the row of v in blockIdx.y; an element id outside
//                    the mesh writes 0.0 and reads nothing.
// Node kernels, node_gather with a term and a store:
//   k_gl_fint           +-fe (fe_term): the internal force.
//   k_gl_group_rhs      fe_term over the elements of group g0 + blockIdx.y, negated: the right-hand side of
//                       K_t s = -d f_int / d q_g (f_int is linear in E*A).  Fixed dofs get 0.0.
//   k_gl_prestress_rhs  +-(ea_e / l0) d_e (geo_term) over such a group: the right-hand side of K_t s = -d f_int / d t_h
//                       for an additive initial strain t_h (f_int is affine in e0).  Fixed dofs get 0.0.
//   k_gl_strain_rhs     +-(c_e / l0^2) d_e (geo_term): B^T c, the adjoint right-hand side of a strain misfit.  Fixed dofs
//                       get 0.0, or stay untouched when it accumulates.
// k_group_sum: out[g] = sum of values[e] * weights[e] over the elements of group g (CSR, ascending element id): one
//   workgroup per group, thread t adds elements t, t + 256, ... in that order, then pf_block_sum_d.  No atomics.
// Explicit dynamics (central differences, lumped mass, mass-proportional damping):
//   k_gl_dyn_step       node_gather with +-(ea (e - e0) / l0) d formed from d0 and u (dyn_term), the store advancing the
//                       node's own v (in place) and u (into the other of two buffers): one launch per time step.
//   k_gl_dyn_clock      adds a sequence's length to the step number on the device, so that a captured sequence replays.
//   k_gl_dyn_energy     per-block partials of the kinetic and strain energy, f_ext.u and max |v|; k_gl_dyn_energy_sum adds
//                       them in one block.  pf_block_sum_d, a fixed order, no atomics.
//   Tension-only (cable) elements: the <DIM, true> instantiations of the step and of the energy kernel read one flag per
//   element, and a flagged element with e - e0 < 0 is slack: N = 0 by a select on the value, so it adds +-0.0 in its place
//   in the incidence order, no strain energy, and 1 to a fifth partial, the slack count.  The <DIM, false> instantiations
//   are the bar kernels, untouched: the flag is a template parameter, and their trailing operand is never read.
//   Time histories: the <DIM, CABLE, pf_dyn_hist> instantiations of the step read the load factor and the support-motion scale of
//   their step from arrays the host sampled at the step times (pf_dyn_hist), by the step number of the device clock: two
//   launch-uniform loads, no search, and a replayed graph reads the samples of the steps it then stands at.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <type_traits>
#include "pf_common.h"
#include "pf_graph.h"

namespace {

// out = v[nj] - v[ni], a node vector's difference along an element
template <int DIM>
__device__ __forceinline__ void node_diff(const double* v, int ni, int nj, double* out) {
  if (DIM == 2) {
    const double2 vi = reinterpret_cast<const double2*>(v)[ni], vj = reinterpret_cast<const double2*>(v)[nj];
    out[0] = vj.x - vi.x; out[DIM - 1] = vj.y - vi.y;
  } else {
    out[0] = v[nj] - v[ni];
  }
}

// the element's geometry: its nodes ni and nj, d0 = X_j - X_i and du = u_j - u_i
template <int DIM>
__device__ __forceinline__ void load_gl_geo(const pf_mesh& M, const double* d0_in, const double* u, int e, int& ni, int& nj,
                                            double* d0, double* du) {
  const int2 nn = reinterpret_cast<const int2*>(M.conn)[e];
  ni = nn.x; nj = nn.y;
  if (DIM == 2) {
    const double2 a = reinterpret_cast<const double2*>(d0_in)[e];
    d0[0] = a.x; d0[DIM - 1] = a.y;
  } else {
    d0[0] = d0_in[e];
  }
  node_diff<DIM>(u, ni, nj, du);
}

// what the CABLE instantiations of k_gl_state read and write beside the bar's operands
struct gl_cable_set {
  const unsigned char* __restrict__ cable;   // [n_elems] the tension-only flags
  unsigned char* __restrict__ slack;         // [n_elems] in: the previous call's set; out: this call's (1 = slack)
  double* __restrict__ part;                 // [gridDim.x][2] out: the block's slack elements and changed flags
};

// what the <DIM, false, gl_plastic_set> instantiations of k_gl_state read and write beside the bar's operands: pf_gl_plastic's
// arrays, and the block partials behind its counts
struct gl_plastic_set {
  const double* __restrict__ ey;             // [n_elems] yield strain, +inf = never yields
  const double* __restrict__ kappa;          // [n_elems] hardening ratio H / E
  const double* __restrict__ ep_n;           // [n_elems] committed plastic strain
  const double* __restrict__ al_n;           // [n_elems] committed accumulated plastic strain
  double* __restrict__ ep;                   // [n_elems] out: the trial plastic strain (never ep_n: the host refuses it)
  double* __restrict__ al;                   // [n_elems] out: the trial accumulated plastic strain
  unsigned char* __restrict__ yielding;      // [n_elems] in: the previous call's flags; out: this call's (1 = plastic)
  double* __restrict__ part;                 // [gridDim.x][2] out: the block's plastic elements and changed flags
};

// The return map of 1-D plasticity with linear isotropic hardening from the committed (ep_n, al_n), exact for it:
//   tr = se - ep_n,  r = ey + kappa al_n,  f = |tr| - r,  plastic <=> f > 2^-40 r,  dg = f / (1 + kappa),
//   (ep, al) = (ep_n + dg sign(tr), al_n + dg),  s = tr - dg sign(tr),  E*A_t = E*A kappa / (1 + kappa),
// each a select on the value, so an element that is not plastic gets tr, E*A, ep_n and al_n back to the bit.  Every
// operation is rounded on its own (no contraction): the branch an element takes is the one the host's float64 takes.
// Returns whether the element is plastic.
__device__ __forceinline__ bool gl_return_map(double se, double ea, double ey, double kappa, double ep_n, double al_n,
                                              double& s, double& ea_t, double& ep, double& al) {
#pragma clang fp contract(off)
  const double tr = se - ep_n;
  const double r = ey + kappa * al_n;
  const double f = fabs(tr) - r;
  const bool plastic = f > 0x1p-40 * r;
  const double dg = f / (1.0 + kappa);
  const double step = tr < 0.0 ? -dg : dg;
  s = plastic ? tr - step : tr;
  ea_t = plastic ? ea * kappa / (1.0 + kappa) : ea;
  ep = plastic ? ep_n + step : ep_n;
  al = plastic ? al_n + dg : al_n;
  return plastic;
}

// CABLE: an element with cable[e] != 0 and e - e0 < 0 is slack (the rule of dyn_term): it carries no N and no E*A, by a
// select on the value, so its fe and kt are +0.0 and its strain stays e; every other element keeps the bar's values.
// SET: empty, or gl_cable_set (CABLE) or gl_plastic_set (not CABLE) and one more operand.  With gl_plastic_set the strain that
// carries stress and the E*A of the material term go through gl_return_map; the <DIM, false> instantiations are the bar
// kernels, untouched: there `s` and `ea_t` are se and ea themselves.
template <int DIM, bool CABLE, class... SET>
__global__ __launch_bounds__(256) void k_gl_state(pf_problem P, pf_gl G, const double* __restrict__ u,
                                                  const double* __restrict__ ea_in, const double* __restrict__ e0_in,
                                                  SET... set) {
  constexpr bool PLASTIC = (std::is_same_v<SET, gl_plastic_set> || ...);
  static_assert(!(CABLE && PLASTIC), "a cable set or a plastic set, not both");
  const pf_mesh& M = P.mesh;
  [[maybe_unused]] double n_set = 0.0, n_changed = 0.0;     // the slack (or plastic) elements, the changed flags
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < M.n_elems; e += gridDim.x * blockDim.x) {
    int ni, nj;
    double d0[DIM], du[DIM];
    load_gl_geo<DIM>(M, G.d0, u, e, ni, nj, d0, du);
    const double ea = ea_in ? ea_in[e] : elem_ea64(P, e);
    double l02 = 0.0, d0du = 0.0, dudu = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) { l02 += d0[c] * d0[c]; d0du += d0[c] * du[c]; dudu += du[c] * du[c]; }
    const double l0 = sqrt(l02);
    const double strain = (2.0 * d0du + dudu) / (2.0 * l02);
    const double se = e0_in ? strain - e0_in[e] : strain;     // the strain that carries stress; e - 0.0 is e to the bit
    double s = se, ea_t = ea;                        // PLASTIC: the elastic part of se and the tangent modulus
    if constexpr (PLASTIC) {
      const gl_plastic_set& S = (set, ...);
      double ep, al;
      const bool plastic = gl_return_map(se, ea, S.ey[e], S.kappa[e], S.ep_n[e], S.al_n[e], s, ea_t, ep, al);
      S.ep[e] = ep; S.al[e] = al;
      n_set += plastic ? 1.0 : 0.0;
      n_changed += (S.yielding[e] != 0) != plastic ? 1.0 : 0.0;
      S.yielding[e] = plastic ? 1 : 0;
    }
    const double n_l0 = (ea * s) / l0;               // N / l0
    const double k = ea_t / (l02 * l0);              // E*A / l0^3 (PLASTIC: E*A_t / l0^3)
    double d[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) d[c] = d0[c] + du[c];
    // CABLE selects +0.0 for every value a slack element stores (on the stored values: 0.0 for N / l0 and E*A / l0^3 alone
    // would leave them the signs of d); the bar's `put` is the identity
    [[maybe_unused]] bool slack = false;
    if constexpr (CABLE) {
      const gl_cable_set& S = (set, ...);
      slack = S.cable[e] && se < 0.0;
      n_set += slack ? 1.0 : 0.0;
      n_changed += (S.slack[e] != 0) != slack ? 1.0 : 0.0;
      S.slack[e] = slack ? 1 : 0;
    }
    const auto put = [&](double x) { return CABLE && slack ? 0.0 : x; };
    G.strain[e] = strain;
    if (DIM == 2) {
      reinterpret_cast<double2*>(G.fe)[e] = make_double2(put(n_l0 * d[0]), put(n_l0 * d[DIM - 1]));
      double* __restrict__ b = G.kt + 3 * (size_t)e;
      b[0] = put(k * (d[0] * d[0]) + n_l0);
      b[1] = put(k * (d[0] * d[DIM - 1]));
      b[2] = put(k * (d[DIM - 1] * d[DIM - 1]) + n_l0);
    } else {
      G.fe[e] = put(n_l0 * d[0]);
      G.kt[e] = put(k * (d[0] * d[0]) + n_l0);
    }
  }
  if constexpr (CABLE || PLASTIC) {
    __shared__ double red[8];
    const auto& S = (set, ...);
    const double s0 = pf_block_sum_d(n_set, red), s1 = pf_block_sum_d(n_changed, red);     // exact integers
    if (threadIdx.x == 0) { S.part[2 * (size_t)blockIdx.x] = s0; S.part[2 * (size_t)blockIdx.x + 1] = s1; }
  }
}

// counts[0..1] = the sums of the nb block partials behind them (counts + 2), thread t adding blocks t, t + 256, ... in that
// order: k_gl_dyn_energy_sum's pattern
__global__ __launch_bounds__(256) void k_gl_cable_counts(double* __restrict__ counts, int nb) {
  __shared__ double red[8];
  const double* __restrict__ part = counts + 2;
  double a0 = 0.0, a1 = 0.0;
  for (int b = (int)threadIdx.x; b < nb; b += (int)blockDim.x) { a0 += part[2 * b]; a1 += part[2 * b + 1]; }
  const double s0 = pf_block_sum_d(a0, red), s1 = pf_block_sum_d(a1, red);
  if (threadIdx.x == 0) { counts[0] = s0; counts[1] = s1; }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_gl_sens(pf_problem P, const double* __restrict__ d0_in, const double* __restrict__ u,
                                                 const double* __restrict__ a, const double* __restrict__ e0_in, int accumulate,
                                                 double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < M.n_elems; e += gridDim.x * blockDim.x) {
    int ni, nj;
    double d0[DIM], du[DIM], da[DIM];
    load_gl_geo<DIM>(M, d0_in, u, e, ni, nj, d0, du);
    node_diff<DIM>(a, ni, nj, da);
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
      int ni, nj;
      double d0[DIM], du[DIM], dv[DIM];
      load_gl_geo<DIM>(M, d0_in, u, e, ni, nj, d0, du);
      node_diff<DIM>(vk, ni, nj, dv);
      double l02 = 0.0, ddv = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) { l02 += d0[c] * d0[c]; ddv += (d0[c] + du[c]) * dv[c]; }
      r = ddv / l02;
    }
    row[i] = r;
  }
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
    const double t = pf_block_sum_d(acc, red);
    if (threadIdx.x == 0) out[g] = t;
  }
}

// ---- the node gather ---------------------------------------------------------------------------------------------------
// store(dof, s) for every dof of `node`, s = the sum of term(code) over the node's incidences (adjacency codes: element
// id << 1 | end) in ascending order.  Two incidences per round: their codes, group ids and the term's records are loaded
// together, and the odd last round repeats its incidence and drops it by a select, not a branch (the node kernels of
// pf_node.h issue theirs the same way).  GROUPED: only the elements e with elem_group[e] == group count, another group's
// incidence adding +0.0, so the matching terms are summed in the ungrouped order.
// The two sums are written differently on purpose.  `acc + t` with t a product may be contracted into an FMA, an add of a
// select may not, so each kernel keeps the form it was measured with and its bits.
template <int DIM, bool GROUPED, class Term, class Store>
__device__ __forceinline__ void node_gather(const pf_mesh& M, int node, const int* __restrict__ elem_group, int group,
                                            const Term& term, const Store& store) {
  const int b = M.adj_ptr[node], e_ = M.adj_ptr[node + 1];
  double acc[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
  for (int idx = b; idx < e_; idx += 2) {
    const bool two = idx + 1 < e_;
    const int code0 = M.adj[idx], code1 = M.adj[two ? idx + 1 : idx];
    bool in0 = true, in1 = two;
    if (GROUPED) { in0 = elem_group[code0 >> 1] == group; in1 = two && elem_group[code1 >> 1] == group; }
    double t0[DIM], t1[DIM];
    term(code0, t0);
    term(code1, t1);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      if (GROUPED) {
        acc[c] += in0 ? t0[c] : 0.0;
        acc[c] += in1 ? t1[c] : 0.0;
      } else {
        acc[c] += t0[c];
        const double t = acc[c] + t1[c];
        acc[c] = two ? t : acc[c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < DIM; ++c) store(node * DIM + c, acc[c]);
}
// one node per thread, grid-stride.  The loop head stands in the kernel: read in a helper, blockDim keeps the code for a
// partial last workgroup that the compiler drops from a kernel's own read.
#define PF_EACH_NODE(node, M) \
  for (int node = blockIdx.x * blockDim.x + threadIdx.x; node < (M).n_nodes; node += gridDim.x * blockDim.x)

// the terms: out = one incidence's contribution, + at the element's second node (end 1), - at its first
// +-fe
template <int DIM>
struct fe_term {
  const double* __restrict__ fe;
  __device__ __forceinline__ void operator()(int code, double* out) const {
    const int e = code >> 1;
    const double sg = (code & 1) ? 1.0 : -1.0;
    if (DIM == 2) {
      const double2 f = reinterpret_cast<const double2*>(fe)[e];
      out[0] = sg * f.x; out[DIM - 1] = sg * f.y;
    } else {
      out[0] = sg * fe[e];
    }
  }
};

// +-w d with w = weight[e] / l0 (BY_L0) or weight[e] / l0^2; d from d0 and u, so it reads no record of pf_gl_state
template <int DIM, bool BY_L0>
struct geo_term {
  const pf_mesh& M;
  const double* __restrict__ d0_in;
  const double* __restrict__ u;
  const double* __restrict__ weight;
  __device__ __forceinline__ void operator()(int code, double* out) const {
    const int e = code >> 1;
    const double sg = (code & 1) ? 1.0 : -1.0;
    int ni, nj;
    double d0[DIM], du[DIM];
    load_gl_geo<DIM>(M, d0_in, u, e, ni, nj, d0, du);
    double l02 = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) l02 += d0[c] * d0[c];
    const double w = weight[e] / (BY_L0 ? sqrt(l02) : l02);
#pragma unroll
    for (int c = 0; c < DIM; ++c) out[c] = sg * (w * (d0[c] + du[c]));
  }
};

__device__ __forceinline__ bool dof_fixed(const pf_mesh& M, int dof) { return M.dof_flags[dof] & PF_DOF_FIXED; }

template <int DIM>
__global__ __launch_bounds__(256) void k_gl_fint(pf_problem P, const double* __restrict__ fe, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  PF_EACH_NODE(node, M)
    node_gather<DIM, false>(M, node, nullptr, 0, fe_term<DIM>{fe}, [&](int dof, double s) { out[dof] = s; });
}

// out[k][dof] = -(sum of +-fe over the node's elements e with elem_group[e] == g0 + k), k = blockIdx.y; 0.0 on fixed dofs
template <int DIM>
__global__ __launch_bounds__(256) void k_gl_group_rhs(pf_problem P, const double* __restrict__ fe,
                                                      const int* __restrict__ elem_group, int g0, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  double* __restrict__ row = out + (size_t)blockIdx.y * (size_t)M.n_dofs;
  PF_EACH_NODE(node, M)
    node_gather<DIM, true>(M, node, elem_group, g0 + (int)blockIdx.y, fe_term<DIM>{fe},
                           [&](int dof, double s) { row[dof] = dof_fixed(M, dof) ? 0.0 : -s; });
}

// out[k][dof] = sum of +-(ea[e] / l0) d_e over the node's elements e with elem_group[e] == g0 + k, k = blockIdx.y; 0.0 on
// fixed dofs
template <int DIM>
__global__ __launch_bounds__(256) void k_gl_prestress_rhs(pf_problem P, const double* __restrict__ d0_in,
                                                          const double* __restrict__ ea, const double* __restrict__ u,
                                                          const int* __restrict__ elem_group, int g0, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  double* __restrict__ row = out + (size_t)blockIdx.y * (size_t)M.n_dofs;
  PF_EACH_NODE(node, M)
    node_gather<DIM, true>(M, node, elem_group, g0 + (int)blockIdx.y, geo_term<DIM, true>{M, d0_in, u, ea},
                           [&](int dof, double s) { row[dof] = dof_fixed(M, dof) ? 0.0 : s; });
}

// out[dof] = sum over the node's incidences of +-(coef[e] / l0^2) d_e; accumulate: out += that sum, rounded first
template <int DIM>
__global__ __launch_bounds__(256) void k_gl_strain_rhs(pf_problem P, const double* __restrict__ d0_in,
                                                       const double* __restrict__ u, const double* __restrict__ coef,
                                                       int accumulate, double* __restrict__ out) {
  const pf_mesh& M = P.mesh;
  PF_EACH_NODE(node, M)
    node_gather<DIM, false>(M, node, nullptr, 0, geo_term<DIM, false>{M, d0_in, u, coef}, [&](int dof, double s) {
      const bool fixed = dof_fixed(M, dof);
      if (accumulate) {
        if (!fixed) out[dof] = __dadd_rn(out[dof], s);      // s rounded first: the sum of two single calls, to the bit
      } else {
        out[dof] = fixed ? 0.0 : s;
      }
    });
}

// ---- explicit dynamics: the central-difference step -----------------------------------------------------
// the strain that carries stress, e - e0, of element e from d0 and u, with e as k_gl_state forms it (the difference of squares
// written out); also the element's E*A (ea and e0 nullable, the same decision in every thread), d0, du and l0^2
template <int DIM>
__device__ __forceinline__ double dyn_strain(const pf_problem& P, const double* d0_in, const double* u, const double* ea_in,
                                             const double* e0_in, int e, double* d0, double* du, double& l02, double& ea) {
  int ni, nj;
  load_gl_geo<DIM>(P.mesh, d0_in, u, e, ni, nj, d0, du);
  ea = ea_in ? ea_in[e] : elem_ea64(P, e);
  double d0du = 0.0, dudu = 0.0;
  l02 = 0.0;
#pragma unroll
  for (int c = 0; c < DIM; ++c) { l02 += d0[c] * d0[c]; d0du += d0[c] * du[c]; dudu += du[c] * du[c]; }
  const double strain = (2.0 * d0du + dudu) / (2.0 * l02);
  return e0_in ? strain - e0_in[e] : strain;
}

// +-(ea (e - e0) / l0) d: k_gl_state's fe formed per incidence, so a step reads no element record.  CABLE: an element
// with cable[e] != 0 carries no compression: N / l0 = 0.0 where e - e0 < 0, a select on the value, so a slack element's term
// is +-0.0 and the sum keeps its order
template <int DIM, bool CABLE>
struct dyn_term {
  const pf_problem& P;
  const double* __restrict__ d0_in;
  const double* __restrict__ u;
  const double* __restrict__ ea_in;
  const double* __restrict__ e0_in;
  const unsigned char* __restrict__ cable;
  __device__ __forceinline__ void operator()(int code, double* out) const {
    const int e = code >> 1;
    const double sg = (code & 1) ? 1.0 : -1.0;
    double d0[DIM], du[DIM], l02, ea;
    const double se = dyn_strain<DIM>(P, d0_in, u, ea_in, e0_in, e, d0, du, l02, ea);
    double n_l0 = (ea * se) / sqrt(l02);
    if (CABLE) n_l0 = (cable[e] && se < 0.0) ? 0.0 : n_l0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) out[c] = sg * (n_l0 * (d0[c] + du[c]));
  }
};

// the displacements of step n: the steps ping-pong between u0 and u1, step n reads buffer n & 1 and writes the other
__device__ __forceinline__ const double* dyn_u_at(const pf_dyn& D, long long n) { return (n & 1) ? D.u1 : D.u0; }

// the histories of a step: none, or the launch's operand
__device__ __forceinline__ pf_dyn_hist dyn_hist_of() { return pf_dyn_hist{nullptr, nullptr, nullptr, 0}; }
__device__ __forceinline__ pf_dyn_hist dyn_hist_of(const pf_dyn_hist& h) { return h; }

// the sample of step n in a history of last + 1 samples: a step beyond the table reads its last entry (the history is held)
__device__ __forceinline__ long long dyn_sample_at(long long n, long long last) { return n < 0 ? 0 : (n < last ? n : last); }

// Step n = *clock + k of the sequence, one node per thread:
//   v <- c1 v + g (lam(t_n) f_ext - f_int(u_n)) / m,   u_{n+1} = u_n + dt v;   fixed dofs: v = 0, u = 0.
// A thread reads and writes only its own dofs of v (in place); its neighbours read u_n, so u_{n+1} goes to the other buffer.
// cable: [n_elems] the tension-only flags, read by the CABLE instantiations alone (the bar's get nullptr)
// HIST: empty, or pf_dyn_hist and one more operand, the time histories the host sampled at the step times (the <DIM, CABLE>
// instantiations keep their operands and their code): lam = H.lam[i(n)] in place of the ramp where H.lam is given, and a fixed
// dof with an amplitude a != 0.0 gets u_{n+1} = a H.sup[i(n + 1)], one product; i(n) = n held inside the table.  The two
// samples are the same for the whole launch; sup_amp is read under `fixed` alone.  The select on a keeps the bytes of 0.0 on
// a support that is not moved (0.0 * s is -0.0 for a negative s).  v on a fixed dof stays 0.0: the energy kernels never
// divide by a support's minv.
template <int DIM, bool CABLE, class... HIST>
__global__ __launch_bounds__(256) void k_gl_dyn_step(pf_problem P, const double* __restrict__ d0_in, pf_dyn D, long long k,
                                                     double c1, double g, double dt, const unsigned char* __restrict__ cable,
                                                     HIST... hist) {
  constexpr bool with_hist = sizeof...(HIST) > 0;
  const pf_dyn_hist H = dyn_hist_of(hist...);
  const pf_mesh& M = P.mesh;
  const long long n = *D.clock + k;
  const double* __restrict__ u_n = dyn_u_at(D, n);
  double* __restrict__ u_next = const_cast<double*>(dyn_u_at(D, n + 1));
  const double t = (double)n * D.dt;
  double lam = D.t_ramp > 0.0 ? D.lam0 + (D.lam1 - D.lam0) * fmin(1.0, t / D.t_ramp) : D.lam1;
  double s_next = 0.0;
  if (with_hist) {
    const long long last = H.n_samples - 1;
    if (H.lam) lam = H.lam[dyn_sample_at(n, last)];
    if (H.sup) s_next = H.sup[dyn_sample_at(n + 1, last)];
  }
  PF_EACH_NODE(node, M)
    node_gather<DIM, false>(M, node, nullptr, 0, dyn_term<DIM, CABLE>{P, d0_in, u_n, D.ea, D.e0, cable}, [&](int dof, double f_int) {
      const bool fixed = dof_fixed(M, dof);
      const double v = c1 * D.v[dof] + g * ((lam * D.f_ext[dof] - f_int) * D.minv[dof]);
      D.v[dof] = fixed ? 0.0 : v;
      double held = 0.0;
      if (with_hist) {
        if (fixed && H.sup) {
          const double a = H.sup_amp[dof];
          held = a != 0.0 ? a * s_next : 0.0;
        }
      }
      u_next[dof] = fixed ? held : u_n[dof] + dt * v;
    });
}

// the clock after a sequence of n steps: one thread, a plain store
__global__ void k_gl_dyn_clock(long long* clock, long long n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *clock = *clock + n;
}

__device__ __forceinline__ double block_max_d(double v, double* smem) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane == 0) smem[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t = fmax(t, smem[i]);
  return t;
}

// Per block, partial sums at the state the clock points to (u_{n+1}, v_{n+1/2}): kinetic energy sum m v^2 / 2 (m = 1 / minv;
// a dof at rest adds nothing, whatever its minv), strain energy sum E*A l0 (e - e0)^2 / 2, f_ext.u and max |v|.  Thread i
// takes node i and element i.  part: [gridDim.x][4].  CABLE: a slack element (cable[i] != 0 and e - e0 < 0, the step's own
// decision) adds no strain energy and 1.0 to a fifth partial, an exact integer; part: [gridDim.x][5].
template <int DIM, bool CABLE>
__global__ __launch_bounds__(256) void k_gl_dyn_energy(pf_problem P, const double* __restrict__ d0_in, pf_dyn D,
                                                       double* __restrict__ part, const unsigned char* __restrict__ cable) {
  __shared__ double red[8];
  const pf_mesh& M = P.mesh;
  const double* __restrict__ u = dyn_u_at(D, *D.clock);
  double kin = 0.0, se_sum = 0.0, work = 0.0, vmax = 0.0, n_slack = 0.0;
  const int count = M.n_nodes > M.n_elems ? M.n_nodes : M.n_elems;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    if (i < M.n_nodes) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const int dof = i * DIM + c;
        const double v = D.v[dof];
        if (v != 0.0) kin += 0.5 * (v * v) / D.minv[dof];
        work += D.f_ext[dof] * u[dof];
        vmax = fmax(vmax, fabs(v));
      }
    }
    if (i < M.n_elems) {
      double d0[DIM], du[DIM], l02, ea;
      const double se = dyn_strain<DIM>(P, d0_in, u, D.ea, D.e0, i, d0, du, l02, ea);
      double se2 = se * se;
      if (CABLE) {        // the select sits on the factor, so the sum keeps the bar's form (and its contraction) and gets +0.0
        const bool slack = cable[i] && se < 0.0;
        se2 = slack ? 0.0 : se2;
        n_slack += slack ? 1.0 : 0.0;
      }
      se_sum += 0.5 * (ea * sqrt(l02)) * se2;
    }
  }
  const double s0 = pf_block_sum_d(kin, red), s1 = pf_block_sum_d(se_sum, red), s2 = pf_block_sum_d(work, red);
  const double s3 = block_max_d(vmax, red);
  const double s4 = CABLE ? pf_block_sum_d(n_slack, red) : 0.0;
  if (threadIdx.x == 0) {
    double* __restrict__ o = part + (CABLE ? 5 : 4) * (size_t)blockIdx.x;
    o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
    if (CABLE) o[4] = s4;
  }
}

// out[0..2] = the sums of the nb block partials, thread t adding blocks t, t + 256, ... in that order; out[3] = their maximum;
// CABLE: five partials per block, out[4] = the sum of the fifth (the slack count), in the same order
template <bool CABLE>
__global__ __launch_bounds__(256) void k_gl_dyn_energy_sum(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double red[8];
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = (int)threadIdx.x; b < nb; b += (int)blockDim.x) {
    const double* __restrict__ r = part + (CABLE ? 5 : 4) * (size_t)b;
    a[0] += r[0]; a[1] += r[1]; a[2] += r[2]; a[3] = fmax(a[3], r[3]);
    if (CABLE) a[4] += r[4];
  }
  const double s0 = pf_block_sum_d(a[0], red), s1 = pf_block_sum_d(a[1], red), s2 = pf_block_sum_d(a[2], red);
  const double s3 = block_max_d(a[3], red);
  const double s4 = CABLE ? pf_block_sum_d(a[4], red) : 0.0;
  if (threadIdx.x == 0) {
    out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3;
    if (CABLE) out[4] = s4;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int gl_fail(int code, const char* who, const char* what) {
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  pf_set_error(buf);
  return code;
}

bool mesh_ok(const pf_problem* p) { return p && (p->mesh.dim == 1 || p->mesh.dim == 2) && p->mesh.n_elems >= 0; }

// what the node kernels and load_gl_geo read of the mesh
bool node_mesh_ok(const pf_problem* p) {
  return mesh_ok(p) && p->mesh.conn && p->mesh.adj_ptr && p->mesh.adj && p->mesh.dof_flags && p->mesh.n_nodes >= 0 &&
         p->mesh.n_dofs == p->mesh.n_nodes * p->mesh.dim;
}

// m rows in blockIdx.y, of groups g0 .. g0 + m - 1 (`groups`) or of plain rows (g0 = 0)
int rows_ok(const char* who, int g0, int m, bool groups) {
  if (m < 1 || m > 65535) return gl_fail(PF_ERR_ARG, who, groups ? "bad group count (m)" : "bad row count (m)");
  if (g0 < 0 || g0 > INT_MAX - m) return gl_fail(PF_ERR_ARG, who, "bad first group (g0)");
  return PF_OK;
}

int launched(const char* who) {
  return hipGetLastError() == hipSuccess ? PF_OK : gl_fail(PF_ERR_HIP, who, "HIP launch failed");
}

// k2 / k1: the kernel's instantiations for dim 2 and 1
template <class K, class... Args>
int launch(const char* who, const pf_problem* p, K k2, K k1, dim3 grid, void* stream, Args... args) {
  if (p->mesh.dim == 2) hipLaunchKernelGGL(k2, grid, dim3(256), 0, (hipStream_t)stream, *p, args...);
  else hipLaunchKernelGGL(k1, grid, dim3(256), 0, (hipStream_t)stream, *p, args...);
  return launched(who);
}

int elem_blocks(int n_elems) {
  const int nb = (n_elems + 255) / 256;
  return nb > PF_MAX_NODE_BLOCKS ? PF_MAX_NODE_BLOCKS : nb;
}

int gl_state(const char* who, const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const double* u,
             void* stream) {
  if (!mesh_ok(p) || !g || !g->d0 || !g->kt || !g->fe || !g->strain || !u) return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_elems == 0) return PF_OK;
  return launch(who, p, k_gl_state<2, false>, k_gl_state<1, false>, dim3(elem_blocks(p->mesh.n_elems)), stream, *g, u, ea, e0);
}

int gl_sens(const char* who, const pf_problem* p, const pf_gl* g, const double* e0, const double* u, const double* a,
            int accumulate, double* out, void* stream) {
  if (!mesh_ok(p) || !g || !g->d0 || !u || !a || !out || (accumulate != 0 && accumulate != 1))
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_elems == 0) return PF_OK;
  return launch(who, p, k_gl_sens<2>, k_gl_sens<1>, dim3(elem_blocks(p->mesh.n_elems)), stream, g->d0, u, a, e0, accumulate,
                out);
}

// everything a dynamics entry point is given, before anything is enqueued
int dyn_check(const char* who, const pf_problem* p, const pf_gl* g, const pf_dyn* d) {
  if (!node_mesh_ok(p)) return gl_fail(PF_ERR_ARG, who, "bad mesh");
  if (!g || !g->d0 || !d || !d->minv || !d->f_ext || !d->u0 || !d->u1 || !d->v || !d->clock)
    return gl_fail(PF_ERR_ARG, who, "null pointer");
  if (!(d->dt > 0.0) || !isfinite(d->dt)) return gl_fail(PF_ERR_ARG, who, "dt must be positive and finite");
  if (!(d->alpha >= 0.0) || !isfinite(d->alpha)) return gl_fail(PF_ERR_ARG, who, "alpha must not be negative");
  if (!(d->t_ramp >= 0.0) || !isfinite(d->t_ramp)) return gl_fail(PF_ERR_ARG, who, "t_ramp must not be negative");
  if (!isfinite(d->lam0) || !isfinite(d->lam1)) return gl_fail(PF_ERR_ARG, who, "non-finite load factor");
  return PF_OK;
}

// n_steps launches of the step with the coefficients (c1, gk), then the clock's: a single chain on s.  cable: the
// tension-only flags and the step's CABLE instantiation, or null and the bar step.  hist: the time histories and the step's
// HIST instantiation, or null and the step of the ramp and the supports at rest
int dyn_enqueue(const char* who, const pf_problem* p, const pf_gl* g, const pf_dyn* d, const pf_dyn_hist* hist,
                const unsigned char* cable, int n_steps, double c1, double gk, hipStream_t s) {
  if (p->mesh.n_nodes > 0) {
    const dim3 grid(pf_node_blocks(p->mesh.n_nodes));
    const auto k2 = cable ? k_gl_dyn_step<2, true> : k_gl_dyn_step<2, false>;
    const auto k1 = cable ? k_gl_dyn_step<1, true> : k_gl_dyn_step<1, false>;
    const auto h2 = cable ? k_gl_dyn_step<2, true, pf_dyn_hist> : k_gl_dyn_step<2, false, pf_dyn_hist>;
    const auto h1 = cable ? k_gl_dyn_step<1, true, pf_dyn_hist> : k_gl_dyn_step<1, false, pf_dyn_hist>;
    for (int k = 0; k < n_steps; ++k)
      if (const int rc = hist ? launch(who, p, h2, h1, grid, s, g->d0, *d, (long long)k, c1, gk, d->dt, cable, *hist)
                              : launch(who, p, k2, k1, grid, s, g->d0, *d, (long long)k, c1, gk, d->dt, cable))
        return rc;
  }
  hipLaunchKernelGGL(k_gl_dyn_clock, dim3(1), dim3(64), 0, s, d->clock, (long long)n_steps);
  return launched(who);
}

// the coefficients of a full step: c1 = (1 - alpha dt / 2) / (1 + alpha dt / 2), g = dt / (1 + alpha dt / 2)
void dyn_coefficients(const pf_dyn* d, double& c1, double& gk) {
  const double h = 0.5 * d->alpha * d->dt;
  c1 = (1.0 - h) / (1.0 + h);
  gk = d->dt / (1.0 + h);
}

// The four entry points, each stated once for the bar family (cable == null) and the cable family.  A _cable entry point
// refuses a null cable first (cable_given), so a null here always means the bar family.  start, steps and graph_create take
// the time histories too: a _hist entry point refuses a bad record first (hist_given), so a null hist always means none.
int cable_given(const char* who, const unsigned char* cable) {
  return cable ? PF_OK : gl_fail(PF_ERR_ARG, who, "null cable (the entry point without _cable is the run of bars)");
}

int hist_given(const char* who, const pf_dyn_hist* h) {
  if (!h) return gl_fail(PF_ERR_ARG, who, "null hist (the entry point without _hist is the run of the ramp)");
  if (!h->lam && !h->sup) return gl_fail(PF_ERR_ARG, who, "hist holds neither lam nor sup (the entry point without _hist is that run)");
  if (h->sup && !h->sup_amp) return gl_fail(PF_ERR_ARG, who, "sup without sup_amp");
  if (h->n_samples < 1) return gl_fail(PF_ERR_ARG, who, "n_samples must be at least 1");
  return PF_OK;
}

int dyn_start(const char* who, const pf_problem* p, const pf_gl* g, const pf_dyn* d, const pf_dyn_hist* hist,
              const unsigned char* cable, void* stream) {
  if (const int rc = dyn_check(who, p, g, d)) return rc;
  long long clock = -1;
  if (hipMemcpyAsync(&clock, d->clock, sizeof(clock), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return gl_fail(PF_ERR_HIP, who, "reading the clock failed");
  if (clock != 0) return gl_fail(PF_ERR_ARG, who, "the clock must be 0 (the half kick starts a run)");
  return dyn_enqueue(who, p, g, d, hist, cable, 1, 1.0 - 0.5 * d->alpha * d->dt, 0.5 * d->dt, (hipStream_t)stream);
}

int dyn_steps(const char* who, const pf_problem* p, const pf_gl* g, const pf_dyn* d, const pf_dyn_hist* hist,
              const unsigned char* cable, int n_steps, void* stream) {
  if (const int rc = dyn_check(who, p, g, d)) return rc;
  if (n_steps < 1) return gl_fail(PF_ERR_ARG, who, "n_steps must be at least 1");
  double c1, gk;
  dyn_coefficients(d, c1, gk);
  return dyn_enqueue(who, p, g, d, hist, cable, n_steps, c1, gk, (hipStream_t)stream);
}

int dyn_graph_create(const char* who, const pf_problem* p, const pf_gl* g, const pf_dyn* d, const pf_dyn_hist* hist,
                     const unsigned char* cable, int n_steps, void* stream, void** graph_out) {
  if (const int rc = dyn_check(who, p, g, d)) return rc;
  if (n_steps < 1) return gl_fail(PF_ERR_ARG, who, "n_steps must be at least 1");
  if (!graph_out) return gl_fail(PF_ERR_ARG, who, "null pointer");
  double c1, gk;
  dyn_coefficients(d, c1, gk);
  return capture_graph((hipStream_t)stream, 0, hipStreamCaptureModeThreadLocal, graph_out,
                       [&](pf_capture& cap) { return dyn_enqueue(who, p, g, d, hist, cable, n_steps, c1, gk, cap.s); });
}

// out: the results (4, with cable 5), then as many block partials per block
int dyn_energy(const char* who, const pf_problem* p, const pf_gl* g, const pf_dyn* d, const unsigned char* cable, double* out,
               void* stream) {
  if (const int rc = dyn_check(who, p, g, d)) return rc;
  if (!out) return gl_fail(PF_ERR_ARG, who, "null pointer");
  const int count = p->mesh.n_nodes > p->mesh.n_elems ? p->mesh.n_nodes : p->mesh.n_elems;
  const int nb = pf_node_blocks(count);
  double* part = out + (cable ? 5 : 4);
  const auto k2 = cable ? k_gl_dyn_energy<2, true> : k_gl_dyn_energy<2, false>;
  const auto k1 = cable ? k_gl_dyn_energy<1, true> : k_gl_dyn_energy<1, false>;
  if (const int rc = launch(who, p, k2, k1, dim3(nb), stream, g->d0, *d, part, cable)) return rc;
  hipLaunchKernelGGL(cable ? k_gl_dyn_energy_sum<true> : k_gl_dyn_energy_sum<false>, dim3(1), dim3(256), 0, (hipStream_t)stream,
                     (const double*)part, nb, out);
  return launched(who);
}

}  // namespace

extern "C" {

int pf_gl_dyn_start(const pf_problem* p, const pf_gl* g, const pf_dyn* d, void* stream) {
  return dyn_start("pf_gl_dyn_start", p, g, d, nullptr, nullptr, stream);
}

int pf_gl_dyn_steps(const pf_problem* p, const pf_gl* g, const pf_dyn* d, int n_steps, void* stream) {
  return dyn_steps("pf_gl_dyn_steps", p, g, d, nullptr, nullptr, n_steps, stream);
}

int pf_gl_dyn_graph_create(const pf_problem* p, const pf_gl* g, const pf_dyn* d, int n_steps, void* stream, void** graph_out) {
  return dyn_graph_create("pf_gl_dyn_graph_create", p, g, d, nullptr, nullptr, n_steps, stream, graph_out);
}

int pf_gl_dyn_energy(const pf_problem* p, const pf_gl* g, const pf_dyn* d, double* out4, void* stream) {
  return dyn_energy("pf_gl_dyn_energy", p, g, d, nullptr, out4, stream);
}

int pf_gl_dyn_start_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* d, const unsigned char* cable, void* stream) {
  const char* who = "pf_gl_dyn_start_cable";
  if (const int rc = cable_given(who, cable)) return rc;
  return dyn_start(who, p, g, d, nullptr, cable, stream);
}

int pf_gl_dyn_steps_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* d, const unsigned char* cable, int n_steps,
                          void* stream) {
  const char* who = "pf_gl_dyn_steps_cable";
  if (const int rc = cable_given(who, cable)) return rc;
  return dyn_steps(who, p, g, d, nullptr, cable, n_steps, stream);
}

int pf_gl_dyn_graph_create_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* d, const unsigned char* cable, int n_steps,
                                 void* stream, void** graph_out) {
  const char* who = "pf_gl_dyn_graph_create_cable";
  if (const int rc = cable_given(who, cable)) return rc;
  return dyn_graph_create(who, p, g, d, nullptr, cable, n_steps, stream, graph_out);
}

int pf_gl_dyn_energy_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* d, const unsigned char* cable, double* out5,
                           void* stream) {
  const char* who = "pf_gl_dyn_energy_cable";
  if (const int rc = cable_given(who, cable)) return rc;
  return dyn_energy(who, p, g, d, cable, out5, stream);
}

int pf_gl_dyn_start_hist(const pf_problem* p, const pf_gl* g, const pf_dyn* d, const pf_dyn_hist* hist, const unsigned char* cable,
                         void* stream) {
  const char* who = "pf_gl_dyn_start_hist";
  if (const int rc = hist_given(who, hist)) return rc;
  return dyn_start(who, p, g, d, hist, cable, stream);
}

int pf_gl_dyn_steps_hist(const pf_problem* p, const pf_gl* g, const pf_dyn* d, const pf_dyn_hist* hist, const unsigned char* cable,
                         int n_steps, void* stream) {
  const char* who = "pf_gl_dyn_steps_hist";
  if (const int rc = hist_given(who, hist)) return rc;
  return dyn_steps(who, p, g, d, hist, cable, n_steps, stream);
}

int pf_gl_dyn_graph_create_hist(const pf_problem* p, const pf_gl* g, const pf_dyn* d, const pf_dyn_hist* hist,
                                const unsigned char* cable, int n_steps, void* stream, void** graph_out) {
  const char* who = "pf_gl_dyn_graph_create_hist";
  if (const int rc = hist_given(who, hist)) return rc;
  return dyn_graph_create(who, p, g, d, hist, cable, n_steps, stream, graph_out);
}

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

int pf_gl_state_cable(const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const unsigned char* cable,
                      unsigned char* slack, double* counts, const double* u, void* stream) {
  const char* who = "pf_gl_state_cable";
  if (!cable || !slack || !counts)
    return gl_fail(PF_ERR_ARG, who, "null cable, slack or counts (pf_gl_state / pf_gl_state_ea / pf_gl_state_e0 are the run of bars)");
  if (!mesh_ok(p) || !g || !g->d0 || !g->kt || !g->fe || !g->strain || !u) return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_elems == 0) {
    if (hipMemsetAsync(counts, 0, 2 * sizeof(double), (hipStream_t)stream) != hipSuccess)
      return gl_fail(PF_ERR_HIP, who, "clearing the counts failed");
    return PF_OK;
  }
  const int nb = elem_blocks(p->mesh.n_elems);
  const gl_cable_set set{cable, slack, counts + 2};
  if (const int rc = launch(who, p, k_gl_state<2, true, gl_cable_set>, k_gl_state<1, true, gl_cable_set>, dim3(nb), stream, *g,
                            u, ea, e0, set))
    return rc;
  hipLaunchKernelGGL(k_gl_cable_counts, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, nb);
  return launched(who);
}

int pf_gl_state_plastic(const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const pf_gl_plastic* pl,
                        const double* u, void* stream) {
  const char* who = "pf_gl_state_plastic";
  if (!pl || !pl->ey || !pl->kappa || !pl->ep_n || !pl->al_n || !pl->ep || !pl->al || !pl->yielding || !pl->counts)
    return gl_fail(PF_ERR_ARG, who, "null plastic record or a null pointer in it (pf_gl_state / pf_gl_state_ea / pf_gl_state_e0 "
                                    "are the elastic run)");
  if (pl->ep == pl->ep_n || pl->al == pl->al_n)
    return gl_fail(PF_ERR_ARG, who, "ep == ep_n or al == al_n: the trial state is written beside the committed one, never in "
                                    "place (a commit swaps the two pointers)");
  if (!mesh_ok(p) || !g || !g->d0 || !g->kt || !g->fe || !g->strain || !u) return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_elems == 0) {
    if (hipMemsetAsync(pl->counts, 0, 2 * sizeof(double), (hipStream_t)stream) != hipSuccess)
      return gl_fail(PF_ERR_HIP, who, "clearing the counts failed");
    return PF_OK;
  }
  const int nb = elem_blocks(p->mesh.n_elems);
  const gl_plastic_set set{pl->ey, pl->kappa, pl->ep_n, pl->al_n, pl->ep, pl->al, pl->yielding, pl->counts + 2};
  if (const int rc = launch(who, p, k_gl_state<2, false, gl_plastic_set>, k_gl_state<1, false, gl_plastic_set>, dim3(nb), stream,
                            *g, u, ea, e0, set))
    return rc;
  hipLaunchKernelGGL(k_gl_cable_counts, dim3(1), dim3(256), 0, (hipStream_t)stream, pl->counts, nb);
  return launched(who);
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
  return launched(who);
}

int pf_gl_fint(const pf_problem* p, const pf_gl* g, double* f_int_out, void* stream) {
  const char* who = "pf_gl_fint";
  if (!node_mesh_ok(p) || !g || !g->fe || !f_int_out) return gl_fail(PF_ERR_ARG, who, "bad argument");
  return launch(who, p, k_gl_fint<2>, k_gl_fint<1>, dim3(pf_node_blocks(p->mesh.n_nodes)), stream, g->fe, f_int_out);
}

int pf_gl_group_rhs(const pf_problem* p, const pf_gl* g, const int* elem_group, int g0, int m, double* out, void* stream) {
  const char* who = "pf_gl_group_rhs";
  if (!node_mesh_ok(p) || !g || !g->fe || !elem_group || !out) return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (const int rc = rows_ok(who, g0, m, true)) return rc;
  if (p->mesh.n_nodes == 0) return PF_OK;
  return launch(who, p, k_gl_group_rhs<2>, k_gl_group_rhs<1>, dim3(pf_node_blocks(p->mesh.n_nodes), m), stream, g->fe,
                elem_group, g0, out);
}

int pf_gl_prestress_rhs(const pf_problem* p, const pf_gl* g, const double* ea, const double* u, const int* elem_group, int g0,
                        int m, double* out, void* stream) {
  const char* who = "pf_gl_prestress_rhs";
  if (!node_mesh_ok(p) || !g || !g->d0 || !ea || !u || !elem_group || !out) return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (const int rc = rows_ok(who, g0, m, true)) return rc;
  if (p->mesh.n_nodes == 0) return PF_OK;
  return launch(who, p, k_gl_prestress_rhs<2>, k_gl_prestress_rhs<1>, dim3(pf_node_blocks(p->mesh.n_nodes), m), stream, g->d0,
                ea, u, elem_group, g0, out);
}

int pf_gl_strain_rhs(const pf_problem* p, const pf_gl* g, const double* u, const double* coef, int accumulate, double* out,
                     void* stream) {
  const char* who = "pf_gl_strain_rhs";
  if (!node_mesh_ok(p) || !g || !g->d0 || !u || !coef || !out || (accumulate != 0 && accumulate != 1))
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (p->mesh.n_nodes == 0) return PF_OK;
  return launch(who, p, k_gl_strain_rhs<2>, k_gl_strain_rhs<1>, dim3(pf_node_blocks(p->mesh.n_nodes)), stream, g->d0, u, coef,
                accumulate, out);
}

int pf_gl_strain_jvp(const pf_problem* p, const pf_gl* g, const double* u, const int* elems, int n_meas, const double* v,
                     int m, double* out, void* stream) {
  const char* who = "pf_gl_strain_jvp";
  if (!node_mesh_ok(p) || !g || !g->d0 || !u || !elems || !v || !out || n_meas < 0)
    return gl_fail(PF_ERR_ARG, who, "bad argument");
  if (const int rc = rows_ok(who, 0, m, false)) return rc;
  if (n_meas == 0) return PF_OK;
  return launch(who, p, k_gl_strain_jvp<2>, k_gl_strain_jvp<1>, dim3(elem_blocks(n_meas), m), stream, g->d0, u, elems, n_meas,
                v, out);
}

}  // extern "C"
