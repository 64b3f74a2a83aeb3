// pf_node.h — dL/du + Adam(u) of a node, shared by k_node_gradu (pf_mesh.hip) and by the MFMA32 forward launch that runs the
// displacement update of the PREVIOUS iteration beside its own element tasks (pf_net32.hip: k_net32_forward2, gu_nb).
//
// Reference: autograd of fem/nn_assembly.py:96-100,194-195 w.r.t. u + the data term (fem/solver.py:274-283),
// optimizer_u.step() (solver.py:292, torch/optim/adam.py single-tensor arithmetic), u[fixed] = 0 (solver.py:297-298).
// The arithmetic of one dof lives in ONE place (dof_grad_u, dof_adam_u: contraction off, every operation an IEEE single
// operation) so that the two callers agree bit for bit whatever surrounds them.
#pragma once
#include "pf_common.h"

struct GraduConsts { float step_size, bc2s, b1w, b2, b2w, eps, dcoef; };

// PP: pointer to a pf_problem in any address space (the fused forward launch reads its own kernel argument through the
// kernarg segment pointer, so that these values are loaded where a node task starts instead of living in scalar registers
// over the whole launch)
template <class PP>
__device__ __forceinline__ GraduConsts gradu_consts_from(PP p) {
  GraduConsts K;
  const pf_state* st = p->state;
  K.step_size = st->step_size_u;
  K.bc2s = st->bc2_sqrt;
  K.b1w = (float)(1.0 - p->beta1);
  K.b2 = (float)p->beta2;
  K.b2w = (float)(1.0 - p->beta2);
  K.eps = (float)p->eps;
  const float nm = p->n_meas_f;
  K.dcoef = nm > 0.f ? p->alpha_data / nm : 0.f;  // mean backward
  return K;
}
__device__ __forceinline__ GraduConsts gradu_consts(const pf_problem& P) { return gradu_consts_from(&P); }

// what a node task reads of the problem
struct NodeView {
  const int32_t *adj_ptr, *adj, *adj_other;
  const uint8_t* dof_flags;
  const float *meas_val, *g_f;
  float *u, *m_u, *v_u, *grad_u;
  int n_nodes, use_data, fe_mode;
};
// ADJ = false: the view of a task that addresses by node id (node_gradu_task_path): the adjacency pointers are not loaded
template <bool ADJ = true, class PP>
__device__ __forceinline__ NodeView node_view_from(PP p) {
  NodeView V;
  V.adj_ptr = ADJ ? p->mesh.adj_ptr : nullptr;
  V.adj = ADJ ? p->mesh.adj : nullptr;
  V.adj_other = ADJ ? p->adj_other : nullptr;
  V.dof_flags = p->mesh.dof_flags;
  V.meas_val = p->mesh.meas_val;
  V.g_f = p->g_f;
  V.u = p->u;
  V.m_u = p->m_u;
  V.v_u = p->v_u;
  V.grad_u = p->grad_u;
  V.n_nodes = p->mesh.n_nodes;
  V.use_data = p->use_data;
  V.fe_mode = p->fe_mode;
  return V;
}

// dL/du of one dof: the gathered K^T g_f entry + d(alpha_d * mean d^2)/du where the dof is measured
__device__ __forceinline__ float dof_grad_u(const GraduConsts& K, bool measured, float g, float meas, float uo) {
  PF_NO_CONTRACT
  float gu = g;
  if (measured) {
    const float d = meas - uo;
    gu += -(K.dcoef * (2.f * d));
  }
  return gu;
}

// torch.optim.Adam single-tensor arithmetic (torch/optim/adam.py) on one free dof
__device__ __forceinline__ void dof_adam_u(const GraduConsts& K, float gu, float& uo, float& m, float& v) {
  PF_NO_CONTRACT
  m = m + K.b1w * (gu - m);                       // lerp_
  v = v * K.b2;                                   // mul_
  v = v + (K.b2w * gu) * gu;                      // addcmul_
  const float denom = sqrtf(v) / K.bc2s + K.eps;
  uo = uo + (-K.step_size) * (m / denom);         // addcdiv_
}

// ---- what a node task does behind its gather: dL/du, Adam, the clamp and the stores of its M x 64 nodes -------------------
// One copy for both node tasks below (they differ only in how they find the operands of acc = (K^T g_f)[node]).
// node: clamped into the mesh, ok: the lane's node exists (else nothing is stored or summed).  Returns the lane's sum of
// u_free^2 over its nodes, m ascending.
template <int DIM, int M>
__device__ __forceinline__ float node_task_update(const NodeView& P, const GraduConsts& K, const int (&node)[M],
                                                  const bool (&ok)[M], const unsigned (&fl)[M][2], const float (&acc)[M][2],
                                                  const float (&meas)[M][2], const float (&uo)[M][2],
                                                  const float (&mo)[M][2], const float (&vo)[M][2]) {
  float sum_u2 = 0.f;
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const int dof = node[m] * DIM + c;
      const unsigned f = fl[m][c];
      const float gu = dof_grad_u(K, P.use_data && (f & PF_DOF_MEASURED), acc[m][c], meas[m][c], uo[m][c]);
      float un = uo[m][c], mn = mo[m][c], vn = vo[m][c];
      dof_adam_u(K, gu, un, mn, vn);
      const bool fixed = (f & PF_DOF_FIXED) != 0;
      if (ok[m]) {
        if (P.grad_u) P.grad_u[dof] = gu;
        if (fixed) {
          if (uo[m][c] != 0.f) P.u[dof] = 0.f;      // solver.py:297-298
        } else {
          P.m_u[dof] = mn;
          P.v_u[dof] = vn;
          P.u[dof] = un;
        }
      }
      { PF_NO_CONTRACT
        if (ok[m] && !fixed) sum_u2 += un * un; }
    }
  }
  return sum_u2;
}

// ---- M x 64 nodes per wave, every level of the gather in flight for all of them together -----------------------------
// The stand-alone kernel hides the three dependent round trips of a node (adj_ptr -> adjacency -> records and neighbour
// values) behind 32 waves per CU; inside the forward launch there are 16, most of them busy with element tasks, so a node
// task carries M nodes per lane and issues each level's loads for all of them before it waits.  Straight-line code with
// selects: a branch per node would let the compiler sink the loads into it and serialise the round trips.
// elem_k: the stiffness records to read (the iteration graph: the half the PREVIOUS forward launch wrote).
// Needs pf_problem.adj_other; single-GPU meshes only (no ghost elements, no shared dofs).  Accumulation in ascending
// element id like gather_kv (pf_mesh.hip), same ke_rows_times: same bits.
template <int DIM, int M>
__device__ __forceinline__ float node_gradu_task(const NodeView& P, const float* __restrict__ elem_k, const GraduConsts& K,
                                                 int node0, int lane) {
  const int nn = P.n_nodes;
  int node[M], b[M], e_[M];
  bool ok[M];
  float vs[M][2], acc[M][2], uo[M][2], meas[M][2];
  unsigned fl[M][2];
  const float* __restrict__ mvals = P.use_data ? P.meas_val : P.u;     // (a select, not a branch: never read without use_data)
  // level 1: CSR row, the node's own values
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int n_ = node0 + m * 64 + lane;
    ok[m] = n_ < nn;
    node[m] = ok[m] ? n_ : nn - 1;
    b[m] = P.adj_ptr[node[m]];
    e_[m] = P.adj_ptr[node[m] + 1];
    load_vec<DIM>(P.g_f, node[m], vs[m]);
    load_vec<DIM>(P.u, node[m], uo[m]);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      fl[m][c] = P.dof_flags[node[m] * DIM + c];
      meas[m][c] = mvals[node[m] * DIM + c];
      acc[m][c] = 0.f;
    }
  }
  int rounds = 0;
#pragma unroll
  for (int m = 0; m < M; ++m) rounds = max(rounds, (e_[m] - b[m] + 1) >> 1);
  // the Adam moments travel with level 1 too (a fixed dof's are dead state: loaded, never stored)
  float mo[M][2], vo[M][2];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      mo[m][c] = P.m_u[node[m] * DIM + c];
      vo[m][c] = P.v_u[node[m] * DIM + c];
    }
  for (int r = 0; r < rounds; ++r) {
    int code0[M], code1[M], oth0[M], oth1[M];
    bool has[M], two[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int idx = b[m] + 2 * r;
      has[m] = idx < e_[m];
      two[m] = idx + 1 < e_[m];
      const int i0 = has[m] ? idx : 0, i1 = two[m] ? idx + 1 : i0;
      code0[m] = P.adj[i0];
      oth0[m] = P.adj_other[i0];
      code1[m] = P.adj[i1];
      oth1[m] = P.adj_other[i1];
    }
    ElemK k0[M], k1[M];
    float w0[M][2], w1[M][2];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      k0[m] = load_k_record<DIM>(elem_k, code0[m] >> 1);
      k1[m] = load_k_record<DIM>(elem_k, code1[m] >> 1);
      load_vec<DIM>(P.g_f, oth0[m], w0[m]);
      load_vec<DIM>(P.g_f, oth1[m], w1[m]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float fe[2];
      const int end0 = code0[m] & 1, end1 = code1[m] & 1;
      ke_rows_times<DIM>(k0[m], end0, end0 ? w0[m] : vs[m], end0 ? vs[m] : w0[m], fe, P.fe_mode);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const float t = acc[m][c] + fe[c];
        acc[m][c] = has[m] ? t : acc[m][c];
      }
      ke_rows_times<DIM>(k1[m], end1, end1 ? w1[m] : vs[m], end1 ? vs[m] : w1[m], fe, P.fe_mode);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const float t = acc[m][c] + fe[c];
        acc[m][c] = two[m] ? t : acc[m][c];
      }
    }
    // the own values are only USED behind this loop: an (empty) use here keeps their loads in front of it — the compiler
    // may otherwise sink them to their first use, one more round trip per task
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int c = 0; c < DIM; ++c)
        asm volatile("" : "+v"(uo[m][c]), "+v"(meas[m][c]), "+v"(mo[m][c]), "+v"(vo[m][c]));
  }
  return node_task_update<DIM, M>(P, K, node, ok, fl, acc, meas, uo, mo, vo);
}

// ---- the same task on an ORDERED PATH: every address from the node id -------------------------------------------------------
// Where the mesh is a path (pf_api.hip: mesh_is_path) AND its node ids follow it, element e joining node e to node e + 1
// (the synthetic chains, a bar meshed from one end to the other), the adjacency the task above chases is implied: node n
// touches element n-1 at its j end and element n at its i end, and its far nodes are n-1 and n+1.  So the three dependent
// round trips are ONE: the records of n-1 and n, g_f at n-1, n, n+1 and the node's own values all leave together, and the 20
// bytes per node of adj_ptr / adj / adj_other are not read.  Indices past the path's ends are clamped to valid addresses
// and their terms dropped by a select, as the gather drops a missing incidence: the end nodes get the bits of their single
// incidence.  Same partition, same ke_rows_times, same 0 + fe(n-1) + fe(n) sequence, same node_task_update: same bits.
// The neighbours' g_f come from loads, not from the lanes beside: they hit the lines the own values bring in, and a lane
// shift would still need the edge lanes' loads.
template <int DIM, int M>
__device__ __forceinline__ float node_gradu_task_path(const NodeView& P, const float* __restrict__ elem_k,
                                                      const GraduConsts& K, int node0, int lane) {
  const int nn = P.n_nodes, ne = nn - 1;             // (a path: n_nodes == n_elems + 1, n_elems >= 1)
  int node[M];
  bool ok[M];
  float vs[M][2], wb[M][2], wa[M][2], acc[M][2], uo[M][2], meas[M][2], mo[M][2], vo[M][2];
  unsigned fl[M][2];
  ElemK kb[M], ka[M];
  const float* __restrict__ mvals = P.use_data ? P.meas_val : P.u;     // (a select, not a branch: never read without use_data)
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int n_ = node0 + m * 64 + lane;
    ok[m] = n_ < nn;
    node[m] = ok[m] ? n_ : nn - 1;
    const int below = max(node[m] - 1, 0), above = min(node[m] + 1, nn - 1);
    kb[m] = load_k_record<DIM>(elem_k, below);                 // element n-1
    ka[m] = load_k_record<DIM>(elem_k, min(node[m], ne - 1));  // element n
    load_vec<DIM>(P.g_f, below, wb[m]);
    load_vec<DIM>(P.g_f, node[m], vs[m]);
    load_vec<DIM>(P.g_f, above, wa[m]);
    load_vec<DIM>(P.u, node[m], uo[m]);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      fl[m][c] = P.dof_flags[node[m] * DIM + c];
      meas[m][c] = mvals[node[m] * DIM + c];
      mo[m][c] = P.m_u[node[m] * DIM + c];
      vo[m][c] = P.v_u[node[m] * DIM + c];
      acc[m][c] = 0.f;
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const bool has_b = node[m] > 0, has_a = node[m] < ne;
    float fe[2];
    ke_rows_times<DIM>(kb[m], 1, wb[m], vs[m], fe, P.fe_mode);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const float t = acc[m][c] + fe[c];
      acc[m][c] = has_b ? t : acc[m][c];
    }
    ke_rows_times<DIM>(ka[m], 0, vs[m], wa[m], fe, P.fe_mode);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const float t = acc[m][c] + fe[c];
      acc[m][c] = has_a ? t : acc[m][c];
    }
  }
  return node_task_update<DIM, M>(P, K, node, ok, fl, acc, meas, uo, mo, vo);
}

// ---- the same gather for M nodes per THREAD (node kernels): (K(theta) v)[node] over the incident elements of each node,
// every level's loads of all M nodes issued before the first wait.  The stand-alone node kernels walk two nodes per
// thread one after the other (grid-stride): six dependent round trips per thread; taken together they are three.
// Same accumulation order per node as gather_kv (pf_mesh.hip), same ke_rows_times: same bits.  Needs adj_other and the
// stiffness records.
template <int DIM, int M>
__device__ __forceinline__ void gather_kv_multi(const pf_problem& P, const float* __restrict__ elem_k,
                                                const float* __restrict__ v, const int (&node)[M], float (&acc)[M][2]) {
  const pf_mesh& Ms = P.mesh;
  int b[M], e_[M];
  float vs[M][2];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    b[m] = Ms.adj_ptr[node[m]];
    e_[m] = Ms.adj_ptr[node[m] + 1];
    load_vec<DIM>(v, node[m], vs[m]);
    acc[m][0] = 0.f;
    acc[m][1] = 0.f;
  }
  int rounds = 0;
#pragma unroll
  for (int m = 0; m < M; ++m) rounds = max(rounds, (e_[m] - b[m] + 1) >> 1);
  for (int r = 0; r < rounds; ++r) {
    int code0[M], code1[M], oth0[M], oth1[M];
    bool has[M], two[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int idx = b[m] + 2 * r;
      has[m] = idx < e_[m];
      two[m] = idx + 1 < e_[m];
      const int i0 = has[m] ? idx : 0, i1 = two[m] ? idx + 1 : i0;
      code0[m] = Ms.adj[i0];
      oth0[m] = P.adj_other[i0];
      code1[m] = Ms.adj[i1];
      oth1[m] = P.adj_other[i1];
    }
    ElemK k0[M], k1[M];
    float w0[M][2], w1[M][2];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      k0[m] = load_k_record<DIM>(elem_k, code0[m] >> 1);
      k1[m] = load_k_record<DIM>(elem_k, code1[m] >> 1);
      load_vec<DIM>(v, oth0[m], w0[m]);
      load_vec<DIM>(v, oth1[m], w1[m]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float fe[2];
      const int end0 = code0[m] & 1, end1 = code1[m] & 1;
      ke_rows_times<DIM>(k0[m], end0, end0 ? w0[m] : vs[m], end0 ? vs[m] : w0[m], fe, P.fe_mode);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const float t = acc[m][c] + fe[c];
        acc[m][c] = has[m] ? t : acc[m][c];
      }
      ke_rows_times<DIM>(k1[m], end1, end1 ? w1[m] : vs[m], end1 ? vs[m] : w1[m], fe, P.fe_mode);
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const float t = acc[m][c] + fe[c];
        acc[m][c] = two[m] ? t : acc[m][c];
      }
    }
  }
}

// ---- residual, dL/df_int and the loss terms of one dof (fem/solver.py:267-283) -----------------------------------------
// Shared by k_node_residual (pf_mesh.hip), by the path form of the fused backward launch, which forms r and g_f of its
// elements' nodes itself (pf_net32.hip: backward_phase, PATH), and by the blocks that re-sum that form's stored residuals
// (pf_mesh.hip: k_theta_stage1_path).  ONE copy of each expression: under the compiler's default contraction two copies
// of one expression have drifted apart before (pf_common.h: PF_NO_CONTRACT).
// f = the dof's internal force; r comes back as 0 for a fixed dof.
__device__ __forceinline__ void dof_residual(float f, unsigned fl, float fx, float lam, float alpha_physics, float& r, float& gf) {
  r = 0.f;
  gf = 0.f;
  if (!(fl & PF_DOF_FIXED)) {
    r = f - lam * fx;                               // solver.py:267-269
    gf = alpha_physics * r;                         // d(alpha_p * 0.5*sum r^2)/dr
  }
}
// the dof's terms of sum r^2 and sum d^2 (mv, un: measured and current displacement; read only where the dof is measured)
__device__ __forceinline__ void dof_loss_terms(unsigned fl, float r, int use_data, float mv, float un, float& sum_r2, float& sum_d2) {
  const bool mine = !(fl & PF_DOF_GHOST);
  if (!(fl & PF_DOF_FIXED) && mine) sum_r2 += r * r;
  if (mine && use_data && (fl & PF_DOF_MEASURED)) {
    const float d = mv - un;                        // solver.py:274
    sum_d2 += d * d;
  }
}

// ---- the residual on a PATH mesh, from the element side -----------------------------------------------------------------
// On a mesh whose elements form an open path in element order (element e joins node i(e) to j(e) = i(e+1); pf_api.hip:
// mesh_is_path) node i(e) touches only elements e-1 (at its j end) and e (at its i end), so a wave that holds 64 consecutive
// elements, one per lane, can form the internal force of every node it touches without the node adjacency: lane e computes
// its element's two end forces, takes the j-end force of e-1 from the lane below and adds in ascending element id like
// gather_kv_multi above (same ke_rows_times, same 0 + fe0 + fe1 sequence: same bits).  Only the wave's two edge lanes need
// values of an element outside the task (PathEdge).  Every lane of the wave must call this (lane shifts).
// Only the lanes named below ever write their PathEdge; in every other lane it holds whatever it held before (zeros, or an
// earlier task's values) and what path_residual computes from it is dropped by a select.
template <int DIM>
struct PathEdge {
  ElemK k;          // lane 0: record of e-1; lane 63: record of e+1
  float u[2];       // lane 0: u at i(e-1); lane 63: u at j(e+1)
  float fx[2];      // f_ext and dof flags at j(e): lane 63 and the mesh's last element
  unsigned fl;
};
// The wave's values one lane up / down on the vector pipe (DPP wave_shr:1 / wave_shl:1: no LDS round trip, no address
// arithmetic).  The lane without a source (0 resp. 63) gets `edge`: bound_ctrl is off, so it keeps the old operand.
__device__ __forceinline__ float wave_shr1(float x, float edge) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, x),
                                                               0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float x, float edge) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, x),
                                                               0x130, 0xf, 0xf, false));
}
// dof flags of a node, both dofs in one register
template <int DIM>
__device__ __forceinline__ unsigned load_node_flags(const uint8_t* __restrict__ dof_flags, int node) {
  if (DIM == 2) return reinterpret_cast<const uint16_t*>(dof_flags)[node];
  return dof_flags[node];
}
// k: the element's own record; fxi, fli: f_ext and flags at i(e); e < n.  Out: r and g_f at i(e) (what the lane stores), and
// at j(e) (r_j only valid for the mesh's last element, which stores it).
template <int DIM>
__device__ __forceinline__ void path_residual(const ElemK& k, const PathEdge<DIM>& x, const float* ui, const float* uj,
                                              const float* fxi, unsigned fli, int e, int n, int lane, float lam,
                                              float alpha_physics, int fe_mode, float* ri, float* gi, float* rj, float* gj) {
  // The j-end rows of an element are its i-end rows negated (ke_rows_times: the same chain with every product's sign
  // flipped, in both fe_modes; rounding is symmetric), so ONE evaluation per element serves both ends: -A is bit for bit what
  // end = 1 returns, except that an exact zero comes out with the other sign.  Every such value enters its sum behind
  // `0.f + ...`, which gives +0 for either zero, so r and g_f keep their bits.
  // No lane needs both neighbours (lane 0: e-1 at its j end, lane 63: e+1 at its i end), so one more evaluation with the
  // lane's own operands serves both: X = the i-end rows of that element; lane 0 takes -X, lane 63 X.
  float A[2], X[2], vi[2], vj[2];
  ke_rows_times<DIM>(k, 0, ui, uj, A, fe_mode);        // element e at its i end -> node i(e); -A: at its j end -> node j(e)
  const bool lo = lane == 0, first = e == 0, last = e >= n - 1;
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    vi[c] = lo ? x.u[c] : uj[c];                       // lane 0: element e-1 = (i(e-1), i(e)); lane 63: e+1 = (j(e), j(e+1))
    vj[c] = lo ? ui[c] : x.u[c];
  }
  ke_rows_times<DIM>(x.k, 0, vi, vj, X, fe_mode);
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    // minus the j-end force of the element below.  At the path's start there is none: 0 there, and (0 + -0) + A has the
    // bits of 0 + A (A itself, or +0 for either zero), the sum of the node's single incidence.
    const float nBp = wave_shr1(A[c], first ? 0.f : X[c]);
    float acc = 0.f;
    acc = acc + (-nBp);
    acc = acc + A[c];
    dof_residual(acc, fli >> (8 * c), fxi[c], lam, alpha_physics, ri[c], gi[c]);
    float accj = 0.f;
    accj = accj + (-A[c]);
    const float tj = accj + X[c];
    accj = last ? accj : tj;                           // the path's end node has one incidence
    float gje;
    dof_residual(accj, x.fl >> (8 * c), x.fx[c], lam, alpha_physics, rj[c], gje);
    const float above = wave_shl1(gi[c], gje);         // (lane 63 keeps its own gje)
    gj[c] = last ? gje : above;
  }
}
