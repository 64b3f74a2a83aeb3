// pf_api.hip — the C ABI declared in include/pinnfem_hip.h: argument checks, net-shape dispatch,
// and the fused GD-iteration launch sequence (FEM/python/fem/solver.py:254-355).
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include "pf_common.h"
#include "pf_graph.h"
#include "pf_net32.h"

// launchers from pf_mesh.hip
int pf_launch_node_residual(const pf_problem* p, float* f_int_out, int compute_loss, hipStream_t s, int fin_prev = 0);
int pf_launch_elem_adjoint(const pf_problem* p, hipStream_t s);
int pf_launch_node_gradu(const pf_problem* p, int fuse_adam, hipStream_t s, int skip_shared = 0, float* u_out = nullptr);
int pf_launch_u_home(const pf_problem* p, hipStream_t s);
int pf_launch_scalar_residual(const pf_problem* p, const pf_scalar_id* sp, hipStream_t s);
int pf_launch_scalar_update(const pf_problem* p, const pf_scalar_id* sp, hipStream_t s);
int pf_launch_shard_pack(const pf_problem* p, float* buf2, const float* u2_local, hipStream_t s);
int pf_launch_shard_update(const pf_problem* p, const float* buf2, float* u2_local, hipStream_t s);
int pf_launch_shard_flush(const pf_problem* p, const float* u2, hipStream_t s);
int pf_launch_theta_reduce(const pf_problem* p, int fuse_adam, hipStream_t s);
int pf_launch_pack_theta(const pf_problem* p, hipStream_t s);
int pf_launch_finalize(const pf_problem* p, int mode, int with_theta, hipStream_t s, int tn_ready = 0);
int pf_launch_theta_stage1(const pf_problem* p, hipStream_t s);
int pf_launch_theta_stage1_path(const pf_problem* p, hipStream_t s, int fin_prev);
int pf_launch_path_check(const pf_problem* p, int* bad, hipStream_t s);
int pf_launch_theta_stage2(const pf_problem* p, int fuse_adam, hipStream_t s);
int pf_launch_reset(const pf_problem* p, hipStream_t s);
int pf_launch_adam(float* param, const float* grad, float* m, float* v, int n, int step, double lr,
                   double beta1, double beta2, double eps, hipStream_t s);
int pf_launch_diag_k(const pf_problem* p, float* diag, hipStream_t s);
int pf_launch_dense_k(const pf_problem* p, float* K, hipStream_t s);
int pf_launch_coo_k(const pf_problem* p, long long* rows, long long* cols, float* vals, hipStream_t s);

// below this many elements the iteration graph is a plain chain: the kernels are then too short to hide anything behind,
// the branches' fork/join cost (~5 us each against ~1.5 us for a plain boundary) would only add to a launch-bound iteration
#define PF_GRAPH_DAG_MIN_ELEMS 200000   /* measured crossover between 1e5 (chain 0.061 vs DAG 0.067 ms) and 3e5 (0.099 vs 0.092) */

static thread_local char g_err[512] = "";

void pf_set_error(const char* msg) {
  strncpy(g_err, msg, sizeof(g_err) - 1);
  g_err[sizeof(g_err) - 1] = 0;
}

static int fail(int code, const char* msg) {
  pf_set_error(msg);
  return code;
}

static int check_launch(int rc, const char* what) {
  if (rc == PF_OK) return PF_OK;
  if (rc == PF_ERR_HIP) {
    char buf[400];
    snprintf(buf, sizeof(buf), "%s: HIP launch failed: %s", what, hipGetErrorString(hipGetLastError()));
    pf_set_error(buf);
  }
  return rc;
}

static int padded_width(int width) {
  if (width < 1 || width > 32) return PF_ERR_UNSUPPORTED;
  return ((width + 3) / 4) * 4;
}

static int check_problem(const pf_problem* p) {
  if (!p) return fail(PF_ERR_ARG, "null problem");
  const pf_mesh& M = p->mesh;
  if (M.dim != 1 && M.dim != 2) return fail(PF_ERR_ARG, "mesh.dim must be 1 or 2");
  if (M.n_nodes < 1 || M.n_elems < 0 || M.n_dofs != M.n_nodes * M.dim)
    return fail(PF_ERR_ARG, "inconsistent mesh sizes");
  if (!M.conn || !M.egeo || !M.ecent || !M.adj_ptr || !M.adj || !M.f_ext || !M.dof_flags || !M.meas_val)
    return fail(PF_ERR_ARG, "null mesh array");
  if (p->n_part_blocks < 1 || p->n_part_blocks > PF_MAX_BLOCKS)
    return fail(PF_ERR_ARG, "n_part_blocks out of range");
  if (!p->u || !p->g_f || !p->partials || !p->state) return fail(PF_ERR_ARG, "null state/workspace");
  for (int k = 0; k < 2; ++k) {
    const pf_net& n = p->net[k];
    if (!n.enabled) continue;
    if (n.in_dim != M.dim + 1)
      return fail(PF_ERR_ARG, "net in_dim must be mesh.dim+1 (columns load_factor, x[, y])");
    if (padded_width(n.width) < 0 || n.n_hidden < 1 || n.n_hidden > 3)
      return fail(PF_ERR_UNSUPPORTED, "net shape outside the compiled menu (width 1..32, hidden layers 1..3)");
    if (!p->theta || !p->theta_pad || !p->pad_index || !p->g_ea || !p->grad_theta)
      return fail(PF_ERR_ARG, "null parameter workspace");
    if ((k == 0 && !p->prop_e) || (k == 1 && !p->prop_a)) return fail(PF_ERR_ARG, "null property array");
    if (p->wg_mode == PF_WG_MFMA32) {
      if (n.width > PF_N32_WIDTH_MAX)
        return fail(PF_ERR_UNSUPPORTED, "MFMA32 engine supports widths up to 30 (use PF_WG_MFMA44 beyond)");
      if (!p->net_op) return fail(PF_ERR_ARG, "MFMA32 engine needs the operand image workspace (net_op)");
      if (p->mlp_dtype != PF_MLP_F32 && p->mlp_dtype != PF_MLP_BF16) return fail(PF_ERR_ARG, "mlp_dtype must be PF_MLP_F32 or PF_MLP_BF16");
    }
  }
  return PF_OK;
}

#define PF_WIDTH_SWITCH(PREFIX)                                   \
  switch (padded_width(p->net[which].width)) {                    \
    case 4: return PREFIX##4(p, which, s);                        \
    case 8: return PREFIX##8(p, which, s);                        \
    case 12: return PREFIX##12(p, which, s);                      \
    case 16: return PREFIX##16(p, which, s);                      \
    case 20: return PREFIX##20(p, which, s);                      \
    case 24: return PREFIX##24(p, which, s);                      \
    case 28: return PREFIX##28(p, which, s);                      \
    case 32: return PREFIX##32(p, which, s);                      \
  }                                                               \
  return fail(PF_ERR_UNSUPPORTED, "net width outside 1..32");

// MFMA32 engine: one translation unit per register bucket; the width of net NET picks it, the launcher gets the rest
#define PF_NR_SWITCH(PREFIX, NET, ...)                            \
  switch (pf_net32_bucket(p->net[NET].width)) {                   \
    case 2: return PREFIX##2(__VA_ARGS__);                        \
    case 4: return PREFIX##4(__VA_ARGS__);                        \
    case 6: return PREFIX##6(__VA_ARGS__);                        \
    case 8: return PREFIX##8(__VA_ARGS__);                        \
    case 10: return PREFIX##10(__VA_ARGS__);                      \
    case 12: return PREFIX##12(__VA_ARGS__);                      \
    case 15: return PREFIX##15(__VA_ARGS__);                      \
  }                                                               \
  return fail(PF_ERR_UNSUPPORTED, "MFMA32 engine: net width outside 1..30");

static int net_forward_impl(const pf_problem* p, int which, hipStream_t s, int s2_half);
// write_s == 0: this forward is followed by the other net's, which writes the stiffness records (pf_problem.elem_k).
// s2_half >= 0 (MFMA32 engine): the launch first runs the previous iteration's parameter update from that state half.
static int net_forward(const pf_problem* p, int which, hipStream_t s, int write_s = 1, int s2_half = -1) {
  if (write_s || !p->elem_k) return net_forward_impl(p, which, s, s2_half);
  pf_problem q = *p;
  q.elem_k = nullptr;
  return net_forward_impl(&q, which, s, s2_half);
}
static int net_forward_impl(const pf_problem* p, int which, hipStream_t s, int s2_half) {
  if (p->wg_mode == PF_WG_MFMA32 && p->mlp_dtype == PF_MLP_BF16) { PF_NR_SWITCH(pf_launch_net32b_forward_, which, p, which, s, s2_half) }
  if (p->wg_mode == PF_WG_MFMA32) { PF_NR_SWITCH(pf_launch_net32_forward_, which, p, which, s, s2_half) }
  if (s2_half >= 0) return fail(PF_ERR_ARG, "the fused parameter update exists in the MFMA32 engine only");
  if (p->wg_mode == PF_WG_MFMA44) { PF_WIDTH_SWITCH(pf_launch_net44_forward_) }
  PF_WIDTH_SWITCH(pf_launch_net_forward_)
}

// both nets in ONE launch (pf_net32.hip: k_net32_forward2) where the engine has it: MFMA32, both nets enabled, same
// number of hidden layers and inputs.
static bool can_fuse_forward(const pf_problem* p) {
  return p->wg_mode == PF_WG_MFMA32 && p->net[0].enabled && p->net[1].enabled &&
         p->net[0].n_hidden == p->net[1].n_hidden && p->net[0].in_dim == p->net[1].in_dim;
}
static int net_forward2(const pf_problem* p, hipStream_t s, const pf_fwd2_opts& o = pf_fwd2_opts()) {
  if (p->mlp_dtype == PF_MLP_BF16) { PF_NR_SWITCH(pf_launch_net32b_forward2_, 0, p, s, o) }
  PF_NR_SWITCH(pf_launch_net32_forward2_, 0, p, s, o)
}
// the forward pass of every enabled net: the properties and, with the MFMA32 engine, the stiffness records.
// s2_half >= 0: the FIRST launch also runs the parameter update of the previous iteration (graph_form.fuse_s2)
// o.gu_nb (only with graph_form.fuse_gu; fused launch only): see pf_fwd2_opts
static int net_forward_all(const pf_problem* p, hipStream_t s, const pf_fwd2_opts& o = pf_fwd2_opts()) {
  if (can_fuse_forward(p)) return net_forward2(p, s, o);
  int s2_half = o.s2_half >= 0 && o.calc_index ? o.s2_half + 2 : o.s2_half;      // (+ 2: see k_net32_forward)
  for (int k = 0; k < 2; ++k)
    if (p->net[k].enabled) {
      const int rc = net_forward(p, k, s, k == 1 || !p->net[1].enabled, s2_half);
      if (rc != PF_OK) return rc;
      s2_half = -1;
    }
  return PF_OK;
}

static int net_backward(const pf_problem* p, int which, hipStream_t s) {
  if (p->wg_mode == PF_WG_MFMA32 && p->mlp_dtype == PF_MLP_BF16) { PF_NR_SWITCH(pf_launch_net32b_backward_, which, p, which, s) }
  if (p->wg_mode == PF_WG_MFMA32) { PF_NR_SWITCH(pf_launch_net32_backward_, which, p, which, s) }
  if (p->wg_mode == PF_WG_MFMA44) { PF_WIDTH_SWITCH(pf_launch_net44_backward_) }
  PF_WIDTH_SWITCH(pf_launch_net_backward_)
}

// Is the element adjoint (dL/d(EA) per element) computed inside the first net's backward kernel?
static bool fuse_gea_for(const pf_problem* p) { return p->wg_mode == PF_WG_MFMA44 || p->wg_mode == PF_WG_MFMA32; }
// backward that also computes and stores the element adjoint g_ea
static int net_backward_gea(const pf_problem* p, int which, hipStream_t s) {
  if (p->wg_mode == PF_WG_MFMA32 && p->mlp_dtype == PF_MLP_BF16) { PF_NR_SWITCH(pf_launch_net32b_backward_gea_, which, p, which, s) }
  if (p->wg_mode == PF_WG_MFMA32) { PF_NR_SWITCH(pf_launch_net32_backward_gea_, which, p, which, s) }
  PF_WIDTH_SWITCH(pf_launch_net44_backward_gea_)
}

// both backward passes (the first with the fused element adjoint) in ONE launch, two phases (pf_net32.hip:
// k_net32_backward2).
static bool can_fuse_backward(const pf_problem* p) {
  return can_fuse_forward(p) && p->net[0].n_hidden == 2 && fuse_gea_for(p);
}
// path: the launch also forms r and g_f (the iteration graph's path form: graph_form.fold)
static int net_backward2(const pf_problem* p, hipStream_t s, int path = 0) {
  if (p->mlp_dtype == PF_MLP_BF16) { PF_NR_SWITCH(pf_launch_net32b_backward2_, 0, p, s, path) }
  PF_NR_SWITCH(pf_launch_net32_backward2_, 0, p, s, path)
}

#define PF_TRY(expr, what)                       \
  do {                                           \
    int rc__ = check_launch((expr), what);       \
    if (rc__ != PF_OK) return rc__;              \
  } while (0)

// element adjoint + backward of every enabled net (at least one): both nets in one launch where the engine has it, else
// one after the other with the adjoint fused into the first net's backward (fuse_gea_for) or in a launch of its own.
// adj_done (graph capture): recorded on `s` right behind the launch that computes the adjoint, the last reader of u.
static int enqueue_backwards(const pf_problem* p, hipStream_t s, hipEvent_t adj_done = nullptr) {
  auto mark = [&]() { return !adj_done || hipEventRecord(adj_done, s) == hipSuccess; };
  if (can_fuse_backward(p)) {
    PF_TRY(net_backward2(p, s), "net_backward2");
    return mark() ? PF_OK : fail(PF_ERR_HIP, "graph edge failed");
  }
  const bool fuse_gea = fuse_gea_for(p);
  const int first = p->net[0].enabled ? 0 : 1;
  if (!fuse_gea) {
    PF_TRY(pf_launch_elem_adjoint(p, s), "elem_adjoint");
    if (!mark()) return fail(PF_ERR_HIP, "graph edge failed");
  }
  for (int k = 0; k < 2; ++k) {
    if (!p->net[k].enabled) continue;
    PF_TRY(fuse_gea && k == first ? net_backward_gea(p, k, s) : net_backward(p, k, s), "net_backward");
    if (fuse_gea && k == first && !mark()) return fail(PF_ERR_HIP, "graph edge failed");
  }
  return PF_OK;
}

// The form of a problem's iteration graph (enqueue_graph_iterations): every decision that depends neither on the replay
// length nor on the pf_graph_create_ex flags.  pf_fusion_info, the pf_graph_* queries and the capture all read this record,
// so what is reported is what is captured.  (Comments in the kernel sources name three of its fields by the helpers they
// replace: can_fold_residual = fold, can_light_forward = light, can_fuse_gradu with elem_k and prop_double = fuse_gu.)
struct graph_form {
  bool any_net;      // a net is enabled (else the graph is the eager iteration, `iters` times)
  bool fwd2, bwd2;   // both nets in one forward / backward launch (can_fuse_forward, can_fuse_backward)
  bool fuse_s2;      // the forward launch of t+1 runs the parameter update of t: MFMA32 engine with the second state half
  bool fuse_gu;      // ... and the displacement update of t (dL/du + Adam(u) + clamp; pf_net32.hip: k_net32_forward2, gu_nb;
                     // pf_node.h): it reads the records of t = the other half, hence prop_double.  The graph is then ONE CHAIN
  bool dag;          // else, from PF_GRAPH_DAG_MIN_ELEMS elements on: the displacement update on the side branch
  bool u_alt;        // the second displacement vector is there (DAG: the ping-pong; PATH form: it holds r)
  bool fold;         // the PATH form, no residual launch.  graph_form_static: everything but the mesh allows it: wherever
                     // the forward launch carries both updates (so theta stage 1 is a launch of every iteration) and the
                     // backward is the fused two-phase launch with the path variant, on one GPU, with u_alt free to hold r.
                     // graph_form_probed: ... and the mesh is a path (mesh_is_path)
  bool ordered;      // PATH form whose node ids follow the path: node tasks without the adjacency (graph_form_probed)
  bool light;        // PATH form with the LIGHT forward (pf_net32.hip: k_net32_forward2 / backward_phase, LIGHT): the forward
                     // launch evaluates the E net only for the elements at task edges and the backward launch, which recomputes
                     // the E net's hidden layers anyway, stores prop_e and the other records.  forward(i) and backward(i)
                     // always complete together (the stop flag is only raised behind backward(i), in stage 1), and every
                     // reader of prop_e, prop_a and the records — forward(i+1)'s node tasks, the replay's tail,
                     // pf_graph_tail, a continuation head, the results — runs behind backward(i): it sees the bytes the full
                     // forward writes.  (static: where fold is static; probed: final)
  bool calc_index;   // the update prologue computes the padded-image index (pad_index_is_canonical; graph_form_probed)
  int tn_ready;      // k_theta_stage2 leaves the theta-norm monitor in the state (MFMA32 engine)
};

// The part of the record that needs no device work.  No HIP call: pf_fusion_info is answered from it outside any stream.
static graph_form graph_form_static(const pf_problem* p) {
  graph_form f = {};
  f.any_net = p->net[0].enabled || p->net[1].enabled;
  f.fwd2 = can_fuse_forward(p);
  f.bwd2 = can_fuse_backward(p);
  f.fuse_s2 = p->wg_mode == PF_WG_MFMA32 && p->theta_alt != nullptr && p->n_theta_active > 0 && f.any_net;
  f.fuse_gu = p->prop_double != 0 && p->elem_k != nullptr && f.fwd2 &&
              pf_n32_fwd2_can_update_u(p, pf_node_blocks(p->mesh.n_nodes));
  f.dag = !f.fuse_gu && p->mesh.n_elems >= PF_GRAPH_DAG_MIN_ELEMS;
  f.u_alt = p->u_alt != nullptr;
  f.fold = f.fuse_gu && f.u_alt && f.bwd2 && f.fuse_s2 && pf_n32_bwd2_has_path(p) && p->n_iface == 0 &&
           p->mesh.dim == p->net[0].in_dim - 1;
  f.light = f.fold && pf_n32_has_light_forward(p);      // (fold: both nets are enabled)
  f.tn_ready = p->wg_mode == PF_WG_MFMA32 ? 1 : 0;
  return f;
}

extern "C" {

int pf_abi_version(void) { return PF_ABI_VERSION; }
const char* pf_last_error(void) { return g_err; }

int pf_sizeof(int what) {
  switch (what) {
    case 0: return (int)sizeof(pf_mesh);
    case 1: return (int)sizeof(pf_net);
    case 2: return (int)sizeof(pf_state);
    case 3: return (int)sizeof(pf_problem);
    case 4: return (int)sizeof(pf_scalar_id);
    case 5: return (int)sizeof(pf_coarse);
    case 6: return (int)sizeof(pf_gl);
    case 7: return (int)sizeof(pf_dyn);
    case 8: return (int)sizeof(pf_gl_plastic);
  }
  return PF_ERR_ARG;
}

int pf_net_param_count(int in_dim, int width, int n_hidden) {
  if (in_dim < 1 || width < 1 || n_hidden < 1) return PF_ERR_ARG;
  return width * in_dim + width + (n_hidden - 1) * (width * width + width) + width + 1;
}

int pf_padded_width(int width) { return padded_width(width); }

int pf_net_pad_count(int in_dim, int width, int n_hidden) {
  const int hp = padded_width(width);
  if (hp < 0 || n_hidden < 1 || n_hidden > 3 || (in_dim != 2 && in_dim != 3)) return PF_ERR_UNSUPPORTED;
  return pf_pad_count(hp, n_hidden);
}

// padded-image index of torch parameter `local` (0-based inside the net's parameters() order)
int pf_net_pad_index(int in_dim, int width, int n_hidden, int local) {
  const int hp = padded_width(width);
  if (hp < 0 || n_hidden < 1 || n_hidden > 3 || (in_dim != 2 && in_dim != 3)) return PF_ERR_UNSUPPORTED;
  int q = local;
  if (q < 0) return PF_ERR_ARG;
  // W1 (width,in_dim), b1 (width)
  if (q < width * in_dim) return (q / in_dim) * 4 + (q % in_dim);
  q -= width * in_dim;
  if (q < width) return q * 4 + in_dim;
  q -= width;
  for (int l = 2; l <= n_hidden; ++l) {
    if (q < width * width) return pf_pad_wh(hp, l) + (q / width) * (hp + 4) + (q % width);
    q -= width * width;
    if (q < width) return pf_pad_wh(hp, l) + q * (hp + 4) + hp;
    q -= width;
  }
  if (q < width) return pf_pad_wo(hp, n_hidden) + q;
  q -= width;
  if (q == 0) return pf_pad_wo(hp, n_hidden) + hp;
  return PF_ERR_ARG;
}

int pf_net_op_count(int in_dim, int width, int n_hidden) {
  if (width < 1 || width > PF_N32_WIDTH_MAX || n_hidden < 1 || n_hidden > 3 || (in_dim != 2 && in_dim != 3))
    return PF_ERR_UNSUPPORTED;
  return (pf_n32_bytes(n_hidden) + 3) / 4;
}

long long pf_partials_count(const pf_problem* p) {
  if (!p) return PF_ERR_ARG;
  return (long long)PF_PART_WG + ((long long)p->n_part_blocks + PF_RG) * (long long)p->pad_total;
}

int pf_fusion_info(const pf_problem* p) {
  if (check_problem(p) != PF_OK) return PF_ERR_ARG;
  const graph_form f = graph_form_static(p);
  int m = 0;
  if (f.fwd2) m |= PF_FUSED_FORWARD;
  if (f.bwd2) m |= PF_FUSED_BACKWARD;
  if (f.fuse_s2) m |= PF_FUSED_THETA_UPDATE;
  if (f.fuse_gu) m |= PF_FUSED_U_UPDATE;
  if (f.dag && f.u_alt) m |= PF_FUSED_U_PINGPONG;
  return m;
}

int pf_pack_theta(const pf_problem* p, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  PF_TRY(pf_launch_pack_theta(p, (hipStream_t)stream), "pf_pack_theta");
  return PF_OK;
}

int pf_net_forward(const pf_problem* p, int which, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (which < 0 || which > 1 || !p->net[which].enabled) return fail(PF_ERR_ARG, "net not enabled");
  PF_TRY(net_forward(p, which, (hipStream_t)stream), "pf_net_forward");
  return PF_OK;
}

int pf_net_forward_all(const pf_problem* p, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  PF_TRY(net_forward_all(p, (hipStream_t)stream), "pf_net_forward_all");
  return PF_OK;
}

int pf_net_backward_all(const pf_problem* p, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!(p->net[0].enabled || p->net[1].enabled)) return PF_OK;
  return enqueue_backwards(p, (hipStream_t)stream);
}

int pf_internal_force(const pf_problem* p, const float* u, float* f_int_out, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!u || !f_int_out) return fail(PF_ERR_ARG, "null u / f_int_out");
  pf_problem q = *p;
  q.u = const_cast<float*>(u);
  PF_TRY(pf_launch_node_residual(&q, f_int_out, 0, (hipStream_t)stream), "pf_internal_force");
  return PF_OK;
}

int pf_node_residual(const pf_problem* p, float* f_int_out, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  PF_TRY(pf_launch_node_residual(p, f_int_out, 1, (hipStream_t)stream), "pf_node_residual");
  return PF_OK;
}

int pf_elem_adjoint(const pf_problem* p, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!p->g_ea) return fail(PF_ERR_ARG, "null g_ea");
  PF_TRY(pf_launch_elem_adjoint(p, (hipStream_t)stream), "pf_elem_adjoint");
  return PF_OK;
}

int pf_net_backward(const pf_problem* p, int which, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (which < 0 || which > 1 || !p->net[which].enabled) return fail(PF_ERR_ARG, "net not enabled");
  PF_TRY(net_backward(p, which, (hipStream_t)stream), "pf_net_backward");
  return PF_OK;
}

int pf_node_gradu(const pf_problem* p, int fuse_adam, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (fuse_adam && (!p->m_u || !p->v_u)) return fail(PF_ERR_ARG, "null Adam moments for u");
  if (!fuse_adam && !p->grad_u) return fail(PF_ERR_ARG, "grad_u required when Adam is not fused");
  PF_TRY(pf_launch_node_gradu(p, fuse_adam, (hipStream_t)stream), "pf_node_gradu");
  return PF_OK;
}

int pf_theta_reduce(const pf_problem* p, int fuse_adam, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (fuse_adam && p->n_theta_active > 0 && (!p->m_t || !p->v_t))
    return fail(PF_ERR_ARG, "null Adam moments for theta");
  PF_TRY(pf_launch_theta_reduce(p, fuse_adam, (hipStream_t)stream), "pf_theta_reduce");
  return PF_OK;
}

int pf_finalize(const pf_problem* p, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  PF_TRY(pf_launch_finalize(p, 0, 0, (hipStream_t)stream), "pf_finalize");
  return PF_OK;
}

int pf_reset(const pf_problem* p, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!p->m_u || !p->v_u) return fail(PF_ERR_ARG, "null Adam moments for u");
  if (p->n_theta > 0 && (!p->m_t || !p->v_t)) return fail(PF_ERR_ARG, "null Adam moments for theta");
  PF_TRY(pf_launch_reset(p, (hipStream_t)stream), "pf_reset");
  return PF_OK;
}

// kernel slots of one iteration, in launch order (also the index into pf_gd_iterations_timed's output)
enum { K_FWD_E = 0, K_FWD_A, K_RESIDUAL, K_ADJOINT, K_BWD_E, K_BWD_A, K_GRADU, K_THETA, K_FINALIZE, K_COUNT };

// ev: optional array of K_COUNT+1 events; ev[k] is recorded before slot k, ev[K_COUNT] at the end
static int enqueue_iteration(const pf_problem* p, int fuse_adam, int finalize_mode, hipStream_t s,
                             hipEvent_t* ev) {
  const bool any_net = p->net[0].enabled || p->net[1].enabled;
#define PF_MARK(k) do { if (ev && hipEventRecord(ev[k], s) != hipSuccess) return fail(PF_ERR_HIP, "hipEventRecord failed"); } while (0)
  PF_MARK(K_FWD_E);
  const bool fwd2 = can_fuse_forward(p);              // both nets in the first slot's launch; the second slot stays empty
  if (fwd2) PF_TRY(net_forward2(p, s), "net_forward2");
  else if (p->net[0].enabled) PF_TRY(net_forward(p, 0, s, !p->net[1].enabled), "net_forward");
  PF_MARK(K_FWD_A);
  if (!fwd2 && p->net[1].enabled) PF_TRY(net_forward(p, 1, s), "net_forward");
  PF_MARK(K_RESIDUAL);
  PF_TRY(pf_launch_node_residual(p, nullptr, 1, s), "node_residual");
  const bool fuse_gea = any_net && fuse_gea_for(p);
  const int first = p->net[0].enabled ? 0 : 1;
  PF_MARK(K_ADJOINT);
  if (any_net && !fuse_gea) PF_TRY(pf_launch_elem_adjoint(p, s), "elem_adjoint");
  PF_MARK(K_BWD_E);
  const bool bwd2 = can_fuse_backward(p);             // both nets in the first slot's launch; the second slot stays empty
  if (bwd2) PF_TRY(net_backward2(p, s), "net_backward2");
  else if (p->net[0].enabled)
    PF_TRY(fuse_gea && first == 0 ? net_backward_gea(p, 0, s) : net_backward(p, 0, s), "net_backward");
  PF_MARK(K_BWD_A);
  if (!bwd2 && p->net[1].enabled)
    PF_TRY(fuse_gea && first == 1 ? net_backward_gea(p, 1, s) : net_backward(p, 1, s), "net_backward");
  PF_MARK(K_GRADU);
  PF_TRY(pf_launch_node_gradu(p, fuse_adam, s), "node_gradu");
  PF_MARK(K_THETA);
  if (any_net) PF_TRY(pf_launch_theta_stage1(p, s), "theta_stage1");
  PF_MARK(K_FINALIZE);
  PF_TRY(pf_launch_finalize(p, finalize_mode, any_net ? 1 : 0, s), "finalize");
  PF_MARK(K_COUNT);
#undef PF_MARK
  return PF_OK;
}

static int check_gd(const pf_problem* p) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!p->m_u || !p->v_u) return fail(PF_ERR_ARG, "null Adam moments for u");
  if (p->n_theta_active > 0 && (!p->m_t || !p->v_t)) return fail(PF_ERR_ARG, "null Adam moments for theta");
  if (p->n_tensors > 64) return fail(PF_ERR_UNSUPPORTED, "more than 64 parameter tensors");   // PF_MAX_TENSORS (pf_mesh.hip)
  return PF_OK;
}

int pf_gd_iterations(const pf_problem* p, int n_iter, void* stream) {
  int rc = check_gd(p);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n_iter; ++i) {
    rc = enqueue_iteration(p, 1, 0, s, nullptr);
    if (rc) return rc;
  }
  return PF_OK;
}

// The iteration graph (pf_graph_create*): `iters` GD iterations captured on c.s, in one of two forms.
//
// ONE CHAIN (below PF_GRAPH_DAG_MIN_ELEMS elements, and wherever the forward launch can carry the displacement update):
// every launch on c.s, no events: forward, residual, backwards, theta stage 1, gradu.  The forward launch of iteration i
// also runs the parameter update of i-1 (graph_form.fuse_s2; fwd_theta_prologue) and, where it can, the displacement
// update of i-1 (dL/du + Adam(u) + clamp: graph_form.fuse_gu; it reads the stiffness records of i-1 = the other half, which is
// why it needs prop_double); node_residual's block 0 runs the bookkeeping of i-1 (pf_mesh.hip: k_node_residual,
// fin_prev) from the other half of the residual's partial sums (pf_problem.part_half).  Only the replay's last iteration
// keeps the stand-alone parameter and displacement updates, in place, and the bookkeeping follows as a launch of its own.
//
// DAG (the larger problems whose forward launch cannot carry the displacement update: one net, unequal depths, the
// non-MFMA32 engines): gradu runs on the side branch c.a.  What each kernel of iteration t really waits for:
//   forward (E and A in one launch)   the second-level gradient rows of t-1 [theta stage 1 of t-1]: its prologue IS the
//                       parameter update of t-1 (every block for itself; MFMA32 engine);  with prop_double nothing
//                       reads the properties or stiffness records of the other half any more, else [gradu of t-1]
//   node_residual       forward, u(t) [gradu of t-1]; its block 0 = finalize(t-1): the update of t-1, gradu of t-1, and the
//                       OTHER half of the residual's partial sums (part_half)
//   backward #1 (+gea)  g_f; it is the last reader of u(t)
//   gradu + Adam(u)     g_f, the stiffness records, backward #1 done; the Adam scalars          [finalize of t-1]
//   backward #2, theta stage 1   in this order after backward #1 (the last iteration of a replay: + the stand-alone update)
//   finalize(t)         the update and gradu of t: it runs inside node_residual(t+1)
// so gradu (HBM bound) runs beside backward #2 and the theta reduction (compute bound).  With the second displacement
// vector (pf_problem.u_alt, even replay length) the update of iteration i reads U[i & 1] like the residual and the element
// adjoint of i and WRITES U[(i + 1) & 1]: it forks right behind the residual and runs beside the whole backward launch.
// Without it, it forks behind the last read of u.  The runtime keeps the FIRST-created child of a node on its parent's
// hardware queue and moves later children to other queues; every fork or join on the main chain costs ~5 us (kernel
// trace).  So the side branch is created after the main chain's nodes of its iteration.
//
// The stop flag is read by every kernel at its start; a kernel of t+1 that misses a stop raised by finalize(t) only
// rewrites scratch (properties, g_f, partial sums): everything that changes solver state (both Adam kernels, the next
// finalize) is ordered behind finalize(t) and returns at once, so the final state is the reference's `break`.
#define PF_CAP_EV 2   /* pf_capture.ev per iteration: the last reader of u is done | gradu done */

// Does pf_problem.pad_index hold exactly what pf_pad_index_of computes (the layout pinn_fem_amd builds and INTEGRATION.md
// describes: nets in order, pf_net_pad_index + pad_off)?  Then the forward launch's update prologue computes the index
// instead of loading it.  One synchronous copy of the table, at graph creation only.
static bool pad_index_is_canonical(const pf_problem* p) {
  const int n = p->n_theta_active;
  if (n <= 0 || !p->pad_index) return false;
  int* h = new int[n];
  const bool ok = hipMemcpy(h, p->pad_index, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  bool same = ok;
  for (int q = 0; same && q < n; ++q) same = h[q] == pf_pad_index_of(*p, q);
  delete[] h;
  return same;
}

// Is the mesh an open path in element order: every node touches at most element e-1 at its j end and element e at its i end
// (node ids arbitrary)?  A ring, a shuffled element order, a girder, a hub or a mesh with dofs shared between ranks is not.
// Decided on the device (pf_mesh.hip: k_path_check; one flag, a 4-byte copy), at graph creation only: once per captured
// graph (a solve captures up to three), on the null stream — the mesh arrays are uploaded long before, and the synchronous
// copy orders the answer.  A failed allocation, launch or copy answers "not a path": the graph then keeps its residual launch,
// which is always correct; pf_last_error says so and pf_graph_form_info shows the form that was chosen.
// *ordered (where asked for): do the node ids follow the path as well, element e joining node e to node e + 1?  The same
// kernel, the same copy: the second bit of the flag.
static bool mesh_is_path(const pf_problem* p, bool* ordered = nullptr) {
  if (ordered) *ordered = false;
  const pf_mesh& M = p->mesh;
  if (M.n_elems < 1 || M.n_nodes != M.n_elems + 1 || !M.conn || !M.adj_ptr || !M.adj || !M.dof_flags) return false;
  int* bad = nullptr;
  if (hipMalloc(&bad, sizeof(int)) != hipSuccess) {
    pf_set_error("path check of the mesh failed (hipMalloc): the iteration graph keeps its residual launch");
    return false;
  }
  int h = 1;
  bool ok = hipMemset(bad, 0, sizeof(int)) == hipSuccess && pf_launch_path_check(p, bad, nullptr) == PF_OK &&
            hipMemcpy(&h, bad, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(bad);
  if (!ok) pf_set_error("path check of the mesh failed (HIP error): the iteration graph keeps its residual launch");
  if (ordered) *ordered = ok && h == 0;
  return ok && (h & 1) == 0;
}

// The whole record: the static part, completed by the probes.  No probe runs unless the static part already allows what it
// decides: one path probe where the path form is possible, one copy of the index table (with_index: graph creation) where the
// forward launch has the update prologue.  A failed probe answers "not a path" and leaves its message in pf_last_error.
static graph_form graph_form_probed(const pf_problem* p, bool with_index) {
  graph_form f = graph_form_static(p);
  f.calc_index = with_index && f.fuse_s2 && pad_index_is_canonical(p);
  bool ordered = false;
  f.fold = f.fold && mesh_is_path(p, &ordered);
  f.ordered = f.fold && ordered;
  f.light = f.light && f.fold;
  return f;
}

// The buffers iteration i of the graph works on.  Properties and stiffness records ping-pong between iterations
// (prop_double), so the forwards of iteration i do not wait for gradu(i-1), the last reader of the other half.  The
// residual's partial sums always do (part_half).
static pf_problem graph_iteration_view(const pf_problem& p, int i) {
  pf_problem q = p;
  if (p.prop_double != 0 && (i & 1)) {
    q.prop_e += q.mesh.n_elems;
    q.prop_a += q.mesh.n_elems;
    if (q.elem_k) q.elem_k += (size_t)q.mesh.n_elems * (q.mesh.dim == 2 ? 3 : 1);
  }
  q.part_half = i & 1;
  return q;
}

// head_cont: iteration 0 also carries the updates and the bookkeeping of the iteration BEFORE the replay (left pending by a
// no_tail replay); no_tail: the replay ends behind the last iteration's gradient-row reduction, its parameter update,
// displacement update and bookkeeping stay pending (pf_graph_create_ex).  Both only in the one-chain form.
//
// PATH form (graph_form.fold, decided at graph creation): THREE launches per iteration, forward -> backward -> theta
// stage 1.  The backward launch forms r and g_f of its elements' nodes itself (pf_net32.hip: backward_phase, PATH); the
// residual's loss sums and the bookkeeping of i-1 ride in the theta-stage-1 launch of i (pf_mesh.hip: k_theta_stage1_path),
// with the same partition and order of the sums, so nothing changes a bit.  The stop is then raised one launch later than
// above, behind backward(i) instead of beside residual(i): what backward(i) and stage 1(i) write before the flag is seen is
// scratch all the same (g_f, r in u_alt, g_ea, gradient rows, partial sums of the half nobody will read), and every
// state-changing step — the updates inside forward(i+1), or the replay's stand-alone tail — still starts behind stage 1(i),
// reads the flag first and returns at once.
static int enqueue_graph_iterations(const pf_problem* p, int iters, const pf_capture& c, const graph_form& f, int flags) {
  hipStream_t s = c.s;
  if (!f.any_net) {
    for (int i = 0; i < iters; ++i) {
      int rc = enqueue_iteration(p, 1, 0, s, nullptr);
      if (rc != PF_OK) return rc;
    }
    return PF_OK;
  }
  const bool head_cont = (flags & PF_GRAPH_CONT_HEAD) != 0, no_tail = (flags & PF_GRAPH_NO_TAIL) != 0;
  const bool fuse_gu = f.fuse_gu, dag = f.dag, fuse_s2 = f.fuse_s2, fold = f.fold, light = f.light;
  const bool upp = dag && f.u_alt && (iters % 2) == 0;                // DAG with the second displacement vector
  const int tn_ready = f.tn_ready;
  const size_t k_half = (size_t)p->mesh.n_elems * (p->mesh.dim == 2 ? 3 : 1);   // floats of one half of the records
  for (int i = 0; i < iters; ++i) {
    hipEvent_t* e = c.ev + PF_CAP_EV * i;
    hipEvent_t* ep = c.ev + PF_CAP_EV * (i - 1);
    pf_problem q = graph_iteration_view(*p, i);
    float* u_next = nullptr;
    if (upp) {
      u_next = (i & 1) ? q.u : q.u_alt;
      if (i & 1) q.u = q.u_alt;                       // what this iteration's kernels READ
    }
    const bool carries = i > 0 || head_cont;      // this iteration's forward / residual carry the previous iteration's work
    pf_fwd2_opts fo;
    if (fuse_s2 && carries) fo.s2_half = (i - 1) & 1;       // (i = 0 in a continuation: the previous replay's last = half 1)
    fo.calc_index = f.calc_index;
    if (fuse_gu && carries) {
      fo.gu_nb = pf_node_blocks(q.mesh.n_nodes);
      fo.gu_k = p->elem_k + (((i - 1) & 1) ? k_half : 0);   // the records iteration i-1 wrote (the other half)
      fo.gu_ordered = f.ordered ? 1 : 0;                    // (the path form with node ids in path order: no adjacency)
    }
    // (DAG without the second property half: the forwards wait for gradu(i-1), an 11 us hole in the kernel trace)
    if (dag && i > 0 && p->prop_double == 0 && hipStreamWaitEvent(s, ep[1], 0) != hipSuccess)
      return fail(PF_ERR_HIP, "graph edge failed");
    // (both nets in one launch where the engine has it; else one after the other: side by side on two branches they
    // measured slower, the same issue pipe, and the second one writes the stiffness records from both)
    fo.light = light ? 1 : 0;
    PF_TRY(net_forward_all(&q, s, fo), "net_forward");
    if (fold) {
      PF_TRY(net_backward2(&q, s, light ? 2 : 1), "net_backward2");
      PF_TRY(pf_launch_theta_stage1_path(&q, s, carries ? (tn_ready ? 2 : 1) : 0), "theta_stage1");
      if (i == iters - 1 && !no_tail) {
        PF_TRY(pf_launch_theta_stage2(&q, 1, s), "theta_stage2");
        PF_TRY(pf_launch_node_gradu(&q, 1, s, 0, nullptr), "node_gradu");
      }
      continue;
    }
    // residual(i) reads u(i) [gradu(i-1)]; its block 0 is finalize(i-1): behind the theta update of i-1 (this chain:
    // the forward launch above, or the stand-alone kernel) and gradu(i-1)
    if (dag && i > 0 && hipStreamWaitEvent(s, ep[1], 0) != hipSuccess) return fail(PF_ERR_HIP, "graph edge failed");
    PF_TRY(pf_launch_node_residual(&q, nullptr, 1, s, carries ? (tn_ready ? 2 : 1) : 0), "node_residual");
    if (upp && hipEventRecord(e[0], s) != hipSuccess) return fail(PF_ERR_HIP, "graph edge failed");   // gradu forks here
    if (const int rc = enqueue_backwards(&q, s, dag && !upp ? e[0] : nullptr)) return rc;   // (... or here)
    PF_TRY(pf_launch_theta_stage1(&q, s), "theta_stage1");
    if (!fuse_s2 || (i == iters - 1 && !no_tail)) PF_TRY(pf_launch_theta_stage2(&q, 1, s), "theta_stage2");
    if (!dag) {
      if (!fuse_gu || (i == iters - 1 && !no_tail)) PF_TRY(pf_launch_node_gradu(&q, 1, s, 0, nullptr), "node_gradu");
      continue;                                   // (else the next forward launch carries it)
    }
    // side branch: gradu behind the last reader of u
    if (hipStreamWaitEvent(c.a, e[0], 0) != hipSuccess) return fail(PF_ERR_HIP, "graph edge failed");
    PF_TRY(pf_launch_node_gradu(&q, 1, c.a, 0, u_next), "node_gradu");
    if (hipEventRecord(e[1], c.a) != hipSuccess) return fail(PF_ERR_HIP, "graph edge failed");
  }
  // finalize of the last iteration: behind stage 2 (this chain) and the last gradu
  if (no_tail) return PF_OK;
  if (dag && hipStreamWaitEvent(s, c.ev[PF_CAP_EV * (iters - 1) + 1], 0) != hipSuccess)
    return fail(PF_ERR_HIP, "graph join failed");
  if (upp) PF_TRY(pf_launch_u_home(p, s), "u_home");      // (only a stop in mid-replay leaves anything to copy)
  pf_problem q = *p;
  q.part_half = (iters - 1) & 1;
  PF_TRY(pf_launch_finalize(&q, 0, 0, s, tn_ready), "finalize");
  return PF_OK;
}

int pf_graph_form_info(const pf_problem* p) {
  if (check_problem(p) != PF_OK) return PF_ERR_ARG;
  return graph_form_probed(p, false).fold ? PF_GRAPH_FORM_FOLDED_RESIDUAL : 0;
}

int pf_graph_light_forward(const pf_problem* p) {
  if (check_problem(p) != PF_OK) return PF_ERR_ARG;
  return graph_form_probed(p, false).light ? 1 : 0;
}

int pf_graph_ordered_path(const pf_problem* p) {
  if (check_problem(p) != PF_OK) return PF_ERR_ARG;
  return graph_form_probed(p, false).ordered ? 1 : 0;
}

int pf_graph_create(const pf_problem* p, int iters_per_graph, void* stream, void** graph_out) {
  return pf_graph_create_ex(p, iters_per_graph, 0, stream, graph_out);
}

// can the iteration graph of this form be cut into replays that hand their last iteration's updates to the next one?
static bool can_chain_replays(const graph_form& f, int iters) { return (iters % 2) == 0 && f.fuse_gu && f.fuse_s2; }

int pf_graph_create_ex(const pf_problem* p, int iters_per_graph, int flags, void* stream, void** graph_out) {
  int rc = check_gd(p);
  if (rc) return rc;
  if (!graph_out || iters_per_graph < 1) return fail(PF_ERR_ARG, "pf_graph_create_ex: bad argument");
  if ((flags & (PF_GRAPH_CONT_HEAD | PF_GRAPH_NO_TAIL)) && !can_chain_replays(graph_form_static(p), iters_per_graph))
    return fail(PF_ERR_UNSUPPORTED, "pf_graph_create_ex: replays of this problem's graph cannot hand over their tail");
  const graph_form f = graph_form_probed(p, true);
  return capture_graph((hipStream_t)stream, PF_CAP_EV * iters_per_graph, hipStreamCaptureModeThreadLocal, graph_out,
                       [&](pf_capture& cap) { return enqueue_graph_iterations(p, iters_per_graph, cap, f, flags); });
}

// the pending tail of a PF_GRAPH_NO_TAIL replay: what the last iteration of a plain replay ends with
int pf_graph_tail(const pf_problem* p, int iters_per_graph, void* stream) {
  int rc = check_gd(p);
  if (rc) return rc;
  const graph_form f = graph_form_static(p);
  if (!can_chain_replays(f, iters_per_graph)) return fail(PF_ERR_UNSUPPORTED, "pf_graph_tail: not a chained replay");
  hipStream_t s = (hipStream_t)stream;
  const pf_problem q = graph_iteration_view(*p, iters_per_graph - 1);   // the last iteration's halves
  PF_TRY(pf_launch_theta_stage2(&q, 1, s), "theta_stage2");
  PF_TRY(pf_launch_node_gradu(&q, 1, s, 0, nullptr), "node_gradu");
  PF_TRY(pf_launch_finalize(&q, 0, 0, s, f.tn_ready), "finalize");
  return PF_OK;
}

int pf_graph_launch(void* graph, void* stream) {
  if (!graph) return fail(PF_ERR_ARG, "null graph");
  if (hipGraphLaunch((hipGraphExec_t)graph, (hipStream_t)stream) != hipSuccess)
    return fail(PF_ERR_HIP, "hipGraphLaunch failed");
  return PF_OK;
}

int pf_graph_destroy(void* graph) {
  if (!graph) return PF_OK;
  if (hipGraphExecDestroy((hipGraphExec_t)graph) != hipSuccess) return fail(PF_ERR_HIP, "hipGraphExecDestroy failed");
  return PF_OK;
}

int pf_gd_iterations_timed(const pf_problem* p, int n_iter, void* stream, float* ms_per_kernel) {
  int rc = check_gd(p);
  if (rc) return rc;
  if (!ms_per_kernel || n_iter < 1) return fail(PF_ERR_ARG, "pf_gd_iterations_timed: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int per = K_COUNT + 1;
  hipEvent_t* ev = new hipEvent_t[(size_t)n_iter * per];
  int made = 0;
  for (; made < n_iter * per; ++made)
    if (hipEventCreate(&ev[made]) != hipSuccess) break;
  rc = made == n_iter * per ? PF_OK : fail(PF_ERR_HIP, "hipEventCreate failed");
  for (int i = 0; rc == PF_OK && i < n_iter; ++i) rc = enqueue_iteration(p, 1, 0, s, ev + (size_t)i * per);
  if (rc == PF_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(PF_ERR_HIP, "hipStreamSynchronize failed");
  if (rc == PF_OK) {
    for (int k = 0; k < K_COUNT; ++k) ms_per_kernel[k] = 0.f;
    for (int i = 0; i < n_iter; ++i)
      for (int k = 0; k < K_COUNT; ++k) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[(size_t)i * per + k], ev[(size_t)i * per + k + 1]) != hipSuccess) {
          rc = fail(PF_ERR_HIP, "hipEventElapsedTime failed");
          break;
        }
        ms_per_kernel[k] += ms;
      }
    for (int k = 0; k < K_COUNT; ++k) ms_per_kernel[k] /= (float)n_iter;
  }
  for (int i = 0; i < made; ++i) hipEventDestroy(ev[i]);
  delete[] ev;
  return rc;
}

int pf_loss_and_grads(const pf_problem* p, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!p->grad_u) return fail(PF_ERR_ARG, "grad_u required");
  return enqueue_iteration(p, 0, 1, (hipStream_t)stream, nullptr);
}

static int check_shared(const pf_problem* p) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (p->n_shared < 0 || p->n_iface < p->n_shared) return fail(PF_ERR_ARG, "bad interface sizes");
  if (p->n_shared > 0 && (!p->shared_dofs || !p->shared_slot)) return fail(PF_ERR_ARG, "null interface maps");
  if (p->own_lo < 0 || p->own_hi < p->own_lo || p->own_hi > p->mesh.n_elems) return fail(PF_ERR_ARG, "bad own element range");
  return PF_OK;
}

// The own elements as a problem of their own: the element-indexed arrays start at own_lo (node ids in the
// connectivity are untouched), so the element-parallel kernels run on exactly the range whose gradients this rank owns.
static pf_problem own_view(const pf_problem* p) {
  pf_problem q = *p;
  if (p->own_hi > 0) {
    const int lo = p->own_lo;
    q.mesh.conn += 2 * (size_t)lo;
    q.mesh.egeo += 4 * (size_t)lo;
    q.mesh.ecent += (size_t)p->mesh.dim * lo;
    if (q.prop_e) q.prop_e += lo;
    if (q.prop_a) q.prop_a += lo;
    if (q.g_ea) q.g_ea += lo;
    if (q.elem_k) q.elem_k += (size_t)lo * (p->mesh.dim == 2 ? 3 : 1);
    q.mesh.n_elems = p->own_hi - lo;
  }
  return q;
}

int pf_shard_forward(const pf_problem* p, void* stream) {
  int rc = check_shared(p);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  PF_TRY(net_forward_all(p, s), "net_forward");
  return PF_OK;
}

int pf_shard_backward(const pf_problem* p, float* buf, const float* u2_local, void* stream) {
  int rc = check_shared(p);
  if (rc) return rc;
  if (!buf || !u2_local) return fail(PF_ERR_ARG, "null buf / u2_local");
  if (p->n_theta_active > 0 && p->grad_theta != buf + p->n_iface)
    return fail(PF_ERR_ARG, "p->grad_theta must point at buf + n_iface");
  hipStream_t s = (hipStream_t)stream;
  const bool any_net = p->net[0].enabled || p->net[1].enabled;
  PF_TRY(pf_launch_node_residual(p, nullptr, 1, s), "node_residual");
  if (any_net) {
    const pf_problem q = own_view(p);
    rc = enqueue_backwards(&q, s);
    if (rc) return rc;
    PF_TRY(pf_launch_theta_stage1(&q, s), "theta_stage1");
  }
  PF_TRY(pf_launch_shard_pack(p, buf, u2_local, s), "shard_pack");
  return PF_OK;
}

int pf_shard_update_interior(const pf_problem* p, void* stream) {
  int rc = check_shared(p);
  if (rc) return rc;
  if (!p->m_u || !p->v_u) return fail(PF_ERR_ARG, "null Adam moments for u");
  PF_TRY(pf_launch_node_gradu(p, 1, (hipStream_t)stream, 1), "node_gradu");
  return PF_OK;
}

}  // extern "C"
// `iters` complete sharded iterations as ONE hipGraph, the collective included (all_reduce: the caller's, captured on
// the main stream like a kernel).  Per iteration: forwards, residual, first backward -> [fork: gradu of the interior
// dofs] -> second backward, theta stage 1, pack -> all-reduce(buf) -> [join] -> interface update + bookkeeping; i.e.
// the single-engine iteration's shape with the collective on the chain and gradu hidden beside the second backward
// and the collective.  Internal (pf_comm.hip: pf_shard_graph_create).
int pf_shard_graph_capture(const pf_problem* p, int iters, float* buf, float* u2_local, hipStream_t stream,
                           int (*all_reduce)(void* ctx, float* buf, size_t n, hipStream_t s), void* ctx, void** graph_out) {
  int rc = check_shared(p);
  if (rc) return rc;
  if (!buf || !u2_local || !graph_out || !all_reduce || iters < 1 || !p->m_u || !p->v_u)
    return fail(PF_ERR_ARG, "pf_shard_graph_capture: bad argument");
  if (p->n_theta_active > 0 && (p->grad_theta != buf + p->n_iface || !p->m_t || !p->v_t))
    return fail(PF_ERR_ARG, "p->grad_theta must point at buf + n_iface (and the theta moments must exist)");
  const size_t n = (size_t)p->n_iface + (size_t)p->n_theta_active + 3;
  // relaxed capture mode: the collective library may call into the runtime while it enqueues
  return capture_graph(stream, 2 * iters, hipStreamCaptureModeRelaxed, graph_out, [&](pf_capture& c) -> int {
    hipStream_t s = c.s;
    const bool any_net = p->net[0].enabled || p->net[1].enabled;
    for (int i = 0; i < iters; ++i) {
      hipEvent_t* e = c.ev + 2 * i;
      PF_TRY(net_forward_all(p, s), "net_forward");
      PF_TRY(pf_launch_node_residual(p, nullptr, 1, s), "node_residual");
      // e[0]: the last reader of u (the element adjoint) is done
      if (any_net) {
        const pf_problem q = own_view(p);
        if (const int rb = enqueue_backwards(&q, s, e[0])) return rb;
        PF_TRY(pf_launch_theta_stage1(&q, s), "theta_stage1");
      } else if (hipEventRecord(e[0], s) != hipSuccess) {
        return fail(PF_ERR_HIP, "graph edge failed");
      }
      PF_TRY(pf_launch_shard_pack(p, buf, u2_local, s), "shard_pack");
      // the side branch is created AFTER the chain's nodes of this iteration: the runtime keeps the first-created child of
      // a node on its parent's hardware queue, and the chain must be the one that stays (pf_graph_create, same rule)
      if (hipStreamWaitEvent(c.a, e[0], 0) != hipSuccess) return fail(PF_ERR_HIP, "graph edge failed");
      PF_TRY(pf_launch_node_gradu(p, 1, c.a, 1), "node_gradu");
      if (hipEventRecord(e[1], c.a) != hipSuccess) return fail(PF_ERR_HIP, "graph edge failed");
      int r3 = all_reduce(ctx, buf, n, s);
      if (r3 != PF_OK) return r3;
      if (hipStreamWaitEvent(s, e[1], 0) != hipSuccess) return fail(PF_ERR_HIP, "graph join failed");
      PF_TRY(pf_launch_shard_update(p, buf, u2_local, s), "shard_update");
    }
    return PF_OK;
  });
}
extern "C" {

int pf_shard_update_shared(const pf_problem* p, const float* buf, float* u2_local, void* stream) {
  int rc = check_shared(p);
  if (rc) return rc;
  if (!buf || !u2_local || !p->m_u || !p->v_u) return fail(PF_ERR_ARG, "null buffer");
  if (p->n_theta_active > 0 && (!p->m_t || !p->v_t)) return fail(PF_ERR_ARG, "null Adam moments for theta");
  hipStream_t s = (hipStream_t)stream;
  PF_TRY(pf_launch_shard_update(p, buf, u2_local, s), "shard_update");   // (includes the iteration's bookkeeping)
  return PF_OK;
}

int pf_shard_flush(const pf_problem* p, const float* u2_reduced, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!u2_reduced) return fail(PF_ERR_ARG, "null u2");
  PF_TRY(pf_launch_shard_flush(p, u2_reduced, (hipStream_t)stream), "shard_flush");
  return PF_OK;
}

}  // extern "C"
extern "C" {

int pf_scalar_gd_iterations(const pf_problem* p, const pf_scalar_id* sp, int n_iter, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!sp || !sp->p || !sp->m_p || !sp->v_p || n_iter < 0 || (sp->n_rows > 0 && !sp->table))
    return fail(PF_ERR_ARG, "pf_scalar_gd_iterations: bad argument");
  if (p->net[0].enabled || p->net[1].enabled) return fail(PF_ERR_ARG, "pf_scalar_gd_iterations: scalar materials only");
  if (!p->m_u || !p->v_u || !(sp->n_free_f > 0.f)) return fail(PF_ERR_ARG, "pf_scalar_gd_iterations: missing state");
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n_iter; ++i) {
    PF_TRY(pf_launch_scalar_residual(p, sp, s), "scalar_residual");
    PF_TRY(pf_launch_node_gradu(p, 1, s), "node_gradu");
    PF_TRY(pf_launch_scalar_update(p, sp, s), "scalar_update");
  }
  return PF_OK;
}

int pf_adam(float* param, const float* grad, float* m, float* v, int n, int step, double lr,
            double beta1, double beta2, double eps, void* stream) {
  if (!param || !grad || !m || !v || n < 0 || step < 1) return fail(PF_ERR_ARG, "pf_adam: bad argument");
  PF_TRY(pf_launch_adam(param, grad, m, v, n, step, lr, beta1, beta2, eps, (hipStream_t)stream), "pf_adam");
  return PF_OK;
}

int pf_diag_k(const pf_problem* p, float* diag_out, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!diag_out) return fail(PF_ERR_ARG, "null diag_out");
  PF_TRY(pf_launch_diag_k(p, diag_out, (hipStream_t)stream), "pf_diag_k");
  return PF_OK;
}

int pf_coo_k(const pf_problem* p, long long* rows_out, long long* cols_out, float* vals_out, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!rows_out || !cols_out || !vals_out) return fail(PF_ERR_ARG, "null COO output");
  PF_TRY(pf_launch_coo_k(p, rows_out, cols_out, vals_out, (hipStream_t)stream), "pf_coo_k");
  return PF_OK;
}

int pf_dense_k(const pf_problem* p, float* k_out, void* stream) {
  int rc = check_problem(p);
  if (rc) return rc;
  if (!k_out) return fail(PF_ERR_ARG, "null k_out");
  if (p->mesh.n_dofs > 4096) return fail(PF_ERR_ARG, "dense K is a small-problem view (n_dofs <= 4096)");
  PF_TRY(pf_launch_dense_k(p, k_out, (hipStream_t)stream), "pf_dense_k");
  return PF_OK;
}

}  // extern "C"
