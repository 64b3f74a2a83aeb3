/*
 * pinnfem_hip.h — C ABI of libpinnfem_hip.so (gfx950 / MI355X).
 *
 * The library is the hand-written HIP implementation of ONE path of the reference
 * (rpacheco-blazquez/PINN-FEM): the body of the PINN+GD iteration
 *     assemble_system_torch -> residual/loss -> loss.backward() -> Adam(u), Adam(theta)
 *     -> BC clamp -> monitors/stop test          (FEM/python/fem/solver.py:252-355)
 * The reference has no native code and no FFI; every entry point below names the Python
 * lines it replaces.  A Python binding (ctypes) is in pinn_fem_amd/_capi.py and the stub a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every pointer marked "dev" is a DEVICE pointer owned by the caller
 *     (PyTorch's allocator in our host code); the library allocates nothing and keeps no
 *     state between calls, so every call is re-entrant and graph-capturable;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work (no sync);
 *   - return value: 0 = ok, <0 = error (see pf_last_error()); no exceptions cross the ABI;
 *   - all floating point is IEEE float32 unless a field says double.
 */
#ifndef PINNFEM_HIP_H
#define PINNFEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9 still covers pf_coarse_setup_t, pf_pcg2t_*, pf_pcgtm_* and pf_pcg2tm_*: they are additive (new symbols only, no struct or signature changed), so
 * a binding built against the earlier 9 keeps working; a binding that needs them finds them by name */
#define PF_ABI_VERSION 9

/* error codes */
#define PF_OK 0
#define PF_ERR_ARG (-1)          /* bad argument / inconsistent sizes */
#define PF_ERR_UNSUPPORTED (-2)  /* net shape outside the compiled menu */
#define PF_ERR_HIP (-3)          /* a HIP runtime call failed */

/* dof flag bits (pf_mesh.dof_flags) */
#define PF_DOF_FIXED 1u
#define PF_DOF_MEASURED 2u
#define PF_DOF_SHARED 4u   /* dof of a node that also belongs to another rank's shard (multi-GPU) */
#define PF_DOF_GHOST 8u    /* shared and owned by another rank: excluded from this rank's global sums */

/* MLP engines (pf_problem.wg_mode) */
#define PF_WG_SHUFFLE 0 /* VALU mat-vecs, weight gradients by wave shuffles (slow cross-check) */
#define PF_WG_MFMA 1    /* VALU mat-vecs, weight gradients on v_mfma_f32_16x16x4_f32 (LDS tiles) */
#define PF_WG_MFMA44 2  /* everything on v_mfma_f32_4x4x1_16B_f32, one element per lane (exact f32 fma chains) */
#define PF_WG_MFMA32 3  /* v_mfma_f32_32x32x16_f16 with 2-way split operands (f32-grade products on the f16 matrix
                           cores; default for widths <= PF_N32_WIDTH_MAX) */
#define PF_N32_WIDTH_MAX 30
#define PF_MLP_F32 0
#define PF_MLP_BF16 1

/* element-force formulations */
#define PF_FE_REFERENCE 0 /* 4-term dot per row, the reference's order (nn_assembly.py:96-100) */
#define PF_FE_DELTA 1     /* on d = u_j - u_i: same algebra, no float32 cancellation (opt-in) */

/* Mesh-derived immutable data ("plan").  Replaces the per-iteration Python work of
 * fem/nn_assembly.py:181-205 (dof numbering, centroid, direction cosines) and
 * fem/boundary.py:8-13 (free/fixed partition).  All arrays dev. */
typedef struct pf_mesh {
  int32_t dim;             /* 1 (nn_assembly.py:129-179) or 2 (:181-229) */
  int32_t n_nodes;
  int32_t n_elems;
  int32_t n_dofs;          /* n_nodes*dim */
  const int32_t* conn;     /* [n_elems][2] node ids (i,j) */
  const float* egeo;       /* [n_elems][4] = c2, cs, s2, l0  (float32 of the float64 values the
                              reference computes, nn_assembly.py:64-82; 1-D: 1,0,0,|dx|) */
  const float* ecent;      /* [n_elems][dim] centroid = NN input columns after load_factor */
  const int32_t* adj_ptr;  /* [n_nodes+1] CSR node -> incident elements, ascending element id */
  const int32_t* adj;      /* [adj_ptr[n_nodes]] entries (elem<<1)|end, end=0: node is i */
  const float* f_ext;      /* [n_dofs] external loads (solver.py:218) */
  const uint8_t* dof_flags;/* [n_dofs] PF_DOF_* */
  const float* meas_val;   /* [n_dofs] measured displacement where PF_DOF_MEASURED */
  int32_t n_meas;          /* number of measurements m (denominator of the mean, solver.py:275) */
  int32_t _pad;
} pf_mesh;

/* One material property: constant, or MLP(load_factor, x[, y]) -> softplus -> *scale
 * (fem/properties.py:97-161, examples/json/generic.py:118-142). */
typedef struct pf_net {
  int32_t enabled;     /* 0: constant property = scale */
  int32_t in_dim;      /* must be mesh.dim+1: columns [load_factor, x(, y)] (properties.py:119) */
  int32_t width;       /* hidden width h (1..32) */
  int32_t n_hidden;    /* hidden layers (1..3) */
  int32_t positive;    /* softplus on the output (enforce_positive) */
  float scale;         /* output scale = base property value */
  int32_t theta_off;   /* offset of this net's first parameter in the flat theta vector */
  int32_t pad_off;     /* offset of this net in the padded-parameter workspace */
} pf_net;

/* Device-resident iteration state; written only by kernels.  One per solve_gd call. */
typedef struct pf_state {
  int32_t iter;        /* completed iterations (= Adam step count) */
  int32_t done;        /* 1 once the stop test fired (solver.py:341-355); later launches no-op */
  int32_t converged;   /* same as done (kept separate for max_iterations exits) */
  int32_t theta_half;  /* which half holds the current theta / Adam moments: 0 = p->theta, m_t, v_t; 1 = p->theta_alt
                          (only the iteration graph ever leaves it at 1, and only between its own kernels) */
  /* Adam scalars for the NEXT step, computed in double like torch does on the host */
  float step_size_u, step_size_t, bc2_sqrt, _pad2;
  /* last iteration's monitors (solver.py:304-320) */
  float loss_total, loss_physics, loss_data, u_norm, residual_norm, theta_norm;
  int32_t u_half;      /* 1: the current displacements are in p->u_alt (only between the kernels of an iteration graph) */
  float _pad3;
} pf_state;

#define PF_HIST_COLS 6 /* loss_total, loss_physics, loss_data, u_norm, residual_norm, theta_norm */

/* Everything one GD iteration touches.  Filled by the host once per solve_gd call. */
typedef struct pf_problem {
  pf_mesh mesh;
  pf_net net[2];           /* 0: young, 1: area (density is never evaluated, nn_assembly.py:207) */
  /* unknowns + Adam moments (solver.py:205-216, 234-236); all dev */
  float* u;                /* [n_dofs] */
  float* m_u;
  float* v_u;
  float* theta;            /* [n_theta] flat, torch parameters() order young->area->density */
  float* m_t;
  float* v_t;
  int32_t n_theta;         /* all parameters incl. density net */
  int32_t n_theta_active;  /* leading parameters that receive gradients (young+area nets) */
  const int32_t* tensor_off; /* dev [n_tensors+1] parameter-tensor boundaries for theta_norm */
  int32_t n_tensors;
  int32_t wg_mode;         /* PF_WG_* : which MLP engine runs the net kernels */
  /* scalars of SolverConfig (solver.py:35-62) */
  float lam;               /* load factor of this increment */
  float alpha_physics, alpha_data;
  float lr_u, lr_t;
  double tol;
  double beta1, beta2, eps;
  int32_t use_data;        /* has_measurements && alpha_data>0 (solver.py:273) */
  int32_t max_iter;
  /* workspaces, all dev; sizes: theta_pad pf_net_pad_count() per net, partials pf_partials_count() */
  float* theta_pad;        /* padded parameter image the net kernels read */
  float* prop_e;           /* [n_elems] young per element */
  float* prop_a;           /* [n_elems] area per element */
  float* g_f;              /* [n_dofs] dL/df_int (alpha_p*r on free dofs, 0 on fixed) */
  float* g_ea;             /* [n_elems] dL/d(E*A) per element */
  float* grad_u;           /* [n_dofs] or NULL (only needed by the autograd binding) */
  float* grad_theta;       /* [n_theta] reduced parameter gradient */
  float* partials;         /* block partial sums (scalars + padded weight gradients) */
  float* hist;             /* [max_iter][PF_HIST_COLS] per-iteration monitors */
  pf_state* state;
  int32_t n_part_blocks;   /* grid size used for partial sums (host picks, <= PF_MAX_BLOCKS) */
  int32_t pad_total;       /* floats of the padded-parameter image of all active nets */
  const int32_t* pad_index;/* dev [n_theta_active] torch-layout index -> padded-image index */
  float n_meas_f;          /* (float)mesh.n_meas; multi-GPU: the GLOBAL count */
  int32_t fe_mode;         /* PF_FE_* : how fe = ke @ u_e is evaluated */
  /* multi-GPU shard interface (NULL / 0 on one GPU): the dofs of this rank's INTERFACE nodes = nodes shared with
   * other ranks plus the other nodes of the elements around them (ghost nodes here, or boundary-near nodes of which
   * another rank holds a ghost copy).  Their grad_u is completed by the iteration's all-reduce. */
  const int32_t* shared_dofs; /* dev [n_shared] local dof index */
  const int32_t* shared_slot; /* dev [n_shared] position in the global interface vector */
  int32_t n_shared;
  int32_t n_iface;         /* length of the global interface vector */
  /* multi-GPU: the local mesh = this rank's OWN elements plus the ghost elements (other ranks' elements incident to a
   * shared node), sorted by global id, so the own elements are the local range [own_lo, own_hi); 0, 0 on one GPU.
   * Gradients (MLP backward, grad_u) are taken over the own elements only. */
  int32_t own_lo, own_hi;
  int32_t part_half;        /* 0|1: which half of the residual's block partial sums this launch writes / the stand-alone
                               pf_finalize reads (0 unless the caller pipelines finalize into the next residual) */
  /* != 0: prop_e and prop_a hold 2*n_elems floats; the iteration graph then alternates between the two
   * halves, so the forwards of iteration t+1 need not wait for the last reader of iteration t's properties */
  int32_t prop_double;
  /* MFMA32 engine: split-f16 operand image of the enabled nets (pf_net_op_count() floats each, at op_off[k]),
   * rebuilt from theta by pf_pack_theta and by every theta update; NULL unless wg_mode == PF_WG_MFMA32 */
  float* net_op;
  int32_t op_off[2];
  /* 2^coord_exp * max |centroid coordinate| <= 2^14: scale of the coordinates inside the f16 gradient products */
  int32_t coord_exp;
  /* MFMA32 engine, precision of the hidden-layer and gradient matrix products: PF_MLP_F32 (2-way split f16
   * operands, float32-grade; default) or PF_MLP_BF16 (plain bf16 operands, f32 accumulate) */
  int32_t mlp_dtype;
  /* per element, the three distinct entries of ke = s*pattern, s = (E*A)/l0: [n_elems][3] = s*c2, s*cs, s*s2 (2-D),
   * [n_elems] = s (1-D); twice that with prop_double.  Written by the MFMA32 forward pass (the launch that evaluates the
   * LAST enabled net, or the fused launch of both) with the float operations of nn_assembly.py:74, 84-94, and read by the
   * node kernels instead of E, A and the geometry record (12 B per incidence instead of 20); NULL: the node kernels form
   * the same numbers from prop_e / prop_a / the constant properties and mesh.egeo */
  float* elem_k;
  /* second half of the parameter state: [3][n_theta] floats = theta | m_t | v_t, or NULL.  With it the iteration graph
   * folds the parameter update of iteration t (sum of the second-level partial rows, optimizer_theta.step(),
   * solver.py:293-294, operand images) into the prologue of the forward launch of iteration t+1: EVERY block of that
   * launch computes the update for itself from the half the previous update wrote and builds the operand images in its
   * own LDS; block 0 stores the new state into the OTHER half (nobody reads that one during the launch) and flips
   * state->theta_half.  The single-block update launch and one kernel boundary leave the critical path; a replay ends
   * with a stand-alone update that brings the state back to half 0. */
  float* theta_alt;
  /* second displacement vector [n_dofs], or NULL.  With it the iteration graph lets the displacement update of
   * iteration t (pf_node_gradu + Adam) WRITE the other vector than the one the residual and the element adjoint of t
   * read, so the update runs beside the whole backward launch instead of behind the adjoint's last read of u; the
   * vectors swap roles every iteration, an even number of iterations per replay ends in p->u, and a replay cut short by
   * the stop test copies the result home (state->u_half).
   * In the path form of the graph (pf_graph_form_info: PF_GRAPH_FORM_FOLDED_RESIDUAL; it needs u_alt) the vector is
   * SCRATCH instead: every iteration of a replay overwrites it with the residual r (0 at fixed dofs), which the
   * theta-stage-1 launch re-sums.  Do not keep anything in it across a replay. */
  float* u_alt;
  /* per CSR entry of mesh.adj: the node at the OTHER end of that element ([adj_ptr[n_nodes]] int32).  With it the node
   * kernels fetch a neighbour's values one dependent load earlier (adj -> value instead of adj -> conn -> value) and
   * two incidences at a time; NULL: they go through mesh.conn. */
  const int32_t* adj_other;
} pf_problem;

#define PF_MAX_BLOCKS 1024
/* node-parallel kernels run one node per thread on up to PF_MAX_NODE_BLOCKS blocks of 256 threads;
 * each block owns one slot of the three scalar partial-sum arrays (PF_NODE_SLOTS floats each, one
 * extra slot for the multi-GPU interface dofs) at the head of `partials` */
#define PF_MAX_NODE_BLOCKS 4096
#define PF_NODE_SLOTS (PF_MAX_NODE_BLOCKS + 8)

/* ---- introspection ------------------------------------------------------------------ */
int pf_abi_version(void);
const char* pf_last_error(void);
/* number of parameters of an MLP in torch parameters() order (generic.py:121-134) */
int pf_net_param_count(int in_dim, int width, int n_hidden);
/* padded width the kernels use for `width`, or PF_ERR_UNSUPPORTED */
int pf_padded_width(int width);
/* floats of padded-parameter workspace one net needs, or <0 */
int pf_net_pad_count(int in_dim, int width, int n_hidden);
/* padded-image index (inside the net's image) of the net's `local`-th torch parameter */
int pf_net_pad_index(int in_dim, int width, int n_hidden, int local);
/* sizeof of the ABI structs: 0 pf_mesh, 1 pf_net, 2 pf_state, 3 pf_problem, 4 pf_scalar_id, 5 pf_coarse, 6 pf_gl, 7 pf_dyn (binding self-check) */
int pf_sizeof(int what);
/* floats of operand-image workspace (pf_problem.net_op) one net needs with the MFMA32 engine, or <0 */
int pf_net_op_count(int in_dim, int width, int n_hidden);
/* floats needed in pf_problem.partials for the given block count */
long long pf_partials_count(const pf_problem* p);
/* which launches of one GD iteration are fused for this problem (MFMA32 engine; bit mask): 1 the forward pass of both nets
 * is ONE launch, 2 both backward passes (with the element adjoint) are ONE two-phase launch, 4 the iteration graph folds
 * the parameter update into the next forward launch, 8 the iteration graph ping-pongs two displacement vectors (the
 * displacement update on a side branch), 16 the iteration graph folds the displacement update (dL/du + Adam(u) + clamp)
 * into the next forward launch as well and is ONE chain of four launches per iteration (8 and 16 exclude each other).  In the
 * per-slot times of pf_gd_iterations_timed a fused launch is booked on the FIRST of its two slots. */
#define PF_FUSED_FORWARD 1
#define PF_FUSED_BACKWARD 2
#define PF_FUSED_THETA_UPDATE 4
#define PF_FUSED_U_PINGPONG 8
#define PF_FUSED_U_UPDATE 16
int pf_fusion_info(const pf_problem* p);
/* the form of this problem's iteration graph beyond pf_fusion_info (bit mask).  PF_GRAPH_FORM_FOLDED_RESIDUAL: the mesh is an
 * open path in element order (every node touches at most element e-1 at its j end and element e at its i end; node ids
 * arbitrary — a bar, a synthetic chain) on a problem of the PF_FUSED_U_UPDATE one-chain form with PF_FUSED_BACKWARD and
 * PF_FUSED_THETA_UPDATE and u_alt present: the graph then has no residual launch.  The fused backward launch forms r and g_f
 * itself, the loss sums and the previous iteration's bookkeeping ride in the theta-stage-1 launch: three launches per
 * iteration, same bits.  Further conditions: both nets at most 24 wide (the register buckets whose fused backward runs its
 * phases without a barrier), mesh.dim == in_dim - 1, no interface dofs; with mesh.dim == 2 mesh.dof_flags must be 2-byte
 * aligned (a node's two flags are read as one 16-bit load).  Wider nets keep the four-launch chain.  u_alt is scratch in this
 * form (see pf_problem.u_alt).  Eager launches and the building blocks are not affected.  The query inspects the mesh on the
 * device (one small launch and a 4-byte copy; synchronous), as pf_graph_create does. */
#define PF_GRAPH_FORM_FOLDED_RESIDUAL 1
int pf_graph_form_info(const pf_problem* p);
/* Does this problem's iteration graph run its path form (PF_GRAPH_FORM_FOLDED_RESIDUAL) with the LIGHT forward?  1 / 0, or
 * PF_ERR_ARG.  1: both nets enabled, two hidden layers, split-f16 operands (the bf16-operand build keeps the full forward), and
 * not a young net 21 to 24 wide with three inputs (its backward kernel has no register left for the form).
 * The graph's forward launch then evaluates the E net only for the first and the last element of every 64-element task and
 * stores prop_a and those elements' stiffness records; the fused backward launch, which recomputes the E net's hidden layers
 * anyway, forms E itself and stores prop_e and every other record.  Same bits in prop_e, prop_a, elem_k and everything
 * computed from them; each location is written once per iteration, and both launches of an iteration always complete
 * together.  Eager launches and every other graph form run the full forward.  pf_graph_form_info is not affected.
 * Additive: PF_ABI_VERSION stays 9. */
int pf_graph_light_forward(const pf_problem* p);
/* Do the node tasks of this problem's iteration graph address by node id?  1 / 0, or PF_ERR_ARG.  1: the graph runs its path
 * form (PF_GRAPH_FORM_FOLDED_RESIDUAL) AND the node ids follow the path, conn[2e] == e and conn[2e+1] == e + 1 for every
 * element (a bar meshed from one end to the other, a synthetic chain).  The displacement update inside the graph's forward
 * launch then reads the records of elements n-1 and n and g_f at nodes n-1, n, n+1 for node n instead of walking adj_ptr,
 * adj and adj_other: one round trip through memory instead of three, the adjacency is not read.  Same partition, same
 * order of the sums, same bits, the u-norm monitor included.  A path with other node ids (reversed, shuffled) keeps the
 * gather; so do eager launches, pf_graph_tail and every other graph form.  Decided by the same device pass as
 * pf_graph_form_info.  pf_graph_form_info and pf_graph_light_forward are not affected.  Additive: PF_ABI_VERSION stays 9. */
int pf_graph_ordered_path(const pf_problem* p);

/* ---- building blocks (each replaces the cited reference lines) ------------------------ */
/* torch-layout theta -> padded image (no reference analogue; internal layout change) */
int pf_pack_theta(const pf_problem* p, void* stream);
/* NNProperty.value for every element: properties.py:116-161 + generic.py:141 (batch of n_elems
 * instead of n_elems batch-1 calls).  which: 0 young, 1 area.  Output p->prop_e / prop_a. */
int pf_net_forward(const pf_problem* p, int which, void* stream);
/* the forward pass of EVERY enabled net (one launch where pf_fusion_info says so) incl. the stiffness records, and the
 * backward pass of every enabled net with the element adjoint (one two-phase launch where fused; else adjoint + one
 * launch per net): what one GD iteration enqueues for these two steps.  Idempotent: may be repeated for timing. */
int pf_net_forward_all(const pf_problem* p, void* stream);
int pf_net_backward_all(const pf_problem* p, void* stream);
/* f_int = K(theta) u by node-wise gather of fe = (s*pattern) @ u_elem:
 * nn_assembly.py:64-100 + 226-227 (f_int only; K is never formed).  f_int_out dev [n_dofs]. */
int pf_internal_force(const pf_problem* p, const float* u, float* f_int_out, void* stream);
/* residual + losses + dL/df_int: solver.py:267-283.  Fuses pf_internal_force.  Writes p->g_f and
 * block partials of sum r^2, sum d^2; f_int_out may be NULL. */
int pf_node_residual(const pf_problem* p, float* f_int_out, void* stream);
/* per-element dL/d(EA): the part of loss.backward() (solver.py:289) through ke = s*pattern,
 * fe = ke@u (nn_assembly.py:96-100).  Writes p->g_ea. */
int pf_elem_adjoint(const pf_problem* p, void* stream);
/* backward of NNProperty.value for every element + reduction over elements of the parameter
 * gradient (autograd of properties.py:150-156 / generic.py:141).  Writes block partials. */
int pf_net_backward(const pf_problem* p, int which, void* stream);
/* dL/du by node-wise gather (K^T g_f) + data term (solver.py:273-279 backward).
 * fuse_adam!=0: also optimizer_u.step() + u[fixed]=0 (solver.py:292, 297-298) in the same pass
 * and block partials of ||u_free||^2 (solver.py:304). */
int pf_node_gradu(const pf_problem* p, int fuse_adam, void* stream);
/* sum the parameter-gradient partials in fixed order -> p->grad_theta; fuse_adam!=0: also
 * optimizer_theta.step() (solver.py:293-294) and refresh of the padded image. */
int pf_theta_reduce(const pf_problem* p, int fuse_adam, void* stream);
/* monitors, history row, stop test, Adam scalars of the next step: solver.py:304-355. */
int pf_finalize(const pf_problem* p, void* stream);
/* reset state for a new solve_gd call (fresh Adam: solver.py:234-238): zero moments, iter=0 */
int pf_reset(const pf_problem* p, void* stream);

/* ---- the fused loop ------------------------------------------------------------------- */
/* Enqueue n_iter complete GD iterations (solver.py:254-355).  Once the device-side stop test
 * fires, remaining launches are no-ops, so the final state equals the reference's `break`. */
int pf_gd_iterations(const pf_problem* p, int n_iter, void* stream);
/* hipGraph form of pf_gd_iterations: capture `iters_per_graph` iterations once, replay many times
 * (removes the per-launch host cost and most of the inter-kernel gaps).  The graph bakes in the
 * pf_problem record by value: create it after the record is final (one per solve_gd call) and destroy
 * it before changing any field.  *graph_out is an opaque handle owned by the caller.  iters_per_graph >= 1.
 * In every form the bookkeeping of iteration t (pf_finalize's work) runs as one extra block of the residual launch of
 * t+1 (on a path mesh, pf_graph_form_info: of the theta-stage-1 launch of t+1), reading the other half of the residual's
 * partial sums (part_half); the last iteration of a replay gets a stand-alone pf_finalize.  The form (pf_fusion_info
 * reports it):
 *  - ONE CHAIN where the forward launch carries the displacement update of the previous iteration (PF_FUSED_U_UPDATE:
 *    MFMA32 engine, both nets enabled with equal depths, elem_k, adj_other and prop_double present, one GPU), at any
 *    size; and below 2e5 elements otherwise, with grad_u + Adam(u) as a stand-alone launch on the chain.
 *  - A DEPENDENCY DAG from 2e5 elements (mesh.n_elems) up when the displacement update is not fused: grad_u + Adam(u)
 *    runs on a side branch beside the backward launches.  With u_alt and an even iters_per_graph it ping-pongs the
 *    displacements between u and u_alt (PF_FUSED_U_PINGPONG; a replay always ends with them in u) and starts right
 *    behind the residual; otherwise it starts behind the last reader of u.
 * The state (u, theta), both optimisers' moments and every history column except the u_norm monitor are bit-identical to
 * pf_gd_iterations.  The u_norm monitor (history column 3, pf_state.u_norm) is the exception: in the PF_FUSED_U_UPDATE form it
 * sums the same block partials in another grouping and may differ in the last bits. */
int pf_graph_create(const pf_problem* p, int iters_per_graph, void* stream, void** graph_out);
/* Replays that hand their last iteration's tail to the next replay (one-chain form of the graph only, even
 * iters_per_graph; PF_ERR_UNSUPPORTED otherwise).  A plain replay ends with three stand-alone launches — the parameter
 * update, the displacement update and the bookkeeping of its last iteration (~45 us at 10^6 elements).  PF_GRAPH_NO_TAIL
 * leaves them PENDING behind the last gradient-row reduction; PF_GRAPH_CONT_HEAD makes iteration 0 carry the pending work of
 * the replay before it (as every other iteration of a replay carries its predecessor's).  Sequence: [NO_TAIL] then any
 * number of [CONT_HEAD | NO_TAIL], then pf_graph_tail (eager launches) before anything reads the state; a stop raised on
 * the device is honoured as in a plain replay (solver.py:341-355 semantics: the final state is that of the stopping
 * iteration). */
#define PF_GRAPH_CONT_HEAD 1
#define PF_GRAPH_NO_TAIL 2
int pf_graph_create_ex(const pf_problem* p, int iters_per_graph, int flags, void* stream, void** graph_out);
int pf_graph_tail(const pf_problem* p, int iters_per_graph, void* stream);
int pf_graph_launch(void* graph, void* stream);
int pf_graph_destroy(void* graph);
/* Profiling twin of pf_gd_iterations: same launches with a HIP event before every kernel slot, then
 * a stream synchronise; ms_per_kernel (HOST, PF_KERNEL_SLOTS floats) receives the average duration
 * of each slot: 0 net_forward(young) 1 net_forward(area) 2 node_residual 3 elem_adjoint
 * 4 net_backward(young) 5 net_backward(area) 6 node_gradu+Adam 7 theta_reduce+Adam 8 finalize. */
#define PF_KERNEL_SLOTS 9
int pf_gd_iterations_timed(const pf_problem* p, int n_iter, void* stream, float* ms_per_kernel);
/* loss and gradients only (no optimiser): what torch.autograd.Function.forward/backward need.
 * Requires p->grad_u != NULL.  Leaves loss terms in p->state, gradients in grad_u/grad_theta. */
int pf_loss_and_grads(const pf_problem* p, void* stream);

/* ---- multi-GPU (elements sharded across ranks) ----------------------------------------------------
 * No reference analogue: the reference is single-process.  A rank holds its own elements plus one ring of GHOST
 * elements (every element of another rank that touches a node shared with this rank), so the internal force of every
 * node of an own element is complete without communication.  One sharded iteration is
 *   pf_shard_forward          the nets on all local elements (own + ghost)
 *   pf_shard_backward         residual + losses, nets backward over the OWN elements, theta reduction into
 *                             p->grad_theta (which the host points inside buf), this rank's share of grad_u on the
 *                             interface dofs, local sums
 *                             -> buf = [iface grad_u (n_iface) | grad_theta (n_theta_active) | r2, d2, u2 of the previous iteration]
 *   pf_shard_update_interior  grad_u + Adam(u) + clamp of every dof that is NOT an interface dof
 *                                                                                      => ONE all-reduce(buf), issued by the host
 *   pf_shard_update_shared    Adam(theta) from the reduced gradient, Adam(u) of the interface dofs (every rank that
 *                             holds a copy applies the same step), u2_local[0] = this rank's sum u_free^2 over its
 *                             dofs, then the bookkeeping of the iteration (monitors, history row, stop test) from the
 *                             reduced sums; the u-norm, a monitor only, lags one iteration behind
 * and after the last iteration of a chunk: all-reduce(u2_local) => pf_shard_flush completes the last history row. */
int pf_shard_forward(const pf_problem* p, void* stream);
int pf_shard_backward(const pf_problem* p, float* buf, const float* u2_local, void* stream);
int pf_shard_update_interior(const pf_problem* p, void* stream);
int pf_shard_update_shared(const pf_problem* p, const float* buf, float* u2_local, void* stream);
int pf_shard_flush(const pf_problem* p, const float* u2_reduced, void* stream);

/* The same iteration driven from C with an own RCCL communicator (pf_comm.hip): the product path on real multi-GPU
 * runs.  librccl is dlopen'ed from `librccl_path` (the library PyTorch loaded; NULL/"" = "librccl.so"); there is no
 * link-time dependency.
 *   rank 0: pf_comm_unique_id -> 128 bytes, broadcast by the host (torch.distributed) -> every rank:
 *   pf_comm_create (collective, like ncclCommInitRank).
 * pf_shard_iterations enqueues n_iter iterations on `stream` (the four calls above around ONE ncclAllReduce each) plus
 * the closing flush, and returns without waiting for the device.  buf = dev [n_iface + n_theta_active + 3],
 * u2_local = dev [1], and p->grad_theta must point at buf + n_iface. */
#define PF_COMM_ID_BYTES 128
int pf_comm_unique_id(const char* librccl_path, void* id_out);
int pf_comm_create(const char* librccl_path, const void* id, int rank, int world, void** comm_out);
int pf_comm_destroy(void* comm);
/* failure path: ncclCommAbort instead of ncclCommDestroy — does not wait for outstanding collectives, so a rank that
 * raised can leave while its peers sit in (or it has itself enqueued) a collective that will never be matched.  Do not
 * synchronise the device first. */
int pf_comm_abort(void* comm);
/* rank and rank count as the communicator reports them (ncclCommUserRank, ncclCommCount) */
int pf_comm_info(void* comm, int* rank_out, int* nranks_out);
/* sum over ranks of buf[0..n), in place, on `stream` (the collective pf_shard_iterations issues, on its own) */
int pf_comm_all_reduce(void* comm, float* buf, int n, void* stream);
int pf_shard_iterations(const pf_problem* p, void* comm, int n_iter, float* buf, float* u2_local, void* stream);
/* iters_per_graph sharded iterations as ONE hipGraph with the collective captured inside (handle for pf_graph_destroy):
 * the single-engine iteration's dependency shape (grad_u + Adam(u) of the interior dofs beside the second backward and
 * the collective) without a host launch per kernel.  It bakes in *p, buf, u2_local and the communicator; every rank
 * must create and replay it alike.  pf_shard_iterations_graph = pf_shard_iterations replaying that graph for whole
 * multiples of iters_per_graph and launching the remainder eagerly; results are bit-identical to pf_shard_iterations. */
int pf_shard_graph_create(const pf_problem* p, void* comm, int iters_per_graph, float* buf, float* u2_local, void* stream,
                          void** graph_out);
int pf_shard_iterations_graph(const pf_problem* p, void* comm, void* graph, int iters_per_graph, int n_iter, float* buf,
                              float* u2_local, void* stream);

/* ---- classical Newton-Raphson support (pf_pcg.hip) ---------------------------
 * The reference's solve_nr (FEM/python/fem/solver.py:408-512) solves K_ff du_f = rhs_f with
 * np.linalg.solve on the dense float64 tangent of fem/assembly.py:16-75.  Here K is never formed:
 * pf_kv_f64 applies it matrix-free in float64 and pf_pcg_* run a conjugate-gradient solve preconditioned
 * with diag(K_ff) (Jacobi).  Vectors are double [n_dofs], fixed dofs carried as zeros; E and A come from
 * p->prop_e / p->prop_a when the net is enabled, else from net.scale (scalar materials). */
/* out = K v (all rows; zero_fixed != 0: rows of fixed dofs set to 0) */
int pf_kv_f64(const pf_problem* p, const double* v, double* out, int zero_fixed, void* stream);
/* doubles of workspace pf_pcg_* need */
long long pf_pcg_workspace_count(const pf_problem* p);
/* start a solve of K_ff x = b (entries of b on fixed dofs are ignored), x = 0; stop when |r| <= rtol*|b|
 * (rtol >= 0).  Enqueues only: rtol^2 travels as a kernel argument. */
int pf_pcg_begin(const pf_problem* p, const double* b, double* x, double* ws, double rtol, void* stream);
/* n_iter CG iterations (no-ops after the stop test fired).  state_out: host double[4] or NULL =
 * [iterations done, stopped (0/1), |r|^2, |b|^2], read back after a stream synchronisation. */
int pf_pcg_iterations(const pf_problem* p, double* x, double* ws, int n_iter, double* state_out, void* stream);
/* the same n_iter iterations captured as one hipGraph (handle for pf_graph_launch / pf_graph_destroy), and the
 * state read-back on its own */
int pf_pcg_graph_create(const pf_problem* p, double* x, double* ws, int n_iter, void* stream, void** graph_out);
int pf_pcg_state(const pf_problem* p, double* ws, double* state_out, void* stream);

/* ---- two-level preconditioner for the same solve (pf_pcg.hip) ------------------------------------------------------
 *   M^-1 r = D^-1 r + Z (Z^T K Z)^-1 Z^T r,   D = diag(K_ff)
 * Z holds per aggregate of nodes its rigid-body modes (2-D: two translations and the rotation about the centroid; 1-D: the
 * translation), zero on fixed dofs, orthonormalised per aggregate by the host (pinn_fem_amd/coarse.py).  At most
 * PF_COARSE_MODES columns touch a dof, so Z is held as per-dof coefficients and never formed.  Opt-in: the pf_pcg_* family
 * above is unchanged.  The workspace is that of pf_pcg_* (same layout) followed by w = Z^T r and y = A^-1 w
 * (PF_COARSE_MAX doubles each).  All arrays dev, caller-owned. */
#define PF_COARSE_MAX_AGG 256
#define PF_COARSE_MODES 3
#define PF_COARSE_MAX (PF_COARSE_MAX_AGG * PF_COARSE_MODES)
typedef struct pf_coarse {
  int32_t n_agg;             /* aggregates, 1..PF_COARSE_MAX_AGG */
  int32_t n_coarse;          /* columns of Z = agg_off[n_agg], 0..PF_COARSE_MODES*n_agg */
  const int32_t* node_agg;   /* [n_nodes] aggregate of every node */
  const int32_t* agg_off;    /* [n_agg+1] first column of every aggregate (0..PF_COARSE_MODES columns each) */
  const double* zcoef;       /* [n_dofs][PF_COARSE_MODES]: Z[dof][agg_off[a] + k] = zcoef[dof][k], a = node_agg[node of dof];
                                0 on fixed dofs and for k beyond the aggregate's column count */
  const int32_t* agg_ptr;    /* [n_agg+1] aggregate -> its nodes in agg_nodes */
  const int32_t* agg_nodes;  /* [n_nodes] node ids, ascending inside an aggregate: the order of every sum over it */
  const double* a_inv;       /* [n_coarse][n_coarse] (Z^T K Z)^-1, row-major; the host inverts what pf_coarse_setup
                                formed (not read by pf_coarse_setup itself) */
} pf_coarse;
/* a_c_out (dev [n_coarse][n_coarse], row-major) = Z^T K Z with the element stiffness of pf_kv_f64; one workgroup per
 * aggregate owns that aggregate's rows, sums over its nodes run in ascending node id, no atomics */
int pf_coarse_setup(const pf_problem* p, const pf_coarse* c, double* a_c_out, void* stream);
/* doubles of workspace pf_pcg2_* need */
long long pf_pcg2_workspace_count(const pf_problem* p);
/* as pf_pcg_begin / pf_pcg_iterations / pf_pcg_graph_create / pf_pcg_state, with z = M^-1 r in place of z = D^-1 r.
 * |r|^2, |b|^2 and the stop test are those of pf_pcg_*.  One iteration is a chain of six launches: K p, alpha, the
 * update of x and r with the restriction w = Z^T r (one workgroup per aggregate), y = A^-1 w with z = D^-1 r + Z y,
 * beta and the stop test, p = z + beta p. */
int pf_pcg2_begin(const pf_problem* p, const pf_coarse* c, const double* b, double* x, double* ws, double rtol, void* stream);
int pf_pcg2_iterations(const pf_problem* p, const pf_coarse* c, double* x, double* ws, int n_iter, double* state_out,
                       void* stream);
int pf_pcg2_graph_create(const pf_problem* p, const pf_coarse* c, double* x, double* ws, int n_iter, void* stream,
                         void** graph_out);
int pf_pcg2_state(const pf_problem* p, double* ws, double* state_out, void* stream);

/* ---- large displacements: the Green-Lagrange truss element and its tangent operator (pf_nl.hip, pf_pcg.hip) -----------
 * Total-Lagrangian element in float64, per element with nodes i, j:  d0 = X_j - X_i,  du = u_j - u_i,  d = d0 + du,
 *   e  = (2 d0.du + du.du) / (2 l0^2)        (not (l^2 - l0^2) / (2 l0^2): that form cancels at small strain)
 *   N  = E*A * e                             E*A as pf_kv_f64 forms it (per-element properties if a net is enabled)
 *   fe = (N / l0) d                          f_int[j] += fe, f_int[i] -= fe
 *   B  = (E*A / l0^3) d d^T + (N / l0) I     K_t v: row j += B (v_j - v_i), row i -= B (v_j - v_i)
 * 1-D: d, fe and B are scalars.  At u = 0, B is the linear element block s*(c2, cs; cs, s2).  This is the consistent
 * element of the virtual-work derivation, not the reference's truss2d_element_state (fem/element.py:105-133), whose force
 * has the other sign and no 1/l0 and whose stiffness lacks the geometric term.  All arrays dev, caller-owned. */
typedef struct pf_gl {
  const double* d0;   /* [n_elems][dim] X_j - X_i in float64, from the model's float64 coordinates (not from the f32 egeo) */
  double* kt;         /* [n_elems][3] = B11, B12, B22   (1-D: [n_elems]) */
  double* fe;         /* [n_elems][dim] */
  double* strain;     /* [n_elems] e */
} pf_gl;
/* kt, fe and strain of every element at the displacements u (dev double [n_dofs]); one element per thread */
int pf_gl_state(const pf_problem* p, const pf_gl* g, const double* u, void* stream);
/* pf_gl_state with E*A of every element from ea (dev double [n_elems]) in place of the problem's own: the same kernel,
 * so with ea filled with the problem's E*A it gives pf_gl_state's bits.  kt is what every tangent family reads
 * (pf_kt_v_f64, pf_pcgt_*, pf_pcg2t_*, pf_pcgtm_*, pf_pcg2tm_*, pf_coarse_setup_t), so they all follow.  A null ea is
 * PF_ERR_ARG, never a silent solve with the problem's E*A.  The three entry points below are additive: the version stays 9. */
int pf_gl_state_ea(const pf_problem* p, const pf_gl* g, const double* ea, const double* u, void* stream);
/* pf_gl_state with an initial (eigen-) strain e0 of every element (dev double [n_elems], a Green-Lagrange strain in the
 * measure of g->strain: prestress e0 = -T / (E*A), thermal e0 = alpha * dT, lack of fit e0 = (L_natural - l0) / l0):
 *   N = E*A * (e - e0),  fe = (N / l0) d,  B = (E*A / l0^3) d d^T + (N / l0) I,
 * the derivative chain of sum E*A * l0 * (e - e0)^2 / 2.  g->strain stays the total strain e.  ea: as pf_gl_state_ea, or
 * null for the problem's own E*A.  The same kernel: e - e0[e] is formed once, after e, so an all-zero e0 gives
 * pf_gl_state's (pf_gl_state_ea's) bits.  A null e0 is PF_ERR_ARG, never a silent unstrained solve.  Additive: the
 * version stays 9. */
int pf_gl_state_e0(const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const double* u, void* stream);
/* pf_gl_state* with tension-only (cable) elements, the static counterpart of pf_gl_dyn_*_cable and the same rule: an
 * element with cable[e] != 0 and e - e0 < 0 (e - 0.0 where e0 is null; the subtraction of pf_gl_state_e0) is slack.  A
 * slack element writes strain[e] = e, fe = +0.0 and a tangent block of +0.0 (0.0 is selected for N / l0 and for
 * E*A / l0^3, a select on the value); every other element writes pf_gl_state*'s bits.  It is the bar kernel's <DIM, true>
 * instantiation; the bar entry points launch <DIM, false>, untouched.  Whatever reads kt and fe follows (pf_gl_fint,
 * pf_kt_v_f64, pf_kt_diag_f64, pf_pcgt_*, pf_pcg2t_*, pf_coarse_setup_t).
 *   ea, e0  dev double [n_elems], each nullable as in pf_gl_state_e0 / pf_gl_state
 *   cable   dev unsigned char [n_elems], 0 = a bar
 *   slack   dev unsigned char [n_elems], in/out: on entry the set of the previous call (the caller clears it to start a
 *           solve), on exit the current one (1 = slack)
 *   counts  dev double [PF_GL_CABLE_COUNT]: counts[0] = the number of slack elements, counts[1] = the number of elements
 *           whose flag differs from its entry value, exact integers; behind them the per-block partials they are the
 *           fixed-order sums of (no atomics: the same bytes on every repeat)
 * A null cable, slack or counts is PF_ERR_ARG, never a silent run of bars; nothing is enqueued on an error.  n_elems == 0
 * writes zero counts.  Two launches on the stream.  Additive: the version stays 9, pf_gl and pf_problem are unchanged. */
#define PF_GL_CABLE_COUNT (2 + 2 * PF_MAX_NODE_BLOCKS)
int pf_gl_state_cable(const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const unsigned char* cable,
                      unsigned char* slack, double* counts, const double* u, void* stream);
/* pf_gl_state* with elastoplastic elements: one-dimensional rate-independent plasticity with linear isotropic hardening,
 * written in the Green-Lagrange strain and its conjugate force.  Per element, with ey > 0 the yield strain
 * sigma_y / E (+inf: the element never yields), kappa >= 0 the hardening ratio H / E and (ep_n, al_n) the committed
 * plastic strain and accumulated plastic strain:
 *   e    as pf_gl_state forms it;  se = e - e0 (e0 nullable, as pf_gl_state_e0)
 *   tr   = se - ep_n
 *   r    = ey + kappa * al_n
 *   f    = |tr| - r
 *   plastic  <=>  f > 2^-40 * r
 *   dg   = plastic ? f / (1 + kappa) : 0 ;   sg = tr < 0 ? -1 : +1
 *   ep   = plastic ? ep_n + dg * sg : ep_n        al = plastic ? al_n + dg : al_n
 *   s    = plastic ? tr - dg * sg   : tr          (the strain that carries stress)
 *   N    = E*A * s ;  fe = (N / l0) d
 *   B    = (E*A_t / l0^3) d d^T + (N / l0) I ,  E*A_t = plastic ? E*A * kappa / (1 + kappa) : E*A
 * The return map is exact for linear hardening, so B is the consistent tangent.  The selects act on values: an element
 * that is not plastic stores pf_gl_state*'s bits (with ep_n = 0 those of the bar entry point with the same ea and e0; with
 * e0 null and a committed ep_n those of pf_gl_state_e0 at e0 := ep_n); g->strain stays the total strain e.  The relative threshold keeps an element that ended
 * an increment on the yield surface (f = +-round-off of r there) elastic on an unloading step; the stress it may carry in
 * excess is 2^-40 of its yield stress.  Every operation of the map is rounded on its own.
 * The evaluation always starts from the committed (ep_n, al_n), never from a previous call's (ep, al): those go to
 * buffers of their own, and a commit is the caller's swap of the two pointer pairs, not a launch.
 *   ey, kappa, ep_n, al_n   dev double [n_elems], in
 *   ep, al                  dev double [n_elems], out; ep == ep_n or al == al_n (an update in place) is PF_ERR_ARG
 *   yielding                dev unsigned char [n_elems], in/out: the previous call's flags in, this call's out (1 = plastic)
 *   counts                  dev double [PF_GL_CABLE_COUNT]: counts[0] = the number of plastic elements, counts[1] = the
 *                           number whose flag differs from its entry value, exact integers, the fixed-order sums of the
 *                           per-block partials behind them (no atomics), as pf_gl_state_cable's
 * ea, e0: as pf_gl_state_cable's.  A null pl or a null pointer in it is PF_ERR_ARG, never a silent elastic run; nothing is
 * enqueued on an error.  n_elems == 0 writes zero counts.  Two launches on the stream.  It is the <DIM, false,
 * gl_plastic_set> instantiation of the bar kernel; the bar and cable entry points launch theirs, untouched.  Whatever reads
 * kt and fe follows (pf_gl_fint, pf_kt_v_f64, pf_kt_diag_f64, pf_pcgt_*, pf_pcg2t_*, pf_coarse_setup_t); the
 * sensitivities and the dynamics stay elastic.  Additive: the version stays 9, pf_gl and pf_problem are unchanged;
 * pf_sizeof(8) is sizeof(pf_gl_plastic). */
typedef struct pf_gl_plastic {
  const double* ey;
  const double* kappa;
  const double* ep_n;
  const double* al_n;
  double* ep;
  double* al;
  unsigned char* yielding;
  double* counts;
} pf_gl_plastic;
int pf_gl_state_plastic(const pf_problem* p, const pf_gl* g, const double* ea, const double* e0, const pf_gl_plastic* pl,
                        const double* u, void* stream);
/* Sensitivity of a misfit J(u) to every element's E*A through the adjoint a (K_t(u) a = dJ/du on the free dofs, zero on
 * the fixed ones): s_e = -(e / l0) d.(a_j - a_i) with d = d0 + u_j - u_i and e the strain as pf_gl_state forms it.  It
 * does not contain E*A and reads g->d0 only.  out (dev double [n_elems]) = s (accumulate 0) or out + s (accumulate 1:
 * load levels sum in call order).  One element per thread, no atomics. */
int pf_gl_sens(const pf_problem* p, const pf_gl* g, const double* u, const double* a, int accumulate, double* out,
               void* stream);
/* pf_gl_sens for elements with the initial strain e0 of pf_gl_state_e0: s_e = -((e - e0) / l0) d.(a_j - a_i), the same
 * kernel and accumulate rule; an all-zero e0 gives pf_gl_sens's bits.  A null e0 is PF_ERR_ARG.  Additive: the version
 * stays 9. */
int pf_gl_sens_e0(const pf_problem* p, const pf_gl* g, const double* e0, const double* u, const double* a, int accumulate,
                  double* out, void* stream);
/* out[g] (dev double [n_groups]) = sum of values[e] * weights[e] (weights null: of values[e]) over e = group_elems[k],
 * group_ptr[g] <= k < group_ptr[g + 1] (dev int CSR; ids outside 0..n_elems-1 add nothing).  One workgroup per group, a
 * fixed summation order, no atomics: the same bits on every run.  An empty group gives 0.0. */
int pf_group_sum_f64(int n_elems, const double* values, const double* weights, const int* group_ptr, const int* group_elems,
                     int n_groups, double* out, void* stream);
/* f_int_out (dev double [n_dofs], every row) = the node gather of +-g->fe, ascending element id, no atomics */
int pf_gl_fint(const pf_problem* p, const pf_gl* g, double* f_int_out, void* stream);
/* Right-hand sides of the sensitivity solves K_t s = -d f_int / d q_g for m groups of elements (q_g: a log-factor on E*A
 * of group g; f_int is linear in E*A, so the derivative is the internal force of the group's elements alone).  Row k of
 * out (dev double [m][n_dofs]) belongs to group g0 + k: out[k][dof] = -(sum of +-g->fe over the elements e of the dof's
 * node with elem_group[e] == g0 + k), pf_gl_fint's signs and ascending element id order, 0.0 on PF_DOF_FIXED dofs.  It
 * reads the fe of the last pf_gl_state / pf_gl_state_ea.  elem_group: dev int [n_elems]; an id outside g0..g0+m-1
 * (negative ids included) adds nothing, a node without elements gives zeros.  One node per thread, the group in
 * blockIdx.y, no atomics: with every element in one group the row is -f_int to the bit on the free dofs.  A null
 * pointer, m < 1 (or above 65535, the grid's limit), g0 < 0 or a bad mesh is PF_ERR_ARG before anything is enqueued.
 * Additive: the version stays 9. */
int pf_gl_group_rhs(const pf_problem* p, const pf_gl* g, const int* elem_group, int g0, int m, double* out, void* stream);
/* The derivative of the Green-Lagrange strains with respect to u, B = d e / d u, for strain-gauge data in the
 * identification:  d e_e / d u_j = +d_e / l0^2,  d e_e / d u_i = -d_e / l0^2  with d = d0 + u_j - u_i formed from g->d0 and u
 * as pf_gl_sens forms it (e is quadratic in u, so this is exact).  Neither entry point contains E*A or needs a previous
 * pf_gl_state.  Both are additive: the version stays 9.
 * pf_gl_strain_rhs: B^T coef, the adjoint right-hand side.  out[dof] (dev double [n_dofs]) = the sum over the node's
 * incidences, in ascending order, of +-(coef[e] / l0^2) d_e: + at the element's second node, - at its first.  coef: dev
 * double [n_elems], dense (0.0 where nothing is measured: a dof whose elements all have coef 0.0 gets exactly 0.0).
 * accumulate 0: out = the sum, 0.0 on PF_DOF_FIXED dofs; accumulate 1: out = out + the sum (rounded first) and fixed dofs
 * are left untouched.  One node per thread, no atomics.
 * pf_gl_strain_jvp: B v at n_meas measured elements for m vectors.  out[k * n_meas + i] (dev double [m][n_meas]) =
 * (d_e / l0^2).(v_k[j] - v_k[i]) for e = elems[i] (dev int [n_meas]) and v_k row k of v (dev double [m][n_dofs]).  An id
 * outside 0..n_elems-1 writes 0.0 and reads nothing.  One (gauge, row) pair per thread, the row in blockIdx.y:
 * 1 <= m <= 65535.  n_meas 0 is PF_OK with nothing enqueued.
 * A null pointer, a bad mesh, accumulate outside {0, 1}, n_meas < 0 or a bad m is PF_ERR_ARG before anything is enqueued. */
int pf_gl_strain_rhs(const pf_problem* p, const pf_gl* g, const double* u, const double* coef, int accumulate, double* out,
                     void* stream);
int pf_gl_strain_jvp(const pf_problem* p, const pf_gl* g, const double* u, const int* elems, int n_meas, const double* v,
                     int m, double* out, void* stream);
/* Right-hand sides of the sensitivity solves K_t s = -d f_int / d t_h for m groups of elements (t_h: a strain ADDED to the
 * initial strain e0 of every element of group h; the identification of a prestress, fem/prestress.py).  f_int is affine in
 * e0 with d fe / d e0 = -(E*A / l0) d, so row k of out (dev double [m][n_dofs]) is, per dof, the sum over the elements e of
 * the dof's node with elem_group[e] == g0 + k of +-(ea[e] / l0) d_e: + at the element's second node, - at its first,
 * ascending incidence order, 0.0 on PF_DOF_FIXED dofs.  d = d0 + u_j - u_i is formed from g->d0 and u as pf_gl_strain_rhs
 * forms it and l0 = |d0|: it needs no previous pf_gl_state and does not contain e0.  ea: dev double [n_elems], never null
 * (the host fills the problem's own E*A in); elem_group: dev int [n_elems]; an id outside g0..g0+m-1 (-1, "e0 is given",
 * included) adds nothing.  One node per thread, the group in blockIdx.y, no atomics: the same bits on every run, and row k
 * of an m-row call is the bits of the (g0 + k, 1) call.  A null pointer, m < 1 (or above 65535, the grid's limit), g0 < 0
 * or a bad mesh is PF_ERR_ARG before anything is enqueued.  Additive: the version stays 9. */
int pf_gl_prestress_rhs(const pf_problem* p, const pf_gl* g, const double* ea, const double* u, const int* elem_group, int g0,
                        int m, double* out, void* stream);
/* ---- explicit dynamics of the Green-Lagrange element (pf_nl.hip) ------------------------------------------
 * Central differences with a lumped mass and mass-proportional damping alpha.  With u_n, v_{n-1/2}, t_n = n dt and
 * lam(t) = lam0 + (lam1 - lam0) min(1, t / t_ramp) (t_ramp = 0: lam1), step n is ONE launch, one node per thread:
 *   f_int(u_n)  the element above, N = E*A (e - e0), formed per incidence from g->d0 and u_n and summed per node in
 *               ascending incidence order (it reads no record of pf_gl_state and writes none)
 *   v_{n+1/2} = c1 v_{n-1/2} + gk (lam(t_n) f_ext - f_int(u_n)) minv     c1 = (1 - alpha dt/2) / (1 + alpha dt/2)
 *   u_{n+1}   = u_n + dt v_{n+1/2}                                       gk = dt / (1 + alpha dt/2)
 * and PF_DOF_FIXED dofs get v = 0.0, u = 0.0 (any other lam(t), and supports that move: pf_dyn_hist below).  v is advanced in place; u_n is read from u0 for even n and from u1 for odd n
 * and u_{n+1} is written to the other.  n lives on the device in *clock: launch k of a sequence uses *clock + k, and a
 * last one-thread launch adds the sequence's length, so a captured sequence can be replayed.  No atomics: the same bits on
 * every run, eager or replayed.  All arrays dev double, caller-owned. */
typedef struct pf_dyn {
  const double* minv;    /* [n_dofs] 1 / lumped mass of the dof's node */
  const double* f_ext;   /* [n_dofs] the load at load factor 1 */
  const double* ea;      /* [n_elems] E*A of every element, or null: the problem's own (as pf_gl_state_ea) */
  const double* e0;      /* [n_elems] initial strain, or null (as pf_gl_state_e0) */
  double* u0;            /* [n_dofs] u_n for even n */
  double* u1;            /* [n_dofs] u_n for odd n */
  double* v;             /* [n_dofs] v_{n-1/2} */
  long long* clock;      /* [1] n */
  double dt, alpha, lam0, lam1, t_ramp;
} pf_dyn;
/* doubles of pf_gl_dyn_energy's out4: the four results, then its block partials */
#define PF_DYN_ENERGY_COUNT (4 + 4 * PF_MAX_NODE_BLOCKS)
/* pf_gl_dyn_start: the half kick from (u_0, v_0) at *clock == 0 (read back and checked; anything else is PF_ERR_ARG): the
 *   step's launch with c1 = 1 - alpha dt/2 and gk = dt/2, which leaves v_{1/2} and u_1, and the clock at 1.
 * pf_gl_dyn_steps: n_steps step launches and the clock's.
 * pf_gl_dyn_graph_create: the same sequence captured as one hipGraph, a single chain (handle for pf_graph_launch /
 *   pf_graph_destroy); the record is baked in by value, the clock is read when the launches run.
 * pf_gl_dyn_energy: at the state the clock points to (u_{n+1}, v_{n+1/2}), out4[0] = sum m v^2 / 2, out4[1] =
 *   sum E*A l0 (e - e0)^2 / 2, out4[2] = f_ext.u, out4[3] = max |v|; out4: dev double [PF_DYN_ENERGY_COUNT].  Two launches
 *   (block partials, then one block), a fixed order.
 * A null required pointer (ea and e0 may be null), dt <= 0 or non-finite, alpha < 0, t_ramp < 0, n_steps < 1 or a bad mesh
 * is PF_ERR_ARG, with a pf_last_error text that begins with the function's name, before anything is enqueued.  Additive:
 * the version stays 9. */
int pf_gl_dyn_start(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, void* stream);
int pf_gl_dyn_steps(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, int n_steps, void* stream);
int pf_gl_dyn_graph_create(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, int n_steps, void* stream,
                           void** graph_out);
int pf_gl_dyn_energy(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, double* out4, void* stream);
/* Tension-only (cable) elements in the explicit dynamics.  cable: dev unsigned char [n_elems], non-zero = the element
 * carries no compression: where e - e0 < 0 it is slack, N = 0, it adds +-0.0 to f_int in its place in the incidence order
 * (a dof whose elements are all slack gets f_int == 0.0 to the bit) and nothing to the strain energy.  Unflagged elements, and
 * flagged ones in tension, are the bar's arithmetic: all-zero flags give the bits of the entry points above.  Each entry
 * point is its namesake above with `cable` right behind `dyn`, in kernels of its own (the bar's are untouched), and refuses
 * what the namesake refuses in the same way; a null cable is PF_ERR_ARG too, never a silent bar run.  pf_dyn is unchanged.
 * pf_gl_dyn_energy_cable: out5[0..3] as out4, the strain energy without the slack elements; out5[4] = the number of slack
 * elements at that state, an exact integer; out5: dev double [PF_DYN_CABLE_ENERGY_COUNT].  Of the dynamics only these four
 * know cables; pf_gl_state_cable is the static counterpart, and the sensitivities stay bars.  Additive: the version stays 9. */
#define PF_DYN_CABLE_ENERGY_COUNT (5 + 5 * PF_MAX_NODE_BLOCKS)
int pf_gl_dyn_start_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, const unsigned char* cable, void* stream);
int pf_gl_dyn_steps_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, const unsigned char* cable, int n_steps,
                          void* stream);
int pf_gl_dyn_graph_create_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, const unsigned char* cable,
                                 int n_steps, void* stream, void** graph_out);
int pf_gl_dyn_energy_cable(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, const unsigned char* cable, double* out5,
                           void* stream);
/* Load and support-motion time histories in the explicit dynamics.  The caller samples every history at the step times
 * t_n = n dt once, before the run, and step n = *clock + k reads its samples by that number: no search and no interpolation
 * on the device, and a replayed graph reads the samples of the steps it then stands at.  With i(n) = min(n, n_samples - 1)
 * (a step beyond the table reads its last sample: the history is held),
 *   lam     = lam[i(n)] where lam is given, otherwise pf_dyn's ramp as above
 *   u_{n+1} = sup_amp[dof] * sup[i(n + 1)] on a PF_DOF_FIXED dof whose sup_amp is not 0.0 (one product), where sup is given;
 *             every other fixed dof gets the bytes of 0.0 as above (a select on the amplitude, never 0.0 * s, which is -0.0
 *             for a negative s).  v on a fixed dof stays 0.0 also where the dof moves: pf_gl_dyn_energy[_cable] are
 *             unchanged, count no kinetic energy of a support and never divide by its minv.
 * Free dofs are the step above but for where lam comes from.  pf_gl_dyn_start_hist is the half kick with lam[i(0)] and writes
 * sup[i(1)]; u_0 on the moved dofs is the caller's (sup_amp * s(0)).  Each entry point is its namesake above with `hist`
 * right behind `dyn` and `cable` behind that; here cable MAY be null, which means bars (the _cable entry points refuse a
 * null).  The kernels are instantiations of their own: the entry points above run the code they ran before.  A null hist,
 * lam and sup both null (never a silent plain run), sup without sup_amp, n_samples < 1 and everything the namesake refuses is
 * PF_ERR_ARG, with a pf_last_error text that begins with the function's name, before anything is enqueued.  All arrays dev
 * double, caller-owned, 16 bytes per step for both histories.  pf_dyn is unchanged.  Additive: the version stays 9. */
typedef struct pf_dyn_hist {
  const double* lam;      /* [n_samples] load factor of step n, lam[n] = lam(t_n); null: pf_dyn's ramp */
  const double* sup;      /* [n_samples] support-motion scale s(t_n); null: the supports stay at 0 */
  const double* sup_amp;  /* [n_dofs] amplitude per dof, read on PF_DOF_FIXED dofs only; required with sup */
  long long n_samples;    /* an index beyond the last sample reads the last one (the history is held) */
} pf_dyn_hist;
int pf_gl_dyn_start_hist(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, const pf_dyn_hist* hist,
                         const unsigned char* cable, void* stream);
int pf_gl_dyn_steps_hist(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, const pf_dyn_hist* hist,
                         const unsigned char* cable, int n_steps, void* stream);
int pf_gl_dyn_graph_create_hist(const pf_problem* p, const pf_gl* g, const pf_dyn* dyn, const pf_dyn_hist* hist,
                                const unsigned char* cable, int n_steps, void* stream, void** graph_out);
/* out = K_t v with the element blocks of kt (as pf_gl_state wrote them); otherwise pf_kv_f64 */
int pf_kt_v_f64(const pf_problem* p, const double* kt, const double* v, double* out, int zero_fixed, void* stream);
/* out (dev double [n_dofs]) = the diagonal of K_t from the element blocks of kt: per dof the sum of the diagonal entries
 * of the node's elements in ascending incidence order, exactly what pf_pcgt_begin inverts for the Jacobi preconditioner;
 * 0.0 on PF_DOF_FIXED dofs.  One node per thread, no atomics.  A null kt or out is PF_ERR_ARG.  Additive: the version
 * stays 9. */
int pf_kt_diag_f64(const pf_problem* p, const double* kt, double* out, void* stream);
/* as pf_pcg_begin / pf_pcg_iterations / pf_pcg_graph_create / pf_pcg_state on K_t: the same kernels, workspace
 * (pf_pcg_workspace_count), stop test and single-chain graph, the Jacobi preconditioner from kt's diagonal.  kt is read
 * when the launches RUN, so a graph stays valid while pf_gl_state overwrites kt in place between solves.  A null kt is
 * PF_ERR_ARG from every one of them, never a silent linear solve.  CG needs K_t positive definite on the free dofs: the
 * caller checks rhs.du > 0.  The two-level form is pf_pcg2t_*, below. */
int pf_pcgt_begin(const pf_problem* p, const double* kt, const double* b, double* x, double* ws, double rtol, void* stream);
int pf_pcgt_iterations(const pf_problem* p, const double* kt, double* x, double* ws, int n_iter, double* state_out,
                       void* stream);
int pf_pcgt_graph_create(const pf_problem* p, const double* kt, double* x, double* ws, int n_iter, void* stream,
                         void** graph_out);
int pf_pcgt_state(const pf_problem* p, const double* kt, double* ws, double* state_out, void* stream);
/* the two-level preconditioner on K_t.  The near-null space of K_t(u) is the rigid motions of the DEFORMED body, so the
 * host rebuilds the columns on X + u and Z^T K_t Z is formed and factored again at every Newton iteration; the
 * aggregation stays that of the reference configuration, and every buffer of the pf_coarse record is refreshed in place
 * (n_coarse and agg_off may change with the configuration).
 * pf_coarse_setup_t: pf_coarse_setup with the element blocks of kt, the same workgroup-per-aggregate sums.
 * pf_pcg2t_*: pf_pcg2_* on K_t: the same kernels, workspace (pf_pcg2_workspace_count), stop test and single-chain graph.
 * kt, zcoef and a_inv are read when the launches RUN.  A null kt, or a null or inconsistent coarse space (a_inv
 * included), is PF_ERR_ARG before anything is enqueued: never a silent linear solve, never a silent Jacobi solve. */
int pf_coarse_setup_t(const pf_problem* p, const pf_coarse* c, const double* kt, double* a_c_out, void* stream);
int pf_pcg2t_begin(const pf_problem* p, const pf_coarse* c, const double* kt, const double* b, double* x, double* ws,
                   double rtol, void* stream);
int pf_pcg2t_iterations(const pf_problem* p, const pf_coarse* c, const double* kt, double* x, double* ws, int n_iter,
                        double* state_out, void* stream);
int pf_pcg2t_graph_create(const pf_problem* p, const pf_coarse* c, const double* kt, double* x, double* ws, int n_iter,
                          void* stream, void** graph_out);
int pf_pcg2t_state(const pf_problem* p, const double* kt, double* ws, double* state_out, void* stream);
/* m right-hand sides through the same launches: pf_pcgt_* / pf_pcg2t_* with every launch given grid (blocks, m), right-hand
 * side k = blockIdx.y.  b and x are dev double [m][n_dofs]; ws is m complete workspaces, one after the other
 * (pf_pcg_workspace_count doubles each for pf_pcgtm_*, pf_pcg2_workspace_count for pf_pcg2tm_*), so every right-hand side
 * has its own vectors, partial sums and state; kt, the coarse space and a_inv are shared.  Each right-hand side runs the
 * arithmetic of its own single solve in the same order (bit for bit), stops by its own test and from then on returns at
 * kernel entry while the others go on; state_out is host double [m][4].  The graph is still one chain of kernel nodes.
 * 1 <= m <= PF_PCG_MAX_RHS; a bad m, a null kt or (pf_pcg2tm_*) a bad coarse space is PF_ERR_ARG before anything is
 * enqueued.  The caller is displacement control in the Newton solve: K' a = f' and K' b = -R' - ... per iteration cost
 * the launches of one solve.  There is no batch of the linear operator (nothing calls one). */
#define PF_PCG_MAX_RHS 2
int pf_pcgtm_begin(const pf_problem* p, const double* kt, int m, const double* b, double* x, double* ws, double rtol,
                   void* stream);
int pf_pcgtm_iterations(const pf_problem* p, const double* kt, int m, double* x, double* ws, int n_iter, double* state_out,
                        void* stream);
int pf_pcgtm_graph_create(const pf_problem* p, const double* kt, int m, double* x, double* ws, int n_iter, void* stream,
                          void** graph_out);
int pf_pcgtm_state(const pf_problem* p, const double* kt, int m, double* ws, double* state_out, void* stream);
int pf_pcg2tm_begin(const pf_problem* p, const pf_coarse* c, const double* kt, int m, const double* b, double* x, double* ws,
                    double rtol, void* stream);
int pf_pcg2tm_iterations(const pf_problem* p, const pf_coarse* c, const double* kt, int m, double* x, double* ws, int n_iter,
                         double* state_out, void* stream);
int pf_pcg2tm_graph_create(const pf_problem* p, const pf_coarse* c, const double* kt, int m, double* x, double* ws, int n_iter,
                           void* stream, void** graph_out);
int pf_pcg2tm_state(const pf_problem* p, const double* kt, int m, double* ws, double* state_out, void* stream);

/* ---- scalar (E, A) identification: the device loop of pinn_inverse_problem_gd -------------------------------------
 * FEM/python/api_pinn_gradient_descent.py:102-121 calls pinn_inverse_problem_gd(nodes, elements, f_ext, fixed_dofs,
 * young_init, area_init, u_measured, measured_dofs, n_iterations, learning_rate, alpha, beta) — a callee the reference
 * never defines (ImportError at :19).  The build defines it after the nearest existing code, fem/nn_solver_gd.py:105-125:
 *   loss = alpha * mean(r_free^2) + beta * mean((u_meas - u[md])^2),   r = c K_1 u - f_ext / (E0 A0),   c = exp(p_E + p_A)
 * with E = E0 exp(p_E), A = A0 exp(p_A), Adam on u (lr_u = p->lr_u) and on (p_E, p_A) (lr_p), u[fixed] = 0 after the step,
 * optional box bounds on p.  `p` describes the unit-stiffness problem (both nets disabled, scale 1, measurements in the
 * mesh, alpha_physics = alpha, alpha_data = beta); K_1 u and its transpose are the node kernels of the GD path.
 * One iteration = three launches, no host synchronisation: residual + sums, displacement update, scalar update + table. */
typedef struct pf_scalar_id {
  float* p;            /* dev [2] log-multipliers (p_E, p_A), updated in place */
  float* m_p;          /* dev [2] Adam first moments */
  float* v_p;          /* dev [2] Adam second moments */
  float* table;        /* dev [n_rows][5] per iteration: loss_total, loss_physics, loss_data, p_E, p_A (after the step) */
  int32_t n_rows;      /* rows of `table` (iterations beyond are not recorded) */
  int32_t has_bounds;  /* clamp p to [lo, hi] after the step */
  float lo[2], hi[2];
  float inv_ea0;       /* 1 / (E0 * A0): the residual is scaled so that its size does not depend on the units of E */
  float lr_p;          /* learning rate of (p_E, p_A) */
  float n_free_f;      /* number of free dofs (denominator of the mean over the residual) */
  float _pad;
} pf_scalar_id;
/* enqueue n_iter iterations (state->iter counts them; pf_reset starts a run) */
int pf_scalar_gd_iterations(const pf_problem* p, const pf_scalar_id* sp, int n_iter, void* stream);

/* ---- extensions (off the default path) ------------------------------------------------ */
/* generic Adam (torch.optim.Adam single-tensor arithmetic) on a flat vector */
int pf_adam(float* param, const float* grad, float* m, float* v, int n, int step,
            double lr, double beta1, double beta2, double eps, void* stream);
/* diag(K(theta)) [n_dofs] — the Jacobi preconditioner the north-star names; the reference has
 * no such preconditioner (solver.py:113-195 is a two-phase schedule), so nothing calls this
 * by default.  Uses p->prop_e/prop_a from the last pf_net_forward. */
int pf_diag_k(const pf_problem* p, float* diag_out, void* stream);
/* k_global in coordinate format for meshes of any size (SURVEY 7.1b `assemble_coo`): the (2*dim)^2 entries
 * `k_global[g, h] += ke[a, b]` of every element (nn_assembly.py:228-229) as triplets, element after element; rows_out /
 * cols_out dev int64 [n_elems*(2*dim)^2], vals_out dev float32; duplicates are summed by the consumer (coalesce). */
int pf_coo_k(const pf_problem* p, long long* rows_out, long long* cols_out, float* vals_out, void* stream);
/* dense k_global [n_dofs][n_dofs] row-major, for assemble_system_torch's return value
 * (nn_assembly.py:228-231); small n_dofs only (<= 4096). */
int pf_dense_k(const pf_problem* p, float* k_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PINNFEM_HIP_H */
