/*
 * super_lm.h -- C ABI of libsuper_lm.so: the MI355X (gfx950) implementation of
 * SuPer's per-frame embedded-deformation Levenberg-Marquardt step.
 *
 * Drop-in boundary.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root):
 *
 *   slm_create / slm_destroy   <- LM_Solver.__init__            super/LM.py:11-34
 *   slm_bind_frame             <- {Data,ARAP,Rot}Loss.prepare   super/loss.py:212-220,408-426,480-485
 *   slm_prepare_model          <- its model-side half, ahead of the frame (see there)
 *   slm_run                    <- LM_Solver.LM                  super/LM.py:81-122
 *   slm_assemble               <- LM_Solver.prepareCostTerm(grad=True)   super/LM.py:54-68
 *   slm_loss                   <- LM_Solver.prepareCostTerm(grad=False)  super/LM.py:70-78
 *   slm_solve / slm_solve_dense <- LM_Solver.Solver             super/LM.py:37-51
 *   slm_data_residuals         <- DataLoss.forward internals    super/loss.py:222-255
 *   slm_apply_update           <- Surfels.update                super/nodes.py:193-223
 *   slm_knn                    <- Surfels.update_sfed_knn / update_ed / find_knn
 *                                                               super/nodes.py:154-191, utils/utils.py:212-221
 *
 * Conventions
 *   - Every pointer marked "device" is a HIP device pointer owned by the caller;
 *     the library never frees or reallocates caller memory.
 *   - Indices are int32.  The MODEL STATE (surfel positions, skinning weights, node positions --
 *     float64 tensors in the reference, true float64 values from the first Surfels.update on) is
 *     read as float64 when slm_frame.state_f64 != 0 (what the Python mirror passes: the caller's
 *     tensors are used in place, nothing is rounded) or as float32 (state_f64 == 0: the compact
 *     layout of BASELINE.json's fp32 configs).  The per-frame target tables are float32: the
 *     reference widens float32 back-projections to float64 (utils/data_loader.py:453-462), so
 *     float32 holds them exactly.  All arithmetic, the normal equations and the solve are float64
 *     (the reference computes in float64).
 *   - beta is (J,7) float64 row-major [qw,qx,qy,qz,bx,by,bz] (super/LM.py:85-88).
 *   - Every call returns an int status (SLM_OK == 0), never throws, and takes the
 *     hipStream_t (as void*) it enqueues on.  Only slm_bind_frame (one 4-byte
 *     read-back to size the band), slm_get_records and slm_status synchronise.
 *   - A solver owns `max_frames` independent slots; slm_run advances the LM
 *     problems of slots [0, n_frames) together in the same launches (the
 *     many-frame / many-hypothesis batch dimension).
 */
#ifndef SUPER_LM_H
#define SUPER_LM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SLM_OK = 0,
  SLM_ERR_INVALID = 1,      /* bad argument */
  SLM_ERR_HIP = 2,          /* a HIP runtime call failed (slm_last_error has the text) */
  SLM_ERR_NO_DEVICE = 3,    /* no gfx950 device / kernels cannot run */
  SLM_ERR_UNBOUND = 4,      /* slot used before slm_bind_frame */
  SLM_ERR_UNSUPPORTED = 5   /* e.g. num_neighbors outside 1..8, frames of one batch with different num_neighbors */
};

/* per-iteration status in slm_iter_record.status */
enum {
  SLM_ITER_OK = 0,
  SLM_ITER_SOLVER_FAILED = 1, /* Cholesky pivot <= 0: "Solver failed: Ill-posed system!" (super/LM.py:99-103) */
  SLM_ITER_NOT_RUN = 2,       /* iteration skipped because an earlier one stopped the loop */
  SLM_ITER_SOLVER_TIMEOUT = 3 /* the task-graph solve gave up waiting (a scheduling time-out of the persistent launch, not
                                 a property of the matrix); the loop stops like after a failed factorisation */
};

/* ABI handshake.  The structs of this header are passed by pointer and have grown between rounds; a caller built
 * against another revision of the header must get an error, not out-of-bounds reads.  slm_abi_version() returns
 * SLM_ABI_VERSION of the header the library was built from; slm_abi_check() also compares the caller's sizeof of
 * the five structs that carry pointers or were extended (returns SLM_OK or SLM_ERR_INVALID with the mismatch in
 * slm_last_error()).  Bindings call it once after loading the library (super_amd/_lib.py does). */
#define SLM_ABI_VERSION 3
#define SLM_PLAN_INFO_DOUBLES 16
int slm_abi_version(void);
int slm_abi_check(int32_t abi_version, int32_t sizeof_slm_config, int32_t sizeof_slm_frame, int32_t sizeof_slm_gf_config,
                  int32_t sizeof_slm_gf_frame, int32_t sizeof_slm_iter_record);

typedef struct slm_solver slm_solver; /* opaque */

/* Flags read from `opt` by LM_Solver.__init__/LM (super/LM.py:18-31,81-82). */
typedef struct slm_config {
  int32_t num_iterations;   /* opt.num_optimize_iterations (options.py:42), default 10 */
  int32_t phase_test;       /* opt.phase == "test": accept/reject; 0 = "train": always accept */
  int32_t use_data;         /* opt.sf_point_plane */
  int32_t use_arap;         /* opt.mesh_arap */
  int32_t use_rot;          /* opt.mesh_rot */
  int32_t max_frames;       /* number of slots (>= 1).  Performance note (results do not depend on it): the symbolic plan of
                             * a slot is built for the solver form this slot count implies -- a solver whose max_frames x J
                             * fits ONE task-graph launch (<= 8 000 frames x nodes, or <= 2 slots) dissects down to 50-node
                             * leaves, any other to 18-node leaves -- and cached plans keep the leaf size they were built
                             * with, whatever n_frames a later slm_run passes.  Create the solver with the slot count it
                             * will be run with. */
  int32_t data_path;        /* 0 = tuple-sorted MFMA assembly, node-pair blocks merged per workgroup in
                               LDS (default); 1 = per-entry f64 atomics (simple cross-check path, also
                               used when J >= 65536); 2 = MFMA assembly with one Gram per run in HBM */
  int32_t solver_path;      /* 0..4, anything else is rejected by slm_create.  0 = nested-dissection multifrontal Cholesky (default, needs data_path 0); its numeric
                               phase runs as ONE persistent launch over a static task graph (per-tile flags instead
                               of launch boundaries: the latency form) for small launches (one or two frames, or frames x nodes
                               <= 8 000: three or four frames of 2 000 nodes, eight of 512), and as one
                               launch per level / tile column / phase for larger batches (the throughput form),
                               with the top of the tree (the root front and its children: a chain of dependent tile
                               columns) as a task graph over all frames when the frames' trees have the same depth
                               (the hybrid form); 2 / 3 / 4 force the task-graph / the per-level / the hybrid form
                               (4 falls back to 3 when the trees differ in depth); 1 = block-banded Cholesky */
  double w_data;            /* opt.sf_point_plane_weight (1.0) */
  double w_arap;            /* opt.mesh_arap_weight (10.0) */
  double w_rot;             /* opt.mesh_rot_weight (1.0) */
  double u0;                /* LM(..., u=10)            super/LM.py:81 */
  double v;                 /* LM(..., v=7.5)                          */
  double minimal_loss0;     /* LM(..., minimal_loss=1e10)              */
} slm_config;

/* What LM reads from sf / inputs / new_data, as device pointers. */
typedef struct slm_frame {
  int32_t N;                /* surfels */
  int32_t J;                /* ED nodes (sf.ED_nodes.num) */
  int32_t T;                /* rows of the target tables */
  int32_t H, W;             /* image size (inputs[("color",0)] shape) */
  int32_t K;                /* surfel->node neighbours (opt.num_neighbors, README.md:175 / options.py:49): 1..8.  4, the reference's
                             * default, takes the tuple-sorted MFMA assembly; any other value the K-generic pair path (one sort of
                             * the coupled-pair keys at the bind, per-pair records filled by run-length-accumulated atomics) -- both
                             * on the SAME nested-dissection multifrontal solver in every form, and both accepted by the
                             * surfel-sharded mode (data_path = 1 / solver_path = 1 / J >= 65536: per-entry atomics into the band +
                             * block-banded solve); the frames of one batch share their K */
  int32_t K_ED;             /* node->node neighbours (opt.num_ED_neighbors), 1..8 */
  float fx, fy, cx, cy;     /* inputs["K"][0] entries [0,0],[1,1],[0,2],[1,2] (float32 like the reference) */
  const void* sf_points;      /* device (N,3)      sf.points            float32, or float64 with state_f64 */
  const int32_t* sf_knn_idx;  /* device (N,K)      sf.knn_indices: a row holds K DISTINCT ids in [0, J), so J >= K (a top-k in
                              * the reference); the binds refuse any other table with SLM_ERR_INVALID */
  const void* sf_knn_w;       /* device (N,K)      sf.knn_w             float32 / float64 */
  const void* ed_points;      /* device (J,3)      sf.ED_nodes.points   float32 / float64 */
  const int32_t* ed_knn_idx;  /* device (J,K_ED)   sf.ED_nodes.knn_indices: ids in [0, J) (refused otherwise) */
  const float* tgt_points;    /* device (T,3)      new_data.points */
  const float* tgt_norms;     /* device (T,3)      new_data.norms */
  const int32_t* index_map;   /* device (H,W)      new_data.index_map, -1 = invalid */
  const uint8_t* tgt_valid;   /* device (H*W)      new_data.valid */
  int32_t state_f64;          /* 0: sf_points / sf_knn_w / ed_points are float32; 1: float64 (the reference's
                                 own dtype: no rounding of the model state between frames) */
  int32_t pad;
} slm_frame;

typedef struct slm_iter_record {
  double loss;        /* sum of squared residuals at the trial beta (super/LM.py:107) */
  double u;           /* damping used for this iteration's solve */
  int32_t accepted;   /* 1 = step accepted */
  int32_t status;     /* SLM_ITER_* */
  int32_t M_grad;     /* matched surfels in the Jacobian pass */
  int32_t M_loss;     /* matched surfels in the loss pass (fresh match set) */
} slm_iter_record;

/* -- lifetime ------------------------------------------------------------------ */
int slm_create(const slm_config* cfg, slm_solver** out);
int slm_destroy(slm_solver* s);
const char* slm_last_error(void);
/* number of visible HIP devices, or 0 (never initialises a context) */
int slm_device_count(void);

/* -- per-frame binding (loss_term.prepare) ------------------------------------- */
/* Binds device pointers to `slot`, builds the frame's assembly plan (tuple-sorted surfel copies, coupled node pairs)
 * and the symbolic plan of the solver (kept while the coupling graph is unchanged), (re)sizes the slot's workspace and
 * resets beta to identity.  Stream-synchronising (one small device->host read when the slot's plan still applies).
 * A KNN index outside [0, J) -- an IndexError in the reference, super/loss.py:189-197 -- in sf_knn_idx or ed_knn_idx, a
 * surfel row of sf_knn_idx that repeats an id, or J < K with N > 0 (the reference's top-k gives neither) is found and
 * refused on every data path: SLM_ERR_INVALID, nothing was read out of bounds.  A bind that fails leaves the slot UNBOUND (slm_run
 * and friends return SLM_ERR_UNBOUND for it) until a later bind succeeds. */
int slm_bind_frame(slm_solver* s, int32_t slot, const slm_frame* frame, void* stream);
/* The same for the n_frames frames of a batch, slots [first_slot, first_slot + n_frames), `frames` an array in
 * host memory.  The preparation of a frame is a chain of small launches and size read-backs (latency, not
 * throughput), so the frames are bound concurrently: one host thread, stream and set of scratch buffers per frame
 * inside the library (at most 8 at a time), forked from `stream` (they see the work enqueued on it so far) and
 * joined back into it before the call returns.  Results are those of n_frames slm_bind_frame calls. */
int slm_bind_frames(slm_solver* s, int32_t first_slot, int32_t n_frames, const slm_frame* frames, void* stream);

/* The MODEL-side half of slm_bind_frame, ahead of time and asynchronously.  What a bind derives from the surfel model
 * alone -- the tuple-sorted copies and the pair index of the data term (from sf.points, sf.knn_indices, sf.knn_w), the
 * hash of the coupling graph and, when it changed, the symbolic plan of the solver (a host analysis) -- is known as soon
 * as the PREVIOUS frame has finished with the model (after Surfels.update / fuseInputData / the swap: super/super.py:66-73,
 * super/nodes.py:170-191), long before the next frame's target exists.  `model` carries N, J, K, K_ED, state_f64 and the
 * five model pointers (sf_points, sf_knn_idx, sf_knn_w, ed_points, ed_knn_idx); the target fields are ignored.  The call
 * records an event on `stream` (the preparation sees everything enqueued on it so far), queues the work on the solver's
 * own worker thread and stream, and RETURNS AT ONCE; the slot is unbound until the next slm_bind_frame.  That bind joins
 * the preparation; if its model fields are the ones prepared it only binds the target side (no sort, no read-back of
 * sizes, no analysis inside the frame's critical path), otherwise it discards the preparation and binds in full.  The
 * caller must leave the model arrays unchanged (and alive) between the two calls.  An error of the preparation is
 * returned by the bind that consumes it.  Replaces the model-side part of loss_term.prepare, super/loss.py:212-220,
 * 408-426, moved to where its inputs become final. */
int slm_prepare_model(slm_solver* s, int32_t slot, const slm_frame* model, void* stream);
/* Drops the slot's queued / finished preparation: the next slm_bind_frame binds in full whatever its pointers are.  The
 * library can only compare SIZES and POINTERS of the model arrays; a caller that knows the arrays were rewritten in place
 * after slm_prepare_model (same buffers, new values -- the host mirror sees it in the tensors' version counters) calls
 * this before the bind, otherwise the bind would consume a plan sorted from the old values.  Joins the worker; the bind
 * that follows is ordered behind the preparation's launches either way. */
int slm_discard_prepared(slm_solver* s, int32_t slot);

/* -- the LM loop ------------------------------------------------------------------ */
/* Enqueues num_iterations damped accept/reject iterations for slots [0,n_frames),
 * entirely on the device (no host synchronisation).  Running again without binding continues the loop from the slot's
 * current state; the library may then reuse what it derived from the bound input buffers (the Jacobian records of a
 * rejected step), so a caller that changes those buffers IN PLACE must bind the slot again before the next run. */
int slm_run(slm_solver* s, int32_t n_frames, void* stream);
/* Copies the slot's current beta (J*7 doubles) into caller device memory. */
int slm_get_beta(slm_solver* s, int32_t slot, double* beta_out_device, void* stream);
/* Overwrites the slot's beta from caller device memory (hypotheses / warm start / tests). */
int slm_set_beta(slm_solver* s, int32_t slot, const double* beta_in_device, void* stream);
/* Synchronises `stream` and copies the per-iteration records to HOST memory. */
int slm_get_records(slm_solver* s, int32_t slot, slm_iter_record* host_out, int32_t max_records,
                    void* stream);

/* Host-side facts about the slot's per-frame plan (after slm_bind_frame).  info_out has room for `capacity` doubles;
 * the first min(capacity, SLM_PLAN_INFO_DOUBLES) entries are written (a caller built for fewer entries is never
 * overrun, one that asks for more gets zeros):
 * [0] solver in use (0 nested dissection, 1 band), [1] fronts, [2] tree levels,
 * [3] FLOPs of one factorisation (padded dense fronts, or P*w^2 for the band),
 * [4] factor storage bytes, [5] distinct KNN tuples, [6] Gram runs, [7] coupled node pairs,
 * [8] workgroup-merged (workgroup, pair) records (0: one Gram per run in HBM), [9] padded positions,
 * [10] FLOPs of one factorisation without the padding of the fronts to 64, [11] tasks of the task-graph solver,
 * [12] pivot-column tiles of the fronts, [13] of them PURE FILL: no assembled block reaches them, some child maps into
 *      them -- neither zeroed per iteration nor read by their first toucher (0 with SLM_PURE_FILL=0),
 * [14] the preparation that built the slot's tuple-sorted plan (0 none / pair-record form, 1 binned, 2 rocPRIM pipeline),
 * [15] the largest bin the last build of that plan saw (surfels per smallest node, pair entries per larger node; 0 under
 *      the rocPRIM pipeline). */
int slm_get_plan_info(slm_solver* s, int32_t slot, double* info_out, int32_t capacity);

/* -- one LARGE frame sharded over the GPUs of a node ----------------
 * After slm_set_shard(rank, world) (before slm_bind_frame; every rank binds the WHOLE frame so that
 * all ranks build the same plan; world == 1 is allowed and runs the same exchange protocol on one rank) a context evaluates only its share of the surfels: workgroups
 * [n_wg*rank/world, ...) of the Jacobian pass and surfels [N*rank/world, ...) of the loss pass.
 * The library holds no communicator; per LM iteration the caller runs on every rank
 *     slm_lm_grad_local   zero, data-term Gram records of the share, per-pair partial sums
 *       -> all-reduce(sum) of SLM_X_PAIR_BLOCKS   (coupled pairs x 56 doubles + matched count;
 *                                                   7 MB at C2 = the block-sparse J^T J and J^T r)
 *     slm_lm_solve        reduced blocks -> fronts, ARAP / Rot rows, factor + solve
 *       -> broadcast of SLM_X_DELTA from rank 0   (keeps every rank on bit-identical parameters)
 *     slm_lm_loss_local   trial point, data loss of the share, regularisation loss
 *       -> all-reduce(sum) of SLM_X_DATA_LOSS     (1024 doubles)
 *     slm_lm_accept       accept / reject, record
 * with slm_lm_exchange_get / _set moving the buffers device to device to and from the caller's
 * tensor (torch.distributed = RCCL over xGMI on the GPU box).
 * The shares are fixed at the bind: with N surfels, lo = N*rank/world and hi = N*(rank+1)/world in integers,
 *   pair-record form (slm_enable_data_weights, or num_neighbors != 4): the Jacobian pass takes positions [lo, hi) of the
 *     neighbour-set-ordered surfel list, the loss pass surfels [lo, hi) of the caller's order -- two different partitions of
 *     the same frame, each summed over the ranks by its own exchange;
 *   tuple-sorted form (num_neighbors == 4, unweighted): both passes take the rank's 256-position workgroups of the
 *     tuple-sorted list.
 * A rank whose share holds no surfel, no matched surfel or only weights 0 adds exactly nothing and ends on the same beta.
 * A frame without surfels (N == 0) has no multifrontal data plan and is refused at the bind (SLM_ERR_UNSUPPORTED).
 * slm_set_shard on a handle with bound slots unbinds them (SLM_ERR_UNBOUND, "slot used before slm_bind_frame", until
 * they are bound again).  slm_run refuses a handle with world > 1.  The parity entry points on a sharded handle: see
 * slm_assemble / slm_loss below. */
#define SLM_X_PAIR_BLOCKS 0
#define SLM_X_DELTA 1
#define SLM_X_DATA_LOSS 2
int slm_set_shard(slm_solver* s, int32_t rank, int32_t world);
int slm_lm_grad_local(slm_solver* s, int32_t n_frames, void* stream);
int slm_lm_solve(slm_solver* s, int32_t n_frames, void* stream);
int slm_lm_loss_local(slm_solver* s, int32_t n_frames, void* stream);
int slm_lm_accept(slm_solver* s, int32_t n_frames, void* stream);
int slm_lm_exchange_size(slm_solver* s, int32_t slot, int32_t what, int64_t* n_doubles);
/* The library's own exchange buffer (device pointer, n_doubles long): a caller whose collective can run on foreign
 * device memory reduces IN PLACE on it (no get / set copies).  Valid until the slot is bound again. */
int slm_lm_exchange_ptr(slm_solver* s, int32_t slot, int32_t what, double** device_ptr_out, int64_t* n_doubles);
int slm_lm_exchange_get(slm_solver* s, int32_t slot, int32_t what, double* out_device, void* stream);
int slm_lm_exchange_set(slm_solver* s, int32_t slot, int32_t what, const double* in_device, void* stream);

/* -- flow-correspondence term of the LM path (opt.sf_corr; the reference left it commented out, super/LM.py:27-29) ------
 * A fourth term beside ICP + ARAP + Rot: per surfel i a target point o_i, a target normal n_i and a flag valid_i, FROZEN at
 * the bind and constant for the whole LM run.  T_i(beta) the skinned surfel, lambda = weight (loss = (lambda ...)^2 like
 * the other LM terms; GraphFit multiplies the squared sum by its weight instead):
 *   mode 1 'point-point':  r_i = lambda (T_i - o_i), three rows  lambda [ w_k d(R(q_k)(p - g_k))/dq_k | w_k I3 ] per neighbour
 *   mode 2 'point-plane':  r_i = lambda n_i.(T_i - o_i), one row, n_i^T times the rows above
 * No dependence through the projection (the targets do not move with beta).  The loss sum_valid |r_i|^2 is part of the
 * iteration's loss (accept / reject, slm_iter_record.loss); M_grad / M_loss stay the ICP match counts.
 *
 * slm_enable_corr: after slm_create, before the first bind.  mode 0 switches the option off again.  An enabled solver
 * takes the pair-record form of the data term (k_data_grad_pairs, the form of num_neighbors != 4) for EVERY num_neighbors,
 * 4 included, for binds and slm_prepare_model, with or without bound correspondences: at num_neighbors 4 that form is
 * slower than the default tuple-sorted one.  Refusals:
 *   SLM_ERR_INVALID      "slm_enable_corr: null argument"
 *                        "slm_enable_corr: mode must be 0 (off), 1 (point-point) or 2 (point-plane)"
 *                        "slm_enable_corr: weight must be finite"
 *                        "slm_enable_corr: a slot is already bound; call it after slm_create and before the first bind"
 *   SLM_ERR_UNSUPPORTED  "slm_enable_corr: needs the pair-record data path (data_path 0 or 2)"
 *                        "slm_enable_corr: needs a nested-dissection solver_path (0, 2, 3 or 4)"
 *                        "slm_enable_corr: needs the data term (use_data 1)"
 *                        "slm_enable_corr: the solver is sharded (slm_set_shard); the term needs every surfel of the frame on one device"
 *   and, on an enabled solver,
 *   SLM_ERR_UNSUPPORTED  "slm_set_shard: the correspondence term is enabled (slm_enable_corr); it needs every surfel of the frame on one device"
 *                        "slm_bind_frame: the correspondence term (slm_enable_corr) needs J < 65536"
 *
 * slm_bind_corr_flow: after slm_bind_frame.  flow (2,H,W) float32 device, x then y displacement; the targets are built
 * on the device exactly as GraphFit's term reads them at zero deformation: (u, v) = the unrounded projection of
 * sf_points[i] (Z + 1e-8), the flow sampled there grid_sample-style (float32 grid, bilinear, zero padding,
 * align_corners=False), validity margin 1 on the shifted float coordinates, o / n from the four taps through index_map (all
 * four mapped).  slm_bind_corr_points copies the caller's targets instead (device pointers: pts (N,3), nrm (N,3) -- may be
 * null in mode 1 --, valid (N)).  slm_bind_frame clears a slot's correspondences; a slot with none runs without the term.
 *   SLM_ERR_INVALID      "<fn>: null argument"   "<fn>: bad slot"
 *                        "slm_bind_corr_points: nrm is required in mode 2 (point-plane)"
 *   SLM_ERR_UNSUPPORTED  "<fn>: slm_enable_corr first"
 *   SLM_ERR_UNBOUND      "<fn>: slm_bind_frame first"
 *
 * slm_corr_get_targets: the slot's targets back (device pointers, each may be null).  slm_corr_loss: out_device[0] =
 * sum_valid |r_i|^2 at the slot's current beta, [1] = the kept count; {0, 0} for a slot without correspondences.  Both
 * refuse like the binds, and slm_corr_get_targets also with
 *   SLM_ERR_UNBOUND      "slm_corr_get_targets: no correspondences bound to the slot" */
int slm_enable_corr(slm_solver* s, int32_t mode, double weight);
int slm_bind_corr_flow(slm_solver* s, int32_t slot, const float* flow, void* stream);
int slm_bind_corr_points(slm_solver* s, int32_t slot, const double* pts, const double* nrm, const uint8_t* valid, void* stream);
int slm_corr_get_targets(slm_solver* s, int32_t slot, double* pts, double* nrm, uint8_t* valid, void* stream);
int slm_corr_loss(slm_solver* s, int32_t slot, double* out_device, void* stream);

/* -- per-residual weights of the LM path's point-to-plane term (reference super/loss.py:347-399, on the first-order path:
 * slm_gf_config seg_mode / pp_max) ---------------------------------------------------------------------------------------
 * Opt-in.  For every surfel i of the match set (unchanged), with e = T_i(beta) - o, s_i = (n.e)^2 (no lambda):
 *   seg_mode 1 (hard) / 2 (soft): conf = sum over the residual's four taps of wv_t tgt_seg_conf[row_t, :], q = softmax(conf)
 *     (the reference softmaxes the sampled confidences again); hard w_i = [sf_seg[i] == argmax q] (the first maximum wins),
 *     soft w_i = exp(-0.1 JSD(sf_seg_conf[i], q)) in the eps = 1e-13 form of the reference.  pp_max is ignored, like there.
 *   seg_mode 0 with pp_max > 0: w_i = [s_i < pp_max]  (the reference's max = 2e-5 for RAFT-stereo depth).
 * The weights are constants of the linearisation: the Jacobian pass uses row_i sqrt(w_i) and r_i sqrt(w_i) with w_i at beta,
 * the loss pass sums w_i r_i^2 with w_i and the match set fresh at the trial point.  M_grad / M_loss stay the match-set
 * counts: a surfel of weight 0 is matched and contributes nothing.  The reference's Huber weight is not built: on squared
 * residuals in m^2 its formula is the constant huber_th, and no reference caller passes it.
 *
 * slm_enable_data_weights: after slm_create, before the first bind.  (0, 0.0) switches the option off again.  An enabled
 * solver takes the pair-record form of the data term for every num_neighbors, 4 included (as slm_enable_corr, with which it
 * may be combined; slm_set_shard is allowed too: the weight is local to a surfel).  It refuses with
 *   SLM_ERR_INVALID      "slm_enable_data_weights: null argument"
 *                        "slm_enable_data_weights: seg_mode must be 0 (none), 1 (hard) or 2 (soft)"
 *                        "slm_enable_data_weights: pp_max must be finite and >= 0"
 *                        "slm_enable_data_weights: a slot is already bound; call it after slm_create and before the first bind"
 *   SLM_ERR_UNSUPPORTED  "slm_enable_data_weights: needs the pair-record data path (data_path 0 or 2)"
 *                        "slm_enable_data_weights: needs a nested-dissection solver_path (0, 2, 3 or 4)"
 *                        "slm_enable_data_weights: needs the data term (use_data 1)"
 * and on an enabled solver
 *   SLM_ERR_UNSUPPORTED  "slm_bind_frame: the data weights (slm_enable_data_weights) need J < 65536"
 *
 * slm_bind_data_semantic: after slm_bind_frame.  Device pointers, read in place like the frame's own (they must stay valid
 * and unchanged while the slot is used): sf_seg (N) int32, sf_seg_conf (N,C) float32, tgt_seg_conf (T,C) float32, rows as
 * the target table's.  slm_bind_frame / slm_bind_frames clear a slot's semantic inputs.  It refuses with
 *   SLM_ERR_INVALID      "<fn>: null argument"   "<fn>: bad slot"
 *   SLM_ERR_UNSUPPORTED  "<fn>: slm_enable_data_weights first"
 *                        "slm_bind_data_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)"
 *   SLM_ERR_UNBOUND      "<fn>: slm_bind_frame first"
 * With seg_mode != 0, slm_run, slm_loss, slm_assemble, slm_solve, slm_lm_grad_local, slm_lm_loss_local and slm_data_weights
 * over a slot without the inputs return (there is no silent unweighted run)
 *   SLM_ERR_UNBOUND      "<fn>: slot <i> has no semantic inputs; call slm_bind_data_semantic after slm_bind_frame"
 *
 * slm_data_weights: w_device (N) float64 = w_i at the slot's current beta, 0 for unmatched surfels: the diagnostic twin of
 * slm_data_residuals, which stays unweighted.  Refuses like slm_bind_data_semantic. */
int slm_enable_data_weights(slm_solver* s, int32_t seg_mode, double pp_max);
int slm_bind_data_semantic(slm_solver* s, int32_t slot, int32_t num_classes, const int32_t* sf_seg, const float* sf_seg_conf,
                           const float* tgt_seg_conf, void* stream);
int slm_data_weights(slm_solver* s, int32_t slot, double* w_device, void* stream);

/* -- triangle-area face term of the LM path (opt.mesh_face; the reference has only the first-order form,
 * super/deform_mesh.py:51-60, which slm_gf_config.use_face carries) ---------------------------------------------------
 * Opt-in.  Per triangle t of the slot's mesh with node ids (i0, i1, i2): v_a = g_a + beta[i_a, 4:7] (node position plus
 * translation; rotations do not enter, and the LM path has no global row), e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2,
 * A = sqrt(|c|^2 + 1e-13) / 2 and
 *   r_t = lambda (A - A0_t),   one row with nine non-zeros on the columns 7 i_a + 4..6:
 *   dA/dv1 = (e2 x c) / 4A,  dA/dv2 = (c x e1) / 4A,  dA/dv0 = -(dA/dv1 + dA/dv2)
 * A0_t is the caller's area, taken as given.  The constant keeps a degenerate triangle finite (A >= 1.58e-7, gradient 0).
 * lambda = weight multiplies the RESIDUAL, as for every LM term: loss = sum_t r_t^2 = lambda^2 sum (A - A0)^2.  GraphFit
 * multiplies the squared sum by its weight instead, so slm_gf_config.w_face = lambda^2 gives the same objective.  The loss
 * at the trial point is part of the iteration's loss (accept / reject, slm_iter_record.loss); M_grad / M_loss stay the ICP
 * match counts.  All arithmetic is float64.  The six node pairs of a triangle are in general neither surfel-KNN pairs nor
 * node-KNN edges: the bind adds them to the frame's coupled pairs (slm_get_plan_info [7] counts them), so the cached
 * symbolic plan is rebuilt when a mesh brings new pairs.
 *
 * slm_enable_face: after slm_create, before the first bind.  A weight of 0 switches the option off again.  An enabled
 * solver takes the pair-record form of the data term for every num_neighbors, 4 included (as slm_enable_corr and
 * slm_enable_data_weights, with which it may be combined).  Refusals:
 *   SLM_ERR_INVALID      "slm_enable_face: null argument"
 *                        "slm_enable_face: weight must be finite"
 *                        "slm_enable_face: a slot is already bound; call it after slm_create and before the first bind"
 *   SLM_ERR_UNSUPPORTED  "slm_enable_face: needs the pair-record data path (data_path 0 or 2)"
 *                        "slm_enable_face: needs a nested-dissection solver_path (0, 2, 3 or 4)"
 *                        "slm_enable_face: needs the data term (use_data 1)"
 *                        "slm_enable_face: the solver is sharded (slm_set_shard); the term's mesh is not sharded"
 *   and, on an enabled solver,
 *   SLM_ERR_UNSUPPORTED  "slm_set_shard: the face term is enabled (slm_enable_face); its mesh is not sharded"
 *                        "slm_bind_frame: the face term (slm_enable_face) needs J < 65536"
 *
 * slm_set_face_mesh: after slm_enable_face, before the slot's slm_bind_frame / slm_bind_frames / slm_prepare_model.  tri is
 * device (3, F) int32 (row a = vertex a of every triangle), areas device (F) float64; both are COPIED on `stream` into
 * buffers the slot owns, because the mesh outlives a frame: it stays with the slot over later binds until replaced.
 * n_triangles = 0 clears it (tri / areas may then be null), and a slot without a mesh runs without the term.  The call
 * leaves the slot unbound and drops a model prepared ahead: bind again.  A frame without surfels (N = 0) runs without the
 * term.  Refusals:
 *   SLM_ERR_INVALID      "slm_set_face_mesh: null argument"   "slm_set_face_mesh: bad slot"
 *                        "slm_set_face_mesh: n_triangles must be >= 0"
 *   SLM_ERR_UNSUPPORTED  "slm_set_face_mesh: slm_enable_face first"
 * The ids are checked where J is known: a bind or a prepared model whose mesh has an id outside [0, J), or a triangle that
 * repeats an id, is refused, the slot stays unbound and nothing is read out of bounds:
 *   SLM_ERR_INVALID      "slm_bind_frame: a triangle of the slot's face mesh (slm_set_face_mesh) has a node id outside [0, J) or repeats an id"
 *
 * slm_face_loss: out_device[0] = sum_t r_t^2 at the slot's current beta, [1] = the triangle count; {0, 0} for a slot
 * without a mesh.  The diagnostic twin of slm_corr_loss.  Refusals:
 *   SLM_ERR_INVALID      "slm_face_loss: null argument"   "slm_face_loss: bad slot"
 *   SLM_ERR_UNSUPPORTED  "slm_face_loss: slm_enable_face first"
 *   SLM_ERR_UNBOUND      "slm_face_loss: slm_bind_frame first"
 * Not built: the term on the tuple-sorted MFMA assembly, on sharded frames and for J >= 65536. */
int slm_enable_face(slm_solver* s, double weight);
int slm_set_face_mesh(slm_solver* s, int32_t slot, int32_t n_triangles, const int32_t* tri, const double* areas, void* stream);
int slm_face_loss(slm_solver* s, int32_t slot, double* out_device, void* stream);

/* -- semantic boundary-morph term of the LM path (opt.sf_bn_morph; the reference has only the first-order form,
 * super/deform_mesh.py:126-194, which slm_gf_config.use_bn_morph carries) ---------------------------------------------
 * Opt-in.  All arithmetic is float64.  T = T_i(beta) is the skinned surfel i; it projects to
 *   x = T.x fx / Ze + cx,  y = T.y fy / Ze + cy,  Ze = T.z + 1e-8   (fx .. cy: the frame's float32 values widened).
 * Surfel i is a CANDIDATE when argmax_c grid_sample(img_seg_conf)(x, y) != sf_seg[i] (bilinear taps, zero padding,
 * align_corners=False, the first maximum wins), the normalised coordinates are strictly inside (-1, 1) and its class has at
 * least 2 boundary pixels (a single pixel counts as no boundary).  The boundary lists per class are those of
 * slm_gf_bind_semantic (find_edge_region, kernel 3, margin 1, row-major), built once per slm_bind_morph.  e1, e2 are the two
 * nearest boundary pixels of the surfel's own class in (distance, list position) order, d1 <= d2 their squared distances.  A
 * candidate is KEPT when !(sqrt(d1) > dte || sqrt(d2) > dte) with dte = min(x, y, W - x, H - y) and l_i = (d1 + d2) / 2 > 15.
 * n = the kept surfels of the slot.  lambda = weight multiplies the RESIDUAL, as for every LM term:
 *   loss = lambda^2 / n sum_kept l_i   (the reference's mean times the weight; slm_gf_config.w_bn_morph = lambda^2 gives the
 *   same objective).  n = 0: the term contributes nothing -- the one departure: the reference's mean over an empty selection
 *   is NaN, which would reject every LM step.
 * The selection, the targets m_i = (e1 + e2) / 2 and n are constants of the linearisation (the rule slm_enable_data_weights
 * states for its weights).  Each kept surfel gives two rows r_i = lambda / sqrt(n) ((x, y) - m_i),
 *   x row: c = (fx / Ze, 0, -fx T.x / Ze^2),  y row: c = (0, fy / Ze, -fy T.y / Ze^2),
 *   per neighbour k: lambda / sqrt(n) w_k [c^T dR(q_k)(p - g_k)/dq_k | c]   (the correspondence term's rows with this c).
 * The loss pass at the trial point evaluates everything afresh there -- new selection, new n, and the full l_i including the
 * constant |e1 - e2|^2 / 4 -- so accept / reject sees the reference's loss; slm_iter_record.loss includes the term, M_grad /
 * M_loss stay the ICP match counts.  The term couples only a surfel's own K nodes: no new pairs, no plan changes.
 *
 * slm_enable_morph: after slm_create, before the first bind.  A weight of 0 switches the option off again.  An enabled
 * solver takes the pair-record form of the data term for every num_neighbors, 4 included (as slm_enable_corr,
 * slm_enable_face and slm_enable_data_weights, with which it may be combined).  Refusals:
 *   SLM_ERR_INVALID      "slm_enable_morph: null argument"
 *                        "slm_enable_morph: weight must be finite"
 *                        "slm_enable_morph: a slot is already bound; call it after slm_create and before the first bind"
 *   SLM_ERR_UNSUPPORTED  "slm_enable_morph: needs the pair-record data path (data_path 0 or 2)"
 *                        "slm_enable_morph: needs a nested-dissection solver_path (0, 2, 3 or 4)"
 *                        "slm_enable_morph: needs the data term (use_data 1)"
 *                        "slm_enable_morph: the solver is sharded (slm_set_shard); the term needs every surfel of the frame on one device"
 *   and, on an enabled solver,
 *   SLM_ERR_UNSUPPORTED  "slm_set_shard: the boundary-morph term is enabled (slm_enable_morph); it needs every surfel of the frame on one device"
 *                        "slm_bind_frame: the boundary-morph term (slm_enable_morph) needs J < 65536"
 *
 * slm_bind_morph: after slm_bind_frame.  Device pointers: img_seg (H,W) int32 is read by this call only (the boundary lists
 * are built here, with a size read-back: the host waits for `stream`); img_seg_conf (C,H,W) float32 and sf_seg (N) int32 are
 * read in place like the frame's own (they must stay valid while the slot is used).  edge_counts_host (C) or null receives
 * the boundary-list lengths.  slm_bind_frame(s) clears the slot's inputs: a slot without them runs without the term.
 *   SLM_ERR_INVALID      "slm_bind_morph: null argument"   "slm_bind_morph: bad slot"
 *   SLM_ERR_UNSUPPORTED  "slm_bind_morph: slm_enable_morph first"
 *                        "slm_bind_morph: num_classes must be in 1..SLM_MAX_CLASSES (4)"
 *   SLM_ERR_UNBOUND      "slm_bind_morph: slm_bind_frame first"
 *
 * slm_morph_loss: out_device[0] = the term's loss at the slot's current beta, [1] = kept n, [2] = candidates; {0, 0, 0} for
 * a slot without inputs.  slm_morph_targets: the selection at the slot's current beta -- kept (N) uint8, target_xy (N,2)
 * float64 (m_i; zeros where not kept), li (N) float64 (l_i; zero where not kept), all device, each may be null.  Refusals
 * (<fn> = either):
 *   SLM_ERR_INVALID      "<fn>: null argument"   "<fn>: bad slot"
 *   SLM_ERR_UNSUPPORTED  "<fn>: slm_enable_morph first"
 *   SLM_ERR_UNBOUND      "<fn>: slm_bind_frame first"   "slm_morph_targets: slm_bind_morph first"
 * Not built: the term on the tuple-sorted MFMA assembly, on sharded frames, for J >= 65536 and without the data term. */
int slm_enable_morph(slm_solver* s, double weight);
int slm_bind_morph(slm_solver* s, int32_t slot, int32_t num_classes, const int32_t* img_seg /*(H,W)*/,
                   const float* img_seg_conf /*(C,H,W)*/, const int32_t* sf_seg /*(N)*/,
                   int32_t* edge_counts_host /*(C) or null*/, void* stream);
int slm_morph_loss(slm_solver* s, int32_t slot, double* out_device /*[3]: loss, kept n, candidates*/, void* stream);
int slm_morph_targets(slm_solver* s, int32_t slot, uint8_t* kept /*(N)*/, double* target_xy /*(N,2)*/,
                      double* li /*(N)*/, void* stream);

/* -- phase timing (bench.py roofline leg) ----------------------------------------- */
/* With profiling on, slm_run brackets each phase of every LM iteration with HIP events
 * recorded on the launch stream.  Phases: */
enum {
  SLM_PH_ZERO = 0,       /* band / rhs zeroing */
  SLM_PH_DATA_GRAD = 1,  /* fused data-term Jacobian pass: exactly ONE kernel launch per iteration */
  SLM_PH_REG_GRAD = 2,   /* 7x7 block gather into the band + ARAP / Rot Jacobian pass */
  SLM_PH_SOLVE = 3,      /* banded Cholesky factor + substitutions (many launches) */
  SLM_PH_DATA_LOSS = 4,  /* fused data-term loss pass: exactly ONE kernel launch per iteration */
  SLM_PH_ACCEPT = 5,     /* regulariser loss + accept/reject */
  SLM_PH_COUNT = 6
};
int slm_profile_enable(slm_solver* s, int32_t on);
/* Synchronises the recorded events; adds per-phase elapsed milliseconds and interval
 * counts into ms_out[SLM_PH_COUNT] / count_out[SLM_PH_COUNT] (host arrays, overwritten),
 * then clears the accumulated intervals. */
int slm_profile_read(slm_solver* s, double* ms_out, int64_t* count_out);

/* -- parity / building-block entry points -------------------------------------- */
/* JtJ and jtl = -Jt r at the slot's current beta.  jtj_dense_device is (P,P)
 * float64 row-major (symmetric, full) or NULL; jtl_device is (P) or NULL. P = 7J. */
int slm_assemble(slm_solver* s, int32_t slot, double* jtj_dense_device, double* jtl_device,
                 void* stream);
/* Sum of squared residuals per term at the slot's current beta:
 * out_device[0..2] = data, arap, rot; out_device[3] = matched count (as double).
 * On a sharded handle (slm_set_shard, world > 1) slm_assemble and slm_loss return THIS RANK'S PARTIAL: its share of the
 * data term plus every regulariser in full.  slm_loss: data loss and matched count of the surfels [N*rank/world,
 * N*(rank+1)/world) of the caller's order, in either data form.  slm_assemble: the data blocks of the same window in the
 * pair-record form, of the rank's workgroups of tuple positions in the tuple-sorted form.  Over the ranks the data parts
 * sum to the frame's; the regularisers are counted world times (sum_r A_r - (world - 1) A_reg is the frame's system).
 * slm_solve on such a handle solves that partial system: it is no step of the frame. */
int slm_loss(slm_solver* s, int32_t slot, double* out_device, void* stream);
/* Assemble at the current beta, add u to the diagonal, Cholesky-solve; writes delta (P).
 * status_device (int32) receives SLM_ITER_OK or SLM_ITER_SOLVER_FAILED. */
int slm_solve(slm_solver* s, int32_t slot, double u, double* delta_device,
              int32_t* status_device, void* stream);
/* LM_Solver.Solver(A, b, "cholesky") on a caller-supplied dense system: A_device is
 * (P,P) float64 row-major symmetric positive definite, b_device (P); writes x (P) and
 * status (SLM_ITER_OK / SLM_ITER_SOLVER_FAILED).  Compatibility entry point (allocates
 * and frees its workspace, synchronises `stream`); the LM loop never uses it. */
int slm_solve_dense(int32_t P, const double* A_device, const double* b_device, double* x_device,
                    int32_t* status_device, void* stream);
/* Per-surfel data-term internals at the current beta: r_device (N) float64
 * (lambda * n.(T(p)-o), 0 where unmatched), match_device (N) uint8,
 * taps_device (N,4) int32 target rows of the four bilinear taps (-1 invalid).
 * The match set (every form of the data term uses this rule; tests/data_edge_cases.py sits on its edges): project T(p) with
 * Z + 1e-8, round (u_, v_) half-to-even; the ROUNDED pixel must satisfy 0 <= v < H-1, 0 <= u < W-1 (so -0.5 <= v_ rounds to
 * a valid 0, and v_ = H-1.5 rounds down only when H-2 is even) and `valid` is read at that rounded pixel alone, not at the
 * taps.  The four taps (floor|ceil v_, floor|ceil u_) must all lie inside the image, be mapped (index_map >= 0) and hold
 * finite points and normals, else the surfel is dropped: a rounded pixel 0 with floor tap -1 is dropped, a valid but
 * unmapped pixel drops through the taps, an invalid but mapped tap still counts.  On an exactly integer coordinate floor ==
 * ceil and BOTH coinciding taps carry weight 1 (the reference's sum, kept).  A point behind the camera that projects onto
 * valid pixels matches; a non-finite projection does not.  taps_device rows are filled where the rounded pixel is valid. */
int slm_data_residuals(slm_solver* s, int32_t slot, double* r_device, uint8_t* match_device,
                       int32_t* taps_device, void* stream);

/* -- Surfels.update (LM variant, no global row) ---------------------------------- */
/* In place on float32 device arrays: skin points, blend+normalise normals, move
 * nodes, rotate node normals.  beta_device is (J,7) float64. */
int slm_apply_update(int32_t N, int32_t J, int32_t K, float* sf_points, float* sf_norms,
                     const int32_t* sf_knn_idx, const float* sf_knn_w, float* ed_points,
                     float* ed_norms, const double* beta_device, void* stream);
/* The same in place on float64 device arrays (the reference's dtype; nothing is rounded). */
int slm_apply_update_f64(int32_t N, int32_t J, int32_t K, double* sf_points, double* sf_norms,
                         const int32_t* sf_knn_idx, const double* sf_knn_w, double* ed_points,
                         double* ed_norms, const double* beta_device, void* stream);

/* -- KNN feeder --------------------------------------------------------------------- */
/* K nearest `nodes` for every query point: squared L2 in float64, ascending, ties ->
 * lowest index.  skip_self != 0 drops the first (self) hit (update_ed).  Outputs:
 * idx (Nq,K) int32, dist (Nq,K) float32 = sqrt(d2). */
int slm_knn(int32_t Nq, int32_t Nn, int32_t K, int32_t skip_self, const float* query_points,
            const float* node_points, int32_t* idx_out, float* dist_out, void* stream);
/* softmax(exp(-dist/radius)) weights (super/nodes.py:166,191) and the stability
 * test any(dist <= radius) (super/nodes.py:182).  radius_mode 0: radius of each
 * neighbour node (surfels); 1: radius of the query node itself (node-node).
 * stable_io (Nq) uint8 is AND-ed in place, may be NULL. */
int slm_knn_weights(int32_t Nq, int32_t K, int32_t radius_mode, const int32_t* idx,
                    const float* dist, const float* node_radii, float* w_out,
                    uint8_t* stable_io, void* stream);

/* float64 feeder with the Semantic-SuPer branches (the reference's tensors are float64):
 * q_seg / node_seg (both or neither): a query only sees the nodes of its own class -- find_knn with
 * num_classes, utils/utils.py:223-242, used by update_ed / update_sfed_knn under hard_seg
 * (super/nodes.py:157-160,172-175); a class with fewer nodes than asked for is an error like the
 * reference's assert (the call synchronises `stream` in that mode).  dist (Nq,K) float64. */
int slm_knn_f64(int32_t Nq, int32_t Nn, int32_t K, int32_t skip_self, const double* query_points,
                const double* node_points, const int32_t* q_seg, const int32_t* node_seg, int32_t* idx_out,
                double* dist_out, void* stream);
/* As slm_knn_weights in float64; num_classes > 0 with q_seg_conf (Nq,C) and node_seg_conf (Nn,C):
 * softmax(exp(-JSD(node, query))^(1/2) * exp(-dist/radius)^(1/2)), super/nodes.py:183-189. */
int slm_knn_weights_f64(int32_t Nq, int32_t K, int32_t radius_mode, const int32_t* idx, const double* dist,
                        const double* node_radii, int32_t num_classes, const double* q_seg_conf,
                        const double* node_seg_conf, double* w_out, uint8_t* stable_io, void* stream);

/* =====================================================================================
 * The reference's DEFAULT per-frame optimiser (no --use_derived_gradient): GraphFit,
 * autograd + SGD(momentum 0.9) / Adam over (J+1,7) rows, last row = global transform T_g.
 *   slm_gf_create / destroy   <- GraphFit.__init__                  super/deform_mesh.py:11-17
 *   slm_gf_bind_frame         <- arguments of GraphFit.forward      super/deform_mesh.py:232-247
 *   slm_gf_run                <- GraphFit.deform_superedg           super/deform_mesh.py:251-379
 *   slm_gf_loss_grad          <- deform_source + get_losses + backward (one evaluation)
 *                                                                    super/deform_mesh.py:25-230
 *   slm_apply_update_gf       <- Surfels.update, autograd variant   super/nodes.py:193-223
 * The gradients that the reference obtains by autograd are hand-derived here (2 J^T r per
 * term, chained through the global row); results are checked against the autograd oracle.
 * ===================================================================================== */
typedef struct slm_gf slm_gf; /* opaque */

typedef struct slm_gf_config {
  int32_t num_iterations;  /* opt.num_optimize_iterations (10) */
  int32_t optimizer;       /* 0 = "SGD" (momentum 0.9, the reference default), 1 = "Adam" */
  int32_t use_data;        /* opt.sf_point_plane */
  int32_t use_arap;        /* opt.mesh_arap (weighted by the node KNN weights on this path) */
  int32_t use_rot;         /* opt.mesh_rot (all J+1 rows) */
  int32_t use_face;        /* opt.mesh_face */
  int32_t max_frames;
  int32_t seg_mode;        /* point-plane semantic weight: 0 none, 1 opt.sf_hard_seg_point_plane,
                              2 opt.sf_soft_seg_point_plane (either implies the point-plane term,
                              super/deform_mesh.py:76-92; needs slm_gf_bind_semantic) */
  int32_t use_bn_morph;    /* opt.sf_bn_morph (needs slm_gf_bind_semantic) */
  int32_t corr_mode;       /* opt.sf_corr: 0 off, 1 opt.sf_corr_loss_type 'point-point', 2 'point-plane'
                              (super/deform_mesh.py:100-109; needs slm_gf_bind_flow) */
  double w_data, w_arap, w_rot, w_face; /* opt.*_weight */
  double lr;               /* opt.learning_rate (5e-5) */
  double w_bn_morph;       /* opt.sf_bn_morph_weight (0.1) */
  double pp_max;           /* > 0: drop squared point-plane residuals >= pp_max (2e-5 when
                              opt.depth_model == "raft_stereo", super/deform_mesh.py:97;
                              ignored with seg_mode != 0 like the reference) */
  double w_corr;           /* opt.sf_corr_weight (0.001) */
} slm_gf_config;
#define SLM_GF_NTERMS 10   /* doubles in the loss-term block of slm_gf_loss_grad / slm_gf_get_partial */

typedef struct slm_gf_frame {
  slm_frame base;                 /* same fields as the LM path (tgt_valid is not read here) */
  const uint8_t* sf_stable;       /* device (N) sf.isStable, or NULL = all stable */
  const void* ed_knn_w;           /* device (J,K_ED) sf.ED_nodes.knn_w   float32, or float64 with base.state_f64 */
  const int32_t* ed_triangles;    /* device (3,Tr) sf.ED_nodes.triangles, or NULL */
  const void* ed_triangle_areas;  /* device (Tr)   sf.ED_nodes.triangles_areas   float32 / float64 */
  int32_t n_triangles;
  int32_t pad;
} slm_gf_frame;

#define SLM_MAX_CLASSES 4
/* Semantic-SuPer inputs of one frame (super/deform_mesh.py:76-92,126-194, super/loss.py:346-399). */
typedef struct slm_gf_semantic {
  int32_t num_classes;        /* opt.num_classes, 1..SLM_MAX_CLASSES */
  int32_t pad;
  const int32_t* sf_seg;      /* device (N)     src.seg        (indexed like sf_points) */
  const float* sf_seg_conf;   /* device (N,C)   src.seg_conf */
  const float* tgt_seg_conf;  /* device (T,C)   trg.seg_conf */
  const float* img_seg_conf;  /* device (C,H,W) inputs[("seg_conf",0)][0] */
  const int32_t* img_seg;     /* device (H,W)   inputs[("seg",0)][0,0] */
} slm_gf_semantic;

int slm_gf_create(const slm_gf_config* cfg, slm_gf** out);
int slm_gf_destroy(slm_gf* g);
/* Binds device pointers to `slot` and resets deform_verts to identity, optimiser state to 0.  The KNN tables are
 * checked as slm_bind_frame checks them (distinct sf_knn_idx ids per row, every id in [0, J), J >= K): SLM_ERR_INVALID
 * and an unbound slot otherwise.  A frame with N = 0 (node terms only) may leave sf_points, sf_knn_idx and sf_knn_w
 * NULL.  Stream-synchronising. */
int slm_gf_bind_frame(slm_gf* g, int32_t slot, const slm_gf_frame* frame, void* stream);
/* After slm_gf_bind_frame: binds the semantic inputs of the slot and extracts, per class, the
 * class-boundary pixels of img_seg in row-major order (find_edge_region with kernel 3 +
 * margin test, utils/utils.py:276-301, super/deform_mesh.py:149-165).  edge_counts_host, if not
 * NULL, receives num_classes counts (synchronises `stream`). */
int slm_gf_bind_semantic(slm_gf* g, int32_t slot, const slm_gf_semantic* sem, int32_t* edge_counts_host,
                         void* stream);
/* After slm_gf_bind_frame: binds the optical flow of the frame for the surfel-correspondence term (corr_mode):
 * flow_device is (2,H,W) float32, channel 0 the x (u) and channel 1 the y (v) displacement in pixels -- the output
 * of the reference's models.optical_flow(src.rgb, inputs[("color",0)]) (super/deform_mesh.py:286-320), which stays
 * with the caller.  The term samples it at each surfel's unrounded projection exactly like
 * F.grid_sample(flow, grid.float()) (bilinear, zero padding, align_corners=False; super/loss.py:318-323), moves
 * the projection by it and evaluates the 4-tap residual there; the gradient includes d(flow)/d(u,v).  May be called
 * again between the iterations of a frame (slm_gf_eval_* / slm_gf_step): it replaces the flow only. */
int slm_gf_bind_flow(slm_gf* g, int32_t slot, const float* flow_device, void* stream);
/* Copies the slot's boundary pixels of `class_id` ((x,y) float pairs, row-major pixel order) to
 * device memory `xy_out_device` (capacity max_points pairs). */
int slm_gf_get_edge_points(slm_gf* g, int32_t slot, int32_t class_id, float* xy_out_device,
                           int32_t max_points, void* stream);
/* num_iterations optimiser steps for slots [0,n_frames), entirely on the device. */
int slm_gf_run(slm_gf* g, int32_t n_frames, void* stream);

/* -- one large frame sharded over the GPUs of a node (BASELINE configs[4]) --
 * After slm_gf_set_shard(rank, world) (before slm_gf_bind_frame) this context evaluates the
 * surfels [N*rank/world, N*(rank+1)/world) of every slot; rank 0 also evaluates the node terms
 * (ARAP / Rot / face).  The library holds no communicator: per optimiser iteration the caller runs
 *     slm_gf_eval_morph   -> all-reduce(sum) of the partial state   (only with use_bn_morph: the
 *                            global kept count scales the back-propagation)
 *     slm_gf_eval_losses  -> all-reduce(sum) of the partial state   (gradient + loss terms)
 *     slm_gf_step
 * on every rank; the partial state is [(J+1)*7 gradient | SLM_GF_NTERMS terms] doubles, moved with
 * slm_gf_get_partial / slm_gf_set_partial (device to device) so that the collective runs on the
 * caller's own buffer (torch.distributed all_reduce = RCCL over xGMI).
 * What the terms hold: behind slm_gf_eval_morph a rank's own morphing sum [5], kept count [6] and candidates flag [7],
 * the rest 0; behind the first all-reduce [5..7] are the frame's (the flag: the number of ranks with a candidate).
 * slm_gf_eval_losses back-propagates with that count, adds the rank's own [0..4], [8], [9] and, on every rank but 0,
 * clears [5..7] again: both exchanges sum the WHOLE state, and rank 0's copy alone carries the frame's morphing entries
 * through the second.  Behind the second all-reduce every entry is the frame's; slm_gf_step turns [5] into the weighted
 * mean and [7] into 0 / 1, so a slm_gf_get_partial behind the step reads the terms slm_gf_loss_grad documents, the same
 * on every rank.  slm_gf_set_shard unbinds every slot (the shard bounds are fixed at the bind): bind the frames again.
 * slm_gf_run refuses a sharded context with world > 1, and so does slm_gf_loss_grad with the morphing term when terms
 * or grad is asked for (one rank cannot take the mean; null terms and grad, which only set deform_verts, stay allowed):
 *   SLM_ERR_UNSUPPORTED  "slm_gf_loss_grad: surfels are sharded and the boundary-morph term is on; its mean needs the global kept count: drive slm_gf_eval_morph / eval_losses with an all-reduce of slm_gf_get_partial behind each (null terms and grad only set deform_verts)"
 * Without the term slm_gf_loss_grad returns the rank's partial sums (the global row divided by J). */
int slm_gf_set_shard(slm_gf* g, int32_t rank, int32_t world);
int slm_gf_eval_morph(slm_gf* g, int32_t n_frames, void* stream);
int slm_gf_eval_losses(slm_gf* g, int32_t n_frames, void* stream);
int slm_gf_step(slm_gf* g, int32_t n_frames, void* stream);
int slm_gf_get_partial(slm_gf* g, int32_t slot, double* out_device, void* stream);
int slm_gf_set_partial(slm_gf* g, int32_t slot, const double* in_device, void* stream);
/* Copies deform_verts ((J+1)*7 doubles) of the slot into caller device memory. */
int slm_gf_get_deform(slm_gf* g, int32_t slot, double* out_device, void* stream);
/* One loss + gradient evaluation at dv_device ((J+1)*7): terms_device[SLM_GF_NTERMS]: [0..3] = face, arap,
 * rot, point_plane losses (already weighted), [4] = point-plane residuals kept, [5] = boundary
 * morphing loss (weighted; NaN when candidates exist but none passes the > 15 test, like the
 * reference's mean over an empty tensor), [6] = surfels kept by the morphing term,
 * [7] = 1 when some class contributed to it (the loss key exists in the reference),
 * [8] = flow-correspondence loss (weighted), [9] = its residuals kept;
 * grad_device ((J+1)*7) = d(sum)/d(dv) with the global row divided by J like the reference. */
int slm_gf_loss_grad(slm_gf* g, int32_t slot, const double* dv_device, double* terms_device,
                     double* grad_device, void* stream);
/* Surfels.update for this path: deform_device is (J+1,7); the global row's translation is
 * added to points / nodes and its rotation applied to the normals (super/nodes.py:204-222). */
int slm_apply_update_gf(int32_t N, int32_t J, int32_t K, float* sf_points, float* sf_norms,
                        const int32_t* sf_knn_idx, const float* sf_knn_w, float* ed_points,
                        float* ed_norms, const double* deform_device, void* stream);
int slm_apply_update_gf_f64(int32_t N, int32_t J, int32_t K, double* sf_points, double* sf_norms,
                            const int32_t* sf_knn_idx, const double* sf_knn_w, double* ed_points,
                            double* ed_norms, const double* deform_device, void* stream);

/* ===================================================================================
 * "Next" row f2: depth map -> per-frame target `new_data`
 *   slm_depth_*  <- depth_preprocessing  utils/data_loader.py:333-523 (+ getN :532-584,
 *                   BackprojectDepth depth/monodepth2/layers.py:139-167, torch_dilate /
 *                   find_edge_region utils/utils.py:152-157,276-301)
 * Produces exactly what slm_bind_frame consumes (tgt_points, tgt_norms, index_map, tgt_valid)
 * plus the other fields of the reference's Data object.  The optional SSIM confidence
 * (opt.disable_ssim_conf == False, needs the stereo pair) is not built.
 * =================================================================================== */
typedef struct slm_depth slm_depth; /* opaque: scratch buffers for one image size */

typedef struct slm_depth_config {
  int32_t H, W;                  /* opt.height, opt.width */
  int32_t data_mode;             /* 0 = opt.data "superv1", 1 = "superv2" */
  int32_t raft_stereo;           /* opt.depth_model == "raft_stereo" (superv1 rules) */
  int32_t dilate_invalid_kernel; /* opt.dilate_invalid_kernel (superv1) */
  int32_t load_depth;            /* opt.load_depth (superv2) */
  int32_t normal_model;          /* 0 = "naive", 1 = "8neighbors" */
  int32_t num_classes;           /* opt.num_classes (with segmentation inputs), <= SLM_MAX_CLASSES */
  int32_t n_del_classes;         /* len(opt.del_seg_classes) <= 3 */
  int32_t del_classes[3];
  float depth_width_range[2];    /* opt.depth_width_range (superv2 without load_depth) */
  float inv_K[9];                /* inputs["inv_K"][0,:3,:3], row-major */
  float fx, fy, cx, cy;          /* inputs["K"][0] */
  double divterm;                /* inputs["divterm"] */
  int32_t use_ssim_conf;         /* hasattr(opt, "disable_ssim_conf") and not opt.disable_ssim_conf (the CLI default):
                                    confs = 0.5 * confs + 0.5 * sigmoid(stereo SSIM confidence), data_loader.py:359-373,477-479 */
  float stereo_P[12];            /* torch.matmul(inputs["K"], inputs["stereo_T"])[0,:3,:] row-major (float32) */
} slm_depth_config;

typedef struct slm_depth_inputs {   /* device pointers */
  const float* depth;            /* (H,W)   inputs[("depth",0)][0,0] */
  const float* color;            /* (3,H,W) inputs[("color",0)][0] */
  const uint8_t* valid_mask;     /* (H,W) or NULL: the opt.load_valid_mask image (superv1) */
  const int32_t* seg;            /* (H,W) or NULL: inputs[("seg",0)][0,0] */
  const float* seg_conf;         /* (C,H,W) or NULL: inputs[("seg_conf",0)][0] */
} slm_depth_inputs;

typedef struct slm_depth_outputs {  /* device pointers; row capacity H*W; NULL = not wanted */
  float* points;                 /* (T,3) data.points (the reference widens these float32 values to float64) */
  float* norms;                  /* (T,3) data.norms */
  float* colors;                 /* (T,3) data.colors */
  double* radii;                 /* (T)   data.radii */
  float* confs;                  /* (T)   data.confs */
  int32_t* index_map;            /* (H,W) data.index_map, -1 invalid */
  uint8_t* valid;                /* (H*W) data.valid */
  int32_t* seg;                  /* (T)   data.seg */
  double* seg_conf;              /* (T,C) data.seg_conf (per-pixel softmax) */
  double* dist2edge;             /* (T)   data.dist2edge */
  uint8_t* inval;                /* (H*W) the invalid-pixel map of step 1 (the reference NaNs depth / disp / pcd there) */
  float* disp_conf;              /* (H,W) inputs[("disp_conf",0)] with use_ssim_conf: SSIM between the image and its
                                    warp through the stereo transform, mean over the channels */
} slm_depth_outputs;

int slm_depth_create(int32_t H, int32_t W, slm_depth** out);
int slm_depth_destroy(slm_depth* d);
/* Runs the whole step on `stream`; *n_valid_host receives T (synchronises the stream). */
int slm_depth_preprocess(slm_depth* d, const slm_depth_config* cfg, const slm_depth_inputs* in,
                         const slm_depth_outputs* out, int32_t* n_valid_host, void* stream);

/* ===================================================================================
 * "Next" row f1: surfel fusion, the step right after the solve every frame
 *   slm_fuse_input_data   <- Surfels.fuseInputData                     super/nodes.py:268-541
 *   slm_fuse_swap_stable  <- Surfels.prepareStableIndexNSwapAllModel   super/nodes.py:543-585
 * for opt.method == "super" and "semantic-super" (slm_fuse_bind_semantic).  Geometry is float64 like the
 * reference's tensors, colours / confidences / time stamps float32.  Unpinned by the reference:
 * the order of surfels with EQUAL confidence on one pixel (torch.sort(descending=True) is not
 * stable); here the lower index comes first.
 * =================================================================================== */
typedef struct slm_fuse slm_fuse; /* opaque: sort / layer-map / compaction scratch */

typedef struct slm_fuse_config {
  int32_t H, W;                   /* opt.height, opt.width */
  int32_t merge_new;              /* !opt.disable_merging_new_surfels */
  int32_t merge_exist;            /* !opt.disable_merging_exist_surfels */
  int32_t add_new;                /* !opt.disable_adding_new_surfels */
  int32_t remove_unstable;        /* !opt.disable_removing_unstable_surfels */
  int32_t phase_test;             /* opt.phase == "test": merged surfels get the frame's time stamp */
  int32_t th_time_steps;          /* opt.th_time_steps (30) */
  double th_dist;                 /* opt.th_dist (0.1) */
  double th_cosine_ang;           /* opt.th_cosine_ang (0.4) */
  float fx, fy, cx, cy;           /* inputs["K"][0] */
} slm_fuse_config;

typedef struct slm_surfel_model {  /* device pointers with room for `cap` rows; n rows in use */
  int32_t n, cap;
  double* points;                 /* (cap,3) sf.points */
  double* norms;                  /* (cap,3) sf.norms */
  float* colors;                  /* (cap,3) sf.colors */
  double* radii;                  /* (cap)   sf.radii */
  float* confs;                   /* (cap)   sf.confs */
  float* time_stamp;              /* (cap)   sf.time_stamp */
  uint8_t* is_stable;             /* (cap)   sf.isStable */
  int32_t* knn_idx;               /* (cap,K) sf.knn_indices */
  double* knn_w;                  /* (cap,K) sf.knn_w */
  float* projdata;                /* (cap,2) sf.projdata */
  int32_t J;
  int32_t K;                      /* opt.num_neighbors, 1..8; 0 is read as 4 (the field was zero padding before round 6: same struct size,
                                     same SLM_ABI_VERSION -- a caller that leaves it 0 gets the former behaviour) */
  const double* ed_points;        /* (J,3) sf.ED_nodes.points */
  const double* ed_radii;         /* (J)   sf.ED_nodes.radii */
  int32_t* merged_into;           /* (cap) or NULL.  slm_fuse_input_data: the surfel that absorbed row i
                                     (-1: none) -- what the reference uses to re-point its tracked
                                     evaluation ids, super/nodes.py:440-445 */
} slm_surfel_model;

typedef struct slm_new_frame {     /* sfdata from depth_preprocessing, device pointers */
  int32_t T, time;                /* rows, sfdata.time */
  const double* points;           /* (T,3) */
  const double* norms;            /* (T,3) */
  const float* colors;            /* (T,3) */
  const double* radii;            /* (T) */
  const float* confs;             /* (T) */
  const uint8_t* valid;           /* (H*W) */
  const int32_t* index_map;       /* (H,W), -1 invalid */
} slm_new_frame;

/* Segmentation fields of Semantic-SuPer (sf.seg / sf.seg_conf / sf.dist2edge exist iff the frames carry
 * them, super/nodes.py:60-75): fused in merge_data (nodes.py:348-353), appended with the new surfels
 * (nodes.py:524-525), compacted by the swap (nodes.py:572-575).  All device pointers. */
typedef struct slm_fuse_semantic {
  int32_t num_classes;            /* C, 1..SLM_MAX_CLASSES */
  int32_t soft_weights;           /* opt.method == "semantic-super": skinning weights
                                     softmax(exp(-JSD(node, surfel))^(1/2) * exp(-d/r)^(1/2)), nodes.py:467-477;
                                     for the NEW surfels only without hard_seg (nodes.py:503-509) */
  int32_t hard_seg;               /* sf.hard_seg: new surfels take their 4 nodes among the nodes of their own
                                     class (find_knn with num_classes, utils/utils.py:223-242); a class with
                                     fewer than 4 nodes is an error like the reference's assert */
  int32_t merge_same_class;       /* hard_seg or opt.data == "superv1": only equal classes merge (nodes.py:314-316) */
  int32_t* seg;                   /* (cap)   sf.seg */
  double* seg_conf;               /* (cap,C) sf.seg_conf */
  double* dist2edge;              /* (cap)   sf.dist2edge */
  const int32_t* ed_seg;          /* (J)     sf.ED_nodes.seg      (hard_seg) */
  const double* ed_seg_conf;      /* (J,C)   sf.ED_nodes.seg_conf (soft_weights) */
  const int32_t* new_seg;         /* (T)     sfdata.seg */
  const double* new_seg_conf;     /* (T,C)   sfdata.seg_conf */
  const double* new_dist2edge;    /* (T)     sfdata.dist2edge */
} slm_fuse_semantic;

int slm_fuse_create(int32_t H, int32_t W, int32_t max_surfels, slm_fuse** out);
/* Binds (sem != NULL) or drops (NULL) the segmentation fields used by the next slm_fuse_input_data /
 * slm_fuse_swap_stable calls on `f`; the struct is copied.  The swap only needs seg / seg_conf / dist2edge. */
int slm_fuse_bind_semantic(slm_fuse* f, const slm_fuse_semantic* sem);
int slm_fuse_destroy(slm_fuse* f);
/* Fuses the frame into the model in place; model->n (host struct) becomes the new row count.
 * Synchronises `stream` (three count read-backs). */
int slm_fuse_input_data(slm_fuse* f, const slm_fuse_config* cfg, slm_surfel_model* model,
                        const slm_new_frame* frame, void* stream);
/* Drops unstable / stale surfels (time = inputs["time"]); model->n becomes the new row count.
 * keep_ids (device, n_keep entries, may be NULL): rows kept regardless (the tracked evaluation
 * points, super/nodes.py:559-560); new_index (device, old row count entries, may be NULL): new row
 * of every old row or -1 (the reference's id_map, super/nodes.py:578-581). */
int slm_fuse_swap_stable(slm_fuse* f, const slm_fuse_config* cfg, slm_surfel_model* model, int32_t time,
                         const int32_t* keep_ids, int32_t n_keep, int32_t* new_index, void* stream);

/* ===================================================================================
 * Forward surfel renderer (Pulsar's blend at the reference's parameters)
 *   slm_render_points  <- Pulsar.forward                      renderer/renderer.py:12-78
 *   slm_gf_render      <- models.renderer(inputs, new_data)   super/deform_mesh.py:292-298
 * Every point is a sphere of radius `radius`.  Pixel (i,j) casts the line through the camera centre and
 * (u,v) = (j,i); sphere k is hit when the distance rho_k from its centre to that line is < radius.  Centres
 * with Z outside [z_near, z_far] are culled.  Of the hits of a pixel, the n_track with the largest
 * zt = (z_far - Z)/(z_far - z_near) take part (equal zt: lower row first); with zt_max the first of them,
 *   w_k = (1 - rho_k/radius) exp((zt_k - zt_max)/gamma),   w_bg = exp((bg_eps - zt_max)/gamma),
 *   colour = (sum w_k c_k + w_bg bg) / (sum w_k + w_bg),   bg where nothing is hit.
 * Positions are rounded to float32 first (Pulsar is called with points.float()).  The image is written
 * (height,width,3) float32, channels last.  Results are bitwise reproducible.  Each call synchronises
 * `stream` once (a 8-byte read-back that sizes the tile lists).
 * =================================================================================== */
typedef struct slm_render slm_render; /* opaque: per-surfel projections, tile lists and their scratch */

#define SLM_RENDER_MAX_TRACK 64
typedef struct slm_render_params {
  int32_t width, height;   /* w = int(W view_scale), h = int(H view_scale) */
  int32_t n_track;         /* hits that take part per pixel, 1..SLM_RENDER_MAX_TRACK (64) */
  int32_t points_f64;      /* slm_render_points: positions are float64 (else float32) */
  double focal;            /* f = K[0,0] view_scale (one focal length: fy is not used) */
  double ccx, ccy;         /* principal point: u = f X/Z + ccx, v = f Y/Z + ccy */
  double radius;           /* opt.renderer_rad, the same for every point */
  double z_near, z_far;    /* 0.01, 15.0 */
  double gamma;            /* 1e-5 */
  double bg_eps;           /* 1e-9 */
  float bg[3];             /* background colour */
  int32_t pad;
} slm_render_params;

/* Renders of up to H x W pixels and max_points points. */
int slm_render_create(int32_t H, int32_t W, int32_t max_points, slm_render** out);
int slm_render_destroy(slm_render* r);
/* points (N,3) device, float32 or float64 (p->points_f64); colors (N,3) device float32, row i at
 * colors + i * color_stride (color_stride >= 3).  image (height,width,3) device float32.  front_id (height,width)
 * int32 (the row of the first hit, -1 where nothing is hit) and hit_count (height,width) int32 (hits that took
 * part, <= n_track) may be NULL. */
int slm_render_points(slm_render* r, const slm_render_params* p, int32_t N, const void* points, const float* colors,
                      int32_t color_stride, float* image, int32_t* front_id, int32_t* hit_count, void* stream);
/* The same for the CURRENT deformed stable surfels of GraphFit slot `slot` (deform_source's new_data.points,
 * global row included, super/deform_mesh.py:198-230), computed on the device from the slot's deform_verts.
 * Colours are indexed by surfel row like sf_points (pass sf.colors; rows of unstable surfels are not read),
 * front_id holds surfel rows.  p->points_f64 is ignored. */
int slm_gf_render(slm_gf* g, int32_t slot, slm_render* r, const slm_render_params* p, const float* colors,
                  int32_t color_stride, float* image, int32_t* front_id, int32_t* hit_count, void* stream);

/* Renderer backward and the render loss of GraphFit (opt.render_loss, super/deform_mesh.py:113-123)
 *   slm_render_backward   <- the gradient Pulsar's backward feeds into new_data.points   super/deform_mesh.py:115,317
 *   slm_render_ssim_loss  <- SSIM(kernel=11) + mask + selection + weighted sum           super/deform_mesh.py:115-121,
 *                                                                                        depth/monodepth2/layers.py:217-247
 * slm_render_backward: dL/dP of the image of the LAST forward on `r` (slm_render_points or slm_gf_render), the exact
 * derivative of the blend above.  With W = sum w_k + w_bg, C the float64 colour and g = dL/dC of the pixel,
 *   dL/dP_k = sum over the pixels k takes part in of  g.(c_k - C)/W ( -(e_k/radius) drho_k/dP - w_k/(gamma (z_far - z_near)) z )
 * with e_k = exp((zt_k - zt_max)/gamma), drho/dP = (P - (P.d)d)/rho for the pixel's unit ray d (0 at rho = 0).  Hit
 * membership, rho < radius and the n_track cut are the forward's (discrete); zt_max cancels.  P is the float32-rounded
 * centre and the gradient passes the rounding unchanged.  grad_image (height,width,3) float64 device; grad_points
 * (N,3) float64 device, N the forward's point count -- for slm_gf_render surfel rows, 0 on unstable rows and on culled
 * points.  p must equal the forward's parameters field by field.  SLM_ERR_INVALID when no forward completed on `r` or
 * p differs.  Bitwise reproducible (no float atomics); does not synchronise. */
int slm_render_backward(slm_render* r, const slm_render_params* p, const double* grad_image, double* grad_points,
                        void* stream);
/* slm_render_backward_ex: slm_render_backward with the colour gradient as well (Pulsar's autograd gives both).  With W and
 * g as above,
 *   dL/dc_k = sum over the pixels k takes part in of  g w_k / W    (per channel)
 * at the forward's hit sets (rho < radius, the n_track cut).  Colours are the forward's float32 copy and the gradient
 * passes that cast unchanged.  grad_points and grad_colors: (N,3) float64 device, rows as for slm_render_backward (0 on
 * unstable rows and on culled points); either may be NULL, not both.  grad_points equals slm_render_backward's bitwise,
 * and grad_colors does not depend on whether grad_points is requested.  The same two passes and the same refusals; the
 * slab grows from 3 to 6 doubles per tile-list entry when both are requested.  Bitwise reproducible; does not
 * synchronise. */
int slm_render_backward_ex(slm_render* r, const slm_render_params* p, const double* grad_image, double* grad_points,
                           double* grad_colors, void* stream);
/* The render loss at the image (h,w,3) float32 `image_hwc` (a render) against the target (3,h,w) float32 `target_chw`
 * (inputs[("color",0)][0]): per channel monodepth2's SSIM with kernel 11 -- reflection padding 5, 11x11 box means of
 * x, y, x^2, y^2, xy, C1 = 0.01^2, C2 = 0.03^2, clamp((1 - n/d)/2, 0, 1) -- then m = mean_c(SSIM_c)^2; a pixel is kept
 * when every pixel of its border-clipped 11x11 window has all three image channels > 0 (maxpool11(-min_c x) < 0) and
 * m < 0.1.  loss_out (device, 2 doubles) = weight sum_kept m (fixed summation order), kept pixel count.  grad_image
 * (h,w,3) float64 device, may be NULL: dL/dimage with the mask and the selection constant and the clamp passing the
 * gradient where 0 <= value <= 1; the target gets none.  Arithmetic is float64 on the float32 inputs (the reference
 * runs float32).  h, w >= 6.  Allocates its scratch stream-ordered; does not synchronise. */
int slm_render_ssim_loss(int32_t h, int32_t w, const float* image_hwc, const float* target_chw, double weight,
                         double* loss_out, double* grad_image, void* stream);

/* Per-point radii (Pulsar's vert_rad is a float32 (N,) tensor; the surfel model carries one radius per surfel)
 *   slm_render_points_radii    <- Pulsar's vert_rad as the caller's (N,) tensor
 *   slm_gf_render_radii        <- the same for the deformed stable surfels of a GraphFit slot
 *   slm_render_backward_radii  <- dL/dP, dL/dc and dL/dr of such a render
 * The blend above with r_k, the float32 `radii[k]` widened to double, in place of `radius`: sphere k is hit when
 * rho_k < r_k, its silhouette box is that of r_k (a sphere with Z^2 - r_k^2 <= 0 is a candidate of every pixel), and
 *   w_k = (1 - rho_k/r_k) exp((zt_k - zt_max)/gamma).
 * A row whose radius is not finite or not > 0 is culled like a centre outside [z_near, z_far]: it is hit nowhere, front_id
 * never names it and its gradient rows are 0.  The order of the hits, the n_track cut, the tie rule, the background term and
 * the float64 arithmetic are unchanged; with all radii equal to one float32 value v the results are bitwise those of the
 * one-radius entries at radius = (double)v.  p->radius must still be valid (> 0, finite) and must still match at the
 * backward, but the geometry does not read it.  The context keeps the radii with the centres, so a later backward does not
 * read `radii` again.  Other arguments, the synchronisation and the reproducibility are those of slm_render_points /
 * slm_gf_render.  radii: (N) float32 device; for slm_gf_render_radii indexed by surfel row like the colours (rows of
 * unstable surfels are not read). */
int slm_render_points_radii(slm_render* r, const slm_render_params* p, int32_t N, const void* points, const float* radii,
                            const float* colors, int32_t color_stride, float* image, int32_t* front_id,
                            int32_t* hit_count, void* stream);
int slm_gf_render_radii(slm_gf* g, int32_t slot, slm_render* r, const slm_render_params* p, const float* radii,
                        const float* colors, int32_t color_stride, float* image, int32_t* front_id, int32_t* hit_count,
                        void* stream);
/* slm_render_backward_ex with the radius gradient as well.  After a per-point forward, with s_k = g.(c_k - C)/W,
 *   dL/dP_k and dL/dc_k as above with r_k in place of `radius`,
 *   dL/dr_k = sum over the pixels k takes part in of  s_k e_k rho_k / r_k^2      (dw_k/dr_k = e_k rho_k / r_k^2)
 * at the forward's hit sets (discrete).  The gradient passes the float32 radius unchanged.  grad_radii: (N) float64 device,
 * 0 on culled and unstable rows.  Any of the three outputs may be NULL, not all three; each output is bitwise the same
 * whichever others are requested, and grad_points / grad_colors equal those of slm_render_backward /
 * slm_render_backward_ex, which after a per-point forward use the stored radii too.  After a forward with one radius it
 * serves grad_points and grad_colors like slm_render_backward_ex and refuses a non-NULL grad_radii with SLM_ERR_INVALID
 * ("slm_render_backward_radii: grad_radii after a forward with one radius").  The same two passes (one more slab double
 * per tile-list entry), the same refusals otherwise.  Bitwise reproducible (no float atomics); does not synchronise. */
int slm_render_backward_radii(slm_render* r, const slm_render_params* p, const double* grad_image, double* grad_points,
                              double* grad_colors, double* grad_radii, void* stream);
/* N-channel features (Pulsar's n_channels: a feature vector per point -- class probabilities, a confidence, a depth
 * column, colour plus any of these -- blended in one geometry pass)
 *   slm_render_points_channels    <- Renderer(..., n_channels=C)
 *   slm_render_backward_channels  <- dL/dP, dL/dfeatures and dL/dr of such a render
 * The blend above with channel c of `features` in place of a colour channel, 1 <= C <= SLM_RENDER_MAX_CHANNELS:
 *   out_c = (sum_k w_k f_kc + w_bg bg_c) / (sum_k w_k + w_bg),   bg_c where nothing is hit.
 * The geometry, the culling (a bad per-point radius included), the hit test, the order of the hits with its tie rule, the
 * n_track cut, w_k, w_bg, front_id and hit_count are those of slm_render_points (radii == NULL: p->radius for every point)
 * or slm_render_points_radii (radii (N) float32 device).  Every channel is summed on its own, in float64, by one lane in
 * list order, with the operations of the three-channel entries: channel c is bitwise what slm_render_points /
 * slm_render_points_radii write for the same column of numbers and the same background value, and with C == 3 and
 * bg == p->bg the whole image is theirs.  features (N,C) device float32, row i at features + i * feature_stride
 * (feature_stride >= C); bg: C floats on the HOST (p->bg is not read); image (height,width,C) device float32.  The context
 * keeps a copy of the features, so a later backward does not read `features` again; the buffers that are C wide are
 * allocated by the first such call on a context.  One synchronisation of `stream`, as for slm_render_points.
 * SLM_ERR_INVALID, before any device call, for C outside 1..8, feature_stride < C, or a null bg, image or (N > 0) features. */
#define SLM_RENDER_MAX_CHANNELS 8
int slm_render_points_channels(slm_render* r, const slm_render_params* p, int32_t N, const void* points,
                               const float* radii /* NULL: p->radius for every point */, int32_t C, const float* features,
                               int32_t feature_stride /* >= C */, const float* bg /* host, C floats; p->bg is not read */,
                               float* image /* (height,width,C) */, int32_t* front_id, int32_t* hit_count, void* stream);
/* The backward of the last forward on `r`, which must be a completed slm_render_points_channels with the same C and the same
 * p (field by field, bg excepted).  With F the float64 channels of a pixel, g = dL/dF and s_k = sum_c g_c (f_kc - F_c) / W,
 *   dL/dP_k and dL/dr_k as for slm_render_backward_radii with that s_k,
 *   dL/df_kc = sum over the pixels k takes part in of  g_c w_k / W
 * at the forward's hit sets.  grad_image (height,width,C) float64 device; grad_points (N,3), grad_features (N,C), grad_radii
 * (N) float64 device, 0 on culled rows.  Any of the three may be NULL, not all three; each is bitwise the same whichever
 * others are requested.  grad_radii after a forward with radii == NULL is refused ("slm_render_backward_channels: grad_radii
 * after a forward with one radius").  After a channels forward slm_render_backward, _ex and _radii refuse (the per-pixel
 * record is laid out differently, also at C == 3), and this entry refuses after a three-channel forward.  The same two
 * store-and-sum passes: a slab entry holds 3 + C + 1 doubles when everything is requested.  Bitwise reproducible (no float
 * atomics); does not synchronise.  There is no GraphFit twin: nothing in GraphFit consumes more than three channels. */
int slm_render_backward_channels(slm_render* r, const slm_render_params* p, int32_t C,
                                 const double* grad_image /* (height,width,C) */, double* grad_points /* (N,3) */,
                                 double* grad_features /* (N,C) */, double* grad_radii /* (N) */, void* stream);
/* After slm_gf_bind_frame: binds dL/dP (N,3) float64 device, by surfel row, of an outside term (the render loss:
 * slm_render_backward of an slm_gf_render).  Every later evaluation of the slot -- slm_gf_eval_losses, slm_gf_loss_grad,
 * each iteration of slm_gf_run -- adds it to each stable surfel's dL/dP before the chain rule to the node rows and the
 * global row (the global row's gradient is then divided by J as for every term).  The gradient belongs to the current
 * deform_verts: bind it again before every evaluation.  NULL clears it; slm_gf_bind_frame clears it too.  The buffer
 * is read, not copied.  Synchronises `stream`. */
int slm_gf_bind_point_grad(slm_gf* g, int32_t slot, const double* grad_device, void* stream);

/* The render loss as a term of the run: after slm_gf_bind_frame, binds to the slot the render of its deformed stable surfels
 * on `r` (slm_gf_render; radii != NULL: slm_gf_render_radii, (N) float32 device by surfel row), the SSIM loss of that render
 * against target_chw with `weight` (slm_render_ssim_loss) and its point gradient (slm_render_backward).  Every later
 * evaluation of the slot -- slm_gf_eval_losses, slm_gf_loss_grad, each iteration of slm_gf_run for every slot of the batch
 * that has the term -- enqueues the three in front of its losses and adds the gradient like a bound point gradient.  Those
 * calls stay enqueue-only: no synchronisation, read-back or allocation.
 *   The tile lists cannot be sized from a read-back then, so their capacity is fixed here: one render of the slot's current
 * state through slm_gf_render's path (one synchronisation) gives the total T0, the context's lists and slab are grown for
 * L = T0 + T0 / 4 + 1024 entries, and L is the entry limit of every render of the term.  A device-side guard compares each
 * render's total with L.  Within L the image, the per-pixel records and the point gradient are bitwise those of slm_gf_render
 * + slm_render_backward on the same state.  Over L the render is EMPTY -- no tile-list entry is written or read, the image is
 * the background, the point gradient 0 -- and the context's status record counts it: read slm_gf_render_loss_status after the
 * run and bind again with a larger entry_limit.  entry_limit > 0 sets L to exactly that value (the buffers hold at least the
 * sizing render's head-room as well, so a limit below the need only empties renders).
 *   The slot owns the image, its gradient, the point gradient and the loss; colors (rows of color_stride >= 3 floats, by
 * surfel row), radii and target_chw ((3,height,width) float32 device) are read, not copied, and `r` must outlive the binding.
 * r == NULL clears the term; slm_gf_bind_frame clears it too.  Refused: a slot with a point gradient bound
 * (slm_gf_bind_point_grad, which in turn refuses a slot with the term), a context bound to another slot of `g`, sharded
 * surfels, height or width < 6, and whatever slm_gf_render refuses.  Afterwards slm_render_backward* on `r` refuse until the
 * next forward through an existing entry point.  Synchronises `stream`. */
int slm_gf_bind_render_loss(slm_gf* g, int32_t slot, slm_render* r, const slm_render_params* p,
                            const float* radii /* NULL: p->radius */, const float* colors, int32_t color_stride,
                            const float* target_chw, double weight, int64_t entry_limit /* 0: from a sizing render */,
                            void* stream);
/* out_host: {weighted loss, kept pixel count} of the term's last evaluation (0, 0 before the first), the renders over the
 * entry limit and the largest tile-list total since the bind (the sizing render included).  Synchronises `stream`. */
int slm_gf_render_loss_status(slm_gf* g, int32_t slot, double out_host[4], void* stream);
/* Copies the render (height,width,3) float32 and the point gradient (N,3) float64 of the term's last evaluation to device
 * buffers (either may be NULL); after the bind and before an evaluation: the sizing render and zeros.  Does not synchronise. */
int slm_gf_render_loss_read(slm_gf* g, int32_t slot, float* image_device, double* grad_points_device, void* stream);

/* ===================================================================================
 * "Next" row f3: ED-graph construction at frame 0
 *   slm_graph_init  <- init_graph + DirectDeformGraph (grid_mesh)   super/graph_encoder.py:11-67,128-195
 * Anchors on a pixel grid of step opt.mesh_step_size (row-major numbering), four edges and two
 * triangles per grid cell (kept when all their vertices are valid anchors), node radius = mean
 * length of the incident edges (isolated nodes get the mean of the others), triangle rest areas.
 * Capacities: nodes <= ceil((H-1)/step) * ceil((W-1)/step), edges <= 4 * nodes, triangles <= 2 * nodes;
 * edge_index / triangles are written row by row with row stride `cap_nodes * 4` / `cap_nodes * 2`.
 * =================================================================================== */
typedef struct slm_graph_outputs {  /* device pointers */
  int32_t cap_nodes, pad;
  double* points;                 /* (cap_nodes,3) graph.points */
  double* norms;                  /* (cap_nodes,3) graph.norms */
  double* radii;                  /* (cap_nodes)   graph.radii */
  int32_t* edge_index;            /* (2, 4*cap_nodes) graph.edge_index */
  double* edges_lens;             /* (4*cap_nodes)    graph.edges_lens */
  int32_t* triangles;             /* (3, 2*cap_nodes) graph.triangles */
  double* triangles_areas;        /* (2*cap_nodes)    graph.triangles_areas */
} slm_graph_outputs;

/* valid (H*W) = data.valid, index_map (H,W) = data.index_map, points / norms (T,3) = data.points /
 * data.norms.  counts_host[3] = {nodes, edges, triangles}.  Synchronises `stream`. */
int slm_graph_init(int32_t H, int32_t W, int32_t step, const uint8_t* valid, const int32_t* index_map,
                   const double* points, const double* norms, const slm_graph_outputs* out,
                   int32_t* counts_host, void* stream);

/* Semantic-SuPer variant (super/graph_encoder.py:134-151,190-192): seg_conf (T,C) = data.seg_conf; every
 * node also gets node_seg_conf (cap_nodes,C) = seg_conf of its row and node_seg (cap_nodes) = first maximum;
 * prune_class_edges (opt.hard_seg and opt.mesh_face): edges / triangles whose vertices differ in class are
 * dropped before lengths, radii and areas are computed. */
int slm_graph_init_semantic(int32_t H, int32_t W, int32_t step, const uint8_t* valid, const int32_t* index_map,
                            const double* points, const double* norms, int32_t num_classes, const double* seg_conf,
                            int32_t prune_class_edges, const slm_graph_outputs* out, int32_t* node_seg,
                            double* node_seg_conf, int32_t* counts_host, void* stream);

/* Diagnostics: {device buffer reallocations in the LM solver, bytes asked for, symbolic analyses,
 * plan reuses with a changed pair list} since the library was loaded. */
/* Form of the numeric phase the last slm_run / slm_lm_solve / slm_solve of this solver enqueued: 0 = per-level
 * launches, 1 = task graph (one persistent launch), 2 = hybrid (per-level launches below, task graph for the top of
 * the tree), -1 = none yet (block-banded path or nothing run). */
int slm_debug_last_solver_form(slm_solver* s);
/* Mode word of the last task-graph launch (k_fdag) this solver enqueued: bit 0 = XCD-affine ticket streams (a multiple of
 * 8 frames per launch on a device whose launches land on the XCD ids 0..7); -1 = the last solve ran no task graph. */
int slm_debug_last_dag_mode(slm_solver* s);
int slm_debug_counters(int64_t out[4]);
/* Diagnostics: copies a solver work buffer of the slot to HOST memory (synchronises `stream`): what = 0 front
 * tiles, 1 front vectors, 2 inverses of the diagonal factor blocks, 3 delta.  *n_doubles receives the buffer's
 * length; at most max_doubles are copied. */
/* Diagnostics of the task-graph solver (solver_path 2): with on != 0 every task of the slot records
 * {start, last dependency ready, end} (10 ns ticks) and its workgroup into a trace that slm_debug_read returns
 * as what = 4 (24 int64 per task, reinterpret the doubles) and what = 5 (the task words, 2 int32 per task; what = 6: the
 * task words of the top-of-tree list the hybrid form runs, which the trace is indexed by after a hybrid solve). */
int slm_debug_dag_trace(slm_solver* s, int32_t slot, int32_t on, void* stream);
/* Diagnostics / tests: the deadline of a wait inside the task-graph solver, in ticks of the 100 MHz wall clock, for every
 * solver of the process on the current device (0 restores the default of 3 s).  A wait that exceeds it aborts the launch;
 * the slots whose solve did not finish record SLM_ITER_SOLVER_TIMEOUT and stop like after a failed factorisation. */
int slm_debug_dag_timeout(int64_t ticks);
/* Tests: leaves slots [0, n_frames) in the state an ABORTED task-graph launch leaves behind (flags reset, abort flag up,
 * no front has published its solution), runs the check every launch ends with and the accept step: every slot must
 * record SLM_ITER_SOLVER_TIMEOUT for its current iteration and stop (also the slots past the first 64 of a batch). */
int slm_debug_dag_abort(slm_solver* s, int32_t n_frames, void* stream);
int slm_debug_read(slm_solver* s, int32_t slot, int32_t what, double* host_out, int64_t max_doubles,
                   int64_t* n_doubles, void* stream);
/* Diagnostics / tests: copies one array of the slot's per-frame assembly plan (the output of the preparation, slm_prep.hip) to
 * HOST memory as raw bytes (synchronises `stream`): what = 0 s_idx, 1 grp_run, 2 run_nodes, 3 s_w, 4 blk_key, 5 blk_start,
 * 6 blk_entry, 7 wg_first, 8 wg_last, 9 run_lidx, 10 blk2_start, 11 blk2_entry, 12 s_pts.  *n_bytes receives the array's
 * length; at most max_bytes are copied.  (tests/test_gpu_prepare_binned.py: the binned preparation against the rocPRIM
 * pipeline, array by array; tests/test_gpu_prep_plan.py: both against the NumPy construction of tests/prep_plan_model.py.)
 * A slot without that plan refuses 0..12 with SLM_ERR_UNSUPPORTED "slm_debug_read_plan: the slot has no tuple-sorted plan".
 * what = 13..16 read the pair plan of a slot on the pair-record form (num_neighbors != 4, or an enabled slm_enable_corr /
 * _data_weights / _face / _morph), all int32: 13 blk_key (coupled pairs: the ascending distinct keys max(a,b) * J + min(a,b),
 * unsigned), 14 sf_pidx (N, K(K+1)/2: the position in blk_key of the pair (c[ra], c[rb]) at slot ra(ra+1)/2 + rb, c the
 * surfel's ids ascending), 15 sf_perm (N: the surfels in lexicographic order of c, ties by surfel id), 16 tri_pidx (F, 6: the
 * positions of a face-mesh triangle's pairs -- the diagonals of vertex 0, 1, 2, then (0,1), (0,2), (1,2); length 0 without a
 * mesh).  A slot without a pair plan refuses them with SLM_ERR_UNSUPPORTED "slm_debug_read_plan: the slot has no pair plan".
 * (tests/test_gpu_pair_plan.py: against the NumPy construction of tests/pair_plan_model.py.) */
int slm_debug_read_plan(slm_solver* s, int32_t slot, int32_t what, void* host_out, int64_t max_bytes, int64_t* n_bytes,
                        void* stream);

/* =====================================================================================
 * Global rigid pre-alignment of the LM path: T_g ahead of the node solve.
 * The first-order path carries the reference's global row T_g (super/deform_mesh.py:213-223); the LM path has none and
 * must explain bulk motion of the scene against the camera with its per-node transforms.  This stage estimates
 * T_g = (q, t) by the reference's own LM loop (super/LM.py:81-122) run on ONE node at the origin -- every surfel attached
 * to it with weight 1, K = 1, beta_g = (q, t) started at identity -- with the terms
 *   data  r_i = w_data n.(T(p_i) - o),  T(p) = R(q) p + t  (the un-normalised quaternion formula of the node solve)
 *   Rot   w_rot (1 - |q|^2), in float32 like the node solve's; ALWAYS on here (without it |q| is a free scale)
 * and the rules of the node solve's data term (see slm_data_residuals: projection with Z + 1e-8, validity on the rounded
 * pixel, four taps, NaN drop, the integer-coordinate double tap; c = n(I - A) + e B with the plain Z in dPi; the row
 * w_data [c dR(q)p/dq | c]).  The data term is the plain one unless slm_rigid_set_terms asks for more (below).  u, v, minimal_loss,
 * accept / reject under phase_test and the fresh match set of the loss at the trial point are LM()'s.  The caller then
 * moves the model by T_g (slm_rigid_transform) and runs the unchanged node LM on the moved model.
 *
 * A free-standing context (like slm_depth / slm_fuse / slm_render): independent of slm_solver, the caller's arrays are read
 * in place, nothing is bound.  Of each slm_frame the stage reads N, T, H, W, fx .. cy, sf_points, state_f64 and the four
 * target fields; the KNN and node fields are ignored and may be null.
 *
 * The sums (the 7 x 7 normal equations, the loss, the match count) have a FIXED order: every 256 consecutive surfels give
 * one partial (lane butterflies, then the four waves through LDS), one wave adds the partials in index order.  No float
 * atomics; two runs give the same bits, whatever grid the launch chose.  One pass over the surfels per iteration yields the
 * loss at the trial point AND the normal equations there (the next iteration's, if the step is accepted); a one-wave kernel
 * accepts or rejects, damps, factors (Cholesky), solves and writes the next trial point and the record: two launches per
 * iteration, no host synchronisation, the frame index a grid dimension.
 *
 * slm_rigid_run: the whole loop for frames[0 .. n_frames) (an array in HOST memory, copied by the call) into slots
 *   [0, n_frames).  N = 0 or T = 0 is not an error: the result is identity, every record has M_grad = 0; so does a frame
 *   where nothing matches (its system is the Rot term plus u I: positive definite, zero right-hand side).  A failed
 *   factorisation (a pivot that is not > 0, NaN included) records SLM_ITER_SOLVER_FAILED for that iteration and ends that
 *   frame's loop like LM()'s break (later records SLM_ITER_NOT_RUN); the other frames of the batch go on.
 * slm_rigid_get: Tg7_device[7] = (q / |q|, t) of the slot's last run.  slm_rigid_get_beta: the raw 7 doubles.
 * slm_rigid_get_records: synchronises `stream`, copies min(max_records, num_iterations of the last run) records to HOST
 *   memory; *n_out (may be null) receives that count.
 * slm_rigid_assemble: the normal equations and the loss of ONE frame at a given point (what slm_assemble / slm_loss are
 *   to the solver): JtJ49 (7,7) row-major symmetric, jtl7 = -J^T r, loss_M = {sum of squared residuals, matched count};
 *   each output is device memory and may be null.  Uses a slot of its own: the results of a run are kept.
 * slm_rigid_transform: in place on (n,3) device arrays, float64 (f64 != 0) or float32: p <- R(q) p + t,
 *   n <- R(q) n / max(|R(q) n|, 1e-12) (F.normalize: a zero normal stays zero); norms may be null.  For surfels and nodes.
 *
 * Refusals (<fn> = the entry point):
 *   SLM_ERR_INVALID    "<fn>: null argument"
 *                      "slm_rigid_create: max_frames must be >= 1"
 *                      "slm_rigid_run: n_frames must be in 1..max_frames"
 *                      "<fn>: num_iterations must be >= 0"           (slm_rigid_run, slm_rigid_assemble)
 *                      "<fn>: H and W must be >= 2"
 *                      "<fn>: N and T must be >= 0"
 *                      "<fn>: N > 0 needs sf_points"
 *                      "<fn>: T > 0 needs tgt_points, tgt_norms, index_map and tgt_valid"
 *                      "<fn>: bad slot"                              (slm_rigid_get, _get_beta, _get_records)
 *                      "slm_rigid_get_records: max_records must be >= 0"
 *                      "slm_rigid_transform: n must be >= 0"
 *                      "slm_rigid_abi_check: caller's slm_rigid_config has <a> bytes, the library's <b>"
 *   SLM_ERR_NO_DEVICE  "slm_rigid_create: no HIP device visible"
 * ===================================================================================== */
typedef struct slm_rigid slm_rigid; /* opaque */

typedef struct slm_rigid_config {
  int32_t num_iterations;   /* opt.num_optimize_iterations */
  int32_t phase_test;       /* opt.phase == "test": accept/reject; 0 = "train": always accept */
  double w_data;            /* opt.sf_point_plane_weight */
  double w_rot;             /* opt.mesh_rot_weight */
  double u0;                /* LM(..., u=10) */
  double v;                 /* LM(..., v=7.5) */
  double minimal_loss0;     /* LM(..., minimal_loss=1e10) */
} slm_rigid_config;

/* The handshake of this stage's one struct (slm_abi_check keeps its signature: the stage is an addition to ABI 3, no
 * existing struct or entry point changed); bindings call it once after loading the library (super_amd/_lib.py does). */
int slm_rigid_abi_check(int32_t sizeof_slm_rigid_config);
int slm_rigid_create(int32_t max_frames, slm_rigid** out);
int slm_rigid_destroy(slm_rigid* r);
int slm_rigid_run(slm_rigid* r, const slm_rigid_config* cfg, int32_t n_frames, const slm_frame* frames /*host array*/,
                  void* stream);
int slm_rigid_get(slm_rigid* r, int32_t slot, double* Tg7_device, void* stream);
int slm_rigid_get_beta(slm_rigid* r, int32_t slot, double* beta7_device, void* stream);
int slm_rigid_get_records(slm_rigid* r, int32_t slot, slm_iter_record* host_out, int32_t max_records, int32_t* n_out,
                          void* stream);
int slm_rigid_assemble(slm_rigid* r, const slm_rigid_config* cfg, const slm_frame* frame, const double* beta7_device,
                       double* JtJ49_device, double* jtl7_device, double* loss_M_device /*[2]*/, void* stream);
int slm_rigid_transform(int32_t n, void* points, void* norms /*may be null*/, int32_t f64, const double* Tg7_device,
                        void* stream);

/* -- opt-in terms of the rigid stage (additions to ABI 3; a context that never calls them runs the plain stage) ----------
 * The plain stage sees point-to-plane rows only: motion ALONG a near-planar surface is invisible to it, and a tool that
 * crosses the view pulls T_g with it.  Two terms of the node solve can be carried by the stage:
 *   correspondence rows  (slm_enable_corr's modes and weight): a surfel with valid_i adds, for one node at the origin with
 *       weight 1, the rows corr_weight [c dR(q)p/dq | c] with residual corr_weight c.(R(q)p + t - o_i); c = e_x, e_y, e_z in
 *       mode 1 (point-point), c = n_i in mode 2 (point-plane).  The targets do not move with beta_g.  A surfel adds these
 *       rows whether or not the data term matches it, and the other way round.
 *   data weights  (slm_enable_data_weights's seg_mode and pp_max): every matched data row and its residual are scaled by
 *       sqrt(w_i), w_i evaluated at the point of the pass from s_i = (n.e)^2 without w_data -- seg_mode 1 hard / 2 soft
 *       semantic weight (pp_max then ignored), seg_mode 0 with pp_max > 0 the truncation [s_i < pp_max].  Weight 0 is
 *       matched and contributes nothing: M_grad / M_loss stay the match set's counts.
 * The iteration's loss is weighted data + correspondence + Rot; one pass still yields the loss at the trial point and the
 * normal equations there, both with w at that point.  The sums keep their fixed order (same partials, same reduction):
 * two runs give the same bits.
 *
 * slm_rigid_set_terms: the context's terms for later slm_rigid_run / slm_rigid_assemble calls; (0, 0, 0, 0) is the plain
 *   stage.  EVERY call clears every slot's inputs.
 * slm_rigid_set_corr / slm_rigid_set_semantic: register DEVICE arrays that later runs of that slot read in place -- pts
 *   (N,3), nrm (N,3; may be null in mode 1), valid (N); sf_seg (N), sf_seg_conf (N,C), tgt_seg_conf (T,C).  Slots
 *   [0, max_frames) are slm_rigid_run's, slot max_frames is slm_rigid_assemble's own.  Null pts / null sf_seg clears the
 *   slot's inputs.  A slot without correspondences runs without that term; with seg_mode != 0 a run or assemble over a slot
 *   without semantic inputs is refused: there is no silent unweighted run.
 * slm_rigid_corr_targets: the targets slm_bind_corr_flow builds, for a raw frame and without a context: the unrounded
 *   projection of sf_points, the flow (2,H,W float32) sampled grid_sample-style, margin 1, all four taps mapped and finite;
 *   zeros where invalid.  Reads N, H, W, the intrinsics, sf_points, state_f64 and the target tables.  pts, nrm (N,3), valid
 *   (N) are device memory.
 * slm_rigid_get_terms: out4_device = {sum w r^2 of the data rows, matched count, sum |r_c|^2 of the correspondence rows,
 *   count of surfels that contributed them} of the sums kept at the slot's beta (slot max_frames: at the point of the last
 *   slm_rigid_assemble).
 *
 * Refusals:
 *   SLM_ERR_INVALID      "<fn>: null argument"
 *                        "<fn>: bad slot"                 (slm_rigid_set_corr, _set_semantic, _get_terms: outside [0, max_frames])
 *                        "slm_rigid_set_terms: corr_mode must be 0 (none), 1 (point-point) or 2 (point-plane)"
 *                        "slm_rigid_set_terms: corr_weight must be finite"
 *                        "slm_rigid_set_terms: seg_mode must be 0 (none), 1 (hard) or 2 (soft)"
 *                        "slm_rigid_set_terms: pp_max must be finite and >= 0"
 *                        "slm_rigid_set_corr: the correspondence term is off; call slm_rigid_set_terms with corr_mode 1 or 2 first"
 *                        "slm_rigid_set_corr: corr_mode 2 (point-plane) needs nrm"
 *                        "slm_rigid_set_semantic: the semantic weight is off; call slm_rigid_set_terms with seg_mode 1 or 2 first"
 *                        "slm_rigid_corr_targets: T must be > 0"
 *                        the frame texts of slm_rigid_run, with <fn> = slm_rigid_corr_targets
 *   SLM_ERR_UNSUPPORTED  "slm_rigid_set_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)"
 *   SLM_ERR_UNBOUND      "<fn>: slot <k> has no semantic inputs; call slm_rigid_set_semantic"   (slm_rigid_run, _assemble) */
int slm_rigid_set_terms(slm_rigid* r, int32_t corr_mode, double corr_weight, int32_t seg_mode, double pp_max);
int slm_rigid_set_corr(slm_rigid* r, int32_t slot, const double* pts, const double* nrm, const uint8_t* valid);
int slm_rigid_set_semantic(slm_rigid* r, int32_t slot, int32_t num_classes, const int32_t* sf_seg,
                           const float* sf_seg_conf, const float* tgt_seg_conf);
int slm_rigid_corr_targets(const slm_frame* frame, const float* flow, double* pts, double* nrm, uint8_t* valid, void* stream);
int slm_rigid_get_terms(slm_rigid* r, int32_t slot, double* out4_device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUPER_LM_H */
