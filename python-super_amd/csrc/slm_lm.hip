// slm_lm.hip -- the LM step of the LM host: the dimensions of a batch of bound slots, the choice of the solver's form,
// the stages of an iteration in the batch's data form (enqueue_*), and the entry points made of them: slm_run, the
// sharded step with its exchange and the parity entry points (slm_assemble / slm_loss / slm_solve).  The entry points of
// the opt-in terms are slm_terms.hip.  Host side only orchestrates launches.
#include "slm_solver.h"

namespace {
struct BatchDims {
  int maxN = 0, maxJKe = 0, nt_max = 0, wb_cap = 0, n_reg_part = 0;
  int max_pos = 0, max_blocks = 0, maxP = 0;
  bool corr = false;   // some slot of the batch has correspondences bound (the term's Jacobian pass runs)
  int max_tri = 0;     // most triangles of a slot's face mesh (0: no slot has one, the face term's Jacobian pass does not run)
  bool morph = false;  // some slot of the batch has the boundary-morph term's inputs bound (its selection and Jacobian pass run)
  const CorrDev* corr_dev = nullptr;   // the batch's first descriptors of the terms (null: the term is off)
  const FaceDev* face_dev = nullptr;
  const MorphDev* morph_dev = nullptr;
  LossParts parts{};   // where the terms' loss partials sit, and what k_accept sums behind the data partials
  bool weights = false;   // the solver carries per-residual data weights (slm_enable_data_weights): the weighted kernels run
  DataWArgs wargs{};      // ... with these arguments (the batch's first semantic descriptor, seg_mode, pp_max)
  int K = 0;        // num_neighbors of the batch's slots (-1: they differ -- refused by the callers of the per-surfel kernels)
  int gram_variants = 0;   // bit0: workgroup-merged records in use, bit1: per-run slab in use
  bool nd = true;   // every slot of the batch has a nested-dissection plan (false: the block-banded solver)
  DataForm form = DataForm::none;   // the batch's data-term form; the launch arguments that follow from it:
  const int* reuse = nullptr;   // k_data_eval / k_data_gram / k_iter_begin_nd skip the slots whose records are kept
  bool fused_begin = false;     // the LM loop's zeroing rides on the Jacobian pass (k_begin_and_gram)
  int* accept_reuse = nullptr;  // k_accept keeps / clears the slots' reuse flags (the form writes records)
  int accept_eval = 0;          // k_accept: the loss pass left {r, c} in the evaluation buffer (k_data_eval)
  int max_tasks = 0;   // tasks of the persistent task-graph solver (maximum over the batch)
  // hybrid solve: every slot has the same number of levels and the same top-of-tree cut (-1: not available)
  int hybrid_cut = -2, hybrid_levels = -1, max_top_tasks = 0;
  std::vector<NDLevelSched> sched;   // per-level launch bounds over the batch
};
// band: the block-banded solver whatever the slots' plans (slm_assemble)
BatchDims dims_of(slm_solver* s, int first, int n, bool band = false) {
  BatchDims d;
  bool all_v1 = true, all_vk = true;
  for (int i = first; i < first + n; ++i) {
    const FrameDev& h = s->slots[i].h;
    d.maxN = std::max(d.maxN, h.f.N);
    d.K = (d.K == 0 || d.K == h.f.K) ? h.f.K : -1;
    d.maxJKe = std::max(d.maxJKe, h.f.J * h.f.K_ED);
    d.nt_max = std::max(d.nt_max, h.nt);
    d.wb_cap = std::max(d.wb_cap, h.wb);
    d.max_pos = std::max(d.max_pos, h.n_pos);
    d.max_blocks = std::max(d.max_blocks, h.n_blocks);
    all_v1 = all_v1 && h.v1_ready;
    all_vk = all_vk && h.vk_ready;
    if (h.v1_ready) d.gram_variants |= h.v2_ready ? 1 : 2;
    d.nd = d.nd && h.nd_ready;
    d.max_tasks = std::max(d.max_tasks, h.nd_ready ? h.n_dag_tasks : 0);
    if (h.nd_ready) {
      const int cut = h.n_dag_top_tasks > 0 ? h.dag_cut_depth : -1;
      if (d.hybrid_cut == -2) { d.hybrid_cut = cut; d.hybrid_levels = h.n_levels; }
      else if (d.hybrid_cut != cut || d.hybrid_levels != h.n_levels) d.hybrid_cut = -1;
      d.max_top_tasks = std::max(d.max_top_tasks, h.n_dag_top_tasks);
    }
    d.maxP = std::max(d.maxP, h.P);
    d.corr = d.corr || (s->corr_mode && s->slots[i].corr.has);
    d.morph = d.morph || (s->morph_on && s->slots[i].morph.has);
    if (s->face_on && s->slots[i].face.ready) d.max_tri = std::max(d.max_tri, s->slots[i].face.n_tri);
  }
  d.nd = d.nd && !band;
  // tuple-sorted on either solver; the pair records need the multifrontal one; per-entry atomics otherwise
  const slm_config& c = s->cfg;
  d.form = all_v1 ? DataForm::tuple : (d.nd && all_vk) ? DataForm::pairs : c.use_data ? DataForm::per_entry : DataForm::none;
  const bool tuple = d.form == DataForm::tuple;
  // (records of the Jacobian pass are reused after a rejected step on the multifrontal path, where the assembly re-reads
  //  them; the banded path adds into the band in place)
  if (d.nd && tuple && c.phase_test && !s->no_reuse) d.reuse = s->reuse_dev + first;
  // (round 6) the zeroing rides on the Jacobian pass's launch when every slot takes the workgroup-merged records
  d.fused_begin = d.nd && tuple && d.gram_variants == 1 && d.max_pos > 0 && s->fuse_begin;
  if (tuple && c.phase_test) d.accept_reuse = s->reuse_dev + first;
  d.accept_eval = tuple ? 1 : 0;
  if (d.nd) {
    for (int i = first; i < first + n; ++i) {
      const auto& sc = s->slots[i].cache.nd.sched;
      if (sc.size() > d.sched.size()) d.sched.resize(sc.size(), NDLevelSched{0, 0, 0, 0, 0, -2, 0, -2, 0, -2});
      for (size_t l = 0; l < sc.size(); ++l) {
        NDLevelSched& m = d.sched[l];
        // same first front and front count in every slot -> passed to the kernels by value
        if (m.first == -2) m.first = sc[l].first;
        else if (m.first != sc[l].first || m.n_fronts != sc[l].n_fronts) m.first = -1;
        m.n_fronts = std::max(m.n_fronts, sc[l].n_fronts);
        m.max_npt = std::max(m.max_npt, sc[l].max_npt);
        m.max_nt = std::max(m.max_nt, sc[l].max_nt);
        m.max_pairs = std::max(m.max_pairs, sc[l].max_pairs);
        m.max_n2p = std::max(m.max_n2p, sc[l].max_n2p);
        if (m.schur_at == -2) m.schur_at = sc[l].schur_at;
        else if (m.schur_at != sc[l].schur_at || m.n_schur != sc[l].n_schur) m.schur_at = -1;
        m.n_schur = std::max(m.n_schur, sc[l].n_schur);
        if (m.pull_at == -2) m.pull_at = sc[l].pull_at;
        else if (m.pull_at != sc[l].pull_at || m.n_pull != sc[l].n_pull) m.pull_at = -1;
        m.n_pull = std::max(m.n_pull, sc[l].n_pull);
      }
    }
  }
  if (d.nd && n > 1) {
    // slots with fewer levels than the batch maximum: their level tables must be read on the device
    for (int i = first; i < first + n; ++i)
      for (size_t l = s->slots[i].cache.nd.sched.size(); l < d.sched.size(); ++l)
        d.sched[l].first = d.sched[l].schur_at = d.sched[l].pull_at = -1;
  }
  for (auto& m : d.sched) {
    if (m.first == -2) m.first = -1;
    if (m.first < 0) m.schur_at = m.pull_at = -1;
    if (m.schur_at == -2) m.schur_at = -1;
    if (m.pull_at == -2) m.pull_at = -1;
  }
  if (s->cfg.use_arap || s->cfg.use_rot)
    d.n_reg_part = std::min(kRegBlocksMax, (d.maxJKe + 255) / 256);
  d.parts = loss_parts(s, d.n_reg_part);
  if (s->corr_mode) d.corr_dev = s->corr_dev + first;
  if (s->face_on) d.face_dev = s->face_dev + first;
  if (s->morph_on) d.morph_dev = s->morph_dev + first;
  d.weights = s->weights_on;
  d.wargs = DataWArgs{s->w_seg_mode ? s->w_dev.p + first : nullptr, s->w_pp_max, s->w_seg_mode, 0};
  return d;
}
}  // namespace

// factor + substitutions of the assembled fronts: one persistent task-graph launch (solver_path 2) or the
// per-level launches (solver_path 0)
// solver_path 0 picks by batch size: the task graph is a latency scheduler (one or two frames per launch: the
// drop-in case, one frame at a time); larger batches are throughput-bound and run the per-level launches
// Round 5 (two workgroups per CU in the task graph): "small" is frames x nodes, not frames -- the task graph wins while its
// tasks find workgroups.  C2 (2 000 nodes), ms per LM iteration, task graph / hybrid: 3 frames 1.290 / 1.481, 4 frames
// 1.549 / 1.654, 6 frames 2.124 / 2.063, 8 frames 2.754 / 2.409; C1 (512 nodes) 8 frames 0.605 / 0.755; C4 (4 000 nodes)
// 1 frame 1.396 / 1.753, 4 frames 3.510 / 3.330.
bool solve_is_task_graph(const slm_solver* s, int n, int J) {   // (slm_solver.h: the bind asks too)
  return s->cfg.solver_path == 2 || (s->cfg.solver_path == 0 && (n <= 2 || (long)n * J <= s->dag_max_nodes));
}

namespace {
static bool solve_is_hybrid(const slm_solver* s, int n, const BatchDims& d) {
  return !solve_is_task_graph(s, n, d.maxP / 7) && (s->cfg.solver_path == 4 || (s->cfg.solver_path == 0 && s->hybrid_batches)) &&
         d.hybrid_cut >= 0 && d.hybrid_levels == (int)d.sched.size() && d.hybrid_cut + 1 < d.hybrid_levels;
}
// what this batch's solve needs reset before its task-graph launch (k_iter_begin_nd's dag_cut): -1 the whole tree, >= 0 the
// fronts of depth <= the hybrid cut, -2 nothing (per-level launches only)
static int dag_cut_of(const slm_solver* s, int n, const BatchDims& d) {
  if (solve_is_task_graph(s, n, d.maxP / 7)) return -1;
  return solve_is_hybrid(s, n, d) ? d.hybrid_cut : -2;
}
// dag_reset_done: this iteration's k_iter_begin_nd already reset the task graph's flags / mailboxes (launched with
// dag_cut_of(...)); otherwise launch_front_solve_dag resets them with a launch of its own
// dag_check_later: the caller's next launch (k_after_solve) settles a timed-out task-graph launch instead of k_dag_check
// Returns the mode word of the task-graph launch (bit 0: XCD-affine ticket streams -- the caller's completion check must then
// be unconditional, launch_front_solve_dag), -1 when the solve ran no task graph.
int enqueue_front_solve(slm_solver* s, const FrameDev* fr, int n, const BatchDims& d, double u_override, hipStream_t st,
                        bool dag_reset_done = false, bool dag_check_later = false) {
  const bool dag = solve_is_task_graph(s, n, d.maxP / 7);
  // batches: the levels with many fronts as launches (throughput-bound), the top of the tree -- a chain of ~20
  // dependent tile columns with a handful of fronts -- as tasks of ONE persistent launch for all frames
  const bool hybrid = solve_is_hybrid(s, n, d);
  s->last_solver_form = dag ? 1 : (hybrid ? 2 : 0);
  int mode = -1;
  if (dag) {
    mode = launch_front_solve_dag(fr, n, d.max_tasks, u_override, st, -1, !dag_reset_done, !dag_check_later);
  } else if (hybrid) {
    const int n_levels = (int)d.sched.size(), l_cut = n_levels - 1 - d.hybrid_cut;
    launch_front_levels(fr, n, d.sched.data(), n_levels, l_cut, 0, u_override, st);
    // the task graph: the fronts above the cut, then the back substitution of the WHOLE tree (the list dag_top_tasks
    // ends with the BACKB / BACK tasks of the deeper fronts -- 24 small per-level launches, 0.25 ms at C2, otherwise)
    mode = launch_front_solve_dag(fr, n, d.max_top_tasks, u_override, st, d.hybrid_cut, !dag_reset_done, !dag_check_later);
  } else {
    launch_front_solve(fr, n, d.sched.data(), (int)d.sched.size(), u_override, st);
  }
  s->last_dag_mode = mode;
  return mode;
}

// The stages of an LM step in the batch's data form and solver form; the entry points differ only in their arguments.
// Zeroing of the normal matrix (k_iter_begin_nd / k_iter_begin): `reuse` slots keep their records, `dag_cut` what of the
// task graph's state is reset with it (dag_cut_of; -2 nothing), `fused` leaves it to the Jacobian pass.
void enqueue_zero(const FrameDev* fr, int n, const BatchDims& d, hipStream_t st, const int* reuse, int dag_cut, bool fused) {
  if (!d.nd) launch_iter_begin(fr, n, st);
  else if (!fused) launch_iter_begin_nd(fr, n, st, reuse, dag_cut);
}

// Jacobian pass of the data term.  Tuple-sorted: k_data_eval in `eval_mode` first (-1: none, the evaluation buffer already
// holds {r, c} at beta), then the Grams (with the zeroing when `fused`); the K-generic forms: records or per-entry atomics.
void enqueue_jacobian(slm_solver* s, const FrameDev* fr, int n, const BatchDims& d, hipStream_t st, int eval_mode,
                      const int* reuse, int dag_cut, bool fused) {
  const double w = s->cfg.w_data;
  switch (d.form) {
    case DataForm::tuple:
      if (eval_mode >= 0) launch_data_eval(fr, n, kLossBlocks, w, eval_mode, st, reuse);
      if (fused) launch_begin_and_gram(fr, n, w, st, reuse, dag_cut, s->gram_wgs, s->n_cus);
      else launch_data_gram(fr, n, d.max_pos, w, d.gram_variants, st, reuse, s->gram_wgs, s->n_cus);
      break;
    case DataForm::pairs:   // per-pair records (zeroed, then filled; the correspondence term adds into them)
      launch_data_grad_pairs(fr, n, d.maxN, d.K, w, st, d.weights ? &d.wargs : nullptr);
      if (d.corr) launch_corr_grad_pairs(fr, d.corr_dev, n, d.maxN, d.K, s->corr_mode, s->corr_w, st);
      if (d.max_tri) launch_face_grad(fr, d.face_dev, n, d.max_tri, s->face_w, st);
      if (d.morph) {   // (the selection at beta and its count n first: constants of the linearisation)
        launch_morph_select(fr, d.morph_dev, n, d.maxN, d.K, s->morph_w, 0, -1, nullptr, st);
        launch_morph_grad_pairs(fr, d.morph_dev, n, d.maxN, d.K, s->morph_w, st);
      }
      break;
    case DataForm::per_entry:
      launch_data_grad(fr, n, d.maxN, d.K, w, st, d.weights ? &d.wargs : nullptr);
      if (d.corr) launch_corr_grad(fr, d.corr_dev, n, d.maxN, d.K, s->corr_mode, s->corr_w, st);
      if (d.max_tri) launch_face_grad_band(fr, d.face_dev, n, d.max_tri, s->face_w, st);
      if (d.morph) {
        launch_morph_select(fr, d.morph_dev, n, d.maxN, d.K, s->morph_w, 0, -1, nullptr, st);
        launch_morph_grad(fr, d.morph_dev, n, d.maxN, d.K, s->morph_w, st);
      }
      break;
    case DataForm::none: break;
  }
}

// Scatter of the data term's records into the solver's storage, then the regularisers.  A sharded step splits it around
// the exchange of the pair records: before_exchange reduces the tuple-sorted Grams to pair records (the pair form wrote
// them already), after_exchange scatters the exchanged records and adds the regularisers.
enum class Shard { whole, before_exchange, after_exchange };
void enqueue_scatter(slm_solver* s, const FrameDev* fr, int n, const BatchDims& d, hipStream_t st, Shard part) {
  const slm_config& c = s->cfg;
  const bool tuple = d.form == DataForm::tuple;
  if (part == Shard::before_exchange) {
    if (tuple) launch_pair_reduce(fr, n, d.max_blocks, st);
    return;
  }
  if (part == Shard::after_exchange || d.form == DataForm::pairs) launch_pair_scatter(fr, n, d.max_blocks, st);
  else if (tuple && d.nd) launch_front_assemble(fr, n, d.max_blocks, st);
  else if (tuple) launch_band_assemble(fr, n, d.max_blocks, st);
  if (d.nd) {
    launch_reg_grad_nd(fr, n, d.maxP / 7, c.use_arap, c.w_arap, c.use_rot, c.w_rot, st);
    if (!c.use_arap && !c.use_rot) launch_front_load_rhs(fr, n, d.maxP, st);   // (else k_reg_grad_nd did it)
  } else {
    launch_reg_grad(fr, n, d.maxJKe, c.use_arap, c.w_arap, c.use_rot, c.w_rot, st);
  }
}

// Data loss at the trial point beta + delta (tuple-sorted: k_data_eval's loss pass, whose {r, c} feed the next Jacobian
// pass) or, `at_beta` (slm_loss), k_data_loss at beta for every form.
void enqueue_data_loss(slm_solver* s, const FrameDev* fr, int n, const BatchDims& d, hipStream_t st, bool at_beta) {
  if (d.form == DataForm::tuple && !at_beta) launch_data_eval(fr, n, kLossBlocks, s->cfg.w_data, 0, st);
  else if (d.form != DataForm::none)
    launch_data_loss(fr, n, kLossBlocks, d.K, s->cfg.w_data, at_beta ? 0 : 1, st, d.weights ? &d.wargs : nullptr);
  // the correspondence term's partials, behind the regularisers' (every slot of an enabled solver: zeros without targets)
  if (s->corr_mode && d.K >= 1)
    launch_corr_loss(fr, d.corr_dev, n, d.K, s->corr_mode, s->corr_w, at_beta ? 0 : 1, d.parts.corr, d.parts.corr_cnt, st);
  // the face term's, behind those (likewise: zeros without a mesh)
  if (s->face_on) launch_face_loss(fr, d.face_dev, n, s->face_w, at_beta ? 0 : 1, d.parts.face, st);
  // the boundary-morph term's, behind those: a fresh selection there, then the fold (alone when no slot has inputs: zeros)
  if (s->morph_on && d.K >= 1)
    launch_morph_select(fr, d.morph_dev, n, d.morph ? d.maxN : 0, d.K, s->morph_w, at_beta ? 0 : 1, d.parts.morph, nullptr, st);
}
}  // namespace

// With a semantic weight on, every slot of [first, first + n) needs its semantic inputs: no silent unweighted run.
int weights_check(const slm_solver* s, const char* fn, int first, int n) {
  if (!s->w_seg_mode) return SLM_OK;
  for (int i = first; i < first + n; ++i)
    if (!s->slots[i].wdev.has)
      return fail(SLM_ERR_UNBOUND, std::string(fn) + ": slot " + std::to_string(i) +
                                       " has no semantic inputs; call slm_bind_data_semantic after slm_bind_frame");
  return SLM_OK;
}

int clear_flags(slm_solver* s, int slot, hipStream_t st) {
  // stopped / counters live at the tail of LMState: zero {iter..pad}
  LMState* p = s->slots[slot].h.st;
  HIPCHK(hipMemsetAsync(&p->stopped, 0, sizeof(int32_t) * 4, st));
  return SLM_OK;
}

extern "C" {

static hipEvent_t take_event(slm_solver* s) {
  if (!s->ev_pool.empty()) {
    hipEvent_t e = s->ev_pool.back();
    s->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// ---- one frame sharded over several GPUs ----------------------------------------------------
int slm_set_shard(slm_solver* s, int32_t rank, int32_t world) {
  if (!s || world < 1 || rank < 0 || rank >= world) return fail(SLM_ERR_INVALID, "slm_set_shard: bad rank/world");
  if (s->cfg.data_path != 0 || s->cfg.solver_path == 1)
    return fail(SLM_ERR_UNSUPPORTED, "slm_set_shard: needs data_path 0 and a nested-dissection solver_path (0, 2, 3 or 4)");
  if (s->corr_mode)
    return fail(SLM_ERR_UNSUPPORTED, "slm_set_shard: the correspondence term is enabled (slm_enable_corr); it needs every surfel of "
                                     "the frame on one device");
  if (s->face_on)
    return fail(SLM_ERR_UNSUPPORTED, "slm_set_shard: the face term is enabled (slm_enable_face); its mesh is not sharded");
  if (s->morph_on)
    return fail(SLM_ERR_UNSUPPORTED, "slm_set_shard: the boundary-morph term is enabled (slm_enable_morph); it needs every surfel of "
                                     "the frame on one device");
  s->rank = rank;
  s->world = world;
  s->shard_mode = true;
  for (size_t i = 0; i < s->slots.size(); ++i) {   // the shares are fixed at bind time
    join_prepare(s, (int)i);
    s->slots[i].model_ready = false;
    s->slots[i].h.bound = 0;
  }
  HIPCHK(hipMemset(s->frames_dev, 0, sizeof(FrameDev) * s->slots.size()));
  return SLM_OK;
}

static int shard_dims(slm_solver* s, int n_frames, BatchDims& d, const char* fn = nullptr) {
  int rc = check_slots(s, 0, n_frames);
  if (rc) return rc;
  if (fn && (rc = weights_check(s, fn, 0, n_frames)) != SLM_OK) return rc;
  d = dims_of(s, 0, n_frames);
  if (!d.nd || (d.form != DataForm::tuple && d.form != DataForm::pairs))
    return fail(SLM_ERR_UNSUPPORTED, "sharded LM step: every slot needs a multifrontal data path (tuple-sorted or K-generic) and the ND solver");
  return SLM_OK;
}

int slm_lm_grad_local(slm_solver* s, int32_t n_frames, void* stream) {
  BatchDims d;
  int rc = shard_dims(s, n_frames, d, "slm_lm_grad_local");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const FrameDev* fr = s->frames_dev;
  enqueue_zero(fr, n_frames, d, st, d.reuse, -2, false);
  enqueue_jacobian(s, fr, n_frames, d, st, 1, d.reuse, -2, false);   // (k_data_eval: only slots whose buffer is not the current beta's)
  enqueue_scatter(s, fr, n_frames, d, st, Shard::before_exchange);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_lm_solve(slm_solver* s, int32_t n_frames, void* stream) {
  BatchDims d;
  int rc = shard_dims(s, n_frames, d);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const FrameDev* fr = s->frames_dev;
  enqueue_scatter(s, fr, n_frames, d, st, Shard::after_exchange);
  enqueue_front_solve(s, fr, n_frames, d, -1.0, st);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_lm_loss_local(slm_solver* s, int32_t n_frames, void* stream) {
  BatchDims d;
  int rc = shard_dims(s, n_frames, d, "slm_lm_loss_local");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const FrameDev* fr = s->frames_dev;
  const slm_config& c = s->cfg;
  launch_make_trial(fr, n_frames, d.maxJKe, st);
  enqueue_data_loss(s, fr, n_frames, d, st, false);
  if (d.n_reg_part > 0)
    launch_reg_loss(fr, n_frames, d.n_reg_part, c.use_arap, c.w_arap, c.use_rot, c.w_rot, 1, st);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_lm_accept(slm_solver* s, int32_t n_frames, void* stream) {
  BatchDims d;
  int rc = shard_dims(s, n_frames, d);
  if (rc) return rc;
  // k_accept sums d.n_reg_part partial pairs behind the data partials here, where slm_run sums d.parts.n_acc_part.  The two
  // are equal only while no opt-in term puts partials behind the regularisers': the correspondence, face and morph terms
  // all refuse a sharded solver (slm_set_shard, slm_enable_*).  A term that learns to shard must change this argument.
  launch_accept(s->frames_dev, n_frames, s->cfg.phase_test, d.n_reg_part, std::max(s->cfg.num_iterations, 1), (hipStream_t)stream,
                d.accept_reuse, d.accept_eval);   // (slm_lm_loss_local ran k_data_eval)
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

static int exchange_buf(slm_solver* s, int slot, int what, double** p, int64_t* n) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  const FrameDev& h = s->slots[slot].h;
  switch (what) {
    case SLM_X_PAIR_BLOCKS:
      if (!h.pairbuf) return fail(SLM_ERR_UNBOUND, "slm_lm_exchange: the slot was bound without slm_set_shard");
      *p = h.pairbuf;
      *n = (int64_t)h.n_blocks * SLM_WREC + (h.vk_ready ? SLM_VK_TAIL : 1);   // records + matched count (spread on the K-generic path)
      return SLM_OK;
    case SLM_X_DELTA:
      *p = h.delta;
      *n = h.P;
      return SLM_OK;
    case SLM_X_DATA_LOSS:
      *p = h.loss_part;
      *n = 2 * (int64_t)h.n_loss_part;
      return SLM_OK;
  }
  return fail(SLM_ERR_INVALID, "slm_lm_exchange: unknown buffer");
}

int slm_lm_exchange_size(slm_solver* s, int32_t slot, int32_t what, int64_t* n_doubles) {
  double* p;
  if (!n_doubles) return fail(SLM_ERR_INVALID, "slm_lm_exchange_size: null output");
  return exchange_buf(s, slot, what, &p, n_doubles);
}

int slm_lm_exchange_ptr(slm_solver* s, int32_t slot, int32_t what, double** ptr_out, int64_t* n_doubles) {
  if (!ptr_out || !n_doubles) return fail(SLM_ERR_INVALID, "slm_lm_exchange_ptr: null output");
  return exchange_buf(s, slot, what, ptr_out, n_doubles);
}

int slm_lm_exchange_get(slm_solver* s, int32_t slot, int32_t what, double* out, void* stream) {
  double* p;
  int64_t n;
  int rc = exchange_buf(s, slot, what, &p, &n);
  if (rc) return rc;
  if (!out) return fail(SLM_ERR_INVALID, "slm_lm_exchange_get: null output");
  HIPCHK(hipMemcpyAsync(out, p, sizeof(double) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SLM_OK;
}

int slm_lm_exchange_set(slm_solver* s, int32_t slot, int32_t what, const double* in, void* stream) {
  double* p;
  int64_t n;
  int rc = exchange_buf(s, slot, what, &p, &n);
  if (rc) return rc;
  if (!in) return fail(SLM_ERR_INVALID, "slm_lm_exchange_set: null input");
  HIPCHK(hipMemcpyAsync(p, in, sizeof(double) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SLM_OK;
}

// One LM iteration of slots [first, first + n) on `st`.
static void enqueue_lm_iteration(slm_solver* s, int first, int n, const BatchDims& d, hipStream_t st, bool first_iteration) {
  const FrameDev* fr = s->frames_dev + first;
  const slm_config& c = s->cfg;
  std::vector<hipEvent_t>* evs = nullptr;
  if (s->profile) {
    s->ev_runs.emplace_back();
    evs = &s->ev_runs.back();
  }
  auto mark = [&]() {
    if (!evs) return;
    hipEvent_t e = take_event(s);
    if (e) (void)hipEventRecord(e, st);
    evs->push_back(e);
  };
  mark();
  const int dag_cut = d.nd ? dag_cut_of(s, n, d) : -2;
  enqueue_zero(fr, n, d, st, d.reuse, dag_cut, d.fused_begin);
  mark();
  // The Jacobian pass reads {r, c} of every position from the evaluation buffer.  Inside the loop the buffer is what the
  // loss pass of the previous iteration left at the accepted trial point (a rejected step reuses the records and runs no
  // Jacobian pass at all); a pass of its own is only needed at the first iteration of a run (skipped on the device for
  // slots whose buffer is valid) and after a reject when records are not reused.
  const int eval_mode = (first_iteration || (c.phase_test && !d.reuse)) ? 1 : -1;
  enqueue_jacobian(s, fr, n, d, st, eval_mode, d.reuse, dag_cut, d.fused_begin);
  mark();
  enqueue_scatter(s, fr, n, d, st, Shard::whole);
  mark();
  // the trial point beta + delta (node_pk_try), the regularisers' loss there and the task graph's abort check: one launch
  const bool tail = c.use_data || d.n_reg_part > 0;
  int dag_mode = -1;
  if (d.nd) dag_mode = enqueue_front_solve(s, fr, n, d, -1.0, st, true, tail);
  else launch_band_solve(fr, n, d.nt_max, d.wb_cap, -1.0, st);
  if (tail)   // (dag_check 2 behind an XCD-affine task-graph launch: the completion check runs whether or not the abort flag is up)
    launch_after_solve(fr, n, c.use_data ? d.maxP / 7 : 0, d.n_reg_part, c.use_arap, c.w_arap, c.use_rot, c.w_rot,
                       dag_cut >= -1 ? ((dag_mode > 0 && (dag_mode & 1)) ? 2 : 1) : 0, st);
  mark();
  enqueue_data_loss(s, fr, n, d, st, false);
  mark();
  launch_accept(fr, n, c.phase_test, d.parts.n_acc_part, std::max(c.num_iterations, 1), st, d.accept_reuse, d.accept_eval);
  mark();
}

int slm_run(slm_solver* s, int32_t n_frames, void* stream) {
  int rc = check_slots(s, 0, n_frames);
  if (rc) return rc;
  if (s->world > 1)
    return fail(SLM_ERR_UNSUPPORTED,
                "slm_run: the frame is sharded; drive slm_lm_grad_local / slm_lm_solve / slm_lm_loss_local / "
                "slm_lm_accept with the exchanges between them");
  if ((rc = weights_check(s, "slm_run", 0, n_frames)) != SLM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const slm_config& c = s->cfg;
  BatchDims d = dims_of(s, 0, n_frames);
  if (!d.nd) {
    // A batch runs ONE solver form.  When some slot has no nested-dissection plan (a frame without surfels, a graph
    // the analysis refuses) all of them take the block-banded path -- whose storage the slots WITH a plan have not
    // been given at bind time: provide it now (a read-back per such slot; the rare path).
    std::lock_guard<std::mutex> lock(s->band_mutex);
    for (int i = 0; i < n_frames; ++i) {
      rc = ensure_band(s, i, st);
      if (rc) return rc;
    }
    d = dims_of(s, 0, n_frames);
  }
  for (int it = 0; it < c.num_iterations; ++it) enqueue_lm_iteration(s, 0, n_frames, d, st, it == 0);
  // The reuse flag of a slot says "the Gram records in HBM were computed at the slot's CURRENT beta".  k_accept keeps it
  // on every path that writes records (banded path included: a later multifrontal run may then reuse them); a run that
  // wrote none (per-entry atomics) leaves nothing to reuse.
  if (!d.accept_reuse) HIPCHK(hipMemsetAsync(s->reuse_dev, 0, sizeof(int) * n_frames, st));
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_assemble(slm_solver* s, int32_t slot, double* jtj_dense, double* jtl, void* stream) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  if ((rc = weights_check(s, "slm_assemble", slot, 1)) != SLM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = clear_flags(s, slot, st);
  if (rc) return rc;
  rc = ensure_band(s, slot, st);
  if (rc) return rc;
  const BatchDims d = dims_of(s, slot, 1, true);
  const FrameDev* fr = s->frames_dev + slot;
  const FrameDev& h = s->slots[slot].h;
  enqueue_zero(fr, 1, d, st, nullptr, -2, false);
  enqueue_jacobian(s, fr, 1, d, st, 2, nullptr, -2, false);   // (k_data_eval mode 2 clobbers the loss partials)
  enqueue_scatter(s, fr, 1, d, st, Shard::whole);
  if (jtj_dense) launch_band_to_dense(s->frames_dev, slot, jtj_dense, st);
  if (jtl)
    HIPCHK(hipMemcpyAsync(jtl, h.rhs, sizeof(double) * h.P, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_loss(slm_solver* s, int32_t slot, double* out, void* stream) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  if (!out) return fail(SLM_ERR_INVALID, "slm_loss: null output");
  if ((rc = weights_check(s, "slm_loss", slot, 1)) != SLM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = clear_flags(s, slot, st);
  if (rc) return rc;
  const BatchDims d = dims_of(s, slot, 1);
  const FrameDev* fr = s->frames_dev + slot;
  const slm_config& c = s->cfg;
  enqueue_data_loss(s, fr, 1, d, st, true);
  if (d.n_reg_part > 0) launch_reg_loss(fr, 1, d.n_reg_part, c.use_arap, c.w_arap, c.use_rot, c.w_rot, 0, st);
  launch_loss_out(s->frames_dev, slot, d.n_reg_part, out, st);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_solve(slm_solver* s, int32_t slot, double u, double* delta, int32_t* status, void* stream) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  if (!delta || !(u >= 0.0)) return fail(SLM_ERR_INVALID, "slm_solve: bad argument");
  if ((rc = weights_check(s, "slm_solve", slot, 1)) != SLM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = clear_flags(s, slot, st);
  if (rc) return rc;
  const BatchDims d = dims_of(s, slot, 1);
  const FrameDev* fr = s->frames_dev + slot;
  const FrameDev& h = s->slots[slot].h;
  enqueue_zero(fr, 1, d, st, nullptr, -2, false);
  enqueue_jacobian(s, fr, 1, d, st, 2, nullptr, -2, false);
  enqueue_scatter(s, fr, 1, d, st, Shard::whole);
  if (d.nd) enqueue_front_solve(s, fr, 1, d, u, st);
  else launch_band_solve(fr, 1, d.nt_max, d.wb_cap, u, st);
  HIPCHK(hipMemcpyAsync(delta, h.delta, sizeof(double) * h.P, hipMemcpyDeviceToDevice, st));
  if (status)
    HIPCHK(hipMemcpyAsync(status, &h.st->chol_fail, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

}  // extern "C"
