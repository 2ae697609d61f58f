// slm_bind.hip -- the bind of the LM host: a frame into a slot.  The model-side half (data-term plan, symbolic plan of
// the solver, the slot's work buffers) and the target-side half, alone (slm_bind_frame), ahead of the target
// (slm_prepare_model) or a batch at a time on the bind workers (slm_bind_frames).  Host side only orchestrates launches.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>

#include "slm_solver.h"

// what the reference could never have been given (its KNN ids come from a top-k: distinct and inside [0, J))
static const char* const kBadKnn =
    "slm_bind_frame: a KNN index (sf_knn_idx or ed_knn_idx) lies outside [0, J) or a surfel's row of sf_knn_idx repeats an id";
static const char* const kBadFace =
    "slm_bind_frame: a triangle of the slot's face mesh (slm_set_face_mesh) has a node id outside [0, J) or repeats an id";

// a frame's form, decided at bind (a plan that comes out empty leaves the slot per_entry: bind_model_part)
// corr: the solver carries the correspondence term (slm_enable_corr), which adds into the pair records, or the per-residual
// weights (slm_enable_data_weights), whose kernels are the pair form's: pairs for every K
static DataForm data_form_of(const slm_config& c, const slm_frame& f, bool corr) {
  if (!c.use_data || f.N <= 0) return DataForm::none;
  if (c.data_path == 1 || f.J >= 65536) return DataForm::per_entry;
  if (f.K == SLM_K && !corr) return DataForm::tuple;
  return c.solver_path != 1 ? DataForm::pairs : DataForm::per_entry;
}

// Block-banded path on demand: tile half-bandwidth of the normal matrix from the KNN tables (one
// 8-byte read-back, with the tables' check), band + diagonal-inverse storage, refreshed device copy of the slot.
int ensure_band(slm_solver* s, int slot, hipStream_t st) {
  Slot& sl = s->slots[slot];
  if (sl.band_ready) return SLM_OK;
  FrameDev& h = sl.h;
  launch_bandwidth(h.f, s->bw_dev, st);
  if (s->face_on && sl.face.ready) launch_face_bandwidth(sl.face.tri, sl.face.n_tri, s->bw_dev, st);   // (ids checked by the bind)
  HIPCHK(hipMemcpyAsync(s->bw_host.data(), s->bw_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (s->bw_host[1]) return fail(SLM_ERR_INVALID, kBadKnn);
  int wb = s->bw_host[0];
  if (wb > h.nt - 1) wb = h.nt - 1;
  h.wb = wb;
  HIPCHK(grow(sl.band, (size_t)h.nt * (wb + 1) * SLM_NB * SLM_NB));
  HIPCHK(grow(sl.linv, (size_t)h.nt * SLM_NB * SLM_NB));
  h.band = sl.band.p;
  h.linv = sl.linv.p;
  HIPCHK(hipMemcpyAsync(s->frames_dev + slot, &h, sizeof(FrameDev), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  sl.band_ready = true;
  return SLM_OK;
}

// Diagnostics (SLM_BIND_TRACE=<ms>): a bind that takes longer than <ms> on the host prints the time stamps of its
// stages -- which stage of which worker carried a rare multi-millisecond stall (tools/studies/stall_hunt.py).
namespace {
struct BindTrace {
  double t[8];
  int n;
};
thread_local BindTrace g_bt;
inline double bt_now() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline double bind_trace_threshold() {
  static const double th = [] {
    const char* e = getenv("SLM_BIND_TRACE");
    return e ? atof(e) : -1.0;
  }();
  return th;
}
// the stamps of one bind, in order (a stage that does not run leaves none): entry | data-term plan done, its size
// read-backs included | pair list / node table on the host (read back only when the graph changed) | symbolic plan
// settled | descriptor on its way | end
enum BindStamp { BT_ENTRY, BT_DATA_PLAN, BT_READBACK, BT_SYMBOLIC, BT_DESCRIPTOR, BT_END };
inline void bt_mark(BindStamp stage) {
  if (stage == BT_ENTRY) g_bt.n = 0;
  if (bind_trace_threshold() >= 0.0 && g_bt.n < 8) g_bt.t[g_bt.n++] = bt_now();
}
}  // namespace

static int check_model_args(const slm_solver* s, int32_t slot, const slm_frame* f) {
  if (slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, "slm_bind_frame: bad slot");
  // num_neighbors (reference options.py:49, README.md:175; super/loss.py:213-220 and super/utils.py:30-36 are K-generic):
  // 4 takes the tuple-sorted MFMA path; any other value in 1..8 the K-generic pair path on the multifrontal solver, or
  // the per-entry atomics on the block-banded one (data_form_of)
  if (f->K < 1 || f->K > 8) return fail(SLM_ERR_UNSUPPORTED, "slm_bind_frame: num_neighbors must be in 1..8");
  if (f->K_ED < 1 || f->K_ED > SLM_MAX_KED)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_frame: num_ED_neighbors must be in 1..8");
  if (f->N < 0 || f->J < 1) return fail(SLM_ERR_INVALID, "slm_bind_frame: bad sizes");
  if (s->corr_mode && f->J >= 65536)   // (the pair keys are a * J + b in 32 bits: such a frame takes the per-entry form)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_frame: the correspondence term (slm_enable_corr) needs J < 65536");
  if (s->weights_on && f->J >= 65536)   // (the same: the weighted kernels are those of the pair form)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_frame: the data weights (slm_enable_data_weights) need J < 65536");
  if (s->face_on && f->J >= 65536)   // (the same: the term adds into the pair records)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_frame: the face term (slm_enable_face) needs J < 65536");
  if (s->morph_on && f->J >= 65536)   // (the same)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_frame: the boundary-morph term (slm_enable_morph) needs J < 65536");
  if (f->N > 0 && f->J < f->K)   // (the reference's top-k of K among J nodes raises; the device checks below assume J >= K)
    return fail(SLM_ERR_INVALID, "slm_bind_frame: fewer nodes (J) than num_neighbors: sf_knn_idx cannot hold K distinct ids");
  if ((f->N > 0 && (!f->sf_points || !f->sf_knn_idx || !f->sf_knn_w)) || !f->ed_points || !f->ed_knn_idx)
    return fail(SLM_ERR_INVALID, "slm_bind_frame: null device pointer");
  return SLM_OK;
}

// The descriptor back to "nothing bound" for frame f, and the slot's grow-only work buffers at f's sizes.
static int reset_slot(slm_solver* s, Slot& sl, const slm_frame* f, hipStream_t st) {
  FrameDev& h = sl.h;
  const int P = 7 * f->J;
  const int nt = (P + SLM_NB - 1) / SLM_NB;
  sl.band_ready = false;
  h.dag_trace = nullptr;   // a trace buffer is sized for the plan it was enabled on
  h.bound = 0;             // a bind that fails half way leaves the slot unbound (slm_run refuses it)
  h.f = *f;
  h.P = P;
  h.nt = nt;
  // the tile half-bandwidth and the band storage are only needed by the block-banded path
  // (solver_path 1, a frame without an ND plan, slm_assemble): ensure_band() fills them in on demand
  h.wb = 0;
  h.band = sl.band.p;
  h.linv = sl.linv.p;
  h.n_loss_part = s->cfg.use_data ? kLossBlocks : 0;
  HIPCHK(grow(sl.beta, (size_t)P));
  HIPCHK(grow(sl.node_pk, (size_t)2 * SLM_NPK * f->J));
  HIPCHK(grow(sl.delta, (size_t)nt * SLM_NB));
  HIPCHK(grow(sl.rhs, (size_t)nt * SLM_NB));
  h.beta = sl.beta.p;
  h.node_pk = sl.node_pk.p;
  h.node_pk_try = sl.node_pk.p + (size_t)SLM_NPK * f->J;
  h.delta = sl.delta.p;
  h.rhs = sl.rhs.p;
  // the buffers of one size for good: allocated by the slot's first bind (st, dbg and rec exactly, outside the counters)
  if (!sl.loss_part) {
    const size_t n_part = loss_parts(s, 0).doubles;
    HIPCHK(grow(sl.loss_part, n_part));
    HIPCHK(hipMemsetAsync(sl.loss_part, 0, sizeof(double) * n_part, st));
  }
  HIPCHK(sl.st.grow(1, 1));
#ifdef SLM_STAMPS
  if (!sl.dbg) {
    HIPCHK(sl.dbg.grow(64, 64));
    HIPCHK(hipMemset(sl.dbg, 0, sizeof(unsigned long long) * 64));
  }
#endif
  const size_t n_rec = s->cfg.num_iterations > 0 ? s->cfg.num_iterations : 1;
  HIPCHK(sl.rec.grow(n_rec, n_rec));
  h.loss_part = sl.loss_part.p;
  h.st = sl.st.p;
  h.dbg = sl.dbg.p;
  h.rec = sl.rec.p;
  return SLM_OK;
}

// The data-term plan of the frame's form (DataLoss.prepare analogue).  form: the form that actually holds -- an empty
// plan leaves the slot per_entry, as dims_of counts it; the two hashes of the coupling graph come from the device with
// the plan's sizes.
struct DataPlan {
  DataForm form = DataForm::none;
  uint64_t knn_hash = 0, graph_hash = 0;
};
static int bind_data_plan(slm_solver* s, Slot& sl, const slm_frame* f, hipStream_t st, PrepBuffers* prep, DataPlan& out) {
  FrameDev& h = sl.h;
  h.v1_ready = 0;
  h.vk_ready = 0;
  sl.prep_kind = 0;
  sl.prep_max_bin = 0;
  sl.face.ready = 0;
  sl.face.tri_pidx = nullptr;
  out.form = data_form_of(s->cfg, *f, s->corr_mode != 0 || s->weights_on || s->face_on || s->morph_on);
  if (out.form == DataForm::tuple) {
    V1Sizes sz;
    HIPCHK(prep_v1(prep, *f, sl.plan, &sz, st));
    if (sz.bad_knn) return fail(SLM_ERR_INVALID, kBadKnn);
    out.knn_hash = sz.knn_hash;
    out.graph_hash = sz.graph_hash;
    bt_mark(BT_DATA_PLAN);
    if (sz.n_tuples > 0) {
      h.n_tuples = sz.n_tuples;
      h.n_pos = sz.n_pos;
      h.n_runs = sz.n_runs;
      h.n_blocks = sz.n_blocks;
      h.s_pts = sl.plan.s_pts;
      h.s_idx = sl.plan.s_idx;
      h.s_w = sl.plan.s_w;
      h.grp_run = sl.plan.grp_run;
      h.run_nodes = sl.plan.run_nodes;
      h.slab = sl.plan.slab;
      h.blk_key = sl.plan.blk_key;
      h.blk_start = sl.plan.blk_start;
      h.blk_entry = sl.plan.blk_entry;
      HIPCHK(grow(sl.ev_rc, (size_t)4 * sz.n_pos));   // evaluation buffer {r, c} per position
      h.ev_rc = sl.ev_rc.p;
      h.v1_ready = 1;
      sl.prep_kind = sz.prep_kind;
      sl.prep_max_bin = sz.max_bin;
      // workgroup-merged records (default); data_path 2 keeps the per-run slab
      h.v2_ready = 0;
      if (s->cfg.data_path == 0 && sz.n_wblk > 0 && sz.max_wblk_per_wg <= SLM_LB_MAX) {
        h.n_wblk = sz.n_wblk;
        h.wg_first = sl.plan.wg_first;
        h.wg_last = sl.plan.wg_last;
        h.run_lidx = sl.plan.run_lidx;
        h.wgslab = sl.plan.wgslab;
        h.blk2_start = sl.plan.blk2_start;
        h.blk2_entry = sl.plan.blk2_entry;
        h.v2_ready = 1;
      }
    }
  } else if (out.form == DataForm::pairs) {
    // the coupled-pair list and every surfel's pair indices from one sort (prep_pairs), the multifrontal solver on that
    // list, the data term through per-pair records (pairbuf)
    PairSizes sz;
    // (the face term's mesh joins the pair list: its six pairs per triangle get records, destinations and a place in the fronts)
    const FaceMesh mesh = s->face_on ? FaceMesh{sl.face.tri, sl.face.n_tri} : FaceMesh();
    HIPCHK(prep_pairs(prep, *f, sl.pplan, &sz, st, mesh));
    if (sz.bad_knn) return fail(SLM_ERR_INVALID, kBadKnn);
    if (sz.bad_face) return fail(SLM_ERR_INVALID, kBadFace);
    out.knn_hash = sz.knn_hash;
    out.graph_hash = sz.graph_hash;
    bt_mark(BT_DATA_PLAN);
    if (sz.n_blocks > 0) {
      h.n_blocks = sz.n_blocks;
      h.blk_key = sl.pplan.blk_key;
      h.sf_pidx = sl.pplan.sf_pidx;
      h.sf_perm = sl.pplan.sf_perm;
      h.vk_ready = 1;
      if (mesh.n_tri > 0) {
        sl.face.tri_pidx = sl.pplan.tri_pidx;
        sl.face.ready = 1;
      }
    }
  } else if (out.form == DataForm::per_entry) {
    // the per-entry atomics dereference the tables too: same refusal
    // (use_data 0: ensure_band's pass over the tables checks them)
    bool bad = false;
    HIPCHK(prep_check_knn(prep, *f, &bad, st));
    if (bad) return fail(SLM_ERR_INVALID, kBadKnn);
  }
  if ((out.form == DataForm::tuple && !h.v1_ready) || (out.form == DataForm::pairs && !h.vk_ready)) out.form = DataForm::per_entry;
  return SLM_OK;
}

// Share of this rank when the frame is sharded over several GPUs (whole frame otherwise), and the pair-record buffer.
static int bind_shard_share(slm_solver* s, Slot& sl, const slm_frame* f, DataForm form, hipStream_t st) {
  FrameDev& h = sl.h;
  const int n_wg = (form == DataForm::tuple ? h.n_pos + 255 : 0) / 256;
  h.wg_lo = (int32_t)((int64_t)n_wg * s->rank / s->world);
  h.wg_hi = (int32_t)((int64_t)n_wg * (s->rank + 1) / s->world);
  h.sf_lo = (int32_t)((int64_t)f->N * s->rank / s->world);
  h.sf_hi = (int32_t)((int64_t)f->N * (s->rank + 1) / s->world);
  h.pairbuf = nullptr;
  if (s->shard_mode && form != DataForm::tuple && form != DataForm::pairs)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_frame: sharded frames need the multifrontal data paths "
                                     "(data_path 0 or 2, J < 65536)");
  if (s->shard_mode || form == DataForm::pairs) {   // (the K-generic pair path always assembles through the pair records)
    HIPCHK(grow(sl.pairbuf, (size_t)h.n_blocks * SLM_WREC + SLM_VK_TAIL + 2));
    h.pairbuf = sl.pairbuf.p;
  }
  if (s->shard_mode) {
    // records (or per-run Grams) of the other ranks' workgroups stay zero for the whole frame
    if (h.v2_ready) HIPCHK(hipMemsetAsync(h.wgslab, 0, sizeof(double) * SLM_WREC * (size_t)h.n_wblk, st));
    else if (form == DataForm::tuple) HIPCHK(hipMemsetAsync(h.slab, 0, sizeof(double) * SLM_SLAB_STRIDE * (size_t)h.n_runs, st));
  }
  return SLM_OK;
}

// What the host analysis reads: the frame's pair list, the node KNN table and the node positions (pinned read-backs).
static int read_back_graph(Slot& sl, const slm_frame* f, hipStream_t st) {
  const FrameDev& h = sl.h;
  HIPCHK(sl.h_pairs.resize(h.n_blocks));
  HIPCHK(sl.h_knn.resize((size_t)f->J * f->K_ED));
  HIPCHK(sl.h_pts.resize((size_t)f->J * 3));
  HIPCHK(hipMemcpyAsync(sl.h_pairs.data(), h.blk_key, sizeof(uint32_t) * h.n_blocks, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(sl.h_knn.data(), f->ed_knn_idx, sizeof(int32_t) * sl.h_knn.size(), hipMemcpyDeviceToHost, st));
  if (f->state_f64) {
    HIPCHK(sl.h_pts64.resize(sl.h_pts.size()));
    HIPCHK(hipMemcpyAsync(sl.h_pts64.data(), f->ed_points, sizeof(double) * sl.h_pts64.size(), hipMemcpyDeviceToHost, st));
  } else {
    HIPCHK(hipMemcpyAsync(sl.h_pts.data(), f->ed_points, sizeof(float) * sl.h_pts.size(), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  // the node positions only steer the geometric bisection of the symbolic plan: float32 is plenty
  if (f->state_f64)
    for (size_t i = 0; i < sl.h_pts.size(); ++i) sl.h_pts[i] = (float)sl.h_pts64[i];
  return SLM_OK;
}

// The int32 arrays of a plan share ONE device buffer (Slot::d_ints), in this order: its size and the copies both come
// from this table.
struct PlanInts {
  GP<const int32_t> FrameDev::*field;
  std::vector<int32_t> NDPlanHost::*src;
};
static const PlanInts kPlanInts[] = {
    {&FrameDev::level_start, &NDPlanHost::level_start}, {&FrameDev::nd_nodes, &NDPlanHost::nodes},
    {&FrameDev::nd_eamap, &NDPlanHost::eamap},          {&FrameDev::node_front, &NDPlanHost::node_front},
    {&FrameDev::node_pos, &NDPlanHost::node_pos},       {&FrameDev::in_start, &NDPlanHost::in_start},
    {&FrameDev::in_edge, &NDPlanHost::in_edge},         {&FrameDev::item_off, &NDPlanHost::item_off},
    {&FrameDev::dag_tasks, &NDPlanHost::dag_tasks},     {&FrameDev::dag_top_tasks, &NDPlanHost::dag_top_tasks},
    {&FrameDev::front_kids, &NDPlanHost::front_kids},   {&FrameDev::pull_off, &NDPlanHost::pull_off},
    {&FrameDev::pullmap, &NDPlanHost::pullmap},         {&FrameDev::prng_off, &NDPlanHost::prng_off},
    {&FrameDev::prng, &NDPlanHost::prng},
};

// A new plan to the device: front descriptors, work items, the int32 arrays, the destinations of the plan's pairs and
// of the ARAP pairs; the slot's factor storage at the plan's sizes.
static int upload_plan(Slot& sl, hipStream_t st) {
  const NDPlanHost& nd = sl.cache.nd;
  FrameDev& h = sl.h;
  size_t n_ints = 0;
  for (const PlanInts& a : kPlanInts) n_ints += (nd.*a.src).size();
  HIPCHK(grow(sl.d_fronts, nd.fronts.size()));
  HIPCHK(grow(sl.d_ints, n_ints));
  HIPCHK(grow(sl.d_dests, nd.block_dest.size() + nd.pair_dest.size()));
  HIPCHK(grow(sl.ftiles, (size_t)nd.tile_doubles));
  HIPCHK(grow(sl.fvec, (size_t)nd.vec_doubles));
  HIPCHK(grow(sl.flinv, (size_t)nd.linv_doubles + 1));
  HIPCHK(grow(sl.fmail, (size_t)(nd.linv_doubles / (SLM_NB * SLM_NB)) * 2560 + 1));   // SLM_MAIL_DOUBLES per pivot tile column
  HIPCHK(hipMemcpyAsync(sl.d_fronts, nd.fronts.data(), sizeof(NDFront) * nd.fronts.size(), hipMemcpyHostToDevice, st));
  int32_t* p = sl.d_ints;
  for (const PlanInts& a : kPlanInts) {
    if (a.field == &FrameDev::dag_tasks) {   // (the work items travel here: the order of the copies on the stream is kept)
      HIPCHK(grow(sl.d_items, nd.tile_items.size() + 1));
      if (!nd.tile_items.empty())
        HIPCHK(hipMemcpyAsync(sl.d_items, nd.tile_items.data(), sizeof(NDTileItem) * nd.tile_items.size(), hipMemcpyHostToDevice, st));
    }
    const std::vector<int32_t>& v = nd.*a.src;
    h.*a.field = p;
    if (!v.empty()) HIPCHK(hipMemcpyAsync(p, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice, st));
    p += v.size();
  }
  h.tile_items = sl.d_items.p;
  h.n_dag_tasks = (int32_t)(nd.dag_tasks.size() / 2);
  h.n_dag_top_tasks = (int32_t)(nd.dag_top_tasks.size() / 2);
  h.dag_cut_depth = nd.dag_cut_depth;
  h.dag_n_tiles = (int32_t)(nd.tile_doubles / (SLM_NB * SLM_NB));
  h.dag_n_pcols = (int32_t)(nd.linv_doubles / (SLM_NB * SLM_NB));
  h.dag_n_flags = 8 + h.dag_n_tiles + 7 * h.dag_n_pcols;
  HIPCHK(grow(sl.d_dag_flags, (size_t)h.dag_n_flags));
  h.dag_flags = sl.d_dag_flags.p;
  if (!nd.block_dest.empty())
    HIPCHK(hipMemcpyAsync(sl.d_dests, nd.block_dest.data(), sizeof(NDDest) * nd.block_dest.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(sl.d_dests + nd.block_dest.size(), nd.pair_dest.data(), sizeof(NDDest) * nd.pair_dest.size(), hipMemcpyHostToDevice, st));
  h.pair_dest = sl.d_dests + nd.block_dest.size();
  h.fronts = sl.d_fronts.p;
  h.n_fronts = (int)nd.fronts.size();
  h.n_levels = (int)nd.level_start.size() - 1;
  h.ftiles = sl.ftiles.p;
  h.fvec = sl.fvec.p;
  h.flinv = sl.flinv.p;
  h.fmail = sl.fmail.p;
  h.zero_tile_doubles = nd.tile_zero_doubles;
  h.zero_vec_doubles = nd.vec_doubles;
  return SLM_OK;
}

// The bound frame's pair -> destination table (PlanCache::frame_dest) to the device.
static int upload_frame_dests(Slot& sl, hipStream_t st) {
  const std::vector<NDDest>& dest = sl.cache.frame_dest;
  HIPCHK(grow(sl.d_cur_dests, dest.size() + 1));
  if (!dest.empty()) HIPCHK(hipMemcpyAsync(sl.d_cur_dests, dest.data(), sizeof(NDDest) * dest.size(), hipMemcpyHostToDevice, st));
  sl.h.block_dest = sl.d_cur_dests.p;
  return SLM_OK;
}

// The kinds of the plan's pivot-column tiles (nd_tile_kinds) to the device.
static int upload_tile_kinds(const slm_solver* s, Slot& sl, hipStream_t st) {
  HIPCHK(hipStreamSynchronize(st));   // an earlier upload from the two host vectors may still be in flight
  std::vector<uint8_t>& kind = sl.h_tile_kind;
  std::vector<long long>& zero = sl.h_zero_tiles;
  nd_tile_kinds(sl.cache.nd, s->pure_fill, kind, zero, sl.n_piv_tiles, sl.n_pure_tiles);
  HIPCHK(grow(sl.d_tile_kind, kind.size()));
  HIPCHK(grow(sl.d_zero_tiles, zero.size() + 1));
  HIPCHK(hipMemcpyAsync(sl.d_tile_kind, kind.data(), kind.size(), hipMemcpyHostToDevice, st));
  if (!zero.empty()) HIPCHK(hipMemcpyAsync(sl.d_zero_tiles, zero.data(), sizeof(long long) * zero.size(), hipMemcpyHostToDevice, st));
  sl.h.tile_kind = sl.d_tile_kind.p;
  sl.h.zero_tiles = sl.d_zero_tiles.p;
  sl.h.n_zero_tiles = (int32_t)zero.size();
  return SLM_OK;
}

// Nested-dissection plan (symbolic analysis on the host from the coupled-pair list).  It depends only on the coupling
// graph (node KNN table + coupled-pair list): reuse it while the graph is unchanged.  The graph's hashes come from the
// device with the sizes of the data-term plan: a frame whose graph is the slot's cached one reads nothing else back --
// the lists only travel to the host when the hash says that they changed.
static int bind_symbolic_plan(slm_solver* s, Slot& sl, const slm_frame* f, const DataPlan& dp, hipStream_t st) {
  FrameDev& h = sl.h;
  PlanCache& pc = sl.cache;
  if (pc.valid && pc.knn_hash != dp.knn_hash) pc.drop_plan();   // another node graph: nothing of the old plan applies
  // same_graph: the device mirrors of the plan and of this pair list are still in place (pointers kept in h)
  enum { same_graph, reuse_plan, rebuild } what = same_graph;
  int rc = SLM_OK;
  size_t fill_hits = 0;
  if (!(pc.valid && pc.frame_hash == dp.graph_hash && pc.frame_blocks == h.n_blocks)) {
    if ((rc = read_back_graph(sl, f, st)) != SLM_OK) return rc;
    what = rebuild;
  }
  bt_mark(BT_READBACK);
  // a frame whose pairs all have a place in the plan (fill positions included) needs no new analysis
  if (what != same_graph && pc.valid && nd_frame_dests(pc.nd, f->J, sl.h_pairs.data(), sl.h_pairs.size(), pc.frame_dest, &fill_hits))
    what = reuse_plan;
  g_plan_fill_hits += (long long)fill_hits;
  if (what == rebuild) {
    // new pairs: analyse the union of what the plan already covers and this frame's list
    std::vector<uint32_t> all_pairs(pc.nd.plan_pairs.size() + sl.h_pairs.size());
    all_pairs.resize(std::set_union(pc.nd.plan_pairs.begin(), pc.nd.plan_pairs.end(), sl.h_pairs.begin(), sl.h_pairs.end(),
                                    all_pairs.begin()) - all_pairs.begin());
    // (a solver that runs its launches as one task graph -- at most two slots, or solver_path 2 -- takes the larger
    //  leaves: SLM_ND_LEAF_LATENCY, slm_nd.h)
    const int leaf = solve_is_task_graph(s, (int)s->slots.size(), f->J) ? SLM_ND_LEAF_LATENCY : SLM_ND_LEAF;
    if (!nd_build_plan(f->J, f->K_ED, sl.h_pts.data(), sl.h_knn.data(), all_pairs.data(), (int)all_pairs.size(), pc.nd, leaf)) {
      pc.drop_plan();   // no plan for this graph: the slot runs on the block-banded solver
      return SLM_OK;
    }
    ++g_plan_builds;
    rc = upload_plan(sl, st);
    if (rc == SLM_OK && !nd_frame_dests(pc.nd, f->J, sl.h_pairs.data(), sl.h_pairs.size(), pc.frame_dest, &fill_hits))
      rc = fail(SLM_ERR_INVALID, "slm_bind_frame: internal error (pair missing from its own plan)");
  } else if (what == reuse_plan) {
    ++g_plan_reuses;
  }
  if (what != same_graph) {
    // (after a reuse too: the plan's destination list may have grown by fill-position pairs)
    if (rc == SLM_OK) rc = upload_frame_dests(sl, st);
    if (rc == SLM_OK) rc = upload_tile_kinds(s, sl, st);
    if (rc != SLM_OK) {   // device mirrors freed or half written: a later bind of the same graph must not trust them
      if (what == rebuild) pc.drop_plan();
      else pc.frame_stale();
      return rc;
    }
    pc.valid = true;
    pc.knn_hash = dp.knn_hash;
    pc.frame_hash = dp.graph_hash;
    pc.frame_blocks = h.n_blocks;
  }
  h.nd_ready = 1;
  return SLM_OK;
}

// The MODEL-side half of a bind (what depends on sf.points / sf.knn_indices / sf.knn_w / ED_nodes only: the tuple-sorted
// copies and indices of the data term, the hashes of the coupling graph, the symbolic plan of the solver, the slot's
// grow-only work buffers).  Leaves the slot UNBOUND; bind_target_part completes it.
static int bind_model_part(slm_solver* s, int32_t slot, const slm_frame* f, hipStream_t st, PrepBuffers* prep) {
  int rc = check_model_args(s, slot, f);
  if (rc != SLM_OK) return rc;
  Slot& sl = s->slots[slot];
  bt_mark(BT_ENTRY);
  DataPlan dp;
  if ((rc = reset_slot(s, sl, f, st)) != SLM_OK) return rc;
  if ((rc = bind_data_plan(s, sl, f, st, prep, dp)) != SLM_OK) return rc;
  if ((rc = bind_shard_share(s, sl, f, dp.form, st)) != SLM_OK) return rc;
  sl.h.nd_ready = 0;
  if ((dp.form == DataForm::tuple || dp.form == DataForm::pairs) && s->cfg.solver_path != 1)
    if ((rc = bind_symbolic_plan(s, sl, f, dp, st)) != SLM_OK) return rc;
  bt_mark(BT_SYMBOLIC);
  return SLM_OK;
}

// The TARGET-side half: the frame's target tables, image size and intrinsics; descriptor upload, LM state reset.
static int bind_target_part(slm_solver* s, int32_t slot, const slm_frame* f, hipStream_t st) {
  if (f->H < 2 || f->W < 2 || f->T < 0) return fail(SLM_ERR_INVALID, "slm_bind_frame: bad sizes");
  if ((f->T > 0 && (!f->tgt_points || !f->tgt_norms)) || !f->index_map || !f->tgt_valid)
    return fail(SLM_ERR_INVALID, "slm_bind_frame: null device pointer");
  Slot& sl = s->slots[slot];
  FrameDev& h = sl.h;
  h.f = *f;
  HIPCHK(grow(sl.tgt_pn, (size_t)2 * (f->T > 0 ? f->T : 1)));
  h.tgt_pn = sl.tgt_pn.p;
  launch_pack_target(f->T, f->tgt_points, f->tgt_norms, h.tgt_pn, st);
  HIPCHK(grow(sl.tgt_px, (size_t)2 * f->H * f->W));
  h.tgt_px = sl.tgt_px.p;
  launch_pack_target_px(f->H * f->W, f->index_map, f->tgt_valid, f->tgt_points, f->tgt_norms, h.tgt_px, st);
  h.bound = 1;
  if (s->corr_mode) {   // a new frame: the slot's correspondences belonged to the last one
    sl.corr.has = 0;
    HIPCHK(hipMemsetAsync(&s->corr_dev[slot].has, 0, sizeof(int32_t), st));
  }
  if (s->weights_on) {   // and so did its semantic inputs
    sl.wdev.has = 0;
    HIPCHK(hipMemsetAsync(&s->w_dev[slot].has, 0, sizeof(int32_t), st));
  }
  if (s->morph_on) {   // and the inputs of the boundary-morph term: the slot runs without the term until slm_bind_morph
    sl.morph.has = 0;
    HIPCHK(hipMemsetAsync(&s->morph_dev[slot].has, 0, sizeof(int32_t), st));
  }
  if (s->face_on) {   // the slot's mesh as this bind's plan placed it (through a pinned mirror, like the descriptor below)
    HIPCHK(sl.face_pin.grow(1, 1));
    memcpy(sl.face_pin.data(), &sl.face, sizeof(FaceDev));
    HIPCHK(hipMemcpyAsync(s->face_dev + slot, sl.face_pin.data(), sizeof(FaceDev), hipMemcpyHostToDevice, st));
  }
  // descriptor -> device through the slot's pinned mirror: no wait for the copy (the mirror always holds the newest
  // host state, and every change of it is followed by another copy on the stream)
  HIPCHK(sl.h_pin.grow(1, 1));
  memcpy(sl.h_pin.data(), &h, sizeof(FrameDev));
  HIPCHK(hipMemcpyAsync(s->frames_dev + slot, sl.h_pin.data(), sizeof(FrameDev), hipMemcpyHostToDevice, st));
  bt_mark(BT_DESCRIPTOR);
  if (!h.nd_ready) {
    std::lock_guard<std::mutex> lock(s->band_mutex);
    int rc = ensure_band(s, slot, st);
    if (rc) {   // (a refused table: the slot stays unbound, on the device too)
      h.bound = 0;
      memcpy(sl.h_pin.data(), &h, sizeof(FrameDev));
      (void)hipMemcpyAsync(s->frames_dev + slot, sl.h_pin.data(), sizeof(FrameDev), hipMemcpyHostToDevice, st);
      return rc;
    }
  }
  launch_init_slot(s->frames_dev, slot, f->J, s->cfg, st);
  HIPCHK(hipMemsetAsync(s->reuse_dev + slot, 0, sizeof(int), st));   // a new frame: nothing to reuse
  HIPCHK(hipGetLastError());
  bt_mark(BT_END);
  if (bind_trace_threshold() >= 0.0 && g_bt.n >= 2 && g_bt.t[g_bt.n - 1] - g_bt.t[0] > bind_trace_threshold()) {
    char buf[256];
    int o = snprintf(buf, sizeof(buf), "[slm bind trace] slot %d start %.3f stages(ms):", slot, g_bt.t[0]);
    for (int i = 1; i < g_bt.n && o < 220; ++i) o += snprintf(buf + o, sizeof(buf) - o, " %.3f", g_bt.t[i] - g_bt.t[i - 1]);
    fprintf(stderr, "%s\n", buf);
  }
  return SLM_OK;
}

static bool same_model(const slm_frame& a, const slm_frame& b) {
  return a.N == b.N && a.J == b.J && a.K == b.K && a.K_ED == b.K_ED && a.state_f64 == b.state_f64 && a.sf_points == b.sf_points &&
         a.sf_knn_idx == b.sf_knn_idx && a.sf_knn_w == b.sf_knn_w && a.ed_points == b.ed_points && a.ed_knn_idx == b.ed_knn_idx;
}

// waits for the slot's queued model-side preparation, if any (host side: the worker has finished the job)
void join_prepare(slm_solver* s, int slot) {
  Slot& sl = s->slots[slot];
  if (sl.prep_ticket) {
    s->prep_worker.wait(sl.prep_ticket);
    sl.prep_ticket = 0;
  }
}

static int bind_frame_impl(slm_solver* s, int32_t slot, const slm_frame* f, hipStream_t st, PrepBuffers* prep) {
  if (slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, "slm_bind_frame: bad slot");
  Slot& sl = s->slots[slot];
  join_prepare(s, slot);
  // A model prepared ahead (slm_prepare_model) serves ONE bind, and only the bind of the very arrays it read: the
  // frame's update / fusion rewrites them in place afterwards.
  const bool prepared = sl.model_ready && same_model(sl.prep_model, *f);
  sl.model_ready = false;
  // Whatever becomes of the preparation, its launches ran on the solver's own stream and wrote this slot's plan buffers
  // (and read the caller's arrays): everything the bind enqueues comes after them -- also when the preparation is NOT
  // used (another model, slm_discard_prepared) and the full bind rewrites the same buffers.
  if (sl.prep_recorded) {
    sl.prep_recorded = false;
    HIPCHK(hipStreamWaitEvent(st, sl.prep_done, 0));
  }
  if (prepared) {
    if (sl.prep_rc != SLM_OK) return fail(sl.prep_rc, sl.prep_err.c_str());
    bt_mark(BT_ENTRY);
  } else {
    const int rc = bind_model_part(s, slot, f, st, prep);
    if (rc != SLM_OK) return rc;
  }
  return bind_target_part(s, slot, f, st);
}

extern "C" {

int slm_bind_frame(slm_solver* s, int32_t slot, const slm_frame* f, void* stream) {
  if (!s || !f) return fail(SLM_ERR_INVALID, "slm_bind_frame: null argument");
  return bind_frame_impl(s, slot, f, (hipStream_t)stream, s->prep);
}

int slm_prepare_model(slm_solver* s, int32_t slot, const slm_frame* model, void* stream) {
  if (!s || !model) return fail(SLM_ERR_INVALID, "slm_prepare_model: null argument");
  if (slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, "slm_prepare_model: bad slot");
  Slot& sl = s->slots[slot];
  join_prepare(s, slot);
  sl.model_ready = false;
  sl.h.bound = 0;                   // the slot's plan is being rebuilt: unbound until the next slm_bind_frame
  if (!s->prep_stream) HIPCHK(hipStreamCreateWithFlags(&s->prep_stream, hipStreamNonBlocking));
  if (!s->prep_async) {
    s->prep_async = prep_create();
    if (!s->prep_async) return fail(SLM_ERR_HIP, "slm_prepare_model: out of memory");
  }
  if (!sl.prep_fork) HIPCHK(hipEventCreateWithFlags(&sl.prep_fork, hipEventDisableTiming));
  if (!sl.prep_done) HIPCHK(hipEventCreateWithFlags(&sl.prep_done, hipEventDisableTiming));
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  sl.prep_model = *model;
  sl.prep_model.T = 0;              // (only the model fields are read)
  sl.prep_model.tgt_points = sl.prep_model.tgt_norms = nullptr;
  sl.prep_model.index_map = nullptr;
  sl.prep_model.tgt_valid = nullptr;
  sl.prep_rc = SLM_OK;
  HIPCHK(hipEventRecord(sl.prep_fork, (hipStream_t)stream));   // the preparation sees what the caller has enqueued so far
  try {
    sl.prep_err.clear();
    sl.prep_ticket = s->prep_worker.submit([s, slot, dev] {
      Slot& w = s->slots[slot];
      int rc = SLM_OK;
      try {
        if (hipSetDevice(dev) != hipSuccess || hipStreamWaitEvent(s->prep_stream, w.prep_fork, 0) != hipSuccess) {
          rc = fail(SLM_ERR_HIP, "slm_prepare_model: worker setup failed");
        } else {
          rc = bind_model_part(s, slot, &w.prep_model, s->prep_stream, s->prep_async);
          // (recorded after a failed preparation too: its launches up to the failure still touch the slot)
          if (hipEventRecord(w.prep_done, s->prep_stream) != hipSuccess) {
            if (rc == SLM_OK) rc = fail(SLM_ERR_HIP, "slm_prepare_model: hipEventRecord failed");
          } else {
            w.prep_recorded = true;
          }
        }
        if (rc != SLM_OK) w.prep_err = slm_last_error();   // (thread-local text of the worker)
      } catch (...) {
        rc = SLM_ERR_HIP;
        try { w.prep_err = "slm_prepare_model: out of host memory in the worker"; } catch (...) {}
      }
      w.prep_rc = rc;
      w.model_ready = true;         // (an error is reported by the bind that consumes the preparation)
    });
  } catch (...) {
    sl.prep_ticket = 0;
    return fail(SLM_ERR_HIP, "slm_prepare_model: could not start the worker");
  }
  return SLM_OK;
}

int slm_discard_prepared(slm_solver* s, int32_t slot) {
  if (!s) return fail(SLM_ERR_INVALID, "slm_discard_prepared: null argument");
  if (slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, "slm_discard_prepared: bad slot");
  join_prepare(s, slot);
  s->slots[slot].model_ready = false;   // (prep_recorded stays: the next bind of the slot still orders itself behind the launches)
  return SLM_OK;
}

// Scratch buffers, a stream and an event per bind worker, and the fork event.  Each one is pushed into its pool as soon as
// it exists, so a failure half way leaves nothing behind that slm_destroy does not release (the pools are reserved
// first: push_back cannot throw after).
static int ensure_bind_workers(slm_solver* s, int W) {
  try {
    s->bind_prep.reserve(64);
    s->bind_streams.reserve(64);
    s->bind_events.reserve(65);
  } catch (...) {
    return fail(SLM_ERR_HIP, "slm_bind_frames: out of host memory");
  }
  while ((int)s->bind_prep.size() < W) {
    PrepBuffers* pb = prep_create();
    if (!pb) return fail(SLM_ERR_HIP, "slm_bind_frames: out of memory");
    s->bind_prep.push_back(pb);
  }
  while ((int)s->bind_streams.size() < W) {
    hipStream_t q = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    s->bind_streams.push_back(q);
  }
  while ((int)s->bind_events.size() < W + 1) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s->bind_events.push_back(e);
  }
  return SLM_OK;
}

// Host wait for the work already on `st`.  The binds read sizes back, so they wait for it in any case: wait HERE, on one
// thread, rather than with W workers spinning in their first read-back for as long as the previous LM run takes (8 busy
// threads for tens of milliseconds per step cost the process its CPU quota on the GPU box).
// This is the one LONG host wait of a tracking step (the LM run of the previous step, tens of milliseconds).  Every
// blocking wait of this HIP runtime spins (hipStreamSynchronize, hipEventSynchronize with or without
// hipEventBlockingSync: one CPU at 100 %, tools/studies/wait_cpu.py), which counts where the ranks of a node share a
// CPU quota: the wait is therefore a poll of an event with naps while the end is far (estimated from the previous
// wait on this solver) and a tight poll only over the last stretch.  SLM_SPIN_WAIT=1: hipStreamSynchronize instead.
static int drain_stream(slm_solver* s, hipStream_t st) {
  static const bool spin_wait = [] {
    const char* e = getenv("SLM_SPIN_WAIT");
    return e && atoi(e) != 0;
  }();
  if (spin_wait) {
    HIPCHK(hipStreamSynchronize(st));
    return SLM_OK;
  }
  if (!s->drain_event) HIPCHK(hipEventCreateWithFlags(&s->drain_event, hipEventDisableTiming));
  HIPCHK(hipEventRecord(s->drain_event, st));
  const auto w0 = std::chrono::steady_clock::now();
  auto waited_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count(); };
  const double est = s->drain_est_ms;
  for (;;) {
    const hipError_t q = hipEventQuery(s->drain_event);
    if (q == hipSuccess) break;
    (void)hipGetLastError();   // hipErrorNotReady is not an error here: keep it out of the sticky last-error slot
    if (q != hipErrorNotReady) return fail(SLM_ERR_HIP, hipGetErrorString(q));
    const double w = waited_ms();
    if (w < 0.85 * est - 0.4) {
      std::this_thread::sleep_for(std::chrono::microseconds(300));    // far from the expected end
    } else if (w > est + 1.5) {
      std::this_thread::sleep_for(std::chrono::microseconds(100));    // overdue (the step got longer): nap again
    } else {
      __builtin_ia32_pause();                                          // the last stretch: poll
    }
  }
  s->drain_est_ms = waited_ms();
  return SLM_OK;
}

int slm_bind_frames(slm_solver* s, int32_t first_slot, int32_t n_frames, const slm_frame* frames, void* stream) {
  if (!s || !frames) return fail(SLM_ERR_INVALID, "slm_bind_frames: null argument");
  if (first_slot < 0 || n_frames < 1 || first_slot + n_frames > (int)s->slots.size())
    return fail(SLM_ERR_INVALID, "slm_bind_frames: slot range out of bounds");
  hipStream_t st = (hipStream_t)stream;
  if (n_frames == 1) return bind_frame_impl(s, first_slot, frames, st, s->prep);
  // The preparation of a frame is a chain of ~40 small launches and four size read-backs: latency, not
  // throughput.  The frames of a batch are therefore bound CONCURRENTLY -- one host thread, stream and set of
  // scratch buffers per frame (up to kBindWorkers at a time), forked from and joined into the caller's stream.
  constexpr int kBindWorkers = 8;
  const int W = std::min(n_frames, kBindWorkers);
  int rc = ensure_bind_workers(s, W);
  if (rc != SLM_OK) return rc;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const double bt0 = bind_trace_threshold() >= 0.0 ? bt_now() : 0.0;
  if ((rc = drain_stream(s, st)) != SLM_OK) return rc;
  const double bt1 = bind_trace_threshold() >= 0.0 ? bt_now() : 0.0;
  HIPCHK(hipEventRecord(s->bind_events[W], st));            // fork: the workers see everything enqueued on `st` so far
  // (no exception may cross the extern "C" boundary: the containers are sized before any worker starts, the pool throws
  //  only from thread creation, and a worker catches whatever its bind throws -- std::bad_alloc from a plan vector)
  int rcs[64];
  std::string errs[64];
  for (int w = 0; w < W; ++w) rcs[w] = SLM_OK;
  const std::function<void(int)> work = [&](int w) {
    try {
      if (hipSetDevice(dev) != hipSuccess || hipStreamWaitEvent(s->bind_streams[w], s->bind_events[W], 0) != hipSuccess) {
        rcs[w] = SLM_ERR_HIP;
        errs[w] = "slm_bind_frames: worker setup failed";
        return;
      }
      for (int i = w; i < n_frames; i += W) {
        const int rc = bind_frame_impl(s, first_slot + i, frames + i, s->bind_streams[w], s->bind_prep[w]);
        if (rc != SLM_OK) {
          rcs[w] = rc;
          errs[w] = slm_last_error();   // thread-local text of this worker
          return;
        }
      }
      if (hipEventRecord(s->bind_events[w], s->bind_streams[w]) != hipSuccess) rcs[w] = SLM_ERR_HIP;
    } catch (...) {
      rcs[w] = SLM_ERR_HIP;
      try { errs[w] = "slm_bind_frames: out of host memory in a bind worker"; } catch (...) {}
    }
  };
  try {
    s->bind_pool.run(W, work);
  } catch (...) {
    return fail(SLM_ERR_HIP, "slm_bind_frames: could not start the bind workers");
  }
  for (int w = 0; w < W; ++w)
    if (rcs[w] != SLM_OK) return fail(rcs[w], errs[w].c_str());
  if (bind_trace_threshold() >= 0.0 && bt_now() - bt1 > bind_trace_threshold())
    fprintf(stderr, "[slm bind trace] batch of %d: drained the stream at %.3f (waited %.3f ms), workers done %.3f ms later\n",
            n_frames, bt1, bt1 - bt0, bt_now() - bt1);
  for (int w = 0; w < W; ++w) HIPCHK(hipStreamWaitEvent(st, s->bind_events[w], 0));   // join
  return SLM_OK;
}

}  // extern "C"
