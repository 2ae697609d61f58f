// slm_terms.hip -- the entry points of the LM path's opt-in terms (include/super_lm.h): the flow-correspondence term
// (kernels in slm_corr.hip), the triangle-area face term (slm_face.hip), the semantic boundary-morph term (slm_morph.hip)
// and the per-residual weights of the data term (the weighted kernels in slm_data.hip).  Enabling, binding a slot's inputs
// and the parity read-outs; the LM step that runs the terms is slm_lm.hip.  Host side only orchestrates launches.
#include "slm_solver.h"

namespace {
// the argument checks the per-slot entry points of a term share (enabled: the term is on; enable: the call that turns it
// on); *out = the slot
int term_slot(const char* fn, slm_solver* s, bool args_ok, int32_t slot, bool enabled, const char* enable, Slot** out) {
  const std::string pre = std::string(fn) + ": ";
  if (!s || !args_ok) return fail(SLM_ERR_INVALID, pre + "null argument");
  if (slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, pre + "bad slot");
  if (!enabled) return fail(SLM_ERR_UNSUPPORTED, pre + enable + " first");
  join_prepare(s, slot);
  if (!s->slots[slot].h.bound) return fail(SLM_ERR_UNBOUND, pre + "slm_bind_frame first");
  *out = &s->slots[slot];
  return SLM_OK;
}
}  // namespace

extern "C" {

// ---- flow-correspondence term (include/super_lm.h; kernels in slm_corr.hip) -----------------------------------------
int slm_enable_corr(slm_solver* s, int32_t mode, double weight) {
  if (!s) return fail(SLM_ERR_INVALID, "slm_enable_corr: null argument");
  if (mode < 0 || mode > 2) return fail(SLM_ERR_INVALID, "slm_enable_corr: mode must be 0 (off), 1 (point-point) or 2 (point-plane)");
  if (!(weight - weight == 0.0)) return fail(SLM_ERR_INVALID, "slm_enable_corr: weight must be finite");
  if (s->cfg.data_path == 1) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_corr: needs the pair-record data path (data_path 0 or 2)");
  if (s->cfg.solver_path == 1) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_corr: needs a nested-dissection solver_path (0, 2, 3 or 4)");
  if (!s->cfg.use_data) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_corr: needs the data term (use_data 1)");
  if (s->shard_mode)
    return fail(SLM_ERR_UNSUPPORTED, "slm_enable_corr: the solver is sharded (slm_set_shard); the term needs every surfel of the frame "
                                     "on one device");
  for (const Slot& sl : s->slots)
    if (sl.h.bound || sl.prep_ticket || sl.model_ready)
      return fail(SLM_ERR_INVALID, "slm_enable_corr: a slot is already bound; call it after slm_create and before the first bind");
  if (mode && !s->corr_dev) {
    HIPCHK(s->corr_dev.grow(s->slots.size(), s->slots.size()));
    HIPCHK(hipMemset(s->corr_dev, 0, sizeof(CorrDev) * s->slots.size()));
  }
  s->corr_mode = mode;
  s->corr_w = mode ? weight : 0.0;
  return SLM_OK;
}

// the slot's target buffers at the bound frame's size, and the descriptor (has = 1) on its way to the device
static int corr_publish(slm_solver* s, int slot, Slot& sl, hipStream_t st) {
  sl.corr.has = 1;
  HIPCHK(hipMemcpyAsync(s->corr_dev + slot, &sl.corr, sizeof(CorrDev), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // (the source is the slot's own mirror, which the next bind rewrites)
  return SLM_OK;
}
static int corr_buffers(Slot& sl) {
  const size_t N = (size_t)std::max(sl.h.f.N, 1);
  HIPCHK(grow(sl.corr_o, 3 * N));
  HIPCHK(grow(sl.corr_n, 3 * N));
  HIPCHK(grow(sl.corr_valid, N));
  sl.corr.o = sl.corr_o.p;
  sl.corr.n = sl.corr_n.p;
  sl.corr.valid = sl.corr_valid.p;
  return SLM_OK;
}

int slm_bind_corr_flow(slm_solver* s, int32_t slot, const float* flow, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_bind_corr_flow", s, flow != nullptr, slot, s && s->corr_mode, "slm_enable_corr", &sp);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = corr_buffers(*sp)) != SLM_OK) return rc;
  // (the kernel reads the buffers' addresses from the device descriptor: publish first)
  if ((rc = corr_publish(s, slot, *sp, st)) != SLM_OK) return rc;
  launch_corr_targets(s->frames_dev, s->corr_dev, slot, sp->h.f.N, flow, st);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_bind_corr_points(slm_solver* s, int32_t slot, const double* pts, const double* nrm, const uint8_t* valid, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_bind_corr_points", s, pts != nullptr && valid != nullptr, slot, s && s->corr_mode, "slm_enable_corr", &sp);
  if (rc) return rc;
  if (s->corr_mode == 2 && !nrm) return fail(SLM_ERR_INVALID, "slm_bind_corr_points: nrm is required in mode 2 (point-plane)");
  hipStream_t st = (hipStream_t)stream;
  if ((rc = corr_buffers(*sp)) != SLM_OK) return rc;
  const size_t N = (size_t)sp->h.f.N;
  if (N > 0) {
    HIPCHK(hipMemcpyAsync(sp->corr.o, pts, sizeof(double) * 3 * N, hipMemcpyDeviceToDevice, st));
    if (nrm) HIPCHK(hipMemcpyAsync(sp->corr.n, nrm, sizeof(double) * 3 * N, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemsetAsync(sp->corr.n, 0, sizeof(double) * 3 * N, st));
    HIPCHK(hipMemcpyAsync(sp->corr.valid, valid, N, hipMemcpyDeviceToDevice, st));
  }
  return corr_publish(s, slot, *sp, st);
}

int slm_corr_get_targets(slm_solver* s, int32_t slot, double* pts, double* nrm, uint8_t* valid, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_corr_get_targets", s, true, slot, s && s->corr_mode, "slm_enable_corr", &sp);
  if (rc) return rc;
  if (!sp->corr.has) return fail(SLM_ERR_UNBOUND, "slm_corr_get_targets: no correspondences bound to the slot");
  hipStream_t st = (hipStream_t)stream;
  const size_t N = (size_t)sp->h.f.N;
  if (N > 0) {
    if (pts) HIPCHK(hipMemcpyAsync(pts, sp->corr.o, sizeof(double) * 3 * N, hipMemcpyDeviceToDevice, st));
    if (nrm) HIPCHK(hipMemcpyAsync(nrm, sp->corr.n, sizeof(double) * 3 * N, hipMemcpyDeviceToDevice, st));
    if (valid) HIPCHK(hipMemcpyAsync(valid, sp->corr.valid, N, hipMemcpyDeviceToDevice, st));
  }
  return SLM_OK;
}

int slm_corr_loss(slm_solver* s, int32_t slot, double* out, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_corr_loss", s, out != nullptr, slot, s && s->corr_mode, "slm_enable_corr", &sp);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = clear_flags(s, slot, st)) != SLM_OK) return rc;
  const LossParts lp = loss_parts(s, 0);
  launch_corr_loss(s->frames_dev + slot, s->corr_dev + slot, 1, sp->h.f.K, s->corr_mode, s->corr_w, 0, lp.corr_direct, lp.corr_cnt, st);
  launch_term_loss_out(s->frames_dev, slot, lp.corr_direct, kCorrBlocks, lp.corr_cnt, nullptr, out, st);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

// ---- triangle-area face term (include/super_lm.h; kernels in slm_face.hip) -------------------------------------------
int slm_enable_face(slm_solver* s, double weight) {
  if (!s) return fail(SLM_ERR_INVALID, "slm_enable_face: null argument");
  if (!(weight - weight == 0.0)) return fail(SLM_ERR_INVALID, "slm_enable_face: weight must be finite");
  if (s->cfg.data_path == 1) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_face: needs the pair-record data path (data_path 0 or 2)");
  if (s->cfg.solver_path == 1) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_face: needs a nested-dissection solver_path (0, 2, 3 or 4)");
  if (!s->cfg.use_data) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_face: needs the data term (use_data 1)");
  if (s->shard_mode)
    return fail(SLM_ERR_UNSUPPORTED, "slm_enable_face: the solver is sharded (slm_set_shard); the term's mesh is not sharded");
  for (const Slot& sl : s->slots)
    if (sl.h.bound || sl.prep_ticket || sl.model_ready || sl.loss_part)   // (loss_part: the first bind sizes it for the term)
      return fail(SLM_ERR_INVALID, "slm_enable_face: a slot is already bound; call it after slm_create and before the first bind");
  const bool on = weight != 0.0;
  if (on && !s->face_dev) {
    HIPCHK(s->face_dev.grow(s->slots.size(), s->slots.size()));
    HIPCHK(hipMemset(s->face_dev, 0, sizeof(FaceDev) * s->slots.size()));
  }
  s->face_on = on;
  s->face_w = on ? weight : 0.0;
  return SLM_OK;
}

int slm_set_face_mesh(slm_solver* s, int32_t slot, int32_t n_triangles, const int32_t* tri, const double* areas, void* stream) {
  if (!s || (n_triangles > 0 && (!tri || !areas))) return fail(SLM_ERR_INVALID, "slm_set_face_mesh: null argument");
  if (slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, "slm_set_face_mesh: bad slot");
  if (n_triangles < 0) return fail(SLM_ERR_INVALID, "slm_set_face_mesh: n_triangles must be >= 0");
  if (!s->face_on) return fail(SLM_ERR_UNSUPPORTED, "slm_set_face_mesh: slm_enable_face first");
  hipStream_t st = (hipStream_t)stream;
  Slot& sl = s->slots[slot];
  // the slot's plan holds the pairs of the mesh it was bound with: a queued preparation is settled and dropped, and the
  // slot is unbound until its next bind
  join_prepare(s, slot);
  sl.model_ready = false;
  sl.h.bound = 0;
  sl.face = FaceDev{};
  const size_t F = (size_t)n_triangles;
  if (F > 0) {
    HIPCHK(grow(sl.face_tri, 3 * F));
    HIPCHK(grow(sl.face_areas, F));
    HIPCHK(hipMemcpyAsync(sl.face_tri, tri, sizeof(int32_t) * 3 * F, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(sl.face_areas, areas, sizeof(double) * F, hipMemcpyDeviceToDevice, st));
    sl.face.tri = sl.face_tri.p;
    sl.face.areas = sl.face_areas.p;
    sl.face.n_tri = n_triangles;
  }
  HIPCHK(hipMemsetAsync(s->face_dev + slot, 0, sizeof(FaceDev), st));   // (ready = 0 on the device until the bind publishes it)
  HIPCHK(hipMemsetAsync(&s->frames_dev[slot].bound, 0, sizeof(int32_t), st));
  return SLM_OK;
}

int slm_face_loss(slm_solver* s, int32_t slot, double* out, void* stream) {
  if (!s || !out) return fail(SLM_ERR_INVALID, "slm_face_loss: null argument");
  if (slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, "slm_face_loss: bad slot");
  if (!s->face_on) return fail(SLM_ERR_UNSUPPORTED, "slm_face_loss: slm_enable_face first");
  join_prepare(s, slot);
  if (!s->slots[slot].h.bound) return fail(SLM_ERR_UNBOUND, "slm_face_loss: slm_bind_frame first");
  hipStream_t st = (hipStream_t)stream;
  int rc = clear_flags(s, slot, st);
  if (rc != SLM_OK) return rc;
  const int part = loss_parts(s, 0).face_direct;
  launch_face_loss(s->frames_dev + slot, s->face_dev + slot, 1, s->face_w, 0, part, st);
  launch_term_loss_out(s->frames_dev, slot, part, kFaceBlocks, -1, s->face_dev, out, st);   // (the count: the mesh's triangles)
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

// ---- semantic boundary-morph term (include/super_lm.h; kernels in slm_morph.hip) --------------------------------------
int slm_enable_morph(slm_solver* s, double weight) {
  if (!s) return fail(SLM_ERR_INVALID, "slm_enable_morph: null argument");
  if (!(weight - weight == 0.0)) return fail(SLM_ERR_INVALID, "slm_enable_morph: weight must be finite");
  if (s->cfg.data_path == 1) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_morph: needs the pair-record data path (data_path 0 or 2)");
  if (s->cfg.solver_path == 1) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_morph: needs a nested-dissection solver_path (0, 2, 3 or 4)");
  if (!s->cfg.use_data) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_morph: needs the data term (use_data 1)");
  if (s->shard_mode)
    return fail(SLM_ERR_UNSUPPORTED, "slm_enable_morph: the solver is sharded (slm_set_shard); the term needs every surfel of the frame "
                                     "on one device");
  for (const Slot& sl : s->slots)
    if (sl.h.bound || sl.prep_ticket || sl.model_ready || sl.loss_part)   // (loss_part: the first bind sizes it for the term)
      return fail(SLM_ERR_INVALID, "slm_enable_morph: a slot is already bound; call it after slm_create and before the first bind");
  const bool on = weight != 0.0;
  if (on && !s->morph_dev) {
    HIPCHK(s->morph_dev.grow(s->slots.size(), s->slots.size()));
    HIPCHK(hipMemset(s->morph_dev, 0, sizeof(MorphDev) * s->slots.size()));
  }
  s->morph_on = on;
  s->morph_w = on ? weight : 0.0;
  return SLM_OK;
}

int slm_bind_morph(slm_solver* s, int32_t slot, int32_t num_classes, const int32_t* img_seg, const float* img_seg_conf,
                   const int32_t* sf_seg, int32_t* edge_counts_host, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_bind_morph", s, img_seg != nullptr && img_seg_conf != nullptr && sf_seg != nullptr, slot, s && s->morph_on,
                     "slm_enable_morph", &sp);
  if (rc) return rc;
  if (num_classes < 1 || num_classes > SLM_MAX_CLASSES)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_morph: num_classes must be in 1..SLM_MAX_CLASSES (4)");
  hipStream_t st = (hipStream_t)stream;
  Slot& sl = *sp;
  const slm_frame& f = sl.h.f;
  // the boundary lists of the frame's classes, once per bind (a size read-back: the host waits for the stream here)
  HIPCHK(sem_extract_edges(sl.morph_edges, num_classes, img_seg, f.H, f.W, sl.morph.edge_off, st));
  const size_t N = (size_t)std::max(f.N, 1);
  HIPCHK(grow(sl.morph_kept, N));
  HIPCHK(grow(sl.morph_target, 2 * N));
  HIPCHK(grow(sl.morph_li, N));
  HIPCHK(grow(sl.morph_part, 3 * ((N + 255) / 256)));
  HIPCHK(grow(sl.morph_stat, 4));
  HIPCHK(hipMemsetAsync(sl.morph_stat, 0, sizeof(double) * 4, st));
  sl.morph.img_seg_conf = img_seg_conf;
  sl.morph.sf_seg = sf_seg;
  sl.morph.edge_xy = sl.morph_edges.edge_xy;
  sl.morph.kept = sl.morph_kept.p;
  sl.morph.target = sl.morph_target.p;
  sl.morph.li = sl.morph_li.p;
  sl.morph.part = sl.morph_part.p;
  sl.morph.stat = sl.morph_stat.p;
  sl.morph.C = num_classes;
  sl.morph.has = 1;
  HIPCHK(hipMemcpyAsync(s->morph_dev + slot, &sl.morph, sizeof(MorphDev), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // (the source is the slot's own mirror, which the next bind rewrites)
  if (edge_counts_host)
    for (int c = 0; c < num_classes; ++c) edge_counts_host[c] = sl.morph.edge_off[c + 1] - sl.morph.edge_off[c];
  return SLM_OK;
}

int slm_morph_loss(slm_solver* s, int32_t slot, double* out, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_morph_loss", s, out != nullptr, slot, s && s->morph_on, "slm_enable_morph", &sp);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = clear_flags(s, slot, st)) != SLM_OK) return rc;
  // (a slot without inputs: the fold alone, which stores {0, 0, 0})
  launch_morph_select(s->frames_dev + slot, s->morph_dev + slot, 1, sp->morph.has ? sp->h.f.N : 0, sp->h.f.K, s->morph_w, 0, -1, out, st);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_morph_targets(slm_solver* s, int32_t slot, uint8_t* kept, double* target_xy, double* li, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_morph_targets", s, true, slot, s && s->morph_on, "slm_enable_morph", &sp);
  if (rc) return rc;
  if (!sp->morph.has) return fail(SLM_ERR_UNBOUND, "slm_morph_targets: slm_bind_morph first");
  hipStream_t st = (hipStream_t)stream;
  if ((rc = clear_flags(s, slot, st)) != SLM_OK) return rc;
  const size_t N = (size_t)sp->h.f.N;
  launch_morph_select(s->frames_dev + slot, s->morph_dev + slot, 1, sp->h.f.N, sp->h.f.K, s->morph_w, 0, -1, nullptr, st);
  HIPCHK(hipGetLastError());
  if (N > 0) {
    if (kept) HIPCHK(hipMemcpyAsync(kept, sp->morph.kept, N, hipMemcpyDeviceToDevice, st));
    if (target_xy) HIPCHK(hipMemcpyAsync(target_xy, sp->morph.target, sizeof(double) * 2 * N, hipMemcpyDeviceToDevice, st));
    if (li) HIPCHK(hipMemcpyAsync(li, sp->morph.li, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
  }
  return SLM_OK;
}

// ---- per-residual weights of the data term (include/super_lm.h; the weighted kernels in slm_data.hip) -----------------
int slm_enable_data_weights(slm_solver* s, int32_t seg_mode, double pp_max) {
  if (!s) return fail(SLM_ERR_INVALID, "slm_enable_data_weights: null argument");
  if (seg_mode < 0 || seg_mode > 2) return fail(SLM_ERR_INVALID, "slm_enable_data_weights: seg_mode must be 0 (none), 1 (hard) or 2 (soft)");
  if (!(pp_max - pp_max == 0.0) || pp_max < 0.0) return fail(SLM_ERR_INVALID, "slm_enable_data_weights: pp_max must be finite and >= 0");
  if (s->cfg.data_path == 1)
    return fail(SLM_ERR_UNSUPPORTED, "slm_enable_data_weights: needs the pair-record data path (data_path 0 or 2)");
  if (s->cfg.solver_path == 1)
    return fail(SLM_ERR_UNSUPPORTED, "slm_enable_data_weights: needs a nested-dissection solver_path (0, 2, 3 or 4)");
  if (!s->cfg.use_data) return fail(SLM_ERR_UNSUPPORTED, "slm_enable_data_weights: needs the data term (use_data 1)");
  for (const Slot& sl : s->slots)
    if (sl.h.bound || sl.prep_ticket || sl.model_ready)
      return fail(SLM_ERR_INVALID, "slm_enable_data_weights: a slot is already bound; call it after slm_create and before the first bind");
  const bool on = seg_mode != 0 || pp_max > 0.0;
  if (on && !s->w_dev) {
    HIPCHK(s->w_dev.grow(s->slots.size(), s->slots.size()));
    HIPCHK(hipMemset(s->w_dev, 0, sizeof(DataWeightDev) * s->slots.size()));
  }
  s->weights_on = on;
  s->w_seg_mode = seg_mode;
  s->w_pp_max = seg_mode ? 0.0 : pp_max;   // (ignored with a semantic weight, like the reference)
  return SLM_OK;
}

int slm_bind_data_semantic(slm_solver* s, int32_t slot, int32_t num_classes, const int32_t* sf_seg, const float* sf_seg_conf,
                           const float* tgt_seg_conf, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_bind_data_semantic", s, sf_seg != nullptr && sf_seg_conf != nullptr && tgt_seg_conf != nullptr, slot,
                     s && s->weights_on, "slm_enable_data_weights", &sp);
  if (rc) return rc;
  if (num_classes < 1 || num_classes > SLM_MAX_CLASSES)
    return fail(SLM_ERR_UNSUPPORTED, "slm_bind_data_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)");
  hipStream_t st = (hipStream_t)stream;
  sp->wdev.sf_seg = const_cast<int32_t*>(sf_seg);
  sp->wdev.sf_seg_conf = const_cast<float*>(sf_seg_conf);
  sp->wdev.tgt_seg_conf = const_cast<float*>(tgt_seg_conf);
  sp->wdev.C = num_classes;
  sp->wdev.has = 1;
  HIPCHK(hipMemcpyAsync(s->w_dev + slot, &sp->wdev, sizeof(DataWeightDev), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // (the source is the slot's own mirror, which the next bind rewrites)
  return SLM_OK;
}

int slm_data_weights(slm_solver* s, int32_t slot, double* w_device, void* stream) {
  Slot* sp = nullptr;
  int rc = term_slot("slm_data_weights", s, w_device != nullptr, slot, s && s->weights_on, "slm_enable_data_weights", &sp);
  if (rc) return rc;
  if ((rc = weights_check(s, "slm_data_weights", slot, 1)) != SLM_OK) return rc;
  const FrameDev& h = sp->h;
  const DataWArgs wa{s->w_seg_mode ? s->w_dev.p : nullptr, s->w_pp_max, s->w_seg_mode, 0};
  launch_data_weights(s->frames_dev, slot, h.f.N, h.f.K, s->cfg.w_data, wa, w_device, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

}  // extern "C"
