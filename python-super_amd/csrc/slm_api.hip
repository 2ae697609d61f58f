// slm_api.hip -- the LM solver as a handle of the C ABI (include/super_lm.h): the error channel and the ABI handshake,
// slm_create / slm_destroy with the environment knobs, the getters, setters and diagnostics of a solver, and
// slm_solve_dense.  The bind is slm_bind.hip, the LM step slm_lm.hip; what they share is slm_solver.h.  (The stateless
// entry points of the node feeder are slm_nodes.hip.)
#include <new>
#include <cstdio>

#include "slm_solver.h"

static thread_local std::string g_err;   // what slm_last_error() returns

// every translation unit reports through it (slm_host.h: fail, HIPCHK)
void slm_set_error_text(const char* msg) { g_err = msg; }

std::atomic<long long> g_reallocs{0}, g_realloc_bytes{0}, g_plan_builds{0}, g_plan_reuses{0}, g_plan_fill_hits{0};   // (slm_solver.h)

int check_slots(slm_solver* s, int first, int n) {
  if (!s) return fail(SLM_ERR_INVALID, "null solver");
  if (first < 0 || n < 1 || first + n > (int)s->slots.size())
    return fail(SLM_ERR_INVALID, "slot range out of bounds");
  for (int i = first; i < first + n; ++i) {
    join_prepare(s, i);             // (a queued slm_prepare_model owns the slot until it is done; it leaves it unbound)
    if (!s->slots[i].h.bound) return fail(SLM_ERR_UNBOUND, "slot used before slm_bind_frame");
    // the slots of one launch share their per-surfel kernels, which are instantiated per num_neighbors
    if (s->slots[i].h.f.K != s->slots[first].h.f.K)
      return fail(SLM_ERR_UNSUPPORTED, "the frames of one batch must have the same num_neighbors");
  }
  return SLM_OK;
}

extern "C" {

const char* slm_last_error(void) { return g_err.c_str(); }

int slm_debug_last_solver_form(slm_solver* s) { return s ? s->last_solver_form : -1; }
int slm_debug_last_dag_mode(slm_solver* s) { return s ? s->last_dag_mode : -1; }

int slm_debug_counters(int64_t out[4]) {
  if (!out) return fail(SLM_ERR_INVALID, "slm_debug_counters: null output");
  out[0] = g_reallocs;
  out[1] = g_realloc_bytes;
  out[2] = g_plan_builds;
  out[3] = g_plan_reuses;
  return SLM_OK;
}

int slm_debug_dag_timeout(int64_t ticks) {
  if (ticks < 0) return fail(SLM_ERR_INVALID, "slm_debug_dag_timeout: negative");
  HIPCHK(set_dag_timeout_ticks(ticks == 0 ? 300000000ll : (long long)ticks));
  return SLM_OK;
}

int slm_debug_dag_abort(slm_solver* s, int32_t n_frames, void* stream) {
  int rc = check_slots(s, 0, n_frames);
  if (rc) return rc;
  for (int i = 0; i < n_frames; ++i)
    if (!s->slots[i].h.nd_ready) return fail(SLM_ERR_UNSUPPORTED, "slm_debug_dag_abort: every slot needs a nested-dissection plan");
  hipStream_t st = (hipStream_t)stream;
  launch_dag_abort_check(s->frames_dev, n_frames, st);
  launch_accept(s->frames_dev, n_frames, s->cfg.phase_test, 0, std::max(s->cfg.num_iterations, 1), st);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_debug_dag_trace(slm_solver* s, int32_t slot, int32_t on, void* stream) {
  if (!s || slot < 0 || slot >= (int)s->slots.size()) return fail(SLM_ERR_INVALID, "slm_debug_dag_trace: bad argument");
  Slot& sl = s->slots[slot];
  if (!sl.h.bound || !sl.h.nd_ready) return fail(SLM_ERR_UNBOUND, "slm_debug_dag_trace: no nested-dissection plan bound");
  hipStream_t st = (hipStream_t)stream;
  if (on) {
    HIPCHK(grow(sl.d_dag_trace, (size_t)24 * sl.h.n_dag_tasks + 8));
    HIPCHK(hipMemsetAsync(sl.d_dag_trace, 0, sizeof(long long) * 24 * (size_t)sl.h.n_dag_tasks, st));
  }
  sl.h.dag_trace = on ? sl.d_dag_trace.p : nullptr;
  HIPCHK(hipMemcpyAsync(s->frames_dev + slot, &sl.h, sizeof(FrameDev), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return SLM_OK;
}

int slm_debug_read(slm_solver* s, int32_t slot, int32_t what, double* host_out, int64_t max_doubles,
                   int64_t* n_doubles, void* stream) {
  if (!s || slot < 0 || slot >= (int)s->slots.size() || !n_doubles) return fail(SLM_ERR_INVALID, "slm_debug_read: bad argument");
  const Slot& sl = s->slots[slot];
  if (!sl.h.bound) return fail(SLM_ERR_UNBOUND, "slm_debug_read: slot used before slm_bind_frame");
  const double* src = nullptr;
  int64_t n = 0;
  switch (what) {
    case 0: src = sl.ftiles; n = sl.h.nd_ready ? sl.cache.nd.tile_doubles : 0; break;
    case 1: src = sl.fvec; n = sl.h.nd_ready ? sl.cache.nd.vec_doubles : 0; break;
    case 2: src = sl.flinv; n = sl.h.nd_ready ? sl.cache.nd.linv_doubles : 0; break;
    case 3: src = sl.h.delta; n = sl.h.P; break;
    case 4: src = reinterpret_cast<const double*>(sl.h.dag_trace.get()); n = sl.h.dag_trace ? 24 * (int64_t)sl.h.n_dag_tasks : 0; break;
    case 5: src = reinterpret_cast<const double*>(sl.h.dag_tasks.get()); n = sl.h.nd_ready ? sl.h.n_dag_tasks : 0; break;
    case 6: src = reinterpret_cast<const double*>(sl.h.dag_top_tasks.get()); n = sl.h.nd_ready ? sl.h.n_dag_top_tasks : 0; break;
    default: return fail(SLM_ERR_INVALID, "slm_debug_read: unknown buffer");
  }
  *n_doubles = n;
  const int64_t m = n < max_doubles ? n : max_doubles;
  if (m > 0 && host_out && src) HIPCHK(hipMemcpyAsync(host_out, src, sizeof(double) * m, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return SLM_OK;
}

int slm_debug_read_plan(slm_solver* s, int32_t slot, int32_t what, void* host_out, int64_t max_bytes, int64_t* n_bytes, void* stream) {
  if (!s || slot < 0 || slot >= (int)s->slots.size() || !n_bytes) return fail(SLM_ERR_INVALID, "slm_debug_read_plan: bad argument");
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  const Slot& sl = s->slots[slot];
  const FrameDev& h = sl.h;
  const bool pair = what >= 13 && what <= 16;   // an array of the pair plan (prep_pairs), on a slot of the pair-record form
  if (pair && !h.vk_ready) return fail(SLM_ERR_UNSUPPORTED, "slm_debug_read_plan: the slot has no pair plan");
  if (!pair && !h.v1_ready) return fail(SLM_ERR_UNSUPPORTED, "slm_debug_read_plan: the slot has no tuple-sorted plan");
  const size_t esz = h.f.state_f64 ? 8 : 4;
  const size_t n_wg = (size_t)h.n_pos / 256 + ((h.n_pos % 256) ? 1 : 0);
  const size_t n_slots = (size_t)h.f.K * (h.f.K + 1) / 2;   // canonical pair slots of a surfel
  const bool mesh = sl.face.ready != 0;                     // the bind keyed a face mesh: tri_pidx is the slot's
  const void* src = nullptr;
  size_t n = 0;
  switch (what) {
    case 0: src = h.s_idx.get(); n = sizeof(int32_t) * 4 * (size_t)h.n_pos; break;
    case 1: src = h.grp_run.get(); n = sizeof(int32_t) * (size_t)h.n_pos / 4; break;
    case 2: src = h.run_nodes.get(); n = sizeof(int32_t) * 4 * (size_t)h.n_runs; break;
    case 3: src = h.s_w.get(); n = esz * 4 * (size_t)h.n_pos; break;
    case 4: src = h.blk_key.get(); n = sizeof(int32_t) * (size_t)h.n_blocks; break;
    case 5: src = h.blk_start.get(); n = sizeof(int32_t) * ((size_t)h.n_blocks + 1); break;
    case 6: src = h.blk_entry.get(); n = sizeof(int32_t) * 10 * (size_t)h.n_runs; break;
    case 7: src = h.v2_ready ? h.wg_first.get() : nullptr; n = h.v2_ready ? sizeof(int32_t) * n_wg : 0; break;
    case 8: src = h.v2_ready ? h.wg_last.get() : nullptr; n = h.v2_ready ? sizeof(int32_t) * n_wg : 0; break;
    case 9: src = h.v2_ready ? h.run_lidx.get() : nullptr; n = h.v2_ready ? 10 * (size_t)h.n_runs : 0; break;
    case 10: src = h.v2_ready ? h.blk2_start.get() : nullptr; n = h.v2_ready ? sizeof(int32_t) * ((size_t)h.n_blocks + 1) : 0; break;
    case 11: src = h.v2_ready ? h.blk2_entry.get() : nullptr; n = h.v2_ready ? sizeof(int32_t) * (size_t)h.n_wblk : 0; break;
    case 12: src = h.s_pts.get(); n = esz * 3 * (size_t)h.n_pos; break;
    case 13: src = h.blk_key.get(); n = sizeof(int32_t) * (size_t)h.n_blocks; break;
    case 14: src = h.sf_pidx.get(); n = sizeof(int32_t) * n_slots * (size_t)h.f.N; break;
    case 15: src = h.sf_perm.get(); n = sizeof(int32_t) * (size_t)h.f.N; break;
    case 16: src = mesh ? sl.face.tri_pidx.get() : nullptr; n = mesh ? sizeof(int32_t) * 6 * (size_t)sl.face.n_tri : 0; break;
    default: return fail(SLM_ERR_INVALID, "slm_debug_read_plan: unknown array");
  }
  *n_bytes = (int64_t)n;
  const size_t m = n < (size_t)(max_bytes > 0 ? max_bytes : 0) ? n : (size_t)(max_bytes > 0 ? max_bytes : 0);
  if (m > 0 && host_out && src) HIPCHK(hipMemcpyAsync(host_out, src, m, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return SLM_OK;
}

int slm_abi_version(void) { return SLM_ABI_VERSION; }

int slm_abi_check(int32_t abi_version, int32_t sz_config, int32_t sz_frame, int32_t sz_gf_config, int32_t sz_gf_frame,
                  int32_t sz_iter_record) {
  if (abi_version != SLM_ABI_VERSION || sz_config != (int32_t)sizeof(slm_config) || sz_frame != (int32_t)sizeof(slm_frame) ||
      sz_gf_config != (int32_t)sizeof(slm_gf_config) || sz_gf_frame != (int32_t)sizeof(slm_gf_frame) ||
      sz_iter_record != (int32_t)sizeof(slm_iter_record)) {
    char buf[320];
    snprintf(buf, sizeof(buf),
             "slm_abi_check: caller built for ABI %d (slm_config %d, slm_frame %d, slm_gf_config %d, slm_gf_frame %d, "
             "slm_iter_record %d bytes), library is ABI %d (%zu, %zu, %zu, %zu, %zu)",
             abi_version, sz_config, sz_frame, sz_gf_config, sz_gf_frame, sz_iter_record, SLM_ABI_VERSION, sizeof(slm_config),
             sizeof(slm_frame), sizeof(slm_gf_config), sizeof(slm_gf_frame), sizeof(slm_iter_record));
    return fail(SLM_ERR_INVALID, buf);
  }
  return SLM_OK;
}

int slm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int slm_create(const slm_config* cfg, slm_solver** out) {
  if (!cfg || !out) return fail(SLM_ERR_INVALID, "slm_create: null argument");
  if (cfg->max_frames < 1 || cfg->num_iterations < 0 || !(cfg->v > 0.0))
    return fail(SLM_ERR_INVALID, "slm_create: bad config");
  if (cfg->solver_path < 0 || cfg->solver_path > 4) return fail(SLM_ERR_INVALID, "slm_create: solver_path must be 0..4");
  if (cfg->data_path < 0 || cfg->data_path > 2) return fail(SLM_ERR_INVALID, "slm_create: data_path must be 0..2");
  if (slm_device_count() < 1) return fail(SLM_ERR_NO_DEVICE, "slm_create: no HIP device visible");
  slm_solver* s = new (std::nothrow) slm_solver();
  if (!s) return fail(SLM_ERR_HIP, "slm_create: out of host memory");
  s->cfg = *cfg;
  try {
    s->slots.resize(cfg->max_frames);
  } catch (...) {
    delete s;
    return fail(SLM_ERR_HIP, "slm_create: out of host memory");
  }
  const size_t n_slots = (size_t)cfg->max_frames;
  hipError_t e = s->frames_dev.grow(n_slots, n_slots);
  if (e == hipSuccess) e = hipMemset(s->frames_dev, 0, sizeof(FrameDev) * n_slots);
  if (e == hipSuccess) e = s->bw_dev.grow(2, 2);   // {half-bandwidth, bad KNN table}
  if (e == hipSuccess) e = s->reuse_dev.grow(n_slots, n_slots);
  if (e == hipSuccess) e = hipMemset(s->reuse_dev, 0, sizeof(int) * n_slots);
  if (e == hipSuccess) e = s->bw_host.grow(2, 2);
  if (e == hipSuccess) {
    s->prep = prep_create();
    if (!s->prep) e = hipErrorOutOfMemory;
  }
  if (e != hipSuccess) {
    g_err = std::string("slm_create: ") + hipGetErrorString(e);
    slm_destroy(s);
    return SLM_ERR_HIP;
  }
  {   // per-device set-up of the task-graph launch (LDS attribute, workgroup count, XCD probe): here, not inside an LM iteration
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)dag_device_setup(dev, nullptr);
  }
  if (const char* hb = getenv("SLM_HYBRID")) s->hybrid_batches = atoi(hb) != 0;   // experiments
  if (const char* dm = getenv("SLM_DAG_MAX_NODES")) s->dag_max_nodes = atol(dm);   // experiments / tests
  if (const char* nr = getenv("SLM_NO_REUSE")) s->no_reuse = atoi(nr) != 0;       // tests: recompute after a reject
  if (const char* pf = getenv("SLM_PURE_FILL")) s->pure_fill = atoi(pf) != 0;     // tests: differential check of the pure-fill tiles
  if (const char* fb = getenv("SLM_FUSE_BEGIN")) s->fuse_begin = atoi(fb) != 0;   // A/B: the zeroing as a launch of its own
  if (const char* gw = getenv("SLM_GRAM_WGS")) s->gram_wgs = std::min(std::max(atoi(gw), 0), 65535);   // A/B, tests
  {
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) s->n_cus = cus;
  }
  *out = s;
  return SLM_OK;
}

int slm_destroy(slm_solver* s) {
  if (!s) return SLM_OK;
  // Both pools first, whatever the order of the members: queued jobs reference the slots (the worker runs what is
  // still queued).
  s->prep_worker.shutdown();
  s->bind_pool.shutdown();
  for (Slot& sl : s->slots) {   // what a slot holds beside its DevBuf / PinnedBuf members
    plan_free(sl.plan);
    pairplan_free(sl.pplan);
    sem_free(sl.morph_edges);
    if (sl.prep_fork) (void)hipEventDestroy(sl.prep_fork);
    if (sl.prep_done) (void)hipEventDestroy(sl.prep_done);
  }
  s->slots.clear();   // the slots' buffers first: hipFree waits for the device, so the streams and events below are idle
  prep_destroy(s->prep);
  prep_destroy(s->prep_async);
  if (s->prep_stream) (void)hipStreamDestroy(s->prep_stream);
  for (PrepBuffers* pb : s->bind_prep) prep_destroy(pb);
  for (hipStream_t q : s->bind_streams) (void)hipStreamDestroy(q);
  for (hipEvent_t e : s->bind_events) (void)hipEventDestroy(e);
  for (auto& evs : s->ev_runs)
    for (hipEvent_t e : evs)
      if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : s->ev_pool) (void)hipEventDestroy(e);
  if (s->drain_event) (void)hipEventDestroy(s->drain_event);
  delete s;   // (the solver's own arrays: frames_dev, bw_dev, bw_host, reuse_dev, corr_dev, face_dev, morph_dev)
  return SLM_OK;
}

int slm_get_plan_info(slm_solver* s, int32_t slot, double* out_caller, int32_t capacity) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  if (!out_caller || capacity < 0) return fail(SLM_ERR_INVALID, "slm_get_plan_info: bad output");
  const Slot& sl = s->slots[slot];
  const FrameDev& h = sl.h;
  double out[SLM_PLAN_INFO_DOUBLES];
  for (int i = 0; i < SLM_PLAN_INFO_DOUBLES; ++i) out[i] = 0.0;
  if (h.nd_ready) {
    out[0] = 0.0;
    out[1] = (double)sl.cache.nd.fronts.size();
    out[2] = (double)sl.cache.nd.level_start.size() - 1.0;
    out[3] = sl.cache.nd.flops;
    out[10] = sl.cache.nd.flops_exact;
    out[11] = (double)sl.cache.nd.dag_tasks.size() / 2.0;
    out[4] = 8.0 * (double)sl.cache.nd.tile_doubles;
    out[12] = (double)sl.n_piv_tiles;
    out[13] = (double)sl.n_pure_tiles;
  } else {
    out[0] = 1.0;
    const double w = (double)h.wb * SLM_NB;
    out[3] = (double)h.P * w * w;
    out[4] = 8.0 * (double)h.nt * (h.wb + 1) * SLM_NB * SLM_NB;
  }
  out[5] = h.n_tuples;
  out[6] = h.n_runs;
  out[7] = h.n_blocks;
  out[8] = h.v1_ready && h.v2_ready ? h.n_wblk : 0;
  out[9] = h.n_pos;
  out[14] = h.v1_ready ? sl.prep_kind : 0;
  out[15] = h.v1_ready ? sl.prep_max_bin : 0;
  for (int i = 0; i < capacity; ++i) out_caller[i] = i < SLM_PLAN_INFO_DOUBLES ? out[i] : 0.0;
  return SLM_OK;
}

int slm_profile_enable(slm_solver* s, int32_t on) {
  if (!s) return fail(SLM_ERR_INVALID, "slm_profile_enable: null solver");
  s->profile = on != 0;
  return SLM_OK;
}

int slm_profile_read(slm_solver* s, double* ms_out, int64_t* count_out) {
  if (!s || !ms_out || !count_out) return fail(SLM_ERR_INVALID, "slm_profile_read: null argument");
  for (int p = 0; p < SLM_PH_COUNT; ++p) {
    ms_out[p] = 0.0;
    count_out[p] = 0;
  }
  for (size_t r = 0; r < s->ev_runs.size(); ++r) {
    auto& evs = s->ev_runs[r];
    if ((int)evs.size() == SLM_PH_COUNT + 1 && evs.back()) {
      HIPCHK(hipEventSynchronize(evs.back()));
      for (int p = 0; p < SLM_PH_COUNT; ++p) {
        if (!evs[p] || !evs[p + 1]) continue;
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, evs[p], evs[p + 1]));
        ms_out[p] += ms;
        count_out[p] += 1;
      }
    }
    for (hipEvent_t e : evs)
      if (e) s->ev_pool.push_back(e);
  }
  s->ev_runs.clear();
  return SLM_OK;
}

int slm_get_beta(slm_solver* s, int32_t slot, double* out, void* stream) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  if (!out) return fail(SLM_ERR_INVALID, "slm_get_beta: null output");
  const FrameDev& h = s->slots[slot].h;
  HIPCHK(hipMemcpyAsync(out, h.beta, sizeof(double) * h.P, hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  return SLM_OK;
}

int slm_set_beta(slm_solver* s, int32_t slot, const double* in, void* stream) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  if (!in) return fail(SLM_ERR_INVALID, "slm_set_beta: null input");
  const FrameDev& h = s->slots[slot].h;
  hipStream_t st = (hipStream_t)stream;
  // fresh LM state (u0, minimal_loss0, records), then the caller's beta
  launch_init_slot(s->frames_dev, slot, h.f.J, s->cfg, st);
  HIPCHK(hipMemsetAsync(s->reuse_dev + slot, 0, sizeof(int), st));   // another beta: the kept records do not apply
  HIPCHK(hipMemcpyAsync(h.beta, in, sizeof(double) * h.P, hipMemcpyDeviceToDevice, st));
  launch_pack_nodes(s->frames_dev, slot, h.f.J, st);
  return SLM_OK;
}

int slm_get_records(slm_solver* s, int32_t slot, slm_iter_record* host_out, int32_t max_records,
                    void* stream) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  if (!host_out || max_records < 0) return fail(SLM_ERR_INVALID, "slm_get_records: bad output");
  int n = std::min(max_records, s->cfg.num_iterations);
  hipStream_t st = (hipStream_t)stream;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(host_out, s->slots[slot].h.rec, sizeof(slm_iter_record) * n,
                          hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
#ifdef SLM_STAMPS
  if (s->slots[slot].h.dbg) {
    unsigned long long t[64];
    HIPCHK(hipMemcpy(t, s->slots[slot].h.dbg, sizeof(t), hipMemcpyDeviceToHost));
    fprintf(stderr, "[slm stamps slot %d] deltas (cycles):", slot);
    for (int i = 1; i < 16; ++i) fprintf(stderr, " %d:%lld", i, t[i] ? (long long)(t[i] - t[i - 1]) : -1LL);
    fprintf(stderr, "\n");
  }
#endif
  return SLM_OK;
}

int slm_solve_dense(int32_t P, const double* A, const double* b, double* x, int32_t* status,
                    void* stream) {
  if (P < 1 || !A || !b || !x) return fail(SLM_ERR_INVALID, "slm_solve_dense: bad argument");
  hipStream_t st = (hipStream_t)stream;
  FrameDev h{};
  h.P = P;
  h.nt = (P + SLM_NB - 1) / SLM_NB;
  h.wb = h.nt - 1;
  h.bound = 1;
  const size_t nvec = (size_t)h.nt * SLM_NB;
  const size_t nband = (size_t)h.nt * (h.wb + 1) * SLM_NB * SLM_NB;
  const size_t nlinv = (size_t)h.nt * SLM_NB * SLM_NB;
  char* ws = nullptr;
  const size_t bytes = sizeof(double) * (2 * nvec + nband + nlinv) + sizeof(LMState) + sizeof(FrameDev);
  HIPCHK(hipMalloc((void**)&ws, bytes));
  double* p = reinterpret_cast<double*>(ws);
  h.delta = p;
  h.rhs = p + nvec;
  h.band = p + 2 * nvec;
  h.linv = h.band + nband;
  h.st = reinterpret_cast<LMState*>(h.linv + nlinv);
  FrameDev* fdev = reinterpret_cast<FrameDev*>(h.st + 1);
  int rc = SLM_OK;
  hipError_t e = hipMemsetAsync(h.st, 0, sizeof(LMState), st);
  if (e == hipSuccess) e = hipMemcpyAsync(fdev, &h, sizeof(FrameDev), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    launch_dense_to_band(fdev, A, b, st);
    launch_band_solve(fdev, 1, h.nt, h.wb, 0.0, st);
    e = hipMemcpyAsync(x, h.delta, sizeof(double) * P, hipMemcpyDeviceToDevice, st);
  }
  if (e == hipSuccess && status)
    e = hipMemcpyAsync(status, &h.st->chol_fail, sizeof(int32_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    g_err = std::string("slm_solve_dense: ") + hipGetErrorString(e);
    rc = SLM_ERR_HIP;
  }
  (void)hipFree(ws);
  return rc;
}

int slm_data_residuals(slm_solver* s, int32_t slot, double* r, uint8_t* match, int32_t* taps,
                       void* stream) {
  int rc = check_slots(s, slot, 1);
  if (rc) return rc;
  const FrameDev& h = s->slots[slot].h;
  launch_data_resid(s->frames_dev, slot, h.f.N, h.f.K, s->cfg.w_data, r, match, taps, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

}  // extern "C"
