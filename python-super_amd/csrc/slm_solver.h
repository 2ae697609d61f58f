// slm_solver.h -- internal to the LM host (slm_api.hip, slm_bind.hip, slm_lm.hip, slm_terms.hip): what a solver and its slots
// hold, where the loss partials of its terms sit (LossParts), and the few functions that cross those units.  Device memory
// is owned by DevBuf / PinnedBuf members (slm_host.h); the descriptors (FrameDev, CorrDev, FaceDev, MorphDev, DataWeightDev)
// only mirror addresses.
#pragma once
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "slm_common.h"
#include "slm_corr.h"
#include "slm_data.h"
#include "slm_face.h"
#include "slm_host.h"
#include "slm_launch.h"
#include "slm_morph.h"
#include "slm_prep.h"
#include "slm_sem.h"
#include "slm_workers.h"

constexpr int kLossBlocks = 512;   // data-loss partial sums per slot
constexpr int kRegBlocksMax = 64;
// loss partials of the terms per slot (LossParts)
constexpr int kCorrBlocks = SLM_CORR_BLOCKS, kFaceBlocks = SLM_FACE_BLOCKS, kMorphBlocks = SLM_MORPH_BLOCKS;

// The form of the data term: which plan the bind prepares and which kernels the LM entry points launch.
enum class DataForm {
  none,        // no data term (use_data 0) or no surfels
  tuple,       // num_neighbors 4: tuple-sorted positions, k_data_eval + k_data_gram, then k_front_assemble / k_band_assemble
  pairs,       // any other num_neighbors on the multifrontal solver: k_data_grad_pairs into per-pair records, k_pair_scatter
  per_entry,   // data_path 1, J >= 65 536, a K-generic frame on the block-banded solver: k_data_grad<K>'s atomics
};

// The symbolic-plan cache of a slot.  Surfels that appear / disappear change the pair list a little from frame to frame:
// the plan covers the union of the lists seen since the node graph last changed, and a frame whose pairs are all in it only
// needs its own pair -> destination table (a merge of two sorted lists), not a new symbolic analysis (1.7 ms at C2).
struct PlanCache {
  NDPlanHost nd;
  bool valid = false;           // nd is complete and the device holds it
  uint64_t knn_hash = 0;        // hash of (J, K_ED, node KNN) nd was built for
  uint64_t frame_hash = 0;      // hash of the coupled-pair list + node KNN of the frame bound last ...
  int frame_blocks = -1;        // ... and its pair count: the frame the device's destination table and tile kinds are for
  std::vector<NDDest> frame_dest;   // destinations of that frame's pairs
  void frame_stale() { frame_hash = 0; frame_blocks = -1; }   // the per-frame device mirrors are not to be trusted; the plan's are
  void drop_plan() { valid = false; nd.plan_pairs.clear(); frame_stale(); }   // nothing of the plan applies any more
};

struct Slot {
  FrameDev h{};                 // host mirror of the device descriptor: addresses of the buffers below, none owned
  // state and work vectors at the frame's sizes (grow-only; loss_part, st, rec and dbg have one size for good)
  DevBuf<double> beta, delta, rhs, node_pk, loss_part;
  DevBuf<LMState> st;
  DevBuf<slm_iter_record> rec;
  DevBuf<unsigned long long> dbg;   // diagnostic builds only (-DSLM_STAMPS)
  DevBuf<float4> tgt_pn, tgt_px;    // packed target tables
  DevBuf<double> ev_rc;             // evaluation buffer {r, c} per position of the tuple-sorted plan
  V1Plan plan;                  // tuple-sorted assembly buffers (grow-only)
  CorrDev corr{};               // correspondence term: host mirror of the slot's targets, which are
  DevBuf<double> corr_o, corr_n;
  DevBuf<uint8_t> corr_valid;
  FaceDev face{};               // face term: host mirror of the slot's mesh descriptor; the mesh itself is the slot's own copy
  DevBuf<int32_t> face_tri;
  DevBuf<double> face_areas;
  PinnedBuf<FaceDev> face_pin;  // pinned mirror of `face` for the asynchronous upload of a bind
  MorphDev morph{};             // boundary-morph term: host mirror of the slot's descriptor (the caller's semantic inputs, none
  SemScratch morph_edges;       // owned), the slot's own boundary lists (slm_bind_morph; released by slm_destroy) and the
                                // arrays every selection rewrites
  DevBuf<uint8_t> morph_kept;
  DevBuf<double> morph_target, morph_li, morph_part, morph_stat;
  DataWeightDev wdev{};         // data weights: host mirror of the slot's semantic inputs (the caller's arrays, none owned)
  PairPlan pplan;               // K-generic pair path (num_neighbors != 4): pair keys, per-surfel pair indices, surfel order
  PlanCache cache;              // nested-dissection plan: host copy; its device mirrors below (grow-only)
  DevBuf<NDDest> d_cur_dests;   // PlanCache::frame_dest on the device
  PinnedBuf<uint32_t> h_pairs;   // read-backs of the bind (pinned)
  PinnedBuf<int32_t> h_knn;
  PinnedBuf<float> h_pts;
  PinnedBuf<double> h_pts64;
  PinnedBuf<FrameDev> h_pin;       // pinned mirror of `h` for the asynchronous descriptor upload of a bind
  DevBuf<NDFront> d_fronts;
  DevBuf<NDTileItem> d_items;      // work lists of the pull-form kernels
  DevBuf<uint8_t> d_tile_kind;     // FrameDev::tile_kind / zero_tiles (slm_common.h): per tile 1 = pure fill; the tiles to zero
  DevBuf<long long> d_zero_tiles;
  int n_piv_tiles = 0, n_pure_tiles = 0;  // pivot-column tiles of the plan / of them pure fill (slm_get_plan_info)
  int prep_kind = 0, prep_max_bin = 0;    // the preparation that built the tuple-sorted plan (V1Sizes), its largest bin (slm_get_plan_info)
  std::vector<uint8_t> h_tile_kind;      // host sources of the two uploads (kept: the copies are asynchronous)
  std::vector<long long> h_zero_tiles;
  DevBuf<int32_t> d_ints;          // the plan's int32 arrays, one behind the other (kPlanInts)
  DevBuf<long long> d_dag_trace;   // diagnostics
  DevBuf<int32_t> d_dag_flags;     // persistent task-graph solver: ticket, counters, per-tile / per-column flags
  DevBuf<NDDest> d_dests;          // block_dest | pair_dest
  DevBuf<double> ftiles, fvec, flinv, fmail;
  DevBuf<double> pairbuf;          // sharded frames: per-pair sums to exchange
  DevBuf<double> band, linv;       // block-banded path (allocated on demand)
  bool band_ready = false;
  // slm_prepare_model: the model-side half of a bind, done ahead of the frame's target (possibly still running on the
  // solver's worker thread: prep_ticket)
  bool model_ready = false;        // the model part below is complete and valid for prep_model
  slm_frame prep_model{};          // the model fields it was prepared for
  unsigned long long prep_ticket = 0;   // job number on the worker (0: none pending)
  int prep_rc = SLM_OK;
  bool prep_recorded = false;      // prep_done was recorded on the solver's stream and nothing has waited for it yet
  std::string prep_err;
  hipEvent_t prep_fork = nullptr, prep_done = nullptr;
};

struct slm_solver {
  PrepBuffers* prep = nullptr;
  BindPool bind_pool;
  // slm_prepare_model: worker thread, its stream and scratch buffers
  AsyncWorker prep_worker;
  PrepBuffers* prep_async = nullptr;
  hipStream_t prep_stream = nullptr;
  // slm_bind_frames: one worker (scratch buffers + stream + events) per frame bound concurrently
  std::vector<PrepBuffers*> bind_prep;
  std::vector<hipStream_t> bind_streams;
  std::vector<hipEvent_t> bind_events;
  std::mutex band_mutex;        // the bandwidth read-back buffer of ensure_band is shared
  hipEvent_t drain_event = nullptr;   // slm_bind_frames' wait for the caller's stream (polled, see there)
  double drain_est_ms = 0.0;          // how long that wait took last time
  int last_solver_form = -1;    // diagnostics: 0 per-level launches, 1 task graph, 2 hybrid (slm_debug_last_solver_form)
  int last_dag_mode = -1;       // diagnostics: mode word of the last task-graph launch (bit 0: XCD-affine), -1 none (slm_debug_last_dag_mode)
  bool no_reuse = false;        // SLM_NO_REUSE=1 (tests): every Jacobian pass recomputes its records, also after a reject
  bool hybrid_batches = true;   // solver_path 0, larger batches: per-level launches + task graph for the top levels
  long dag_max_nodes = 8000;    // solver_path 0: launches of at most this many frames x nodes run as ONE task graph (SLM_DAG_MAX_NODES)
  bool fuse_begin = true;       // SLM_FUSE_BEGIN=0 (A/B, tests): k_iter_begin_nd as a launch of its own in front of the Jacobian pass, as in rounds 1-5
  int gram_wgs = 0;             // SLM_GRAM_WGS (A/B, tests): workgroups per slot of the resident Jacobian pass; 0: one residency over the batch
  int n_cus = 256;              // compute units of the device (sizes that residency)
  bool pure_fill = true;        // SLM_PURE_FILL=0 (tests): every pivot-column tile is zeroed and read-modify-written, as in rounds 1-4
  bool profile = false;
  std::vector<hipEvent_t> ev_pool;            // recycled events
  std::vector<std::vector<hipEvent_t>> ev_runs;  // per recorded iteration: SLM_PH_COUNT+1 events
  slm_config cfg{};
  std::vector<Slot> slots;
  DevBuf<FrameDev> frames_dev;
  DevBuf<int> bw_dev;
  PinnedBuf<int> bw_host;
  DevBuf<int> reuse_dev;        // per slot: 1 after a rejected iteration -- the next Jacobian pass of the LM loop reuses the
                                // records of the last one (k_accept writes, k_data_gram / k_iter_begin_nd read)
  int rank = 0, world = 1;      // surfel sharding of every frame (slm_set_shard)
  int corr_mode = 0;            // slm_enable_corr: 0 off, 1 point-point, 2 point-plane; its weight; the slots' targets on the device
  double corr_w = 0.0;
  DevBuf<CorrDev> corr_dev;
  bool weights_on = false;      // slm_enable_data_weights: seg_mode != 0 or pp_max > 0; the slots' semantic inputs on the device
  int w_seg_mode = 0;
  double w_pp_max = 0.0;
  DevBuf<DataWeightDev> w_dev;
  bool face_on = false;         // slm_enable_face with a non-zero weight; its weight; the slots' meshes on the device
  double face_w = 0.0;
  DevBuf<FaceDev> face_dev;
  bool morph_on = false;        // slm_enable_morph with a non-zero weight; its weight; the slots' inputs on the device
  double morph_w = 0.0;
  DevBuf<MorphDev> morph_dev;
  bool shard_mode = false;      // slm_set_shard was called (world == 1 included): slots carry the exchange buffers
};

// Where the terms' loss partials sit in a slot's loss_part: every offset in doubles from the start of the regularisers'
// partials (loss_part + 2 n_loss_part).  An LM launch packs its {sum, 0} pairs -- the n_reg_part of the regularisers, then
// the correspondence term's kCorrBlocks, then the face term's kFaceBlocks, then the boundary-morph term's kMorphBlocks, each
// only on a solver with the term enabled -- so that k_accept sums them as n_acc_part pairs.  A direct call (slm_corr_loss,
// slm_face_loss) stores its pairs at a fixed place behind kRegBlocksMax pairs (any place among the pairs would do: every LM
// iteration rewrites its own).  The correspondence term's kept counts sit behind every pair; only a solver with the face
// term has room for that term's pairs, its counts sit that much further back and its slots' loss_part is that much longer;
// the boundary-morph term's pair likewise (a direct call of that term writes its caller's array, no pair).
struct LossParts {
  int corr, face, morph;           // the terms' pairs of an LM launch
  int corr_direct, face_direct;    // ... of a direct call
  int corr_cnt;                    // the correspondence term's kCorrBlocks kept counts
  int n_acc_part;                  // pairs k_accept sums behind the data partials
  size_t doubles;                  // of a slot's loss_part (kLossBlocks data pairs in front)
};
inline LossParts loss_parts(const slm_solver* s, int n_reg_part) {
  LossParts p;
  p.corr = 2 * n_reg_part;
  p.n_acc_part = n_reg_part + (s->corr_mode ? kCorrBlocks : 0);
  p.face = 2 * p.n_acc_part;
  if (s->face_on) p.n_acc_part += kFaceBlocks;
  p.morph = 2 * p.n_acc_part;
  if (s->morph_on) p.n_acc_part += kMorphBlocks;
  p.corr_direct = 2 * kRegBlocksMax;
  p.face_direct = p.corr_direct + 2 * kCorrBlocks;
  p.corr_cnt = p.face_direct + (s->face_on ? 2 * kFaceBlocks : 0) + (s->morph_on ? 2 * kMorphBlocks : 0);
  p.doubles = (size_t)2 * kLossBlocks + p.corr_cnt + kCorrBlocks;
  return p;
}

// diagnostics (slm_debug_counters, slm_api.hip): device reallocations and symbolic analyses since the library was loaded
extern std::atomic<long long> g_reallocs, g_realloc_bytes, g_plan_builds, g_plan_reuses, g_plan_fill_hits;   // (binds may run on worker threads)

// The solver's form of DevBuf::grow: 12 % of head-room, and every growth counts into slm_debug_counters.
template <typename T>
hipError_t grow(DevBuf<T>& b, size_t need) {
  if (need <= b.cap) return hipSuccess;
  const size_t want = need + need / 8;
  ++g_reallocs;
  g_realloc_bytes += (long long)(want * sizeof(T));
  return b.grow(need, want);
}

// What crosses the four units (hidden: the library's dynamic symbols stay the C ABI and what they were).
#pragma GCC visibility push(hidden)
// slm_api.hip: the slots [first, first + n) are bound and may share a launch (waits for their queued preparations)
int check_slots(slm_solver* s, int first, int n);
// slm_bind.hip: waits for the slot's queued slm_prepare_model; the block-banded storage of a slot on demand
void join_prepare(slm_solver* s, int slot);
int ensure_band(slm_solver* s, int slot, hipStream_t st);
// slm_lm.hip: which form of the solver a launch of n frames of J nodes takes (the bind sizes the plan's leaves by it);
// the stopped flag and counters of a slot cleared ahead of a parity entry point; with a semantic weight on, every slot of
// [first, first + n) has its semantic inputs (fn: the refused entry point's name)
bool solve_is_task_graph(const slm_solver* s, int n, int J);
int clear_flags(slm_solver* s, int slot, hipStream_t st);
int weights_check(const slm_solver* s, const char* fn, int first, int n);
#pragma GCC visibility pop
