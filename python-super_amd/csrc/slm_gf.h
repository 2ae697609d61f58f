// slm_gf.h -- state shared by the GraphFit kernels (slm_gf.hip) and the Semantic-SuPer
// kernels (slm_sem.hip): the spread block partials and their one fold, the slot descriptor, the skinning sum.
#pragma once
#include "slm_data.h"

// Block partials of the per-slot scalars (the global row's gradient, the loss terms, the counts) go to GF_NCOPY spread copies
// behind `terms` -- copy (blockIdx.x % GF_NCOPY), entry a: gf_part(s, copy)[a] -- and k_gf_fold / k_gf_step sum the copies in a
// fixed order (gf_part_fold) into grad[7J..] / terms[].  One global f64 atomic per block and scalar onto ONE address serialises
// in the L2: 782 blocks x ~0.1 us = the whole 82 us of k_gf_data at C2 (round 6); spread over 64 addresses it is 12 per address.
#define GF_NCOPY 64
enum GfPart {
  GFP_GLOBAL = 0,                        // 0..6 the global row's gradient (k_gf_data, k_gf_reg)
  GFP_PP_LOSS = 7, GFP_PP_KEPT = 8,      // point-plane loss, residuals kept (k_gf_data)
  GFP_CORR_LOSS = 9, GFP_CORR_KEPT = 10, // flow-correspondence loss, residuals kept (k_gf_data)
  GFP_FACE = 11, GFP_ARAP = 12, GFP_ROT = 13,   // the node terms (gf_reg_body)
  GFP_MORPH_SUM = 14, GFP_MORPH_KEPT = 15,      // morphing sum, kept (k_gf_morph)
  GF_NPART = 16
};
#define GF_PART_DOUBLES (GF_NPART * GF_NCOPY)
// which of the partials a launch folds: k_gf_fold's `which`
enum GfFoldWhich { GF_FOLD_DATA = 1,     // the entries of k_gf_data / k_gf_reg (0..13)
                   GF_FOLD_MORPH = 2,    // those of k_gf_morph (14, 15)
                   GF_FOLD_DROP_MORPH = 4 };   // terms[5..7] = 0: a sharded rank other than 0 behind its back-propagation -- the
                                               // entries hold the GLOBAL sum, count and flag since the first exchange, and the
                                               // second exchange sums the whole block again (rank 0 alone keeps them)
// k_gf_step's `fold` (see there)
enum GfStepFold { GF_STEP_FOLD = 1,      // it sums the partials of k_gf_data / k_gf_reg itself (no k_gf_fold launch)
                  GF_STEP_OWN = 2,       // it owns them: clears what it summed and ASSIGNS the loss terms
                  GF_STEP_REZERO = 4,    // it leaves the gradient zeroed for the next iteration
                  GF_STEP_MORPH = 8 };   // it also owns the morphing term's partials

struct GfSlot {
  slm_gf_frame f;
  int32_t bound;
  int32_t step;          // optimiser steps done
  int32_t shard_lo, shard_hi;   // surfels [lo,hi) are evaluated by this rank (slm_gf_set_shard)
  double* dv;            // (J+1,7)
  double* grad;          // (J+1,7)
  double* m1;            // momentum buffer / Adam exp_avg
  double* m2;            // Adam exp_avg_sq
  double* terms;         // [0..3] face, arap, rot, point-plane; [4] residuals kept;
                         // [5] morphing loss sum (weighted mean after k_gf_finish), [6] kept, [7] candidates;
                         // [8] flow-correspondence loss, [9] its residuals kept   (SLM_GF_NTERMS)
  const float* flow;     // (2,H,W) optical flow of the frame (slm_gf_bind_flow) or null
  // ---- Semantic-SuPer (slm_gf_bind_semantic) ----
  slm_gf_semantic sem;
  int32_t sem_bound;
  int32_t edge_off[SLM_MAX_CLASSES + 1];   // class c owns edge_xy[edge_off[c] .. edge_off[c+1])
  float2* edge_xy;       // boundary pixels (x,y), per class, row-major pixel order
  double2* morph_g;      // (N) d(loss_i)/d(x,y) of the morphing term, 0 when not kept
};

// GfSlot as DEVICE code reads it: the same bytes, every pointer typed GP<> (global address space, slm_common.h) so that
// the kernels issue global_load / global_store instead of FLAT accesses.  Host code keeps using GfSlot.
struct GfFrameIn {
  FrameIn base;
  GP<const uint8_t> sf_stable;
  GP<const void> ed_knn_w;
  GP<const int32_t> ed_triangles;
  GP<const void> ed_triangle_areas;
  int32_t n_triangles;
  int32_t pad;
};
struct GfSemIn {
  int32_t num_classes;
  int32_t pad;
  GP<const int32_t> sf_seg;
  GP<const float> sf_seg_conf;
  GP<const float> tgt_seg_conf;
  GP<const float> img_seg_conf;
  GP<const int32_t> img_seg;
};
struct GfSlotDev {
  GfFrameIn f;
  int32_t bound;
  int32_t step;
  int32_t shard_lo, shard_hi;
  GP<double> dv;
  GP<double> grad;
  GP<double> m1;
  GP<double> m2;
  GP<double> terms;
  GP<const float> flow;
  GfSemIn sem;
  int32_t sem_bound;
  int32_t edge_off[SLM_MAX_CLASSES + 1];
  GP<float2> edge_xy;
  GP<double2> morph_g;
};
static_assert(sizeof(GfFrameIn) == sizeof(slm_gf_frame) && sizeof(GfSemIn) == sizeof(slm_gf_semantic) &&
              sizeof(GfSlotDev) == sizeof(GfSlot), "GfSlotDev mirrors GfSlot");
static_assert(offsetof(GfSlotDev, dv) == offsetof(GfSlot, dv) && offsetof(GfSlotDev, flow) == offsetof(GfSlot, flow) &&
              offsetof(GfSlotDev, sem) == offsetof(GfSlot, sem) && offsetof(GfSlotDev, edge_xy) == offsetof(GfSlot, edge_xy) &&
              offsetof(GfSlotDev, morph_g) == offsetof(GfSlot, morph_g) && offsetof(GfFrameIn, ed_triangle_areas) == offsetof(slm_gf_frame, ed_triangle_areas) &&
              offsetof(GfSemIn, img_seg) == offsetof(slm_gf_semantic, img_seg), "GfSlotDev mirrors GfSlot");
__device__ __forceinline__ GfSlotDev* gf_dev(GfSlot* slots) { return reinterpret_cast<GfSlotDev*>(slots); }

// R(q)^T c for an un-normalised quaternion = R(conj q) c
__device__ __forceinline__ d3 quat_apply_t(double w, d3 v, d3 c) {
  return quat_apply(w, {-v.x, -v.y, -v.z}, c);
}

// entry a of the partials -> the index in terms[] it is summed into (-1: the global row, grad[7J + a])
__device__ __forceinline__ int gf_part_term(int a) {
  constexpr int map[GF_NPART] = {-1, -1, -1, -1, -1, -1, -1, 3, 4, 8, 9, 0, 1, 2, 5, 6};
  return map[a];
}
// the spread copy of the partials a block adds to
__device__ __forceinline__ double* gf_part(GfSlotDev& s, int copy) { return s.terms.get() + SLM_GF_NTERMS + GF_NPART * copy; }
// sum of the GF_NCOPY copies of entry a, in copy order; clear: the caller owns the partials and leaves them zeroed
__device__ __forceinline__ double gf_part_fold(GfSlotDev& s, int a, bool clear) {
  double* part = gf_part(s, 0);
  double t = 0.0;
  for (int c = 0; c < GF_NCOPY; ++c) {
    t += part[GF_NPART * c + a];
    if (clear) part[GF_NPART * c + a] = 0.0;
  }
  return t;
}

// deformed surfel i: T(p) = sum_k w_k [R(q_k)(p-g_k) + b_k + g_k], P = R(q_g) T + b_g
// (deform_source, super/deform_mesh.py:198-221; K-generic like the reference: KK = opt.num_neighbors, 1..8)
// The sum is written once: gf_skin_add is one neighbour's term, gf_skin_global the global row; gf_skin<KK> (K at compile
// time) and gf_skin_pos (K at run time) walk the neighbours in list order through them.
__device__ __forceinline__ void gf_skin_add(const GfSlotDev& s, const d3 p, const int id, const double w, d3& T) {
  const FrameIn& f = s.f.base;
  const double* b = s.dv + 7 * id;
  const d3 g = ld_state3(f.ed_points, (size_t)id, f.state_f64);
  d3 t = quat_apply(b[0], {b[1], b[2], b[3]}, p - g);
  t = {t.x + b[4] + g.x, t.y + b[5] + g.y, t.z + b[6] + g.z};
  T = {T.x + w * t.x, T.y + w * t.y, T.z + w * t.z};
}
__device__ __forceinline__ d3 gf_skin_global(const GfSlotDev& s, const d3 T, double& gw, d3& gv) {
  const double* bgl = s.dv + 7 * s.f.base.J;
  gw = bgl[0];
  gv = {bgl[1], bgl[2], bgl[3]};
  const d3 P = quat_apply(gw, gv, T);
  return {P.x + bgl[4], P.y + bgl[5], P.z + bgl[6]};
}

// What a surfel's evaluation keeps: ids, weights, p, T, P and the global row -- no per-neighbour state.  k_gf_data holds THIS
// across its sampling phase (26 + 3 K registers) and re-reads the nodes -- cache hits -- when it back-propagates: with the
// rotations and offsets of every neighbour held live (30 + 17 K) the kernel needed more than 256 VGPRs and ran at ONE wave
// per SIMD (round 6).
template <int KK>
struct GfSkin {
  int id[KK];
  double w[KK];
  d3 p, T, P;
  double gw;
  d3 gv;
};
template <int KK>
__device__ __forceinline__ void gf_skin(const GfSlotDev& s, int i, GfSkin<KK>& k) {
  const FrameIn& f = s.f.base;
  k.p = ld_state3(f.sf_points, (size_t)i, f.state_f64);
  if constexpr (KK == SLM_K) {
    const int4 ids = *reinterpret_cast<const int4*>(f.sf_knn_idx + 4 * (size_t)i);
    k.id[0] = ids.x; k.id[1] = ids.y; k.id[2] = ids.z; k.id[3] = ids.w;
    ld_state4(f.sf_knn_w, (size_t)i, f.state_f64, k.w);
  } else {
#pragma unroll
    for (int a = 0; a < KK; ++a) {
      k.id[a] = f.sf_knn_idx[(size_t)KK * i + a];
      k.w[a] = ld_state1(f.sf_knn_w, (size_t)KK * i + a, f.state_f64);
    }
  }
  k.T = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < KK; ++a) gf_skin_add(s, k.p, k.id[a], k.w[a], k.T);
  k.P = gf_skin_global(s, k.T, k.gw, k.gv);
}

// the deformed position alone, K at run time (k_gf_morph at K != 4: it needs P only)
__device__ __forceinline__ d3 gf_skin_pos(const GfSlotDev& s, int i) {
  const FrameIn& f = s.f.base;
  const int K = f.K;
  const d3 p = ld_state3(f.sf_points, (size_t)i, f.state_f64);
  d3 T = {0, 0, 0};
  for (int a = 0; a < K; ++a)
    gf_skin_add(s, p, f.sf_knn_idx[(size_t)K * i + a], ld_state1(f.sf_knn_w, (size_t)K * i + a, f.state_f64), T);
  double gw;
  d3 gv;
  return gf_skin_global(s, T, gw, gv);
}

// slm_gf_render (slm_render.hip): the device descriptor of bound slot `slot` (its current deform_verts) and its
// surfel count; SLM_OK or an error status with the text set.
int gf_render_slot(slm_gf* g, int32_t slot, GfSlot** dev, int32_t* n_surfels, const char* who = "slm_gf_render");

// ---- the render loss as a term of the run (slm_gf_bind_render_loss, slm_gf.hip) ----------------------------------------------
// What a slot with the term holds: the caller's context, inputs and parameters, the entry limit of the tile lists fixed at the
// bind, and the buffers the slot owns (grow-only, kept across binds).  ctx == null: no term.
struct GfRenderTerm {
  slm_render* ctx = nullptr;
  slm_render_params p{};
  const float* radii = nullptr;    // (N) float32 by surfel row, or null: p.radius
  const float* colors = nullptr;
  int cstride = 0;
  const float* target = nullptr;   // (3,h,w) float32
  double weight = 0.0;
  unsigned long long limit = 0;
  float* image = nullptr;          // (h,w,3) the render of the last evaluation
  double* gimg = nullptr;          // (h,w,3) dL/dimage
  double* pgrad = nullptr;         // (N,3) dL/dP by surfel row: what k_gf_data<K, true> reads
  double* loss = nullptr;          // [weighted loss, kept pixels] of the last evaluation
  double* scratch = nullptr;       // k_ssim_*'s
  size_t cap_image = 0, cap_gimg = 0, cap_pgrad = 0, cap_loss = 0, cap_scratch = 0;
};

// slm_render.hip: the guarded, enqueue-only renderer behind the term (see there)
int rn_gf_check(const char* who, const slm_render* r, const slm_render_params* p, int N, const float* colors, int cstride);
int rn_gf_size(const char* who, slm_render* r, const slm_render_params* p, GfSlot* gslot, int N, const float* radii,
               const float* colors, int cstride, float* image, int64_t entry_limit, unsigned long long* limit_out,
               void* stream);
void rn_gf_forward(slm_render* r, const slm_render_params* p, GfSlot* gslot, int N, const float* radii, const float* colors,
                   int cstride, float* image, unsigned long long limit, hipStream_t st);
void rn_gf_backward(slm_render* r, const slm_render_params* p, int N, bool per_point, const double* grad_image,
                    double* grad_points, hipStream_t st);
hipError_t rn_gf_status(const slm_render* r, unsigned long long out_host[2], hipStream_t st);
// slm_ssim.hip: slm_render_ssim_loss's launches on the caller's scratch
size_t ssim_scratch_doubles(int h, int w, bool with_grad);
void ssim_enqueue(int h, int w, const float* image_hwc, const float* target_chw, double weight, double* loss_out,
                  double* grad_image, double* scratch, hipStream_t st);
