// slm_corr.h -- the flow-correspondence term of the LM path (slm_enable_corr, include/super_lm.h): the per-slot
// descriptor of the frozen targets and the launch functions of slm_corr.hip.
#pragma once
#include "slm_common.h"

// Targets of a slot, resident in HBM as an array beside the FrameDev array (same index); constant for a whole LM run.
struct CorrDev {
  GP<double> o;         // (N,3) target points
  GP<double> n;         // (N,3) target normals (zeros when the caller gave none: mode 1)
  GP<uint8_t> valid;    // (N) 1 where the surfel has a correspondence
  int32_t has;          // 1 once slm_bind_corr_flow / slm_bind_corr_points ran for the bound frame
  int32_t pad;
};

#if defined(__HIPCC__)
#include "slm_gf_sample.h"
// The frozen target of surfel i of a frame from the flow (2,H,W), as GraphFit's term reads it at zero deformation: the
// unrounded projection of the surfel, the flow sampled there grid_sample-style, margin 1 on the shifted coordinates, all four
// taps mapped and finite; zeros where invalid.  o / n: (N,3), valid: (N).  Shared by k_corr_targets (slm_corr.hip, a bound
// slot) and k_rg_corr_targets (slm_rigid.hip, a raw slm_frame).
__device__ __forceinline__ void corr_target_of(const FrameIn& f, const int i, const float* __restrict__ flow, double* __restrict__ o_out,
                                               double* __restrict__ n_out, uint8_t* __restrict__ valid) {
  const d3 p = ld_state3(f.sf_points, (size_t)i, f.state_f64);
  const GfProj pr = gf_project(f, p);
  double fl[2], D[4];
  gf_flow_sample(flow, f.H, f.W, pr.u, pr.v, fl, D);
  const double uc = pr.u + fl[0], vc = pr.v + fl[1];
  // margin 1 on the shifted float coordinates (false for NaN): every tap of gf_sample is inside the image
  bool ok = vc >= 1.0 && vc < (double)(f.H - 2) && uc >= 1.0 && uc < (double)(f.W - 2);
  GfSample q;
  if (ok) ok = gf_sample(f, uc, vc, q);
  if (ok) ok = q.o.x == q.o.x && q.o.y == q.o.y && q.o.z == q.o.z && q.n.x == q.n.x && q.n.y == q.n.y && q.n.z == q.n.z;
  double* o = o_out + 3 * (size_t)i;
  double* n = n_out + 3 * (size_t)i;
  o[0] = ok ? q.o.x : 0.0;
  o[1] = ok ? q.o.y : 0.0;
  o[2] = ok ? q.o.z : 0.0;
  n[0] = ok ? q.n.x : 0.0;
  n[1] = ok ? q.n.y : 0.0;
  n[2] = ok ? q.n.z : 0.0;
  valid[i] = ok ? 1 : 0;
}
#endif

#define SLM_CORR_BLOCKS 64  // loss partials of the term per slot (LossParts, slm_solver.h)

// corr_part / cnt_part: where the term's loss pairs and its kept counts go (LossParts, slm_solver.h).  mode 1 point-point,
// 2 point-plane; lam = the term's weight.
void launch_corr_targets(const FrameDev*, const CorrDev*, int slot, int N, const float* flow, hipStream_t);
void launch_corr_grad_pairs(const FrameDev*, const CorrDev*, int n_frames, int max_pos, int K, int mode, double lam, hipStream_t);
void launch_corr_grad(const FrameDev*, const CorrDev*, int n_frames, int maxN, int K, int mode, double lam, hipStream_t);
void launch_corr_loss(const FrameDev*, const CorrDev*, int n_frames, int K, int mode, double lam, int use_delta, int corr_part,
                      int cnt_part, hipStream_t);
