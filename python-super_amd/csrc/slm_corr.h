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

#define SLM_CORR_BLOCKS 64   // loss partials of the term per slot (LossParts, slm_solver.h)

// corr_part / cnt_part: where the term's loss pairs and its kept counts go (LossParts, slm_solver.h).  mode 1 point-point,
// 2 point-plane; lam = the term's weight.
void launch_corr_targets(const FrameDev*, const CorrDev*, int slot, int N, const float* flow, hipStream_t);
void launch_corr_grad_pairs(const FrameDev*, const CorrDev*, int n_frames, int max_pos, int K, int mode, double lam, hipStream_t);
void launch_corr_grad(const FrameDev*, const CorrDev*, int n_frames, int maxN, int K, int mode, double lam, hipStream_t);
void launch_corr_loss(const FrameDev*, const CorrDev*, int n_frames, int K, int mode, double lam, int use_delta, int corr_part,
                      int cnt_part, hipStream_t);
