// slm_morph.h -- the semantic boundary-morph term of the LM path (slm_enable_morph, include/super_lm.h): the per-slot
// descriptor of the term's inputs and work arrays and the launch functions of slm_morph.hip.
#pragma once
#include "slm_common.h"

// Inputs and work arrays of a slot, resident in HBM as an array beside the FrameDev array (same index).  img_seg_conf and
// sf_seg are the caller's (read in place); the boundary lists are the slot's own, built by slm_bind_morph; the rest is
// rewritten by every selection pass (k_morph_select + k_morph_fold).
struct MorphDev {
  GP<const float> img_seg_conf;   // (C,H,W)
  GP<const int32_t> sf_seg;       // (N)
  GP<const float2> edge_xy;       // boundary pixels (x,y), per class, row-major pixel order
  GP<uint8_t> kept;               // (N) 1 where the last selection kept the surfel
  GP<double> target;              // (N,2) m_i = (e1 + e2) / 2 of a kept surfel, zeros otherwise
  GP<double> li;                  // (N) l_i = (d1 + d2) / 2 of a kept surfel, zero otherwise
  GP<double> part;                // (ceil(N / 256), 3) per block of the selection: sum l_i, kept, candidates
  GP<double> stat;                // [4] of the last selection: sum l_i, kept n, candidates, lambda^2 / n sum l_i
  int32_t edge_off[SLM_MAX_CLASSES + 1];   // class c owns edge_xy[edge_off[c] .. edge_off[c+1])
  int32_t C;                      // num_classes
  int32_t has;                    // 1 once slm_bind_morph ran for the bound frame
  int32_t pad;
};

#define SLM_MORPH_BLOCKS 1   // loss pairs of the term per slot (LossParts, slm_solver.h): the fold's one scaled sum

// Selection at beta (use_delta 0) or at the trial point, then the fold per slot: n, the sums and, with morph_part >= 0, the
// term's loss lambda^2 / n sum l_i as the pair at morph_part (LossParts); out (one slot only, or null) <- {loss, n, candidates}.
void launch_morph_select(const FrameDev*, const MorphDev*, int n_frames, int maxN, int K, double lam, int use_delta, int morph_part,
                         double* out, hipStream_t);
// The term's rows at the selection the last launch_morph_select(use_delta 0) left: into the pair records / into the band.
void launch_morph_grad_pairs(const FrameDev*, const MorphDev*, int n_frames, int max_pos, int K, double lam, hipStream_t);
void launch_morph_grad(const FrameDev*, const MorphDev*, int n_frames, int maxN, int K, double lam, hipStream_t);
