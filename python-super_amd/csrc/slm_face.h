// slm_face.h -- the triangle-area face term of the LM path (slm_enable_face, include/super_lm.h): the per-slot descriptor
// of the mesh and the launch functions of slm_face.hip.
#pragma once
#include "slm_common.h"

// Mesh of a slot, resident in HBM as an array beside the FrameDev array (same index).  tri / areas are the slot's own
// copies (slm_set_face_mesh: the mesh outlives a frame); tri_pidx belongs to the slot's pair plan and is rebuilt by every bind.
struct FaceDev {
  GP<const int32_t> tri;        // (3, F) node ids, row a = vertex a of every triangle
  GP<const double> areas;       // (F) rest areas A0
  GP<const int32_t> tri_pidx;   // (F, 6) pair records of a triangle: diagonals of vertex 0, 1, 2, then pairs (0,1), (0,2), (1,2)
  int32_t n_tri;
  int32_t ready;                // 1 once a bind has checked the ids against J and placed the six pairs in the slot's plan
};

#define SLM_FACE_BLOCKS 16   // loss partials of the term per slot (LossParts, slm_solver.h)

// face_part: where the term's loss pairs go (LossParts, slm_solver.h); lam = the term's weight.
void launch_face_grad(const FrameDev*, const FaceDev*, int n_frames, int max_tri, double lam, hipStream_t);
void launch_face_grad_band(const FrameDev*, const FaceDev*, int n_frames, int max_tri, double lam, hipStream_t);
void launch_face_loss(const FrameDev*, const FaceDev*, int n_frames, double lam, int use_delta, int face_part, hipStream_t);
void launch_face_bandwidth(const int32_t* tri, int n_tri, int* out, hipStream_t);
