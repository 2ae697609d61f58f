// slm_nodes.h -- the device routines of the model-side node feeder, each written once (reference super/nodes.py:
// find_knn, update_ed, update_sfed_knn, Surfels.update).  These are the formulas where the reference is unusual -- a
// softmax OF an exponential, eps inside the log of the JSD, the translation added to the rotated normal -- so the kernels
// of slm_nodes.hip and the fusion kernels of slm_fuse.hip share them instead of carrying copies that can drift.
#pragma once
#include "slm_common.h"

// Jensen-Shannon divergence of two class distributions (utils/utils.py:244-254):
// JSD(P, Q) = (KL(P|M) + KL(Q|M)) / 2, M = (P + Q) / 2, KL(P|Q) = sum P log(P / (Q + eps) + eps)
__device__ __forceinline__ double node_jsd(const double* P, const double* Q, int C) {
  double a = 0.0, b = 0.0;
  for (int k = 0; k < C; ++k) {
    const double M = 0.5 * (P[k] + Q[k]);
    a += P[k] * log(P[k] / (M + 1e-13) + 1e-13);
    b += Q[k] * log(Q[k] / (M + 1e-13) + 1e-13);
  }
  return 0.5 * (a + b);
}

// The argument of the weights' softmax for one neighbour: exp(-d / r) (nodes.py:166,182,191); with js, its JSD against
// the query, exp(-JSD)^(1/2) * exp(-d/r)^(1/2) (nodes.py:183-189,472-477, power_arg = (1/2, 1/2)).
__device__ __forceinline__ double node_weight_arg(const double d, const double r) { return exp(-d / r); }
__device__ __forceinline__ double node_weight_arg(const double d, const double r, const double js) {
  return sqrt(exp(-js)) * sqrt(exp(-d / r));
}

// w = softmax(node_weight_arg) over the K neighbours -- a softmax OF an exponential; js = nullptr: no semantic factor.
// The sum runs k ascending.  K <= KMAX, the length of the arrays; the loops are unrolled over KMAX.
template <int KMAX>
__device__ __forceinline__ void node_softmax_weights(const int K, const double (&d)[KMAX], const double (&r)[KMAX],
                                                     const double* js, double (&w)[KMAX]) {
  double mx = -1e300, s = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      w[k] = js ? node_weight_arg(d[k], r[k], js[k]) : node_weight_arg(d[k], r[k]);
      mx = fmax(mx, w[k]);
    }
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      w[k] = exp(w[k] - mx);
      s += w[k];
    }
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) w[k] /= s;
}

// Surfels.update of surfel i (nodes.py:193-223), in place on float32 or float64 arrays (RT): the skinned point, the
// blended and normalised normal.  node_skin_term adds one neighbour (its row b of dv, its position g) with weight w to
// both sums: the reference rotates the normals with the 7-wide beta, so the translation b_k is ADDED to the rotated
// normal before blending (nodes.py:207-213).
__device__ __forceinline__ void node_skin_term(const double w, const d3 p, const d3 n0, const double* __restrict__ b,
                                               const d3 g, d3& T, d3& Nn) {
  const d3 qv = {b[1], b[2], b[3]};
  d3 t = quat_apply(b[0], qv, p - g);
  t = {t.x + b[4] + g.x, t.y + b[5] + g.y, t.z + b[6] + g.z};
  T = {T.x + w * t.x, T.y + w * t.y, T.z + w * t.z};
  d3 rn = quat_apply(b[0], qv, n0);
  rn = {rn.x + b[4], rn.y + b[5], rn.z + b[6]};
  Nn = {Nn.x + w * rn.x, Nn.y + w * rn.y, Nn.z + w * rn.z};
}

// KK = opt.num_neighbors as a constant (the row is loaded first, the loop unrolled), or 0: a loop over the runtime K.
// GLOBAL: dv has the (J+1, 7) form of the autograd path, whose last row T_g rotates the blended normal and translates the
// point; without it nothing is added.  Reads the OLD node positions: node_move_update of the same dv runs after it.
template <typename RT, int KK, bool GLOBAL>
__device__ __forceinline__ void node_skin_update(const int i, const int J, const int K, RT* __restrict__ pts_, RT* __restrict__ nrm_,
                                                 const int* __restrict__ knn_idx, const RT* __restrict__ knn_w,
                                                 const RT* __restrict__ ed_pts, const double* __restrict__ dv) {
  RT* pts = pts_ + 3 * (size_t)i - 3 * i;   // 64-bit row offsets below go through these bases
  RT* nrm = nrm_ + 3 * (size_t)i - 3 * i;
  const d3 p = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
  const d3 n0 = {(double)nrm[3 * i], (double)nrm[3 * i + 1], (double)nrm[3 * i + 2]};
  d3 T = {0, 0, 0}, Nn = {0, 0, 0};
  // (the sums run k = 0, 1, ... like the reference's sum over dim 1)
  if constexpr (KK > 0) {
    int id[KK];
    double w[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      id[k] = knn_idx[(size_t)KK * i + k];
      w[k] = (double)knn_w[(size_t)KK * i + k];
    }
#pragma unroll
    for (int k = 0; k < KK; ++k)
      node_skin_term(w[k], p, n0, dv + 7 * id[k],
                     {(double)ed_pts[3 * id[k]], (double)ed_pts[3 * id[k] + 1], (double)ed_pts[3 * id[k] + 2]}, T, Nn);
  } else {
    for (int k = 0; k < K; ++k) {
      const int id = knn_idx[(size_t)K * i + k];
      node_skin_term((double)knn_w[(size_t)K * i + k], p, n0, dv + 7 * id,
                     {(double)ed_pts[3 * id], (double)ed_pts[3 * id + 1], (double)ed_pts[3 * id + 2]}, T, Nn);
    }
  }
  d3 tg = {0, 0, 0};
  if constexpr (GLOBAL) {
    const double* bgl = dv + 7 * J;
    Nn = quat_apply(bgl[0], {bgl[1], bgl[2], bgl[3]}, Nn);
    tg = {bgl[4], bgl[5], bgl[6]};
  }
  const double nl = fmax(sqrt(dot(Nn, Nn)), 1e-12);   // F.normalize eps
  pts[3 * i] = (RT)(GLOBAL ? T.x + tg.x : T.x);
  pts[3 * i + 1] = (RT)(GLOBAL ? T.y + tg.y : T.y);
  pts[3 * i + 2] = (RT)(GLOBAL ? T.z + tg.z : T.z);
  nrm[3 * i] = (RT)(Nn.x / nl);
  nrm[3 * i + 1] = (RT)(Nn.y / nl);
  nrm[3 * i + 2] = (RT)(Nn.z / nl);
}

// ... and of node j: moved by its translation (GLOBAL: and the global one), its normal rotated (GLOBAL: then by the
// global rotation) and normalised.
template <typename RT, bool GLOBAL>
__device__ __forceinline__ void node_move_update(const int j, const int J, RT* __restrict__ ed_pts, RT* __restrict__ ed_nrm,
                                                 const double* __restrict__ dv) {
  const double* b = dv + 7 * j;
  const d3 n0 = {(double)ed_nrm[3 * j], (double)ed_nrm[3 * j + 1], (double)ed_nrm[3 * j + 2]};
  d3 rn = quat_apply(b[0], {b[1], b[2], b[3]}, n0);
  d3 t = {(double)ed_pts[3 * j] + b[4], (double)ed_pts[3 * j + 1] + b[5], (double)ed_pts[3 * j + 2] + b[6]};
  if constexpr (GLOBAL) {
    const double* bgl = dv + 7 * J;
    rn = quat_apply(bgl[0], {bgl[1], bgl[2], bgl[3]}, rn);
    t = {t.x + bgl[4], t.y + bgl[5], t.z + bgl[6]};
  }
  const double nl = fmax(sqrt(dot(rn, rn)), 1e-12);
  ed_pts[3 * j] = (RT)t.x;
  ed_pts[3 * j + 1] = (RT)t.y;
  ed_pts[3 * j + 2] = (RT)t.z;
  ed_nrm[3 * j] = (RT)(rn.x / nl);
  ed_nrm[3 * j + 1] = (RT)(rn.y / nl);
  ed_nrm[3 * j + 2] = (RT)(rn.z / nl);
}
