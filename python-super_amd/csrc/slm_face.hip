// slm_face.hip -- triangle-area face term of the LM path (slm_enable_face, include/super_lm.h; the reference has only the
// first-order form, super/deform_mesh.py:51-60, which GraphFit carries: slm_gf.hip use_face).
//
//   k_face_grad        : J^T J blocks and J^T r of the term into the pair records (pairbuf) of the K-generic data path,
//                        between k_data_grad_pairs and k_pair_scatter
//   k_face_grad_band   : the same into the band with per-entry atomics (slm_assemble)
//   k_face_loss        : sum_t r_t^2 at beta or at the trial point, per-block partials behind the correspondence term's
//                        (read out for slm_face_loss by k_term_loss_out, slm_misc.hip)
//   k_face_bandwidth   : tile half-bandwidth the mesh's pairs need (ensure_band)
//
// Residual of triangle t with nodes (i0, i1, i2), lambda = weight: v_a = g_a + beta[a, 4:7] (rotations do not enter),
// e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2, A = sqrt(|c|^2 + 1e-13) / 2, r = lambda (A - A0_t).  One row with nine non-zeros
// on the translation columns 7 i_a + 4..6: dA/dv1 = (e2 x c) / 4A, dA/dv2 = (c x e1) / 4A, dA/dv0 = -(their sum).  The
// constant keeps a degenerate triangle finite (A >= 1.58e-7, gradient 0).  The loss is sum r^2: the weight multiplies
// the residual, as for every LM term (GraphFit multiplies the squared sum instead).
#include <algorithm>

#include "slm_face.h"
#include "slm_host.h"

namespace {
struct FaceRow {
  int i0, i1, i2;   // node ids
  d3 g0, g1, g2;    // lambda dA/dv_a
  double r;         // lambda (A - A0)
};

__device__ __forceinline__ d3 face_vertex(const double* __restrict__ npk, int j) {
  const double* q = npk + (size_t)SLM_NPK * j;
  return {q[7] + q[4], q[8] + q[5], q[9] + q[6]};
}

// ids, residual and (GRAD) the nine-vector of triangle t at the node table npk
template <bool GRAD>
__device__ __forceinline__ void face_row(const FaceDev& fc, const double* __restrict__ npk, int t, double lam, FaceRow& o) {
  const int F = fc.n_tri;
  o.i0 = fc.tri[t];
  o.i1 = fc.tri[(size_t)F + t];
  o.i2 = fc.tri[2 * (size_t)F + t];
  const d3 v0 = face_vertex(npk, o.i0), v1 = face_vertex(npk, o.i1), v2 = face_vertex(npk, o.i2);
  const d3 e1 = v1 - v0, e2 = v2 - v0;
  const d3 c = cross(e1, e2);
  const double A = 0.5 * sqrt(dot(c, c) + 1e-13);
  o.r = lam * (A - fc.areas[t]);
  if (GRAD) {
    const double s = lam / (4.0 * A);
    o.g1 = s * cross(e2, c);
    o.g2 = s * cross(c, e1);
    o.g0 = {-(o.g1.x + o.g2.x), -(o.g1.y + o.g2.y), -(o.g1.z + o.g2.z)};
  }
}
// (selects, not indexed loads: a runtime index into the row would send it to scratch)
__device__ __forceinline__ double comp(const d3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
__device__ __forceinline__ d3 sel3(const d3 a, const d3 b, const d3 c, int k) {
  return {k == 0 ? a.x : (k == 1 ? b.x : c.x), k == 0 ? a.y : (k == 1 ? b.y : c.y), k == 0 ? a.z : (k == 1 ? b.z : c.z)};
}
__device__ __forceinline__ d3 grad_of(const FaceRow& f, int k) { return sel3(f.g0, f.g1, f.g2, k); }
__device__ __forceinline__ int id_of(const FaceRow& f, int k) { return k == 0 ? f.i0 : (k == 1 ? f.i1 : f.i2); }
}  // namespace

// One thread per (triangle, record): records 0..2 are the diagonal pairs of the three vertices -- the lower 3 x 3 of the
// translation block (rows / columns 4..6 of the 7 x 7) and J^T r into entries 49 + 4..6 --, records 3..5 the cross pairs
// (0,1), (0,2), (1,2), whose 3 x 3 block is stored with the larger node id as the row (as the pair keys).  Six threads
// repeat a triangle's geometry (36 loads, ~60 flops) so that each issues 9 atomics instead of one thread 54 in a row:
// the pass is bound by the latency of the f64 atomics, not by arithmetic.  The plan holds every one of these pairs
// (prep_pairs appends the mesh's keys), and the bind has checked the ids.
// grid = (ceil(6 max F / 256), n_frames)
__global__ void __launch_bounds__(256) k_face_grad(const FrameDev* __restrict__ frames, const FaceDev* __restrict__ face, double lam) {
  const FrameDev& fd = frames[blockIdx.y];
  const FaceDev& fc = face[blockIdx.y];
  if (!fd.bound || fd.st->stopped || !fd.vk_ready || !fc.ready) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = e / 6, rec = e - 6 * t;
  if (t >= fc.n_tri) return;
  FaceRow fr;
  face_row<true>(fc, fd.node_pk, t, lam, fr);
  double* pb = fd.pairbuf + (size_t)fc.tri_pidx[6 * (size_t)t + rec] * SLM_WREC;
  if (rec < 3) {
    const d3 g = grad_of(fr, rec);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) atomic_add_f64(pb + 7 * (4 + i) + 4 + j, comp(g, i) * comp(g, j));
      atomic_add_f64(pb + 49 + 4 + i, comp(g, i) * fr.r);
    }
  } else {
    const int va = rec == 5 ? 1 : 0, vb = rec == 3 ? 1 : 2;
    const bool a_row = id_of(fr, va) > id_of(fr, vb);
    const d3 ga = grad_of(fr, va), gb = grad_of(fr, vb);
    const d3 gr = a_row ? ga : gb, gc = a_row ? gb : ga;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) atomic_add_f64(pb + 7 * (4 + i) + 4 + j, comp(gr, i) * comp(gc, j));
  }
}

// per-entry form (k_corr_grad's sums): row^T row into the lower band, -row^T r into rhs.  One thread per triangle.
// grid = (ceil(max F / 64), n_frames)
__global__ void __launch_bounds__(64) k_face_grad_band(const FrameDev* __restrict__ frames, const FaceDev* __restrict__ face, double lam) {
  const FrameDev& fd = frames[blockIdx.y];
  const FaceDev& fc = face[blockIdx.y];
  if (!fd.bound || fd.st->stopped || !fc.ready) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= fc.n_tri) return;
  FaceRow fr;
  face_row<true>(fc, fd.node_pk, t, lam, fr);
#pragma unroll
  for (int a = 0; a < 9; ++a) {
    const int ia = 7 * id_of(fr, a / 3) + 4 + a % 3;
    const double ja = comp(grad_of(fr, a / 3), a % 3);
    atomic_add_f64(fd.rhs + ia, -ja * fr.r);
#pragma unroll
    for (int b = 0; b < 9; ++b) {
      const int ib = 7 * id_of(fr, b / 3) + 4 + b % 3;
      if (ia >= ib) atomic_add_f64(band_entry(fd, ia, ib), ja * comp(grad_of(fr, b / 3), b % 3));
    }
  }
}

// grid = (SLM_FACE_BLOCKS, n_frames); grid-stride over triangles.  Block b of a slot stores its sum as the pair b at face_part
// (term_loss_store); a slot without a mesh stores zeros.
__global__ void __launch_bounds__(256) k_face_loss(const FrameDev* __restrict__ frames, const FaceDev* __restrict__ face, double lam,
                                                    int use_delta, int face_part) {
  __shared__ double sm[16];
  const FrameDev& fd = frames[blockIdx.y];
  const FaceDev& fc = face[blockIdx.y];
  if (!fd.bound || fd.st->stopped) return;
  double acc = 0.0;
  if (fc.ready) {
    const double* npk = use_delta ? fd.node_pk_try : fd.node_pk;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < fc.n_tri; t += gridDim.x * blockDim.x) {
      FaceRow fr;
      face_row<false>(fc, npk, t, lam, fr);
      acc += fr.r * fr.r;
    }
  }
  const double s = block_sum(acc, sm);
  if (threadIdx.x == 0) term_loss_store(fd, face_part, s);
}

// max over the triangles of tile(7 hi + 6) - tile(7 lo), as k_bandwidth's over the KNN tables (nothing indexes with the ids)
__global__ void __launch_bounds__(256) k_face_bandwidth(const int32_t* __restrict__ tri, int F, int* __restrict__ out) {
  int wmax = 0;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < F; t += gridDim.x * blockDim.x) {
    const int a = tri[t], b = tri[(size_t)F + t], c = tri[2 * (size_t)F + t];
    const int lo = min(a, min(b, c)), hi = max(a, max(b, c));
    wmax = max(wmax, (7 * hi + 6) / SLM_NB - (7 * lo) / SLM_NB);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wmax = max(wmax, __shfl_down(wmax, o, 64));
  if ((threadIdx.x & 63) == 0 && wmax > 0) atomicMax(out, wmax);
}

// ---- host launchers (called from slm_lm.hip, slm_terms.hip, slm_bind.hip) ---------------------------
void launch_face_grad(const FrameDev* frames_dev, const FaceDev* face_dev, int n_frames, int max_tri, double lam, hipStream_t st) {
  if (max_tri <= 0) return;
  const long long n = 6ll * max_tri;
  hipLaunchKernelGGL(k_face_grad, dim3((unsigned)((n + 255) / 256), n_frames), dim3(256), 0, st, frames_dev, face_dev, lam);
}

void launch_face_grad_band(const FrameDev* frames_dev, const FaceDev* face_dev, int n_frames, int max_tri, double lam, hipStream_t st) {
  if (max_tri <= 0) return;
  hipLaunchKernelGGL(k_face_grad_band, dim3((max_tri + 63) / 64, n_frames), dim3(64), 0, st, frames_dev, face_dev, lam);
}

void launch_face_loss(const FrameDev* frames_dev, const FaceDev* face_dev, int n_frames, double lam, int use_delta, int face_part,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_face_loss, dim3(SLM_FACE_BLOCKS, n_frames), dim3(256), 0, st, frames_dev, face_dev, lam, use_delta, face_part);
}

void launch_face_bandwidth(const int32_t* tri, int n_tri, int* out, hipStream_t st) {
  if (n_tri <= 0) return;
  hipLaunchKernelGGL(k_face_bandwidth, dim3(std::min((n_tri + 255) / 256, 64)), dim3(256), 0, st, tri, n_tri, out);
}
