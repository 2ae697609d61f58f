// slm_nodes.hip -- the model-side node feeder (reference super/nodes.py: find_knn, update_ed, update_sfed_knn,
// Surfels.update): the brute-force KNN search, the skinning weights, the update of the surfels and nodes by a solved
// warp, the KNN-table check of the binds, and the eight stateless entry points of the C ABI that launch them.
// The formulas are the device routines of slm_nodes.h, shared with the fusion kernels (slm_fuse.hip).
#include "slm_nodes.h"
#include "slm_host.h"

// ---------------------------------------------------------------------------------
// Brute-force KNN (replaces pytorch3d.ops.knn_points as called by utils/utils.py:217):
// node tiles staged through LDS, every thread keeps its K best in registers
// (squared L2 in f64, ascending, ties -> lowest index because nodes are visited in order
// and a candidate replaces only on strictly smaller distance).
// BY_CLASS: the Semantic-SuPer branch (find_knn with num_classes, utils/utils.py:223-242): a query only sees the nodes of
// its own class; counter[0] counts the queries that found fewer than K (+ self) of them -- the reference asserts on those.
#define KNN_MAXK 9
#define KNN_TILE 1024
template <typename RT, bool BY_CLASS>
__global__ void __launch_bounds__(256) k_knn(int Nq, int Nn, int K, int skip_self, const RT* __restrict__ q,
                                              const RT* __restrict__ nodes, const int* __restrict__ q_seg,
                                              const int* __restrict__ node_seg, int* __restrict__ idx_out,
                                              RT* __restrict__ dist_out, int* __restrict__ counter) {
  __shared__ RT sx[KNN_TILE], sy[KNN_TILE], sz[KNN_TILE];
  __shared__ int sc[BY_CLASS ? KNN_TILE : 1];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double bd[KNN_MAXK];
  int bi[KNN_MAXK];
#pragma unroll
  for (int k = 0; k < KNN_MAXK; ++k) {
    bd[k] = 1e300;
    bi[k] = -1;
  }
  double px = 0, py = 0, pz = 0;
  int cls = 0;
  if (i < Nq) {
    px = q[3 * (size_t)i];
    py = q[3 * (size_t)i + 1];
    pz = q[3 * (size_t)i + 2];
    if constexpr (BY_CLASS) cls = q_seg[i];
  }
  for (int base = 0; base < Nn; base += KNN_TILE) {
    const int cnt = min(KNN_TILE, Nn - base);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
      sx[t] = nodes[3 * (size_t)(base + t)];
      sy[t] = nodes[3 * (size_t)(base + t) + 1];
      sz[t] = nodes[3 * (size_t)(base + t) + 2];
      if constexpr (BY_CLASS) sc[t] = node_seg[base + t];
    }
    __syncthreads();
    if (i < Nq) {
      for (int t = 0; t < cnt; ++t) {
        if constexpr (BY_CLASS)
          if (sc[t] != cls) continue;
        const double dx = px - (double)sx[t], dy = py - (double)sy[t], dz = pz - (double)sz[t];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < bd[KNN_MAXK - 1]) {
          // insertion into the sorted list (static indexing keeps it in registers): the candidate goes in front of the
          // first strictly farther entry, and every entry from there on moves down one slot -- unconditionally, so that an
          // entry never passes behind a later one at the same distance (which has the higher index)
          double cd = d2;
          int ci = base + t;
          bool shift = false;
#pragma unroll
          for (int k = 0; k < KNN_MAXK; ++k) {
            shift = shift || cd < bd[k];
            if (shift) {
              const double td = bd[k];
              const int ti = bi[k];
              bd[k] = cd;
              bi[k] = ci;
              cd = td;
              ci = ti;
            }
          }
        }
      }
    }
  }
  if (i < Nq) {
    const int off = skip_self ? 1 : 0;
    bool short_of = false;
    for (int k = 0; k < K; ++k) {
      idx_out[(size_t)i * K + k] = bi[k + off];
      dist_out[(size_t)i * K + k] = (RT)sqrt(bd[k + off]);
      short_of = short_of || bi[k + off] < 0;
    }
    if constexpr (BY_CLASS)
      if (short_of) atomicAdd(counter, 1);
  }
}

// softmax(node_weight_arg) weights + the stability test any(dist <= radius) (nodes.py:166,182,191), on float32 or float64
// tables; SEM: q_seg_conf / node_seg_conf (C columns, float64) switch on the Jensen-Shannon factor (nodes.py:183-189).
// radius_mode 0: the radius of the neighbour, 1: of the query itself.  K <= KNN_MAXK at run time: the loops over k are
// the kernel's own (node_softmax_weights unrolls over a constant; measured, that form is slower here -- LAB_NOTEBOOK).
template <typename RT, bool SEM>
__global__ void __launch_bounds__(256) k_knn_weights(int Nq, int K, int radius_mode, const int* __restrict__ idx,
                                                      const RT* __restrict__ dist, const RT* __restrict__ radii, int C,
                                                      const double* __restrict__ q_seg_conf,
                                                      const double* __restrict__ node_seg_conf, RT* __restrict__ w_out,
                                                      uint8_t* __restrict__ stable_io) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Nq) return;
  double e[KNN_MAXK];
  double emax = -1e300;
  bool any_in = false;
  for (int k = 0; k < K; ++k) {
    const int j = idx[(size_t)i * K + k];
    const double r = (double)radii[radius_mode == 0 ? j : i];
    const double d = (double)dist[(size_t)i * K + k];
    any_in = any_in || (d <= r);
    if constexpr (SEM)
      e[k] = node_weight_arg(d, r, node_jsd(node_seg_conf + (size_t)C * j, q_seg_conf + (size_t)C * i, C));
    else
      e[k] = node_weight_arg(d, r);
    emax = fmax(emax, e[k]);
  }
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    e[k] = exp(e[k] - emax);
    s += e[k];
  }
  for (int k = 0; k < K; ++k) w_out[(size_t)i * K + k] = (RT)(e[k] / s);
  if (stable_io && !any_in) stable_io[i] = 0;
}

// ---------------------------------------------------------------------------------
// Surfels.update (nodes.py:193-223): node_skin_update per surfel, node_move_update per node.  dv is the (J, 7) beta of the
// LM path, or with GLOBAL the (J+1, 7) deformation of the autograd path.
template <typename RT, int KK, bool GLOBAL>
__global__ void __launch_bounds__(256) k_update_surfels(int N, int J, int K, RT* __restrict__ pts, RT* __restrict__ nrm,
                                                         const int* __restrict__ knn_idx, const RT* __restrict__ knn_w,
                                                         const RT* __restrict__ ed_pts, const double* __restrict__ dv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) node_skin_update<RT, KK, GLOBAL>(i, J, K, pts, nrm, knn_idx, knn_w, ed_pts, dv);
}

// must run AFTER k_update_surfels (which reads the old node positions)
template <typename RT, bool GLOBAL>
__global__ void __launch_bounds__(256) k_update_nodes(int J, RT* __restrict__ ed_pts, RT* __restrict__ ed_nrm,
                                                       const double* __restrict__ dv) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < J) node_move_update<RT, GLOBAL>(j, J, ed_pts, ed_nrm, dv);
}

// ---------------------------------------------------------------------------------
// The binds' test of a frame's KNN tables as the reference's top-k makes them: knn_row_bad for every surfel row, and
// every ed_knn_idx entry (n_ed = J * K_ED of them) in [0, J).  *bad = 1 when the frame must be refused.  Reads the
// tables only.
__global__ void __launch_bounds__(256) k_check_knn(int N, int K, int J, const int* __restrict__ knn, long long n_ed,
                                                    const int* __restrict__ ed_knn, int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N && knn_row_bad(knn + (size_t)K * i, K, J)) *bad = 1;
  if (i < n_ed && (unsigned)ed_knn[i] >= (unsigned)J) *bad = 1;
}

void launch_check_knn(const slm_frame& f, int* bad, void* stream) {
  const long long n_ed = (long long)f.J * f.K_ED, n_thr = n_ed > f.N ? n_ed : (long long)f.N;
  hipLaunchKernelGGL(k_check_knn, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f.N, f.K, f.J,
                     f.sf_knn_idx, n_ed, f.ed_knn_idx, bad);
}

// ---- the stateless entry points -----------------------------------------------------------------------------------
// `who` names the entry point in its refusals (slm_apply_update_gf_f64 answers as slm_apply_update_gf).
template <typename RT, bool GLOBAL>
static int apply_update_t(const char* who, int32_t N, int32_t J, int32_t K, RT* sf_points, RT* sf_norms,
                          const int32_t* sf_knn_idx, const RT* sf_knn_w, RT* ed_points, RT* ed_norms, const double* dv,
                          void* stream) {
  if (K < 1 || K > 8) return fail(SLM_ERR_UNSUPPORTED, std::string(who) + ": num_neighbors must be in 1..8");
  if (N < 0 || J < 1 || !ed_points || !ed_norms || !dv || (N > 0 && (!sf_points || !sf_norms || !sf_knn_idx || !sf_knn_w)))
    return fail(SLM_ERR_INVALID, std::string(who) + ": bad argument");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((N + 255) / 256), blk(256);
  const RT* ed_old = ed_points;
  if constexpr (GLOBAL) {
    if (N > 0)
      SLM_K_DISPATCH(K, hipLaunchKernelGGL((k_update_surfels<RT, KK, true>), grid, blk, 0, st, N, J, K, sf_points, sf_norms,
                                          sf_knn_idx, sf_knn_w, ed_old, dv));
  } else if (N > 0) {   // the LM form keeps its loop over the runtime K (KK = 0): measured, LAB_NOTEBOOK
    hipLaunchKernelGGL((k_update_surfels<RT, 0, false>), grid, blk, 0, st, N, J, K, sf_points, sf_norms, sf_knn_idx, sf_knn_w,
                       ed_old, dv);
  }
  hipLaunchKernelGGL((k_update_nodes<RT, GLOBAL>), dim3((J + 255) / 256), dim3(256), 0, st, J, ed_points, ed_norms, dv);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

template <typename RT, bool BY_CLASS>
static void launch_knn(int Nq, int Nn, int K, int skip_self, const RT* q, const RT* nodes, const int* q_seg, const int* node_seg,
                       int* idx, RT* dist, int* counter, hipStream_t st) {
  if (Nq <= 0) return;
  hipLaunchKernelGGL((k_knn<RT, BY_CLASS>), dim3((Nq + 255) / 256), dim3(256), 0, st, Nq, Nn, K, skip_self, q, nodes, q_seg,
                     node_seg, idx, dist, counter);
}

template <typename RT, bool SEM>
static void launch_knn_weights(int Nq, int K, int radius_mode, const int* idx, const RT* dist, const RT* radii, int C,
                               const double* q_conf, const double* node_conf, RT* w, uint8_t* stable, hipStream_t st) {
  if (Nq <= 0) return;
  hipLaunchKernelGGL((k_knn_weights<RT, SEM>), dim3((Nq + 255) / 256), dim3(256), 0, st, Nq, K, radius_mode, idx, dist, radii, C,
                     q_conf, node_conf, w, stable);
}

extern "C" {

int slm_apply_update(int32_t N, int32_t J, int32_t K, float* sf_points, float* sf_norms,
                     const int32_t* sf_knn_idx, const float* sf_knn_w, float* ed_points,
                     float* ed_norms, const double* beta, void* stream) {
  return apply_update_t<float, false>("slm_apply_update", N, J, K, sf_points, sf_norms, sf_knn_idx, sf_knn_w, ed_points,
                                      ed_norms, beta, stream);
}

int slm_apply_update_f64(int32_t N, int32_t J, int32_t K, double* sf_points, double* sf_norms,
                         const int32_t* sf_knn_idx, const double* sf_knn_w, double* ed_points,
                         double* ed_norms, const double* beta, void* stream) {
  return apply_update_t<double, false>("slm_apply_update_f64", N, J, K, sf_points, sf_norms, sf_knn_idx, sf_knn_w,
                                       ed_points, ed_norms, beta, stream);
}

int slm_apply_update_gf(int32_t N, int32_t J, int32_t K, float* sf_points, float* sf_norms,
                        const int32_t* sf_knn_idx, const float* sf_knn_w, float* ed_points, float* ed_norms,
                        const double* deform, void* stream) {
  return apply_update_t<float, true>("slm_apply_update_gf", N, J, K, sf_points, sf_norms, sf_knn_idx, sf_knn_w, ed_points,
                                     ed_norms, deform, stream);
}

int slm_apply_update_gf_f64(int32_t N, int32_t J, int32_t K, double* sf_points, double* sf_norms,
                            const int32_t* sf_knn_idx, const double* sf_knn_w, double* ed_points, double* ed_norms,
                            const double* deform, void* stream) {
  return apply_update_t<double, true>("slm_apply_update_gf", N, J, K, sf_points, sf_norms, sf_knn_idx, sf_knn_w,
                                      ed_points, ed_norms, deform, stream);
}

int slm_knn(int32_t Nq, int32_t Nn, int32_t K, int32_t skip_self, const float* q, const float* nodes,
            int32_t* idx, float* dist, void* stream) {
  if (Nq < 0 || Nn < 1 || K < 1 || K + (skip_self ? 1 : 0) > 9 || !nodes || !idx || !dist ||
      (Nq > 0 && !q))
    return fail(SLM_ERR_INVALID, "slm_knn: bad argument (K + skip_self <= 9)");
  // fewer nodes than neighbours asked for would leave index -1 / distance inf in the tables that
  // slm_bind_frame, slm_knn_weights and slm_apply_update index with (the reference's knn_points fails too)
  if (Nn < K + (skip_self ? 1 : 0))
    return fail(SLM_ERR_INVALID, "slm_knn: fewer nodes than K (+ self)");
  launch_knn<float, false>(Nq, Nn, K, skip_self, q, nodes, nullptr, nullptr, idx, dist, nullptr, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_knn_weights(int32_t Nq, int32_t K, int32_t radius_mode, const int32_t* idx, const float* dist,
                    const float* radii, float* w, uint8_t* stable, void* stream) {
  if (Nq < 0 || K < 1 || K > 9 || !idx || !dist || !radii || !w)
    return fail(SLM_ERR_INVALID, "slm_knn_weights: bad argument");
  launch_knn_weights<float, false>(Nq, K, radius_mode, idx, dist, radii, 0, nullptr, nullptr, w, stable, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_knn_f64(int32_t Nq, int32_t Nn, int32_t K, int32_t skip_self, const double* q, const double* nodes,
                const int32_t* q_seg, const int32_t* node_seg, int32_t* idx, double* dist, void* stream) {
  if (Nq < 0 || Nn < 1 || K < 1 || K + (skip_self ? 1 : 0) > 9 || !nodes || !idx || !dist || (Nq > 0 && !q) ||
      ((q_seg == nullptr) != (node_seg == nullptr)))
    return fail(SLM_ERR_INVALID, "slm_knn_f64: bad argument (K + skip_self <= 9; both class arrays or none)");
  if (Nn < K + (skip_self ? 1 : 0)) return fail(SLM_ERR_INVALID, "slm_knn_f64: fewer nodes than K (+ self)");
  hipStream_t st = (hipStream_t)stream;
  int* counter = nullptr;
  if (q_seg) {
    HIPCHK(hipMalloc((void**)&counter, sizeof(int)));
    HIPCHK(hipMemsetAsync(counter, 0, sizeof(int), st));
  }
  if (q_seg)
    launch_knn<double, true>(Nq, Nn, K, skip_self, q, nodes, q_seg, node_seg, idx, dist, counter, st);
  else
    launch_knn<double, false>(Nq, Nn, K, skip_self, q, nodes, nullptr, nullptr, idx, dist, nullptr, st);
  HIPCHK(hipGetLastError());
  if (counter) {
    int n_short = 0;
    HIPCHK(hipMemcpyAsync(&n_short, counter, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipFree(counter));
    if (n_short > 0)
      return fail(SLM_ERR_INVALID, "slm_knn_f64: a class has fewer nodes than the neighbours asked for");
  }
  return SLM_OK;
}

int slm_knn_weights_f64(int32_t Nq, int32_t K, int32_t radius_mode, const int32_t* idx, const double* dist,
                        const double* radii, int32_t num_classes, const double* q_seg_conf,
                        const double* node_seg_conf, double* w, uint8_t* stable, void* stream) {
  if (Nq < 0 || K < 1 || K > 9 || !idx || !dist || !radii || !w || num_classes < 0 || num_classes > SLM_MAX_CLASSES ||
      (num_classes > 0 && (!q_seg_conf || !node_seg_conf)))
    return fail(SLM_ERR_INVALID, "slm_knn_weights_f64: bad argument");
  if (num_classes > 0)
    launch_knn_weights<double, true>(Nq, K, radius_mode, idx, dist, radii, num_classes, q_seg_conf, node_seg_conf, w, stable,
                                     (hipStream_t)stream);
  else
    launch_knn_weights<double, false>(Nq, K, radius_mode, idx, dist, radii, 0, nullptr, nullptr, w, stable, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

}  // extern "C"
