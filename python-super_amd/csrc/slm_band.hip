// slm_band.hip -- damped normal equations (JtJ + uI) delta = jtl as a block-banded
// float64 Cholesky (replaces the reference's dense torch.linalg.cholesky +
// cholesky_solve on a (7J)^2 matrix, super/LM.py:37-51,97-100).
//
// Storage: lower band in NB x NB tiles, column-major inside a tile; tile (r,c),
// c <= r <= c+wb, at band[(c*(wb+1) + (r-c)) * NB*NB].  The ED graph couples only
// nearby nodes, so wb << nt (half-bandwidth ~156 node blocks at J=2k).
//
// Per tile column c (right-looking):
//   k_panel(c)  block d: factor A(c,c)+uI = L L^T and form L^-1 in LDS (every block,
//               redundantly); d=0 stores L^-1 and forward-substitutes y_c = L^-1 b_c;
//               d>=1: L(c+d,c) = A(c+d,c) L^-T on the f64 MFMA (v_mfma_f64_16x16x4_f64).
//   k_trail(c)  A(r,s) -= L(r,c) L(s,c)^T for the wb x wb window (MFMA); b_s -= L(s,c) y_c.
// Back substitution k_backsub(c), c = nt-1..0: x_c = L_cc^-T y_c, y_(c-d) -= L(c,c-d)^T x_c.
// A non-positive pivot sets st->chol_fail (reference: RuntimeError -> "Solver failed").
#include "slm_tile.h"
#include "slm_launch.h"

// ---------------------------------------------------------------------------------
// Tile half-bandwidth from the KNN tables: max over coupled node pairs (a >= b) of
// tile(7a+6) - tile(7b).  Surfel tuples couple all pairs among their K nodes
// (loss.py:277-288); ARAP couples (j, k) (loss.py:414-426).
// out[1]: the tables hold a row or an index the binds refuse (knn_row_bad, an ed_knn_idx entry outside [0, J)) -- the
// check of the frames that take no data-term preparation (use_data 0); nothing here indexes with the ids.
__global__ void __launch_bounds__(256) k_bandwidth(slm_frame f, int* __restrict__ out) {
  int wmax = 0;
  bool bad = false;
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < f.N; i += stride) {
    bad |= knn_row_bad(f.sf_knn_idx + (size_t)f.K * i, f.K, f.J);
    int lo = f.sf_knn_idx[(size_t)f.K * i], hi = lo;
    for (int k = 1; k < f.K; ++k) {   // (K = num_neighbors, any value)
      const int id = f.sf_knn_idx[(size_t)f.K * i + k];
      lo = min(lo, id);
      hi = max(hi, id);
    }
    wmax = max(wmax, (7 * hi + 6) / NB - (7 * lo) / NB);
  }
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < f.J * f.K_ED; t += stride) {
    const int j = t / f.K_ED, k = f.ed_knn_idx[t];
    bad |= (unsigned)k >= (unsigned)f.J;
    int lo = min(j, k), hi = max(j, k);
    wmax = max(wmax, (7 * hi + 6) / NB - (7 * lo) / NB);
  }
  if (bad) out[1] = 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wmax = max(wmax, __shfl_down(wmax, o, 64));
  if ((threadIdx.x & 63) == 0 && wmax > 0) atomicMax(out, wmax);
}

// grid = (wb_cap + 1, n_frames), 256 threads
__global__ void __launch_bounds__(256) k_panel(const FrameDev* __restrict__ frames, int c,
                                                double u_override) {
  extern __shared__ double lds[];   // PanelLds; of its exchange buffer and ints only s_ok is used (potrf64 + inverse_assemble64)
  double *S = PanelLds::S(lds), *M = PanelLds::M(lds), *dinv = PanelLds::dinv(lds), *wt = PanelLds::wt(lds), *vec = PanelLds::vec(lds);
  int* s_ok = PanelLds::s_ok(lds);
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped || c >= fd.nt) return;
  const int d = blockIdx.x;
  if (d > fd.wb || c + d >= fd.nt) return;
  const double u = (u_override >= 0.0) ? u_override : fd.st->u;
  const bool stamp = (c == 8 && blockIdx.y == 0 && d == 1);
  SLM_STAMP(fd, stamp, 0);
  const size_t col = (size_t)c * (fd.wb + 1);
  double* At = fd.band + (col + d) * TILE;
  double* yv = fd.rhs + (size_t)c * NB;
  double4_t a[4];
  panel_column_stage(d, At, yv, fd.band + col * TILE, c * NB, fd.P, u, S, vec, a);
  SLM_STAMP(fd, stamp, 1);
  const bool ok = potrf64(S, dinv, wt, s_ok, fd, stamp);
  SLM_STAMP(fd, stamp, 14);
  if (d == 0) {
    if (!ok && threadIdx.x == 0) fd.st->chol_fail = 1;
    // full inverse of the diagonal block: used by the substitutions (one parallel matvec each)
    inverse_assemble64(S, M, dinv, wt);
  }
  panel_column_finish(d, At, yv, fd.linv + (size_t)c * TILE, S, M, dinv, vec, a);
  SLM_STAMP(fd, stamp, 15);
}

// grid = (wb_cap*(wb_cap+1)/2 + wb_cap, n_frames)
__global__ void __launch_bounds__(256) k_trail(const FrameDev* __restrict__ frames, int c,
                                                int wb_cap) {
  __shared__ double Bl[TILE];
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped || c >= fd.nt) return;
  const int ntri = wb_cap * (wb_cap + 1) / 2;
  int t = blockIdx.x;
  const size_t col = (size_t)c * (fd.wb + 1);
  if (t < ntri) {
    // (a,b), 1 <= b <= a <= wb_cap, row-major over the lower triangle
    int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((a + 1) * (a + 2) / 2 <= t) ++a;
    while (a * (a + 1) / 2 > t) --a;
    const int b = t - a * (a + 1) / 2;
    const int da = a + 1, db = b + 1;
    if (da > fd.wb || c + da >= fd.nt) return;
    // A(c+da, c+db) -= L(c+da, c) L(c+db, c)^T
    tile_product<true, false, true>(fd.band + (col + db) * TILE, fd.band + (col + da) * TILE,
                                    fd.band + ((size_t)(c + db) * (fd.wb + 1) + (da - db)) * TILE, Bl);
  } else {
    // rhs: b_s -= L(s,c) y_c, s = c + db
    const int db = t - ntri + 1;
    if (db > fd.wb || c + db >= fd.nt) return;
    __shared__ double y[NB];
    __shared__ double part[4 * NB];
    trail_rhs(fd.band + (col + db) * TILE, fd.rhs + (size_t)c * NB, fd.rhs + (size_t)(c + db) * NB, y, part);
  }
}

// grid = (wb_cap + 1, n_frames)
__global__ void __launch_bounds__(256) k_backsub(const FrameDev* __restrict__ frames, int c_from_end) {
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped) return;
  const int c = fd.nt - 1 - c_from_end;
  if (c < 0) return;
  const int d = blockIdx.x;
  if (d > fd.wb || c - d < 0) return;
  __shared__ double y[NB];
  __shared__ double x[NB];
  __shared__ double part[4 * NB];
  backsub_x(fd.linv + (size_t)c * TILE, fd.rhs + (size_t)c * NB, y, x, part);
  if (d == 0) {
    if (threadIdx.x < NB) fd.delta[(size_t)c * NB + threadIdx.x] = x[threadIdx.x];
  } else {
    // tile (c, c-d) is at column c-d, offset d
    backsub_update(fd.band + ((size_t)(c - d) * (fd.wb + 1) + d) * TILE, x, fd.rhs + (size_t)(c - d) * NB);
  }
}

// Expand the assembled lower band to a dense symmetric (P,P) row-major matrix (parity tests).
__global__ void __launch_bounds__(256) k_band_to_dense(const FrameDev* __restrict__ frames, int slot,
                                                        double* __restrict__ out) {
  const FrameDev& fd = frames[slot];
  const size_t P = fd.P;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < P * P;
       e += (size_t)gridDim.x * blockDim.x) {
    int i = (int)(e / P), j = (int)(e % P);
    int hi = max(i, j), lo = min(i, j);
    double v = 0.0;
    if (hi / NB - lo / NB <= fd.wb) v = *band_entry(fd, hi, lo);
    out[e] = v;
  }
}

// Pack a dense symmetric (P,P) row-major matrix into the (full-width) band (slm_solve_dense).
__global__ void __launch_bounds__(256) k_dense_to_band(const FrameDev* __restrict__ frames,
                                                        const double* __restrict__ A,
                                                        const double* __restrict__ b) {
  const FrameDev& fd = frames[0];
  const size_t P = fd.P, Ppad = (size_t)fd.nt * NB;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < Ppad * Ppad;
       e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / Ppad), j = (int)(e % Ppad);
    if (i < j) continue;
    *band_entry(fd, i, j) = (i < (int)P && j < (int)P) ? A[(size_t)i * P + j] : 0.0;
  }
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < Ppad;
       e += (size_t)gridDim.x * blockDim.x)
    fd.rhs[e] = e < P ? b[e] : 0.0;
}

// ---- host launchers --------------------------------------------------------------
void launch_dense_to_band(const FrameDev* frames_dev, const double* A, const double* b,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_dense_to_band, dim3(1024), dim3(256), 0, st, frames_dev, A, b);
}

void launch_bandwidth(const slm_frame& f, int* out_dev, hipStream_t st) {
  (void)hipMemsetAsync(out_dev, 0, 2 * sizeof(int), st);
  hipLaunchKernelGGL(k_bandwidth, dim3(256), dim3(256), 0, st, f, out_dev);
}

// Factor + forward substitution + back substitution for all frames; nt_max / wb_cap are
// the maxima over the batch (blocks beyond a frame's own nt / wb exit immediately).
void launch_band_solve(const FrameDev* frames_dev, int n_frames, int nt_max, int wb_cap,
                       double u_override, hipStream_t st) {
  const size_t lds = PANEL_LDS_DOUBLES * sizeof(double);
  if (!ensure_dynamic_lds((const void*)k_panel, lds)) return;   // (sticky HIP error: the caller's hipGetLastError reports it)
  const int ntrail = wb_cap * (wb_cap + 1) / 2 + wb_cap;
  for (int c = 0; c < nt_max; ++c) {
    hipLaunchKernelGGL(k_panel, dim3(wb_cap + 1, n_frames), dim3(256), lds, st, frames_dev, c,
                       u_override);
    if (ntrail > 0)
      hipLaunchKernelGGL(k_trail, dim3(ntrail, n_frames), dim3(256), 0, st, frames_dev, c, wb_cap);
  }
  for (int e = 0; e < nt_max; ++e)
    hipLaunchKernelGGL(k_backsub, dim3(wb_cap + 1, n_frames), dim3(256), 0, st, frames_dev, e);
}

void launch_band_to_dense(const FrameDev* frames_dev, int slot, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_band_to_dense, dim3(1024), dim3(256), 0, st, frames_dev, slot, out);
}
