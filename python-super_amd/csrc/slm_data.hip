// slm_data.hip -- data-term passes (point-to-plane ICP), v0: one thread per surfel.
//
//   k_data_grad   : JtJ (lower band) and jtl = -Jt r accumulation  (loss.py:222-288)
//   k_data_grad_pairs : the same into the pair records of the multifrontal path (num_neighbors != 4); the wave's Gram
//                       is pair_gram, slm_pairs.h
//   k_data_loss   : sum r^2 at beta (+ delta), fresh match set     (loss.py:222-255,290)
//   k_data_resid  : per-surfel r / match / taps for parity tests
//   k_data_weights: per-surfel weight of an enabled solver (slm_data_weights)
//
// Weighted variants (slm_enable_data_weights): k_data_grad, k_data_loss and k_data_grad_pairs take a trailing parameter
// pack W; instantiated with W = DataWArgs they evaluate the per-residual weight w at the point of the pass (data_weight,
// slm_data.h) and use row sqrt(w), r sqrt(w) (Jacobian passes) or w r^2 (loss pass).  The matched counts do not change: a
// surfel with weight 0 is matched and contributes nothing.  With the empty pack the kernels are what they were.
#include "slm_data.h"
#include "slm_host.h"
#include "slm_launch.h"
#include "slm_pairs.h"

// surfel i at npk in a weighted launch (W = DataWArgs: the pack expands to this one argument): ev and wt = its weight; the
// slot's semantic descriptor sits at the slot's index, like its FrameDev
template <int MODE, int KK>
__device__ __forceinline__ void eval_surfel_weighted(const FrameDev& fd, double lam, const double* npk, int i, SurfelEvalT<KK>& ev,
                                                     double& wt, const DataWArgs& a) {
  eval_surfel_w<MODE, KK>(fd, lam, npk, i, ev, a, a.wd ? a.wd + blockIdx.y : nullptr, wt);
}

// grid = (ceil(maxN/256), n_frames); KK = opt.num_neighbors of every slot of the launch (a slot with another K is skipped:
// the launcher only sees the batch's common value)
template <int KK, typename... W>
__global__ void __launch_bounds__(256) k_data_grad(const FrameDev* __restrict__ frames, double lam, W... wa) {
  constexpr bool WT = sizeof...(W) > 0;
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  SurfelEvalT<KK> ev;
  ev.match = false;
  [[maybe_unused]] double wt = 1.0;
  // [sf_lo, sf_hi) = all surfels unless the frame is sharded over several GPUs (slm_assemble on a sharded handle: the
  // rank's share in the caller's order, as k_data_loss has it)
  const bool mine = i >= fd.sf_lo && i < fd.sf_hi;
  if constexpr (WT) {
    if (mine) eval_surfel_weighted<1, KK>(fd, lam, fd.node_pk, i, ev, wt, wa...);
  } else {
    if (mine) eval_surfel<1, KK>(fd, lam, fd.node_pk, i, ev);
  }

  // matched-surfel count: one atomic per wave
  unsigned long long m = __ballot(ev.match);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&fd.st->m_grad, __popcll(m));
  if (!ev.match) return;
  if constexpr (WT) {
    // Launched with 64 threads (launch_data_grad): the scaled row and its node ids sit in LDS, one odd-strided line per
    // thread, so the two entry loops index them without scratch (as k_corr_grad, slm_corr.hip).
    constexpr int NR = 7 * KK, LDW = NR | 1;
    __shared__ double s_row[64 * LDW];
    __shared__ int s_id[64 * KK];
    if (wt == 0.0) return;   // (counted above: matched, contributes nothing)
    const double sw = sqrt(wt), r = ev.r * sw;
    double* row = s_row + threadIdx.x * LDW;   // (each thread reads back only what it wrote: no barrier)
    int* id = s_id + threadIdx.x * KK;
#pragma unroll
    for (int k = 0; k < KK; ++k) id[k] = ev.id[k];
#pragma unroll
    for (int a = 0; a < NR; ++a) row[a] = ev.row[a] * sw;
    band_scatter_row<NR>(fd, id, row, r);
    return;
  }
  band_scatter_row<7 * KK>(fd, ev.id, ev.row, ev.r);   // (256 threads, the private row)
}

// grid = (n_loss_blocks, n_frames); grid-stride over surfels; partial sums per block
template <int KK, typename... W>
__global__ void __launch_bounds__(256) k_data_loss(const FrameDev* __restrict__ frames, double lam,
                                                    int use_delta, W... wa) {
  __shared__ double sm[16];
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK) return;
  double acc = 0.0;
  int cnt = 0;
  // [sf_lo, sf_hi) = all surfels unless the frame is sharded over several GPUs
  for (int i = fd.sf_lo + blockIdx.x * blockDim.x + threadIdx.x; i < fd.sf_hi; i += gridDim.x * blockDim.x) {
    SurfelEvalT<KK> ev;
    if constexpr (sizeof...(W) > 0) {   // w r^2, w fresh at this point; the count stays the match set's
      double wt;
      eval_surfel_weighted<0, KK>(fd, lam, use_delta ? fd.node_pk_try : fd.node_pk, i, ev, wt, wa...);
      if (ev.match) {
        acc += wt * (ev.r * ev.r);
        ++cnt;
      }
      continue;
    }
    eval_surfel<0, KK>(fd, lam, use_delta ? fd.node_pk_try : fd.node_pk, i, ev);
    if (ev.match) {
      acc += ev.r * ev.r;
      ++cnt;
    }
  }
  double s = block_sum(acc, sm);
  double c = block_sum((double)cnt, sm);
  if (threadIdx.x == 0) {
    fd.loss_part[2 * blockIdx.x] = s;
    fd.loss_part[2 * blockIdx.x + 1] = c;
  }
}

template <int KK>
__global__ void __launch_bounds__(256) k_data_resid(const FrameDev* __restrict__ frames, int slot,
                                                     double lam, double* __restrict__ r_out,
                                                     uint8_t* __restrict__ match_out,
                                                     int32_t* __restrict__ taps_out) {
  const FrameDev& fd = frames[slot];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fd.f.N) return;
  SurfelEvalT<KK> ev;
  eval_surfel<0, KK>(fd, lam, fd.node_pk, i, ev);
  if (r_out) r_out[i] = ev.match ? ev.r : 0.0;
  if (match_out) match_out[i] = ev.match ? 1 : 0;
  if (taps_out) {
    taps_out[4 * i + 0] = ev.taps[0];
    taps_out[4 * i + 1] = ev.taps[1];
    taps_out[4 * i + 2] = ev.taps[2];
    taps_out[4 * i + 3] = ev.taps[3];
  }
}

// the weight of every surfel of slot `slot` at its current beta, 0 for unmatched surfels (slm_data_weights)
template <int KK>
__global__ void __launch_bounds__(256) k_data_weights(const FrameDev* __restrict__ frames, int slot, double lam, DataWArgs wa,
                                                       double* __restrict__ w_out) {
  const FrameDev& fd = frames[slot];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fd.f.N) return;
  SurfelEvalT<KK> ev;
  double wt;
  eval_surfel_w<0, KK>(fd, lam, fd.node_pk, i, ev, wa, wa.wd ? wa.wd + slot : nullptr, wt);
  w_out[i] = ev.match ? wt : 0.0;
}

// ---- K-generic data term on the multifrontal path (num_neighbors != 4) ------------------------------------------------
// The data term's share of the pair records: evaluate, count the matched, the rows (scaled by sqrt(w) when weighted) into
// the wave's LDS, then the run Gram -- the design, the record order and the measurements are above PairLds (slm_pairs.h).
// grid = (ceil(max positions / 64), n_frames), ONE wave per workgroup
template <int KK, typename... W>
__global__ void __launch_bounds__(64) k_data_grad_pairs(const FrameDev* __restrict__ frames, double lam, W... wa) {
  constexpr bool WT = sizeof...(W) > 0;
  typedef PairLds<KK, 1> L;
  __shared__ L lds;
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK || !fd.vk_ready) return;
  const int l = threadIdx.x;
  const int pos = fd.sf_lo + blockIdx.x * 64 + l;   // [sf_lo, sf_hi): all positions unless the frame is sharded over several GPUs
  SurfelEvalT<KK> ev;
  ev.match = false;
  int i = 0;
  [[maybe_unused]] double sw = 1.0;   // sqrt of the surfel's weight
  if (pos < fd.sf_hi) {
    i = fd.sf_perm[pos];
    if constexpr (WT) {
      double wt;
      eval_surfel_weighted<1, KK>(fd, lam, fd.node_pk, i, ev, wt, wa...);
      sw = sqrt(wt);
    } else {
      eval_surfel<1, KK>(fd, lam, fd.node_pk, i, ev);
    }
  }
  const unsigned long long m = __ballot(ev.match);
  if (!m) return;
  // the matched count rides behind the records, spread over SLM_VK_TAIL doubles (k_pair_scatter sums them into m_grad)
  if (l == 0) atomic_add_f64(fd.pairbuf + (size_t)fd.n_blocks * SLM_WREC + (blockIdx.x % SLM_VK_TAIL), (double)__popcll(m));
  pair_zero_rows(lds, l);
  if (ev.match) {
    double* rw = lds.s_row + l * L::LDR;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      const int rank = pair_rank<KK>(ev.id, k);
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        if constexpr (WT) rw[7 * rank + c] = ev.row[7 * k + c] * sw;   // (weight 0: a zero row of the wave's Gram)
        else rw[7 * rank + c] = ev.row[7 * k + c];
      }
      lds.s_cid[l * KK + rank] = ev.id[k];
    }
    if constexpr (WT) rw[L::NR] = ev.r * sw;
    else rw[L::NR] = ev.r;
    pair_load_pidx(lds, fd, l, i);
  }
  pair_gram(lds, fd.pairbuf, ev.match, m);
}

// zero the pair records (+ the matched count behind them) of the slots that take the K-generic pair path
__global__ void __launch_bounds__(256) k_zero_pairbuf(const FrameDev* __restrict__ frames) {
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || !fd.vk_ready || !fd.pairbuf || fd.st->stopped) return;
  const size_t n = (size_t)fd.n_blocks * SLM_WREC + SLM_VK_TAIL;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) fd.pairbuf[e] = 0.0;
}

// ---- host launchers (called from slm_api.hip) ------------------------------------
// K = the batch's num_neighbors (1..SLM_KMAX): one instantiation per value (SLM_K_DISPATCH, slm_host.h)
// wa: the weighted variant (an enabled solver), else null
void launch_data_grad(const FrameDev* frames_dev, int n_frames, int maxN, int K, double lam, hipStream_t st, const DataWArgs* wa) {
  if (maxN <= 0) return;
  dim3 grid((maxN + 255) / 256, n_frames);
  if (wa) {   // (64 threads: the weighted variant keeps its rows in LDS)
    const dim3 grid_w((maxN + 63) / 64, n_frames);
    SLM_K_DISPATCH(K, hipLaunchKernelGGL((k_data_grad<KK, DataWArgs>), grid_w, dim3(64), 0, st, frames_dev, lam, *wa));
  } else {
    SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_data_grad<KK>, grid, dim3(256), 0, st, frames_dev, lam));
  }
}

void launch_data_loss(const FrameDev* frames_dev, int n_frames, int n_blocks, int K, double lam, int use_delta, hipStream_t st,
                      const DataWArgs* wa) {
  dim3 grid(n_blocks, n_frames);
  if (wa) {
    SLM_K_DISPATCH(K, hipLaunchKernelGGL((k_data_loss<KK, DataWArgs>), grid, dim3(256), 0, st, frames_dev, lam, use_delta, *wa));
  } else {
    SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_data_loss<KK>, grid, dim3(256), 0, st, frames_dev, lam, use_delta));
  }
}

void launch_data_weights(const FrameDev* frames_dev, int slot, int N, int K, double lam, const DataWArgs& wa, double* w, hipStream_t st) {
  if (N <= 0) return;
  SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_data_weights<KK>, dim3((N + 255) / 256), dim3(256), 0, st, frames_dev, slot, lam, wa, w));
}

void launch_data_resid(const FrameDev* frames_dev, int slot, int N, int K, double lam, double* r, uint8_t* match, int32_t* taps,
                       hipStream_t st) {
  if (N <= 0) return;
  SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_data_resid<KK>, dim3((N + 255) / 256), dim3(256), 0, st, frames_dev, slot, lam, r, match, taps));
}

// the K-generic Jacobian pass of the multifrontal path: pair records zeroed, then filled (max_pos = the batch's largest surfel count)
void launch_data_grad_pairs(const FrameDev* frames_dev, int n_frames, int max_pos, int K, double lam, hipStream_t st,
                            const DataWArgs* wa) {
  if (max_pos <= 0) return;
  hipLaunchKernelGGL(k_zero_pairbuf, dim3(128, n_frames), dim3(256), 0, st, frames_dev);
  dim3 grid((max_pos + 63) / 64, n_frames);
  if (wa) {
    SLM_K_DISPATCH(K, hipLaunchKernelGGL((k_data_grad_pairs<KK, DataWArgs>), grid, dim3(64), 0, st, frames_dev, lam, *wa));
  } else {
    SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_data_grad_pairs<KK>, grid, dim3(64), 0, st, frames_dev, lam));
  }
}
