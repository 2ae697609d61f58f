// slm_corr.hip -- flow-correspondence term of the LM path (slm_enable_corr, include/super_lm.h; the reference left it as a
// commented-out CorrLoss in super/LM.py:27-29, GraphFit carries it: slm_gf.hip gf_corr).
//
//   k_corr_targets      : the frozen targets of a slot from an optical flow, as GraphFit's term reads them at zero deformation
//   k_corr_grad_pairs   : J^T J blocks and J^T r of the term into the pair records (pairbuf) of the K-generic data path,
//                         between k_data_grad_pairs and k_pair_scatter
//   k_corr_grad         : the same into the band with per-entry atomics (slm_assemble, slots without a multifrontal plan)
//   k_corr_loss         : sum_valid |r|^2 at beta or at the trial point, per-block partials behind the regularisers'
//                         (read out for slm_corr_loss by k_term_loss_out, slm_misc.hip)
//
// Residuals (lambda = weight): mode 1 r = lambda (T(p) - o), three rows lambda [w_k c^T dR(q_k)(p - g_k)/dq_k | w_k c] with
// c = e_x, e_y, e_z; mode 2 r = lambda n.(T(p) - o), the one row with c = n.  The targets do not move with beta: nothing
// comes through the projection, so a row is the data term's row (slm_data.h) with c in place of its c.
#include "slm_corr.h"
#include "slm_gf_sample.h"
#include "slm_host.h"
#include "slm_pairs.h"

// the skinning state of surfel i at the node table npk: neighbours, T(p) - o, the target normal
template <int KK>
struct CorrSkin : PairSkin<KK> {
  d3 e, n;
};
template <int KK>
__device__ __forceinline__ void corr_skin(const FrameDev& fd, const CorrDev& cd, const double* __restrict__ npk, int i, CorrSkin<KK>& s) {
  pair_skin<KK>(fd, npk, i, s);
  const d3 T = s.T;
  const double* o = cd.o.get() + 3 * (size_t)i;
  const double* n = cd.n.get() + 3 * (size_t)i;
  s.e = {T.x - o[0], T.y - o[1], T.z - o[2]};
  s.n = {n[0], n[1], n[2]};
}
// row number `comp` of the surfel: c (mode 1: the unit vector of the component; mode 2: the normal) and r = lambda c.e
__device__ __forceinline__ d3 corr_c(int mode, int comp, const d3 n) {
  if (mode == 2) return n;
  return {comp == 0 ? 1.0 : 0.0, comp == 1 ? 1.0 : 0.0, comp == 2 ? 1.0 : 0.0};
}

// grid = (ceil(N / 256)); the targets of slot `slot` from the flow (2,H,W)
__global__ void __launch_bounds__(256) k_corr_targets(const FrameDev* __restrict__ frames, const CorrDev* __restrict__ corr, int slot,
                                                       const float* __restrict__ flow) {
  const FrameDev& fd = frames[slot];
  const CorrDev& cd = corr[slot];
  const FrameIn& f = frame_in(fd);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.N) return;
  corr_target_of(f, i, flow, cd.o.get(), cd.n.get(), cd.valid.get());
}

// The term's share of the pair records: skin, the NC rows of a surfel with a correspondence (mode 1: the three components;
// mode 2: one) into the wave's LDS, then the run Gram -- the design and the record order are above PairLds (slm_pairs.h).
// The matched count behind the records (SLM_VK_TAIL) is the ICP term's: not touched here.
// grid = (ceil(max N / 64), n_frames), ONE wave per workgroup
template <int KK, int NC>
__global__ void __launch_bounds__(64) k_corr_grad_pairs(const FrameDev* __restrict__ frames, const CorrDev* __restrict__ corr,
                                                         double lam) {
  typedef PairLds<KK, NC> L;
  constexpr int MODE = NC == 3 ? 1 : 2;
  __shared__ L lds;
  const FrameDev& fd = frames[blockIdx.y];
  const CorrDev& cd = corr[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK || !fd.vk_ready || !cd.has) return;
  const int l = threadIdx.x;
  const int pos = blockIdx.x * 64 + l;
  bool on = false;
  int i = 0;
  if (pos < fd.f.N) {
    i = fd.sf_perm[pos];
    on = cd.valid[i] != 0;
  }
  const unsigned long long m = __ballot(on);
  if (!m) return;
  pair_zero_rows(lds, l);
  if (on) {
    CorrSkin<KK> sk;
    corr_skin<KK>(fd, cd, fd.node_pk, i, sk);
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      const int rank = pair_rank<KK>(sk.id, k);
      lds.s_cid[l * KK + rank] = sk.id[k];
      const double lw = lam * sk.w[k];
#pragma unroll
      for (int comp = 0; comp < NC; ++comp) {
        const d3 c = corr_c(MODE, comp, sk.n);
        double jq[4];
        quat_jac_row(sk.qw[k], sk.qv[k], sk.dk[k], c, jq);
        double* rw = lds.s_row + (NC * l + comp) * L::LDR + 7 * rank;
        rw[0] = lw * jq[0];
        rw[1] = lw * jq[1];
        rw[2] = lw * jq[2];
        rw[3] = lw * jq[3];
        rw[4] = lw * c.x;
        rw[5] = lw * c.y;
        rw[6] = lw * c.z;
      }
    }
#pragma unroll
    for (int comp = 0; comp < NC; ++comp) lds.s_row[(NC * l + comp) * L::LDR + L::NR] = lam * dot(corr_c(MODE, comp, sk.n), sk.e);
    pair_load_pidx(lds, fd, l, i);
  }
  pair_gram(lds, fd.pairbuf, on, m);
}

// per-entry form (k_data_grad's sums): row^T row into the lower band, -row^T r into rhs.  The row and its node ids sit in
// LDS (one odd-strided line per thread), so the two entry loops index them without scratch.
// grid = (ceil(maxN / 64), n_frames), 64 threads
template <int KK>
__global__ void __launch_bounds__(64) k_corr_grad(const FrameDev* __restrict__ frames, const CorrDev* __restrict__ corr, int mode,
                                                   double lam) {
  constexpr int NR = 7 * KK, LDW = NR | 1;
  __shared__ double s_row[64 * LDW];
  __shared__ int s_id[64 * KK];
  const FrameDev& fd = frames[blockIdx.y];
  const CorrDev& cd = corr[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK || !cd.has) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fd.f.N || !cd.valid[i]) return;
  CorrSkin<KK> sk;
  corr_skin<KK>(fd, cd, fd.node_pk, i, sk);
  double* row = s_row + threadIdx.x * LDW;   // (each thread reads back only what it wrote: no barrier)
  int* id = s_id + threadIdx.x * KK;
#pragma unroll
  for (int k = 0; k < KK; ++k) id[k] = sk.id[k];
  const int nc = mode == 1 ? 3 : 1;
#pragma unroll 1
  for (int comp = 0; comp < nc; ++comp) {
    const d3 c = corr_c(mode, comp, sk.n);
    const double r = lam * dot(c, sk.e);
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      double jq[4];
      quat_jac_row(sk.qw[k], sk.qv[k], sk.dk[k], c, jq);
      const double lw = lam * sk.w[k];
      row[7 * k + 0] = lw * jq[0];
      row[7 * k + 1] = lw * jq[1];
      row[7 * k + 2] = lw * jq[2];
      row[7 * k + 3] = lw * jq[3];
      row[7 * k + 4] = lw * c.x;
      row[7 * k + 5] = lw * c.y;
      row[7 * k + 6] = lw * c.z;
    }
    band_scatter_row<NR>(fd, id, row, r);
  }
}

// grid = (SLM_CORR_BLOCKS, n_frames); grid-stride over surfels.  Block b of a slot stores its sum as the pair b at corr_part
// (term_loss_store) and its kept count to reg[cnt_part + b], reg = the regularisers' partials; a slot without
// correspondences stores zeros.
template <int KK>
__global__ void __launch_bounds__(256) k_corr_loss(const FrameDev* __restrict__ frames, const CorrDev* __restrict__ corr, int mode,
                                                    double lam, int use_delta, int corr_part, int cnt_part) {
  __shared__ double sm[16];
  const FrameDev& fd = frames[blockIdx.y];
  const CorrDev& cd = corr[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK) return;
  double acc = 0.0;
  int cnt = 0;
  if (cd.has) {
    const double* npk = use_delta ? fd.node_pk_try : fd.node_pk;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < fd.f.N; i += gridDim.x * blockDim.x) {
      if (!cd.valid[i]) continue;
      CorrSkin<KK> sk;
      corr_skin<KK>(fd, cd, npk, i, sk);
      if (mode == 1) {
        acc += lam * lam * dot(sk.e, sk.e);
      } else {
        const double r = lam * dot(sk.n, sk.e);
        acc += r * r;
      }
      ++cnt;
    }
  }
  const double s = block_sum(acc, sm);
  const double c = block_sum((double)cnt, sm);
  if (threadIdx.x == 0) {
    term_loss_store(fd, corr_part, s);
    fd.loss_part[2 * (size_t)fd.n_loss_part + cnt_part + blockIdx.x] = c;
  }
}

// ---- host launchers (called from slm_lm.hip, slm_terms.hip) ------------------------------------
void launch_corr_targets(const FrameDev* frames_dev, const CorrDev* corr_dev, int slot, int N, const float* flow, hipStream_t st) {
  if (N <= 0) return;
  hipLaunchKernelGGL(k_corr_targets, dim3((N + 255) / 256), dim3(256), 0, st, frames_dev, corr_dev, slot, flow);
}

void launch_corr_grad_pairs(const FrameDev* frames_dev, const CorrDev* corr_dev, int n_frames, int max_pos, int K, int mode, double lam,
                            hipStream_t st) {
  if (max_pos <= 0) return;
  const dim3 grid((max_pos + 63) / 64, n_frames);
  if (mode == 1) {
    SLM_K_DISPATCH(K, hipLaunchKernelGGL((k_corr_grad_pairs<KK, 3>), grid, dim3(64), 0, st, frames_dev, corr_dev, lam));
  } else {
    SLM_K_DISPATCH(K, hipLaunchKernelGGL((k_corr_grad_pairs<KK, 1>), grid, dim3(64), 0, st, frames_dev, corr_dev, lam));
  }
}

void launch_corr_grad(const FrameDev* frames_dev, const CorrDev* corr_dev, int n_frames, int maxN, int K, int mode, double lam,
                      hipStream_t st) {
  if (maxN <= 0) return;
  const dim3 grid((maxN + 63) / 64, n_frames);
  SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_corr_grad<KK>, grid, dim3(64), 0, st, frames_dev, corr_dev, mode, lam));
}

void launch_corr_loss(const FrameDev* frames_dev, const CorrDev* corr_dev, int n_frames, int K, int mode, double lam, int use_delta,
                      int corr_part, int cnt_part, hipStream_t st) {
  const dim3 grid(SLM_CORR_BLOCKS, n_frames);
  SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_corr_loss<KK>, grid, dim3(256), 0, st, frames_dev, corr_dev, mode, lam, use_delta, corr_part,
                                       cnt_part));
}
