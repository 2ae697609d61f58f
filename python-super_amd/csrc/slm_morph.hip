// slm_morph.hip -- semantic boundary-morph term of the LM path (slm_enable_morph, include/super_lm.h; the reference has only
// the first-order form, super/deform_mesh.py:126-194, which GraphFit carries: k_gf_morph, slm_sem.hip).
//
//   k_morph_select      : which surfels the term keeps at beta or at the trial point, their targets m_i and l_i, and per
//                         block the partial sums of l_i, kept and candidates (the class sampling, the search and the keep
//                         test are k_gf_morph's: slm_sem_search.h)
//   k_morph_fold        : per slot the sums of those partials in a fixed order, the kept count n for the Jacobian pass and
//                         the term's loss lambda^2 / n sum l_i as its pair of the loss partials (LossParts, slm_solver.h)
//   k_morph_grad_pairs  : J^T J blocks and J^T r of the term into the pair records (pairbuf) of the K-generic data path,
//                         between k_data_grad_pairs and k_pair_scatter
//   k_morph_grad        : the same into the band with per-entry atomics (slm_assemble, slots without a multifrontal plan)
//
// A kept surfel i projects to (x, y) = (fx T.x / Ze + cx, fy T.y / Ze + cy), Ze = T.z + 1e-8, T = T_i(beta), and is pulled
// towards m_i = (e1 + e2) / 2, the mean of the two nearest boundary pixels of its own class: two rows
// r = lambda / sqrt(n) ((x, y) - m_i), lambda / sqrt(n) [w_k c^T dR(q_k)(p - g_k)/dq_k | w_k c] with c = d x / d T and
// d y / d T -- the correspondence term's rows (slm_corr.hip) with this c.  The selection, the targets and n are constants of
// the linearisation; the loss is the reference's: lambda^2 / n sum_kept l_i with l_i = (d1 + d2) / 2 =
// |(x, y) - m_i|^2 + |e1 - e2|^2 / 4, evaluated afresh (new selection, new n) wherever it is asked for.  n = 0: no rows and
// a loss of 0 (the reference's mean over nothing is NaN, which would reject every step).
#include "slm_gf_sample.h"
#include "slm_host.h"
#include "slm_morph.h"
#include "slm_pairs.h"
#include "slm_sem_search.h"

namespace {
// rows of a kept surfel at the skinning state sk: c and the residual of component comp (0: x, 1: y), unscaled
struct MorphRows {
  d3 c[2];
  double r[2];
};
__device__ __forceinline__ MorphRows morph_rows(const FrameIn& f, const MorphDev& md, int i, const d3 T) {
  const GfProj pr = gf_project(f, T);
  const double* m = md.target.get() + 2 * (size_t)i;
  MorphRows o;
  o.c[0] = pr.Pi0;
  o.c[1] = pr.Pi1;
  o.r[0] = pr.u - m[0];
  o.r[1] = pr.v - m[1];
  return o;
}
// lambda / sqrt(n) of the slot's last selection (n >= 1 wherever a surfel is kept)
__device__ __forceinline__ double morph_scale(const MorphDev& md, double lam) { return lam / sqrt(md.stat[1]); }
}  // namespace

// grid = (ceil(max N / 256), n_frames)
template <int KK>
__global__ void __launch_bounds__(256) k_morph_select(const FrameDev* __restrict__ frames, const MorphDev* __restrict__ morph,
                                                       int use_delta) {
  __shared__ double sm[16];
  __shared__ SemCandLds cand;
  const FrameDev& fd = frames[blockIdx.y];
  const MorphDev& md = morph[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK || !md.has) return;
  const FrameIn& f = frame_in(fd);
  if (blockIdx.x * 256 >= f.N) return;   // (the fold reads the ceil(N / 256) partials of the slot's own blocks)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int H = f.H, W = f.W;
  if (threadIdx.x == 0) cand.n_cand = 0;
  __syncthreads();
  int my_cand = -1;
  double my_x = 0.0, my_y = 0.0;
  if (i < f.N) {
    PairSkin<KK> sk;
    pair_skin<KK>(fd, use_delta ? fd.node_pk_try : fd.node_pk, i, sk);
    const GfProj pr = gf_project(f, sk.T);
    const double x = pr.u, y = pr.v;
    double gx, gy;
    const int best = sem_sample_class(md.img_seg_conf, md.C, H, W, x, y, gx, gy);
    const int cls = md.sf_seg[i];
    const bool val = best != cls && gx > -1.0 && gx < 1.0 && gy > -1.0 && gy < 1.0;
    if (val && cls >= 0 && cls < md.C) {
      const int e0 = md.edge_off[cls], e1 = md.edge_off[cls + 1];
      if (e1 - e0 >= 2) {   // a single boundary pixel has no 2nd neighbour: treated as no boundary
        const int k = atomicAdd(&cand.n_cand, 1);
        cand.x[k] = x;
        cand.y[k] = y;
        cand.e0[k] = e0;
        cand.e1[k] = e1;
        my_cand = k;
        my_x = x;
        my_y = y;
      }
    }
  }
  __syncthreads();
  sem_search_candidates(cand, md.edge_xy);
  __syncthreads();
  double li_sum = 0.0, kept = 0.0;
  if (i < f.N) {
    double mx = 0.0, my = 0.0, li = 0.0;
    bool keep = false;
    if (my_cand >= 0) {
      const float2 p1 = md.edge_xy[cand.i1[my_cand]], p2 = md.edge_xy[cand.i2[my_cand]];
      keep = sem_morph_keep(my_x, my_y, W, H, cand.d1[my_cand], cand.d2[my_cand], li);
      if (keep) {
        mx = ((double)p1.x + (double)p2.x) / 2.0;
        my = ((double)p1.y + (double)p2.y) / 2.0;
        li_sum = li;
        kept = 1.0;
      }
    }
    md.kept[i] = keep ? 1 : 0;
    md.target[2 * (size_t)i] = mx;
    md.target[2 * (size_t)i + 1] = my;
    md.li[i] = keep ? li : 0.0;
  }
  // (small-integer counts in doubles stay exact; every sum below is in a fixed order)
  const double a = block_sum(li_sum, sm), b = block_sum(kept, sm), c = block_sum(my_cand >= 0 ? 1.0 : 0.0, sm);
  if (threadIdx.x == 0) {
    double* part = md.part.get() + 3 * (size_t)blockIdx.x;
    part[0] = a;
    part[1] = b;
    part[2] = c;
  }
}

// n is not known until every block of the selection is done: one workgroup per slot in a launch of its own behind it.
// grid = (1, n_frames).  A slot without the term's inputs stores a loss of zero.
__global__ void __launch_bounds__(256) k_morph_fold(const FrameDev* __restrict__ frames, const MorphDev* __restrict__ morph, double lam,
                                                     int morph_part, double* __restrict__ out) {
  __shared__ double sm[16];
  const FrameDev& fd = frames[blockIdx.y];
  const MorphDev& md = morph[blockIdx.y];
  if (!fd.bound || fd.st->stopped) return;
  double a = 0.0, b = 0.0, c = 0.0;
  if (md.has) {
    const int nb = (fd.f.N + 255) / 256;
    for (int t = threadIdx.x; t < nb; t += blockDim.x) {
      a += md.part[3 * (size_t)t];
      b += md.part[3 * (size_t)t + 1];
      c += md.part[3 * (size_t)t + 2];
    }
  }
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  c = block_sum(c, sm);
  if (threadIdx.x == 0) {
    const double loss = b > 0.0 ? lam * lam / b * a : 0.0;
    if (md.has) {
      md.stat[0] = a;
      md.stat[1] = b;
      md.stat[2] = c;
      md.stat[3] = loss;
    }
    if (morph_part >= 0) term_loss_store(fd, morph_part, loss);
    if (out) {
      out[0] = loss;
      out[1] = b;
      out[2] = c;
    }
  }
}

// The term's share of the pair records: k_corr_grad_pairs (slm_corr.hip) with NC = 2 and the projection's rows as c, over
// the surfels the selection kept.
// grid = (ceil(max N / 64), n_frames), ONE wave per workgroup
template <int KK>
__global__ void __launch_bounds__(64) k_morph_grad_pairs(const FrameDev* __restrict__ frames, const MorphDev* __restrict__ morph,
                                                          double lam) {
  typedef PairLds<KK, 2> L;
  __shared__ L lds;
  const FrameDev& fd = frames[blockIdx.y];
  const MorphDev& md = morph[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK || !fd.vk_ready || !md.has) return;
  const int l = threadIdx.x;
  const int pos = blockIdx.x * 64 + l;
  bool on = false;
  int i = 0;
  if (pos < fd.f.N) {
    i = fd.sf_perm[pos];
    on = md.kept[i] != 0;
  }
  const unsigned long long m = __ballot(on);
  if (!m) return;
  pair_zero_rows(lds, l);
  if (on) {
    const double sc = morph_scale(md, lam);
    PairSkin<KK> sk;
    pair_skin<KK>(fd, fd.node_pk, i, sk);
    const MorphRows mr = morph_rows(frame_in(fd), md, i, sk.T);
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      const int rank = pair_rank<KK>(sk.id, k);
      lds.s_cid[l * KK + rank] = sk.id[k];
      const double lw = sc * sk.w[k];
#pragma unroll
      for (int comp = 0; comp < 2; ++comp) {
        const d3 c = mr.c[comp];
        double jq[4];
        quat_jac_row(sk.qw[k], sk.qv[k], sk.dk[k], c, jq);
        double* rw = lds.s_row + (2 * l + comp) * L::LDR + 7 * rank;
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
    for (int comp = 0; comp < 2; ++comp) lds.s_row[(2 * l + comp) * L::LDR + L::NR] = sc * mr.r[comp];
    pair_load_pidx(lds, fd, l, i);
  }
  pair_gram(lds, fd.pairbuf, on, m);
}

// per-entry form (k_corr_grad's): row^T row into the lower band, -row^T r into rhs, through the shared band scatter.
// grid = (ceil(maxN / 64), n_frames), 64 threads
template <int KK>
__global__ void __launch_bounds__(64) k_morph_grad(const FrameDev* __restrict__ frames, const MorphDev* __restrict__ morph, double lam) {
  constexpr int NR = 7 * KK, LDW = NR | 1;
  __shared__ double s_row[64 * LDW];
  __shared__ int s_id[64 * KK];
  const FrameDev& fd = frames[blockIdx.y];
  const MorphDev& md = morph[blockIdx.y];
  if (!fd.bound || fd.st->stopped || fd.f.K != KK || !md.has) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fd.f.N || !md.kept[i]) return;
  const double sc = morph_scale(md, lam);
  PairSkin<KK> sk;
  pair_skin<KK>(fd, fd.node_pk, i, sk);
  const MorphRows mr = morph_rows(frame_in(fd), md, i, sk.T);
  double* row = s_row + threadIdx.x * LDW;   // (each thread reads back only what it wrote: no barrier)
  int* id = s_id + threadIdx.x * KK;
#pragma unroll
  for (int k = 0; k < KK; ++k) id[k] = sk.id[k];
#pragma unroll 1
  for (int comp = 0; comp < 2; ++comp) {
    const d3 c = comp == 0 ? mr.c[0] : mr.c[1];
    const double r = sc * (comp == 0 ? mr.r[0] : mr.r[1]);
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      double jq[4];
      quat_jac_row(sk.qw[k], sk.qv[k], sk.dk[k], c, jq);
      const double lw = sc * sk.w[k];
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

// ---- host launchers (called from slm_lm.hip, slm_terms.hip) ------------------------------------
void launch_morph_select(const FrameDev* frames_dev, const MorphDev* morph_dev, int n_frames, int maxN, int K, double lam, int use_delta,
                         int morph_part, double* out, hipStream_t st) {
  if (maxN > 0) {
    const dim3 grid((maxN + 255) / 256, n_frames);
    SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_morph_select<KK>, grid, dim3(256), 0, st, frames_dev, morph_dev, use_delta));
  }
  hipLaunchKernelGGL(k_morph_fold, dim3(1, n_frames), dim3(256), 0, st, frames_dev, morph_dev, lam, morph_part, out);
}

void launch_morph_grad_pairs(const FrameDev* frames_dev, const MorphDev* morph_dev, int n_frames, int max_pos, int K, double lam,
                             hipStream_t st) {
  if (max_pos <= 0) return;
  const dim3 grid((max_pos + 63) / 64, n_frames);
  SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_morph_grad_pairs<KK>, grid, dim3(64), 0, st, frames_dev, morph_dev, lam));
}

void launch_morph_grad(const FrameDev* frames_dev, const MorphDev* morph_dev, int n_frames, int maxN, int K, double lam, hipStream_t st) {
  if (maxN <= 0) return;
  const dim3 grid((maxN + 63) / 64, n_frames);
  SLM_K_DISPATCH(K, hipLaunchKernelGGL(k_morph_grad<KK>, grid, dim3(64), 0, st, frames_dev, morph_dev, lam));
}
