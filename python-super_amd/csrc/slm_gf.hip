// slm_gf.hip -- the reference's default per-frame optimiser (GraphFit, autograd + SGD/Adam,
// super/deform_mesh.py:198-379) with hand-derived gradients, entirely on the device.
//
// Parameters: dv (J+1,7), rows 0..J-1 local warps, row J the global transform T_g = (q_g,b_g).
//   surfel:  T(p) = sum_k w_k [R(q_k)(p-g_k) + b_k + g_k],   P = R(q_g) T(p) + b_g
//   node:    V_j  = R(q_g)(g_j + b_j) + b_g
// Losses (super/deform_mesh.py:25-196, super/loss.py:293-401,458-473,502-505):
//   point-plane  w_d sum (n.(P-o))^2   margin-1 validity on rounded coords, all 4 taps mapped
//   ARAP         w_a sum_jk w^ED_jk |R(q_k)d + b_k - f32(d) - b_j|^2   (f32-rounded d: loss.py:468)
//   Rot          w_r sum_{rows 0..J} (1 - |q|^2)^2
//   face         w_f sum_tri (area(V) - area0)^2,  area = 1/2 sqrt(|e1 x e2|^2 + 1e-13)
// Gradient of the global row is divided by J before the step (deform_mesh.py:326).
// Local rows: summed per workgroup in an LDS table, then one f64 atomic per entry and touched node; the global row is reduced per block first.
//
// Layout of this file: k_gf_zero / k_gf_fold; the stages of k_gf_data, each a function with its inputs and outputs in its
// signature (the samplers gf_sample / gf_flow_sample and gf_project come from slm_gf_sample.h; gf_sem_weight, gf_point_plane, gf_corr, gf_row_pass,
// gf_table_flush, gf_block_partials) and the kernel that runs them; the node terms (gf_reg_body); k_gf_step; bind / update
// kernels.  Host: gf_slot (every entry point's argument checks), gf_dims, gf_publish_pgrad, gf_upload_slot, gf_launch_step,
// gf_enqueue_morph / gf_enqueue_eval (the one evaluation sequence), then the entry points.
#include <cmath>
#include <string>
#include <vector>

#include "slm_host.h"
#include "slm_sem.h"
#include "slm_lane.h"
#include "slm_gf_sample.h"

__global__ void __launch_bounds__(256) k_gf_zero(GfSlot* __restrict__ slots) {
  GfSlotDev& s = gf_dev(slots)[blockIdx.y];
  if (!s.bound) return;
  const int n = (s.f.base.J + 1) * 7;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) s.grad[e] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x < SLM_GF_NTERMS) s.terms[threadIdx.x] = 0.0;
  if (blockIdx.x == 1 % gridDim.x)
    for (int e = threadIdx.x; e < GF_PART_DOUBLES; e += blockDim.x) s.terms[SLM_GF_NTERMS + e] = 0.0;
}

// the spread block partials (slm_gf.h) -> grad[7J + 0..6] and terms[], copies summed in a fixed order, then cleared.
// which: GfFoldWhich bits.  grid = (1, n_frames), 64 threads
__global__ void __launch_bounds__(64) k_gf_fold(GfSlot* __restrict__ slots, int which) {
  GfSlotDev& s = gf_dev(slots)[blockIdx.y];
  if (!s.bound) return;
  const int a = threadIdx.x;
  if (a >= GF_NPART) {   // (threads behind the partials' entries: no fold writes terms[5..7] in a launch with DROP_MORPH)
    if ((which & GF_FOLD_DROP_MORPH) && a < GF_NPART + 3) s.terms[5 + a - GF_NPART] = 0.0;
    return;
  }
  if (!(which & (a < GFP_MORPH_SUM ? GF_FOLD_DATA : GF_FOLD_MORPH))) return;
  const double t = gf_part_fold(s, a, true);
  if (t == 0.0) return;
  if (a < GFP_PP_LOSS) s.grad[7 * s.f.base.J + a] += t;
  else s.terms[gf_part_term(a)] += t;
}

struct GfRegArgs {
  int use_arap, use_rot, use_face, pad;
  double lam_a, lam_r, lam_f;
};
__device__ __forceinline__ void gf_reg_body(GfSlotDev& s, const int bx, const GfRegArgs ra, double* sm);

// What a k_gf_data launch is given, built once on the host (gf_enqueue_eval).  The EXTRA = false instantiation reads
// use_pp, lam, n_data_blocks and ra only.
struct GfDataArgs {
  int use_pp;          // the point-plane term is on
  int seg_mode;        // 0 none, 1 hard, 2 soft semantic weight on the squared residual (loss.py:379-399)
  int use_morph;       // adds the back-propagation of the morphing term prepared by k_gf_morph (2: the kept count is still
                       // in the spread partials)
  int corr_mode;       // 0 none, 1 'point-point', 2 'point-plane' flow-correspondence term
  int n_data_blocks;   // blocks [0, n_data_blocks) of a slot evaluate surfels; the blocks behind them, if any, run the node
                       // terms (gf_reg_body: independent work that only meets this kernel's in the gradient's atomics --
                       // slm_gf_run's loop saves a launch)
  int pad;
  double lam;          // weight of the point-plane term
  double pp_max;       // > 0 (and no seg_mode): squared residuals >= pp_max are dropped (loss.py:369-370)
  double w_morph, lam_c;
  GfRegArgs ra;
  const double* const* pgrad;   // per slot of the launch a bound (N,3) dL/dP or null, added where morph_g is; or null
};

// ---- the stages of k_gf_data, in the order the kernel runs them --------------------------------------------------------------

// G (n + s0 A + s1 B): dL/dP of a residual along n whose sample position moves with P by A = du/dP, B = dv/dP
__device__ __forceinline__ d3 gf_resid_grad(const double G, const d3 n, const double s0, const double s1, const d3 A, const d3 B) {
  return {G * (n.x + s0 * A.x + s1 * B.x), G * (n.y + s0 * A.y + s1 * B.y), G * (n.z + s0 * A.z + s1 * B.z)};
}

// the semantic weight of surfel i's squared residual: conf = the target's class scores at the sample (C of them).
// seg_mode 1: 1 where the surfel's class is the sample's, else 0; 2: exp(-0.1 JSD) of the two distributions.
__device__ __forceinline__ double gf_sem_weight(const GfSlotDev& s, const int i, const int seg_mode, const int C, const double* conf) {
  // sampled trg.seg_conf is softmaxed again (loss.py:357); weights are detached
  double mx = conf[0];
  int am = 0;
  for (int c = 1; c < C; ++c)
    if (conf[c] > mx) {
      mx = conf[c];
      am = c;
    }
  if (seg_mode == 1) return (s.sem.sf_seg[i] == am) ? 1.0 : 0.0;
  double q[SLM_MAX_CLASSES], den = 0.0;
  for (int c = 0; c < C; ++c) {
    q[c] = exp(conf[c] - mx);
    den += q[c];
  }
  // JSD(P, Q) = (KL(P|M) + KL(Q|M)) / 2, KL(P|Q) = sum P log(P / (Q + eps) + eps)  (utils.py:244-254)
  // (node_jsd of slm_nodes.h, kept inline: k_gf_data is register-bound under its launch bounds, Q is normalised in the loop)
  const double eps = 1e-13;
  double k1 = 0.0, k2 = 0.0;
  for (int c = 0; c < C; ++c) {
    const double pc = (double)s.sem.sf_seg_conf[(size_t)i * C + c], qc = q[c] / den;
    const double m = 0.5 * (pc + qc);
    k1 += pc * log(pc / (m + eps) + eps);
    k2 += qc * log(qc / (m + eps) + eps);
  }
  return exp(-0.1 * (0.5 * (k1 + k2)));
}

// the point-plane term of surfel i at P: true when its residual is kept, then loss = lam wgt r^2 and gP = its dL/dP
__device__ __forceinline__ bool gf_point_plane(const GfSlotDev& s, const int i, const d3 P, const GfProj& pr, const int seg_mode,
                                               const double pp_max, const double lam, double& loss, d3& gP) {
  const FrameIn& f = s.f.base;
  const double ur = rint(pr.u), vr = rint(pr.v);
  // valid_margin = 1 (loss.py:306-309)
  if (!(vr >= 1.0 && vr < (double)(f.H - 2) && ur >= 1.0 && ur < (double)(f.W - 2))) return false;
  GfSample q;
  if (!gf_sample(f, pr.u, pr.v, q)) return false;
  const d3 o = q.o, n = q.n, dou = q.dou, dov = q.dov, dnu = q.dnu, dnv = q.dnv;
  double conf[SLM_MAX_CLASSES] = {0, 0, 0, 0};
  const int C = (seg_mode && s.sem_bound) ? s.sem.num_classes : 0;
  for (int t = 0; t < 4; ++t)
    for (int c = 0; c < C; ++c) conf[c] += (double)s.sem.tgt_seg_conf[(size_t)q.rows[t] * C + c] * q.wv[t];
  const d3 e = P - o;
  const double r = dot(n, e);
  double wgt = 1.0;
  if (C > 0) wgt = gf_sem_weight(s, i, seg_mode, C, conf);
  else if (pp_max > 0.0 && !((r * r) < pp_max)) return false;
  loss = lam * wgt * r * r;
  // c = dr/dP
  const double s0 = dot(e, dnu) - dot(n, dou), s1 = dot(e, dnv) - dot(n, dov);
  gP = gf_resid_grad(2.0 * lam * wgt * r, n, s0, s1, pr.Pi0, pr.Pi1);
  return true;
}

// flow-correspondence term (opt.sf_corr, deform_mesh.py:100-109 -> loss.py:293-345 with flow): the UNROUNDED projection is moved
// by the flow sampled at it, validity is margin 1 on the moved float coordinates.  True when kept: lossc set, gP += its dL/dP
__device__ __forceinline__ bool gf_corr(const GfSlotDev& s, const d3 P, const GfProj& pr, const int corr_mode, const double lam_c,
                                        double& lossc, d3& gP) {
  const FrameIn& f = s.f.base;
  const int H = f.H, W = f.W;
  double fl[2], D[4];
  gf_flow_sample(s.flow, H, W, pr.u, pr.v, fl, D);
  const double uc = pr.u + fl[0], vc = pr.v + fl[1];
  if (!(vc >= 1.0 && vc < (double)(H - 2) && uc >= 1.0 && uc < (double)(W - 2))) return false;
  GfSample q;
  if (!gf_sample(f, uc, vc, q)) return false;
  // d(u', v')/dP = (I + dflow/d(u,v)) Pi
  const d3 Pi0 = pr.Pi0, Pi1 = pr.Pi1;
  const d3 Au = {(1.0 + D[0]) * Pi0.x + D[1] * Pi1.x, (1.0 + D[0]) * Pi0.y + D[1] * Pi1.y,
                 (1.0 + D[0]) * Pi0.z + D[1] * Pi1.z};
  const d3 Av = {D[2] * Pi0.x + (1.0 + D[3]) * Pi1.x, D[2] * Pi0.y + (1.0 + D[3]) * Pi1.y,
                 D[2] * Pi0.z + (1.0 + D[3]) * Pi1.z};
  const d3 e = P - q.o;
  d3 g;
  if (corr_mode == 1) {          // 'point-point': |P - o|^2
    lossc = lam_c * dot(e, e);
    g = gf_resid_grad(2.0 * lam_c, e, -dot(e, q.dou), -dot(e, q.dov), Au, Av);
  } else {                       // 'point-plane': (n.(P - o))^2
    const double r = dot(q.n, e);
    lossc = lam_c * r * r;
    g = gf_resid_grad(2.0 * lam_c * r, q.n, dot(e, q.dnu) - dot(q.n, q.dou), dot(e, q.dnv) - dot(q.n, q.dov), Au, Av);
  }
  gP = {gP.x + g.x, gP.y + g.y, gP.z + g.z};
  return true;
}

#define GF_TAB 128   // LDS gradient table: slots per workgroup (power of two)
// The local rows.  The 256 surfels of a workgroup are neighbours on the image and share a few dozen ED nodes: their
// gradient rows are summed in an LDS table keyed by node (tkey / tval, ds_add_f64) and flushed with one global
// atomic per entry and touched node (gf_table_flush) -- about 20x fewer memory-side f64 atomics than one per surfel
// and entry.  A slot taken by another node (direct-mapped, node & 127) falls back to global atomics.
// The WAVE turns round (round 6).  One LDS atomic per surfel, neighbour and entry -- 28 per surfel,
// most of them onto the few addresses the wave's surfels share -- serialised inside every instruction (k_gf_data was 8x
// slower per surfel than the LM path's evaluation pass).  Now the gradient rows of 16 surfels at a time go to LDS in
// canonical slot order (s_gval / s_gid, per wave) and lane e < 7 KK owns ENTRY (slot e / 7, component e % 7): it walks the
// surfels, accumulates in a register while the slot's node stays the same and adds to the workgroup's table when it changes
// -- one conflict-free add per run of surfels with a common node instead of one conflicting add per surfel.
// in: the surfel's skinning state k and cl = dL/dT(p) where has_grad
template <int KK>
__device__ __forceinline__ void gf_row_pass(GfSlotDev& s, const GfSkin<KK>& k, const d3 cl, const bool has_grad, int* tkey,
                                            double* tval, double (*s_gval)[16][7 * KK], int (*s_gid)[16][KK]) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long am = __ballot(has_grad);
  // WG entry-lane groups of 7 KK lanes share a round's 16 surfels (K = 4: lanes 0..27 walk surfels 0..7, lanes 28..55
  // surfels 8..15): half the steps per round for one more flush per lane and round
  constexpr int WG = (7 * KK <= 16) ? 4 : ((7 * KK <= 32) ? 2 : 1), WS = 16 / WG;
  const int grp = l / (7 * KK), el = l - 7 * KK * grp;   // group, entry inside the group
  const int slot = el / 7;
  double acc = 0.0;
  int prev = -1;
  auto flush = [&]() {
    if (prev < 0) return;
    const int ts = prev & (GF_TAB - 1);
    const int old = atomicCAS(&tkey[ts], -1, prev);
    if (old == -1 || old == prev) unsafeAtomicAdd(&tval[7 * ts + (el - 7 * slot)], acc);
    else atomic_add_f64(s.grad + 7 * prev + (el - 7 * slot), acc);
  };
  // K <= 4: every lane forms the quaternion parts of its K rows NOW, all 64 lanes at once (the node rows / positions are
  // read again -- cache hits -- and held: 8 K registers); only the staging goes 16 surfels at a time.  (Formed inside the
  // rounds by the 16 lanes of the round, the same instructions issued four times: 40 of the launch's 200 us at 8 C2 frames.)
  constexpr bool EAGER = KK <= 4;
  double jqa[EAGER ? KK : 1][4];
  if (EAGER && has_grad) {
    const FrameIn& f = s.f.base;
#pragma unroll
    for (int a = 0; a < (EAGER ? KK : 0); ++a) {
      const double* b = s.dv + 7 * k.id[a];
      const d3 g = ld_state3(f.ed_points, (size_t)k.id[a], f.state_f64);
      quat_jac_row(b[0], {b[1], b[2], b[3]}, k.p - g, cl, jqa[a]);
    }
  }
  if (!am) return;
#pragma unroll 1
  for (int sb = 0; sb < 4; ++sb) {
    const unsigned mask16 = (unsigned)((am >> (16 * sb)) & 0xFFFFull);
    if (mask16 == 0u) continue;                       // (uniform)
    if ((l >> 4) == sb && has_grad) {
      // this sub-batch's surfels form their rows now and write them straight to LDS (nothing per neighbour was held
      // across the sampling phase: the node rows / positions are read again -- cache hits)
      const FrameIn& f = s.f.base;
#pragma unroll
      for (int a = 0; a < KK; ++a) {
        double jq[4];
        if constexpr (EAGER) {
#pragma unroll
          for (int c = 0; c < 4; ++c) jq[c] = jqa[a][c];
        } else {
          const double* b = s.dv + 7 * k.id[a];
          const d3 g = ld_state3(f.ed_points, (size_t)k.id[a], f.state_f64);
          quat_jac_row(b[0], {b[1], b[2], b[3]}, k.p - g, cl, jq);
        }
        const double wk = k.w[a];
        // canonical slot of neighbour a: its rank among the surfel's node ids (two surfels with the same neighbour SET
        // have the same node in every slot, whatever the distance order of their KNN lists; the ids are distinct:
        // slm_gf_bind_frame refuses a row that repeats one)
        int rank = 0;
#pragma unroll
        for (int b2 = 0; b2 < KK; ++b2) rank += (k.id[b2] < k.id[a]) ? 1 : 0;
        s_gid[w][l & 15][rank] = k.id[a];
        double* dst = &s_gval[w][l & 15][7 * rank];
        dst[0] = wk * jq[0]; dst[1] = wk * jq[1]; dst[2] = wk * jq[2]; dst[3] = wk * jq[3];
        dst[4] = wk * cl.x;  dst[5] = wk * cl.y;  dst[6] = wk * cl.z;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (grp < WG) {
      for (unsigned mm = mask16 & (((1u << WS) - 1u) << (WS * grp)); mm; mm &= mm - 1) {
        const int si = __builtin_ctz(mm);
        const int id = s_gid[w][si][slot];
        const double v = s_gval[w][si][el];
        if (id != prev) {
          flush();
          prev = id;
          acc = v;
        } else {
          acc += v;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (grp < WG) flush();
}

// the workgroup's table -> the gradient: one global atomic per entry and touched node (behind a barrier)
__device__ __forceinline__ void gf_table_flush(GfSlotDev& s, const int* tkey, const double* tval) {
  for (int t = threadIdx.x; t < GF_TAB * 7; t += blockDim.x) {
    const int node = tkey[t / 7];
    const double v = tval[t];
    if (node >= 0 && v != 0.0) atomic_add_f64(s.grad + 7 * node + t % 7, v);
  }
}

// the block's sums of the first n_entries partial entries (vals: this thread's, by GfPart) -> its spread copy: one butterfly
// over the 16 values of a thread per wave (col_reduce16, slm_lane.h: lane 4 a holds the wave's sum of value a), the four waves'
// sums through LDS, then one atomic each (9 block_sums with two barriers each before: 19 of the launch's 215 us at 8 C2
// frames, tools/diag/gf_ablate_time.py)
__device__ __forceinline__ void gf_block_partials(GfSlotDev& s, double vals[GF_NPART], double* s_part, const int n_entries) {
  const double r = col_reduce16(vals);
  const int l = threadIdx.x & 63;
  if ((l & 3) == 0) s_part[(threadIdx.x >> 6) * 16 + (l >> 2)] = r;
  __syncthreads();
  const int a = threadIdx.x;
  if (a < n_entries) {
    const double t = s_part[a] + s_part[16 + a] + s_part[32 + a] + s_part[48 + a];
    if (t != 0.0) atomic_add_f64(gf_part(s, blockIdx.x % GF_NCOPY) + a, t);
  }
}

// grid = (ceil(maxN/256) [+ the regulariser's blocks], n_frames)
// KK = opt.num_neighbors of the launch's slots (deform_source is K-generic, super/deform_mesh.py:198-221)
// EXTRA = false: the plain point-plane term only (no segmentation weight, clip, morphing or correspondence term) -- the
// instantiation the default options run: those code paths, and the registers they hold, are compiled out (round 6: the
// kernel ran at ONE wave per SIMD with everything in one body).
template <int KK, bool EXTRA>
__global__ void __launch_bounds__(256, (EXTRA || KK > 4) ? 3 : 4) k_gf_data(GfSlot* __restrict__ slots, const GfDataArgs A) {
  const int seg_mode = EXTRA ? A.seg_mode : 0, use_morph = EXTRA ? A.use_morph : 0, corr_mode = EXTRA ? A.corr_mode : 0;
  const double pp_max = EXTRA ? A.pp_max : 0.0;
  __shared__ double sm[16];
  if ((int)blockIdx.x >= A.n_data_blocks) {
    GfSlotDev& sr = gf_dev(slots)[blockIdx.y];
    if (sr.bound) gf_reg_body(sr, blockIdx.x - A.n_data_blocks, A.ra, sm);
    return;
  }
  __shared__ int tkey[GF_TAB];               // gf_row_pass's table: node per slot, 7 sums per slot
  __shared__ double tval[GF_TAB * 7];
  __shared__ double s_gval[4][16][7 * KK];   // gradient rows of 16 surfels of each wave, canonical slot order
  __shared__ int s_gid[4][16][KK];
  __shared__ double s_part[64];              // the four waves' sums of the 16 per-thread scalars
  __shared__ double s_kept;                  // the morphing term's kept count (use_morph == 2)
  GfSlotDev& s = gf_dev(slots)[blockIdx.y];
  if (!s.bound || s.f.base.K != KK) return;
  for (int t = threadIdx.x; t < GF_TAB; t += blockDim.x) tkey[t] = -1;
  for (int t = threadIdx.x; t < GF_TAB * 7; t += blockDim.x) tval[t] = 0.0;
  if (use_morph == 2 && threadIdx.x < 64) {
    const double v = wave_sum((double)gf_part(s, threadIdx.x)[GFP_MORPH_KEPT]);
    if (threadIdx.x == 0) s_kept = v;
  }
  __syncthreads();
  const FrameIn& f = s.f.base;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double gq[4] = {0, 0, 0, 0}, gb[3] = {0, 0, 0}, loss = 0.0, cnt = 0.0, lossc = 0.0, cntc = 0.0;
  bool has_grad = false;
  d3 cl = {0, 0, 0};          // dL/dT(p) of this surfel (the global rotation undone): what its neighbours' rows are formed from
  GfSkin<KK> k;
#pragma unroll
  for (int a = 0; a < KK; ++a) k.id[a] = 0;
  if (i >= s.shard_lo && i < s.shard_hi && (!s.f.sf_stable || s.f.sf_stable[i])) {
    gf_skin<KK>(s, i, k);
    const d3 P = k.P;
    const GfProj pr = gf_project(f, P);
    d3 gP = {0, 0, 0};   // dL/dP of this surfel
    bool any = false;
    if (A.use_pp && gf_point_plane(s, i, P, pr, seg_mode, pp_max, A.lam, loss, gP)) {
      cnt = 1.0;
      any = true;
    }
    if (corr_mode && s.flow && gf_corr(s, P, pr, corr_mode, A.lam_c, lossc, gP)) {
      cntc = 1.0;
      any = true;
    }
    if (use_morph && s.sem_bound) {
      // mean over the kept surfels (count from k_gf_morph, earlier in the stream: folded into terms[6] by k_gf_fold, or --
      // use_morph == 2, slm_gf_run's loop -- still in the 64 spread copies of its entry: summed once per block, s_kept; a
      // count, exact in any order)
      const double2 mg = s.morph_g[i];
      const double kept = use_morph == 2 ? s_kept : (double)s.terms[6];
      if (kept > 0.0 && (mg.x != 0.0 || mg.y != 0.0)) {
        const double sc = A.w_morph / kept;
        gP = {gP.x + sc * (mg.x * pr.Pi0.x + mg.y * pr.Pi1.x), gP.y + sc * (mg.x * pr.Pi0.y + mg.y * pr.Pi1.y),
              gP.z + sc * (mg.x * pr.Pi0.z + mg.y * pr.Pi1.z)};
        any = true;
      }
    }
    if (EXTRA && A.pgrad) {
      // an outside term's dL/dP by surfel row (slm_gf_bind_point_grad: the render loss through slm_render_backward)
      const double* pg = A.pgrad[blockIdx.y];
      if (pg) {
        const double ax = pg[3 * (size_t)i], ay = pg[3 * (size_t)i + 1], az = pg[3 * (size_t)i + 2];
        if (ax != 0.0 || ay != 0.0 || az != 0.0) {
          gP = {gP.x + ax, gP.y + ay, gP.z + az};
          any = true;
        }
      }
    }
    if (any) {
      double jq[4];
      quat_jac_row(k.gw, k.gv, k.T, gP, jq);
#pragma unroll
      for (int a = 0; a < 4; ++a) gq[a] = jq[a];
      gb[0] = gP.x;
      gb[1] = gP.y;
      gb[2] = gP.z;
      cl = quat_apply_t(k.gw, k.gv, gP);
      has_grad = true;
    }
  }
  gf_row_pass<KK>(s, k, cl, has_grad, tkey, tval, s_gval, s_gid);
  __syncthreads();
  gf_table_flush(s, tkey, tval);
  double vals[GF_NPART] = {gq[0], gq[1], gq[2], gq[3], gb[0], gb[1], gb[2], loss, cnt, lossc, cntc, 0.0, 0.0, 0.0, 0.0, 0.0};
  gf_block_partials(s, vals, s_part, corr_mode ? GFP_CORR_KEPT + 1 : GFP_PP_KEPT + 1);
}

// ARAP: one thread per (node, slot); Rot: one thread per row (J+1); face: one per triangle.
// grid = (ceil(max(J*K_ED, J+1, Tr)/256), n_frames)
// bx: the block's index among the regulariser's blocks (its own launch, or the tail blocks of k_gf_data's)
__device__ __forceinline__ void gf_reg_body(GfSlotDev& s, const int bx, const GfRegArgs ra, double* sm) {
  const int use_arap = ra.use_arap, use_rot = ra.use_rot, use_face = ra.use_face;
  const double lam_a = ra.lam_a, lam_r = ra.lam_r, lam_f = ra.lam_f;
  const FrameIn& f = s.f.base;
  const int J = f.J, Ke = f.K_ED;
  const int t = bx * blockDim.x + threadIdx.x;
  double la = 0.0, lr = 0.0, lf = 0.0;
  double gq[4] = {0, 0, 0, 0}, gb[3] = {0, 0, 0};   // global-row contributions of this thread
  if (use_arap && t < J * Ke) {
    const int j = t / Ke, k = f.ed_knn_idx[t];
    const d3 d = ld_state3(f.ed_points, (size_t)j, f.state_f64) - ld_state3(f.ed_points, (size_t)k, f.state_f64);
    const d3 d32 = {(double)(float)d.x, (double)(float)d.y, (double)(float)d.z};
    const double* bk = s.dv + 7 * k;
    const double* bj = s.dv + 7 * j;
    const d3 qv = {bk[1], bk[2], bk[3]};
    const d3 tr = quat_apply(bk[0], qv, d);
    const d3 r = {tr.x + bk[4] - d32.x - bj[4], tr.y + bk[5] - d32.y - bj[5], tr.z + bk[6] - d32.z - bj[6]};
    const double wjk = ld_state1(s.f.ed_knn_w, (size_t)t, f.state_f64);
    la = lam_a * wjk * dot(r, r);
    const double G = 2.0 * lam_a * wjk;
    double jq[4];
    quat_jac_row(bk[0], qv, d, r, jq);
    double* gk = s.grad + 7 * k;
    double* gj = s.grad + 7 * j;
    atomic_add_f64(gk + 0, G * jq[0]);
    atomic_add_f64(gk + 1, G * jq[1]);
    atomic_add_f64(gk + 2, G * jq[2]);
    atomic_add_f64(gk + 3, G * jq[3]);
    atomic_add_f64(gk + 4, G * r.x);
    atomic_add_f64(gk + 5, G * r.y);
    atomic_add_f64(gk + 6, G * r.z);
    atomic_add_f64(gj + 4, -G * r.x);
    atomic_add_f64(gj + 5, -G * r.y);
    atomic_add_f64(gj + 6, -G * r.z);
  }
  if (use_rot && t <= J) {
    const double* q = s.dv + 7 * t;
    const double sres = 1.0 - (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    lr = lam_r * sres * sres;
    const double G = -4.0 * lam_r * sres;
    double* gr = s.grad + 7 * t;
    atomic_add_f64(gr + 0, G * q[0]);
    atomic_add_f64(gr + 1, G * q[1]);
    atomic_add_f64(gr + 2, G * q[2]);
    atomic_add_f64(gr + 3, G * q[3]);
  }
  if (use_face && s.f.ed_triangles && t < s.f.n_triangles) {
    const int Tr = s.f.n_triangles;
    const int iv[3] = {s.f.ed_triangles[t], s.f.ed_triangles[Tr + t], s.f.ed_triangles[2 * Tr + t]};
    const double* bgl = s.dv + 7 * J;
    const double gw = bgl[0];
    const d3 gv = {bgl[1], bgl[2], bgl[3]};
    d3 loc[3], V[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double* b = s.dv + 7 * iv[a];
      const d3 gn = ld_state3(f.ed_points, (size_t)iv[a], f.state_f64);
      loc[a] = {gn.x + b[4], gn.y + b[5], gn.z + b[6]};
      V[a] = quat_apply(gw, gv, loc[a]);   // + b_g cancels in the edge vectors
    }
    const d3 e1 = V[1] - V[0], e2 = V[2] - V[0];
    const d3 cr = cross(e1, e2);
    const double area = 0.5 * sqrt(dot(cr, cr) + 1e-13);
    const double da = area - ld_state1(s.f.ed_triangle_areas, (size_t)t, f.state_f64);
    lf = lam_f * da * da;
    const double coef = 2.0 * lam_f * da / (4.0 * area);
    const d3 y = {coef * cr.x, coef * cr.y, coef * cr.z};     // dL/d(cr)
    d3 gV[3];
    gV[1] = cross(e2, y);
    gV[2] = cross(y, e1);
    gV[0] = {-gV[1].x - gV[2].x, -gV[1].y - gV[2].y, -gV[1].z - gV[2].z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double jq[4];
      quat_jac_row(gw, gv, loc[a], gV[a], jq);
#pragma unroll
      for (int c = 0; c < 4; ++c) gq[c] += jq[c];
      gb[0] += gV[a].x;
      gb[1] += gV[a].y;
      gb[2] += gV[a].z;
      const d3 gl = quat_apply_t(gw, gv, gV[a]);
      double* gr = s.grad + 7 * iv[a];
      atomic_add_f64(gr + 4, gl.x);
      atomic_add_f64(gr + 5, gl.y);
      atomic_add_f64(gr + 6, gl.z);
    }
  }
  double vals[10] = {gq[0], gq[1], gq[2], gq[3], gb[0], gb[1], gb[2], lf, la, lr};
#pragma unroll
  for (int a = 0; a < 10; ++a) {
    const double tt = block_sum(vals[a], sm);
    // (spread block partials: the global row, then face / arap / rot)
    if (threadIdx.x == 0 && tt != 0.0) atomic_add_f64(gf_part(s, bx % GF_NCOPY) + (a < 7 ? GFP_GLOBAL + a : GFP_FACE + a - 7), tt);
  }
}
__global__ void __launch_bounds__(256) k_gf_reg(GfSlot* __restrict__ slots, GfRegArgs ra) {
  __shared__ double sm[16];
  GfSlotDev& s = gf_dev(slots)[blockIdx.y];
  if (!s.bound) return;
  gf_reg_body(s, blockIdx.x, ra, sm);
}

// grad[J] /= J, then torch.optim.SGD(momentum=0.9) or torch.optim.Adam step (float64).
// Also turns the morphing term's sum into the reference's weighted mean (NaN over an empty set).
// fold (GfStepFold bits): GF_STEP_FOLD -- this launch also sums the spread block partials of k_gf_data / k_gf_reg (what
// k_gf_fold(GF_FOLD_DATA) does as a launch of its own: slm_gf_run's loop saves that launch; the thread of a global-row entry
// sums its own 64 copies, threads 0..6 the loss terms');  GF_STEP_OWN -- the launch OWNS the partials: it clears what it summed
// and ASSIGNS the loss terms (nothing else wrote them since the last k_gf_zero);  GF_STEP_REZERO -- it leaves the gradient zeroed
// for the next iteration (OWN + REZERO: slm_gf_run's loop needs no k_gf_zero between two iterations);  GF_STEP_MORPH -- the
// launch also owns the morphing term's partials (k_gf_fold(GF_FOLD_MORPH) as a launch of its own otherwise): it assigns
// terms[5] / [6] from them, clears them and, with REZERO, resets the candidates flag terms[7] for the next iteration's k_gf_morph.
// step_off: optimiser steps of this run that s.step does not count yet (k_gf_advance adds them at the end of the run)
__global__ void __launch_bounds__(256) k_gf_step(GfSlot* __restrict__ slots, int optimizer, double lr,
                                                  int apply, int use_morph, double w_morph, int fold, int step_off) {
  GfSlotDev& s = gf_dev(slots)[blockIdx.y];
  if (!s.bound) return;
  const int J = s.f.base.J, n = (J + 1) * 7;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0 && use_morph) {
    double li = s.terms[5], kept = s.terms[6];
    if (fold & GF_STEP_MORPH) {
      li = gf_part_fold(s, GFP_MORPH_SUM, true);
      kept = gf_part_fold(s, GFP_MORPH_KEPT, true);
      s.terms[6] = kept;
    }
    s.terms[5] = s.terms[7] != 0.0 ? (kept > 0.0 ? w_morph * li / kept : nan("")) : 0.0;
    if ((fold & (GF_STEP_REZERO | GF_STEP_MORPH)) == (GF_STEP_REZERO | GF_STEP_MORPH)) s.terms[7] = 0.0;
    else if (s.terms[7] != 0.0) s.terms[7] = 1.0;   // (sharded: the exchanges summed the ranks' flags)
  }
  if (e >= n) return;
  double g = s.grad[e];
  if (fold & GF_STEP_FOLD) {
    const bool own = (fold & GF_STEP_OWN) != 0;
    if (e < GFP_MORPH_SUM - GFP_PP_LOSS) {   // thread e: the loss term of entry GFP_PP_LOSS + e (point-plane .. rot)
      const int a = GFP_PP_LOSS + e;
      const double t = gf_part_fold(s, a, own);
      if (own) s.terms[gf_part_term(a)] = t;
      else if (t != 0.0) s.terms[gf_part_term(a)] += t;
    }
    if (e >= 7 * J) g += gf_part_fold(s, GFP_GLOBAL + e - 7 * J, own);
  }
  if (e >= 7 * J) {
    g /= (double)J;
    s.grad[e] = g;
  }
  if (fold & GF_STEP_REZERO) s.grad[e] = 0.0;
  if (!apply) return;
  const int t = s.step + 1 + step_off;
  if (optimizer == 0) {
    const double buf = (t == 1) ? g : 0.9 * s.m1[e] + g;
    s.m1[e] = buf;
    s.dv[e] -= lr * buf;
  } else {
    const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
    const double m = b1 * s.m1[e] + (1.0 - b1) * g;
    const double v = b2 * s.m2[e] + (1.0 - b2) * g * g;
    s.m1[e] = m;
    s.m2[e] = v;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    const double denom = sqrt(v) / sqrt(bc2) + eps;
    s.dv[e] -= (lr / bc1) * m / denom;
  }
}

__global__ void k_gf_advance(GfSlot* __restrict__ slots, int inc) {
  GfSlotDev& s = gf_dev(slots)[blockIdx.x];
  if (s.bound && threadIdx.x == 0) s.step += inc;
}

__global__ void __launch_bounds__(256) k_gf_init(GfSlot* __restrict__ slots, int slot) {
  GfSlotDev& s = gf_dev(slots)[slot];
  const int n = (s.f.base.J + 1) * 7;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) {
    s.dv[e] = (e % 7 == 0) ? 1.0 : 0.0;
    s.grad[e] = 0.0;
    s.m1[e] = 0.0;
    s.m2[e] = 0.0;
  }
  if (e == 0) s.step = 0;
}

// ---------------------------------------------------------------------------------------
struct slm_gf {
  int batch_K = SLM_K;       // num_neighbors of the slots of the launch being enqueued (gf_dims: they must agree)
  slm_gf_config cfg{};
  std::vector<GfSlot> host;
  std::vector<size_t> cap;   // per slot: doubles of its one allocation (GfSlot::dv)
  std::vector<SemScratch> sem;
  GfSlot* dev = nullptr;
  int* knn_bad = nullptr;    // device flag of slm_gf_bind_frame's table check
  int rank = 0, world = 1;   // surfel sharding of every slot (slm_gf_set_shard)
  const double** pgrad = nullptr;             // (max_frames) device: slm_gf_bind_point_grad's buffer per slot, or null
  std::vector<const double*> pgrad_host;      // the same on the host: selects the EXTRA launch
  std::vector<GfRenderTerm> rterm;            // per slot: the render loss of slm_gf_bind_render_loss (its pgrad is the slot's)
};

// ---- what every entry point goes through ---------------------------------------------------------------------------------------
// The slots [first, first + n) of an entry point `who`: g, the other required arguments (args_ok) and the range checked, and --
// need_bound -- that slot `first` holds a frame; *out = the host copy of slot `first`.  The texts are each family's own.
struct GfSlotTexts {
  const char *null_arg, *range, *unbound;
};
static const GfSlotTexts GF_TEXTS_BIND = {"null argument", "bad slot", "slm_gf_bind_frame first"};
static const GfSlotTexts GF_TEXTS_RENDER = {"bad slot", "bad slot", "slm_gf_bind_frame first"};
static const GfSlotTexts GF_TEXTS_EDGE = {"bad argument", "bad argument", nullptr};
static const GfSlotTexts GF_TEXTS_RANGE = {"slot range out of bounds", "slot range out of bounds", "slot used before slm_gf_bind_frame"};
static int gf_slot(const char* who, const GfSlotTexts& tx, slm_gf* g, bool args_ok, int first, int n, bool need_bound, GfSlot** out) {
  auto refuse = [who](int code, const char* text) { return fail(code, std::string(who) + ": " + text); };   // (no string unless refused)
  if (!g || !args_ok) return refuse(SLM_ERR_INVALID, tx.null_arg);
  if (first < 0 || n < 1 || first + n > (int)g->host.size()) return refuse(SLM_ERR_INVALID, tx.range);
  if (need_bound && !g->host[first].bound) return refuse(SLM_ERR_UNBOUND, tx.unbound);
  if (out) *out = &g->host[first];
  return SLM_OK;
}

// the launch sizes over the slots [first, first + n) of an evaluation entry point, every slot checked for what the
// configuration needs bound; sets g->batch_K
struct GfDims {
  int maxN = 0, maxReg = 0, maxP = 0;
};
static int gf_dims(slm_gf* g, int first, int n, GfDims* d) {
  if (const int rc = gf_slot("slm_gf", GF_TEXTS_RANGE, g, true, first, n, false, nullptr)) return rc;
  *d = GfDims{};
  for (int i = first; i < first + n; ++i) {
    GfSlot* sp = nullptr;
    if (const int rc = gf_slot("slm_gf", GF_TEXTS_RANGE, g, true, i, 1, true, &sp)) return rc;
    const GfSlot& s = *sp;
    if ((g->cfg.seg_mode || g->cfg.use_bn_morph) && !s.sem_bound)
      return fail(SLM_ERR_UNBOUND, "slm_gf: semantic terms enabled but slm_gf_bind_semantic was not called");
    if (g->cfg.corr_mode && !s.flow)
      return fail(SLM_ERR_UNBOUND, "slm_gf: corr_mode set but slm_gf_bind_flow was not called");
    if (s.f.base.K != g->host[first].f.base.K)
      return fail(SLM_ERR_UNSUPPORTED, "slm_gf: the frames of one batch must have the same num_neighbors");
    d->maxN = std::max(d->maxN, s.f.base.N);
    int reg = std::max(s.f.base.J * s.f.base.K_ED, s.f.base.J + 1);
    if (g->cfg.use_face) reg = std::max(reg, s.f.n_triangles);
    d->maxReg = std::max(d->maxReg, reg);
    d->maxP = std::max(d->maxP, (s.f.base.J + 1) * 7);
  }
  g->batch_K = g->host[first].f.base.K;
  return SLM_OK;
}

// the slot's point gradient (what k_gf_data<K, true> adds), on the host and in the device table; wait: behind the copy
static int gf_publish_pgrad(slm_gf* g, int slot, const double* pgrad, hipStream_t st, bool wait = true) {
  g->pgrad_host[slot] = pgrad;
  HIPCHK(hipMemcpyAsync(g->pgrad + slot, &g->pgrad_host[slot], sizeof(const double*), hipMemcpyHostToDevice, st));
  if (wait) HIPCHK(hipStreamSynchronize(st));
  return SLM_OK;
}

// the host copy of the slot's descriptor -> the device, waited for
static int gf_upload_slot(slm_gf* g, int slot, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(g->dev + slot, &g->host[slot], sizeof(GfSlot), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return SLM_OK;
}

// k_gf_step over the slots [first, first + n): fold = GfStepFold bits, step_off as the kernel's
static void gf_launch_step(slm_gf* g, int first, int n, const GfDims& d, int apply, int fold, int step_off, hipStream_t st) {
  hipLaunchKernelGGL(k_gf_step, dim3((d.maxP + 255) / 256, n), dim3(256), 0, st, g->dev + first, g->cfg.optimizer, g->cfg.lr, apply,
                     g->cfg.use_bn_morph, g->cfg.w_bn_morph, fold, step_off);
}

// The render loss of the slots [first, first + n) that have it, in front of an evaluation: the guarded forward of the slot's
// current deform_verts, the SSIM loss with its image gradient, the guarded backward into the buffer k_gf_data<K, true> reads.
// Launches only: the buffers and the lists' entry limit were fixed by slm_gf_bind_render_loss.
static void gf_enqueue_render(slm_gf* g, int first, int n, hipStream_t st) {
  for (int k = first; k < first + n; ++k) {
    const GfRenderTerm& t = g->rterm[k];
    if (!t.ctx) continue;
    const int N = g->host[k].f.base.N;
    rn_gf_forward(t.ctx, &t.p, g->dev + k, N, t.radii, t.colors, t.cstride, t.image, t.limit, st);
    ssim_enqueue(t.p.height, t.p.width, t.image, t.target, t.weight, t.loss, t.gimg, t.scratch, st);
    if (N > 0) rn_gf_backward(t.ctx, &t.p, N, t.radii != nullptr, t.gimg, t.pgrad, st);
  }
}

// takes the term off the slot (the buffers stay for the next bind); the slot's point gradient goes with it
static int gf_clear_render(slm_gf* g, int slot, hipStream_t st) {
  if (!g->rterm[slot].ctx) return SLM_OK;
  g->rterm[slot].ctx = nullptr;
  return gf_publish_pgrad(g, slot, nullptr, st);
}

// What an evaluation consists of (gf_enqueue_morph, gf_enqueue_eval)
enum GfEval {
  GF_EVAL_ZERO = 1,     // k_gf_zero in front of pass 1
  GF_EVAL_PASS1 = 2,    // gf_enqueue_eval: pass 1 (gf_enqueue_morph) in front of pass 2
  GF_EVAL_IN_RUN = 4    // an iteration of slm_gf_run's loop: no k_gf_fold launches (k_gf_data reads the morphing term's kept count
                        // from the partials, the caller's k_gf_step folds) and the render terms sit behind pass 1, not in front
};

// pass 1 of an evaluation: [zero the gradient / terms], then the morphing term's per-surfel pass (sum, count) into the spread
// partials; stepwise, k_gf_fold puts them into terms[5], [6], what the back-propagation divides by
static void gf_enqueue_morph(slm_gf* g, int first, int n, const GfDims& d, hipStream_t st, int what) {
  GfSlot* slots = g->dev + first;
  if (what & GF_EVAL_ZERO) hipLaunchKernelGGL(k_gf_zero, dim3(32, n), dim3(256), 0, st, slots);
  if (!g->cfg.use_bn_morph) return;
  launch_gf_morph(slots, n, d.maxN, st);
  if (!(what & GF_EVAL_IN_RUN)) hipLaunchKernelGGL(k_gf_fold, dim3(1, n), dim3(64), 0, st, slots, (int)GF_FOLD_MORPH);
}

// One evaluation of the slots [first, first + n), launches only; what = GfEval bits.  Pass 2 is point-plane (+ morphing
// back-propagation, which needs the GLOBAL kept count) and the node terms (on rank 0 only when the surfels are sharded: the
// caller sums the partials), the node terms as the tail blocks of k_gf_data.
//   stepwise:        the render terms, [pass 1 with its fold], pass 2, k_gf_fold -- gradient and terms are complete behind it
//   GF_EVAL_IN_RUN:  [pass 1 without the fold], the render terms, pass 2; no fold
static void gf_enqueue_eval(slm_gf* g, int first, int n, const GfDims& d, hipStream_t st, int what) {
  const slm_gf_config& c = g->cfg;
  GfSlot* slots = g->dev + first;
  const bool in_run = (what & GF_EVAL_IN_RUN) != 0;
  if (!in_run) gf_enqueue_render(g, first, n, st);   // (nothing without slm_gf_bind_render_loss)
  if (what & GF_EVAL_PASS1) gf_enqueue_morph(g, first, n, d, st, what);
  if (in_run) gf_enqueue_render(g, first, n, st);
  GfDataArgs A{};
  A.use_pp = (c.use_data || c.seg_mode) ? 1 : 0;   // either flag enables the term (deform_mesh.py:81)
  const bool data = (A.use_pp || c.use_bn_morph || c.corr_mode) && d.maxN > 0;
  const bool reg = g->rank == 0 && (c.use_arap || c.use_rot || c.use_face) && d.maxReg > 0;
  const int nr = reg ? (d.maxReg + 255) / 256 : 0;
  A.n_data_blocks = (d.maxN + 255) / 256;
  A.lam = c.w_data;
  A.ra = {c.use_arap, c.use_rot, c.use_face, 0, c.w_arap, c.w_rot, c.w_face};
  bool pg = false;
  for (int k = first; k < first + n; ++k) pg = pg || g->pgrad_host[k] != nullptr;
  if (data || (pg && d.maxN > 0)) {
    const dim3 grid(A.n_data_blocks + nr, n);
    if (c.seg_mode || c.use_bn_morph || c.corr_mode || c.pp_max > 0.0 || pg) {
      A.seg_mode = c.seg_mode;
      A.pp_max = c.seg_mode ? 0.0 : c.pp_max;
      A.use_morph = c.use_bn_morph ? (in_run ? 2 : 1) : 0;
      A.w_morph = c.w_bn_morph;
      A.corr_mode = c.corr_mode;
      A.lam_c = c.w_corr;
      A.pgrad = pg ? g->pgrad + first : nullptr;
      SLM_K_DISPATCH(g->batch_K, hipLaunchKernelGGL((k_gf_data<KK, true>), grid, dim3(256), 0, st, slots, A));
    } else {
      SLM_K_DISPATCH(g->batch_K, hipLaunchKernelGGL((k_gf_data<KK, false>), grid, dim3(256), 0, st, slots, A));
    }
  } else if (reg) {
    hipLaunchKernelGGL(k_gf_reg, dim3(nr, n), dim3(256), 0, st, slots, A.ra);
  }
  // sharded, the morphing term on: terms[5..7] are global since the exchange behind pass 1 and k_gf_data has read the kept
  // count by now; every rank but 0 clears them, so that the exchange behind this pass -- a sum of the whole block -- leaves
  // the true sum, count and flag on every rank and not `world` times them
  const int drop = (g->rank != 0 && c.use_bn_morph) ? (int)GF_FOLD_DROP_MORPH : 0;
  if (!in_run) hipLaunchKernelGGL(k_gf_fold, dim3(1, n), dim3(64), 0, st, slots, (int)GF_FOLD_DATA | drop);
}

extern "C" {

int slm_gf_create(const slm_gf_config* cfg, slm_gf** out) {
  if (!cfg || !out || cfg->max_frames < 1 || cfg->num_iterations < 0 || (cfg->optimizer != 0 && cfg->optimizer != 1) ||
      cfg->seg_mode < 0 || cfg->seg_mode > 2 || cfg->corr_mode < 0 || cfg->corr_mode > 2)
    return fail(SLM_ERR_INVALID, "slm_gf_create: bad argument");
  if (slm_device_count() < 1) return fail(SLM_ERR_NO_DEVICE, "slm_gf_create: no HIP device visible");
  slm_gf* g = new slm_gf();
  g->cfg = *cfg;
  g->host.assign(cfg->max_frames, GfSlot{});
  g->cap.assign(cfg->max_frames, 0);
  g->sem.assign(cfg->max_frames, SemScratch());
  g->pgrad_host.assign(cfg->max_frames, nullptr);
  g->rterm.assign(cfg->max_frames, GfRenderTerm{});
  hipError_t e = hipMalloc((void**)&g->dev, sizeof(GfSlot) * cfg->max_frames);
  if (e == hipSuccess) e = hipMemset(g->dev, 0, sizeof(GfSlot) * cfg->max_frames);
  if (e == hipSuccess) e = hipMalloc((void**)&g->knn_bad, sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&g->pgrad, sizeof(const double*) * cfg->max_frames);
  if (e == hipSuccess) e = hipMemset(g->pgrad, 0, sizeof(const double*) * cfg->max_frames);
  if (e != hipSuccess) {
    slm_gf_destroy(g);
    return fail(SLM_ERR_HIP, std::string("slm_gf_create: ") + hipGetErrorString(e));
  }
  *out = g;
  return SLM_OK;
}

int slm_gf_destroy(slm_gf* g) {
  if (!g) return SLM_OK;
  for (GfSlot& s : g->host) {
    if (s.dv) (void)hipFree(s.dv);   // dv | grad | m1 | m2 | terms are one allocation
  }
  for (SemScratch& sc : g->sem) sem_free(sc);
  for (GfRenderTerm& t : g->rterm)
    for (void* q : {(void*)t.image, (void*)t.gimg, (void*)t.pgrad, (void*)t.loss, (void*)t.scratch})
      if (q) (void)hipFree(q);
  if (g->dev) (void)hipFree(g->dev);
  if (g->knn_bad) (void)hipFree(g->knn_bad);
  if (g->pgrad) (void)hipFree(g->pgrad);
  delete g;
  return SLM_OK;
}

int slm_gf_bind_frame(slm_gf* g, int32_t slot, const slm_gf_frame* fr, void* stream) {
  GfSlot* sp = nullptr;
  if (const int rc = gf_slot("slm_gf_bind_frame", GF_TEXTS_BIND, g, fr != nullptr, slot, 1, false, &sp)) return rc;
  const slm_frame& f = fr->base;
  if (f.K < 1 || f.K > 8) return fail(SLM_ERR_UNSUPPORTED, "slm_gf_bind_frame: num_neighbors must be in 1..8");
  if (f.K_ED < 1 || f.K_ED > SLM_MAX_KED || f.N < 0 || f.J < 1 || f.H < 4 || f.W < 4)
    return fail(SLM_ERR_INVALID, "slm_gf_bind_frame: bad sizes");
  // (a frame without surfels has node terms only: its surfel arrays are empty and may be null, as in slm_gf_bind_semantic)
  if ((f.N > 0 && (!f.sf_points || !f.sf_knn_idx || !f.sf_knn_w)) || !f.ed_points || !f.ed_knn_idx || !f.tgt_points ||
      !f.tgt_norms || !f.index_map || (g->cfg.use_arap && !fr->ed_knn_w) ||
      (g->cfg.use_face && (!fr->ed_triangles || !fr->ed_triangle_areas)))
    return fail(SLM_ERR_INVALID, "slm_gf_bind_frame: null device pointer");
  if (f.N > 0 && f.J < f.K)   // (the reference's top-k of K among J nodes raises)
    return fail(SLM_ERR_INVALID, "slm_gf_bind_frame: fewer nodes (J) than num_neighbors: sf_knn_idx cannot hold K distinct ids");
  hipStream_t st = (hipStream_t)stream;
  GfSlot& s = *sp;
  const size_t n = (size_t)(f.J + 1) * 7;
  const size_t n_dv = 4 * n + SLM_GF_NTERMS + GF_PART_DOUBLES;   // ... | terms | spread block partials
  HIPCHK(grow(s.dv, g->cap[slot], n_dv, n_dv));
  s.grad = s.dv + n;
  s.m1 = s.dv + 2 * n;
  s.m2 = s.dv + 3 * n;
  s.terms = s.dv + 4 * n;
  s.f = *fr;
  s.bound = 1;
  s.step = 0;
  s.sem_bound = 0;   // semantic inputs, the flow, a point gradient and the render loss belong to the frame: bind them again
  s.flow = nullptr;
  g->rterm[slot].ctx = nullptr;
  if (const int rc = gf_publish_pgrad(g, slot, nullptr, st, false)) return rc;   // (waited for with the descriptor, below)
  s.shard_lo = (int32_t)((int64_t)f.N * g->rank / g->world);
  s.shard_hi = (int32_t)((int64_t)f.N * (g->rank + 1) / g->world);
  // The KNN tables as the reference's top-k makes them: distinct ids in [0, J) (k_gf_data's row pass gives every id of a
  // row an LDS slot of its own and indexes the nodes with them).  The flag comes back with the descriptor's wait below.
  int bad_host = 0;
  HIPCHK(hipMemsetAsync(g->knn_bad, 0, sizeof(int), st));
  launch_check_knn(f, g->knn_bad, st);
  HIPCHK(hipMemcpyAsync(&bad_host, g->knn_bad, sizeof(int), hipMemcpyDeviceToHost, st));
  if (const int rc = gf_upload_slot(g, slot, st)) return rc;
  if (bad_host) {   // refused: the slot stays unbound, on the device too
    s.bound = 0;
    if (const int rc = gf_upload_slot(g, slot, st)) return rc;
    return fail(SLM_ERR_INVALID, "slm_gf_bind_frame: a KNN index (sf_knn_idx or ed_knn_idx) lies outside [0, J) or a "
                                    "surfel's row of sf_knn_idx repeats an id");
  }
  hipLaunchKernelGGL(k_gf_init, dim3((n + 255) / 256), dim3(256), 0, st, g->dev, slot);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_gf_bind_semantic(slm_gf* g, int32_t slot, const slm_gf_semantic* sem, int32_t* edge_counts_host,
                         void* stream) {
  GfSlot* sp = nullptr;
  if (const int rc = gf_slot("slm_gf_bind_semantic", GF_TEXTS_BIND, g, sem != nullptr, slot, 1, true, &sp)) return rc;
  GfSlot& s = *sp;
  if (sem->num_classes < 1 || sem->num_classes > SLM_MAX_CLASSES)
    return fail(SLM_ERR_UNSUPPORTED, "slm_gf_bind_semantic: num_classes must be 1..4");
  const slm_frame& f = s.f.base;
  const bool need_pp = g->cfg.seg_mode != 0, need_morph = g->cfg.use_bn_morph != 0;
  if ((f.N > 0 && !sem->sf_seg) || (need_pp && ((f.N > 0 && !sem->sf_seg_conf) || (f.T > 0 && !sem->tgt_seg_conf))) ||
      (need_morph && (!sem->img_seg_conf || !sem->img_seg)))
    return fail(SLM_ERR_INVALID, "slm_gf_bind_semantic: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  SemScratch& sc = g->sem[slot];
  s.sem = *sem;
  for (int c = 0; c <= SLM_MAX_CLASSES; ++c) s.edge_off[c] = 0;
  if (need_morph) {
    HIPCHK(sem_extract_edges(sc, sem->num_classes, sem->img_seg, f.H, f.W, s.edge_off, st));
    HIPCHK(sem_ensure_morph(sc, f.N));
  }
  s.edge_xy = sc.edge_xy;
  s.morph_g = sc.morph_g;
  s.sem_bound = 1;
  if (edge_counts_host)
    for (int c = 0; c < sem->num_classes; ++c) edge_counts_host[c] = s.edge_off[c + 1] - s.edge_off[c];
  return gf_upload_slot(g, slot, st);
}

int slm_gf_bind_flow(slm_gf* g, int32_t slot, const float* flow, void* stream) {
  GfSlot* sp = nullptr;
  if (const int rc = gf_slot("slm_gf_bind_flow", GF_TEXTS_BIND, g, flow != nullptr, slot, 1, true, &sp)) return rc;
  GfSlot& s = *sp;
  hipStream_t st = (hipStream_t)stream;
  s.flow = flow;
  // the pointer alone: the device copy of the slot also holds the optimiser's step count, which the host copy does not
  // follow (sf_corr_match_renderimg binds a new flow between the iterations of one frame)
  HIPCHK(hipMemcpyAsync(&g->dev[slot].flow, &s.flow, sizeof(s.flow), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return SLM_OK;
}

int slm_gf_bind_point_grad(slm_gf* g, int32_t slot, const double* grad, void* stream) {
  if (const int rc = gf_slot("slm_gf_bind_point_grad", GF_TEXTS_BIND, g, true, slot, 1, true, nullptr)) return rc;
  if (g->rterm[slot].ctx)
    return fail(SLM_ERR_INVALID, "slm_gf_bind_point_grad: the render loss is bound to the slot (slm_gf_bind_render_loss), "
                                    "which owns its point gradient: clear it first");
  return gf_publish_pgrad(g, slot, grad, (hipStream_t)stream);
}

int slm_gf_bind_render_loss(slm_gf* g, int32_t slot, slm_render* r, const slm_render_params* p, const float* radii,
                            const float* colors, int32_t color_stride, const float* target_chw, double weight,
                            int64_t entry_limit, void* stream) {
  const char* who = "slm_gf_bind_render_loss";
  if (const int rc = gf_slot(who, GF_TEXTS_BIND, g, true, slot, 1, false, nullptr)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!r) return gf_clear_render(g, slot, st);
  if (const int rc = gf_slot(who, GF_TEXTS_BIND, g, p && target_chw, slot, 1, true, nullptr)) return rc;
  if (g->world > 1)
    return fail(SLM_ERR_UNSUPPORTED, "slm_gf_bind_render_loss: surfels are sharded; the render loss needs every surfel of "
                                        "the frame on one device");
  GfRenderTerm& t = g->rterm[slot];
  if (!t.ctx && g->pgrad_host[slot])
    return fail(SLM_ERR_INVALID, "slm_gf_bind_render_loss: a point gradient is bound to the slot (slm_gf_bind_point_grad): "
                                    "clear it first");
  for (int k = 0; k < (int)g->rterm.size(); ++k)
    if (k != slot && g->rterm[k].ctx == r)
      return fail(SLM_ERR_INVALID, "slm_gf_bind_render_loss: the context is bound to another slot; one context serves one "
                                      "slot");
  if (!std::isfinite(weight)) return fail(SLM_ERR_INVALID, "slm_gf_bind_render_loss: weight must be finite");
  if (entry_limit < 0 || entry_limit > ((int64_t)1 << 31))
    return fail(SLM_ERR_INVALID, "slm_gf_bind_render_loss: entry_limit must be 0 (from a sizing render) or 1..2^31");
  const int N = g->host[slot].f.base.N;
  if (const int rc = rn_gf_check(who, r, p, N, colors, color_stride)) return rc;
  if (p->height < 6 || p->width < 6)
    return fail(SLM_ERR_INVALID, "slm_gf_bind_render_loss: height and width must be >= 6 (the SSIM window)");
  if (const int rc = gf_clear_render(g, slot, st)) return rc;   // (a failure below leaves the slot without the term)
  const size_t px3 = 3 * (size_t)p->height * p->width, n3 = 3 * (size_t)N + 3;
  const size_t n_scr = ssim_scratch_doubles(p->height, p->width, true);
  HIPCHK(grow(t.image, t.cap_image, px3, px3));
  HIPCHK(grow(t.gimg, t.cap_gimg, px3, px3));
  HIPCHK(grow(t.pgrad, t.cap_pgrad, n3, n3));
  HIPCHK(grow(t.loss, t.cap_loss, 2, 2));
  HIPCHK(grow(t.scratch, t.cap_scratch, n_scr, n_scr));
  unsigned long long limit = 0;
  if (const int rc = rn_gf_size(who, r, p, g->dev + slot, N, radii, colors, color_stride, t.image, entry_limit, &limit, stream))
    return rc;
  HIPCHK(hipMemsetAsync(t.loss, 0, 2 * sizeof(double), st));
  HIPCHK(hipMemsetAsync(t.pgrad, 0, n3 * sizeof(double), st));
  t.p = *p;
  t.radii = radii;
  t.colors = colors;
  t.cstride = color_stride;
  t.target = target_chw;
  t.weight = weight;
  t.limit = limit;
  if (const int rc = gf_publish_pgrad(g, slot, t.pgrad, st)) return rc;
  t.ctx = r;
  return SLM_OK;
}

static int gf_render_term(slm_gf* g, int32_t slot, const char* who, const GfRenderTerm** t) {
  if (const int rc = gf_slot(who, GF_TEXTS_BIND, g, true, slot, 1, false, nullptr)) return rc;
  if (!g->rterm[slot].ctx) return fail(SLM_ERR_UNBOUND, std::string(who) + ": slm_gf_bind_render_loss first");
  *t = &g->rterm[slot];
  return SLM_OK;
}

int slm_gf_render_loss_status(slm_gf* g, int32_t slot, double out_host[4], void* stream) {
  const GfRenderTerm* t = nullptr;
  if (const int rc = gf_render_term(g, slot, "slm_gf_render_loss_status", &t)) return rc;
  if (!out_host) return fail(SLM_ERR_INVALID, "slm_gf_render_loss_status: null argument");
  hipStream_t st = (hipStream_t)stream;
  double loss[2] = {0.0, 0.0};
  unsigned long long stat[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(loss, t->loss, sizeof(loss), hipMemcpyDeviceToHost, st));
  HIPCHK(rn_gf_status(t->ctx, stat, st));
  HIPCHK(hipStreamSynchronize(st));
  out_host[0] = loss[0];
  out_host[1] = loss[1];
  out_host[2] = (double)stat[0];
  out_host[3] = (double)stat[1];
  return SLM_OK;
}

int slm_gf_render_loss_read(slm_gf* g, int32_t slot, float* image, double* grad_points, void* stream) {
  const GfRenderTerm* t = nullptr;
  if (const int rc = gf_render_term(g, slot, "slm_gf_render_loss_read", &t)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t px3 = 3 * (size_t)t->p.height * t->p.width, n3 = 3 * (size_t)g->host[slot].f.base.N;
  if (image) HIPCHK(hipMemcpyAsync(image, t->image, sizeof(float) * px3, hipMemcpyDeviceToDevice, st));
  if (grad_points && n3) HIPCHK(hipMemcpyAsync(grad_points, t->pgrad, sizeof(double) * n3, hipMemcpyDeviceToDevice, st));
  return SLM_OK;
}

int slm_gf_get_edge_points(slm_gf* g, int32_t slot, int32_t class_id, float* xy_out, int32_t max_points,
                           void* stream) {
  GfSlot* sp = nullptr;
  if (const int rc = gf_slot("slm_gf_get_edge_points", GF_TEXTS_EDGE, g, xy_out != nullptr, slot, 1, false, &sp)) return rc;
  const GfSlot& s = *sp;
  if (!s.bound || !s.sem_bound) return fail(SLM_ERR_UNBOUND, "slm_gf_get_edge_points: no semantic inputs bound");
  if (class_id < 0 || class_id >= s.sem.num_classes)
    return fail(SLM_ERR_INVALID, "slm_gf_get_edge_points: bad class");
  const int n = s.edge_off[class_id + 1] - s.edge_off[class_id];
  if (n > max_points) return fail(SLM_ERR_INVALID, "slm_gf_get_edge_points: output too small");
  if (n > 0)
    HIPCHK(hipMemcpyAsync(xy_out, s.edge_xy + s.edge_off[class_id], sizeof(float2) * n, hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return SLM_OK;
}

int slm_gf_set_shard(slm_gf* g, int32_t rank, int32_t world) {
  if (!g || world < 1 || rank < 0 || rank >= world) return fail(SLM_ERR_INVALID, "slm_gf_set_shard: bad rank/world");
  g->rank = rank;
  g->world = world;
  for (GfSlot& s : g->host) s.bound = 0;   // shard bounds are fixed at bind time
  for (size_t k = 0; k < g->rterm.size(); ++k) {
    g->rterm[k].ctx = nullptr;
    g->pgrad_host[k] = nullptr;
  }
  hipError_t e = hipMemset(g->dev, 0, sizeof(GfSlot) * g->host.size());
  if (e != hipSuccess) return fail(SLM_ERR_HIP, hipGetErrorString(e));
  return SLM_OK;
}

int slm_gf_eval_morph(slm_gf* g, int32_t n_frames, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, 0, n_frames, &d)) return rc;
  gf_enqueue_morph(g, 0, n_frames, d, (hipStream_t)stream, GF_EVAL_ZERO);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_gf_eval_losses(slm_gf* g, int32_t n_frames, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, 0, n_frames, &d)) return rc;
  gf_enqueue_eval(g, 0, n_frames, d, (hipStream_t)stream, 0);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_gf_step(slm_gf* g, int32_t n_frames, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, 0, n_frames, &d)) return rc;
  hipStream_t st = (hipStream_t)stream;
  gf_launch_step(g, 0, n_frames, d, 1, 0, 0, st);
  hipLaunchKernelGGL(k_gf_advance, dim3(n_frames), dim3(64), 0, st, g->dev, 1);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_gf_get_partial(slm_gf* g, int32_t slot, double* out, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, slot, 1, &d)) return rc;
  if (!out) return fail(SLM_ERR_INVALID, "slm_gf_get_partial: null output");
  const GfSlot& s = g->host[slot];
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(out, s.grad, sizeof(double) * d.maxP, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(out + d.maxP, s.terms, sizeof(double) * SLM_GF_NTERMS, hipMemcpyDeviceToDevice, st));
  return SLM_OK;
}

int slm_gf_set_partial(slm_gf* g, int32_t slot, const double* in, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, slot, 1, &d)) return rc;
  if (!in) return fail(SLM_ERR_INVALID, "slm_gf_set_partial: null input");
  const GfSlot& s = g->host[slot];
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(s.grad, in, sizeof(double) * d.maxP, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(s.terms, in + d.maxP, sizeof(double) * SLM_GF_NTERMS, hipMemcpyDeviceToDevice, st));
  return SLM_OK;
}

int slm_gf_run(slm_gf* g, int32_t n_frames, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, 0, n_frames, &d)) return rc;
  if (g->world > 1)
    return fail(SLM_ERR_UNSUPPORTED,
                   "slm_gf_run: surfels are sharded; drive slm_gf_eval_morph / eval_losses / step with an "
                   "all-reduce of slm_gf_get_partial between them");
  hipStream_t st = (hipStream_t)stream;
  // An iteration is TWO launches: the losses (k_gf_data with the node terms as its tail blocks) and the step, which folds the
  // block partials, assigns the loss terms and leaves gradient and partials zeroed for the next iteration; k_gf_zero only
  // runs in front of the first.  With the morphing term THREE: k_gf_morph in front -- its kept count stays in the spread
  // partials, k_gf_data sums the 64 copies itself and the step folds them with the rest (k_gf_zero + k_gf_morph + k_gf_fold +
  // k_gf_data + k_gf_step before: five launches of 5-85 us at configs[4]'s size).  The step counter advances once, behind the loop.
  const int n_it = g->cfg.num_iterations;
  for (int it = 0; it < n_it; ++it) {
    gf_enqueue_eval(g, 0, n_frames, d, st, GF_EVAL_PASS1 | GF_EVAL_IN_RUN | (it == 0 ? GF_EVAL_ZERO : 0));
    const int fold = GF_STEP_FOLD | GF_STEP_OWN | (it + 1 < n_it ? GF_STEP_REZERO : 0) | (g->cfg.use_bn_morph ? GF_STEP_MORPH : 0);
    gf_launch_step(g, 0, n_frames, d, 1, fold, it, st);
  }
  if (n_it > 0) hipLaunchKernelGGL(k_gf_advance, dim3(n_frames), dim3(64), 0, st, g->dev, n_it);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_gf_get_deform(slm_gf* g, int32_t slot, double* out, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, slot, 1, &d)) return rc;
  if (!out) return fail(SLM_ERR_INVALID, "slm_gf_get_deform: null output");
  HIPCHK(hipMemcpyAsync(out, g->host[slot].dv, sizeof(double) * d.maxP, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SLM_OK;
}

int slm_gf_loss_grad(slm_gf* g, int32_t slot, const double* dv, double* terms, double* grad, void* stream) {
  GfDims d;
  if (const int rc = gf_dims(g, slot, 1, &d)) return rc;
  if (!dv) return fail(SLM_ERR_INVALID, "slm_gf_loss_grad: null dv");
  if (g->world > 1 && g->cfg.use_bn_morph && (terms || grad))
    return fail(SLM_ERR_UNSUPPORTED,
                   "slm_gf_loss_grad: surfels are sharded and the boundary-morph term is on; its mean needs the global kept "
                   "count: drive slm_gf_eval_morph / eval_losses with an all-reduce of slm_gf_get_partial behind each (null "
                   "terms and grad only set deform_verts)");
  hipStream_t st = (hipStream_t)stream;
  const GfSlot& s = g->host[slot];
  HIPCHK(hipMemcpyAsync(s.dv, dv, sizeof(double) * d.maxP, hipMemcpyDeviceToDevice, st));
  gf_enqueue_eval(g, slot, 1, d, st, GF_EVAL_ZERO | GF_EVAL_PASS1);
  gf_launch_step(g, slot, 1, d, 0, 0, 0, st);   // (no step: the global row's division and the morphing term's mean)
  if (terms) HIPCHK(hipMemcpyAsync(terms, s.terms, sizeof(double) * SLM_GF_NTERMS, hipMemcpyDeviceToDevice, st));
  if (grad) HIPCHK(hipMemcpyAsync(grad, s.grad, sizeof(double) * d.maxP, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

}  // extern "C"

int gf_render_slot(slm_gf* g, int32_t slot, GfSlot** dev, int32_t* n_surfels, const char* who) {
  GfSlot* sp = nullptr;
  if (const int rc = gf_slot(who, GF_TEXTS_RENDER, g, true, slot, 1, true, &sp)) return rc;
  *dev = g->dev + slot;
  *n_surfels = sp->f.base.N;
  return SLM_OK;
}
