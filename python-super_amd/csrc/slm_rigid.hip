// slm_rigid.hip -- global rigid pre-alignment of the LM path (slm_rigid_*, include/super_lm.h): the reference's LM loop
// (super/LM.py:81-122) on ONE node at the origin with every surfel attached to it at weight 1 -- seven parameters
// beta_g = (q, t), data term + Rot term -- ahead of the node solve.
//
// A frame with one node and K = 1 pushed through the node solver puts every surfel's 7 x 7 block on the same 49 addresses.
// Here the whole frame is REDUCED instead:
//   k_rg_pass   per surfel the data term at the trial point (the rules of eval_surfel_coreT, slm_data.h, restated for
//               KK = 1, g = 0, w = 1 over the caller's raw (T,3) tables): 37 sums -- the 28 upper-triangle entries of
//               row row^T, the 7 of row r, r^2 and the match count.  Every RG_CHUNK = 256 consecutive surfels are one
//               PARTIAL: one surfel per thread, three col_reduce16 butterflies per wave (slm_lane.h), the four waves added
//               through LDS in wave order.  A workgroup walks the chunks blockIdx.x, + gridDim.x, ...: which workgroup
//               sums a chunk depends on the grid, what the partial holds does not.
//   k_rg_step   one wave per frame: adds the partials in index order (lane c owns entry c), then lane 0 accepts or rejects
//               the trial point, keeps the sums of the best point, adds the Rot term and u I, factors the 7 x 7 system by
//               Cholesky, solves, writes the next trial point and the record.
// So the loss of iteration i and the normal equations of iteration i + 1 come from ONE pass (same point, same match set),
// an iteration is two launches, nothing synchronises with the host and the frame index is blockIdx.y / blockIdx.x.
//
// Opt-in terms (slm_rigid_set_terms): k_rg_pass<CM, WT> adds the flow-correspondence rows of slm_corr.hip for one node at the
// origin (CM 1 point-point, 2 point-plane) and / or scales the data rows by the per-residual weight of slm_data.h (WT); the
// partial keeps its layout (two of its three free places take the term's sum of squares and count), k_rg_step its sum.
// <0, false> is the plain stage.  k_rg_corr_targets builds the targets of a raw frame from a flow (corr_target_of, slm_corr.h).
#include <algorithm>
#include <string>

#include <vector>

#include "slm_common.h"
#include "slm_corr.h"
#include "slm_data.h"
#include "slm_host.h"
#include "slm_lane.h"

#define RG_CHUNK 256      // surfels per partial = threads per workgroup of k_rg_pass
#define RG_NS 37          // sums per partial: 28 + 7 + r^2 + match count
#define RG_NV 40          // doubles per partial in HBM (padded)
#define RG_R2 35
#define RG_M 36
#define RG_RC 37          // the opt-in terms (slm_rigid_set_terms): sum |r_c|^2 of the correspondence rows ...
#define RG_KC 38          // ... and the count of surfels that contributed them; 0 in the plain stage
#define RG_MAX_GRID 512   // workgroups of k_rg_pass per frame: beyond 512 * 256 surfels a workgroup takes a second chunk
#define RG_INIT_BATCH 8   // frames handed to one k_rg_init launch (as kernel arguments)

// Per-slot state, resident in HBM as an array indexed by the frame's grid coordinate.
struct RigidSlot {
  slm_frame f;               // the caller's frame (read as FrameIn: global, not flat, accesses)
  double beta[7];            // the kept point (the best one in the test phase)
  double trial[7];           // the point the next pass evaluates
  double G[RG_NV];           // the sums at beta
  double u, v, minimal_loss;
  int32_t stopped;           // 1 after a failed factorisation: later kernels are no-ops for the slot
  int32_t m_grad;            // match count of the sums the pending step was solved from
  int32_t n_chunks;          // ceil(N / RG_CHUNK), 0 without surfels or without a target
  int32_t pad;
  GP<double> part;           // (n_chunks, RG_NV)
  GP<slm_iter_record> rec;   // (num_iterations)
};

// The inputs of a slot's opt-in terms, resident in HBM beside the slots (same index): the caller's arrays, read in place.
struct RigidTerms {
  GP<const double> o;        // (N,3) correspondence targets; null: the slot runs without the term
  GP<const double> n;        // (N,3) their normals (mode 2)
  GP<const uint8_t> valid;   // (N)
  DataWeightDev wd;          // semantic inputs of the weighted data term (has = 0: none)
};

struct slm_rigid {
  int corr_mode = 0, seg_mode = 0;     // slm_rigid_set_terms; all zero: the plain stage
  double corr_weight = 0.0, pp_max = 0.0;
  std::vector<RigidTerms> terms_h;     // host mirror, max_frames + 1
  DevBuf<RigidTerms> terms;            // written by k_rg_init on the run's stream
  int max_frames = 0;
  int last_iters = 0;                  // num_iterations of the last slm_rigid_run
  DevBuf<RigidSlot> slots;             // max_frames + 1: the last one belongs to slm_rigid_assemble
  DevBuf<double> part;                 // (max_frames + 1) x cap_chunks x RG_NV
  DevBuf<slm_iter_record> rec;         // max_frames x cap_iters
  size_t cap_chunks = 0, cap_iters = 0;
};

namespace {

struct RgInitArgs {
  slm_frame f[RG_INIT_BATCH];
  RigidTerms t[RG_INIT_BATCH];
};

// what the pass variants with terms are launched with
struct RgTermArgs {
  const RigidTerms* terms;   // indexed like the slots of the launch
  double corr_lam;
  DataWArgs wa;              // wa.wd stays null: the descriptor is the slot's RigidTerms::wd
};

// grid = (frames of this launch), block = 64: slot first + blockIdx.x <- the frame, beta = trial = beta0 (identity when
// null), fresh LM state and records
__global__ void __launch_bounds__(64) k_rg_init(RigidSlot* __restrict__ slots, RigidTerms* __restrict__ terms, int first, RgInitArgs a,
                                                slm_rigid_config cfg,
                                                double* part, size_t part_stride, slm_iter_record* rec, size_t rec_stride,
                                                const double* __restrict__ beta0) {
  const int k = blockIdx.x;
  RigidSlot& s = slots[first + k];
  for (int t = threadIdx.x; t < cfg.num_iterations; t += blockDim.x) {
    slm_iter_record r;
    r.loss = 0.0;
    r.u = 0.0;
    r.accepted = 0;
    r.status = SLM_ITER_NOT_RUN;
    r.M_grad = 0;
    r.M_loss = 0;
    rec[(size_t)(first + k) * rec_stride + t] = r;
  }
  if (threadIdx.x < 7) {
    const double b = beta0 ? beta0[threadIdx.x] : (threadIdx.x == 0 ? 1.0 : 0.0);
    s.beta[threadIdx.x] = b;
    s.trial[threadIdx.x] = b;
  }
  if (threadIdx.x < RG_NV) s.G[threadIdx.x] = 0.0;
  if (threadIdx.x == 0) {
    const slm_frame& f = a.f[k];
    s.f = f;
    terms[first + k] = a.t[k];
    s.u = cfg.u0;
    s.v = cfg.v;
    s.minimal_loss = cfg.minimal_loss0;
    s.stopped = 0;
    s.m_grad = 0;
    s.n_chunks = (f.N > 0 && f.T > 0) ? (int)(((long long)f.N + RG_CHUNK - 1) / RG_CHUNK) : 0;
    s.pad = 0;
    // (stored as plain pointers: GP<> has the layout of T*, and its constructor is host-only in the host pass)
    *reinterpret_cast<double**>(&s.part) = part + (size_t)(first + k) * part_stride;
    *reinterpret_cast<slm_iter_record**>(&s.rec) = rec + (size_t)(first + k) * rec_stride;
  }
}

// The data term of one surfel at beta_g = (qw, qv, tr): eval_surfel_coreT<1, 1> of slm_data.h for a node at the origin with
// weight 1 (T = R(q) p + t; adding g = 0 and scaling by w = 1 are exact), reading the target through index_map and the raw
// (T,3) tables.  A row number outside [0, T) counts as unmapped (the reference would raise; nothing is read out of bounds).
// Returns the match flag; r and row[7] = lam [c dR(q)p/dq | c] are set when matched.  TAPS (the weighted variants): also the
// four tap rows, their bilinear weights and ne = n.e without lambda, what data_weight (slm_data.h) reads.
template <bool TAPS>
__device__ __forceinline__ bool rg_eval(const FrameIn& f, const d3 T, const d3 p, const double qw, const d3 qv, const double lam,
                                        double& r, double row[7], int taps[4], double tapw[4], double& ne) {

  // ---- projection + validity on ROUNDED coordinates ----
  const double fx = (double)f.fx, fy = (double)f.fy, cx = (double)f.cx, cy = (double)f.cy;
  const double Ze = T.z + 1e-8;
  const double u_ = T.x * fx / Ze + cx;
  const double v_ = T.y * fy / Ze + cy;
  const double ur = rint(u_), vr = rint(v_);   // torch.round: half to even
  const int H = f.H, W = f.W, NT = f.T;
  const bool pv = vr >= 0.0 && vr < (double)(H - 1) && ur >= 0.0 && ur < (double)(W - 1);   // false for NaN
  const double fv = floor(v_), cv = ceil(v_), fu = floor(u_), cu = ceil(u_);
  const double nn[4] = {fv, fv, cv, cv};
  const double mm[4] = {fu, cu, fu, cu};
  const int coords = pv ? (int)vr * W + (int)ur : 0;
  const uint8_t tv = pv ? f.tgt_valid[coords] : (uint8_t)0;
  int rows[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ni = (int)nn[t], mi = (int)mm[t];
    const bool inside = pv && (ni >= 0) && (ni < H) && (mi >= 0) && (mi < W);
    rows[t] = inside ? f.index_map[ni * W + mi] : -1;
  }
  if (!tv) return false;
  bool all_ok = true;
#pragma unroll
  for (int t = 0; t < 4; ++t) all_ok = all_ok && ((unsigned)rows[t] < (unsigned)NT);
  if (!all_ok) return false;   // NaN fill -> surfel dropped
  // the eight tap loads together
  float tp[4][3], tn[4][3];
  const float* __restrict__ tpts = f.tgt_points;
  const float* __restrict__ tnrm = f.tgt_norms;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      tp[t][c] = tpts[3 * (size_t)rows[t] + c];
      tn[t][c] = tnrm[3 * (size_t)rows[t] + c];
    }
  d3 o = {0, 0, 0}, n = {0, 0, 0};
  d3 dou = {0, 0, 0}, dov = {0, 0, 0}, dnu = {0, 0, 0}, dnv = {0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double dn = nn[t] - v_, dm = mm[t] - u_;
    const double an = fmax(1.0 - fabs(dn), 0.0), am = fmax(1.0 - fabs(dm), 0.0);
    const d3 P = {(double)tp[t][0], (double)tp[t][1], (double)tp[t][2]};
    const d3 Nn = {(double)tn[t][0], (double)tn[t][1], (double)tn[t][2]};
    const double wv = an * am;
    if (TAPS) {
      taps[t] = rows[t];
      tapw[t] = wv;
    }
    o = {o.x + P.x * wv, o.y + P.y * wv, o.z + P.z * wv};
    n = {n.x + Nn.x * wv, n.y + Nn.y * wv, n.z + Nn.z * wv};
    const double sn = dn >= 0.0 ? 1.0 : -1.0, sm = dm >= 0.0 ? 1.0 : -1.0;
    const double gu = an * sm, gv = am * sn;   // d/du, d/dv weights
    dou = {dou.x + P.x * gu, dou.y + P.y * gu, dou.z + P.z * gu};
    dov = {dov.x + P.x * gv, dov.y + P.y * gv, dov.z + P.z * gv};
    dnu = {dnu.x + Nn.x * gu, dnu.y + Nn.y * gu, dnu.z + Nn.z * gu};
    dnv = {dnv.x + Nn.x * gv, dnv.y + Nn.y * gv, dnv.z + Nn.z * gv};
  }
  // NaN in the tables behaves like the reference's isnan filter
  if (!(o.x == o.x && o.y == o.y && o.z == o.z && n.x == n.x && n.y == n.y && n.z == n.z)) return false;

  const d3 e = T - o;
  if (TAPS) {
    ne = dot(n, e);
    r = lam * ne;
  } else {
    r = lam * dot(n, e);
  }
  // ---- c = n^T (I - A) + e^T B, A = do/d(u,v) Pi, B = dn/d(u,v) Pi ----
  const double Z = T.z;   // no epsilon in dPi
  const d3 Pi0 = {fx / Z, 0.0, -fx * T.x / (Z * Z)};
  const d3 Pi1 = {0.0, fy / Z, -fy * T.y / (Z * Z)};
  const double s0 = dot(e, dnu) - dot(n, dou);
  const double s1 = dot(e, dnv) - dot(n, dov);
  const d3 c = {n.x + s0 * Pi0.x + s1 * Pi1.x, n.y + s0 * Pi0.y + s1 * Pi1.y, n.z + s0 * Pi0.z + s1 * Pi1.z};
  double jq[4];
  quat_jac_row(qw, qv, p, c, jq);
  row[0] = lam * jq[0];
  row[1] = lam * jq[1];
  row[2] = lam * jq[2];
  row[3] = lam * jq[3];
  row[4] = lam * c.x;
  row[5] = lam * c.y;
  row[6] = lam * c.z;
  return true;
}

// grid = (min(chunks of the largest frame, RG_MAX_GRID), frames), block = RG_CHUNK
// CM: correspondence rows (slm_rigid_set_terms) 0 none / 1 point-point / 2 point-plane; WT: the data rows carry the
// per-residual weight of data_weight (slm_data.h).  <0, false> is the plain stage: what a context without terms launches.
// A surfel with valid_i adds the rows lam_c [c dR(q)p/dq | c], r = lam_c c.(R(q)p + t - o_i), c = e_x, e_y, e_z (CM 1) or n_i
// (CM 2), into the same 28 + 7 sums, one row at a time through the data row's registers, whether or not the data term matched
// it; their sum of squares and the count of such surfels go to RG_RC / RG_KC.  WT: row and r scaled by sqrt(w), w at this
// point from s = (n.e)^2 without lambda; the match count stays the match set's (weight 0 is matched and adds nothing).
template <int CM, bool WT>
__global__ void __launch_bounds__(RG_CHUNK) k_rg_pass(const RigidSlot* __restrict__ slots, double lam, RgTermArgs ta) {
  __shared__ double s_part[4 * 48];
  const RigidSlot& s = slots[blockIdx.y];
  if (s.stopped) return;
  const int nc = s.n_chunks;
  if ((int)blockIdx.x >= nc) return;
  const FrameIn& f = reinterpret_cast<const FrameIn&>(s.f);
  const double qw = s.trial[0];
  const d3 qv = {s.trial[1], s.trial[2], s.trial[3]};
  const d3 tr = {s.trial[4], s.trial[5], s.trial[6]};
  const int N = f.N, f64 = f.state_f64;
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int ch = blockIdx.x; ch < nc; ch += gridDim.x) {
    const long long i = (long long)ch * RG_CHUNK + threadIdx.x;
    double vals[48];
#pragma unroll
    for (int a = 0; a < 48; ++a) vals[a] = 0.0;
    if (i < N) {
      double r, row[7], ne = 0.0;
      int taps[4];
      double tapw[4];
      const d3 p = ld_state3(f.sf_points, (size_t)i, f64);
      d3 T = quat_apply(qw, qv, p);
      T = {T.x + tr.x, T.y + tr.y, T.z + tr.z};
      if (rg_eval<WT>(f, T, p, qw, qv, lam, r, row, taps, tapw, ne)) {
        if (WT) {
          const double sw = sqrt(data_weight(ta.wa, &ta.terms[blockIdx.y].wd, (int)i, ne * ne, taps, tapw));
          r *= sw;
#pragma unroll
          for (int a = 0; a < 7; ++a) row[a] *= sw;
        }
        int e = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
          for (int b = a; b < 7; ++b) vals[e++] = row[a] * row[b];
#pragma unroll
        for (int a = 0; a < 7; ++a) vals[28 + a] = row[a] * r;
        vals[RG_R2] = r * r;
        vals[RG_M] = 1.0;
      }
      if (CM != 0) {
        const RigidTerms& tm = ta.terms[blockIdx.y];
        const double* __restrict__ co = tm.o;
        if (co && tm.valid[i]) {
          const d3 ec = {T.x - co[3 * (size_t)i], T.y - co[3 * (size_t)i + 1], T.z - co[3 * (size_t)i + 2]};
          d3 nc3 = {0.0, 0.0, 0.0};
          if (CM == 2) {
            const double* __restrict__ cn = tm.n;
            nc3 = {cn[3 * (size_t)i], cn[3 * (size_t)i + 1], cn[3 * (size_t)i + 2]};
          }
          const double cl = ta.corr_lam;
#pragma unroll
          for (int comp = 0; comp < (CM == 1 ? 3 : 1); ++comp) {
            const d3 c = CM == 2 ? nc3 : d3{comp == 0 ? 1.0 : 0.0, comp == 1 ? 1.0 : 0.0, comp == 2 ? 1.0 : 0.0};
            double jq[4];
            quat_jac_row(qw, qv, p, c, jq);
            row[0] = cl * jq[0];
            row[1] = cl * jq[1];
            row[2] = cl * jq[2];
            row[3] = cl * jq[3];
            row[4] = cl * c.x;
            row[5] = cl * c.y;
            row[6] = cl * c.z;
            r = cl * dot(c, ec);
            int e = 0;
#pragma unroll
            for (int a = 0; a < 7; ++a)
#pragma unroll
              for (int b = a; b < 7; ++b) vals[e++] += row[a] * row[b];
#pragma unroll
            for (int a = 0; a < 7; ++a) vals[28 + a] += row[a] * r;
            vals[RG_RC] += r * r;
          }
          vals[RG_KC] = 1.0;
        }
      }
    }
    // lane 4 a of a wave receives the wave's sum of value a of each group of 16 (col_reduce16)
    const double r0 = col_reduce16(vals), r1 = col_reduce16(vals + 16), r2 = col_reduce16(vals + 32);
    if ((l & 3) == 0) {
      double* q = s_part + wv * 48 + (l >> 2);
      q[0] = r0;
      q[16] = r1;
      q[32] = r2;
    }
    __syncthreads();
    if (threadIdx.x < RG_NV) {
      const int a = threadIdx.x;
      s.part[(size_t)ch * RG_NV + a] = ((s_part[a] + s_part[48 + a]) + s_part[96 + a]) + s_part[144 + a];
    }
    __syncthreads();
  }
}

// the slot's partials added in index order: entry c by lane c, into P[RG_NV] in LDS (one wave)
__device__ __forceinline__ void rg_reduce(const RigidSlot& s, double* P) {
  const int c = threadIdx.x;
  if (c < RG_NV) {
    const double* __restrict__ q = s.part.get() + c;
    const int nc = s.n_chunks;
    double acc = 0.0;
    int ch = 0;
    for (; ch + 8 <= nc; ch += 8) {
      double t[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) t[k] = q[(size_t)(ch + k) * RG_NV];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += t[k];
    }
    for (; ch < nc; ++ch) acc += q[(size_t)ch * RG_NV];
    P[c] = acc;
  }
  __syncthreads();
}

// Rot term at b (lm_oracle.rot_term): residual and Jacobian row in float32, widened; their products are float64
__device__ __forceinline__ void rg_rot(const double b[7], double lam_r, double& r, double jq[4]) {
#pragma clang fp contract(off)   // mul and add separately rounded, like the reference's f32 ops
  const float lam32 = (float)lam_r;
  float q[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = (float)b[c];
  float sq = q[0] * q[0];
  sq = sq + q[1] * q[1];
  sq = sq + q[2] * q[2];
  sq = sq + q[3] * q[3];
  r = (double)(lam32 * (1.0f - sq));
#pragma unroll
  for (int c = 0; c < 4; ++c) jq[c] = (double)((-lam32 * 2.0f) * q[c]);
}

// A (7,7) full symmetric = data sums + Rot, rhs = jtl = -J^T r, at point b with the data sums G
__device__ __forceinline__ void rg_system(const double* G, const double b[7], double lam_r, double A[7][7], double rhs[7],
                                          double& rot_r) {
  int e = 0;
#pragma unroll
  for (int a = 0; a < 7; ++a)
#pragma unroll
    for (int c = a; c < 7; ++c) {
      A[a][c] = G[e];
      A[c][a] = G[e];
      ++e;
    }
#pragma unroll
  for (int a = 0; a < 7; ++a) rhs[a] = -G[28 + a];
  double jq[4];
  rg_rot(b, lam_r, rot_r, jq);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    rhs[a] -= jq[a] * rot_r;
#pragma unroll
    for (int c = 0; c < 4; ++c) A[a][c] += jq[a] * jq[c];
  }
}

// in-place lower Cholesky of A and the solve A x = rhs; false when a pivot is not > 0 (NaN included)
__device__ __forceinline__ bool rg_chol_solve(double A[7][7], const double rhs[7], double x[7]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    ok = ok && (d > 0.0);
    const double ljj = sqrt(d);
    A[j][j] = ljj;
    const double inv = 1.0 / ljj;
#pragma unroll
    for (int i = j + 1; i < 7; ++i) {
      double t = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= A[i][k] * A[j][k];
      A[i][j] = t * inv;
    }
  }
  double y[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    double t = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= A[i][k] * y[k];
    y[i] = t / A[i][i];
  }
#pragma unroll
  for (int i = 6; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < 7; ++k) t -= A[k][i] * x[k];
    x[i] = t / A[i][i];
  }
  return ok;
}

// grid = (frames), block = 64.  stage 0: the pass ran at beta itself (identity): keep its sums, solve the first step.
// stage s >= 1: the pass ran at the trial point of iteration s - 1: accept or reject it, record; solve iteration s if any.
__global__ void __launch_bounds__(64) k_rg_step(RigidSlot* __restrict__ slots, int stage, int n_iter, int phase_test,
                                                double lam_r) {
  __shared__ double P[RG_NV];
  RigidSlot& s = slots[blockIdx.x];
  if (s.stopped) return;
  rg_reduce(s, P);
  if (threadIdx.x != 0) return;
  double b[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) b[c] = s.beta[c];
  bool take = true;   // the sums of the pass become the sums at beta
  if (stage > 0) {
    double tb[7], rr, jq[4];
#pragma unroll
    for (int c = 0; c < 7; ++c) tb[c] = s.trial[c];
    rg_rot(tb, lam_r, rr, jq);
    const double loss = (P[RG_R2] + P[RG_RC]) + rr * rr;   // weighted data + correspondence (0 without the term) + Rot
    const double u_used = s.u;
    int acc = 1;
    if (phase_test) {
      if (loss < s.minimal_loss) {
        s.minimal_loss = loss;
        s.u = u_used / s.v;
      } else {
        acc = 0;
        s.u = u_used * s.v;
      }
    }
    slm_iter_record r;
    r.loss = loss;
    r.u = u_used;
    r.accepted = acc;
    r.status = SLM_ITER_OK;
    r.M_grad = s.m_grad;
    r.M_loss = (int)P[RG_M];
    s.rec[stage - 1] = r;
    take = acc != 0;
    if (take) {
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        b[c] = tb[c];
        s.beta[c] = tb[c];
      }
    }
  }
  double G[RG_NS];
  if (take) {
#pragma unroll
    for (int c = 0; c < RG_NS; ++c) {
      G[c] = P[c];
      s.G[c] = P[c];
    }
    s.G[RG_RC] = P[RG_RC];
    s.G[RG_KC] = P[RG_KC];
  } else {
#pragma unroll
    for (int c = 0; c < RG_NS; ++c) G[c] = s.G[c];
  }
  if (stage >= n_iter) return;
  double A[7][7], rhs[7], x[7], rot_r;
  rg_system(G, b, lam_r, A, rhs, rot_r);
  const double u = s.u;
#pragma unroll
  for (int a = 0; a < 7; ++a) A[a][a] += u;
  s.m_grad = (int)G[RG_M];
  if (!rg_chol_solve(A, rhs, x)) {   // "Solver failed: Ill-posed system!": the frame's loop ends here
    slm_iter_record r = s.rec[stage];
    r.status = SLM_ITER_SOLVER_FAILED;
    r.u = u;
    r.M_grad = (int)G[RG_M];
    s.rec[stage] = r;
    s.stopped = 1;
    return;
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) s.trial[c] = b[c] + x[c];
}

// grid = 1, block = 64: the system and the loss of the pass that just ran at the slot's trial point (slm_rigid_assemble)
__global__ void __launch_bounds__(64) k_rg_assemble_out(RigidSlot* __restrict__ slots, int slot, double lam_r,
                                                        double* __restrict__ jtj, double* __restrict__ jtl,
                                                        double* __restrict__ loss_m) {
  __shared__ double P[RG_NV];
  RigidSlot& s = slots[slot];
  rg_reduce(s, P);
  if (threadIdx.x < RG_NV) s.G[threadIdx.x] = P[threadIdx.x];   // the sums at the point: what slm_rigid_get_terms reads
  if (threadIdx.x != 0) return;
  double b[7], A[7][7], rhs[7], rot_r;
#pragma unroll
  for (int c = 0; c < 7; ++c) b[c] = s.trial[c];
  rg_system(P, b, lam_r, A, rhs, rot_r);
  if (jtj)
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int c = 0; c < 7; ++c) jtj[7 * a + c] = A[a][c];
  if (jtl)
#pragma unroll
    for (int a = 0; a < 7; ++a) jtl[a] = rhs[a];
  if (loss_m) {
    loss_m[0] = (P[RG_R2] + P[RG_RC]) + rot_r * rot_r;
    loss_m[1] = P[RG_M];
  }
}

// out[7] <- the slot's beta, its quaternion normalised when asked for
__global__ void __launch_bounds__(64) k_rg_get(const RigidSlot* __restrict__ slots, int slot, int normalise,
                                               double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const RigidSlot& s = slots[slot];
  double b[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) b[c] = s.beta[c];
  if (normalise) {
    const double nq = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = b[c] / nq;
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) out[c] = b[c];
}

// out[4] <- {sum w r^2, matched count, sum |r_c|^2, kept count} of the sums kept at the slot's beta
__global__ void __launch_bounds__(64) k_rg_get_terms(const RigidSlot* __restrict__ slots, int slot, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const RigidSlot& s = slots[slot];
  out[0] = s.G[RG_R2];
  out[1] = s.G[RG_M];
  out[2] = s.G[RG_RC];
  out[3] = s.G[RG_KC];
}

// grid = (ceil(N / 256)): the correspondence targets of a raw frame from the flow (2,H,W) (corr_target_of, slm_corr.h)
__global__ void __launch_bounds__(256) k_rg_corr_targets(slm_frame fr, const float* __restrict__ flow, double* __restrict__ o,
                                                          double* __restrict__ n, uint8_t* __restrict__ valid) {
  const FrameIn& f = reinterpret_cast<const FrameIn&>(fr);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.N) return;
  corr_target_of(f, i, flow, o, n, valid);
}

// p <- R(q) p + t, nrm <- F.normalize(R(q) nrm), in place; T float or double
template <typename T>
__global__ void __launch_bounds__(256) k_rg_transform(int n, T* __restrict__ pts, T* __restrict__ nrm,
                                                      const double* __restrict__ tg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double qw = tg[0];
  const d3 qv = {tg[1], tg[2], tg[3]};
  if (pts) {
    T* q = pts + 3 * (size_t)i;
    const d3 x = quat_apply(qw, qv, {(double)q[0], (double)q[1], (double)q[2]});
    q[0] = (T)(x.x + tg[4]);
    q[1] = (T)(x.y + tg[5]);
    q[2] = (T)(x.z + tg[6]);
  }
  if (nrm) {
    T* q = nrm + 3 * (size_t)i;
    const d3 x = quat_apply(qw, qv, {(double)q[0], (double)q[1], (double)q[2]});
    const double len = fmax(sqrt(x.x * x.x + x.y * x.y + x.z * x.z), 1e-12);
    q[0] = (T)(x.x / len);
    q[1] = (T)(x.y / len);
    q[2] = (T)(x.z / len);
  }
}

int check_frame(const char* fn, const slm_frame& f) {
  const std::string pre = std::string(fn) + ": ";
  if (f.H < 2 || f.W < 2) return fail(SLM_ERR_INVALID, pre + "H and W must be >= 2");
  if (f.N < 0 || f.T < 0) return fail(SLM_ERR_INVALID, pre + "N and T must be >= 0");
  if (f.N > 0 && !f.sf_points) return fail(SLM_ERR_INVALID, pre + "N > 0 needs sf_points");
  if (f.T > 0 && (!f.tgt_points || !f.tgt_norms || !f.index_map || !f.tgt_valid))
    return fail(SLM_ERR_INVALID, pre + "T > 0 needs tgt_points, tgt_norms, index_map and tgt_valid");
  return SLM_OK;
}

size_t frame_chunks(const slm_frame& f) {
  return (f.N > 0 && f.T > 0) ? ((size_t)f.N + RG_CHUNK - 1) / RG_CHUNK : 0;
}

// room for `chunks` partials per slot and `iters` records per slot (grow-only, with head-room)
hipError_t ensure(slm_rigid* r, size_t chunks, size_t iters) {
  const size_t ns = (size_t)r->max_frames + 1;
  if (chunks > r->cap_chunks) {
    const size_t want = chunks + chunks / 4 + 16;
    r->cap_chunks = 0;
    HIPRET(r->part.grow(ns * want * RG_NV + 1, ns * want * RG_NV + 1));
    r->cap_chunks = want;
  }
  if (iters > r->cap_iters) {
    const size_t want = iters + 6;
    r->cap_iters = 0;
    HIPRET(r->rec.grow(ns * want + 1, ns * want + 1));
    r->cap_iters = want;
  }
  return hipSuccess;
}

void launch_init(slm_rigid* r, int first, int n, const slm_frame* frames, const slm_rigid_config& cfg, const double* beta0,
                 hipStream_t st) {
  for (int b = 0; b < n; b += RG_INIT_BATCH) {
    RgInitArgs a = {};
    const int m = std::min(RG_INIT_BATCH, n - b);
    for (int k = 0; k < m; ++k) {
      a.f[k] = frames[b + k];
      a.t[k] = r->terms_h[first + b + k];
    }
    hipLaunchKernelGGL(k_rg_init, dim3(m), dim3(64), 0, st, r->slots.p, r->terms.p, first + b, a, cfg, r->part.p,
                       r->cap_chunks * RG_NV, r->rec.p, r->cap_iters, beta0);
  }
}

// the pass of slots [first, first + n): the plain kernel unless the context carries terms that a slot of the launch uses
void launch_pass(slm_rigid* r, int first, int n, size_t max_chunks, double lam, hipStream_t st) {
  const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>(max_chunks, RG_MAX_GRID));
  const dim3 grid(gx, n), blk(RG_CHUNK);
  int cm = 0;
  if (r->corr_mode)
    for (int k = first; k < first + n; ++k)
      if (r->terms_h[k].o.get()) cm = r->corr_mode;
  const bool wt = r->seg_mode != 0 || r->pp_max > 0.0;
  RgTermArgs ta = {};
  ta.terms = r->terms.p + first;
  ta.corr_lam = r->corr_weight;
  ta.wa.wd = nullptr;
  ta.wa.pp_max = r->pp_max;
  ta.wa.seg_mode = r->seg_mode;
  const RigidSlot* sl = r->slots.p + first;
#define RG_PASS(CM, WT) hipLaunchKernelGGL((k_rg_pass<CM, WT>), grid, blk, 0, st, sl, lam, ta)
  if (!wt) {
    if (cm == 0) RG_PASS(0, false);
    else if (cm == 1) RG_PASS(1, false);
    else RG_PASS(2, false);
  } else {
    if (cm == 0) RG_PASS(0, true);
    else if (cm == 1) RG_PASS(1, true);
    else RG_PASS(2, true);
  }
#undef RG_PASS
}

// with a semantic weight every slot of the call needs its inputs: no silent unweighted run
int check_semantic(const char* fn, const slm_rigid* r, int first, int n) {
  if (!r->seg_mode) return SLM_OK;
  for (int k = first; k < first + n; ++k)
    if (!r->terms_h[k].wd.has)
      return fail(SLM_ERR_UNBOUND, std::string(fn) + ": slot " + std::to_string(k) + " has no semantic inputs; call slm_rigid_set_semantic");
  return SLM_OK;
}

}  // namespace

extern "C" {

int slm_rigid_abi_check(int32_t sizeof_slm_rigid_config) {
  if (sizeof_slm_rigid_config != (int32_t)sizeof(slm_rigid_config))
    return fail(SLM_ERR_INVALID, "slm_rigid_abi_check: caller's slm_rigid_config has " + std::to_string(sizeof_slm_rigid_config) +
                                     " bytes, the library's " + std::to_string(sizeof(slm_rigid_config)));
  return SLM_OK;
}

int slm_rigid_create(int32_t max_frames, slm_rigid** out) {
  if (!out) return fail(SLM_ERR_INVALID, "slm_rigid_create: null argument");
  if (max_frames < 1) return fail(SLM_ERR_INVALID, "slm_rigid_create: max_frames must be >= 1");
  if (slm_device_count() < 1) return fail(SLM_ERR_NO_DEVICE, "slm_rigid_create: no HIP device visible");
  slm_rigid* r = new slm_rigid();
  r->max_frames = max_frames;
  const size_t ns = (size_t)max_frames + 1;
  r->terms_h.assign(ns, RigidTerms{});
  hipError_t e = r->slots.grow(ns, ns);
  if (e == hipSuccess) e = hipMemset(r->slots.p, 0, sizeof(RigidSlot) * ns);
  if (e == hipSuccess) e = r->terms.grow(ns, ns);
  if (e == hipSuccess) e = hipMemset(r->terms.p, 0, sizeof(RigidTerms) * ns);
  if (e == hipSuccess) e = ensure(r, 64, 10);
  if (e == hipSuccess) {   // every slot reads as a finished run at identity before its first run
    slm_rigid_config cfg = {};
    slm_frame f = {};
    for (size_t k = 0; k < ns; ++k) launch_init(r, (int)k, 1, &f, cfg, nullptr, nullptr);
    e = hipDeviceSynchronize();
  }
  if (e != hipSuccess) {
    slm_rigid_destroy(r);
    return fail(SLM_ERR_HIP, std::string("slm_rigid_create: ") + hipGetErrorString(e));
  }
  *out = r;
  return SLM_OK;
}

int slm_rigid_destroy(slm_rigid* r) {
  delete r;
  return SLM_OK;
}

int slm_rigid_run(slm_rigid* r, const slm_rigid_config* cfg, int32_t n_frames, const slm_frame* frames, void* stream) {
  if (!r || !cfg || !frames) return fail(SLM_ERR_INVALID, "slm_rigid_run: null argument");
  if (n_frames < 1 || n_frames > r->max_frames) return fail(SLM_ERR_INVALID, "slm_rigid_run: n_frames must be in 1..max_frames");
  if (cfg->num_iterations < 0) return fail(SLM_ERR_INVALID, "slm_rigid_run: num_iterations must be >= 0");
  size_t max_chunks = 0;
  for (int k = 0; k < n_frames; ++k) {
    if (const int rc = check_frame("slm_rigid_run", frames[k])) return rc;
    max_chunks = std::max(max_chunks, frame_chunks(frames[k]));
  }
  if (const int rc = check_semantic("slm_rigid_run", r, 0, n_frames)) return rc;
  HIPCHK(ensure(r, max_chunks, (size_t)cfg->num_iterations));
  hipStream_t st = (hipStream_t)stream;
  const int n_iter = cfg->num_iterations;
  r->last_iters = n_iter;
  launch_init(r, 0, n_frames, frames, *cfg, nullptr, st);
  if (n_iter > 0)
    for (int stage = 0; stage <= n_iter; ++stage) {
      launch_pass(r, 0, n_frames, max_chunks, cfg->w_data, st);
      hipLaunchKernelGGL(k_rg_step, dim3(n_frames), dim3(64), 0, st, r->slots.p, stage, n_iter, cfg->phase_test, cfg->w_rot);
    }
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

static int rg_get(const char* fn, slm_rigid* r, int32_t slot, int normalise, double* out, void* stream) {
  if (!r || !out) return fail(SLM_ERR_INVALID, std::string(fn) + ": null argument");
  if (slot < 0 || slot >= r->max_frames) return fail(SLM_ERR_INVALID, std::string(fn) + ": bad slot");
  hipLaunchKernelGGL(k_rg_get, dim3(1), dim3(64), 0, (hipStream_t)stream, r->slots.p, slot, normalise, out);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_rigid_get(slm_rigid* r, int32_t slot, double* Tg7_device, void* stream) {
  return rg_get("slm_rigid_get", r, slot, 1, Tg7_device, stream);
}

int slm_rigid_get_beta(slm_rigid* r, int32_t slot, double* beta7_device, void* stream) {
  return rg_get("slm_rigid_get_beta", r, slot, 0, beta7_device, stream);
}

int slm_rigid_get_records(slm_rigid* r, int32_t slot, slm_iter_record* host_out, int32_t max_records, int32_t* n_out,
                          void* stream) {
  if (!r || !host_out) return fail(SLM_ERR_INVALID, "slm_rigid_get_records: null argument");
  if (slot < 0 || slot >= r->max_frames) return fail(SLM_ERR_INVALID, "slm_rigid_get_records: bad slot");
  if (max_records < 0) return fail(SLM_ERR_INVALID, "slm_rigid_get_records: max_records must be >= 0");
  const int n = std::min(max_records, r->last_iters);
  hipStream_t st = (hipStream_t)stream;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(host_out, r->rec.p + (size_t)slot * r->cap_iters, sizeof(slm_iter_record) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n_out) *n_out = n;
  return SLM_OK;
}

int slm_rigid_assemble(slm_rigid* r, const slm_rigid_config* cfg, const slm_frame* frame, const double* beta7_device,
                       double* JtJ49_device, double* jtl7_device, double* loss_M_device, void* stream) {
  if (!r || !cfg || !frame || !beta7_device) return fail(SLM_ERR_INVALID, "slm_rigid_assemble: null argument");
  if (cfg->num_iterations < 0) return fail(SLM_ERR_INVALID, "slm_rigid_assemble: num_iterations must be >= 0");
  if (const int rc = check_frame("slm_rigid_assemble", *frame)) return rc;
  if (const int rc = check_semantic("slm_rigid_assemble", r, r->max_frames, 1)) return rc;
  const size_t chunks = frame_chunks(*frame);
  HIPCHK(ensure(r, chunks, 0));
  hipStream_t st = (hipStream_t)stream;
  slm_rigid_config c0 = *cfg;
  c0.num_iterations = 0;   // the slot of this call keeps no records
  const int slot = r->max_frames;
  launch_init(r, slot, 1, frame, c0, beta7_device, st);
  launch_pass(r, slot, 1, chunks, cfg->w_data, st);
  hipLaunchKernelGGL(k_rg_assemble_out, dim3(1), dim3(64), 0, st, r->slots.p, slot, cfg->w_rot, JtJ49_device, jtl7_device,
                     loss_M_device);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_rigid_set_terms(slm_rigid* r, int32_t corr_mode, double corr_weight, int32_t seg_mode, double pp_max) {
  if (!r) return fail(SLM_ERR_INVALID, "slm_rigid_set_terms: null argument");
  if (corr_mode < 0 || corr_mode > 2)
    return fail(SLM_ERR_INVALID, "slm_rigid_set_terms: corr_mode must be 0 (none), 1 (point-point) or 2 (point-plane)");
  if (!(corr_weight - corr_weight == 0.0)) return fail(SLM_ERR_INVALID, "slm_rigid_set_terms: corr_weight must be finite");
  if (seg_mode < 0 || seg_mode > 2) return fail(SLM_ERR_INVALID, "slm_rigid_set_terms: seg_mode must be 0 (none), 1 (hard) or 2 (soft)");
  if (!(pp_max - pp_max == 0.0) || pp_max < 0.0) return fail(SLM_ERR_INVALID, "slm_rigid_set_terms: pp_max must be finite and >= 0");
  r->corr_mode = corr_mode;
  r->corr_weight = corr_weight;
  r->seg_mode = seg_mode;
  r->pp_max = pp_max;
  r->terms_h.assign((size_t)r->max_frames + 1, RigidTerms{});   // every call clears every slot's inputs
  return SLM_OK;
}

int slm_rigid_set_corr(slm_rigid* r, int32_t slot, const double* pts, const double* nrm, const uint8_t* valid) {
  if (!r) return fail(SLM_ERR_INVALID, "slm_rigid_set_corr: null argument");
  if (slot < 0 || slot > r->max_frames) return fail(SLM_ERR_INVALID, "slm_rigid_set_corr: bad slot");
  if (!r->corr_mode) return fail(SLM_ERR_INVALID, "slm_rigid_set_corr: the correspondence term is off; call slm_rigid_set_terms with corr_mode 1 or 2 first");
  RigidTerms& t = r->terms_h[slot];
  if (!pts) {   // clears
    t.o = nullptr;
    t.n = nullptr;
    t.valid = nullptr;
    return SLM_OK;
  }
  if (!valid) return fail(SLM_ERR_INVALID, "slm_rigid_set_corr: null argument");
  if (r->corr_mode == 2 && !nrm) return fail(SLM_ERR_INVALID, "slm_rigid_set_corr: corr_mode 2 (point-plane) needs nrm");
  t.o = pts;
  t.n = nrm;
  t.valid = valid;
  return SLM_OK;
}

int slm_rigid_set_semantic(slm_rigid* r, int32_t slot, int32_t num_classes, const int32_t* sf_seg, const float* sf_seg_conf,
                           const float* tgt_seg_conf) {
  if (!r) return fail(SLM_ERR_INVALID, "slm_rigid_set_semantic: null argument");
  if (slot < 0 || slot > r->max_frames) return fail(SLM_ERR_INVALID, "slm_rigid_set_semantic: bad slot");
  if (!r->seg_mode) return fail(SLM_ERR_INVALID, "slm_rigid_set_semantic: the semantic weight is off; call slm_rigid_set_terms with seg_mode 1 or 2 first");
  DataWeightDev& w = r->terms_h[slot].wd;
  if (!sf_seg) {   // clears
    w = DataWeightDev{};
    return SLM_OK;
  }
  if (!sf_seg_conf || !tgt_seg_conf) return fail(SLM_ERR_INVALID, "slm_rigid_set_semantic: null argument");
  if (num_classes < 1 || num_classes > SLM_MAX_CLASSES)
    return fail(SLM_ERR_UNSUPPORTED, "slm_rigid_set_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)");
  w.sf_seg = const_cast<int32_t*>(sf_seg);
  w.sf_seg_conf = const_cast<float*>(sf_seg_conf);
  w.tgt_seg_conf = const_cast<float*>(tgt_seg_conf);
  w.C = num_classes;
  w.has = 1;
  return SLM_OK;
}

int slm_rigid_corr_targets(const slm_frame* frame, const float* flow, double* pts, double* nrm, uint8_t* valid, void* stream) {
  if (!frame || !flow || !pts || !nrm || !valid) return fail(SLM_ERR_INVALID, "slm_rigid_corr_targets: null argument");
  if (const int rc = check_frame("slm_rigid_corr_targets", *frame)) return rc;
  if (frame->N == 0) return SLM_OK;
  if (frame->T == 0) return fail(SLM_ERR_INVALID, "slm_rigid_corr_targets: T must be > 0");
  hipLaunchKernelGGL(k_rg_corr_targets, dim3((frame->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, *frame, flow, pts, nrm, valid);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_rigid_get_terms(slm_rigid* r, int32_t slot, double* out4_device, void* stream) {
  if (!r || !out4_device) return fail(SLM_ERR_INVALID, "slm_rigid_get_terms: null argument");
  if (slot < 0 || slot > r->max_frames) return fail(SLM_ERR_INVALID, "slm_rigid_get_terms: bad slot");
  hipLaunchKernelGGL(k_rg_get_terms, dim3(1), dim3(64), 0, (hipStream_t)stream, r->slots.p, slot, out4_device);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

int slm_rigid_transform(int32_t n, void* points, void* norms, int32_t f64, const double* Tg7_device, void* stream) {
  if (!Tg7_device || (n > 0 && !points)) return fail(SLM_ERR_INVALID, "slm_rigid_transform: null argument");
  if (n < 0) return fail(SLM_ERR_INVALID, "slm_rigid_transform: n must be >= 0");
  if (n == 0) return SLM_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((n + 255) / 256), blk(256);
  if (f64)
    hipLaunchKernelGGL(k_rg_transform<double>, grid, blk, 0, st, n, (double*)points, (double*)norms, Tg7_device);
  else
    hipLaunchKernelGGL(k_rg_transform<float>, grid, blk, 0, st, n, (float*)points, (float*)norms, Tg7_device);
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

}  // extern "C"
