// slm_pairs.h -- the pair-record Gram of a wave (device): what k_data_grad_pairs (slm_data.hip) and k_corr_grad_pairs
// (slm_corr.hip) share behind the evaluation of their rows -- the LDS of the wave, the small steps of filling it, and the
// run Gram itself (pair_gram).  A further term on the pair records fills its rows and calls the same.
#pragma once
#include "slm_common.h"

// ---- K-generic terms on the multifrontal path (num_neighbors != 4) -----------------------------------------------------
// The Jacobian row of a surfel has 7K entries; its outer product lands in the K(K+1)/2 node-pair blocks of the surfel.
// One thread per surfel evaluates (as k_data_grad), then the WAVE forms the Gram matrices of its surfels on the f64 MFMA:
// the rows of its 64 surfels go to LDS in the surfel's canonical neighbour order (ids ascending: slot (ra, rb <= ra) is
// the pair (c[ra], c[rb]), never transposed) with the residual as one more column -- A = [row | r], so that A^T A carries
// J^T r in its last row -- padded to NT 16-column tiles; surfels that are not "on" (unmatched, no correspondence) are zero
// rows.  Surfels are walked in neighbour-set order (FrameDev::sf_perm), so the surfels of a set are consecutive: per RUN of
// surfels with one set the lower tile pairs of A^T A are accumulated over the run's 4-row k-steps
// (v_mfma_f64_16x16x4_f64; a k-step that straddles a run boundary has the other run's rows masked out of one operand), and
// every accumulator entry that belongs to a block -- (slot, ca, cb) with the larger-id node's row index first, or (node, c)
// of J^T r -- is added to the run's pair records with one f64 atomic.  (Round 6, first form: lane = entry,
// 7K(7K + 1) / 2 + 7K scalar multiply-adds per surfel from LDS -- 0.45 ms per C2 frame at K = 6, bound by that loop, not by
// the atomics; a workgroup-level LDS table of pair records on top of it cut the atomics 4 x and was SLOWER: 0.61 ms,
// tools/studies/r06_patches/pair_table_lds.patch.)
// A term has NC rows per surfel (the data term and the point-plane correspondences one, the point-point correspondences
// their three components): k-row NC * position + component, so a run of positions [rs, re) is the run of k-rows
// [NC rs, NC re) and the further rows of a surfel are simply further k-rows of the same Gram.
// The records (pairbuf: 49 block entries row-major (ca, cb) + 7 entries of J^T r of the diagonal pair, as the wgslab
// records of the tuple-sorted path) are placed into the fronts by k_pair_scatter (slm_front.hip).  The plan (blk_key,
// sf_pidx, sf_perm) is built from all surfels, so every block a term needs has a record.
// ONE wave per workgroup; the kernel declares the struct __shared__.
template <int KK, int NC>
struct PairLds {
  static constexpr int NP = KK * (KK + 1) / 2, NR = 7 * KK, NT = (NR + 1 + 15) / 16, NTP = NT * (NT + 1) / 2;
  static constexpr int LDR = 16 * NT + 1;   // odd row stride
  // (s_g in front: with s_row first the register allocation of the weighted data kernel moves -- two VGPRs of
  //  k_data_grad_pairs<7, DataWArgs> go to AGPRs; this order compiles to the figures of the separate arrays it replaces,
  //  tests/test_pair_term_resources.py)
  double s_g[16 * NT * LDR];     // the Gram of one run on its way from the accumulators to record order
  double s_row[NC * 64 * LDR];   // k-row NC l + comp of lane l: [row in canonical order | r | zeros]
  int s_pi[64 * NP];             // the pair records of lane l's surfel (sf_pidx)
  int s_cid[64 * KK];            // its node ids, ascending
};

// The skinning state of surfel i at the node table npk (node_pk or node_pk_try): its neighbours, their rotations, p - g_k
// and the skinned position T(p).  What the terms whose rows are c^T dT/dbeta (the correspondence term, the semantic
// boundary-morph term) evaluate before they choose their c.
template <int KK>
struct PairSkin {
  int id[KK];
  double w[KK], qw[KK];
  d3 qv[KK], dk[KK];
  d3 T;
};
template <int KK>
__device__ __forceinline__ void pair_skin(const FrameDev& fd, const double* __restrict__ npk, int i, PairSkin<KK>& s) {
  const FrameIn& f = frame_in(fd);
  const d3 p = ld_state3(f.sf_points, (size_t)i, fd.f.state_f64);
  d3 T = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    s.id[k] = f.sf_knn_idx[(size_t)KK * i + k];
    s.w[k] = ld_state1(f.sf_knn_w, (size_t)KK * i + k, fd.f.state_f64);
    const double2* nq = reinterpret_cast<const double2*>(npk + (size_t)SLM_NPK * s.id[k]);
    const double2 n0 = nq[0], n1 = nq[1], n2 = nq[2], n3 = nq[3], n4 = nq[4];
    const d3 g = {n3.y, n4.x, n4.y};
    s.qw[k] = n0.x;
    s.qv[k] = {n0.y, n1.x, n1.y};
    s.dk[k] = p - g;
    d3 t = quat_apply(s.qw[k], s.qv[k], s.dk[k]);
    t = {t.x + n2.x + g.x, t.y + n2.y + g.y, t.z + n3.x + g.z};
    T = {T.x + s.w[k] * t.x, T.y + s.w[k] * t.y, T.z + s.w[k] * t.z};
  }
  s.T = T;
}

// canonical slot of neighbour k of a surfel (the ids are distinct: slm_bind_frame refuses a row that repeats one)
template <int KK>
__device__ __forceinline__ int pair_rank(const int (&id)[KK], int k) {
  int rank = 0;
#pragma unroll
  for (int j = 0; j < KK; ++j) rank += (id[j] < id[k]) ? 1 : 0;
  return rank;
}

// lane l's NC padded rows <- 0
template <int KK, int NC>
__device__ __forceinline__ void pair_zero_rows(PairLds<KK, NC>& s, int l) {
#pragma unroll
  for (int comp = 0; comp < NC; ++comp) {
    double* rw = s.s_row + (NC * l + comp) * PairLds<KK, NC>::LDR;
#pragma unroll
    for (int c = 0; c < 16 * PairLds<KK, NC>::NT; ++c) rw[c] = 0.0;
  }
}

// lane l's pair records <- those of surfel i
template <int KK, int NC>
__device__ __forceinline__ void pair_load_pidx(PairLds<KK, NC>& s, const FrameDev& fd, int l, int i) {
  constexpr int NP = PairLds<KK, NC>::NP;
#pragma unroll
  for (int sl = 0; sl < NP; ++sl) s.s_pi[l * NP + sl] = fd.sf_pidx[(size_t)NP * i + sl];
}

// The Grams of the wave's runs into the pair records pb.  on: lane l's rows, ids and records are filled (the rows of the
// other lanes are zero); m = __ballot(on), not 0.  Starts with the barrier behind the fill.
template <int KK, int NC>
__device__ __forceinline__ void pair_gram(PairLds<KK, NC>& s, double* pb, bool on, unsigned long long m) {
  typedef double double4_t __attribute__((ext_vector_type(4)));
  typedef PairLds<KK, NC> L;
  constexpr int NP = L::NP, NR = L::NR, NT = L::NT, NTP = L::NTP, LDR = L::LDR;
  const int l = threadIdx.x, lr = l & 15, lk = l >> 4;
  __syncthreads();
  // runs: an "on" surfel starts one when its neighbour set differs from the previous such surfel's
  bool start = false;
  if (on) {
    const unsigned long long below = m & ((1ull << l) - 1ull);
    if (!below) start = true;
    else {
      const int pl = 63 - __builtin_clzll(below);
#pragma unroll
      for (int k = 0; k < KK; ++k) start = start || (s.s_cid[l * KK + k] != s.s_cid[pl * KK + k]);
    }
  }
  unsigned long long starts = __ballot(start);
  // A run's Gram matrix goes from the accumulators (tile pair tp = (ti, tj <= ti), register r <-> entry (16 ti + lr,
  // 16 tj + lk + 4 r)) through LDS to RECORD order: lane e < 56 owns entry e of every pair record, so one atomic
  // instruction of the wave touches the four cache lines of ONE record instead of a dozen records' (the L2 executes
  // atomics line by line).
  const int eca = l / 7, ecb = l - 7 * eca;   // lane -> (ca, cb) of a block entry (l < 49), or component l - 49 of J^T r
  while (starts) {
    const int rs = __builtin_ctzll(starts);   // uniform
    starts &= starts - 1;
    const int re = starts ? __builtin_ctzll(starts) : 64;
    const int qs = NC * rs, qe = NC * re;     // the run's k-rows
    double4_t acc[NTP];
#pragma unroll
    for (int tp = 0; tp < NTP; ++tp) acc[tp] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int ks = qs >> 2; ks <= (qe - 1) >> 2; ++ks) {
      const int q = 4 * ks + lk;
      const bool inrun = q >= qs && q < qe;
      double v[NT], vm[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        v[t] = s.s_row[q * LDR + 16 * t + lr];
        vm[t] = inrun ? v[t] : 0.0;
      }
      int tp = 0;
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj, ++tp) acc[tp] = __builtin_amdgcn_mfma_f64_16x16x4f64(vm[tj], v[ti], acc[tp], 0, 0, 0);
    }
    {
      int tp = 0;
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj, ++tp)
#pragma unroll
          for (int r = 0; r < 4; ++r) s.s_g[(16 * ti + lr) * LDR + 16 * tj + lk + 4 * r] = acc[tp][r];
    }
    __syncthreads();
    const int* pi = s.s_pi + rs * NP;
    int sl = 0;
#pragma unroll 1
    for (int ra = 0; ra < KK; ++ra)
#pragma unroll 1
      for (int rb = 0; rb <= ra; ++rb, ++sl) {
        double val = 0.0;
        bool put = false;
        if (l < 49) {
          put = ra > rb || eca >= ecb;   // (a diagonal pair's block is symmetric: its lower part is what is placed)
          val = s.s_g[(7 * ra + eca) * LDR + 7 * rb + ecb];
        } else if (l < 56 && ra == rb) {
          put = true;
          val = s.s_g[NR * LDR + 7 * rb + (l - 49)];
        }
        if (put) atomic_add_f64(pb + (size_t)pi[sl] * SLM_WREC + l, val);
      }
    __syncthreads();   // s_g is rewritten by the next run
  }
}
