// slm_data_k4.hip -- tuple-sorted data-term Jacobian pass (JtJ / jtl of the point-to-plane
// term, reference super/loss.py:222-288 + 200-205), no per-entry atomics on the matrix:
//
//   k_data_eval     the TARGET-side half of the per-surfel work, one thread per tuple-sorted position: skin ->
//                   project -> match -> 8 bilinear taps -> residual r and c = dr/dT(p); {r, c} go to the evaluation
//                   buffer (32 B per position), sum r^2 / the matched count to the loss partials.  It IS the loss
//                   pass of the LM loop (trial point beta + delta); when the step is accepted its output is what the
//                   next Jacobian pass needs, so the projection and the taps are done once per iteration, not twice.
//   k_data_gram     one wave per 64 tuple-sorted surfel positions: every lane forms the 28 Jacobian entries of
//                   its surfel from {r, c} and its four nodes (no target access), writes the augmented row [J(28) | r | 0 0 0]
//                   (node slots in ascending-id order) to LDS, and the wave contracts
//                   groups of 4 surfels on the f64 MFMA:  G += row^T row  (32 x 32 as the
//                   three 16x16 tiles 00, 10, 11).  G[28][0..27] = J^T r and G[28][28] =
//                   sum r^2 ride along for free.  One G per (tuple, chunk) run goes to
//                   the slab with plain coalesced stores (no atomics at all).
//   k_band_assemble one wave per coupled node pair (a >= b): sums the 7x7 sub-blocks of
//                   the runs that contain both nodes (inverted index built once per frame
//                   by slm_prep.hip) and stores them into the lower band; the diagonal
//                   pair (a,a) also sums row 28 of its runs into jtl.  Every band / jtl
//                   entry is written by exactly one lane: bitwise reproducible.
#include <cstdlib>

#include "slm_data.h"
#include "slm_begin.h"
#include "slm_launch.h"

#define ROW_STRIDE 17   // doubles per surfel half-row in LDS (odd: conflict-free 64-bit writes)

// Evaluation pass over the tuple-sorted positions [256 wg_lo, min(n_pos, 256 wg_hi)) of every slot (the whole frame unless
// it is sharded over several GPUs).  grid = (n_blocks, n_frames), grid-stride; partial sums per block in a fixed order
// (bitwise reproducible).  mode 0: trial point (node_pk_try), always runs -- the loss pass; 1: current beta, only slots whose
// buffer is not valid (first iteration of a frame; after a reject when records are not reused); 2: current beta, always
// (parity entry points).  The LAST block of a slot (ticket) publishes the matched count of the pass (m_eval) and, for the
// passes at the current beta, marks the buffer valid; for the trial pass k_accept decides (valid iff accepted).
__global__ void __launch_bounds__(256) k_data_eval(const FrameDev* __restrict__ frames, double lam, int mode,
                                                    const int* __restrict__ reuse) {
  __shared__ double sm[16];
  __shared__ int s_skip;
  if (mode == 1 && reuse && reuse[blockIdx.y]) return;   // the Jacobian pass that would read the buffer is skipped too
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || !fd.v1_ready || fd.st->stopped) return;
  if (mode == 1) {
    // (uniform per slot for the whole launch: only the last block to FINISH changes the flag)
    if (threadIdx.x == 0) s_skip = __hip_atomic_load(&fd.st->eval_valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1;
    __syncthreads();
    if (s_skip) return;
  }
  const double* npk = mode == 0 ? fd.node_pk_try.get() : fd.node_pk.get();
  const int p0 = 256 * fd.wg_lo, p1 = min(fd.n_pos, 256 * fd.wg_hi);
  double acc = 0.0;
  int cnt = 0;
  for (int pos = p0 + blockIdx.x * blockDim.x + threadIdx.x; pos < p1; pos += gridDim.x * blockDim.x) {
    const int4 ids = *reinterpret_cast<const int4*>(fd.s_idx + 4 * (size_t)pos);
    double2 o0 = make_double2(0.0, 0.0), o1 = make_double2(0.0, 0.0);
    if (ids.x >= 0) {
      double wk[4];
      ld_state4(fd.s_w, (size_t)pos, fd.f.state_f64, wk);
      const d3 pp = ld_state3(fd.s_pts, (size_t)pos, fd.f.state_f64);
      SurfelEval ev;
      eval_surfel_core<2, true>(fd, pp, ids, wk, lam, npk, ev);   // (target taps from the per-pixel table)
      if (ev.match) {
        acc += ev.r * ev.r;
        ++cnt;
        o0 = make_double2(ev.r, ev.c[0]);
        o1 = make_double2(ev.c[1], ev.c[2]);
      }
    }
    double2* out = reinterpret_cast<double2*>(fd.ev_rc.get() + 4 * (size_t)pos);
    out[0] = o0;
    out[1] = o1;
  }
  const double s = block_sum(acc, sm);
  const double c = block_sum((double)cnt, sm);
  if (threadIdx.x == 0) {
    fd.loss_part[2 * blockIdx.x] = s;
    fd.loss_part[2 * blockIdx.x + 1] = c;
    LMState* st = fd.st;
    const unsigned long long old = __hip_atomic_fetch_add(&st->eval_acc, (1ull << 32) | (unsigned long long)(unsigned)(int)c,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)(old >> 32) == (int)gridDim.x - 1) {            // the last block of the slot to finish
      st->m_eval = (int)(unsigned)(old & 0xFFFFFFFFull) + (int)c;
      __hip_atomic_store(&st->eval_acc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (mode != 0) __hip_atomic_store(&st->eval_valid, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The position-indexed streams of one 256-position chunk as one lane holds them: what k_data_gram requests for chunk i + 1
// before the row / MFMA phase of chunk i.  Weights and point keep the dtype of the state (no conversion, so no wait, at
// the load).
struct GramChunk {
  int my_run;              // lane (l & 15): run of group (l & 15) of the wave's 64 positions, -1 padding / no positions
  int rec0, nrec;          // MERGE: the chunk's records [rec0, rec0 + nrec)
  int4 ids;
  double2 e0, e1;          // {r, c.x}, {c.y, c.z} of the position
  double2 wa, wb;          // weights, f64 state
  double px, py, pz;
  float4 wf;               // weights, f32 state
  float qx, qy, qz;
};
template <bool MERGE>
__device__ __forceinline__ void gram_chunk_load(const FrameDev& fd, int c, int w, int l, int f64, GramChunk& k) {
  k.my_run = -1;
  k.rec0 = k.nrec = 0;
  k.ids = int4{-1, -1, -1, -1};
  k.e0 = k.e1 = k.wa = k.wb = make_double2(0.0, 0.0);
  k.px = k.py = k.pz = 0.0;
  k.wf = make_float4(0.f, 0.f, 0.f, 0.f);
  k.qx = k.qy = k.qz = 0.f;
  if (MERGE) {
    k.rec0 = fd.wg_first[c];
    k.nrec = fd.wg_last[c] - k.rec0 + 1;
  }
  const int base = (c * 4 + w) * 64;
  if (base >= fd.n_pos) return;
  const size_t pos = (size_t)(base + l);
  k.my_run = fd.grp_run[(base >> 2) + (l & 15)];
  const double2* e2 = reinterpret_cast<const double2*>(fd.ev_rc.get() + 4 * pos);
  k.e0 = e2[0];
  k.e1 = e2[1];
  k.ids = *reinterpret_cast<const int4*>(fd.s_idx + 4 * pos);
  if (f64) {
    const double2* q = reinterpret_cast<const double2*>(static_cast<const double*>(fd.s_w.get()) + 4 * pos);
    k.wa = q[0];
    k.wb = q[1];
    const double* pq = static_cast<const double*>(fd.s_pts.get()) + 3 * pos;
    k.px = pq[0]; k.py = pq[1]; k.pz = pq[2];
  } else {
    k.wf = *reinterpret_cast<const float4*>(static_cast<const float*>(fd.s_w.get()) + 4 * pos);
    const float* pq = static_cast<const float*>(fd.s_pts.get()) + 3 * pos;
    k.qx = pq[0]; k.qy = pq[1]; k.qz = pq[2];
  }
}
// record numbers of the wave's runs: entry idx = group * 10 + pair slot, 160 per wave, three per lane
__device__ __forceinline__ void gram_lidx_load(const FrameDev& fd, int my_run, int l, uint8_t lv[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = l + 64 * k;
    const int g = idx / 10, e = idx - 10 * g;
    const int run = __shfl(my_run, g < 16 ? g : 0, 64);
    lv[k] = (idx < 160 && run >= 0) ? fd.run_lidx[10 * (size_t)run + e] : (uint8_t)0;
  }
}
// 16 KB piece pc of the slot's kind-0 pivot-column tiles (two per tile, as zero_fronts counts them), tile offset `off`
__device__ __forceinline__ void zero_front_piece(const FrameDev& fd, long long off, int pc) {
  const dvec2_t zz = {0.0, 0.0};
  dvec2_t* q = reinterpret_cast<dvec2_t*>(fd.ftiles.get() + off) + (size_t)(pc & 1) * 1024 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) __builtin_nontemporal_store(zz, q + 256 * k);
}

// grid = (workgroups per slot, n_frames), 256 threads = 4 waves.  RESIDENT: the launch is about one residency
// (2 workgroups per CU over the slots of the batch); workgroup b of the nwg of a slot walks a contiguous range of the slot's
// 256-position chunks [wg_lo, wg_hi), one 64-position sub-chunk per wave.  Chunk boundaries, records and slabs are what the
// plan defines -- the same per chunk as when every chunk had a workgroup of its own.  Software pipeline: chunk i + 1's
// position-indexed streams (GramChunk) are requested after chunk i's node gathers and land under its row / MFMA / merge
// phase; its record numbers (run_lidx, which need my_run) are requested after the Gram loop and land under the copy-out.
// dbg (diagnostic build only): bit0 skip slab stores, bit1 skip MFMA, bit2 skip surfel evaluation
// The 32-entry rows pass through LDS in two halves of 16 entries (8.7 KB per wave instead of
// 17 KB); the first half's MFMA operands wait in 16 registers per lane.
//
// MERGE (default): the workgroup's 4 waves add the 7x7 node-pair blocks of their runs (and the
// 7-entry J^T r pieces of the diagonal pairs) into LDS records keyed by node pair (ds_add_f64),
// and the workgroup writes one 56-double record per distinct pair -- about 4x fewer HBM bytes
// than one 768-double Gram per run, and the assemble kernels read contiguous records.  The LDS records are zero when a
// chunk starts: zeroed once per workgroup, and the thread that copies an entry out re-zeroes it.
// BEGIN (round 6): the launch also carries the iteration's zeroing (slm_begin.h) -- the Jacobian pass writes records, the
// zeroing writes fronts / vectors / flags, nothing in common.  Every workgroup does its 1 / nwg of the small parts at once
// and spreads its share of the fronts' 16 KB pieces over its chunks, stored right after the next chunk's loads are
// requested: the store stream (HBM-bound) drains under the Gram phase (LDS / MFMA-bound).  A workgroup without chunks
// (more workgroups than chunks, a reused or unbound slot) only zeroes.
template <bool MERGE, bool BEGIN = false>
__global__ void __launch_bounds__(256, 2) k_data_gram(const FrameDev* __restrict__ frames, double lam,
                                                       int dbg, const int* __restrict__ reuse, int dag_cut = -2) {
  __shared__ double rows[4][64 * ROW_STRIDE];
  __shared__ double recs[MERGE ? SLM_LB_MAX * SLM_WREC : 1];
  __shared__ uint8_t lidx[4][MERGE ? 160 : 4];   // per wave: record of each of the 10 node pairs of its 16 groups
  // After a REJECTED step beta is rolled back, so this pass would reproduce the records of the previous iteration
  // entry for entry (reference super/LM.py:114-117 then :96 rebuilds an identical JtJ): the slot keeps them and
  // k_front_assemble re-reads them.
  const bool reused = reuse && reuse[blockIdx.y];
  if (!BEGIN && reused) return;
  const FrameDev& fd = frames[blockIdx.y];
  const int b = blockIdx.x, nwg = gridDim.x;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int lc = l & 15, lq = l >> 4;
  const int f64 = fd.f.state_f64;
  // (no test of st->stopped for the Gram pass: a stopped slot only wastes it)
  // the slot's chunks of this workgroup: [c0, c1) of the shard window (another rank's share is not touched)
  int c0 = 0, c1 = 0;
  if (!reused && fd.bound && fd.v1_ready && MERGE == (fd.v2_ready != 0) && fd.n_pos > 0) {   // the host launches both variants when slots differ
    // the matched count of this pass is the one of the evaluation it consumes (this rank's share of it when sharded)
    if (b == 0 && threadIdx.x == 0) fd.st->m_grad = fd.st->m_eval;
    const int lo = max(fd.wg_lo, 0), hi = min(fd.wg_hi, (fd.n_pos + 255) >> 8);
    if (hi > lo) {
      c0 = lo + (int)((long long)(hi - lo) * b / nwg);
      c1 = lo + (int)((long long)(hi - lo) * (b + 1) / nwg);
    }
  }
  GramChunk cur{}, nxt{};
  if (c0 < c1) gram_chunk_load<MERGE>(fd, c0, w, l, f64, cur);
  // the zeroing: pieces pc = b + k nwg, k in [0, znv), of the slot's 2 n_zero_tiles; at most zper (and 64) per chunk
  int zk = 0, znv = 0, zper = 0;
  if (BEGIN) {
    iter_begin_nd_small(fd, b, nwg, reused, dag_cut, fd.v1_ready && fd.v2_ready);
    if (fd.bound && fd.nd_ready && !fd.st->stopped) {
      const int np = 2 * fd.n_zero_tiles;
      znv = b < np ? (np - b + nwg - 1) / nwg : 0;
      zper = c1 > c0 ? min(64, (znv + (c1 - c0) - 1) / (c1 - c0)) : 0;
    }
  }
  if (MERGE && c0 < c1)
    for (int i = threadIdx.x; i < SLM_LB_MAX * SLM_WREC; i += 256) recs[i] = 0.0;
  double* myrow = &rows[w][l * ROW_STRIDE];
  uint8_t lv[3] = {0, 0, 0};
  if (MERGE && c0 < c1) gram_lidx_load(fd, cur.my_run, l, lv);

  for (int c = c0; c < c1; ++c) {
    const bool wact = (c * 4 + w) * 64 < fd.n_pos;
    // tile offsets of the pieces zeroed under this chunk, lane k the k-th: requested with the node gathers
    int znow = 0;
    long long zoff = 0;
    if (BEGIN) {
      znow = min(zper, znv - zk);
      if (l < znow) zoff = fd.zero_tiles[(b + (zk + l) * nwg) >> 1];
    }
    // ---- the surfel's row from the evaluation buffer: no projection, no target access --------------
    SurfelEval ev;
    ev.match = false;
    ev.r = 0.0;
    ev.id[0] = ev.id[1] = ev.id[2] = ev.id[3] = -1;
    const bool live = wact && cur.ids.x >= 0;
#ifdef SLM_STAMPS
    if (live && !(dbg & 4))
#else
    if (live)
#endif
    {
      ev.id[0] = cur.ids.x; ev.id[1] = cur.ids.y; ev.id[2] = cur.ids.z; ev.id[3] = cur.ids.w;
      // (an unmatched surfel has {r, c} = 0: its row is zero and it adds nothing to the Gram)
      ev.match = cur.e0.x != 0.0 || cur.e0.y != 0.0 || cur.e1.x != 0.0 || cur.e1.y != 0.0;
      ev.r = cur.e0.x;
      if (ev.match) {
        double wk[4];
        d3 pp;
        if (f64) {
          wk[0] = cur.wa.x; wk[1] = cur.wa.y; wk[2] = cur.wb.x; wk[3] = cur.wb.y;
          pp = {cur.px, cur.py, cur.pz};
        } else {
          wk[0] = (double)cur.wf.x; wk[1] = (double)cur.wf.y; wk[2] = (double)cur.wf.z; wk[3] = (double)cur.wf.w;
          pp = {(double)cur.qx, (double)cur.qy, (double)cur.qz};
        }
        rows_from_c(pp, ev.id, wk, lam, fd.node_pk, {cur.e0.y, cur.e1.x, cur.e1.y}, ev.row);
      }
    }
    const int my_run = cur.my_run, rec0 = cur.rec0, nrec = cur.nrec;
    // ---- the next chunk's streams, then this chunk's share of the zeroing: both in flight under the Gram phase ----
    if (c + 1 < c1) gram_chunk_load<MERGE>(fd, c + 1, w, l, f64, nxt);
    if (BEGIN) {
      for (int k = 0; k < znow; ++k) zero_front_piece(fd, __shfl(zoff, k, 64), b + (zk + k) * nwg);
      zk += znow;
    }
    if (MERGE && wact) {
      lidx[w][l] = lv[0];
      lidx[w][l + 64] = lv[1];
      if (l + 128 < 160) lidx[w][l + 128] = lv[2];
    }
    if (MERGE) __syncthreads();   // the records are zero again (copy-out of the chunk before), record numbers in place
    if (wact) {

  // canonical slot of neighbour k = number of neighbour ids smaller than id[k]
  int slot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    slot[k] = 0;
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) slot[k] += (ev.id[k2] < ev.id[k]) ? 1 : 0;
  }
  double a0[16];   // first-half operands of the 16 groups: rows[4g + lq][lc]
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int e = 0; e < 16; ++e) myrow[e] = 0.0;
    if (ev.match) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int cc = 0; cc < 7; ++cc) {
          const int e = 7 * slot[k] + cc - 16 * half;
          if (e >= 0 && e < 16) myrow[e] = ev.row[7 * k + cc];
        }
      if (half == 1) myrow[28 - 16] = ev.r;
    }
    // the operands below are read by other lanes of the same wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (half == 0) {
#pragma unroll
      for (int g = 0; g < 16; ++g) a0[g] = rows[w][(4 * g + lq) * ROW_STRIDE + lc];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }

  // ---- Gram accumulation per run ---------------------------------------------------
  double4_t g00 = {0, 0, 0, 0}, g10 = {0, 0, 0, 0}, g11 = {0, 0, 0, 0};
  int crun = -1;

  auto flush = [&](int run, int grp) {
#ifdef SLM_STAMPS
    if (dbg & 1) return;
#endif
    if (MERGE) {
      // accumulator element (tile, r) of lane l is G[i][j], i = 4r + lq (+16), j = lc (+16)
      const uint8_t* lvp = &lidx[w][10 * grp];   // record of each of the 10 node pairs of this run
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * r + lq + (t >= 1 ? 16 : 0), j = lc + (t == 2 ? 16 : 0);
          const double v = t == 0 ? g00[r] : (t == 1 ? g10[r] : g11[r]);
          const int pa = (i * 37) >> 8, pb = (j * 37) >> 8;   // i / 7 for i < 32
          const int ca = i - 7 * pa, cb = j - 7 * pb;
          const bool jrow = (i == 28);
          const bool act = j < 28 && (jrow || (i < 28 && i >= j));
          // row 28 (J^T r) goes to the diagonal record of node slot pb, entries 49..55
          int ps = jrow ? (pb * (pb + 1) / 2 + pb) : (pa * (pa + 1) / 2 + pb);
          ps = act ? ps : 0;
          const int rec = lvp[ps];
          if (act) unsafeAtomicAdd(&recs[rec * SLM_WREC + (jrow ? 49 + cb : 7 * ca + cb)], v);
        }
    } else {
      double* out = fd.slab + (size_t)run * SLM_SLAB_STRIDE;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        out[r * 64 + l] = g00[r];
        out[256 + r * 64 + l] = g10[r];
        out[512 + r * 64 + l] = g11[r];
      }
      // row 28 of G (= J^T r, sum r^2) travels in the slab; k_*_assemble turns it into jtl
    }
  };

#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int run = __builtin_amdgcn_readlane(my_run, g);
    if (run != crun) {
      if (crun >= 0) flush(crun, g - 1);
      g00 = double4_t{0, 0, 0, 0};
      g10 = double4_t{0, 0, 0, 0};
      g11 = double4_t{0, 0, 0, 0};
      crun = run;
    }
    if (run < 0) continue;
    const double a1 = rows[w][(4 * g + lq) * ROW_STRIDE + lc];
#ifdef SLM_STAMPS
    if (dbg & 2) { g00[0] += a0[g]; g11[0] += a1; continue; }
#endif
    g00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[g], a0[g], g00, 0, 0, 0);
    g10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a0[g], g10, 0, 0, 0);
    g11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, g11, 0, 0, 0);
  }
  if (crun >= 0) flush(crun, 15);
    }   // wave has positions
    if (MERGE) {
      // the next chunk's record numbers (its my_run has had the Gram phase to arrive): in flight under the copy-out
      if (c + 1 < c1) gram_lidx_load(fd, nxt.my_run, l, lv);
      __syncthreads();
      // copy-out: the thread that stores an entry re-zeroes it, so the next chunk needs no zero pass and no second barrier
      double* out = fd.wgslab + (size_t)rec0 * SLM_WREC;
      for (int i = threadIdx.x; i < nrec * SLM_WREC; i += 256) {
        out[i] = recs[i];
        recs[i] = 0.0;
      }
    }
    cur = nxt;
  }
  if (BEGIN)   // what the chunks did not cover (no chunk at all, or more than 64 pieces per chunk)
    while (zk < znv) {
      const int znow = min(64, znv - zk);
      const long long zoff = l < znow ? fd.zero_tiles[(b + (zk + l) * nwg) >> 1] : 0;
      for (int k = 0; k < znow; ++k) zero_front_piece(fd, __shfl(zoff, k, 64), b + (zk + k) * nwg);
      zk += znow;
    }
}

// G[i][j], i >= j, from a slab entry (tiles 00, 10, 11; 16x16 row-major each)
__device__ __forceinline__ double gram_at(const double* g, int i, int j) {
  if (i < 16) return g[16 * i + j];
  if (j < 16) return g[256 + 16 * (i - 16) + j];
  return g[512 + 16 * (i - 16) + (j - 16)];
}

// grid = (ceil(max n_blocks / 4), n_frames), 256 threads: one wave per node pair
__global__ void __launch_bounds__(256) k_band_assemble(const FrameDev* __restrict__ frames) {
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || !fd.v1_ready || fd.st->stopped) return;
  const int bi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bi >= fd.n_blocks) return;
  const int l = threadIdx.x & 63;
  const unsigned key = (unsigned)fd.blk_key[bi];
  const int a = (int)(key / (unsigned)fd.f.J), b = (int)(key % (unsigned)fd.f.J);
  const int ca = l / 7, cb = l % 7;
  const bool act = (l < 49) && (a != b || ca >= cb);   // lower triangle only on diagonal blocks
  const bool jt = (a == b) && l >= 49 && l < 56;       // diagonal block: lanes 49..55 build jtl of node a
  double acc = 0.0;
  if (fd.v2_ready) {
    const int s0 = fd.blk2_start[bi], s1 = fd.blk2_start[bi + 1];
    if (l < SLM_WREC)
      for (int s = s0; s < s1; ++s) acc += fd.wgslab[(size_t)fd.blk2_entry[s] * SLM_WREC + l];
  } else {
    const int s0 = fd.blk_start[bi], s1 = fd.blk_start[bi + 1];
    for (int s = s0; s < s1; ++s) {
      const int pl = fd.blk_entry[s];
      const int run = pl >> 4, pa = (pl >> 2) & 3, pb = pl & 3;
      const double* G = fd.slab + (size_t)run * SLM_SLAB_STRIDE;
      if (act) acc += gram_at(G, 7 * pa + ca, 7 * pb + cb);
      else if (jt) acc += gram_at(G, 28, 7 * pa + (l - 49));     // (J^T r) of node a in this run
    }
  }
  if (act) *band_entry(fd, 7 * a + ca, 7 * b + cb) = acc;
  else if (jt) fd.rhs[7 * a + (l - 49)] = -acc;               // jtl = -J^T r, one writer per entry
}

// Workgroups per slot of the resident Jacobian pass: `wgs` when the solver's knob sets it (SLM_GRAM_WGS), else one
// residency -- 2 workgroups per CU -- shared by the slots of the batch.
static int gram_wgs(int wgs, int n_frames, int n_cus) { return wgs > 0 ? wgs : max(1, 2 * n_cus / max(1, n_frames)); }

// variants: bit0 = some slot uses the workgroup-merged records, bit1 = some slot uses the per-run slab
// The Jacobian pass AND the iteration's zeroing in one launch (every slot of the batch on the workgroup-merged records):
// what slm_run's loop enqueues instead of k_iter_begin_nd + k_data_gram.
void launch_begin_and_gram(const FrameDev* frames_dev, int n_frames, double lam, hipStream_t st, const int* reuse,
                           int dag_cut, int wgs, int n_cus) {
  int dbg = 0;
#ifdef SLM_STAMPS
  if (const char* e = getenv("SLM_DBG")) dbg = atoi(e);
#endif
  hipLaunchKernelGGL((k_data_gram<true, true>), dim3(gram_wgs(wgs, n_frames, n_cus), n_frames), dim3(256), 0, st, frames_dev, lam, dbg,
                     reuse, dag_cut);
}

void launch_data_gram(const FrameDev* frames_dev, int n_frames, int max_pos, double lam, int variants,
                      hipStream_t st, const int* reuse, int wgs, int n_cus) {
  if (max_pos <= 0) return;
  int dbg = 0;
#ifdef SLM_STAMPS
  if (const char* e = getenv("SLM_DBG")) dbg = atoi(e);
#endif
  // (no zeroing to share: a workgroup beyond the chunks of the largest slot would have nothing to do)
  const dim3 grid(wgs > 0 ? wgs : min(gram_wgs(0, n_frames, n_cus), (max_pos + 255) / 256), n_frames);
  if (variants & 1) hipLaunchKernelGGL(k_data_gram<true>, grid, dim3(256), 0, st, frames_dev, lam, dbg, reuse, -2);
  if (variants & 2) hipLaunchKernelGGL(k_data_gram<false>, grid, dim3(256), 0, st, frames_dev, lam, dbg, reuse, -2);
}

void launch_data_eval(const FrameDev* frames_dev, int n_frames, int n_blocks, double lam, int mode, hipStream_t st,
                      const int* reuse) {
  hipLaunchKernelGGL(k_data_eval, dim3(n_blocks, n_frames), dim3(256), 0, st, frames_dev, lam, mode, reuse);
}

void launch_band_assemble(const FrameDev* frames_dev, int n_frames, int max_blocks, hipStream_t st) {
  if (max_blocks <= 0) return;
  hipLaunchKernelGGL(k_band_assemble, dim3((max_blocks + 3) / 4, n_frames), dim3(256), 0, st, frames_dev);
}
