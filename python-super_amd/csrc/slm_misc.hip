// slm_misc.hip -- the LM loop's state kernels (slot initialisation, iteration begin, trial point, accept/reject on the
// device, target packing, loss read-out) and their launchers, nothing else.  (The node feeder is slm_nodes.hip.)
#include "slm_common.h"
#include "slm_face.h"
#include "slm_launch.h"

// ---------------------------------------------------------------------------------
// beta <- identity, state <- initial (reference super/LM.py:81-91)
__global__ void __launch_bounds__(256) k_init_slot(const FrameDev* __restrict__ frames, int slot,
                                                    double u0, double v, double minimal_loss0,
                                                    int num_iterations) {
  const FrameDev& fd = frames[slot];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < fd.f.J) {
    double* b = fd.beta + 7 * t;
    b[0] = 1.0;
#pragma unroll
    for (int c = 1; c < 7; ++c) b[c] = 0.0;
    const double ident[7] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    pack_node(fd.node_pk + (size_t)SLM_NPK * t, ident, ld_state3(frame_in(fd).ed_points, (size_t)t, fd.f.state_f64));
  }
  if (t < num_iterations) {
    slm_iter_record r;
    r.loss = 0.0;
    r.u = 0.0;
    r.accepted = 0;
    r.status = SLM_ITER_NOT_RUN;
    r.M_grad = 0;
    r.M_loss = 0;
    fd.rec[t] = r;
  }
  if (t == 0) {
    LMState s;
    s.u = u0;
    s.v = v;
    s.minimal_loss = minimal_loss0;
    s.iter = 0;
    s.stopped = 0;
    s.m_grad = 0;
    s.m_loss = 0;
    s.chol_fail = 0;
    s.m_grad_local = 0;
    s.eval_valid = 0;
    s.m_eval = 0;
    s.eval_acc = 0;
    *fd.st = s;
  }
}

// Start of an iteration: zero the band, rhs and counters.  grid = (blocks, n_frames)
__global__ void __launch_bounds__(256) k_iter_begin(const FrameDev* __restrict__ frames) {
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped) return;
  const size_t nband = (size_t)fd.nt * (fd.wb + 1) * SLM_NB * SLM_NB;
  const size_t nrhs = (size_t)fd.nt * SLM_NB;
  double2* b2 = reinterpret_cast<double2*>(fd.band.get());
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nband / 2;
       e += (size_t)gridDim.x * blockDim.x)
    b2[e] = make_double2(0.0, 0.0);
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nrhs;
       e += (size_t)gridDim.x * blockDim.x)
    fd.rhs[e] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    fd.st->m_grad = 0;
    fd.st->chol_fail = 0;
  }
}

// End of an iteration (reference super/LM.py:99-117): reduce the loss partials in a
// fixed order, then accept (u /= v, beta += delta) or reject (u *= v, beta kept).
// A failed factorisation stops the loop with beta unchanged.  grid = (1, n_frames), 1024 thr.
// Records are kept for the first n_rec iterations after the bind (the capacity of fd.rec): running again
// without binding continues the loop from the current state and records nothing more.
// eval_pass: the loss pass of this iteration was k_data_eval (it wrote the slot's evaluation buffer at the trial point);
// 0 when the batch took k_data_loss (one slot without a tuple-sorted plan sends all of them there): ev_rc then still
// holds an OLDER evaluation and must not be marked valid.
__global__ void __launch_bounds__(1024) k_accept(const FrameDev* __restrict__ frames, int phase_test,
                                                  int n_reg_part, int n_rec, int* __restrict__ reuse, int eval_pass) {
  __shared__ double sm[16];
  __shared__ int s_accept;
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound) return;
  LMState* st = fd.st;
  if (st->stopped) return;
  const int it = st->iter;
  if (st->chol_fail) {
    if (threadIdx.x == 0) {
      if (it < n_rec) {
        slm_iter_record r = fd.rec[it];
        r.status = st->chol_fail == 2 ? SLM_ITER_SOLVER_TIMEOUT : SLM_ITER_SOLVER_FAILED;
        r.u = st->u;
        r.M_grad = st->m_grad;
        fd.rec[it] = r;
      }
      st->stopped = 1;
    }
    return;
  }
  double ls = 0.0, cnt = 0.0;
  for (int b = threadIdx.x; b < fd.n_loss_part; b += blockDim.x) {
    ls += fd.loss_part[2 * b];
    cnt += fd.loss_part[2 * b + 1];
  }
  const double* reg = fd.loss_part + 2 * (size_t)fd.n_loss_part;
  for (int b = threadIdx.x; b < n_reg_part; b += blockDim.x) ls += reg[2 * b] + reg[2 * b + 1];
  const double loss = block_sum(ls, sm);
  const double m = block_sum(cnt, sm);
  if (threadIdx.x == 0) {
    int acc = 1;
    const double u_used = st->u;
    if (phase_test) {
      if (loss < st->minimal_loss) {
        st->minimal_loss = loss;
        st->u = u_used / st->v;
      } else {
        acc = 0;
        st->u = u_used * st->v;
      }
    }
    slm_iter_record r;
    r.loss = loss;
    r.u = u_used;
    r.accepted = acc;
    r.status = SLM_ITER_OK;
    r.M_grad = st->m_grad;
    r.M_loss = (int)m;
    if (it < n_rec) fd.rec[it] = r;
    st->iter = it + 1;
    s_accept = acc;
    if (reuse) reuse[blockIdx.y] = acc ? 0 : 1;   // rejected: the next Jacobian pass would repeat this one (k_data_gram)
    st->eval_valid = eval_pass ? acc : 0;         // the loss pass evaluated the TRIAL point: the current beta only if accepted
  }
  __syncthreads();
  if (s_accept) {
    for (int e = threadIdx.x; e < fd.P; e += blockDim.x) {
      const double b = fd.beta[e] + fd.delta[e];
      fd.beta[e] = b;
      fd.node_pk[(size_t)SLM_NPK * (e / 7) + e % 7] = b;
    }
  }
}

// node_pk <- beta (after slm_set_beta); grid = (ceil(J/256), 1)
__global__ void __launch_bounds__(256) k_pack_nodes(const FrameDev* __restrict__ frames, int slot) {
  const FrameDev& fd = frames[slot];
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= fd.f.J) return;
  double bb[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) bb[c] = fd.beta[7 * j + c];
  pack_node(fd.node_pk + (size_t)SLM_NPK * j, bb, ld_state3(frame_in(fd).ed_points, (size_t)j, fd.f.state_f64));
}

// node_pk_try <- beta + delta: the trial point of the loss pass; grid = (ceil(maxJ/256), n_frames)
__global__ void __launch_bounds__(256) k_make_trial(const FrameDev* __restrict__ frames) {
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound || fd.st->stopped) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= fd.f.J) return;
  double bb[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) bb[c] = fd.beta[7 * j + c] + fd.delta[7 * j + c];
  pack_node(fd.node_pk_try + (size_t)SLM_NPK * j, bb, ld_state3(frame_in(fd).ed_points, (size_t)j, fd.f.state_f64));
}

// target points + normals -> interleaved float4 pairs; grid = (ceil(T/256))
__global__ void __launch_bounds__(256) k_pack_target(int T, const float* __restrict__ pts,
                                                      const float* __restrict__ nrm,
                                                      float4* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  out[2 * (size_t)t] = make_float4(pts[3 * t], pts[3 * t + 1], pts[3 * t + 2], 0.f);
  out[2 * (size_t)t + 1] = make_float4(nrm[3 * t], nrm[3 * t + 1], nrm[3 * t + 2], 0.f);
}

// per-pixel form of the same (FrameDev::tgt_px); grid = (ceil(H*W/256))
__global__ void __launch_bounds__(256) k_pack_target_px(int HW, const int* __restrict__ index_map, const uint8_t* __restrict__ valid,
                                                         const float* __restrict__ pts, const float* __restrict__ nrm,
                                                         float4* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const int t = index_map[p];
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = make_float4(0.f, 0.f, 0.f, valid[p] ? 1.f : 0.f);
  if (t >= 0) {
    a = make_float4(pts[3 * (size_t)t], pts[3 * (size_t)t + 1], pts[3 * (size_t)t + 2], 1.f);
    b = make_float4(nrm[3 * (size_t)t], nrm[3 * (size_t)t + 1], nrm[3 * (size_t)t + 2], b.w);
  }
  out[2 * (size_t)p] = a;
  out[2 * (size_t)p + 1] = b;
}

// Reduce loss partials into out[0..3] = data, arap, rot, matched count (slm_loss).
__global__ void __launch_bounds__(256) k_loss_out(const FrameDev* __restrict__ frames, int slot,
                                                   int n_reg_part, double* __restrict__ out) {
  __shared__ double sm[16];
  const FrameDev& fd = frames[slot];
  double d = 0.0, c = 0.0, a = 0.0, r = 0.0;
  for (int b = threadIdx.x; b < fd.n_loss_part; b += blockDim.x) {
    d += fd.loss_part[2 * b];
    c += fd.loss_part[2 * b + 1];
  }
  const double* reg = fd.loss_part + 2 * (size_t)fd.n_loss_part;
  for (int b = threadIdx.x; b < n_reg_part; b += blockDim.x) {
    a += reg[2 * b];
    r += reg[2 * b + 1];
  }
  d = block_sum(d, sm);
  c = block_sum(c, sm);
  a = block_sum(a, sm);
  r = block_sum(r, sm);
  if (threadIdx.x == 0) {
    out[0] = d;
    out[1] = a;
    out[2] = r;
    out[3] = c;
  }
}

// out[0] = the loss of a term, out[1] = its count (slm_corr_loss, slm_face_loss): the nb pairs of slot `slot` at `part`
// behind the regularisers' partials (term_loss_store) summed in a fixed order; the count is the sum of the nb kept counts at
// cnt_part or, with `face`, the triangles of the slot's mesh (no mesh: both 0).  one wave
__global__ void __launch_bounds__(64) k_term_loss_out(const FrameDev* __restrict__ frames, int slot, int part, int nb, int cnt_part,
                                                       const FaceDev* __restrict__ face, double* __restrict__ out) {
  const FrameDev& fd = frames[slot];
  const double* reg = fd.loss_part + 2 * (size_t)fd.n_loss_part;
  double s = 0.0, c = 0.0;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    s += reg[part + 2 * b];
    if (!face) c += reg[cnt_part + b];
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if (threadIdx.x == 0) {
    if (face) {
      const bool on = face[slot].ready != 0;
      s = on ? s : 0.0;
      c = on ? (double)face[slot].n_tri : 0.0;
    }
    out[0] = s;
    out[1] = c;
  }
}

__global__ void k_zero_reg_part(const FrameDev* __restrict__ frames, int n_reg_part) {
  const FrameDev& fd = frames[blockIdx.y];
  if (!fd.bound) return;
  double* reg = fd.loss_part + 2 * (size_t)fd.n_loss_part;
  for (int b = threadIdx.x; b < 2 * n_reg_part; b += blockDim.x) reg[b] = 0.0;
}

// ---- host launchers --------------------------------------------------------------
void launch_init_slot(const FrameDev* frames_dev, int slot, int J, const slm_config& cfg,
                      hipStream_t st) {
  int n = J > cfg.num_iterations ? J : cfg.num_iterations;
  if (n < 1) n = 1;
  hipLaunchKernelGGL(k_init_slot, dim3((n + 255) / 256), dim3(256), 0, st, frames_dev, slot, cfg.u0,
                     cfg.v, cfg.minimal_loss0, cfg.num_iterations);
}

void launch_pack_nodes(const FrameDev* frames_dev, int slot, int J, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_nodes, dim3((J + 255) / 256), dim3(256), 0, st, frames_dev, slot);
}

void launch_make_trial(const FrameDev* frames_dev, int n_frames, int maxJ, hipStream_t st) {
  hipLaunchKernelGGL(k_make_trial, dim3((maxJ + 255) / 256, n_frames), dim3(256), 0, st, frames_dev);
}

void launch_pack_target(int T, const float* pts, const float* nrm, float4* out, hipStream_t st) {
  if (T > 0) hipLaunchKernelGGL(k_pack_target, dim3((T + 255) / 256), dim3(256), 0, st, T, pts, nrm, out);
}

void launch_pack_target_px(int HW, const int* index_map, const uint8_t* valid, const float* pts, const float* nrm, float4* out,
                           hipStream_t st) {
  if (HW > 0) hipLaunchKernelGGL(k_pack_target_px, dim3((HW + 255) / 256), dim3(256), 0, st, HW, index_map, valid, pts, nrm, out);
}

void launch_iter_begin(const FrameDev* frames_dev, int n_frames, hipStream_t st) {
  hipLaunchKernelGGL(k_iter_begin, dim3(1024, n_frames), dim3(256), 0, st, frames_dev);
}

void launch_accept(const FrameDev* frames_dev, int n_frames, int phase_test, int n_reg_part, int n_rec,
                   hipStream_t st, int* reuse, int eval_pass) {
  hipLaunchKernelGGL(k_accept, dim3(1, n_frames), dim3(1024), 0, st, frames_dev, phase_test,
                     n_reg_part, n_rec, reuse, eval_pass);
}

void launch_loss_out(const FrameDev* frames_dev, int slot, int n_reg_part, double* out,
                     hipStream_t st) {
  hipLaunchKernelGGL(k_loss_out, dim3(1), dim3(256), 0, st, frames_dev, slot, n_reg_part, out);
}

void launch_term_loss_out(const FrameDev* frames_dev, int slot, int part, int nb, int cnt_part, const FaceDev* face_dev, double* out,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_term_loss_out, dim3(1), dim3(64), 0, st, frames_dev, slot, part, nb, cnt_part, face_dev, out);
}

void launch_zero_reg_part(const FrameDev* frames_dev, int n_frames, int n_reg_part, hipStream_t st) {
  hipLaunchKernelGGL(k_zero_reg_part, dim3(1, n_frames), dim3(256), 0, st, frames_dev, n_reg_part);
}

