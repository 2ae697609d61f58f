// slm_gf_sample.h -- the samplers of the first-order path (GraphFit, slm_gf.hip) that the correspondence term of the LM
// path (slm_corr.hip) shares: the 4-tap gather of the target maps, the grid_sample-style read of the optical flow and the
// projection with its Jacobian rows.  Device code only.
#pragma once
#include "slm_common.h"

// 4-tap gather of the target maps at the float pixel (u_, v_) (bilinear_sample, loss.py:9-80, zero fill):
// false when a tap is unmapped.  o / n = interpolated point / normal, d*u / d*v their derivatives along u / v
// (autograd through clamp(1 - |tap - x|): d|x|/dx = sign(x) with sign(0) = 0).
struct GfSample {
  d3 o, n, dou, dov, dnu, dnv;
  int rows[4];
  double wv[4];
};

__device__ __forceinline__ bool gf_sample(const FrameIn& f, double u_, double v_, GfSample& q) {
  const double fv = floor(v_), cv = ceil(v_), fu = floor(u_), cu = ceil(u_);
  const double nn[4] = {fv, fv, cv, cv}, mm[4] = {fu, cu, fu, cu};
  bool all_ok = true;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    q.rows[t] = f.index_map[(int)nn[t] * f.W + (int)mm[t]];
    all_ok = all_ok && q.rows[t] >= 0;
  }
  if (!all_ok) return false;
  d3 o = {0, 0, 0}, n = {0, 0, 0}, dou = {0, 0, 0}, dov = {0, 0, 0}, dnu = {0, 0, 0}, dnv = {0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double dn = nn[t] - v_, dm = mm[t] - u_;
    const double an = fmax(1.0 - fabs(dn), 0.0), am = fmax(1.0 - fabs(dm), 0.0);
    const float* tp = f.tgt_points + 3 * (size_t)q.rows[t];
    const float* tn = f.tgt_norms + 3 * (size_t)q.rows[t];
    const d3 Pt = {(double)tp[0], (double)tp[1], (double)tp[2]};
    const d3 Nt = {(double)tn[0], (double)tn[1], (double)tn[2]};
    const double wv = an * am;
    const double sn = dn > 0.0 ? 1.0 : (dn < 0.0 ? -1.0 : 0.0);
    const double smm = dm > 0.0 ? 1.0 : (dm < 0.0 ? -1.0 : 0.0);
    const double gu = an * smm, gvv = am * sn;
    q.wv[t] = wv;
    o = {o.x + Pt.x * wv, o.y + Pt.y * wv, o.z + Pt.z * wv};
    n = {n.x + Nt.x * wv, n.y + Nt.y * wv, n.z + Nt.z * wv};
    dou = {dou.x + Pt.x * gu, dou.y + Pt.y * gu, dou.z + Pt.z * gu};
    dov = {dov.x + Pt.x * gvv, dov.y + Pt.y * gvv, dov.z + Pt.z * gvv};
    dnu = {dnu.x + Nt.x * gu, dnu.y + Nt.y * gu, dnu.z + Nt.z * gu};
    dnv = {dnv.x + Nt.x * gvv, dnv.y + Nt.y * gvv, dnv.z + Nt.z * gvv};
  }
  q.o = o; q.n = n; q.dou = dou; q.dov = dov; q.dnu = dnu; q.dnv = dnv;
  return true;
}

// The optical flow (2,H,W float32: x then y displacement) at the float pixel (u, v), sampled the way
// F.grid_sample(flow, grid) does at deform_mesh.py / loss.py:318-323: the grid is float32, bilinear, zero padding,
// align_corners=False, i.e. position ((g + 1) * size - 1) / 2 in float32; fl = (flow_x, flow_y) and
// D = [[dfx/du, dfx/dv], [dfy/du, dfy/dv]] (the grid gradient of the same cell, what autograd returns).
__device__ __forceinline__ void gf_flow_sample(const float* __restrict__ flow, int H, int W, double u, double v,
                                               double fl[2], double D[4]) {
  const float gx = (float)(u * 2.0 / (double)W - 1.0), gy = (float)(v * 2.0 / (double)H - 1.0);
  // The float32 arithmetic is spelt out with fmaf where torch's CPU kernel fuses -- the position (g + 1) * size / 2 - 1 / 2 and
  // every tap behind the first of the blend -- and nowhere else.  (It used to be written with __fmul_rn / __fadd_rn /
  // __fsub_rn, which are plain operators here: under -ffp-contract=fast the compiler fused the position, and the blend of
  // one channel but not of the other, so the sample agreed with neither an unfused nor a fused reading of the reference.
  // Restated in NumPy, the form below gives F.grid_sample's bits on every sample of the 60 x 80 test frames.)
  const float ix = fmaf(gx + 1.f, 0.5f * (float)W, -0.5f);
  const float iy = fmaf(gy + 1.f, 0.5f * (float)H, -0.5f);
  const float xw = floorf(ix), yn = floorf(iy);
  const float w = ix - xw, e = 1.f - w, n = iy - yn, sth = 1.f - n;
  const int x0 = (int)xw, y0 = (int)yn;
  const bool okx0 = x0 >= 0 && x0 < W, okx1 = x0 + 1 >= 0 && x0 + 1 < W;
  const bool oky0 = y0 >= 0 && y0 < H, oky1 = y0 + 1 >= 0 && y0 + 1 < H;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float* fc = flow + (size_t)c * H * W;
    const float nw = (okx0 && oky0) ? fc[(size_t)y0 * W + x0] : 0.f;
    const float ne = (okx1 && oky0) ? fc[(size_t)y0 * W + x0 + 1] : 0.f;
    const float sw = (okx0 && oky1) ? fc[(size_t)(y0 + 1) * W + x0] : 0.f;
    const float se = (okx1 && oky1) ? fc[(size_t)(y0 + 1) * W + x0 + 1] : 0.f;
    float acc = nw * (e * sth);
    acc = fmaf(ne, w * sth, acc);
    acc = fmaf(sw, e * n, acc);
    acc = fmaf(se, w * n, acc);
    fl[c] = (double)acc;
    D[2 * c + 0] = ((double)ne - (double)nw) * (double)sth + ((double)se - (double)sw) * (double)n;
    D[2 * c + 1] = ((double)sw - (double)nw) * (double)e + ((double)se - (double)ne) * (double)w;
  }
}

// the projection of P and the rows of its Jacobian: (u, v) = (fx X / Ze + cx, fy Y / Ze + cy), Ze = Z + 1e-8 -- the forward
// divides by Z + 1e-8, and so does its derivative
struct GfProj {
  double u, v;
  d3 Pi0, Pi1;   // du/dP, dv/dP
};
__device__ __forceinline__ GfProj gf_project(const FrameIn& f, const d3 P) {
  const double fx = (double)f.fx, fy = (double)f.fy, cx = (double)f.cx, cy = (double)f.cy;
  const double Ze = P.z + 1e-8;
  GfProj pr;
  pr.Pi0 = {fx / Ze, 0.0, -fx * P.x / (Ze * Ze)};
  pr.Pi1 = {0.0, fy / Ze, -fy * P.y / (Ze * Ze)};
  pr.u = P.x * fx / Ze + cx;
  pr.v = P.y * fy / Ze + cy;
  return pr;
}
