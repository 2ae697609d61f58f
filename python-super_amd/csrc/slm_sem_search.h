// slm_sem_search.h -- what the two forms of the semantic-boundary morphing term share (k_gf_morph, slm_sem.hip: GraphFit's
// first-order form; k_morph_select, slm_morph.hip: the LM path's Gauss-Newton form): the class a projected surfel lands on,
// the search for the two nearest boundary pixels of its own class by the waves of a workgroup, and the keep test.
// Device code only.
#pragma once
#include "slm_common.h"

// argmax_c F.grid_sample(img_seg_conf, grid)(x, y) with bilinear taps, zero padding, align_corners=False, the first maximum
// winning; gx, gy = the normalised coordinates.
__device__ __forceinline__ int sem_sample_class(const float* __restrict__ img_seg_conf, int C, int H, int W, double x, double y,
                                                double& gx, double& gy) {
  gx = x / (double)W * 2.0 - 1.0;
  gy = y / (double)H * 2.0 - 1.0;
  const double ix = ((gx + 1.0) * (double)W - 1.0) / 2.0, iy = ((gy + 1.0) * (double)H - 1.0) / 2.0;
  const double x0 = floor(ix), y0 = floor(iy);
  const double wnw = (x0 + 1.0 - ix) * (y0 + 1.0 - iy), wne = (ix - x0) * (y0 + 1.0 - iy);
  const double wsw = (x0 + 1.0 - ix) * (iy - y0), wse = (ix - x0) * (iy - y0);
  const bool inx0 = x0 >= 0.0 && x0 <= (double)(W - 1), inx1 = x0 + 1.0 >= 0.0 && x0 + 1.0 <= (double)(W - 1);
  const bool iny0 = y0 >= 0.0 && y0 <= (double)(H - 1), iny1 = y0 + 1.0 >= 0.0 && y0 + 1.0 <= (double)(H - 1);
  int best = 0;
  double bestv = 0.0;
  if (gx > -4.0 && gx < 4.0 && gy > -4.0 && gy < 4.0) {   // far outside: all taps are padding
    const int xi = (int)x0, yi = (int)y0;
    for (int c = 0; c < C; ++c) {
      const float* img = img_seg_conf + (size_t)c * H * W;
      double v = 0.0;
      if (inx0 && iny0) v += (double)img[yi * W + xi] * wnw;
      if (inx1 && iny0) v += (double)img[yi * W + xi + 1] * wne;
      if (inx0 && iny1) v += (double)img[(yi + 1) * W + xi] * wsw;
      if (inx1 && iny1) v += (double)img[(yi + 1) * W + xi + 1] * wse;
      if (c == 0 || v > bestv) {
        bestv = v;
        best = c;
      }
    }
  }
  return best;
}

// The candidates of a 256-thread workgroup (surfels whose projected class differs from their own), compacted into LDS by
// the kernel: position, the range of the class's boundary list, and the answer of the search.
struct SemCandLds {
  int n_cand;
  double x[256], y[256], d1[256], d2[256];
  int e0[256], e1[256], i1[256], i2[256];
};

// The two nearest boundary pixels of every candidate's class: the mismatching surfels are a thin band along the class
// boundaries (a few per cent), so one lane per surfel scanning ~1 000-2 000 boundary pixels left 60 lanes of its wave idle for
// the whole scan (534 us per launch at C4, 80 % of the Semantic-SuPer step).  The workgroup's WAVES take its candidates one
// after the other (wave w the candidates w, w + 4, ...): 64 lanes scan the class's list strided, each keeps its two nearest
// in (distance, list position) order -- the order of the sequential scan with strict <, i.e. find_knn's lowest index on
// ties -- and a butterfly merge gives the candidate's answer to lane 0.  (First form of round 6: the whole workgroup per
// candidate, 256 lanes + a four-way merge through LDS behind two barriers per candidate -- the butterfly and the barriers
// were issued by four waves for one candidate: 68 us per launch at C4.)
// Called by all 256 threads between two barriers of the kernel's own.
__device__ __forceinline__ void sem_search_candidates(SemCandLds& c, const float2* __restrict__ edge_xy) {
  const int nc = c.n_cand;
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = w; k < nc; k += 4) {
    const double x = c.x[k], y = c.y[k];
    const int e0 = c.e0[k], e1 = c.e1[k];
    double d1 = 1e300, d2 = 1e300;
    int i1 = 0x7fffffff, i2 = 0x7fffffff;
    for (int e = e0 + l; e < e1; e += 64) {
      const float2 q = edge_xy[e];
      const double dx = x - (double)q.x, dy = y - (double)q.y;
      const double d = dx * dx + dy * dy;
      if (d < d1) {
        d2 = d1; i2 = i1;
        d1 = d; i1 = e;
      } else if (d < d2) {
        d2 = d; i2 = e;
      }
    }
    // merge of two sorted pairs under (distance, index) order
    auto before = [](double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); };
    auto merge = [&](double od1, int oi1, double od2, int oi2) {
      // the two smallest of {(d1,i1) <= (d2,i2)} and {(od1,oi1) <= (od2,oi2)}
      if (before(od1, oi1, d1, i1)) {
        // other's first leads: second is min(mine first, other's second)
        if (before(od2, oi2, d1, i1)) { d2 = od2; i2 = oi2; }
        else { d2 = d1; i2 = i1; }
        d1 = od1; i1 = oi1;
      } else if (before(od1, oi1, d2, i2)) {
        d2 = od1; i2 = oi1;
      }
    };
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double od1 = __shfl_xor(d1, off, 64), od2 = __shfl_xor(d2, off, 64);
      const int oi1 = __shfl_xor(i1, off, 64), oi2 = __shfl_xor(i2, off, 64);
      merge(od1, oi1, od2, oi2);
    }
    if (l == 0) {
      c.d1[k] = d1; c.d2[k] = d2;
      c.i1[k] = i1; c.i2[k] = i2;
    }
  }
}

// A candidate at (x, y) with squared distances d1 <= d2 to its two nearest boundary pixels is kept when it is not closer to
// the image border than to the class boundary and its mean squared distance li exceeds 15.
__device__ __forceinline__ bool sem_morph_keep(double x, double y, int W, int H, double d1, double d2, double& li) {
  const double dte = fmin(fmin(fmin(x, y), (double)W - x), (double)H - y);
  const bool ok = !(sqrt(d1) > dte || sqrt(d2) > dte);
  li = (d1 + d2) / 2.0;
  return ok && li > 15.0;
}
