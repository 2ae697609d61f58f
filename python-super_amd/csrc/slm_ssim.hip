// slm_ssim.hip -- the render loss of GraphFit (opt.render_loss, super/deform_mesh.py:113-123): monodepth2's SSIM layer
// with kernel 11 (depth/monodepth2/layers.py:217-247) between a render and the input colour frame, the validity mask,
// the m < 0.1 selection, the weighted sum, and dL/d(render).  Specified in include/super_lm.h (slm_render_ssim_loss);
// tests/render_grad_model.py restates it in torch.  Float64 arithmetic on float32 inputs.
//
// Three launches (two without the gradient), one workgroup per 16x16 pixel tile:
//   k_ssim_fwd  the tile's image / target with a halo of 5 (reflected; clipped for the mask) in LDS, per pixel the 11x11
//               sums in row-major order, SSIM, m, mask, selection; the loss and kept count of the tile (fixed-order
//               LDS tree) -> a partial per tile; with the gradient, per pixel and channel dL/d(mu_x, E[x^2], E[xy])
//   k_ssim_bwd  the transpose of the padded box means: pixel q gathers those three maps over the outputs p with
//               |p - q| <= 5 per axis, each weighted by how often q lies in p's reflected window (1..3 per axis)
//   k_ssim_sum  one workgroup: the tile partials in a fixed order -> loss_out
// No float atomics: the loss and the gradient are bitwise reproducible.
#include "slm_gf.h"
#include "slm_host.h"

#define SS_T 16                  // tile edge
#define SS_R 5                   // window radius (kernel 11)
#define SS_E (SS_T + 2 * SS_R)   // tile edge with the halo

namespace {

__device__ __forceinline__ int ss_reflect(int k, int n) {   // ReflectionPad2d index, clamped for the halo of cut-off tiles
  k = k < 0 ? -k : (k >= n ? 2 * n - 2 - k : k);
  return min(max(k, 0), n - 1);
}

// how often q lies in the reflected window of output p along an axis of n pixels (|p - q| <= 5; 0 otherwise)
__device__ __forceinline__ int ss_mult(int q, int p, int n) {
  int m = 1;
  if (q >= 1 && abs(p + q) <= SS_R) ++m;
  if (q <= n - 2 && abs(p - (2 * n - 2 - q)) <= SS_R) ++m;
  return m;
}

// fixed-order tree sum of v over the 256 lanes (every lane gets it)
__device__ __forceinline__ double ss_block_sum(double v, double* sm) {
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(256) k_ssim_fwd(int h, int w, const float* __restrict__ img, const float* __restrict__ tgt,
                                                  double weight, double* __restrict__ G, double* __restrict__ part) {
  __shared__ float sx[3][SS_E * SS_E], sy[3][SS_E * SS_E], smin[SS_E * SS_E];
  __shared__ double sred[256];
  const int tx0 = blockIdx.x * SS_T, ty0 = blockIdx.y * SS_T;
  for (int e = threadIdx.x; e < SS_E * SS_E; e += 256) {
    const int gi = ty0 - SS_R + e / SS_E, gj = tx0 - SS_R + e % SS_E;
    const int ri = ss_reflect(gi, h), rj = ss_reflect(gj, w);
    const size_t px = (size_t)ri * w + rj;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sx[c][e] = img[3 * px + c];
      sy[c][e] = tgt[(size_t)c * h * w + px];
    }
    // the mask's max pool pads with -inf: positions outside the image do not count
    smin[e] = (gi >= 0 && gi < h && gj >= 0 && gj < w) ? fminf(fminf(sx[0][e], sx[1][e]), sx[2][e]) : INFINITY;
  }
  __syncthreads();
  const int li = threadIdx.x / SS_T, lj = threadIdx.x % SS_T, i = ty0 + li, j = tx0 + lj;
  const bool inside = i < h && j < w;
  double loss = 0.0, kept = 0.0;
  double g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (inside) {
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double S[3], v[3], r[3], A1[3], A2[3], B1[3], B2[3], mx[3], my[3];
    for (int c = 0; c < 3; ++c) {
      double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
      for (int a = 0; a < 2 * SS_R + 1; ++a)
        for (int b = 0; b < 2 * SS_R + 1; ++b) {
          const int e = (li + a) * SS_E + lj + b;
          const double x = sx[c][e], y = sy[c][e];
          ax += x;
          ay += y;
          axx += x * x;
          ayy += y * y;
          axy += x * y;
        }
      const double n = 121.0;
      mx[c] = ax / n;
      my[c] = ay / n;
      const double sgx = axx / n - mx[c] * mx[c], sgy = ayy / n - my[c] * my[c], sgxy = axy / n - mx[c] * my[c];
      A1[c] = 2.0 * mx[c] * my[c] + C1;
      A2[c] = 2.0 * sgxy + C2;
      B1[c] = mx[c] * mx[c] + my[c] * my[c] + C1;
      B2[c] = sgx + sgy + C2;
      r[c] = (A1[c] * A2[c]) / (B1[c] * B2[c]);
      v[c] = (1.0 - r[c]) / 2.0;
      S[c] = fmin(fmax(v[c], 0.0), 1.0);
    }
    float mn = INFINITY;
    for (int a = 0; a < 2 * SS_R + 1; ++a)
      for (int b = 0; b < 2 * SS_R + 1; ++b) mn = fminf(mn, smin[(li + a) * SS_E + lj + b]);
    const double mean = (S[0] + S[1] + S[2]) / 3.0, m = mean * mean;
    if (mn > 0.f && m < 0.1) {
      loss = m;
      kept = 1.0;
      // dL/dr_c = weight * 2 mean / 3 * dS/dv * (-1/2), then r = A1 A2 / (B1 B2) by mu_x, E[x^2], E[xy]
      for (int c = 0; c < 3; ++c) {
        if (!(v[c] >= 0.0 && v[c] <= 1.0)) continue;
        const double gr = -weight * mean / 3.0, D = B1[c] * B2[c];
        const double dmx = (2.0 * my[c] * A2[c] - 2.0 * my[c] * A1[c]) / D - r[c] * (2.0 * mx[c] * B2[c] - 2.0 * mx[c] * B1[c]) / D;
        g[3 * c] = gr * dmx;
        g[3 * c + 1] = gr * (-r[c] / B2[c]);
        g[3 * c + 2] = gr * (2.0 * A1[c] / D);
      }
    }
    if (G) {
      double* o = G + 9 * ((size_t)i * w + j);
#pragma unroll
      for (int a = 0; a < 9; ++a) o[a] = g[a];
    }
  }
  const double tl = ss_block_sum(loss, sred), tk = ss_block_sum(kept, sred);
  if (threadIdx.x == 0) {
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[2 * b] = tl;
    part[2 * b + 1] = tk;
  }
}

__global__ void __launch_bounds__(256) k_ssim_bwd(int h, int w, const float* __restrict__ img, const float* __restrict__ tgt,
                                                  const double* __restrict__ G, double* __restrict__ grad) {
  __shared__ double sg[SS_E * SS_E * 9];
  const int tx0 = blockIdx.x * SS_T, ty0 = blockIdx.y * SS_T;
  for (int e = threadIdx.x; e < SS_E * SS_E * 9; e += 256) {
    const int cell = e / 9, a = e - 9 * cell;
    const int pi = ty0 - SS_R + cell / SS_E, pj = tx0 - SS_R + cell % SS_E;
    sg[e] = (pi >= 0 && pi < h && pj >= 0 && pj < w) ? G[9 * ((size_t)pi * w + pj) + a] : 0.0;
  }
  __syncthreads();
  const int li = threadIdx.x / SS_T, lj = threadIdx.x % SS_T, i = ty0 + li, j = tx0 + lj;
  if (i >= h || j >= w) return;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int a = 0; a < 2 * SS_R + 1; ++a) {
    const int pi = i - SS_R + a;
    if (pi < 0 || pi >= h) continue;
    const int mi = ss_mult(i, pi, h);
    for (int b = 0; b < 2 * SS_R + 1; ++b) {
      const int pj = j - SS_R + b;
      if (pj < 0 || pj >= w) continue;
      const double m = (double)(mi * ss_mult(j, pj, w));
      const double* s = sg + 9 * ((li + a) * SS_E + lj + b);
#pragma unroll
      for (int c = 0; c < 9; ++c) acc[c] += m * s[c];
    }
  }
  const size_t px = (size_t)i * w + j;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double x = img[3 * px + c], y = tgt[(size_t)c * h * w + px];
    grad[3 * px + c] = (acc[3 * c] + 2.0 * x * acc[3 * c + 1] + y * acc[3 * c + 2]) / 121.0;
  }
}

__global__ void __launch_bounds__(256) k_ssim_sum(int nb, const double* __restrict__ part, double weight,
                                                  double* __restrict__ loss_out) {
  __shared__ double sred[256];
  double l = 0.0, k = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    l += part[2 * b];
    k += part[2 * b + 1];
  }
  const double tl = ss_block_sum(l, sred), tk = ss_block_sum(k, sred);
  if (threadIdx.x == 0) {
    loss_out[0] = weight * tl;
    loss_out[1] = tk;
  }
}

}  // namespace

// the doubles of scratch one evaluation needs: the tile partials and, with the gradient, the three maps of k_ssim_fwd
size_t ssim_scratch_doubles(int h, int w, bool with_grad) {
  const size_t nb = (size_t)((w + SS_T - 1) / SS_T) * ((h + SS_T - 1) / SS_T);
  return 2 * nb + (with_grad ? 9 * (size_t)h * w : 0);
}

// the launches of one evaluation on the caller's scratch (h, w >= 6; grad_image may be null)
void ssim_enqueue(int h, int w, const float* image_hwc, const float* target_chw, double weight, double* loss_out,
                  double* grad_image, double* scratch, hipStream_t st) {
  const dim3 grid((w + SS_T - 1) / SS_T, (h + SS_T - 1) / SS_T);
  const int nb = (int)(grid.x * grid.y);
  double* part = scratch;
  double* G = grad_image ? scratch + 2 * (size_t)nb : nullptr;
  hipLaunchKernelGGL(k_ssim_fwd, grid, dim3(256), 0, st, h, w, image_hwc, target_chw, weight, G, part);
  hipLaunchKernelGGL(k_ssim_sum, dim3(1), dim3(256), 0, st, nb, part, weight, loss_out);
  if (grad_image) hipLaunchKernelGGL(k_ssim_bwd, grid, dim3(256), 0, st, h, w, image_hwc, target_chw, G, grad_image);
}

extern "C" int slm_render_ssim_loss(int32_t h, int32_t w, const float* image_hwc, const float* target_chw, double weight,
                                    double* loss_out, double* grad_image, void* stream) {
  if (!image_hwc || !target_chw || !loss_out) return fail(SLM_ERR_INVALID, "slm_render_ssim_loss: null argument");
  if (h < SS_R + 1 || w < SS_R + 1) return fail(SLM_ERR_INVALID, "slm_render_ssim_loss: h and w must be >= 6");
  hipStream_t st = (hipStream_t)stream;
  double* scratch = nullptr;
  hipError_t e = hipMallocAsync((void**)&scratch, sizeof(double) * ssim_scratch_doubles(h, w, grad_image != nullptr), st);
  if (e != hipSuccess)
    return fail(SLM_ERR_HIP, std::string("slm_render_ssim_loss: hipMallocAsync: ") + hipGetErrorString(e));
  ssim_enqueue(h, w, image_hwc, target_chw, weight, loss_out, grad_image, scratch, st);
  e = hipGetLastError();
  const hipError_t f = hipFreeAsync(scratch, st);
  if (e == hipSuccess) e = f;
  if (e != hipSuccess)
    return fail(SLM_ERR_HIP, std::string("slm_render_ssim_loss: ") + hipGetErrorString(e));
  return SLM_OK;
}
