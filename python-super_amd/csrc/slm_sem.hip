// slm_sem.hip -- Semantic-SuPer terms of the reference's GraphFit (autograd) path:
//
//   k_edge_flags / sem_extract_edges   class-boundary pixels of inputs[("seg",0)], once per frame
//                                      (find_edge_region with kernel 3, utils/utils.py:276-301, as
//                                      called at super/deform_mesh.py:149-165), row-major order
//   k_gf_morph                         semantic-boundary morphing term (super/deform_mesh.py:126-194):
//                                      surfels that project onto a pixel of another class are pulled
//                                      towards the 2 nearest boundary pixels of their own class
//
// The soft / hard segmentation weight of the point-to-plane term lives in k_gf_data (slm_gf.hip).
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "slm_host.h"
#include "slm_sem.h"
#include "slm_sem_search.h"

namespace {

// one thread per pixel: is it a boundary pixel of its own class?
__global__ void __launch_bounds__(256) k_edge_flags(int H, int W, int C, const int32_t* __restrict__ seg,
                                                     uint8_t* __restrict__ flags, int32_t* __restrict__ counts) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  const int y = pix / W, x = pix % W;
  const int c0 = seg[pix];
  bool edge = false;
  // ignore_img_edge: kernel (3) rows / columns at every image side; the margin-1 test is implied
  if (c0 >= 0 && c0 < C && y >= 3 && y < H - 3 && x >= 3 && x < W - 3) {
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) edge = edge || (seg[(y + dy) * W + (x + dx)] != c0);
  }
  for (int c = 0; c < C; ++c) flags[(size_t)c * H * W + pix] = (edge && c == c0) ? 1 : 0;
  if (edge) atomicAdd(&counts[c0], 1);
}

__global__ void __launch_bounds__(256) k_edge_pack(int n, int HW, int W, const int32_t* __restrict__ sel,
                                                    float2* __restrict__ xy) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int pix = sel[e] % HW;
  xy[e] = make_float2((float)(pix % W), (float)(pix / W));
}

}  // namespace

hipError_t sem_extract_edges(SemScratch& sc, int num_classes, const int32_t* img_seg, int H, int W, int32_t* edge_off,
                             hipStream_t st) {
  const int C = num_classes;
  const size_t HW = (size_t)H * W, n = HW * C;
  HIPRET(grow(sc.flags, sc.cap_flags, n, n));
  if (!sc.counts) HIPRET(hipMalloc((void**)&sc.counts, sizeof(int32_t) * (SLM_MAX_CLASSES + 1)));
  HIPRET(hipMemsetAsync(sc.counts, 0, sizeof(int32_t) * (SLM_MAX_CLASSES + 1), st));
  hipLaunchKernelGGL(k_edge_flags, dim3((HW + 255) / 256), dim3(256), 0, st, H, W, C, img_seg, sc.flags,
                     sc.counts);
  int32_t h[SLM_MAX_CLASSES + 1];
  HIPRET(hipMemcpyAsync(h, sc.counts, sizeof(h), hipMemcpyDeviceToHost, st));
  HIPRET(hipStreamSynchronize(st));
  edge_off[0] = 0;
  for (int c = 0; c < SLM_MAX_CLASSES; ++c) edge_off[c + 1] = edge_off[c] + (c < C ? h[c] : 0);
  const int total = edge_off[C];
  HIPRET(grow(sc.sel, sc.cap_sel, (size_t)total + 1, (size_t)total + 1));
  HIPRET(grow(sc.edge_xy, sc.cap_edge, (size_t)total + 1, (size_t)total + 1));
  if (total == 0) return hipSuccess;
  rocprim::counting_iterator<int32_t> first(0);
  HIPRET(with_scratch(sc.tmp, sc.cap_tmp, [&](void* tmp, size_t& bytes) {
    return rocprim::select(tmp, bytes, first, sc.flags, sc.sel, sc.counts + SLM_MAX_CLASSES, n, st);
  }));
  hipLaunchKernelGGL(k_edge_pack, dim3((total + 255) / 256), dim3(256), 0, st, total, (int)HW, W, sc.sel,
                     sc.edge_xy);
  return hipGetLastError();
}

hipError_t sem_ensure_morph(SemScratch& sc, int N) { return grow(sc.morph_g, sc.cap_morph, (size_t)N + 1, (size_t)N + 1); }

void sem_free(SemScratch& sc) {
  void* ptrs[] = {sc.flags, sc.sel, sc.counts, sc.tmp, sc.edge_xy, sc.morph_g};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  sc = SemScratch();
}

// grid = (ceil(maxN/256), n_frames).  The class sampling, the search and the keep test are slm_sem_search.h's, shared with the
// LM path's form of the term (k_morph_select, slm_morph.hip).
__global__ void __launch_bounds__(256) k_gf_morph(GfSlot* __restrict__ slots) {
  __shared__ double sm[16];
  GfSlotDev& s = gf_dev(slots)[blockIdx.y];
  if (!s.bound || !s.sem_bound) return;
  const FrameIn& f = s.f.base;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double li_sum = 0.0, kept = 0.0;
  // candidates of this workgroup (surfels whose projected class differs from their own), searched cooperatively below
  __shared__ SemCandLds cand;
  if (threadIdx.x == 0) cand.n_cand = 0;
  __syncthreads();
  int my_cand = -1, my_W = 0, my_H = 0;
  double my_x = 0.0, my_y = 0.0;
  if (i < f.N) {
    if (i >= s.shard_lo && i < s.shard_hi && (!s.f.sf_stable || s.f.sf_stable[i])) {
      d3 P;
      if (f.K == SLM_K) {   // (the default: the instantiation the other kernels use, operation for operation)
        GfSkin<SLM_K> k4;
        gf_skin<SLM_K>(s, i, k4);
        P = k4.P;
      } else {
        P = gf_skin_pos(s, i);
      }
      const int H = f.H, W = f.W, C = s.sem.num_classes;
      const double Ze = P.z + 1e-8;
      const double x = P.x * (double)f.fx / Ze + (double)f.cx, y = P.y * (double)f.fy / Ze + (double)f.cy;
      double gx, gy;
      const int best = sem_sample_class(s.sem.img_seg_conf, C, H, W, x, y, gx, gy);
      const int cls = s.sem.sf_seg[i];
      const bool val = best != cls && gx > -1.0 && gx < 1.0 && gy > -1.0 && gy < 1.0;
      if (val && cls >= 0 && cls < C) {
        const int e0 = s.edge_off[cls], e1 = s.edge_off[cls + 1];
        if (e1 - e0 >= 2) {      // a single boundary pixel has no 2nd neighbour: treated as no boundary
          s.terms[7] = 1.0;      // the class contributes a list entry (same value from every writer)
          // a candidate: its search is done by the WHOLE workgroup below
          const int k = atomicAdd(&cand.n_cand, 1);
          cand.x[k] = x;
          cand.y[k] = y;
          cand.e0[k] = e0;
          cand.e1[k] = e1;
          my_cand = k;
          my_x = x;
          my_y = y;
          my_W = W;
          my_H = H;
        }
      }
    }
  }
  __syncthreads();
  sem_search_candidates(cand, s.edge_xy);
  __syncthreads();
  if (i < f.N) {
    double2 g = make_double2(0.0, 0.0);
    if (my_cand >= 0) {
      const double x = my_x, y = my_y, d1 = cand.d1[my_cand], d2 = cand.d2[my_cand];
      const float2 p1 = s.edge_xy[cand.i1[my_cand]], p2 = s.edge_xy[cand.i2[my_cand]];
      // drop surfels closer to the image border than to the class boundary
      double li;
      if (sem_morph_keep(x, y, my_W, my_H, d1, d2, li)) {
        li_sum = li;
        kept = 1.0;
        g = make_double2(-(((double)p1.x - x) + ((double)p2.x - x)), -(((double)p1.y - y) + ((double)p2.y - y)));
      }
    }
    s.morph_g[i] = g;
  }
  const double a = block_sum(li_sum, sm), b = block_sum(kept, sm);
  if (threadIdx.x == 0 && b != 0.0) {   // (spread block partials, slm_gf.h; a fold sums them into terms[5] / [6])
    double* part = gf_part(s, blockIdx.x % GF_NCOPY);
    atomic_add_f64(part + GFP_MORPH_SUM, a);
    atomic_add_f64(part + GFP_MORPH_KEPT, b);
  }
}

void launch_gf_morph(GfSlot* slots, int n_frames, int maxN, hipStream_t st) {
  if (maxN <= 0) return;
  hipLaunchKernelGGL(k_gf_morph, dim3((maxN + 255) / 256, n_frames), dim3(256), 0, st, slots);
}
