// slm_render.hip -- the surfel renderer: Pulsar's blend (Lassner & Zollhoefer, CVPR 2021) at the parameters of the
// reference's call (renderer/renderer.py:23-78), forward and backward.  The image it computes is specified in
// include/super_lm.h and DESIGN.md section "Renderer"; tests/render_model.py restates it on the CPU.
//
// Forward (render_common, behind the five forward entry points): four launches and one 8-byte read-back.
//   k_rn_project  per point: float32 position, cull, pixel box of the sphere's silhouette, count per 16x16 tile
//   k_rn_scan     one workgroup: exclusive scan of the tile counts -> list offsets and scatter cursors
//   (host)        the list total sizes the key buffers
//   k_rn_scatter  per point: its key (rn_key: float bits of Z << 32 | row) into the list of every tile its box touches
//   k_rn_tile     one workgroup per tile, rn_walk: sort the tile's keys front to back (bitonic in LDS; a list longer than
//                 RN_SORT_CAP is sorted in LDS chunk by chunk and merged in global memory), then every lane walks its
//                 pixel's list front to back in LDS chunks, keeps the first n_track hits and blends in float64.
// The keys are unique (one per point and tile), so the sorted order -- and with it every float64 sum, taken by one
// lane in list order -- does not depend on the order the atomic cursors handed out slots: renders are bitwise
// reproducible.  The only atomics are integer ones (tile counts, cursors).
//
// Every forward leaves on the context what a backward needs: the float32 centres and pixel boxes, a copy of the points'
// values, the sorted tile lists (written back to `keys` on both sort paths) and per pixel the float64 blend (zt_max, W, C)
// with the list position of its n_track-th hit.  Backward (rn_backward, behind the four backward entry points): two
// launches, store-and-sum, no float atomics.
//   k_rn_bwd_entry  one workgroup per tile, rn_bwd_tile: the tile's pixel coefficients g/W, g.C/W in LDS, then per list entry
//                   the contributions of the pixels of its box inside the tile, summed in row-major pixel order -> `slab`
//   k_rn_bwd_point  per point, rn_point_entries: the slab entries of its tiles, each found by binary search of its key
//                   (rn_find), summed in tile order
// What is asked for -- the point gradient, the value gradient, the radius gradient -- decides the doubles per slab entry.
//
// Two things vary, and each kernel family has one instantiation per combination:
//   PR        per-point radii (slm_render_points_radii, slm_gf_render_radii, a channels forward with radii): the radius of a
//             point is pos[].w, where k_rn_project<SRC, true> leaves the caller's float32 value (so a later backward does not
//             depend on the caller's buffer); a radius that is not finite or not > 0 culls its row.  Without PR every point
//             has the one double radius of the parameters.  Only a PR forward has a radius gradient.
//   channels  three colours read in place from the caller's rows (k_rn_tile, k_rn_bwd_entry<MODE>, k_rn_bwd_point_ex<MODE>:
//             what is asked for is the compile-time MODE), or C = 1..8 features copied into padded rows on the context
//             (k_rn_tile_ch<CP>, k_rn_bwd_entry_ch, k_rn_bwd_point_ch: C and what is asked for are run-time uniforms).  The
//             two share rn_walk and rn_bwd_tile and differ in how a hit's values are accumulated, in s_k and the value
//             gradient, and in the pixel record (RnPix alone, or RnPix + pixf).
#include <climits>
#include <cmath>
#include <cstring>
#include "slm_gf.h"
#include "slm_host.h"

#define RN_TILE 16            // tile edge in pixels: one lane per pixel, 256 lanes per workgroup
#define RN_SORT_CAP 4096      // keys a workgroup sorts in LDS at once (32 KB)
#define RN_CHUNK 256          // list entries staged in LDS per step of the walk

struct slm_render {
  int H = 0, W = 0, cap = 0;
  float4* pos = nullptr;                 // (cap) float32 centre; w: the point's radius after a per-point forward, else 0
  int4* box = nullptr;                   // (cap) inclusive pixel box x0, x1, y0, y1 (x0 > x1: culled)
  unsigned int* cnt = nullptr;           // (tiles) entries per tile
  unsigned long long* off = nullptr;     // (tiles + 1) exclusive scan of cnt
  unsigned long long* cur = nullptr;     // (tiles) scatter cursors
  unsigned long long* keys = nullptr;    // (cap_keys) tile lists
  unsigned long long* tmp = nullptr;     // (cap_tmp, as many) merge scratch of the overflow path
  size_t cap_keys = 0, cap_tmp = 0;
  unsigned long long* h_total = nullptr; // pinned host copy of off[tiles]
  unsigned long long* stat = nullptr;    // (3) status of the guarded forwards (rn_gf_forward): renders over their entry
                                         // limit, the largest list total, the last total -- since rn_gf_size cleared it
  // ---- state of the last forward, read by slm_render_backward ----
  float4* col = nullptr;                 // (cap) colours of the points, w unused
  struct RnPix* pix = nullptr;           // (H * W) per-pixel blend record
  double* slab = nullptr;                // (cap_slab doubles) per tile-list entry partials: dL/dP and / or dL/dc
  size_t cap_slab = 0;
  slm_render_params last{};              // parameters of the last forward
  int n_last = 0;                        // its point count
  unsigned long long total_last = 0;     // its tile-list entries
  int has_fwd = 0;                       // 1 after a forward that completed; cleared when one starts
  int per_point_last = 0;                // 1 when that forward had per-point radii (pos[].w)
  // ---- only after slm_render_points_channels (grown on its first call; a context without one never allocates them) ----
  float* feat = nullptr;                 // (cap_feat floats) the points' features, rows padded with 0 to 4 or 8 floats
  double* pixf = nullptr;                // (cap_pixf doubles) per pixel the C float64 blended channels; pix holds zt_max, W, cut
  size_t cap_feat = 0, cap_pixf = 0;
  int ch_last = 0;                       // the channel count of that forward when it was a channels one, else 0
};

// the per-pixel record of a forward: float64 blend of the taken hits, and `cut`, the list position of the n_track-th hit
// (INT_MAX: fewer hits) -- entries behind it do not reach the pixel
struct RnPix {
  double zt_max, W, c0, c1, c2;
  int cut, pad;
};

namespace {

struct RnCam {
  int w, h, tiles_x, n_track;
  double f, ccx, ccy, r, zn, zf, gamma, eps;
  float bg0, bg1, bg2;
};

enum { RN_SRC_F32 = 0, RN_SRC_F64 = 1, RN_SRC_GF = 2 };

// inclusive pixel range [lo, hi] of the lines whose slope t (x/z or y/z) lies strictly inside the silhouette
// (c z -+ r sqrt(c^2 + z^2 - r^2)) / (z^2 - r^2) of a sphere seen from the origin, padded by 1e-3 px
__device__ __forceinline__ void rn_range(double c, double z, double r, double f, double cc, int n, int& lo, int& hi) {
  const double den = z * z - r * r, disc = c * c + den;
  if (!(den > 0.0) || !(disc > 0.0)) {   // the sphere reaches the camera plane: every pixel is a candidate
    lo = 0;
    hi = n - 1;
    return;
  }
  const double s = r * sqrt(disc);
  double a = f * (c * z - s) / den + cc - 1e-3, b = f * (c * z + s) / den + cc + 1e-3;
  a = fmin(fmax(a, -1.0), (double)n);
  b = fmin(fmax(b, -1.0), (double)n);
  lo = max((int)ceil(a), 0);
  hi = min((int)floor(b), n - 1);
}

// pixel (i, j)'s ray direction d = (dx, dy, 1) and 1 / |d|
__device__ __forceinline__ void rn_ray(const RnCam& cam, int i, int j, double& dx, double& dy, double& inv_dn) {
  dx = ((double)j - cam.ccx) / cam.f;
  dy = ((double)i - cam.ccy) / cam.f;
  inv_dn = 1.0 / sqrt(dx * dx + dy * dy + 1.0);
}

// |P x d| / |d|: the one expression the forward's and the backward's coverage tests share
__device__ __forceinline__ double rn_rho(double X, double Y, double Z, double dx, double dy, double inv_dn) {
  const double cx = Y - Z * dy, cy = Z * dx - X, cz = X * dy - Y * dx;
  return sqrt(cx * cx + cy * cy + cz * cz) * inv_dn;
}

template <int SRC, bool PR>
__global__ void __launch_bounds__(256) k_rn_project(int N, const void* __restrict__ pts, GfSlot* __restrict__ gslot, RnCam cam,
                                                    float4* __restrict__ pos, int4* __restrict__ box,
                                                    unsigned int* __restrict__ cnt, const float* __restrict__ colors,
                                                    int cstride, float4* __restrict__ col,
                                                    const float* __restrict__ radii) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float X, Y, Z;
  bool live = true;
  if constexpr (SRC == RN_SRC_F32) {
    const float* p = static_cast<const float*>(pts) + 3 * (size_t)i;
    X = p[0]; Y = p[1]; Z = p[2];
  } else if constexpr (SRC == RN_SRC_F64) {
    const double* p = static_cast<const double*>(pts) + 3 * (size_t)i;
    X = (float)p[0]; Y = (float)p[1]; Z = (float)p[2];   // tensor.float(): round to nearest
  } else {
    const GfSlotDev& s = *gf_dev(gslot);
    const uint8_t* st = s.f.sf_stable;
    live = !st || st[i];
    X = Y = Z = 0.f;
    if (live) {
      const d3 P = gf_skin_pos(s, i);
      X = (float)P.x; Y = (float)P.y; Z = (float)P.z;
    }
  }
  if (live) {   // the backward's copy of the colours (rows of unstable surfels are not read)
    const float* c = colors + (size_t)i * cstride;
    col[i] = make_float4(c[0], c[1], c[2], 0.f);
  }
  float rw = 0.f;
  double r = cam.r;
  if constexpr (PR) {   // the point's own radius, by row (rows of unstable surfels are not read); NaN, inf, <= 0: culled
    if (live) {
      rw = radii[i];
      r = (double)rw;
      live = rw > 0.f && rw < INFINITY;
    }
  }
  int4 b = make_int4(1, 0, 1, 0);   // empty
  if (live && (double)Z >= cam.zn && (double)Z <= cam.zf) {
    int x0, x1, y0, y1;
    rn_range((double)X, (double)Z, r, cam.f, cam.ccx, cam.w, x0, x1);
    rn_range((double)Y, (double)Z, r, cam.f, cam.ccy, cam.h, y0, y1);
    if (x0 <= x1 && y0 <= y1) {
      b = make_int4(x0, x1, y0, y1);
      for (int ty = y0 / RN_TILE; ty <= y1 / RN_TILE; ++ty)
        for (int tx = x0 / RN_TILE; tx <= x1 / RN_TILE; ++tx) atomicAdd(cnt + ty * cam.tiles_x + tx, 1u);
    }
  }
  pos[i] = make_float4(X, Y, Z, rw);
  box[i] = b;
}

// exclusive scan of n tile counts, one workgroup of 1024 lanes, 1024 counts per round
// The guarded form (stat != null: the enqueue-only forward, which cannot size the lists from the total) compares the total
// with `limit`, the entries the lists hold: over it every list is left empty (off and cur all 0), so that nothing behind this
// kernel indexes keys, tmp or the slab at all, and stat counts the render; stat also keeps the last and the largest total.
__global__ void __launch_bounds__(1024) k_rn_scan(int n, const unsigned int* __restrict__ cnt,
                                                  unsigned long long* __restrict__ off, unsigned long long* __restrict__ cur,
                                                  unsigned long long limit, unsigned long long* __restrict__ stat) {
  __shared__ unsigned long long s[1024];
  __shared__ unsigned long long carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const unsigned long long v = base + t < n ? cnt[base + t] : 0ull;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const unsigned long long a = t >= d ? s[t - d] : 0ull;
      __syncthreads();
      s[t] += a;
      __syncthreads();
    }
    const unsigned long long ex = carry + s[t] - v;
    if (base + t < n) {
      off[base + t] = ex;
      cur[base + t] = ex;
    }
    __syncthreads();
    if (t == 1023) carry += s[1023];
    __syncthreads();
  }
  const unsigned long long total = carry;
  const bool over = stat && total > limit;
  if (over) {   // (element e was written above by this same lane)
    for (int e = t; e <= n; e += 1024) {
      off[e] = 0;
      if (e < n) cur[e] = 0;
    }
  } else if (t == 0) {
    off[n] = total;
  }
  if (stat && t == 0) {
    if (over) stat[0] += 1;
    if (total > stat[1]) stat[1] = total;
    stat[2] = total;
  }
}

// the key of point i in the list of every tile it touches: ascending keys are front to back (Z > 0), ties by row
__device__ __forceinline__ unsigned long long rn_key(const float4* __restrict__ pos, int i) {
  return ((unsigned long long)__float_as_uint(pos[i].z) << 32) | (unsigned int)i;
}

#define RN_ABSENT (~0ull)

// the position of `key` in tile t's sorted list (keys are unique), or RN_ABSENT
__device__ __forceinline__ unsigned long long rn_find(const unsigned long long* __restrict__ off,
                                                      const unsigned long long* __restrict__ keys, int t, unsigned long long key) {
  unsigned long long lo = off[t], hi = off[t + 1];
  while (lo < hi) {
    const unsigned long long mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo < off[t + 1] && keys[lo] == key ? lo : RN_ABSENT;
}

// total != null (the guarded forward): nothing is written when the render's total, left there by k_rn_scan, is over `limit`
__global__ void __launch_bounds__(256) k_rn_scatter(int N, int tiles_x, const float4* __restrict__ pos,
                                                    const int4* __restrict__ box, unsigned long long* __restrict__ cur,
                                                    unsigned long long* __restrict__ keys,
                                                    const unsigned long long* __restrict__ total, unsigned long long limit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (total && *total > limit) return;
  const int4 b = box[i];
  if (b.x > b.y) return;
  const unsigned long long key = rn_key(pos, i);
  for (int ty = b.z / RN_TILE; ty <= b.w / RN_TILE; ++ty)
    for (int tx = b.x / RN_TILE; tx <= b.y / RN_TILE; ++tx) {
      const unsigned long long at = atomicAdd(cur + ty * tiles_x + tx, 1ull);
      keys[at] = key;
    }
}

// ascending bitonic sort of s[0, n2), n2 a power of two, all 256 lanes
__device__ __forceinline__ void rn_bitonic(unsigned long long* s, int n2) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = threadIdx.x; q < (n2 >> 1); q += 256) {
        const int a = ((q & ~(j - 1)) << 1) | (q & (j - 1)), c = a | j;
        const unsigned long long x = s[a], y = s[c];
        if ((x > y) == ((a & k) == 0)) {
          s[a] = y;
          s[c] = x;
        }
      }
      __syncthreads();
    }
}

// load m keys into LDS, pad to a power of two with ~0, sort
__device__ __forceinline__ void rn_sort_lds(unsigned long long* s, const unsigned long long* g, int m) {
  int n2 = 2;
  while (n2 < m) n2 <<= 1;
  for (int e = threadIdx.x; e < n2; e += 256) s[e] = e < m ? g[e] : ~0ull;
  __syncthreads();
  rn_bitonic(s, n2);
}

// sort the n keys of a tile's list front to back, all 256 lanes; the sorted list ends in `list` on every path and, when
// n <= RN_SORT_CAP, in skey as well.  `scratch` (n keys) serves the merges of a longer list.
__device__ __forceinline__ void rn_tile_sort(unsigned long long* skey, unsigned long long* list, unsigned long long* scratch,
                                             int n) {
  if (n > 0 && n <= RN_SORT_CAP) {
    rn_sort_lds(skey, list, n);
    for (int e = threadIdx.x; e < n; e += 256) list[e] = skey[e];   // the backward finds its keys in the sorted list
  } else if (n > RN_SORT_CAP) {
    // overflow path: sorted runs of RN_SORT_CAP, then pairwise merges (rank of every key in the partner run by
    // binary search -- the keys are unique) ping-ponging between the list and the scratch
    for (int c = 0; c < n; c += RN_SORT_CAP) {
      const int m = min(RN_SORT_CAP, n - c);
      rn_sort_lds(skey, list + c, m);
      for (int e = threadIdx.x; e < m; e += 256) list[c + e] = skey[e];
      __syncthreads();
    }
    unsigned long long *src = list, *dst = scratch;
    for (int wdt = RN_SORT_CAP; wdt < n; wdt <<= 1) {
      for (int e = threadIdx.x; e < n; e += 256) {
        const int run = e / wdt, lo = run * wdt, pb = (run & ~1) * wdt;
        const int plo = (run & 1) ? lo - wdt : lo + wdt, phi = (run & 1) ? lo : min(lo + 2 * wdt, n);
        const unsigned long long k = src[e];
        int a = plo, b = max(plo, phi);
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (src[mid] < k) a = mid + 1; else b = mid;
        }
        dst[pb + (e - lo) + (a - plo)] = k;
      }
      __syncthreads();
      unsigned long long* t = src;
      src = dst;
      dst = t;
    }
    if (src != list) {   // the sorted list ends in `keys` on every path
      for (int e = threadIdx.x; e < n; e += 256) list[e] = src[e];
      __syncthreads();
    }
  }
}

// What the walk of a tile leaves in every lane: its pixel and whether that lies in the image, the hits it took (<= n_track),
// the front-most row (-1: none), the list position of the n_track-th hit (INT_MAX: fewer), the depth term of the first hit
// and the sum of the weights.
struct RnWalk {
  int i, j, nh, first, cut;
  bool inside;
  double zt_max, sw;
};

// The forward of one tile, all 256 lanes of its workgroup: sort the tile's list front to back (it stays in `keys` for the
// backward), then every lane walks its pixel's ray down the list, staged in LDS RN_CHUNK entries at a time, and takes the
// first n_track entries whose box holds the pixel and whose sphere the ray enters (rho < r; r the point's own with PR, else
// the parameters'), each with the weight w_k = (1 - rho / r) exp((zt - zt_max) / gamma).  hit(row, w_k) accumulates the
// point's values: the one step of the walk in which the three-channel and the N-channel kernels differ.  The workgroup
// leaves the list when no lane is active any more.
template <bool PR, typename Hit>
__device__ __forceinline__ RnWalk rn_walk(const RnCam& cam, const unsigned long long* __restrict__ off,
                                          unsigned long long* __restrict__ keys, unsigned long long* __restrict__ tmp,
                                          const float4* __restrict__ pos, const int4* __restrict__ box, Hit hit) {
  __shared__ unsigned long long skey[RN_SORT_CAP];
  __shared__ float4 spos[RN_CHUNK];
  __shared__ int4 sbox[RN_CHUNK];
  __shared__ int sid[RN_CHUNK];
  const int tile = blockIdx.y * cam.tiles_x + blockIdx.x;
  const unsigned long long base = off[tile];
  const int n = (int)(off[tile + 1] - base);
  unsigned long long* list = keys + base;
  const unsigned long long* gl = list;   // the sorted list when it does not fit in LDS
  rn_tile_sort(skey, list, tmp + base, n);
  const bool in_lds = n <= RN_SORT_CAP;

  const int j = blockIdx.x * RN_TILE + (threadIdx.x & (RN_TILE - 1));
  const int i = blockIdx.y * RN_TILE + (threadIdx.x / RN_TILE);
  RnWalk w = {i, j, 0, -1, INT_MAX, i < cam.h && j < cam.w, 0.0, 0.0};
  double dx, dy, inv_dn;
  rn_ray(cam, i, j, dx, dy, inv_dn);
  const double zspan = cam.zf - cam.zn;
  bool active = w.inside;
  for (int c0 = 0; c0 < n; c0 += RN_CHUNK) {
    const int m = min(RN_CHUNK, n - c0);
    if (threadIdx.x < m) {
      const unsigned long long k = in_lds ? skey[c0 + threadIdx.x] : gl[c0 + threadIdx.x];
      const int id = (int)(unsigned int)k;
      sid[threadIdx.x] = id;
      spos[threadIdx.x] = pos[id];
      sbox[threadIdx.x] = box[id];
    }
    __syncthreads();
    if (active) {
      for (int e = 0; e < m; ++e) {
        const int4 b = sbox[e];
        if (j < b.x || j > b.y || i < b.z || i > b.w) continue;
        const float4 p = spos[e];
        const double X = p.x, Y = p.y, Z = p.z;
        const double rho = rn_rho(X, Y, Z, dx, dy, inv_dn);
        const double r = PR ? (double)p.w : cam.r;
        if (!(rho < r)) continue;
        const double zt = (cam.zf - Z) / zspan;
        const int id = sid[e];
        if (w.nh == 0) {
          w.zt_max = zt;
          w.first = id;
        }
        const double wk = (1.0 - rho / r) * exp((zt - w.zt_max) / cam.gamma);
        w.sw += wk;
        hit(id, wk);
        if (++w.nh == cam.n_track) {
          w.cut = c0 + e;
          active = false;
          break;
        }
      }
    }
    if (!__syncthreads_or(active && c0 + RN_CHUNK < n)) break;
  }
  return w;
}

// the three-channel forward: three float64 sums of w_k c_k over the caller's colours; the pixel's record goes to pix
template <bool PR>
__global__ void __launch_bounds__(256) k_rn_tile(RnCam cam, const unsigned long long* __restrict__ off,
                                                 unsigned long long* __restrict__ keys, unsigned long long* __restrict__ tmp,
                                                 const float4* __restrict__ pos, const int4* __restrict__ box,
                                                 const float* __restrict__ colors, int cstride, float* __restrict__ image,
                                                 int* __restrict__ front_id, int* __restrict__ hit_count, RnPix* __restrict__ pix) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const RnWalk w = rn_walk<PR>(cam, off, keys, tmp, pos, box, [&](int id, double wk) {
    const float* c = colors + (size_t)id * cstride;
    s0 += wk * (double)c[0];
    s1 += wk * (double)c[1];
    s2 += wk * (double)c[2];
  });
  if (!w.inside) return;
  const size_t px = (size_t)w.i * cam.w + w.j;
  float o0 = cam.bg0, o1 = cam.bg1, o2 = cam.bg2;
  RnPix rec = {0.0, 0.0, 0.0, 0.0, 0.0, w.cut, 0};
  if (w.nh > 0) {
    const double wbg = exp((cam.eps - w.zt_max) / cam.gamma), den = w.sw + wbg;
    rec.zt_max = w.zt_max;
    rec.W = den;
    rec.c0 = (s0 + wbg * (double)cam.bg0) / den;
    rec.c1 = (s1 + wbg * (double)cam.bg1) / den;
    rec.c2 = (s2 + wbg * (double)cam.bg2) / den;
    o0 = (float)rec.c0;
    o1 = (float)rec.c1;
    o2 = (float)rec.c2;
  }
  pix[px] = rec;
  image[3 * px] = o0;
  image[3 * px + 1] = o1;
  image[3 * px + 2] = o2;
  if (front_id) front_id[px] = w.first;
  if (hit_count) hit_count[px] = w.nh;
}

// ---- N-channel features (slm_render_points_channels) ----------------------------------------------------------------------
// The context's copy of the features has rows of CP floats, CP = 4 for C <= 4 and 8 otherwise, the columns past C zero: the
// walk and the backward read a row as one or two float4 and the padded sums cost a few FMAs on zeros.  k_rn_project then
// reads that copy as its `colors` (stride CP), so the one-radius and per-point projections serve unchanged.
struct RnBg { float v[SLM_RENDER_MAX_CHANNELS]; };

__global__ void __launch_bounds__(256) k_rn_feat(int N, int C, int CP, const float* __restrict__ features, int stride,
                                                 float* __restrict__ feat) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)N * CP) return;
  const size_t i = q / CP;
  const int c = (int)(q - i * CP);
  feat[q] = c < C ? features[i * stride + c] : 0.f;
}

// The N-channel forward: CP accumulators (a compile-time bound, padded: see above) of which the first C are written.  Every
// channel's sum is the FMA chain that k_rn_tile's s0 / s1 / s2 compile to, written out, so a channel is bitwise what the
// three-channel kernel gives for the same column.  The record of a pixel: zt_max, W and cut in pix (its colour fields 0), the
// C float64 channels in pixf.
template <bool PR, int CP>
__global__ void __launch_bounds__(256) k_rn_tile_ch(RnCam cam, RnBg bg, int C, const unsigned long long* __restrict__ off,
                                                    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ tmp,
                                                    const float4* __restrict__ pos, const int4* __restrict__ box,
                                                    const float* __restrict__ feat, float* __restrict__ image,
                                                    int* __restrict__ front_id, int* __restrict__ hit_count,
                                                    RnPix* __restrict__ pix, double* __restrict__ pixf) {
  double s[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) s[c] = 0.0;
  const RnWalk w = rn_walk<PR>(cam, off, keys, tmp, pos, box, [&](int id, double wk) {
    const float4* f = reinterpret_cast<const float4*>(feat + (size_t)id * CP);
#pragma unroll
    for (int q = 0; q < CP / 4; ++q) {
      const float4 v = f[q];
      s[4 * q] = fma(wk, (double)v.x, s[4 * q]);
      s[4 * q + 1] = fma(wk, (double)v.y, s[4 * q + 1]);
      s[4 * q + 2] = fma(wk, (double)v.z, s[4 * q + 2]);
      s[4 * q + 3] = fma(wk, (double)v.w, s[4 * q + 3]);
    }
  });
  if (!w.inside) return;
  const size_t px = (size_t)w.i * cam.w + w.j;
  RnPix rec = {0.0, 0.0, 0.0, 0.0, 0.0, w.cut, 0};
  double den = 1.0, wbg = 0.0;
  if (w.nh > 0) {
    wbg = exp((cam.eps - w.zt_max) / cam.gamma);
    den = w.sw + wbg;
    rec.zt_max = w.zt_max;
    rec.W = den;
  }
  pix[px] = rec;
#pragma unroll
  for (int c = 0; c < CP; ++c)
    if (c < C) {
      float o = bg.v[c];
      double F = 0.0;
      if (w.nh > 0) {
        F = fma(wbg, (double)bg.v[c], s[c]) / den;
        o = (float)F;
      }
      pixf[px * C + c] = F;
      image[px * C + c] = o;
    }
  if (front_id) front_id[px] = w.first;
  if (hit_count) hit_count[px] = w.nh;
}

// Backward, pass 1 (see the top of the file), all 256 lanes of a tile's workgroup.  Lane t stages pixel t of the tile -- its
// ray, zt_max and cut, or cut = -1 when val.stage() says that the pixel has no hit or g = 0 -- then every lane takes list
// entries e = t, t + 256, ... and sums, in row-major order over the pixels of the entry's box inside the tile that it reaches
// (position <= cut, rho < r: the forward's decisions), with e_k = exp((zt - zt_max) / gamma) and w_k = (1 - rho / r) e_k:
//   GP  s_k ( -(e_k / r) drho/dP - w_k / (gamma zspan) z ),   GR  s_k e_k rho / r^2   (per-point radii only),
// into the first three and the last of the entry's S slab doubles.  With PR the radius r is the point's (pos[].w), else the
// parameters'.  The values of the points -- three colours or C features -- are Val's:
//   stage(t, px, rec)  read g at pixel px; false when W = 0 or g = 0, else a = g / W and b = g.C / W of pixel t into LDS
//   entry(id)          read the values of point id, clear its value gradient
//   sk(t)              s_k = a.c_k - b at pixel t (asked only with GP or GR)
//   add(t, w_k)        value gradient += a w_k
//   store(o)           the value gradient into the slab, behind the point's
template <bool PR, typename Val>
__device__ __forceinline__ void rn_bwd_tile(const RnCam& cam, const unsigned long long* __restrict__ off,
                                            const unsigned long long* __restrict__ keys, const float4* __restrict__ pos,
                                            const int4* __restrict__ box, const RnPix* __restrict__ pix,
                                            double* __restrict__ slab, const int S, const bool GP, const bool GR, Val val) {
  __shared__ double sdx[256], sdy[256], sinv[256], szt[256];
  __shared__ int scut[256];
  const int tile = blockIdx.y * cam.tiles_x + blockIdx.x;
  const unsigned long long base = off[tile];
  const int n = (int)(off[tile + 1] - base);
  if (n == 0) return;
  const int tx0 = blockIdx.x * RN_TILE, ty0 = blockIdx.y * RN_TILE;
  {
    const int t = threadIdx.x, j = tx0 + (t & (RN_TILE - 1)), i = ty0 + t / RN_TILE;
    int cut = -1;
    if (i < cam.h && j < cam.w) {
      const size_t px = (size_t)i * cam.w + j;
      const RnPix rec = pix[px];
      if (val.stage(t, px, rec)) {
        cut = rec.cut;
        szt[t] = rec.zt_max;
        double dx, dy, inv_dn;
        rn_ray(cam, i, j, dx, dy, inv_dn);
        sdx[t] = dx;
        sdy[t] = dy;
        sinv[t] = inv_dn;
      }
    }
    scut[t] = cut;
  }
  __syncthreads();
  const double zspan = cam.zf - cam.zn, kz = 1.0 / (cam.gamma * zspan);
  for (int e = threadIdx.x; e < n; e += 256) {
    const int id = (int)(unsigned int)keys[base + e];
    const int4 b = box[id];
    const float4 p = pos[id];
    val.entry(id);
    const double X = p.x, Y = p.y, Z = p.z;
    const double zt = (cam.zf - Z) / zspan;
    const double r = PR ? (double)p.w : cam.r;
    double gx = 0.0, gy = 0.0, gz = 0.0, gr = 0.0;
    const int i0 = max(b.z, ty0), i1 = min(b.w, ty0 + RN_TILE - 1), j0 = max(b.x, tx0), j1 = min(b.y, tx0 + RN_TILE - 1);
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) {
        const int t = (i - ty0) * RN_TILE + (j - tx0);
        if (e > scut[t]) continue;
        const double dx = sdx[t], dy = sdy[t], inv_dn = sinv[t];
        const double rho = rn_rho(X, Y, Z, dx, dy, inv_dn);
        if (!(rho < r)) continue;
        const double ek = exp((zt - szt[t]) / cam.gamma), wk = (1.0 - rho / r) * ek;
        double sk = 0.0;
        if (GP || GR) sk = val.sk(t);
        if (GR) gr += sk * ek * rho / (r * r);
        if (GP) {
          if (rho > 0.0) {
            // drho/dP = (P - (P.d^) d^) / rho, d^ = d / |d|
            const double hx = dx * inv_dn, hy = dy * inv_dn, hz = inv_dn;
            const double pd = X * hx + Y * hy + Z * hz;
            const double q = -sk * ek / (r * rho);
            gx += q * (X - pd * hx);
            gy += q * (Y - pd * hy);
            gz += q * (Z - pd * hz);
          }
          gz -= sk * wk * kz;
        }
        val.add(t, wk);
      }
    double* o = slab + (size_t)S * (base + e);
    if (GP) {
      o[0] = gx;
      o[1] = gy;
      o[2] = gz;
    }
    val.store(o + (GP ? 3 : 0));
    if (GR) o[S - 1] = gr;
  }
}

// What a backward computes: the point gradient, the colour (value) gradient, the radius gradient, or any union of them.  A
// slab entry holds, packed in this order, 3 doubles for the point, 3 (C with channels) for the values, 1 for the radius.
enum { RN_BWD_POINTS = 1, RN_BWD_COLORS = 2, RN_BWD_RADII = 4 };

// pass 1 after a three-channel forward: MODE is a template parameter, so every union of outputs has its own registers and LDS
// (no b, and no read of the colours, for the colour gradient alone).  RN_BWD_RADII needs PR.
template <int MODE, bool PR>
__global__ void __launch_bounds__(256) k_rn_bwd_entry(RnCam cam, const unsigned long long* __restrict__ off,
                                                      const unsigned long long* __restrict__ keys, const float4* __restrict__ pos,
                                                      const int4* __restrict__ box, const float4* __restrict__ col,
                                                      const RnPix* __restrict__ pix, const double* __restrict__ gimg,
                                                      double* __restrict__ slab) {
  constexpr bool GP = (MODE & RN_BWD_POINTS) != 0, GC = (MODE & RN_BWD_COLORS) != 0, GR = (MODE & RN_BWD_RADII) != 0;
  constexpr bool GS = GP || GR;   // s_k is needed: the colour copy and b
  constexpr int S = (GP ? 3 : 0) + (GC ? 3 : 0) + (GR ? 1 : 0);
  static_assert(PR || !GR, "the radius gradient belongs to a per-point forward");
  __shared__ double sa0[256], sa1[256], sa2[256], sb[GS ? 256 : 1];
  struct Val {
    const float4* __restrict__ col;
    const double* __restrict__ gimg;
    float4 c;
    double q0, q1, q2;
    __device__ bool stage(int t, size_t px, const RnPix& rec) {
      const double g0 = gimg[3 * px], g1 = gimg[3 * px + 1], g2 = gimg[3 * px + 2];
      if (!(rec.W > 0.0 && (g0 != 0.0 || g1 != 0.0 || g2 != 0.0))) return false;
      sa0[t] = g0 / rec.W;
      sa1[t] = g1 / rec.W;
      sa2[t] = g2 / rec.W;
      if constexpr (GS) sb[t] = (g0 * rec.c0 + g1 * rec.c1 + g2 * rec.c2) / rec.W;
      return true;
    }
    __device__ void entry(int id) {
      c = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (GS) c = col[id];
      q0 = q1 = q2 = 0.0;
    }
    __device__ double sk(int t) const { return sa0[t] * (double)c.x + sa1[t] * (double)c.y + sa2[t] * (double)c.z - sb[t]; }
    __device__ void add(int t, double wk) {
      if constexpr (GC) {
        q0 += sa0[t] * wk;
        q1 += sa1[t] * wk;
        q2 += sa2[t] * wk;
      }
    }
    __device__ void store(double* o) const {
      if constexpr (GC) {
        o[0] = q0;
        o[1] = q1;
        o[2] = q2;
      }
    }
  };
  rn_bwd_tile<PR>(cam, off, keys, pos, box, pix, slab, S, GP, GR, Val{col, gimg});
}

// pass 1 after a channels forward.  The channel count is a run-time bound of loops unrolled to SLM_RENDER_MAX_CHANNELS, and
// what is wanted (RN_BWD_COLORS: here the features) a run-time uniform too: one instantiation per PR instead of MODE x PR x C.
// Every output is summed in its own registers by the same instructions whatever else is wanted, so it does not depend on the
// others.  In LDS a_c = g_c / W (C x 256 doubles) and b = sum_c g_c F_c / W;  s_k = sum_c a_c f_kc - b.
template <bool PR>
__global__ void __launch_bounds__(256) k_rn_bwd_entry_ch(RnCam cam, int C, int CP, int want,
                                                         const unsigned long long* __restrict__ off,
                                                         const unsigned long long* __restrict__ keys,
                                                         const float4* __restrict__ pos, const int4* __restrict__ box,
                                                         const float* __restrict__ feat, const RnPix* __restrict__ pix,
                                                         const double* __restrict__ pixf, const double* __restrict__ gimg,
                                                         double* __restrict__ slab) {
  constexpr int MC = SLM_RENDER_MAX_CHANNELS;
  __shared__ double sb[256], sa[MC][256];
  const bool GP = (want & RN_BWD_POINTS) != 0, GC = (want & RN_BWD_COLORS) != 0, GR = PR && (want & RN_BWD_RADII) != 0;
  const int S = (GP ? 3 : 0) + (GC ? C : 0) + (GR ? 1 : 0);
  struct Val {
    int C, CP;
    bool GC;
    const float* __restrict__ feat;
    const double* __restrict__ pixf;
    const double* __restrict__ gimg;
    float f[MC];
    double q[MC];
    __device__ bool stage(int t, size_t px, const RnPix& rec) {
      double g[MC];
      bool any = false;
#pragma unroll
      for (int c = 0; c < MC; ++c) {
        g[c] = c < C ? gimg[px * C + c] : 0.0;
        any = any || g[c] != 0.0;
      }
      if (!(rec.W > 0.0 && any)) return false;
      double b = 0.0;
#pragma unroll
      for (int c = 0; c < MC; ++c)
        if (c < C) {
          sa[c][t] = g[c] / rec.W;
          b = fma(g[c], pixf[px * C + c], b);
        }
      sb[t] = b / rec.W;
      return true;
    }
    __device__ void entry(int id) {
      const float4* fr = reinterpret_cast<const float4*>(feat + (size_t)id * CP);
      const float4 v0 = fr[0], v1 = CP > 4 ? fr[1] : make_float4(0.f, 0.f, 0.f, 0.f);
      f[0] = v0.x; f[1] = v0.y; f[2] = v0.z; f[3] = v0.w;
      f[4] = v1.x; f[5] = v1.y; f[6] = v1.z; f[7] = v1.w;
#pragma unroll
      for (int c = 0; c < MC; ++c) q[c] = 0.0;
    }
    __device__ double sk(int t) const {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < MC; ++c)
        if (c < C) s = fma(sa[c][t], (double)f[c], s);
      return s - sb[t];
    }
    __device__ void add(int t, double wk) {
      if (GC) {
#pragma unroll
        for (int c = 0; c < MC; ++c)
          if (c < C) q[c] = fma(sa[c][t], wk, q[c]);
      }
    }
    __device__ void store(double* o) const {
      if (GC) {
#pragma unroll
        for (int c = 0; c < MC; ++c)
          if (c < C) o[c] = q[c];
      }
    }
  };
  rn_bwd_tile<PR>(cam, off, keys, pos, box, pix, slab, S, GP, GR, Val{C, CP, GC, feat, pixf, gimg});
}

// Backward, pass 2: f(at) for the position `at` of point i's entry in the sorted list of every tile its box touches, in the
// scatter's tile order.  Nothing for a culled point (or an unstable surfel).
template <typename F>
__device__ __forceinline__ void rn_point_entries(int i, int tiles_x, const unsigned long long* __restrict__ off,
                                                 const unsigned long long* __restrict__ keys, const float4* __restrict__ pos,
                                                 const int4* __restrict__ box, F f) {
  const int4 b = box[i];
  if (b.x > b.y) return;
  const unsigned long long key = rn_key(pos, i);
  for (int ty = b.z / RN_TILE; ty <= b.w / RN_TILE; ++ty)
    for (int tx = b.x / RN_TILE; tx <= b.y / RN_TILE; ++tx) {
      const unsigned long long at = rn_find(off, keys, ty * tiles_x + tx, key);
      if (at != RN_ABSENT) f(at);
    }
}

// pass 2 after a three-channel forward: per point, the sums of its slab entries' S doubles -- dL/dP (3, RN_BWD_POINTS),
// dL/dc (3, RN_BWD_COLORS), dL/dr (1, RN_BWD_RADII), in that order; an output that is NULL is not written.
template <int MODE>
__global__ void __launch_bounds__(256) k_rn_bwd_point_ex(int N, int tiles_x, const unsigned long long* __restrict__ off,
                                                         const unsigned long long* __restrict__ keys, const float4* __restrict__ pos,
                                                         const int4* __restrict__ box, const double* __restrict__ slab,
                                                         double* __restrict__ out_p, double* __restrict__ out_c,
                                                         double* __restrict__ out_r) {
  constexpr int OC = (MODE & RN_BWD_POINTS) ? 3 : 0;
  constexpr int S = OC + ((MODE & RN_BWD_COLORS) ? 3 : 0) + ((MODE & RN_BWD_RADII) ? 1 : 0);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double g[S];
  for (int q = 0; q < S; ++q) g[q] = 0.0;
  rn_point_entries(i, tiles_x, off, keys, pos, box, [&](unsigned long long at) {
    for (int q = 0; q < S; ++q) g[q] += slab[S * at + q];
  });
  if constexpr ((MODE & RN_BWD_POINTS) != 0) {
    if (out_p)
      for (int q = 0; q < 3; ++q) out_p[3 * (size_t)i + q] = g[q];
  }
  if constexpr ((MODE & RN_BWD_COLORS) != 0) {
    if (out_c)
      for (int q = 0; q < 3; ++q) out_c[3 * (size_t)i + q] = g[OC + q];
  }
  if constexpr ((MODE & RN_BWD_RADII) != 0) {
    if (out_r) out_r[i] = g[S - 1];
  }
}

// pass 2 for the point gradient alone (slm_render_backward, every GraphFit render-loss step): k_rn_bwd_point_ex<RN_BWD_POINTS>
// without the two unused outputs.  Kept beside it because that instantiation, on the same search, has the same 26 VGPRs and no
// scratch but 152 instructions against the 142 here (it clears its sums as six 32-bit moves per site and tests out_p).
__global__ void __launch_bounds__(256) k_rn_bwd_point(int N, int tiles_x, const unsigned long long* __restrict__ off,
                                                      const unsigned long long* __restrict__ keys, const float4* __restrict__ pos,
                                                      const int4* __restrict__ box, const double* __restrict__ slab,
                                                      double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  rn_point_entries(i, tiles_x, off, keys, pos, box, [&](unsigned long long at) {
    gx += slab[3 * at];
    gy += slab[3 * at + 1];
    gz += slab[3 * at + 2];
  });
  out[3 * (size_t)i] = gx;
  out[3 * (size_t)i + 1] = gy;
  out[3 * (size_t)i + 2] = gz;
}

// pass 2 after a channels forward: the same sums with the run-time slab layout of k_rn_bwd_entry_ch
__global__ void __launch_bounds__(256) k_rn_bwd_point_ch(int N, int tiles_x, int C, const unsigned long long* __restrict__ off,
                                                         const unsigned long long* __restrict__ keys,
                                                         const float4* __restrict__ pos, const int4* __restrict__ box,
                                                         const double* __restrict__ slab, double* __restrict__ out_p,
                                                         double* __restrict__ out_f, double* __restrict__ out_r) {
  constexpr int MC = SLM_RENDER_MAX_CHANNELS;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int of = out_p ? 3 : 0, S = of + (out_f ? C : 0) + (out_r ? 1 : 0);
  double ap[3] = {0.0, 0.0, 0.0}, ar = 0.0, af[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) af[c] = 0.0;
  rn_point_entries(i, tiles_x, off, keys, pos, box, [&](unsigned long long at) {
    const double* e = slab + (size_t)S * at;
    if (out_p) {
      ap[0] += e[0];
      ap[1] += e[1];
      ap[2] += e[2];
    }
    if (out_f) {
#pragma unroll
      for (int c = 0; c < MC; ++c)
        if (c < C) af[c] += e[of + c];
    }
    if (out_r) ar += e[S - 1];
  });
  if (out_p)
    for (int q = 0; q < 3; ++q) out_p[3 * (size_t)i + q] = ap[q];
  if (out_f) {
#pragma unroll
    for (int c = 0; c < MC; ++c)
      if (c < C) out_f[(size_t)C * i + c] = af[c];
  }
  if (out_r) out_r[i] = ar;
}

// the device arrays of a context; sizes of slm_render_create: [0] points + 1, [1] tiles, [2] tiles + 1, [3] pixels, [4] 1
#define A(name, mult, unit) DEV_MEMBER(slm_render, name, mult, unit)
constexpr DevMember kRenderArrays[] = {A(pos, 1, 0), A(box, 1, 0), A(cnt, 1, 1), A(off, 1, 2), A(cur, 1, 1), A(col, 1, 0),
                                       A(pix, 1, 3), A(stat, 3, 4), DEV_GROWN(slm_render, keys), DEV_GROWN(slm_render, tmp),
                                       DEV_GROWN(slm_render, slab), DEV_GROWN(slm_render, feat), DEV_GROWN(slm_render, pixf)};
#undef A

int rn_tiles_x(int w) { return (w + RN_TILE - 1) / RN_TILE; }

RnCam rn_cam(const slm_render_params* p) {
  RnCam cam;
  cam.w = p->width;
  cam.h = p->height;
  cam.tiles_x = rn_tiles_x(p->width);
  cam.n_track = p->n_track;
  cam.f = p->focal;
  cam.ccx = p->ccx;
  cam.ccy = p->ccy;
  cam.r = p->radius;
  cam.zn = p->z_near;
  cam.zf = p->z_far;
  cam.gamma = p->gamma;
  cam.eps = p->bg_eps;
  cam.bg0 = p->bg[0];
  cam.bg1 = p->bg[1];
  cam.bg2 = p->bg[2];
  return cam;
}

// the parameters a backward must repeat: those of its forward, field by field (pad excluded); a channels forward does
// not read bg, so its backward does not compare it
bool rn_same_geometry(const slm_render_params& a, const slm_render_params& b) {
  return a.width == b.width && a.height == b.height && a.n_track == b.n_track && a.points_f64 == b.points_f64 &&
         a.focal == b.focal && a.ccx == b.ccx && a.ccy == b.ccy && a.radius == b.radius && a.z_near == b.z_near &&
         a.z_far == b.z_far && a.gamma == b.gamma && a.bg_eps == b.bg_eps;
}
bool rn_same_params(const slm_render_params& a, const slm_render_params& b) {
  return rn_same_geometry(a, b) && a.bg[0] == b.bg[0] && a.bg[1] == b.bg[1] && a.bg[2] == b.bg[2];
}

// the padded row width of the context's feature copy
int rn_padded(int C) { return C <= 4 ? 4 : 8; }

// Every instantiation of a kernel family, indexed by the run-time choices it was compiled for, so that each family is launched
// from one place.  A MODE with RN_BWD_RADII exists only with PR (the entry points refuse grad_radii after a one-radius
// forward): those slots of the PR = false row stay null and are never instantiated.
constexpr decltype(&k_rn_project<0, false>) kProject[3][2] = {   // [SRC][PR]
    {k_rn_project<RN_SRC_F32, false>, k_rn_project<RN_SRC_F32, true>},
    {k_rn_project<RN_SRC_F64, false>, k_rn_project<RN_SRC_F64, true>},
    {k_rn_project<RN_SRC_GF, false>, k_rn_project<RN_SRC_GF, true>}};
constexpr decltype(&k_rn_tile<false>) kTile[2] = {k_rn_tile<false>, k_rn_tile<true>};   // [PR]
constexpr decltype(&k_rn_tile_ch<false, 4>) kTileCh[2][2] = {                            // [CP == 8][PR]
    {k_rn_tile_ch<false, 4>, k_rn_tile_ch<true, 4>}, {k_rn_tile_ch<false, 8>, k_rn_tile_ch<true, 8>}};
constexpr decltype(&k_rn_bwd_entry<1, false>) kBwdEntry[2][8] = {                        // [PR][MODE]
    {nullptr, k_rn_bwd_entry<1, false>, k_rn_bwd_entry<2, false>, k_rn_bwd_entry<3, false>},
    {nullptr, k_rn_bwd_entry<1, true>, k_rn_bwd_entry<2, true>, k_rn_bwd_entry<3, true>, k_rn_bwd_entry<4, true>,
     k_rn_bwd_entry<5, true>, k_rn_bwd_entry<6, true>, k_rn_bwd_entry<7, true>}};
constexpr decltype(&k_rn_bwd_point_ex<2>) kBwdPoint[8] = {                               // [MODE]; 1 is k_rn_bwd_point
    nullptr, nullptr, k_rn_bwd_point_ex<2>, k_rn_bwd_point_ex<3>, k_rn_bwd_point_ex<4>,
    k_rn_bwd_point_ex<5>, k_rn_bwd_point_ex<6>, k_rn_bwd_point_ex<7>};
constexpr decltype(&k_rn_bwd_entry_ch<false>) kBwdEntryCh[2] = {k_rn_bwd_entry_ch<false>, k_rn_bwd_entry_ch<true>};   // [PR]

// one forward, as its entry point describes it
struct RnForward {
  const char* who;       // the entry point's name, for its refusals
  int src;               // RN_SRC_F32 / F64: N rows of `pts`;  RN_SRC_GF: the N surfels of `gslot`
  const void* pts;
  GfSlot* gslot;
  int N;
  bool per_point;        // radii (N) float32 device holds one radius per point (by surfel row for RN_SRC_GF); else p->radius
  const float* radii;
  const float* values;   // the colours (ch = 0) or the features, rows of `stride` floats
  int stride;
  int ch;                // 0: the three colour channels and p->bg;  1..8: that many channels and the host floats `bg`
  const float* bg;
  float* image;
  int32_t *front_id, *hit_count;
  void* stream;
};

// the refusals of a forward on the parameters and the point count, in their order (r and p not null)
int rn_check_params(const std::string& w, const slm_render* r, const slm_render_params* p, int N) {
  if (p->width < 1 || p->height < 1 || p->width > r->W || p->height > r->H)
    return fail(SLM_ERR_INVALID, w + ": image size outside the context's H x W");
  if (p->n_track < 1 || p->n_track > SLM_RENDER_MAX_TRACK) return fail(SLM_ERR_INVALID, w + ": n_track must be 1..64");
  if (!(p->focal > 0.0) || !(p->radius > 0.0) || !(p->gamma > 0.0) || !(p->z_near > 0.0) || !(p->z_far > p->z_near) ||
      !std::isfinite(p->focal) || !std::isfinite(p->ccx) || !std::isfinite(p->ccy) || !std::isfinite(p->z_far) ||
      !std::isfinite(p->radius) || !std::isfinite(p->bg_eps))
    return fail(SLM_ERR_INVALID, w + ": bad camera or blend parameters");
  if (N < 0 || N > r->cap) return fail(SLM_ERR_INVALID, w + ": more points than the context holds");
  return SLM_OK;
}

int render_common(slm_render* r, const slm_render_params* p, const RnForward& f) {
  const std::string w(f.who);
  const int N = f.N, ch = f.ch;
  if (!r || !p || !f.image) return fail(SLM_ERR_INVALID, w + ": null argument");
  if (const int rc = rn_check_params(w, r, p, N)) return rc;
  if (ch && N > 0 && !f.pts) return fail(SLM_ERR_INVALID, w + ": null points");
  if (!ch && N > 0 && ((f.src != RN_SRC_GF && !f.pts) || !f.values || f.stride < 3))
    return fail(SLM_ERR_INVALID, w + ": null points / colours or color_stride < 3");
  r->has_fwd = 0;
  hipStream_t st = (hipStream_t)f.stream;
  const RnCam cam = rn_cam(p);
  const int tiles_y = (p->height + RN_TILE - 1) / RN_TILE, tiles = cam.tiles_x * tiles_y;
  const int CP = rn_padded(ch);
  const float* colors = f.values;
  int cstride = f.stride;
  RnBg bg{};
  if (ch) {   // the wider buffers, first needed here: the feature copy at its widest, the pixel record at this width
    const size_t rows = (size_t)r->cap + 1, pixels = (size_t)r->H * r->W;
    HIPCHK(grow(r->feat, r->cap_feat, rows * CP, rows * SLM_RENDER_MAX_CHANNELS));
    HIPCHK(grow(r->pixf, r->cap_pixf, pixels * ch, pixels * ch));
    for (int c = 0; c < ch; ++c) bg.v[c] = f.bg[c];
    if (N > 0) {
      const size_t cells = (size_t)N * CP;
      hipLaunchKernelGGL(k_rn_feat, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, N, ch, CP, colors, cstride,
                         r->feat);
      colors = r->feat;   // k_rn_project copies its first three columns into col, which nothing reads after this forward
      cstride = CP;
    }
  }
  HIPCHK(hipMemsetAsync(r->cnt, 0, sizeof(unsigned int) * tiles, st));
  const dim3 gp((N + 255) / 256), gt(cam.tiles_x, tiles_y);
  if (N > 0)
    hipLaunchKernelGGL(kProject[f.src][f.per_point], gp, dim3(256), 0, st, N, f.pts, f.gslot, cam, r->pos, r->box, r->cnt,
                       colors, cstride, r->col, f.radii);
  hipLaunchKernelGGL(k_rn_scan, dim3(1), dim3(1024), 0, st, tiles, r->cnt, r->off, r->cur, 0ull, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(r->h_total, r->off + tiles, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const unsigned long long total = *r->h_total;
  if (total > (1ull << 31)) return fail(SLM_ERR_UNSUPPORTED, w + ": more than 2^31 tile entries");
  const size_t want = (size_t)total + total / 4 + 1024;   // (head-room of the tile lists; the slab's follows it)
  HIPCHK(grow(r->keys, r->cap_keys, total, want));
  HIPCHK(grow(r->tmp, r->cap_tmp, total, want));
  if (total > 0)
    hipLaunchKernelGGL(k_rn_scatter, gp, dim3(256), 0, st, N, cam.tiles_x, r->pos, r->box, r->cur, r->keys, nullptr, 0ull);
  if (ch)
    hipLaunchKernelGGL(kTileCh[CP == 8][f.per_point], gt, dim3(256), 0, st, cam, bg, ch, r->off, r->keys, r->tmp, r->pos,
                       r->box, r->feat, f.image, f.front_id, f.hit_count, r->pix, r->pixf);
  else
    hipLaunchKernelGGL(kTile[f.per_point], gt, dim3(256), 0, st, cam, r->off, r->keys, r->tmp, r->pos, r->box, colors,
                       cstride, f.image, f.front_id, f.hit_count, r->pix);
  HIPCHK(hipGetLastError());
  r->last = *p;
  r->per_point_last = f.per_point;
  r->ch_last = ch;
  r->n_last = N;
  r->total_last = total;
  r->has_fwd = 1;
  return SLM_OK;
}

// The refusals that every backward entry point `who` shares, in their order.  C = 0: the entry follows a three-channel
// forward, else a channels forward of C channels (which does not read bg, so bg is not compared).  grad_radii: null where the
// entry has none.
int rn_bwd_check(const char* who, int C, bool channels, const slm_render* r, const slm_render_params* p,
                 const double* grad_image, const double* grad_radii) {
  const std::string w(who);
  if (!r || !p || !grad_image) return fail(SLM_ERR_INVALID, w + ": null argument");
  if (channels && (C < 1 || C > SLM_RENDER_MAX_CHANNELS)) return fail(SLM_ERR_INVALID, w + ": channels must be 1..8");
  if (!r->has_fwd) return fail(SLM_ERR_INVALID, w + ": no completed forward on this context");
  if (!channels && r->ch_last)
    return fail(SLM_ERR_INVALID, w + ": the last forward had N-channel features: use slm_render_backward_channels");
  if (channels && !r->ch_last) return fail(SLM_ERR_INVALID, w + ": the last forward was not slm_render_points_channels");
  if (channels && r->ch_last != C) return fail(SLM_ERR_INVALID, w + ": channels differ from those of the last forward");
  if (!(channels ? rn_same_geometry(*p, r->last) : rn_same_params(*p, r->last)))
    return fail(SLM_ERR_INVALID, w + ": parameters differ from those of the last forward");
  if (grad_radii && !r->per_point_last) return fail(SLM_ERR_INVALID, w + ": grad_radii after a forward with one radius");
  return SLM_OK;
}

// The backward of the last forward on r (checked by the caller; N > 0, one output at least; grad_radii only after a per-point
// forward), C = 0 after a three-channel forward.  The slab holds per tile-list entry 3 doubles for the points, 3 (or C) for
// the values and 1 for the radii, those that are wanted, with the head-room of the tile lists.
int rn_backward(slm_render* r, const slm_render_params* p, int C, const double* grad_image, double* grad_points,
                double* grad_values, double* grad_radii, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const RnCam cam = rn_cam(p);
  const int N = r->n_last, pr = r->per_point_last;
  const int want = (grad_points ? RN_BWD_POINTS : 0) | (grad_values ? RN_BWD_COLORS : 0) | (grad_radii ? RN_BWD_RADII : 0);
  const size_t S = (grad_points ? 3 : 0) + (grad_values ? (C ? C : 3) : 0) + (grad_radii ? 1 : 0);
  const unsigned long long total = r->total_last;
  HIPCHK(grow(r->slab, r->cap_slab, S * total, S * ((size_t)total + total / 4 + 1024)));
  const dim3 gt(cam.tiles_x, (p->height + RN_TILE - 1) / RN_TILE), gp((N + 255) / 256), b(256);
  if (C) {
    if (total > 0)
      hipLaunchKernelGGL(kBwdEntryCh[pr], gt, b, 0, st, cam, C, rn_padded(C), want, r->off, r->keys, r->pos, r->box, r->feat,
                         r->pix, r->pixf, grad_image, r->slab);
    hipLaunchKernelGGL(k_rn_bwd_point_ch, gp, b, 0, st, N, cam.tiles_x, C, r->off, r->keys, r->pos, r->box, r->slab,
                       grad_points, grad_values, grad_radii);
  } else {
    if (total > 0)
      hipLaunchKernelGGL(kBwdEntry[pr][want], gt, b, 0, st, cam, r->off, r->keys, r->pos, r->box, r->col, r->pix, grad_image,
                         r->slab);
    if (want == RN_BWD_POINTS)
      hipLaunchKernelGGL(k_rn_bwd_point, gp, b, 0, st, N, cam.tiles_x, r->off, r->keys, r->pos, r->box, r->slab, grad_points);
    else
      hipLaunchKernelGGL(kBwdPoint[want], gp, b, 0, st, N, cam.tiles_x, r->off, r->keys, r->pos, r->box, r->slab, grad_points,
                         grad_values, grad_radii);
  }
  HIPCHK(hipGetLastError());
  return SLM_OK;
}

}  // namespace

// ---- the render loss inside slm_gf_run (slm_gf.hip; declared in slm_gf.h) ---------------------------------------------------
// rn_gf_size at the bind, then per evaluation rn_gf_forward and rn_gf_backward, which only enqueue: the lists' capacity is the
// entry limit fixed here, and k_rn_scan's guard keeps every render inside it.

int rn_gf_check(const char* who, const slm_render* r, const slm_render_params* p, int N, const float* colors, int cstride) {
  const std::string w(who);
  if (const int rc = rn_check_params(w, r, p, N)) return rc;
  if (N > 0 && (!colors || cstride < 3)) return fail(SLM_ERR_INVALID, w + ": null points / colours or color_stride < 3");
  return SLM_OK;
}

// One render of the slot's current state through render_common (one synchronisation) sizes the lists and the slab (3 doubles
// per entry) with the usual head-room; entry_limit > 0 replaces the logical limit, and the buffers hold at least that too.
// Clears the status record and enters the sizing render's total as the largest seen.
int rn_gf_size(const char* who, slm_render* r, const slm_render_params* p, GfSlot* gslot, int N, const float* radii,
               const float* colors, int cstride, float* image, int64_t entry_limit, unsigned long long* limit_out,
               void* stream) {
  const int rc = render_common(r, p, {who, RN_SRC_GF, nullptr, gslot, N, radii != nullptr, radii, colors, cstride, 0, nullptr,
                                      image, nullptr, nullptr, stream});
  if (rc != SLM_OK) return rc;
  const unsigned long long total = r->total_last;
  const size_t sized = (size_t)total + total / 4 + 1024;
  const size_t limit = entry_limit > 0 ? (size_t)entry_limit : sized, want = limit > sized ? limit : sized;
  HIPCHK(grow(r->keys, r->cap_keys, want, want));
  HIPCHK(grow(r->tmp, r->cap_tmp, want, want));
  HIPCHK(grow(r->slab, r->cap_slab, 3 * want, 3 * want));
  const unsigned long long stat[3] = {0, total, total};
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(r->stat, stat, sizeof(stat), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  r->has_fwd = 0;   // the guarded forwards leave no host-side record: a backward entry point refuses until the next forward
  *limit_out = limit;
  return SLM_OK;
}

// render_common's launches for the surfels of `gslot`, three colour channels, with the guard in place of the read-back
void rn_gf_forward(slm_render* r, const slm_render_params* p, GfSlot* gslot, int N, const float* radii, const float* colors,
                   int cstride, float* image, unsigned long long limit, hipStream_t st) {
  const RnCam cam = rn_cam(p);
  const int tiles_y = (p->height + RN_TILE - 1) / RN_TILE, tiles = cam.tiles_x * tiles_y, pr = radii != nullptr;
  r->has_fwd = 0;
  (void)hipMemsetAsync(r->cnt, 0, sizeof(unsigned int) * tiles, st);
  const dim3 gp((N + 255) / 256), gt(cam.tiles_x, tiles_y);
  if (N > 0)
    hipLaunchKernelGGL(kProject[RN_SRC_GF][pr], gp, dim3(256), 0, st, N, nullptr, gslot, cam, r->pos, r->box, r->cnt, colors,
                       cstride, r->col, radii);
  hipLaunchKernelGGL(k_rn_scan, dim3(1), dim3(1024), 0, st, tiles, r->cnt, r->off, r->cur, limit, r->stat);
  if (N > 0)
    hipLaunchKernelGGL(k_rn_scatter, gp, dim3(256), 0, st, N, cam.tiles_x, r->pos, r->box, r->cur, r->keys, r->stat + 2, limit);
  hipLaunchKernelGGL(kTile[pr], gt, dim3(256), 0, st, cam, r->off, r->keys, r->tmp, r->pos, r->box, colors, cstride, image,
                     nullptr, nullptr, r->pix);
}

// rn_backward's launches for the point gradient of the last rn_gf_forward (N > 0)
void rn_gf_backward(slm_render* r, const slm_render_params* p, int N, bool per_point, const double* grad_image,
                    double* grad_points, hipStream_t st) {
  const RnCam cam = rn_cam(p);
  const dim3 gt(cam.tiles_x, (p->height + RN_TILE - 1) / RN_TILE), gp((N + 255) / 256), b(256);
  hipLaunchKernelGGL(kBwdEntry[per_point][RN_BWD_POINTS], gt, b, 0, st, cam, r->off, r->keys, r->pos, r->box, r->col, r->pix,
                     grad_image, r->slab);
  hipLaunchKernelGGL(k_rn_bwd_point, gp, b, 0, st, N, cam.tiles_x, r->off, r->keys, r->pos, r->box, r->slab, grad_points);
}

// {renders over their limit, largest total} since rn_gf_size, copied to the host on `st` (the caller synchronises)
hipError_t rn_gf_status(const slm_render* r, unsigned long long out_host[2], hipStream_t st) {
  return hipMemcpyAsync(out_host, r->stat, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
}

extern "C" {

int slm_render_create(int32_t H, int32_t W, int32_t max_points, slm_render** out) {
  if (!out || H < 1 || W < 1 || max_points < 0) return fail(SLM_ERR_INVALID, "slm_render_create: bad argument");
  if (slm_device_count() < 1) return fail(SLM_ERR_NO_DEVICE, "slm_render_create: no HIP device visible");
  slm_render* r = new slm_render();
  r->H = H;
  r->W = W;
  r->cap = max_points;
  const size_t cap = (size_t)max_points + 1, tiles = (size_t)rn_tiles_x(W) * ((H + RN_TILE - 1) / RN_TILE);
  const size_t units[] = {cap, tiles, tiles + 1, (size_t)H * W, 1};
  hipError_t e = alloc_members(r, kRenderArrays, units);
  if (e == hipSuccess) e = hipHostMalloc((void**)&r->h_total, sizeof(unsigned long long), hipHostMallocDefault);
  if (e != hipSuccess) {
    slm_render_destroy(r);
    return fail(SLM_ERR_HIP, std::string("slm_render_create: ") + hipGetErrorString(e));
  }
  *out = r;
  return SLM_OK;
}

int slm_render_destroy(slm_render* r) {
  if (!r) return SLM_OK;
  free_members(r, kRenderArrays);
  if (r->h_total) (void)hipHostFree(r->h_total);
  delete r;
  return SLM_OK;
}

int slm_render_points(slm_render* r, const slm_render_params* p, int32_t N, const void* points, const float* colors,
                      int32_t color_stride, float* image, int32_t* front_id, int32_t* hit_count, void* stream) {
  if (!p) return fail(SLM_ERR_INVALID, "slm_render_points: null argument");
  return render_common(r, p, {"slm_render_points", p->points_f64 ? RN_SRC_F64 : RN_SRC_F32, points, nullptr, N, false, nullptr,
                              colors, color_stride, 0, nullptr, image, front_id, hit_count, stream});
}

int slm_render_points_radii(slm_render* r, const slm_render_params* p, int32_t N, const void* points, const float* radii,
                            const float* colors, int32_t color_stride, float* image, int32_t* front_id,
                            int32_t* hit_count, void* stream) {
  if (!r || !p || !image) return fail(SLM_ERR_INVALID, "slm_render_points_radii: null argument");
  if (N > 0 && !radii) return fail(SLM_ERR_INVALID, "slm_render_points_radii: null radii");
  return render_common(r, p, {"slm_render_points_radii", p->points_f64 ? RN_SRC_F64 : RN_SRC_F32, points, nullptr, N, true,
                              radii, colors, color_stride, 0, nullptr, image, front_id, hit_count, stream});
}

int slm_gf_render(slm_gf* g, int32_t slot, slm_render* r, const slm_render_params* p, const float* colors,
                  int32_t color_stride, float* image, int32_t* front_id, int32_t* hit_count, void* stream) {
  GfSlot* dev = nullptr;
  int32_t n = 0;
  const int rc = gf_render_slot(g, slot, &dev, &n);
  if (rc != SLM_OK) return rc;
  return render_common(r, p, {"slm_gf_render", RN_SRC_GF, nullptr, dev, n, false, nullptr, colors, color_stride, 0, nullptr,
                              image, front_id, hit_count, stream});
}

int slm_gf_render_radii(slm_gf* g, int32_t slot, slm_render* r, const slm_render_params* p, const float* radii,
                        const float* colors, int32_t color_stride, float* image, int32_t* front_id, int32_t* hit_count,
                        void* stream) {
  if (!g || !r || !p || !image) return fail(SLM_ERR_INVALID, "slm_gf_render_radii: null argument");
  if (!radii) return fail(SLM_ERR_INVALID, "slm_gf_render_radii: null radii");
  GfSlot* dev = nullptr;
  int32_t n = 0;
  const int rc = gf_render_slot(g, slot, &dev, &n, "slm_gf_render_radii");
  if (rc != SLM_OK) return rc;
  return render_common(r, p, {"slm_gf_render_radii", RN_SRC_GF, nullptr, dev, n, true, radii, colors, color_stride, 0, nullptr,
                              image, front_id, hit_count, stream});
}

int slm_render_points_channels(slm_render* r, const slm_render_params* p, int32_t N, const void* points, const float* radii,
                               int32_t C, const float* features, int32_t feature_stride, const float* bg, float* image,
                               int32_t* front_id, int32_t* hit_count, void* stream) {
  if (!r || !p || !image || !bg) return fail(SLM_ERR_INVALID, "slm_render_points_channels: null argument");
  if (C < 1 || C > SLM_RENDER_MAX_CHANNELS) return fail(SLM_ERR_INVALID, "slm_render_points_channels: channels must be 1..8");
  if (feature_stride < C) return fail(SLM_ERR_INVALID, "slm_render_points_channels: feature_stride < channels");
  if (N > 0 && !features) return fail(SLM_ERR_INVALID, "slm_render_points_channels: null features");
  return render_common(r, p, {"slm_render_points_channels", p->points_f64 ? RN_SRC_F64 : RN_SRC_F32, points, nullptr, N,
                              radii != nullptr, radii, features, feature_stride, C, bg, image, front_id, hit_count, stream});
}

int slm_render_backward(slm_render* r, const slm_render_params* p, const double* grad_image, double* grad_points,
                        void* stream) {
  if (const int rc = rn_bwd_check("slm_render_backward", 0, false, r, p, grad_image, nullptr)) return rc;
  if (r->n_last == 0) return SLM_OK;
  if (!grad_points) return fail(SLM_ERR_INVALID, "slm_render_backward: null grad_points");
  return rn_backward(r, p, 0, grad_image, grad_points, nullptr, nullptr, stream);
}

int slm_render_backward_ex(slm_render* r, const slm_render_params* p, const double* grad_image, double* grad_points,
                           double* grad_colors, void* stream) {
  if (const int rc = rn_bwd_check("slm_render_backward_ex", 0, false, r, p, grad_image, nullptr)) return rc;
  if (r->n_last == 0) return SLM_OK;
  if (!grad_points && !grad_colors) return fail(SLM_ERR_INVALID, "slm_render_backward_ex: null grad_points and grad_colors");
  return rn_backward(r, p, 0, grad_image, grad_points, grad_colors, nullptr, stream);
}

int slm_render_backward_radii(slm_render* r, const slm_render_params* p, const double* grad_image, double* grad_points,
                              double* grad_colors, double* grad_radii, void* stream) {
  if (const int rc = rn_bwd_check("slm_render_backward_radii", 0, false, r, p, grad_image, grad_radii)) return rc;
  if (r->n_last == 0) return SLM_OK;
  if (!grad_points && !grad_colors && !grad_radii)
    return fail(SLM_ERR_INVALID, "slm_render_backward_radii: null grad_points, grad_colors and grad_radii");
  return rn_backward(r, p, 0, grad_image, grad_points, grad_colors, grad_radii, stream);
}

int slm_render_backward_channels(slm_render* r, const slm_render_params* p, int32_t C, const double* grad_image,
                                 double* grad_points, double* grad_features, double* grad_radii, void* stream) {
  if (const int rc = rn_bwd_check("slm_render_backward_channels", C, true, r, p, grad_image, grad_radii)) return rc;
  if (r->n_last == 0) return SLM_OK;
  if (!grad_points && !grad_features && !grad_radii)
    return fail(SLM_ERR_INVALID, "slm_render_backward_channels: null grad_points, grad_features and grad_radii");
  return rn_backward(r, p, C, grad_image, grad_points, grad_features, grad_radii, stream);
}

}  // extern "C"
