// Host-only harness around the symbolic analysis (python-super_amd/csrc/slm_nd_host.hip): builds the plan of a coupling
// graph handed over by tools/studies/nd_order_study.py and returns its cost figures.  Study tool, not part of the library --
// but a TEST DEPENDENCY: tests/test_nd_host_sanitized.py (nd_stats, nd_check_*) and tests/solver_graph_cases.py (nd_node_fronts)
// build this file with slm_nd_host.hip for the host and call it through ctypes; keep those entry points' signatures.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "slm_nd.h"

// Is a task list a valid order for the ticket scheduler of slm_dag.hip (a task only waits for EARLIER tasks)?  Checks, per
// front: POTRF(s) behind POTRF(s-1); POTRF(s) behind the producers of L(s,c) and L(s-1,c), c <= s-2; COL(r,s) behind POTRF(s)
// and behind the producers of L(r,c), L(s,c), c < s; SCHUR(r,sc) behind the producers of L(r,c), L(sc,c), c < npt; a front's
// first task behind the SCHUR tasks of its children; BACK / BACKB behind the front's POTRF tasks and its parent's BACK.
// The producer of tile (r,c), c < npt, r > c: POTRF(r) when r == c + 1 < npt (it owns the tile left of its diagonal one),
// else COL(r,c).  Returns 0, or the 1-based index of the first task that precedes something it waits for.
static int check_order(const NDPlanHost& p, const std::vector<int32_t>& list, bool top_only) {
  const int T = (int)p.fronts.size();
  const size_t n = list.size() / 2;
  std::vector<std::vector<long>> potrf(T), col(T), schur(T);
  std::vector<long> back(T, -1), first(T, -1);
  auto key = [](int r, int s, int nt) { return (size_t)r * nt + s; };
  for (int i = 0; i < T; ++i) {
    const NDFront& f = p.fronts[i];
    potrf[i].assign(f.npt > 0 ? f.npt : 1, -1);
    col[i].assign((size_t)f.nt * f.nt + 1, -1);
    schur[i].assign((size_t)f.nt * f.nt + 1, -1);
  }
  for (size_t k = 0; k < n; ++k) {
    const int type = list[2 * k] >> 24, fi = list[2 * k] & 0xFFFFFF, r = list[2 * k + 1] >> 8, s = list[2 * k + 1] & 255;
    if (fi < 0 || fi >= T) return (int)k + 1;
    const NDFront& f = p.fronts[fi];
    if (first[fi] < 0 && type <= ND_T_SCHUR) first[fi] = (long)k;
    if (type == ND_T_POTRF) potrf[fi][s] = (long)k;
    else if (type == ND_T_COL) col[fi][key(r, s, f.nt)] = (long)k;
    else if (type == ND_T_SCHUR) schur[fi][key(r, s, f.nt)] = (long)k;
    else if (type == ND_T_BACK) back[fi] = (long)k;
  }
  auto producer = [&](int fi, int r, int c) -> long {
    const NDFront& f = p.fronts[fi];
    return (r == c + 1 && r < f.npt) ? potrf[fi][r] : col[fi][key(r, c, f.nt)];
  };
  for (size_t k = 0; k < n; ++k) {
    const int type = list[2 * k] >> 24, fi = list[2 * k] & 0xFFFFFF, r = list[2 * k + 1] >> 8, s = list[2 * k + 1] & 255;
    const NDFront& f = p.fronts[fi];
    const bool listed = !top_only || f.depth <= p.dag_cut_depth;    // (a top list holds no factor tasks of the deeper fronts)
    auto before = [&](long dep) { return dep >= 0 && dep < (long)k; };
    if (type == ND_T_POTRF) {
      if (s > 0 && !before(potrf[fi][s - 1])) return (int)k + 1;
      for (int c = 0; c + 1 < s; ++c)
        if (!before(producer(fi, s, c)) || !before(producer(fi, s - 1, c))) return (int)k + 1;
    } else if (type == ND_T_COL) {
      if (!before(potrf[fi][s])) return (int)k + 1;
      for (int c = 0; c < s; ++c)
        if (!before(producer(fi, r, c)) || !before(producer(fi, s, c))) return (int)k + 1;
    } else if (type == ND_T_SCHUR) {
      for (int c = 0; c < f.npt; ++c)
        if (!before(producer(fi, r, c)) || (s != r && !before(producer(fi, s, c)))) return (int)k + 1;
      if (f.npt > 0 && !before(potrf[fi][f.npt - 1])) return (int)k + 1;
    } else if (type == ND_T_BACK || type == ND_T_BACKB) {
      if (listed)
        for (int c = 0; c < f.npt; ++c)
          if (!before(potrf[fi][c])) return (int)k + 1;
      if (f.parent >= 0 && !before(back[f.parent])) return (int)k + 1;
    }
    if (type <= ND_T_SCHUR && (long)k == first[fi])
      for (int kid = 0; kid < 2; ++kid) {
        const int ch = p.front_kids[2 * (size_t)fi + kid];
        if (ch < 0) continue;
        if (top_only && p.fronts[ch].depth > p.dag_cut_depth) continue;   // factored by the per-level launches before the list runs
        for (long q : schur[ch])
          if (q >= (long)k) return (int)k + 1;
        for (long q : potrf[ch])
          if (p.fronts[ch].npt > 0 && !before(q)) return (int)k + 1;
      }
  }
  return 0;
}

// 0: both task lists of the plan are valid ticket orders; else 1000000 * list + the offending task's 1-based index
extern "C" int nd_check_orders(int J, int K_ED, const float* pts, const int32_t* knn, const uint32_t* pairs, int n_pairs) {
  NDPlanHost p;
  if (!nd_build_plan(J, K_ED, pts, knn, pairs, n_pairs, p)) return -1;
  const int a = check_order(p, p.dag_tasks, false);
  if (a) return 1000000 + a;
  const int b = p.dag_top_tasks.empty() ? 0 : check_order(p, p.dag_top_tasks, true);
  return b ? 2000000 + b : 0;
}

// The host half of a bind's symbolic stage on one plan: a frame's destination table from its sorted pair list
// (nd_frame_dests) and the kinds of the pivot-column tiles (nd_tile_kinds).  Returns 0, or the number of the first check
// that fails: 1 the plan's own list, 2 a random subset, 3 lists with pairs the plan was not built from, 4 tile kinds.
extern "C" int nd_check_frame_dests(int J, int K_ED, const float* pts, const int32_t* knn, const uint32_t* pairs, int n_pairs,
                                    uint32_t seed) {
  NDPlanHost p;
  if (!nd_build_plan(J, K_ED, pts, knn, pairs, n_pairs, p)) return -1;
  auto same = [](const NDDest& a, const NDDest& b) {
    return a.front == b.front && a.prow == b.prow && a.pcol == b.pcol && a.transpose == b.transpose;
  };
  auto same_list = [&](const std::vector<NDDest>& a, const std::vector<NDDest>& b) {
    return a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin(), same);
  };
  auto rnd = [&seed] {
    seed = seed * 1664525u + 1013904223u;
    return seed >> 8;
  };
  const std::vector<uint32_t> own(pairs, pairs + n_pairs);
  const std::vector<NDDest> own_dest = p.block_dest;
  std::vector<NDDest> dest;
  size_t hits = 99;
  if (p.plan_pairs != own) return 1;
  if (!nd_frame_dests(p, J, own.data(), own.size(), dest, &hits) || hits != 0 || !same_list(dest, own_dest)) return 1;
  if (p.plan_pairs != own || !same_list(p.block_dest, own_dest)) return 1;

  std::vector<uint32_t> sub;
  for (uint32_t k : own)
    if (rnd() & 1) sub.push_back(k);
  if (!nd_frame_dests(p, J, sub.data(), sub.size(), dest, &hits) || hits != 0 || dest.size() != sub.size()) return 2;
  for (size_t i = 0; i < sub.size(); ++i) {
    NDDest d;
    if (!nd_dest_of(p, J, sub[i], d) || !same(d, dest[i])) return 2;
  }
  if (p.plan_pairs != own || !same_list(p.block_dest, own_dest)) return 2;

  std::vector<uint32_t> extra, placeable;   // pairs outside the plan's list / those of them with a fill position
  for (int k = 0; k < 2 * J + 8; ++k) {
    const uint32_t a = rnd() % (uint32_t)J, b = rnd() % (a + 1), key = a * (uint32_t)J + b;
    if (!std::binary_search(own.begin(), own.end(), key)) extra.push_back(key);
  }
  std::sort(extra.begin(), extra.end());
  extra.erase(std::unique(extra.begin(), extra.end()), extra.end());
  for (uint32_t k : extra) {
    NDDest d;
    if (nd_dest_of(p, J, k, d)) placeable.push_back(k);
  }
  for (const std::vector<uint32_t>* ex : {&extra, &placeable}) {
    std::vector<uint32_t> list(sub.size() + ex->size());
    list.resize(std::set_union(sub.begin(), sub.end(), ex->begin(), ex->end(), list.begin()) - list.begin());
    const std::vector<uint32_t> keys0 = p.plan_pairs;
    const std::vector<NDDest> dests0 = p.block_dest;
    size_t n_new = 0;
    for (uint32_t k : *ex) n_new += !std::binary_search(keys0.begin(), keys0.end(), k);
    const bool ok = nd_frame_dests(p, J, list.data(), list.size(), dest, &hits);
    if (ok != (ex->size() == placeable.size())) return 3;
    if (!ok) {
      if (hits != 0 || p.plan_pairs != keys0 || !same_list(p.block_dest, dests0)) return 3;
      continue;
    }
    if (hits != n_new || p.block_dest.size() != p.plan_pairs.size() || p.plan_pairs.size() != keys0.size() + n_new) return 3;
    for (size_t i = 1; i < p.plan_pairs.size(); ++i)
      if (p.plan_pairs[i - 1] >= p.plan_pairs[i]) return 3;
    for (size_t i = 0; i < keys0.size(); ++i) {
      const size_t at = std::lower_bound(p.plan_pairs.begin(), p.plan_pairs.end(), keys0[i]) - p.plan_pairs.begin();
      if (at >= p.plan_pairs.size() || p.plan_pairs[at] != keys0[i] || !same(p.block_dest[at], dests0[i])) return 3;
    }
    for (size_t i = 0; i < list.size(); ++i) {
      NDDest d;
      if (dest.size() != list.size() || !nd_dest_of(p, J, list[i], d) || !same(d, dest[i])) return 3;
    }
  }

  for (int pure_fill = 0; pure_fill < 2; ++pure_fill) {
    std::vector<uint8_t> kind;
    std::vector<long long> zero;
    int n_piv = -1, n_pure = -1;
    nd_tile_kinds(p, pure_fill != 0, kind, zero, n_piv, n_pure);
    if (kind.size() != (size_t)(p.tile_doubles / 4096) + 1 || (long long)zero.size() + n_pure != n_piv) return 4;
    long long piv_tiles = 0;
    for (const NDFront& f : p.fronts)
      for (int c = 0; c < f.npt; ++c) piv_tiles += f.nt - c;
    if (n_piv != piv_tiles || (!pure_fill && n_pure != 0)) return 4;
    std::vector<long long> z = zero;
    std::sort(z.begin(), z.end());
    for (size_t i = 0; i < z.size(); ++i)
      if (z[i] < 0 || z[i] >= p.tile_doubles || z[i] % 4096 || (i && z[i] == z[i - 1])) return 4;
    // no tile that a corner of an assembled 7 x 7 block reaches is pure fill
    auto reached_is_pure = [&](int front, int prow, int pcol) {
      if (front < 0) return false;
      const NDFront& f = p.fronts[front];
      const int rb = prow < f.nv ? 7 * prow : f.n1p + 7 * (prow - f.nv), cb = pcol < f.nv ? 7 * pcol : f.n1p + 7 * (pcol - f.nv);
      for (int i : {rb, rb + 6})
        for (int j : {cb, cb + 6}) {
          const int r = std::max(i, j) / 64, c = std::min(i, j) / 64;
          if (c < f.npt && r < f.nt && kind[(size_t)f.tile_first + (size_t)c * f.nt - (size_t)c * (c - 1) / 2 + (r - c)]) return true;
        }
      return false;
    };
    for (const NDDest& d : p.block_dest)
      if (reached_is_pure(d.front, d.prow, d.pcol)) return 4;
    for (const NDDest& d : p.pair_dest)
      if (reached_is_pure(d.front, d.prow, d.pcol)) return 4;
    for (size_t j = 0; j < p.node_front.size(); ++j)
      if (reached_is_pure(p.node_front[j], p.node_pos[j], p.node_pos[j])) return 4;
  }
  return 0;
}

// Where the plan eliminates every node: node_front[j] / node_pos[j] = the front that has node j as a pivot and its local
// position there, for a graph dissected down to leaf_nodes (0: SLM_ND_LEAF); fronts[3 i] / [3 i + 1] / [3 i + 2] = depth, pivot count
// and is_leaf of front i.  Fronts are numbered in processing order, deepest level first: the root is the last one.  Returns their number.
extern "C" int nd_node_fronts(int J, int K_ED, const float* pts, const int32_t* knn, const uint32_t* pairs, int n_pairs,
                              int leaf_nodes, int32_t* node_front, int32_t* node_pos, int32_t* fronts, int max_fronts) {
  NDPlanHost p;
  if (!nd_build_plan(J, K_ED, pts, knn, pairs, n_pairs, p, leaf_nodes)) return -1;
  for (int j = 0; j < J; ++j) {
    node_front[j] = p.node_front[j];
    node_pos[j] = p.node_pos[j];
  }
  const int n = (int)p.fronts.size();
  for (int i = 0; i < n && i < max_fronts; ++i) {
    fronts[3 * i] = p.fronts[i].depth;
    fronts[3 * i + 1] = p.fronts[i].nv;
    fronts[3 * i + 2] = p.fronts[i].is_leaf;
  }
  return n;
}

extern "C" int nd_stats(int J, int K_ED, const float* pts, const int32_t* knn, const uint32_t* pairs, int n_pairs,
                        double* out, int32_t* fronts, int max_fronts, int32_t* kp_out) {
  NDPlanHost p;
  if (!nd_build_plan(J, K_ED, pts, knn, pairs, n_pairs, p)) return -1;
  out[0] = p.flops;
  out[1] = p.flops_exact;
  out[2] = (double)p.fronts.size();
  out[3] = (double)(p.level_start.size() - 1);
  out[4] = p.dag_critical_us;
  out[5] = (double)p.tile_doubles * 8.0;
  out[6] = (double)p.dag_tasks.size() / 2;
  out[7] = (double)p.tile_items.size();
  int n = 0;
  for (const NDFront& f : p.fronts) {
    if (n >= max_fronts) break;
    fronts[4 * n + 0] = f.depth;
    fronts[4 * n + 1] = f.nv;
    fronts[4 * n + 2] = f.nb;
    fronts[4 * n + 3] = f.parent;
    if (kp_out) {   // boundary nodes of the front that are PIVOTS of its parent (they come first: elimination order)
      int kp = 0;
      if (f.parent >= 0)
        for (int b = 0; b < f.nb; ++b) kp += p.eamap[f.eamap_off + b] < p.fronts[f.parent].nv;
      kp_out[n] = kp;
    }
    ++n;
  }
  return n;
}
