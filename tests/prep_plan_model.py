"""The K = 4 preparation plan (python-super_amd/csrc/slm_prep.hip) rebuilt in plain NumPy from the surfel KNN table alone:
the thirteen arrays ``slm_debug_read_plan`` returns (``what`` = 0..12 in include/super_lm.h) and the sizes of
``slm_get_plan_info``.  Written from the layout's specification -- the header comment of slm_prep.hip, slm_prep.h -- with
whole-array operations (``np.unique``, ``np.lexsort``, ``np.repeat``, ``np.searchsorted``): no bins, no per-node passes, no LDS
sorts, no scans over blocks.  It is a different algorithm from both device preparations, which is its value: an error the
binned kernels and the rocPRIM pipeline share does not pass a comparison with it.  Importable without a GPU; consumed by
tests/prep_plan_cases.py, tests/test_prep_plan_cases.py (CPU) and tests/test_gpu_prep_plan.py (MI355X).

The rules it restates:

* tuple = the set of a surfel's four node ids, ascending; tuples ordered by (id0, id1, id2, id3); surfels inside a tuple by
  surfel id;
* every tuple's segment of positions is padded to a multiple of 4; ``n_pos`` = the padded total rounded up to 64; a live
  position carries the surfel's row in its ORIGINAL column order (``s_idx``) and ``s_w`` / ``s_pts`` copied in the state's
  dtype; a padding position carries -1 / 0; ``grp_run[pos / 4]`` is the run of the position group, -1 only in the tail past
  the padded total;
* run = (tuple, 64-position chunk), in position order; ``run_nodes`` = the tuple's ascending ids;
* pair blocks: ``blk_key`` = the distinct ``a * J + b`` (a >= b) over the runs, ascending; ``blk_entry`` = the 10 n_runs
  payloads ``run * 16 + pa * 4 + pb`` ordered by (key, payload); ``blk_start`` with the end marker;
* workgroup = ``pos >> 8``; records = the distinct (workgroup, key), by workgroup then key; ``wg_first`` / ``wg_last`` bound a
  workgroup's records; ``run_lidx[10 run + pa (pa + 1) / 2 + pb]`` = min(local record index, 255); ``blk2_start`` aligned
  with ``blk_key``, ``blk2_entry`` the record ids by (key, record)."""
from types import SimpleNamespace

import numpy as np

ARRAYS = ("s_idx", "grp_run", "run_nodes", "s_w", "blk_key", "blk_start", "blk_entry", "wg_first", "wg_last", "run_lidx",
          "blk2_start", "blk2_entry", "s_pts")          # index = `what` of slm_debug_read_plan
V2_ARRAYS = (7, 8, 9, 10, 11)                           # present only while the workgroup-merged form is in use
PA, PB = np.tril_indices(4)                             # the 10 slot pairs (pa, pb <= pa) in the order pa (pa + 1) / 2 + pb
LB_MAX = 96                                             # SLM_LB_MAX: most records of a workgroup the merged form takes
BIN_CAP = 1024                                          # largest bin the binned preparation sorts


def _excl(x):
    return np.concatenate([[0], np.cumsum(x)[:-1]]).astype(np.int64)


def _layout(sf_knn_idx, J):
    """tuples, positions and runs of a KNN table (everything that does not depend on weights, points or the dtype)"""
    idx = np.asarray(sf_knn_idx, np.int64)
    N = len(idx)
    assert idx.shape == (N, 4) and N > 0 and (idx >= 0).all() and (idx < J).all()
    canon = np.sort(idx, axis=1)
    assert (np.diff(canon, axis=1) > 0).all(), "a surfel row repeats an id"
    tup, inv, cnt = np.unique(canon, axis=0, return_inverse=True, return_counts=True)     # lexicographic
    inv = inv.reshape(-1)
    order = np.lexsort((np.arange(N), inv))                # surfels by (tuple, surfel id)
    pc = (cnt + 3) // 4 * 4
    pstart, tstart = _excl(pc), _excl(cnt)
    ptot = int(pc.sum())
    t_of = inv[order]
    pos = pstart[t_of] + np.arange(N) - tstart[t_of]       # position of order[i]
    c0, c1 = pstart // 64, (pstart + pc - 1) // 64         # first / last chunk a tuple touches
    nr = c1 - c0 + 1
    rstart = _excl(nr)
    run_t = np.repeat(np.arange(len(tup)), nr)
    run_chunk = c0[run_t] + np.arange(int(nr.sum())) - rstart[run_t]
    return SimpleNamespace(idx=idx, N=N, tup=tup, cnt=cnt, pc=pc, pstart=pstart, ptot=ptot, n_pos=(ptot + 63) // 64 * 64,
                           order=order, pos=pos, c0=c0, nr=nr, rstart=rstart, run_t=run_t, run_chunk=run_chunk)


def build_plan(sf_knn_idx, sf_knn_w, sf_points, J, state_dtype):
    """-> namespace: ``arrays`` (the thirteen arrays, by ``what``), the sizes ``tuples``, ``positions``, ``runs``, ``pairs``,
    ``records``, ``max_records_per_wg``, and ``v2`` (the merged form is usable: max_records_per_wg <= LB_MAX)"""
    L = _layout(sf_knn_idx, J)
    dt = np.dtype(state_dtype)
    n_pos, n_runs = L.n_pos, len(L.run_t)
    s_idx = np.full((n_pos, 4), -1, np.int32)
    s_w = np.zeros((n_pos, 4), dt)
    s_pts = np.zeros((n_pos, 3), dt)
    s_idx[L.pos] = L.idx[L.order]
    s_w[L.pos] = np.asarray(sf_knn_w)[L.order].astype(dt)
    s_pts[L.pos] = np.asarray(sf_points)[L.order].astype(dt)
    # position groups: the tuple of group g, then its run through the chunk of its first position
    grp_run = np.full(n_pos // 4, -1, np.int32)
    g_t = np.repeat(np.arange(len(L.tup)), L.pc // 4)
    grp_run[:len(g_t)] = L.rstart[g_t] + (4 * np.arange(len(g_t))) // 64 - L.c0[g_t]
    run_nodes = L.tup[L.run_t].astype(np.int32)
    # pair blocks
    key = (run_nodes[:, PA].astype(np.int64) * J + run_nodes[:, PB]).reshape(-1)
    payload = (np.arange(n_runs)[:, None] * 16 + PA[None, :] * 4 + PB[None, :]).reshape(-1)
    o = np.lexsort((payload, key))
    blk_key = np.unique(key)
    blk_start = np.concatenate([np.searchsorted(key[o], blk_key), [len(key)]])
    blk_entry = payload[o]
    # (workgroup, pair) records
    JJ = int(J) * int(J)
    n_wg = (n_pos + 255) // 256
    wg = np.repeat(L.run_chunk >> 2, 10)
    rec, rec_of = np.unique(wg * JJ + key, return_inverse=True)
    rec_of = rec_of.reshape(-1)
    rec_wg, rec_key = rec // JJ, rec % JJ
    wg_first = np.searchsorted(rec_wg, np.arange(n_wg), side="left")
    wg_last = np.searchsorted(rec_wg, np.arange(n_wg), side="right") - 1
    run_lidx = np.minimum(rec_of - wg_first[wg], 255).astype(np.uint8)     # entry e of run r sits at 10 r + e already
    o2 = np.lexsort((np.arange(len(rec)), rec_key))
    blk2_start = np.concatenate([np.searchsorted(rec_key[o2], blk_key), [len(rec)]])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    arrays = [s_idx, grp_run, run_nodes, s_w, i32(blk_key), i32(blk_start), i32(blk_entry), i32(wg_first), i32(wg_last),
              run_lidx, i32(blk2_start), i32(o2), s_pts]
    per_wg = wg_last - wg_first + 1
    return SimpleNamespace(arrays=arrays, tuples=len(L.tup), positions=n_pos, runs=n_runs, pairs=len(blk_key), records=len(rec),
                           max_records_per_wg=int(per_wg.max()), v2=bool(per_wg.max() <= LB_MAX))


def plan_stats(sf_knn_idx, J):
    """What the fixtures claim about a KNN table, measured: ``bin_a`` surfels per smallest node and ``bin_b`` pair entries per
    larger node (for node n the sum over the runs of slot + 1, slot = n's place in the ascending tuple) -- the bins of the
    binned preparation's two sorting phases --, their maxima, the records of every workgroup, and the layout of the tuples
    (ascending ids, surfel counts, first padded position, runs)."""
    L = _layout(sf_knn_idx, J)
    bin_a = np.bincount(L.tup[:, 0], weights=L.cnt, minlength=J).astype(np.int64)
    nodes = L.tup[L.run_t]
    bin_b = np.bincount(nodes.reshape(-1), weights=np.tile([1, 2, 3, 4], len(nodes)), minlength=J).astype(np.int64)
    key = (nodes[:, PA] * J + nodes[:, PB]).reshape(-1)
    rec = np.unique(np.repeat(L.run_chunk >> 2, 10) * (int(J) * int(J)) + key)
    wg_records = np.bincount(rec // (int(J) * int(J)), minlength=(L.n_pos + 255) // 256)
    return SimpleNamespace(bin_a=bin_a, bin_b=bin_b, max_bin_a=int(bin_a.max()), max_bin_b=int(bin_b.max()),
                           max_bin=int(max(bin_a.max(), bin_b.max())), wg_records=wg_records, tuples=len(L.tup),
                           tuple_ids=L.tup, tuple_surfels=L.cnt, tuple_start=L.pstart, tuple_runs=L.nr, positions=L.n_pos,
                           padded_total=L.ptot, runs=len(L.run_t), ids_used=np.unique(L.idx))
