"""The fixtures of tests/prep_plan_cases.py have the properties their names claim, and the NumPy plan of
tests/prep_plan_model.py -- what tests/test_gpu_prep_plan.py holds both device preparations against, array for array -- is
itself checked against brute force (Python loops over positions, pairs and surfels) on three small frames.  No GPU."""
import numpy as np
import pytest

import prep_plan_cases as ppc
import prep_plan_model as ppm
from super_amd import synth


def _stats(sc):
    return ppm.plan_stats(sc.sf_knn_idx, sc.J)


# ------------------------------------------------------------------------------------------------ what the names claim
@pytest.mark.parametrize("name", [n for n in ppc.SINGLE if n[0] == "n"])
def test_single_tuple_frames(name):
    sc = ppc.single(name)
    N, J = int(name[1:].split("_j")[0]), int(name.split("_j")[1])
    st = _stats(sc)
    assert (sc.N, sc.J) == (N, J) and st.tuples == 1 and st.tuple_surfels.tolist() == [N]
    assert st.positions == (64 if N <= 64 else 128) and st.runs == st.positions // 64
    _common(sc)


def _common(sc):
    """every frame: positive, normalised weights, distinct inside a row; valid rows; columns not all ascending"""
    w, idx = sc.sf_knn_w.astype(np.float64), sc.sf_knn_idx
    assert (w > 0).all() and np.abs(w.sum(1) - 1).max() < 1e-6 and all(len(set(r)) == w.shape[1] for r in w.tolist())
    assert (idx >= 0).all() and (idx < sc.J).all() and all(len(set(r)) == idx.shape[1] for r in idx.tolist())
    assert idx.shape[1] == 1 or not (np.diff(idx, axis=1) > 0).all()
    for k in ppc.PER_SURFEL:
        assert len(getattr(sc, k)) == sc.N


def test_pad_edges():
    sc = ppc.single("pad_edges")
    st = _stats(sc)
    assert sorted(st.tuple_surfels.tolist()) == [1, 2, 3, 4, 5, 63, 64, 65, 300]
    pc = (st.tuple_surfels + 3) // 4 * 4
    two_runs_for_8 = (pc == 8) & (st.tuple_start % 64 == 60) & (st.tuple_runs == 2)
    spans_wg = (st.tuple_start >> 8) != ((st.tuple_start + pc - 1) >> 8)
    assert two_runs_for_8.sum() == 1 and spans_wg.any()
    _common(sc)


def test_shuffled_surfels():
    sc, tiny = ppc.single("shuffled_surfels"), ppc.tiny()
    assert sc.N == tiny.N == 3000
    key = lambda s: sorted(map(tuple, np.concatenate([s.sf_points, s.sf_knn_idx, s.sf_knn_w], axis=1).tolist()))
    assert key(sc) == key(tiny) and not np.array_equal(sc.sf_points, tiny.sf_points)       # the same rows, another order
    a = np.sort(sc.sf_knn_idx, 1)[:, 0]
    waves = [a[i:i + 64] for i in range(0, sc.N, 64)]
    assert np.median([(w[1:] == w[:-1]).mean() for w in waves]) < 0.1                       # lane runs of length 1 prevail
    assert any(((w[:-3] == w[2:-1]) & (w[1:-2] == w[3:]) & (w[:-3] != w[1:-2])).any() for w in waves)   # a, b, a, b in a wave
    assert _stats(sc).tuples == _stats(tiny).tuples


@pytest.mark.parametrize("name", ["binA_1023", "binA_1024", "binA_1025"])
def test_phase_a_bin_at_the_cap(name):
    sc, want = ppc.single(name), int(name.split("_")[1])
    st = _stats(sc)
    assert st.bin_a[0] == want == st.max_bin_a and (st.tuple_ids[:, 0] == 0).sum() >= 3 and np.sort(st.bin_a)[-2] <= 200
    assert st.max_bin_b < ppm.BIN_CAP and (st.max_bin > ppm.BIN_CAP) == (name in ppc.OVER_CAP)
    _common(sc)


@pytest.mark.parametrize("name", ["binB_1024", "binB_1028"])
def test_phase_b_bin_at_the_cap(name):
    sc, want = ppc.single(name), int(name.split("_")[1])
    st = _stats(sc)
    top = st.tuple_ids[:, 3] == sc.J - 1
    assert st.bin_b[sc.J - 1] == want == st.max_bin_b == 4 * top.sum() and (st.tuple_surfels[top] == 1).all()
    assert st.max_bin_a < 200 and (st.max_bin > ppm.BIN_CAP) == (name in ppc.OVER_CAP)
    _common(sc)


@pytest.mark.parametrize("name", ["j1025", "j2050"])
def test_more_bins_than_scan_threads(name):
    sc = ppc.single(name)
    st = _stats(sc)
    assert sc.J == int(name[1:]) and -(-sc.J // 1024) == (2 if name == "j1025" else 3)
    assert 2900 <= sc.N <= 3100 and st.ids_used.max() == sc.J - 1 and (st.bin_a == 0).mean() > 0.5 and (st.bin_b == 0).mean() > 0.5
    assert st.max_bin < ppm.BIN_CAP
    _common(sc)


@pytest.mark.parametrize("name", ["wg_96", "wg_97"])
def test_workgroup_at_the_record_limit(name):
    sc, want = ppc.single(name), int(name.split("_")[1])
    st = _stats(sc)
    assert st.wg_records[0] == want and len(st.wg_records) > 1 and st.wg_records[1:].max() <= ppm.LB_MAX
    assert (want > ppm.LB_MAX) == (name in ppc.NOT_MERGED)
    plan = ppm.build_plan(sc.sf_knn_idx, sc.sf_knn_w, sc.sf_points, sc.J, np.float64)
    assert plan.max_records_per_wg == want and plan.v2 == (name not in ppc.NOT_MERGED)
    _common(sc)


def test_wg_dense():
    sc = ppc.single("wg_dense")
    st = _stats(sc)
    assert st.tuples == sc.N == 64 and st.positions == 256 and st.wg_records.tolist() == [st.wg_records[0]]
    assert st.wg_records[0] > 255                                      # beyond the uint8 clamp of run_lidx
    plan = ppm.build_plan(sc.sf_knn_idx, sc.sf_knn_w, sc.sf_points, sc.J, np.float32)
    assert plan.arrays[9].max() == 255 and not plan.v2
    _common(sc)


@pytest.mark.parametrize("name", ["hint_hold", "hint_miss"])
def test_hint_pairs(name):
    a, b = ppc.pair(name)
    t0, t1 = _stats(a).tuples, _stats(b).tuples
    bound = t0 + t0 // 8 + 64                                           # hinted_tuples (slm_prep.hip) before its min(., N)
    assert t1 == bound + (name == "hint_miss") and b.N > bound and a.J == b.J
    _common(a)
    _common(b)


def test_shrink_and_refused_rows():
    a, b = ppc.pair("shrink")
    assert a.N == 3000 and b.N == 65 and a.J == b.J and _stats(b).positions < _stats(a).positions
    tiny = ppc.tiny()
    for kind in ppc.REFUSED:
        sc = ppc.bad_row(kind)
        diff = np.flatnonzero((sc.sf_knn_idx != tiny.sf_knn_idx).any(1))
        assert diff.tolist() == [sc.N - 1]
        row = sc.sf_knn_idx[-1]
        assert {"dup_row": len(set(row.tolist())) < 4, "oob_row": row.max() == sc.J, "neg_row": row.min() == -1}[kind]
        with pytest.raises(AssertionError):
            ppm.plan_stats(sc.sf_knn_idx, sc.J)
    ppm.plan_stats(tiny.sf_knn_idx, tiny.J)                             # (building a bad row left the base frame alone)


@pytest.mark.parametrize("name", ppc.WIDENED)
@pytest.mark.parametrize("K", ppc.WIDEN_K)
def test_widened_frames(name, K):
    sc, src = ppc.widened(name, K), ppc.single(name)
    assert sc.sf_knn_idx.shape == sc.sf_knn_w.shape == (src.N, K)
    np.testing.assert_array_equal(sc.sf_knn_idx[:, :min(K, 4)], src.sf_knn_idx[:, :min(K, 4)])
    assert src.sf_knn_idx.shape == (src.N, 4)                           # the cached case is untouched
    _common(sc)


@pytest.mark.parametrize("kw", [ppc.TINY, ppc.SMALL], ids=["tiny", "small"])
def test_model_sizes_of_the_synthetic_scenes(kw):
    sc = synth.make_scene(**kw)
    p = ppm.build_plan(sc.sf_knn_idx, sc.sf_knn_w, sc.sf_points, sc.J, np.float32)
    assert min(p.tuples, p.positions, p.runs, p.pairs, p.records, p.max_records_per_wg) > 0
    assert p.positions % 64 == 0 and p.runs >= p.tuples and p.records >= p.pairs and p.positions >= sc.N
    assert p.positions <= (sc.N + 3 * p.tuples + 63) // 64 * 64 and p.runs <= p.tuples + p.positions // 64
    lens = [4 * p.positions, p.positions // 4, 4 * p.runs, 4 * p.positions, p.pairs, p.pairs + 1, 10 * p.runs, -(-p.positions // 256),
            -(-p.positions // 256), 10 * p.runs, p.pairs + 1, p.records, 3 * p.positions]
    assert [a.size for a in p.arrays] == lens
    assert [a.dtype for a in p.arrays] == [np.int32] * 3 + [np.float32] + [np.int32] * 5 + [np.uint8] + [np.int32] * 2 + [np.float32]


# ------------------------------------------------------------------------------------------- the model against brute force
def _brute_force(sc, dtype):
    """every rule of the layout, checked with loops over the plan that build_plan returns for the frame"""
    idx, J, N = sc.sf_knn_idx, sc.J, sc.N
    w = sc.sf_knn_w
    ident = np.stack([np.arange(N), np.zeros(N), np.ones(N)], axis=1)            # s_pts[pos, 0] names the surfel of a position
    p = ppm.build_plan(idx, w, ident, J, dtype)
    s_idx, grp_run, run_nodes, s_w, blk_key, blk_start, blk_entry, wg_first, wg_last, run_lidx, blk2_start, blk2_entry, s_pts = p.arrays
    canon = [tuple(sorted(r)) for r in idx.tolist()]

    # positions: every surfel at exactly one live position, with its own row; padding carries -1 / 0
    n_pos = p.positions
    assert n_pos % 64 == 0 and s_idx.shape == (n_pos, 4) and s_w.shape == (n_pos, 4) and s_pts.shape == (n_pos, 3)
    seen, walk = [], []
    for pos in range(n_pos):
        if s_idx[pos, 0] < 0:
            assert (s_idx[pos] == -1).all() and (s_w[pos] == 0).all() and (s_pts[pos] == 0).all()
            walk.append(None)
            continue
        i = int(s_pts[pos, 0])
        assert s_idx[pos].tolist() == idx[i].tolist() and s_pts[pos].tolist() == [i, 0, 1]
        assert s_w[pos].tolist() == w[i].astype(dtype).tolist() and s_w.dtype == np.dtype(dtype)
        seen.append(i)
        walk.append((canon[i], i))
    assert sorted(seen) == list(range(N))
    live = [x for x in walk if x is not None]
    assert live == sorted(live)                                   # tuples by (id0..id3), surfels inside a tuple by id
    # padding: only behind the last surfel of a tuple, fewer than 4, so that every tuple starts at a multiple of 4
    run, runs_expected, prev_t, tail = -1, [], None, False
    padded_total = 0
    for g in range(n_pos // 4):
        grp = walk[4 * g:4 * g + 4]
        if grp[0] is None:
            assert all(x is None for x in grp)
            tail = True
            assert grp_run[g] == -1                               # -1 only in the tail past the padded total
            continue
        assert not tail
        padded_total = 4 * g + 4
        t = grp[0][0]
        k = sum(x is not None for x in grp)
        assert all(x is not None and x[0] == t for x in grp[:k]) and all(x is None for x in grp[k:])
        if k < 4:                                                 # a padded group ends its tuple
            nxt = walk[4 * g + 4] if 4 * g + 4 < n_pos else None
            assert nxt is None or nxt[0] != t
        if t != prev_t or (4 * g) % 64 == 0:                      # a run = (tuple, 64-position chunk)
            run += 1
            runs_expected.append(t)
        prev_t = t
        assert grp_run[g] == run
    assert n_pos == (padded_total + 63) // 64 * 64
    assert p.runs == run + 1 == len(run_nodes) and [tuple(r) for r in run_nodes.tolist()] == runs_expected
    assert p.tuples == len(set(canon))

    # pair blocks: under every pair exactly the runs whose tuple has both ids, in the slots that hold them
    assert (np.diff(blk_key) > 0).all() and blk_start[0] == 0 and blk_start[-1] == 10 * p.runs == len(blk_entry)
    at = {int(k): n for n, k in enumerate(blk_key.tolist())}
    for a in range(J):
        for b in range(a + 1):
            want = [r for r, t in enumerate(runs_expected) if a in t and b in t]
            if not want:
                assert a * J + b not in at
                continue
            n = at[a * J + b]
            seg = blk_entry[blk_start[n]:blk_start[n + 1]].tolist()
            assert seg == sorted(seg) and [e >> 4 for e in seg] == want
            for e in seg:
                assert run_nodes[e >> 4][(e >> 2) & 3] == a and run_nodes[e >> 4][e & 3] == b and (e >> 2) & 3 >= e & 3
    assert len(at) == p.pairs == sum(1 for a in range(J) for b in range(a + 1) if any(a in t and b in t for t in set(runs_expected)))

    # numbers through the plan: random integer 4 x 4 slot matrices per surfel, per-run sums, then both inverted indices
    rng = np.random.default_rng(5)
    M = rng.integers(-9, 10, (N, 4, 4)).astype(np.int64)
    direct = np.zeros((J, J), np.int64)
    for i in range(N):
        c = canon[i]
        for pa in range(4):
            for pb in range(pa + 1):
                direct[c[pa], c[pb]] += M[i, pa, pb]
    G = np.zeros((p.runs, 4, 4), np.int64)
    for pos in range(n_pos):
        if walk[pos] is not None:
            G[grp_run[pos // 4]] += M[walk[pos][1]]
    got = np.zeros((J, J), np.int64)
    for n, k in enumerate(blk_key.tolist()):
        got[k // J, k % J] = sum(G[e >> 4, (e >> 2) & 3, e & 3] for e in blk_entry[blk_start[n]:blk_start[n + 1]].tolist())
    np.testing.assert_array_equal(got, direct)
    # ... and through the workgroup records: run -> local record (run_lidx) -> pair (blk2_entry)
    n_wg = -(-n_pos // 256)
    assert len(wg_first) == len(wg_last) == n_wg and wg_first[0] == 0 and wg_last[-1] == p.records - 1
    assert (wg_first[1:] == wg_last[:-1] + 1).all() and p.max_records_per_wg == (wg_last - wg_first + 1).max() <= 255
    R = np.zeros(p.records, np.int64)
    rec_wg = np.full(p.records, -1)
    first_pos_of_run = {}
    for g in range(n_pos // 4):
        if grp_run[g] >= 0:
            first_pos_of_run.setdefault(int(grp_run[g]), 4 * g)
    for r in range(p.runs):
        wg = first_pos_of_run[r] >> 8
        for pa in range(4):
            for pb in range(pa + 1):
                u = wg_first[wg] + int(run_lidx[10 * r + pa * (pa + 1) // 2 + pb])
                assert wg_first[wg] <= u <= wg_last[wg]
                R[u] += G[r, pa, pb]
                rec_wg[u] = wg
    assert (rec_wg >= 0).all() and (np.diff(rec_wg) >= 0).all()
    got2 = np.zeros((J, J), np.int64)
    assert len(blk2_start) == p.pairs + 1 and blk2_start[0] == 0 and blk2_start[-1] == p.records == len(blk2_entry)
    assert sorted(blk2_entry.tolist()) == list(range(p.records))
    for n, k in enumerate(blk_key.tolist()):
        seg = blk2_entry[blk2_start[n]:blk2_start[n + 1]].tolist()
        assert seg == sorted(seg) and len(seg) == len({int(rec_wg[u]) for u in seg}) >= 1      # one record per workgroup
        got2[k // J, k % J] = R[seg].sum()
    np.testing.assert_array_equal(got2, direct)
    return p


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["pad_edges", "wg_97", "shuffled_surfels"])
def test_model_against_brute_force(name, dtype):
    sc = ppc.single(name)
    p = _brute_force(sc, dtype)
    st = _stats(sc)
    assert (p.tuples, p.positions, p.runs) == (st.tuples, st.positions, st.runs) and p.max_records_per_wg == st.wg_records.max()
    # the weights and points of the frame itself are copied in the state's dtype, never rounded through another
    w64 = sc.f64("sf_knn_w") + 2.0 ** -40                                       # float64 keeps the 2^-40, float32 cannot
    q = ppm.build_plan(sc.sf_knn_idx, w64, sc.f64("sf_points"), sc.J, dtype)
    live = q.arrays[0][:, 0] >= 0
    ids = p.arrays[12][live, 0].astype(np.int64)                                # (p was built with the surfel id as point)
    np.testing.assert_array_equal(q.arrays[3][live], w64[ids] if dtype is np.float64 else sc.sf_knn_w[ids])
    np.testing.assert_array_equal(q.arrays[12][live], sc.sf_points[ids].astype(dtype))
