"""Pins the match-set edge fixture (tests/data_edge_cases.py) so that it cannot rot, and the oracle against the reference's
own output on it (tests/golden/lm_edges.npz, recorded by tests/golden/make_golden_data_edges.py).  CPU only."""
import os

import numpy as np
import pytest

import data_edge_cases as dec
from helpers import GOLDEN_DIR, coo_dense
from oracle import lm_oracle as orc

TOL = 1e-9          # tests/test_oracle_golden.py: f64 restatement against the f64 reference

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")     # the non-finite groups are meant to be non-finite


def _frame(K, state="f64", n_base=dec.N_BASE):
    sc = dec.edge_scene(K, n_base)
    return orc.Frame.from_scene(sc if state == "f64" else dec.state32(sc))


def _mask(t, N):
    m = np.zeros(N, bool)
    m[t.match] = True
    return m


def _uv(fr, ix):
    T, _ = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, dec.identity())
    v_, u_, _, _ = orc.project(T[ix], fr.K, fr.H, fr.W)
    return u_, v_


def test_layout_is_the_same_for_every_k_and_size():
    assert set(dec.CLASSES.values()) == {"match", "dropped", "mixed"}
    assert all(len(ix) >= 8 for ix in dec.GROUPS.values())
    assert sorted(np.concatenate(list(dec.GROUPS.values()))) == list(range(dec.N_GROUPS))
    a = dec.edge_scene(4)
    assert (a.H, a.W, a.J, a.N) == (60, 80, 48, dec.N_GROUPS + 600)
    assert a.sf_points.dtype == np.float64 and a.K.dtype == np.float32
    for K, n_base in ((1, 600), (6, 600), (4, 450), (4, 300)):
        b = dec.edge_scene(K, n_base)
        assert b.sf_knn_idx.shape == (dec.N_GROUPS + n_base, K)
        g = slice(0, dec.N_GROUPS)
        assert a.sf_points[g].tobytes() == b.sf_points[g].tobytes()
        np.testing.assert_array_equal(a.sf_knn_idx[g, 0], b.sf_knn_idx[g, 0])
        np.testing.assert_array_equal(a.sf_knn_w[g, 0], b.sf_knn_w[g, 0])
        assert not b.sf_knn_w[g, 1:].any()
        assert a.index_map.tobytes() == b.index_map.tobytes() and a.valid.tobytes() == b.valid.tobytes()
        assert a.tgt_points.tobytes() == b.tgt_points.tobytes()
    # the two kinds of one-sided pixel exist, and NaN rows
    vm = a.valid.reshape(a.H, a.W)
    assert (vm & (a.index_map < 0)).sum() >= 8 and (~vm & (a.index_map >= 0)).sum() >= 8 and (~vm & (a.index_map < 0)).sum() >= 9
    assert np.isnan(a.tgt_points).any(1).sum() == 4 and np.isnan(a.tgt_norms).any(1).sum() == 4


@pytest.mark.parametrize("K", dec.KS)
def test_every_group_lands_in_its_class_at_identity(K):
    fr = _frame(K)
    m = _mask(orc.data_term(fr, dec.identity(), 1.0), len(fr.sf_points))
    for name, ix in dec.GROUPS.items():
        np.testing.assert_array_equal(m[ix], dec.EXPECT[ix], err_msg=name)
        want = {"match": m[ix].all(), "dropped": not m[ix].any(), "mixed": m[ix].any() and not m[ix].all()}
        assert want[dec.CLASSES[name]], name
    assert m[dec.N_GROUPS:].mean() > 0.9            # the generic path stays covered


@pytest.mark.parametrize("K", dec.KS)
def test_exact_groups_are_exact_in_both_summation_orders(K):
    sc = dec.edge_scene(K)
    fr = orc.Frame.from_scene(sc)
    ex = np.nonzero(dec.EXACT)[0]
    p, g, w = fr.sf_points[ex], fr.ed_points[fr.sf_knn_idx[ex]], fr.sf_knn_w[ex]
    assert np.isfinite(g).all()
    t = (p[:, None, :] - g) + g                      # identity warp: R d + b + g with R = I, b = 0
    fwd = np.zeros_like(p)
    for k in range(K):
        fwd = fwd + w[:, k, None] * t[:, k]
    bwd = np.zeros_like(p)
    for k in reversed(range(K)):
        bwd = bwd + w[:, k, None] * t[:, k]
    assert fwd.tobytes() == p.tobytes() and bwd.tobytes() == p.tobytes()
    assert orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, dec.identity())[0][ex].tobytes() == p.tobytes()
    # the coordinates that are meant to sit on a boundary do, bit for bit
    frac = lambda x: x - np.floor(x)
    u, v = _uv(fr, dec.GROUPS["int_u"])
    assert (u == np.rint(u)).all() and (frac(v) != 0).all()
    u, v = _uv(fr, dec.GROUPS["int_v"])
    assert (v == np.rint(v)).all() and (frac(u) != 0).all()
    u, v = _uv(fr, dec.GROUPS["int_uv"])
    assert (u == np.rint(u)).all() and (v == np.rint(v)).all()
    for name, odd in (("half_even", 0), ("half_odd", 1)):
        u, v = _uv(fr, dec.GROUPS[name])
        tie = np.concatenate([u[:4], v[4:]])
        assert (frac(tie) == 0.5).all() and (np.floor(tie) % 2 == odd).all(), name
        # they round to the side they name: even k -> the floor tap, odd k -> the ceil tap
        assert (np.rint(tie) == (np.ceil(tie) if odd else np.floor(tie))).all(), name
    u, v = _uv(fr, dec.GROUPS["neg_zero"])
    tie = np.where(v < 0, v, u)
    assert ((tie >= -0.5) & (tie < 0)).all() and (np.rint(tie) == 0).all() and np.signbit(np.rint(tie)).all()
    assert -0.5 in tie and -dec.DELTA in tie
    u, v = _uv(fr, dec.GROUPS["last_ok"])
    assert set(np.rint(v[0::2])) == {fr.H - 2.0} and set(np.rint(u[1::2])) == {fr.W - 2.0}
    assert fr.H - 1.5 in v and fr.H - 1.5 - dec.DELTA in v and fr.W - 1.5 in u and fr.W - 1.5 - dec.DELTA in u
    u, v = _uv(fr, dec.GROUPS["first_bad"])
    assert set(np.rint(v[0::2])) == {fr.H - 1.0} and set(np.rint(u[1::2])) == {fr.W - 1.0}
    assert fr.H - 1.5 + dec.DELTA in v and fr.W - 1.5 + dec.DELTA in u
    u, v = _uv(fr, dec.GROUPS["far_out"])
    assert (np.maximum(np.abs(u), np.abs(v)) >= 0.99e9).all() and (np.abs(u) > 2.0 ** 31).any() and (np.abs(v) > 2.0 ** 40).any()
    T, _ = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, dec.identity())
    assert (T[dec.GROUPS["z_eps"], 2] + 1e-8 == 0.0).all()
    u, v = _uv(fr, dec.GROUPS["z_eps"])
    assert not (np.isfinite(u) & np.isfinite(v)).any()
    assert (T[dec.GROUPS["behind"], 2] < -0.5).all()
    u, v = _uv(fr, dec.GROUPS["behind"])
    assert ((u > 5) & (u < fr.W - 5) & (v > 5) & (v < fr.H - 5)).all()
    assert not np.isfinite(fr.sf_points[dec.GROUPS["nonfinite_p"]]).all(1).any()


def test_coinciding_taps_both_carry_weight_one():
    """defect D4: floor == ceil on an exactly integer coordinate, and both taps get weight 1 -- o is TWICE the linear
    interpolation along the other axis, four times the pixel's row when both coordinates are integer"""
    fr = _frame(4)
    P = fr.tgt_points

    def rows(n, m):
        return P[fr.index_map[n.astype(int), m.astype(int)]]

    u, v = _uv(fr, dec.GROUPS["int_u"])
    o, _, taps = orc.bilinear_lookup(v, u, P, fr.index_map)
    assert (taps[:, 0] == taps[:, 1]).all() and (taps[:, 2] == taps[:, 3]).all() and (taps[:, 0] != taps[:, 2]).all()
    a = (v - np.floor(v))[:, None]
    np.testing.assert_allclose(o, 2 * ((1 - a) * rows(np.floor(v), u) + a * rows(np.ceil(v), u)), rtol=1e-15, atol=0)
    u, v = _uv(fr, dec.GROUPS["int_v"])
    o, _, taps = orc.bilinear_lookup(v, u, P, fr.index_map)
    assert (taps[:, 0] == taps[:, 2]).all() and (taps[:, 1] == taps[:, 3]).all() and (taps[:, 0] != taps[:, 1]).all()
    a = (u - np.floor(u))[:, None]
    np.testing.assert_allclose(o, 2 * ((1 - a) * rows(v, np.floor(u)) + a * rows(v, np.ceil(u))), rtol=1e-15, atol=0)
    u, v = _uv(fr, dec.GROUPS["int_uv"])
    o, _, taps = orc.bilinear_lookup(v, u, P, fr.index_map)
    assert (taps == taps[:, :1]).all()
    np.testing.assert_array_equal(o, 4 * rows(v, u))


@pytest.mark.parametrize("state", ["f64", "f32"])
@pytest.mark.parametrize("K", dec.KS)
def test_generic_beta_leaves_no_ties_and_keeps_both_kinds(K, state):
    fr = _frame(K, state)
    beta = dec.generic_beta()
    assert np.abs(beta - dec.identity()).max() > 1e-3
    td = dec.tie_distance(fr, beta)
    assert (td <= 1e-9).mean() <= 0.01
    m = _mask(orc.data_term(fr, beta, 1.0), len(fr.sf_points))[:dec.N_GROUPS]
    assert 20 < m.sum() < dec.N_GROUPS - 20
    if state == "f64":          # at identity the exact groups ARE ties: the distance says so
        td0 = dec.tie_distance(fr, dec.identity())
        for name in ("int_u", "int_v", "int_uv", "half_even", "half_odd"):
            assert (td0[dec.GROUPS[name]] == 0).all(), name
    else:                       # rounded to float32 they are generic
        assert (dec.tie_distance(fr, dec.identity()) <= 1e-9).mean() <= 0.01


def test_flipped_frames_follow_the_rounded_pixel():
    sc = dec.edge_scene(4)
    for frames, hole in ((dec.flipped_frames(sc), True), (dec.invalid_only_frames(sc), False)):
        assert len(frames) == 8
        got = {}
        for label, fl in frames:
            assert (fl.valid != sc.valid).sum() == 1 and (fl.index_map != sc.index_map).sum() == (1 if hole else 0)
            m = _mask(orc.data_term(orc.Frame.from_scene(fl), dec.identity(), 1.0), sc.N)
            got.setdefault(label.split("@")[0], []).append(bool(m[dec.GROUPS[label.split("@")[0]][0]]))
        if hole:                 # any tap a hole: dropped
            assert got == {"half_even": [False] * 4, "half_odd": [False] * 4}
        else:                    # only the rounded pixel's own valid counts: (floor v, floor u) for even k, (floor v, ceil u) for odd
            assert got == {"half_even": [False, True, True, True], "half_odd": [True, False, True, True]}


@pytest.mark.parametrize("state", ["f64", "f32"])
@pytest.mark.parametrize("K", [4, 6])
def test_oracle_trace_is_decisive_and_rejects(K, state):
    """what tests/test_gpu_data_edges.py relies on: at least 8 of the 10 iterations have no surfel within 1e-9 px of a
    boundary at the current and at the trial warp, and at least one step is rejected and followed by another iteration"""
    fr = _frame(K, state)
    trace = []
    orc.lm(fr, orc.default_opt(), trace=trace)
    assert len(trace) == 10 and all("loss" in t for t in trace)
    cur, decisive = dec.identity(), []
    for t in trace:
        decisive.append(dec.tie_distance(fr, cur).min() > 1e-9 and dec.tie_distance(fr, cur + t["delta"]).min() > 1e-9)
        cur = t["beta"]
    assert sum(decisive) >= 8
    assert False in [t["accepted"] for t in trace][:-1]


# ---- the oracle against the reference's own run -------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["id", "gen"])
@pytest.mark.parametrize("K", [4, 6])
def test_oracle_reproduces_the_reference_on_the_edges(K, tag):
    g = np.load(os.path.join(GOLDEN_DIR, "lm_edges.npz"))
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "lm_edges.npz")) < 1 << 20
    key = f"k{K}_{tag}"
    refused = [str(n) for n in g[key + "_refused"]]
    assert set(refused) <= set(g["refused"].tolist()) and "first_bad" in refused      # defect D2: the reference raises
    assert set(refused) <= {"first_bad", "last_ok"} and (tag == "gen" or refused == ["first_bad"])
    sc = dec.edge_scene(K)
    keep = dec.without_groups(sc, refused)
    sub = dec.subset(sc, keep)
    np.testing.assert_array_equal(g[key + "_in_digest"], dec.digest(sub), err_msg="the scene is not the recorded one")
    fr = orc.Frame.from_scene(sub)
    beta = dec.identity() if tag == "id" else dec.generic_beta()
    opt = orc.default_opt(mesh_arap=False, mesh_rot=False)
    t = orc.data_term(fr, beta, opt.sf_point_plane_weight)
    np.testing.assert_array_equal(keep[t.match], g[key + "_match"])                    # bit-exact
    np.testing.assert_allclose(t.r, g[key + "_data_r"], rtol=0, atol=TOL)
    JtJ, jtl, M = orc.normal_equations(fr, beta, opt)
    assert M == len(g[key + "_match"])
    np.testing.assert_allclose(jtl, g[key + "_jtl"], rtol=0, atol=1e-8)
    P = 7 * sc.J
    ref = coo_dense(g[key + "_jtj_idx"].astype(np.int64), g[key + "_jtj_val"], (P, P))
    assert float(g[key + "_jtj_upper_err"]) == 0.0                                    # the lower triangle is all of it
    np.testing.assert_allclose(np.tril(JtJ), ref, rtol=0, atol=1e-7 * max(1.0, np.abs(ref).max()))
    # the groups the reference ran are in the record with the class the fixture names
    if tag == "id":
        m = np.zeros(sc.N, bool)
        m[g[key + "_match"]] = True
        for name, ix in dec.GROUPS.items():
            if name not in refused:
                np.testing.assert_array_equal(m[ix], dec.EXPECT[ix], err_msg=name)
