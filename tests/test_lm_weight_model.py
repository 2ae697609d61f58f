"""The float64 model of the LM path's per-residual data weights (tests/lm_weight_model.py) checked on the CPU: pinned to
``graphfit_oracle.point_plane`` (itself pinned to the reference's goldens) on scenes where the LM match set (margin 0 on
the rounded pixel) and GraphFit's (margin 1) are both every surfel, and -J^T r of the weighted term against central
differences of the weighted loss with the weights held fixed."""
import numpy as np
import pytest
import torch

import lm_corr_model as lcm
import lm_weight_model as lwm
from oracle import graphfit_oracle as gfo
from oracle import lm_oracle as orc
from super_amd import synth

# (N, J, K, C, seed, src_border): both match sets are all surfels; pp_max = 2e-5 keeps KEPT of them
PIN_SCENES = [(600, 30, 4, 3, 7, 8), (600, 30, 6, 2, 8, 8), (37, 12, 4, 2, 3, 6)]
KEPT = {600 * 4 + 3: 343, 600 * 6 + 2: 331, 37 * 4 + 2: 24}


def pin_scene(N, J, K, C, seed, sb):
    return synth.make_scene(N=N, J=J, H=60, W=80, seed=seed, n_neighbors=K, src_border=sb, tgt_border=3, tgt_holes=0.0,
                            semantic=True, num_classes=C)


@pytest.mark.parametrize("case", PIN_SCENES)
def test_weighted_sums_equal_the_graphfit_oracle(case):
    N, J, K, C, seed, sb = case
    sc = pin_scene(*case)
    fr, sem = orc.Frame.from_scene(sc), lwm.sem_of(sc)
    beta = lcm.random_beta(sc.J, 17, rot=0.01, trans=0.002)
    pb = gfo.Problem(sc)
    dv = torch.cat([torch.from_numpy(beta), torch.tensor([[1.0, 0, 0, 0, 0, 0, 0]], dtype=torch.float64)], 0)   # global row: identity
    _, sf = gfo.deform(pb, dv)
    for name, mode in (("soft", 2), ("hard", 1), (None, 0)):
        ww = lwm.weights(fr, sem, beta, mode)
        assert len(ww.t.match) == N                              # every surfel matched
        lwm.check_conditions(ww, mode, 0.0)
        want, cnt = gfo.point_plane(pb, sf, seg_mode=name)
        mine = float((ww.w * ww.s).sum())
        print(case, name, "model", mine, "oracle", float(want), "rel", abs(mine - float(want)) / abs(float(want)))
        assert int(cnt) == N
        np.testing.assert_allclose(mine, float(want), rtol=1e-12)
        assert lwm.data_loss(fr, sem, beta, 1.0, mode)[0] == pytest.approx(mine, rel=1e-14)
    ww = lwm.weights(fr, sem, beta, 0, 2e-5)
    lwm.check_conditions(ww, 0, 2e-5)
    want, cnt = gfo.point_plane(pb, sf, pp_max=2e-5)
    print(case, "pp_max kept", int(ww.w.sum()), "nearest |s/pp_max - 1|", np.abs(ww.s / 2e-5 - 1).min())
    assert int(ww.w.sum()) == int(cnt) == KEPT[N * K + C]
    np.testing.assert_allclose(float((ww.w * ww.s).sum()), float(want), rtol=1e-12)
    # with a semantic weight pp_max is ignored
    np.testing.assert_array_equal(lwm.weights(fr, sem, beta, 1, 2e-5).w, lwm.weights(fr, sem, beta, 1).w)


@pytest.mark.parametrize("mode,pp_max", [(1, 0.0), (2, 0.0), (0, 2e-5)])
@pytest.mark.parametrize("K", [3, 4, 6])
def test_weighted_gradient_matches_central_differences(K, mode, pp_max):
    """-J^T r of the weighted rows = -(1/2) d/dbeta sum w_i r_i^2 with w held at its value at beta"""
    sc = synth.make_scene(N=400, J=24, H=60, W=80, seed=50 + K, n_neighbors=K, src_border=3, tgt_border=3, semantic=True,
                          num_classes=3)
    fr, sem = orc.Frame.from_scene(sc), lwm.sem_of(sc)
    beta = lcm.random_beta(sc.J, 5, rot=0.01, trans=0.002)
    lam = 0.7
    ww = lwm.weights(fr, sem, beta, mode, pp_max)
    assert 0 < (ww.w > 0).sum() and (mode == 2 or (ww.w == 0).sum() > 0)
    Jd, r = lwm.data_jacobian(fr, sem, beta, lam, mode, pp_max)
    jtl = -Jd.T @ r
    rng = np.random.default_rng(1)
    h = 1e-6
    match = ww.t.match
    for col in rng.choice(7 * sc.J, 25, replace=False):
        d = np.zeros(7 * sc.J)
        d[col] = h
        tp = orc.data_term(fr, beta + d.reshape(-1, 7), lam)
        tm = orc.data_term(fr, beta - d.reshape(-1, 7), lam)
        if not (np.array_equal(tp.match, match) and np.array_equal(tm.match, match)):
            continue                                              # the match set moved inside the stencil: no derivative there
        fd = ((ww.w * tp.r ** 2).sum() - (ww.w * tm.r ** 2).sum()) / (2 * h)
        np.testing.assert_allclose(jtl[col], -0.5 * fd, rtol=0, atol=1e-8 * max(1.0, np.abs(jtl).max()))


def test_weights_move_the_solution_and_all_ones_is_the_plain_loop():
    sc = pin_scene(*PIN_SCENES[0])
    fr, sem, opt = orc.Frame.from_scene(sc), lwm.sem_of(sc), orc.default_opt()
    plain = orc.lm(fr, opt)
    np.testing.assert_allclose(lwm.lm(fr, sem, opt, 0, 1.0), plain, rtol=0, atol=1e-12)     # pp_max = 1: every weight 1
    for mode, pp in ((1, 0.0), (2, 0.0), (0, 2e-5)):
        assert np.abs(lwm.lm(fr, sem, opt, mode, pp) - plain).max() > 1e-6
