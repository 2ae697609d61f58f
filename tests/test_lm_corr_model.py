"""The float64 model of the LM path's flow-correspondence term (tests/lm_corr_model.py) checked on the CPU: its Jacobian
against central differences, its targets and loss against ``graphfit_oracle.corr_term`` and the reference-recorded losses
of ``s60x80_j48_corr``, and the properties the GPU tests rely on (non-trivial kept counts, the term moves the solution, a
named configuration whose trace holds a reject followed by an accept)."""
import numpy as np
import pytest
import torch

import lm_corr_model as lcm
from helpers import GF_CORR_VARIANTS, load_corr_golden, load_golden
from oracle import graphfit_oracle as gfo
from oracle import lm_oracle as orc
from super_amd import synth

# the second scene of the GPU tests (tests/test_gpu_graphfit_corr.py uses the same one)
SCENE2 = dict(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3, tgt_holes=0.02)
FLOW2 = dict(seed=7, amp=(2.5, 1.8))

# The configuration whose LM trace holds a reject followed by an accept (asserted below and run on the GPU in
# tests/test_gpu_lm_corr.py): the scene of the reject fixture s60x80_j48_reject with a smooth flow, point-point, weight 0.3,
# the default damping.  Its trace is five accepts, four rejects, one accept, none of them a rounding-level tie.
REJECT_CASE = dict(golden="s60x80_j48_reject", flow=dict(seed=7, amp=(2.5, 1.8)), mode=1, lam=0.3, u=10.0, v=7.5)


def scene2():
    sc = synth.make_scene(**SCENE2)
    sc.flow = synth.smooth_flow(sc.H, sc.W, FLOW2["seed"], amp=FLOW2["amp"])
    return sc


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("K", [3, 4, 6])
def test_jacobian_matches_central_differences(K, mode):
    sc = synth.make_scene(N=400, J=24, H=60, W=80, seed=50 + K, n_neighbors=K, src_border=3, tgt_border=3)
    flow = synth.smooth_flow(sc.H, sc.W, 3, amp=(2.0, 1.5))
    fr = orc.Frame.from_scene(sc)
    tg = lcm.targets_from_flow(fr, flow)
    assert 50 < tg[2].sum() < sc.N
    beta = lcm.random_beta(sc.J, 5)
    lam = 0.7
    Jc, r = lcm.corr_jacobian(fr, beta, tg, mode, lam)
    assert Jc.shape[0] == (3 if mode == 1 else 1) * tg[2].sum() == len(r)
    Jd = Jc.toarray()
    rng = np.random.default_rng(1)
    h = 1e-6
    for col in rng.choice(7 * sc.J, 25, replace=False):
        d = np.zeros(7 * sc.J)
        d[col] = h
        rp = lcm.corr_term(fr, beta + d.reshape(-1, 7), tg, mode, lam).r
        rm = lcm.corr_term(fr, beta - d.reshape(-1, 7), tg, mode, lam).r
        np.testing.assert_allclose(Jd[:, col], (rp - rm) / (2 * h), rtol=0, atol=1e-8 * max(1.0, np.abs(Jd).max()))


@pytest.mark.parametrize("tag,mode", [("corr", 1), ("corrpp", 2)])
def test_identity_loss_equals_graphfit_oracle_and_reference(tag, mode):
    g, sc = load_corr_golden()
    fr = orc.Frame.from_scene(sc)
    tg = lcm.targets_from_flow(fr, sc.flow)
    ident = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (sc.J, 1))
    mine, kept = lcm.corr_loss(fr, ident, tg, mode, 1.0)
    pb = gfo.Problem(sc)
    dv = torch.zeros((sc.J + 1, 7), dtype=torch.float64)
    dv[:, 0] = 1.0
    # GraphFit's term at zero deformation: sf = the surfels skinned with identity warps, p sum_k w_k.  The fixture's
    # weights are float32 (their sum is 1 to 3e-8), so that is p scaled -- the projection, and with it every target, is
    # the one of p itself, and T(identity) of the LM path is the same sum: 1e-12 relative.  (With sf = p exactly the two
    # differ by the scale: 2.4e-8 point-point, 1.4e-7 point-plane.)
    ref, m = gfo.corr_term(pb, gfo.deform(pb, dv)[1], GF_CORR_VARIANTS[tag]["sf_corr_loss_type"])
    assert kept == m == 1274 and sc.N == 1500
    np.testing.assert_allclose(mine, float(ref), rtol=1e-12)
    rec = float(g[f"gf_{tag}_term_corr_loss"])
    rel = abs(mine * GF_CORR_VARIANTS[tag]["sf_corr_weight"] - rec) / rec
    print(tag, "relative difference to the reference-recorded loss:", rel)
    assert rel < 1e-6


def test_kept_counts_and_tie_share():
    g, sc = load_corr_golden()
    for s, flow, want in ((sc, sc.flow, (1274, 1500)), (scene2(), None, (2377, 3000))):
        flow = s.flow if flow is None else flow
        fr = orc.Frame.from_scene(s)
        _, _, valid = lcm.targets_from_flow(fr, flow)
        assert (int(valid.sum()), s.N) == want
        # surfels within 1e-4 px of an integer / a margin may fall on either side on a device: at most 1 %
        share = float((lcm.tie_distance(fr, flow) <= 1e-4).mean())
        print("share within 1e-4 px of an integer:", share)
        assert share <= 0.01


@pytest.mark.parametrize("mode", [1, 2])
def test_term_moves_the_solution(mode):
    g, sc = load_corr_golden()
    fr = orc.Frame.from_scene(sc)
    opt = orc.default_opt()
    tg = lcm.targets_from_flow(fr, sc.flow)
    with_term = lcm.lm_with_corr(fr, opt, tg, mode, 1.0)
    without = lcm.lm_with_corr(fr, opt, None, mode, 1.0)
    np.testing.assert_allclose(without, orc.lm(fr, opt), rtol=0, atol=0)     # the loop is lm_oracle.lm's
    assert np.abs(with_term - without).max() > 1e-6


def reject_case_scene():
    c = REJECT_CASE
    _, sc, opt = load_golden(c["golden"])
    sc.flow = synth.smooth_flow(sc.H, sc.W, c["flow"]["seed"], amp=c["flow"]["amp"])
    return sc, opt


def reject_case_trace():
    c = REJECT_CASE
    sc, opt = reject_case_scene()
    fr = orc.Frame.from_scene(sc)
    tg = lcm.targets_from_flow(fr, sc.flow)
    trace = []
    beta = lcm.lm_with_corr(fr, opt, tg, c["mode"], c["lam"], u=c["u"], v=c["v"], trace=trace)
    return sc, opt, tg, beta, trace


def decisive(losses):
    """iterations whose accept decision is not a rounding-level tie (tests/test_gpu_parity.py)"""
    losses = np.asarray(losses)
    best = np.minimum.accumulate(np.concatenate([[1e10], losses]))[:-1]
    return np.abs(losses - best) > 1e-9 * np.abs(best)


def test_reject_case_holds_a_reject_followed_by_an_accept():
    _, _, _, _, trace = reject_case_trace()
    acc = [t["accepted"] for t in trace]
    dec = decisive([t["loss"] for t in trace])
    print(acc, dec)
    assert len(acc) == 10
    assert any((not a) and b and da and db for a, b, da, db in zip(acc, acc[1:], dec, dec[1:]))
