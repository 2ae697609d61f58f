"""CPU pins of the surfel-sharded LM fixtures (lm_shard_cases.py): the share bounds, the per-share references and the property
every special scene is there for.  The device tests are test_gpu_lm_sharded.py."""
import numpy as np
import pytest

import lm_shard_cases as lc
import lm_weight_model as lwm
from oracle import lm_oracle as orc

_id = lambda c: c.id    # noqa: E731
SCENE_CFG = sorted({(c.scene, c.cfg) for c in lc.ALL_CASES}, key=str)
# the weighted traces whose accept flags hold a decisive reject followed by an accept: the truncation's.  (The hard and soft
# traces of these scenes accept until the loss stalls and reject only in their last, rounding-level iterations; their flags
# are compared where decisive, and the path behind a reject is carried by the traces below and the two reject goldens.)
REJECT_THEN_ACCEPT = [("k4", "trunc"), ("k6", "trunc"), ("a257", "trunc")]


def _N(name):
    return len(lc.frame(name).sf_points)


@pytest.mark.parametrize("case", lc.ALL_CASES, ids=_id)
def test_share_bounds_tile_the_frame(case):
    N = _N(case.scene)
    b = lc.bounds(N, case.world)
    assert b[0][0] == 0 and b[-1][1] == N and len(b) == case.world
    for (lo, hi), (lo2, _) in zip(b, b[1:]):
        assert lo <= hi == lo2
    owner = np.full(N, -1)
    for r, (lo, hi) in enumerate(b):
        assert (owner[lo:hi] == -1).all()
        owner[lo:hi] = r
    assert (owner >= 0).all()
    sizes = [hi - lo for lo, hi in b]
    assert max(sizes) - min(sizes) <= 1


@pytest.mark.parametrize("name,cfg", SCENE_CFG, ids=lambda v: str(v))
def test_share_losses_and_counts_sum_to_the_frames(name, cfg):
    """at identity and at the perturbed beta, for every world: counts exact, losses to 1e-12 relative; the model's conditions
    hold there (asserted inside)"""
    J = lc.scene(name).J
    for beta in (lc.identity(J), lc.perturbed(name)):
        matched = set(lc.conditions(name, cfg, beta).t.match.tolist())
        for W in lc.WORLDS:
            shares, (loss, count) = lc.share_losses(name, cfg, beta, W)
            assert sum(c for _, c in shares) == count == len(matched)
            np.testing.assert_allclose(sum(s for s, _ in shares), loss, rtol=1e-12, atol=0)
            for (lo, hi), (_, c) in zip(lc.bounds(_N(name), W), shares):
                assert c == len(matched & set(range(lo, hi)))


def test_model_at_weight_one_is_the_oracle():
    """the unweighted reference of the shares (lm_weight_model at seg_mode 0, pp_max 0) is oracle/lm_oracle.py's"""
    name = "k6"
    beta = lc.perturbed(name)
    A, b, M = lwm.normal_equations(lc.frame(name), None, beta, orc.default_opt())
    A0, b0, M0 = orc.normal_equations(lc.frame(name), beta, orc.default_opt())
    assert M == M0
    np.testing.assert_allclose(A, A0, rtol=0, atol=1e-12 * np.abs(A0).max())
    np.testing.assert_allclose(b, b0, rtol=0, atol=1e-12 * np.abs(b0).max())
    t = orc.data_term(lc.frame(name), beta, 1.0)
    np.testing.assert_allclose(lc.share_losses(name, None, beta, 2)[1][0], float((t.r ** 2).sum()), rtol=1e-14)


@pytest.mark.parametrize("K", [4, 6])
def test_empty_share_rank_0_of_4_matches_nothing_at_identity(K):
    name = f"hole{K}"
    sc = lc.scene(name)
    assert sc.N == 1200 and sc.sf_knn_idx.shape[1] == K
    shares, (_, count) = lc.share_losses(name, None, lc.identity(sc.J), 4)
    assert shares[0][1] == 0 and shares[0][0] == 0.0
    assert count > 600 and all(c > 0 for _, c in shares[1:])            # the frame as a whole still matches
    t = orc.data_term(lc.frame(name), lc.identity(sc.J), 1.0)
    assert t.match.min() >= 300 and sc.N - len(t.match) >= 300
    # a reordering: the same surfels as the scene it was made from
    src = lc._make(1200, 40, K, 60 + K, holes=0.1)
    assert sorted(map(tuple, sc.sf_points)) == sorted(map(tuple, src.sf_points))


def test_zero_weight_share_rank_0_of_4_matches_and_weighs_nothing():
    name = "zw4"
    sc = lc.scene(name)
    ww = lc.conditions(name, "hard", lc.identity(sc.J))
    lo, hi = lc.bounds(sc.N, 4)[0]
    mine = (ww.t.match >= lo) & (ww.t.match < hi)
    assert (lo, hi) == (0, 300) and mine.sum() == 300                   # every surfel of the share is matched ...
    assert not ww.w[mine].any()                                          # ... and weighs nothing
    assert int((ww.w == 0).sum()) >= sc.N // 4 and ww.w[~mine].sum() > 600
    shares, _ = lc.share_losses(name, "hard", lc.identity(sc.J), 4)
    assert shares[0] == (0.0, 300) and all(s > 0 for s, _ in shares[1:])


def test_aligned_and_inside_a_wave_bounds():
    assert [lo for lo, _ in lc.bounds(_N("a1024"), 4)] == [0, 256, 512, 768]
    assert [lo for lo, _ in lc.bounds(_N("a256"), 4)] == [0, 64, 128, 192]
    for name, W in (("a257", 2), ("a257", 3), ("n65", 2), ("n65", 3)):
        ends = [hi for _, hi in lc.bounds(_N(name), W)]
        assert all(hi % 64 for hi in ends) or (name, W) == ("a257", 2), (name, W, ends)      # (257 // 2 = 128: its other end, 257)
        assert ends[-1] % 64 == 1


def test_tiny_frames_have_empty_shares():
    assert lc.bounds(_N("t3"), 4) == [(0, 0), (0, 1), (1, 2), (2, 3)]
    assert lc.bounds(_N("t1"), 2) == [(0, 0), (0, 1)]
    assert lc.bounds(_N("t0"), 2) == [(0, 0), (0, 0)]
    for name in ("t3", "t1"):
        assert len(orc.data_term(lc.frame(name), lc.identity(12), 1.0).match) == _N(name)
    assert [what if isinstance(what, str) else what[0] for _, what in lc.TINY] == ["runs"] * 4 + ["bind"] * 2


@pytest.mark.parametrize("name,cfg", REJECT_THEN_ACCEPT)
def test_truncation_traces_hold_a_decisive_reject_followed_by_an_accept(name, cfg):
    _, trace = lc.model_trace(name, cfg)
    acc = np.array([t["accepted"] for t in trace])
    dec = lc.tw.decisive([t["loss"] for t in trace])
    rej = [i for i in range(len(acc) - 1) if dec[i] and not acc[i] and acc[i + 1:].any()]
    assert rej, (acc, dec)
    assert len({t["M_grad"] for t in trace}) > 1 or len({t["M_loss"] for t in trace}) > 1      # the counts move along the trace


def test_every_loop_case_with_a_weighted_trace_is_listed_or_ends_in_ties():
    """a weighted loop outside REJECT_THEN_ACCEPT has no decisive reject before an accept at all: nothing is compared loosely
    that could have been compared strictly"""
    for name, cfg in SCENE_CFG:
        if cfg is None or name == "t0" or (name, cfg) in REJECT_THEN_ACCEPT:
            continue
        _, trace = lc.model_trace(name, cfg)
        acc = np.array([t["accepted"] for t in trace])
        assert not [i for i in range(len(acc) - 1) if not acc[i] and acc[i + 1:].any()], (name, cfg, acc)
