"""What test_gpu_graphfit_sharded.py relies on, pinned on the CPU so that a fixture cannot degrade silently: the shard bounds,
the morphing term's kept counts per shard (they sum to the frame's; some shards keep nothing, one has no candidate), shard
edges inside a staging group, a wave and a workgroup and edges at multiples of 256, the stability masks meeting the edges, the
per-rank reference summing to the frame's, and every new ten-step case being well conditioned (as in test_gf_shape_cases.py:
the oracle's result moves by less than 1e-3 of the GPU tolerance when its surfels are summed in another order)."""
import numpy as np
import pytest

import gf_shape_cases as cases
import gf_shard_cases as shard
from oracle import graphfit_oracle as gfo

_id = lambda c: c.id    # noqa: E731


def test_bounds_follow_n_r_over_w():
    assert shard.bounds(3000, 3) == [(0, 1000), (1000, 2000), (2000, 3000)]
    assert shard.bounds(3000, 4) == [(0, 750), (750, 1500), (1500, 2250), (2250, 3000)]
    assert shard.bounds(257, 2) == [(0, 128), (128, 257)]
    assert shard.bounds(257, 3) == [(0, 85), (85, 171), (171, 257)]
    assert shard.bounds(1024, 4) == [(0, 256), (256, 512), (512, 768), (768, 1024)]
    assert shard.bounds(3, 4) == [(0, 0), (0, 1), (1, 2), (2, 3)]
    assert shard.bounds(0, 2) == [(0, 0), (0, 0)]
    assert shard.bounds(15, 3)[2] == (10, 15) and shard.bounds(15, 2)[1] == (7, 15)
    for sc in shard.SHARDED:
        b = shard.bounds(sc.case.N, sc.world)
        assert b[0][0] == 0 and b[-1][1] == sc.case.N and all(b[r][1] == b[r + 1][0] for r in range(sc.world - 1))
        masks = [shard.shard_mask(sc.case, r, sc.world) for r in range(sc.world)]
        st = cases.stable_of(sc.case)
        np.testing.assert_array_equal(np.sum(masks, axis=0), np.ones(sc.case.N) if st is None else st)


def test_the_table_has_every_family_at_every_world_and_the_named_cases():
    ids = {sc.id for sc in shard.SHARDED}
    assert len(ids) == len(shard.SHARDED)
    assert shard.MORPH_TAGS == ("soft", "softadam", "morph")
    for tag in shard.FAMILY_TAGS:
        for W in (2, 3, 4):
            assert shard.ShardCase(shard.family_case(tag), W) in shard.SHARDED
    assert shard.family_case("corr").flow and shard.family_case("corrpp").flow and shard.family_case("soft").semantic
    assert {sc.case.tag for sc in shard.SHORT_LIST} == {"soft", "morph", "softadam"}
    assert all(sc.case.short_list for sc in shard.SHORT_LIST) and shard.PROCGROUP in shard.SHARDED
    assert (shard.PROCGROUP.case.tag, shard.PROCGROUP.world) == ("softadam", 2)
    assert any(sc.morph and sc.case.K == 6 for sc in shard.SHARDED)
    assert {sc.case.mask for sc in shard.MASKED} == {"random", "groups"}
    assert any(sc.state == "f32" for sc in shard.SHARDED)
    assert {(sc.case.N, sc.world) for sc in shard.DEGENERATE} == {(3, 4), (0, 2)}
    assert all(sc.world <= 4 for sc in shard.SHARDED)        # W handles and the unsharded one: five at most
    assert not any(sc.morph for sc in shard.GRAD_CASES) and len(shard.GRAD_CASES) >= 7 * 3


MORPH_SHARDED = [sc for sc in shard.SHARDED if sc.morph and sc.state is None]


@pytest.mark.parametrize("sc", MORPH_SHARDED, ids=_id)
def test_kept_counts_of_the_shards_sum_to_the_frames(sc):
    for name, dv in (("identity", shard.identity(sc.case)), ("perturbed", cases.perturbed_dv(sc.case))):
        cand, kept = shard.morph_counts(sc.case, dv)
        per = [shard.morph_counts(sc.case, dv, shard.shard_mask(sc.case, r, sc.world)) for r in range(sc.world)]
        print(sc.id, name, "frame (candidates, kept)", (cand, kept), "per shard", per)
        assert sum(p[0] for p in per) == cand and sum(p[1] for p in per) == kept
    want = shard.KEPT_TABLE.get((sc.case.id, sc.world))
    if want is not None:
        assert tuple(p[1] for p in per) == want and kept == sum(want) > 0
    if sc.case.N >= 257:
        assert kept > 0


def test_some_shards_keep_nothing_and_one_has_no_candidate():
    assert {k for k, v in shard.KEPT_TABLE.items() if 0 in v and sum(v) > 0} == set(shard.KEPT_TABLE)
    assert all(shard.ShardCase(c, W) in shard.SHARDED for c in cases.SHORT_LIST[:1] for W in (3, 4))
    short = cases.SHORT_LIST[0]
    dv = cases.perturbed_dv(short)
    assert shard.morph_counts(short, dv, shard.shard_mask(short, 0, 3)) == (9, 0)      # candidates, none kept
    assert shard.morph_counts(short, dv, shard.shard_mask(short, 0, 4)) == (0, 0)      # not one candidate
    # also at identity, where the ten steps start
    assert shard.morph_counts(short, shard.identity(short), shard.shard_mask(short, 0, 4))[1] == 0
    assert shard.morph_counts(short, shard.identity(short))[1] > 0


def test_shard_edges_fall_inside_groups_waves_and_workgroups_and_on_multiples_of_256():
    inner = lambda sc: [b[0] for b in shard.bounds(sc.case.N, sc.world)[1:]]    # noqa: E731
    for sc in shard.FAMILIES:
        e = inner(sc)
        if sc.world == 2:
            assert e == [1500] and e[0] % 16 == 12 and e[0] % 64 and e[0] % 256
        else:
            assert any(x % 16 for x in e) and all(x % 256 for x in e)
    assert inner(shard.ALIGNED[0]) == [256, 512, 768]
    assert [x % 16 for x in inner(shard.FEW_KEPT[1])] == [5, 11]
    # the masks meet the edges: in the wave that holds an edge the in-shard side has stable and unstable surfels
    for sc in shard.MASKED:
        st = cases.stable_of(sc.case)
        met = 0
        for r in range(1, sc.world):
            lo = shard.bounds(sc.case.N, sc.world)[r][0]
            wave_end = (lo // 64 + 1) * 64
            met += bool(st[lo:wave_end].any() and not st[lo:wave_end].all())
        print(sc.id, "edges whose wave has stable and unstable in-shard surfels:", met)
        assert met >= 1 and any(x % 16 for x in inner(sc))


@pytest.mark.parametrize("sc", [s for s in shard.GRAD_CASES if s.state is None], ids=_id)
def test_the_ranks_references_sum_to_the_frames(sc):
    """oracle_partial is the per-rank reference of the gradient check: its sum over the ranks is the frame's gradient."""
    case, W = sc.case, sc.world
    terms, loss, gref, _ = cases.oracle_grad(case)
    parts = [shard.oracle_partial(case, r, W) for r in range(W)]
    g = np.sum([p[1] for p in parts], axis=0)
    g[-1] /= case.J
    t = np.sum([p[0] for p in parts], axis=0)
    err = np.abs(g - gref).max()
    print(sc.id, "sum of the ranks' gradients - frame's", err, "max|g|", np.abs(gref).max(), "matched", terms.get("_matched"))
    assert err <= 1e-13 * max(1.0, np.abs(gref).max())
    np.testing.assert_allclose(t, shard.terms_vector(case, cases.perturbed_dv(case)), rtol=1e-12, atol=0)
    assert t[shard.T_PP_KEPT] == terms["_matched"] and (terms["_matched"] > 0 or case.N == 0)
    if case.flow:
        assert t[shard.T_CORR_KEPT] == terms["_corr_matched"] > 0
    for r in range(1, W):
        assert not parts[r][0][list(shard.NODE_TERMS)].any()
        assert not parts[r][1][~shard.touched_rows(case, r, W)].any()
    if case.N >= 3000:       # a third of the image touches a part of the nodes only: the untouched rows are a real check
        assert any((~shard.touched_rows(case, r, W)[:-1]).sum() >= 4 for r in range(1, W))


def test_the_resharding_frames():
    tiny = shard.RESHARD_TINY
    assert tiny in cases.EDGE and shard.bounds(tiny.N, 3)[2] == (10, 15)      # one wave, one staging round
    v, g = shard.oracle_partial(tiny, 2, 3)
    assert v[shard.T_PP_KEPT] >= 3 and np.abs(g).max() > 0
    assert shard.ShardCase(shard.RESHARD_LARGE, 3) in shard.SHARDED


NEW_TEN_STEP = [c for c in dict.fromkeys(sc.case for sc in shard.SHARDED) if c not in cases.TEN_STEP_CASES]


@pytest.mark.parametrize("case", NEW_TEN_STEP, ids=_id)
def test_ten_steps_of_the_oracle_do_not_depend_on_the_summation_order(case):
    sc = cases.scene_of(case)
    want = cases.oracle_final(case)
    assert np.isfinite(want).all() and cases.step_of(want) > 1e-6
    st = cases.stable_of(case)
    p = cases.surfel_perm(sc.N, 1)
    other = gfo.graphfit(gfo.Problem(cases.shuffle_surfels(sc, 1), stable=None if st is None else st[p]), cases.opt_of(case.tag))
    err, tol = np.abs(other - want).max(), cases.dv_atol(case)
    print(case.id, "step", cases.step_of(want), "GPU atol", tol, "order sensitivity", err)
    assert err < 1e-3 * tol
