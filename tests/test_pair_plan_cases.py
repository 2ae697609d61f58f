"""CPU pin of tests/pair_plan_cases.py and tests/pair_plan_model.py: every case builds with its claims, the model's block
bookkeeping is exact (records cut from the oracle's dense system and summed back reproduce its lower triangle and J^T r bit
for bit), sf_pidx agrees with blk_key, the shares of the world-2 and world-3 tests have a boundary inside a run, and the
inputs of the other users of pair_gram have the patterns they claim."""
import numpy as np
import pytest

import lm_weight_model as lwm
import pair_plan_cases as ppc
import pair_plan_model as ppm


@pytest.mark.parametrize("name", ppc.NAMES)
def test_case_builds_with_its_claims_and_the_model_is_consistent(name):
    c = ppc.case(name)                                            # (the builders assert what the name claims)
    p, sc = c.plan, c.scene
    assert sc.N <= 1500 and sc.J <= 64 and c.K == ppc.case_k(name) and sc.sf_knn_idx.shape == sc.sf_knn_w.shape
    w = sc.sf_knn_w
    assert (w > 0).all() and np.allclose(w.sum(1), 1.0, atol=1e-6) and all(len(set(r)) == c.K for r in w.tolist())
    if c.K > 1 and not name.startswith("shuffled"):
        assert not (np.diff(sc.sf_knn_idx, axis=1) > 0).all(1).any()
    # the plan: keys ascending and distinct, every slot's pair found, the order a permutation sorted by the full tuple
    assert p.blk_key.dtype == np.uint32 and (np.diff(p.blk_key.astype(np.int64)) > 0).all() and (p.key_a >= p.key_b).all()
    ra, rb = ppm.slots(c.K)
    assert (p.key_a[p.sf_pidx] == p.c[:, ra]).all() and (p.key_b[p.sf_pidx] == p.c[:, rb]).all()
    assert sorted(p.sf_perm.tolist()) == list(range(p.N))
    cs = [tuple(r) + (int(i),) for r, i in zip(p.c[p.sf_perm].tolist(), p.sf_perm.tolist())]
    assert cs == sorted(cs)
    for which in ppc.betas(sc.J):
        A, jtl, M = c.system(which)
        assert M > 0 and M == int(c.match(ppc.betas(sc.J)[which]).sum()) and ppm.covered(p, A)
        assert M == sc.N - (0 if c.off is None else int(c.off.sum()))
        rec = ppm.records_of(p, A, jtl)
        L, g = ppm.dense_of(p, rec)
        np.testing.assert_array_equal(L, np.tril(A))
        np.testing.assert_array_equal(g, -jtl)
        off_diag = p.key_a != p.key_b
        assert (rec[off_diag, 49:] == 0).all() and np.abs(rec).max() > 0


@pytest.mark.parametrize("name", ppc.SHARED)
@pytest.mark.parametrize("world", (2, 3))
def test_shares_split_a_run_and_sum_to_the_frame(name, world):
    c = ppc.case(name)
    assert ppc.boundary_inside_a_run(c, world)
    A, jtl, M = c.system("perturbed")
    parts = [c.system("perturbed", lo, hi) for lo, hi in ppc.bounds(c.plan.N, world)]
    assert sum(p[2] for p in parts) == M
    np.testing.assert_allclose(sum(p[0] for p in parts), A, rtol=0, atol=1e-12 * np.abs(A).max())
    np.testing.assert_allclose(sum(p[1] for p in parts), jtl, rtol=0, atol=1e-12 * max(1.0, np.abs(jtl).max()))


@pytest.mark.parametrize("name", ppc.OTHER_USERS)
def test_inputs_of_the_other_users_of_the_run_gram(name):
    c = ppc.case(name)
    J = c.scene.J
    on = c.match(ppc.perturbed(J))
    pat = ppc.edge_pattern(c)
    runs = ppm.runs_in_perm(c.plan, on)
    onp, patp = on[c.plan.sf_perm], pat[c.plan.sf_perm]
    starts = np.array([np.nonzero(onp[a:b])[0][0] + a for _, a, b, _ in runs])
    ends = np.array([np.nonzero(onp[a:b])[0][-1] + a for _, a, b, _ in runs])
    assert (~patp[starts]).sum() >= 5 and (~patp[ends]).sum() >= 5        # "off" at run starts and at run ends
    sem, pat2 = ppc.hard_sem(c)
    ww = lwm.weights(c.fr, sem, ppc.perturbed(J), 1)
    lwm.check_conditions(ww, 1, 0.0)
    assert (ww.w == pat2[ww.t.match]).all() and (ww.w == 0).sum() >= 5      # hard weight 0 exactly where the pattern says
    (tri, areas), plan = ppc.face_mesh(c)
    assert plan.tri_pidx.shape == (24, 6) and (areas > 0).all()
    tp = ppm.tri_pairs(tri)
    assert (plan.key_a[plan.tri_pidx] == tp[..., 0]).all() and (plan.key_b[plan.tri_pidx] == tp[..., 1]).all()
    assert np.array_equal(plan.sf_perm, c.plan.sf_perm)


def test_batches_hold_unlike_cases_of_one_k():
    for K, names in ppc.BATCHES.items():
        cs = [ppc.case(n) for n in names]
        assert all(c.K == K for c in cs) and len({c.scene.N for c in cs}) == 3 and len({c.scene.J for c in cs}) == 1
    assert any(not ppc.case(n).state_f64 for n in ppc.NAMES)
