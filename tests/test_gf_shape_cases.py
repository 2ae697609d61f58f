"""What test_gpu_graphfit_shapes.py relies on, pinned on the CPU so that a fixture cannot degrade silently: the relabelled scene
really collides in k_gf_data's gradient table, the short-list scene really has a boundary list shorter than a wave and
workgroups full of candidates, the relabelling is a pure renaming for the oracle, every edge case has a triangle and a match,
and every ten-step case is well conditioned: the oracle's own result moves by less than 1e-3 of the GPU tolerance when its
surfels are summed in another order (a case that fails that gets another seed, never a wider tolerance)."""
import numpy as np
import pytest
import torch

import gf_shape_cases as cases
from oracle import graphfit_oracle as gfo
from super_amd import synth


@pytest.mark.parametrize("K,at_least", [(2, 50), (4, 100), (8, 150)])
def test_relabelled_scene_collides_in_every_workgroup(K, at_least):
    """Counted: 85 / 108 / 179 nodes at K = 2 / 4 / 8; the bounds sit below them so that a change of the scene generator that
    keeps the property does not fail here."""
    case = next(c for c in cases.COLLISION if c.K == K)
    sc = cases.scene_of(case)
    row_major = synth.make_scene(N=3000, J=300, H=60, W=80, seed=21, n_neighbors=K, src_border=5, tgt_border=3, tgt_holes=0.01)
    assert cases.fallback_nodes(row_major.sf_knn_idx) == (0, 0)
    np.testing.assert_array_equal(sc.sf_knn_idx, np.random.default_rng(1).permutation(300)[row_major.sf_knn_idx])
    nodes, blocks = cases.fallback_nodes(sc.sf_knn_idx)
    print("K", K, "fallback nodes", nodes, "blocks", blocks)
    assert blocks == 12 == (sc.N + 255) // 256
    assert nodes >= at_least
    # with the unstable surfels taken out the stable ones alone still collide in every workgroup
    assert cases.fallback_nodes(sc.sf_knn_idx, cases.stable_of(case))[1] == 12
    sem = cases.scene_of(cases.COLLISION[-1])
    assert sem.num_classes == 3      # the semantic scene has the K = 4 scene's nodes and surfels
    assert cases.fallback_nodes(sem.sf_knn_idx) == cases.fallback_nodes(cases.scene_of(cases.COLLISION[2]).sf_knn_idx)


def test_fallback_nodes_counts_by_block():
    idx = np.zeros((512, 2), np.int64)
    idx[:256] = [3, 131]           # 3 and 131 share slot 3
    idx[256:] = [3, 4]
    idx[300] = [4 + 128, 4 + 256]  # two more on slot 4
    assert cases.fallback_nodes(idx) == (3, 2)
    assert cases.fallback_nodes(idx[256:300]) == (0, 0)


def test_short_list_scene_has_a_short_list_and_full_workgroups_of_candidates():
    sc = cases.short_list_scene()
    lists = [len(e) for e in gfo.edge_points(sc.img_seg, 3)]
    pb = gfo.Problem(sc)
    dv = torch.zeros((sc.J + 1, 7), dtype=torch.float64)
    dv[:, 0] = 1.0
    _, sf = gfo.deform(pb, dv)
    assert gfo.bn_morph(pb, sf) is not None
    stats = {c: (n_list, cand, kept) for c, n_list, cand, kept in pb.morph_stats}
    print("lists", lists, "stats", stats)
    assert 2 <= lists[2] <= 63 and lists[0] >= 64 and lists[1] >= 64
    assert stats[2][0] == lists[2] and stats[2][2] > 0 and stats[1][2] > 0
    cand = pb.morph_candidates.numpy()           # (every surfel is stable: the mask is by surfel row)
    assert cand.sum() == stats[1][1] + stats[2][1]
    full = [b for b in range(0, sc.N - 255, 256) if cand[b:b + 256].all()]
    print("class 2 candidates", stats[2][1], "kept", stats[2][2], "full workgroups at", full)
    assert len(full) >= 1


@pytest.mark.parametrize("case", [cases.COLLISION[2], cases.COLLISION[-1]], ids=lambda c: c.id)
def test_relabelling_is_a_pure_renaming_for_the_oracle(case):
    perm = cases.relabel_perm(case.J)
    dv = cases.perturbed_dv(case)
    t1, loss1, g1, _ = cases.oracle_grad(case)
    t0, loss0, g0, _ = cases.oracle_grad_at(case, cases.unpermute_rows(dv, perm), cases.scene_of(case, relabel=False))
    err = np.abs(cases.unpermute_rows(g1, perm) - g0).max()
    print("relabel: |g_relabelled[perm] - g| max", err, "|g| max", np.abs(g0).max())
    assert t1["_matched"] == t0["_matched"] > 0
    assert abs(loss1 - loss0) <= 1e-14 * abs(loss0)
    assert err < 1e-14


@pytest.mark.parametrize("case", cases.EDGE, ids=lambda c: c.id)
def test_edge_cases_have_a_triangle_and_a_match(case):
    sc = cases.scene_of(case)
    assert (sc.N, sc.J, sc.sf_knn_idx.shape[1], sc.ed_knn_idx.shape[1]) == (case.N, case.J, case.K, min(4, case.J - 1))
    assert sc.ed_triangles.shape[1] >= 1
    t, _, g, _ = cases.oracle_grad(case)
    assert t["_matched"] > 0 and np.isfinite(g).all()
    st = cases.stable_of(case)
    if case.mask == "groups":
        assert not st[256:512].any() and not st[576:640].any() and not st[0:16].any() and st[16:48].all()
        assert t["_matched"] <= st.sum() < sc.N


def test_batch_maxima_come_from_different_slots():
    for tag, K in cases.BATCH_VARIANTS:
        bc = cases.batch_cases(tag, K)
        scs = [cases.scene_of(c) for c in bc]
        assert [s.N for s in scs] == [3000, 16, 2100, 257] and [s.J for s in scs] == [12, 300, 140, 12]
        assert int(np.argmax([s.N for s in scs])) == 0
        assert int(np.argmax([s.J for s in scs])) == 1 == int(np.argmax([s.ed_triangles.shape[1] for s in scs]))
        assert len({c.seed for c in bc}) == 4
        assert all(s.sf_knn_idx.shape[1] == K for s in scs)
        for c in bc:
            t = cases.oracle_grad(c)[0]
            assert t["_matched"] > 0 and (not c.flow or t["_corr_matched"] > 0)


@pytest.mark.parametrize("case", list(dict.fromkeys(cases.TEN_STEP_CASES)), ids=lambda c: c.id)
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
