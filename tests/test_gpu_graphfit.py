"""HIP GraphFit (autograd path with hand-derived gradients) vs the reference's goldens and
the PyTorch-CPU oracle, through the C ABI.  Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

from gf_shape_cases import frames_of
from helpers import GF_SEMANTIC_VARIANTS, load_golden, ref_opt, torch_frame
from oracle import graphfit_oracle as gfo

pytestmark = pytest.mark.gpu

CASES = [("s60x80_j48", "sgd"), ("s60x80_j48", "adam"), ("s60x80_j48", "sgdface"),
         ("s60x80_j48_reject", "sgd"), ("s60x80_j48_reject", "adam")]
# num_neighbors = 6 (round 6; deform_source / get_losses are K-generic in the reference: super/deform_mesh.py:198-230)
CASES += [("s60x80_j48_k6", "sgd"), ("s60x80_j48_k6", "adam"), ("s60x80_j48_k6", "sgdface")]
CASES += [("s60x80_j48_semantic", t) for t in GF_SEMANTIC_VARIANTS]   # Semantic-SuPer terms (configs[4])


def _opt(tag, **kw):
    if tag in GF_SEMANTIC_VARIANTS:
        o = gfo.default_opt(**GF_SEMANTIC_VARIANTS[tag], **kw)
        o.deform_udpate_method, o.num_classes = "super_edg", 3
        return o
    o = gfo.default_opt(optimizer="Adam" if tag == "adam" else "SGD", mesh_face=(tag == "sgdface"), **kw)
    o.deform_udpate_method = "super_edg"
    return o


def _frame(sc):
    inputs, sf, new_data = frames_of(sc)
    return sf, inputs, new_data


@pytest.mark.parametrize("name,tag", CASES)
def test_loss_and_gradient_at_identity_match_reference(name, tag):
    import torch
    from super_amd.deform_mesh import GraphFit
    g, sc, _ = load_golden(name)
    sf, inputs, new_data = _frame(sc)
    gf = GraphFit(_opt(tag))
    dv = torch.zeros((sc.J + 1, 7), dtype=torch.float64, device="cuda")
    dv[:, 0] = 1.0
    terms, matched, grad = gf.loss_and_grad(inputs, sf, new_data, dv)
    for k, v in terms.items():
        key = f"gf_{tag}_term_{k}"
        if key in g.files:
            np.testing.assert_allclose(v, float(g[key]), rtol=1e-9, atol=1e-15)
    assert abs(sum(terms.values()) - float(g[f"gf_{tag}_loss0"])) <= 1e-9 * abs(float(g[f"gf_{tag}_loss0"]))
    ref = g[f"gf_{tag}_grad0"]
    np.testing.assert_allclose(grad.cpu().numpy(), ref, rtol=0, atol=1e-9 * max(1.0, np.abs(ref).max()))
    assert matched > 0


@pytest.mark.parametrize("name,tag", CASES)
def test_final_deform_verts_match_reference(name, tag):
    from super_amd.deform_mesh import GraphFit
    g, sc, _ = load_golden(name)
    sf, inputs, new_data = _frame(sc)
    dv = GraphFit(_opt(tag))(inputs, sf, new_data, None).cpu().numpy()
    np.testing.assert_allclose(dv, g[f"gf_{tag}_final"], rtol=0, atol=1e-9)   # north_star bar: 1e-4


def test_semantic_edge_points_match_find_edge_region():
    """Class-boundary pixels extracted on the device == the oracle's restatement of
    find_edge_region (bit-exact, same row-major order)."""
    import torch
    from super_amd.deform_mesh import GraphFit
    g, sc, _ = load_golden("s60x80_j48_semantic")
    sf, inputs, new_data = _frame(sc)
    gf = GraphFit(_opt("soft"))
    dv = torch.zeros((sc.J + 1, 7), dtype=torch.float64, device="cuda")
    dv[:, 0] = 1.0
    gf.loss_and_grad(inputs, sf, new_data, dv)
    ref = gfo.edge_points(sc.img_seg, 3)
    assert gf.edge_counts == [len(e) for e in ref]
    for c in range(3):
        np.testing.assert_array_equal(gf.edge_points(c).cpu().numpy(), ref[c].numpy().astype(np.float32))


@pytest.mark.parametrize("tag,num_neighbors", [pytest.param("soft", 4, id="soft"), pytest.param("hard", 4, id="hard"),
                                               pytest.param("morph", 4, id="morph"), ("soft", 3), ("soft", 6)])
def test_semantic_gradient_at_random_point_vs_autograd_oracle(tag, num_neighbors):
    """Semantic weights / morphing term away from identity, with unstable surfels, against
    torch autograd on the oracle.  At num_neighbors != 4 k_gf_morph skins with the run-time-K routine: "soft" weighs the
    morphing term 0.1, where it dominates the loss, so a wrong deformed position there cannot hide under the tolerance."""
    import torch
    from super_amd import synth
    from super_amd.deform_mesh import GraphFit
    K = num_neighbors
    if K == 4:
        sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=23, src_border=5, tgt_border=3, tgt_holes=0.01,
                              semantic=True)
        rng = np.random.default_rng(5)
    else:
        sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=40 + K, n_neighbors=K, src_border=5, tgt_border=3,
                              tgt_holes=0.01, semantic=True)
        rng = np.random.default_rng(K)
    dv0 = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (sc.J + 1, 1))
    dv0 += np.concatenate([rng.normal(0, 0.01, (sc.J + 1, 4)), rng.normal(0, 0.003, (sc.J + 1, 3))], axis=1)
    opt = _opt(tag)
    stable = rng.uniform(size=sc.N) > 0.1
    pb = gfo.Problem(sc, stable=stable)
    dvt = torch.from_numpy(dv0.copy()).requires_grad_(True)
    loss, terms = gfo.total_loss(pb, dvt, opt)
    if K != 4:
        assert float(terms["sf_bn_morph_loss"].detach()) != 0.0 and terms["_matched"] != 0
    gref, = torch.autograd.grad(loss, dvt)
    gref = gref.clone()
    gref[-1] /= sc.J
    sf, inputs, new_data = _frame(sc)
    sf.isStable = torch.from_numpy(stable).cuda()
    t, matched, grad = GraphFit(opt).loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv0).cuda())
    assert matched == terms["_matched"]
    for k, v in t.items():
        if k in terms:
            np.testing.assert_allclose(v, float(terms[k].detach()), rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(sum(t.values()), float(loss.detach()), rtol=1e-9)
    np.testing.assert_allclose(grad.cpu().numpy(), gref.numpy(), rtol=0,
                               atol=1e-9 * max(1.0, float(gref.abs().max())))


def test_gradient_at_random_point_vs_autograd_oracle():
    """Away from identity (global row active, face term on) against torch autograd."""
    import torch
    from super_amd import synth
    from super_amd.deform_mesh import GraphFit
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=21, src_border=5, tgt_border=3, tgt_holes=0.01)
    rng = np.random.default_rng(3)
    dv0 = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (sc.J + 1, 1))
    dv0 += np.concatenate([rng.normal(0, 0.01, (sc.J + 1, 4)), rng.normal(0, 0.003, (sc.J + 1, 3))], axis=1)
    opt = _opt("sgdface")
    stable = rng.uniform(size=sc.N) > 0.1
    pb = gfo.Problem(sc, stable=stable)
    dvt = torch.from_numpy(dv0.copy()).requires_grad_(True)
    loss, terms = gfo.total_loss(pb, dvt, opt)
    gref, = torch.autograd.grad(loss, dvt)
    gref = gref.clone()
    gref[-1] /= sc.J
    sf, inputs, new_data = _frame(sc)
    sf.isStable = torch.from_numpy(stable).cuda()
    t, matched, grad = GraphFit(opt).loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv0).cuda())
    assert matched == terms["_matched"]
    np.testing.assert_allclose(sum(t.values()), float(loss.detach()), rtol=1e-10)
    np.testing.assert_allclose(grad.cpu().numpy(), gref.numpy(), rtol=0,
                               atol=1e-9 * max(1.0, float(gref.abs().max())))


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_gradient_and_ten_steps_at_other_num_neighbors_vs_autograd_oracle(K):
    """k_gf_data's row pass has a form per num_neighbors range (K <= 2: four entry-lane groups, 3..4: two + rows formed by all
    lanes at once, >= 5: one group, rows formed inside the staging rounds): the gradient away from identity against torch
    autograd and ten Adam steps against the oracle's optimiser, at a K of every range (4 and 6 have reference goldens)."""
    import torch
    from super_amd import synth
    from super_amd.deform_mesh import GraphFit
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=30 + K, n_neighbors=K, src_border=5, tgt_border=3, tgt_holes=0.01)
    rng = np.random.default_rng(K)
    dv0 = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (sc.J + 1, 1))
    dv0 += np.concatenate([rng.normal(0, 0.01, (sc.J + 1, 4)), rng.normal(0, 0.003, (sc.J + 1, 3))], axis=1)
    opt = _opt("adam")
    stable = rng.uniform(size=sc.N) > 0.1
    pb = gfo.Problem(sc, stable=stable)
    dvt = torch.from_numpy(dv0.copy()).requires_grad_(True)
    loss, terms = gfo.total_loss(pb, dvt, opt)
    gref, = torch.autograd.grad(loss, dvt)
    gref = gref.clone()
    gref[-1] /= sc.J
    sf, inputs, new_data = _frame(sc)
    sf.isStable = torch.from_numpy(stable).cuda()
    gf = GraphFit(opt)
    t, matched, grad = gf.loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv0).cuda())
    assert matched == terms["_matched"] and matched > 0
    np.testing.assert_allclose(sum(t.values()), float(loss.detach()), rtol=1e-10)
    np.testing.assert_allclose(grad.cpu().numpy(), gref.numpy(), rtol=0, atol=1e-9 * max(1.0, float(gref.abs().max())))
    want = gfo.graphfit(pb, opt)
    got = GraphFit(opt)(inputs, sf, new_data, None).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_update_autograd_variant_matches_reference():
    import torch
    from super_amd import nodes
    g, sc, opt = load_golden("s60x80_j48")
    sf, _, _ = torch_frame(sc)
    sf.opt = ref_opt(opt)
    sf.opt.use_derived_gradient = False
    nodes.update(sf, torch.from_numpy(g["gf_sgd_final"]).cuda())
    for mine, key in ((sf.points, "gf_upd_points"), (sf.norms, "gf_upd_norms"),
                      (sf.ED_nodes.points, "gf_upd_ed_points"), (sf.ED_nodes.norms, "gf_upd_ed_norms")):
        np.testing.assert_allclose(mine.cpu().numpy(), g[key], rtol=0, atol=2e-7)


@pytest.mark.parametrize("tag,world", [("soft", 2), ("sgd", 3), ("morph", 4)])
def test_surfel_sharded_ranks_reproduce_the_single_gpu_solve(tag, world):
    """One frame split over `world` ranks (all on this GPU, the all-reduce emulated by summing
    the ranks' partial buffers) takes the same optimiser steps as the unsharded solve."""
    import torch
    from super_amd.deform_mesh import GraphFit
    name = "s60x80_j48_semantic" if tag in GF_SEMANTIC_VARIANTS else "s60x80_j48"
    g, sc, _ = load_golden(name)
    sf, inputs, new_data = _frame(sc)
    opt = _opt(tag)
    ranks = [GraphFit(opt, rank=r, world=world, all_reduce=lambda t: None) for r in range(world)]
    for gf in ranks:
        gf.bind(inputs, sf, new_data)
    n = (sc.J + 1) * 7 + 10      # SLM_GF_NTERMS
    bufs = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in ranks]

    def all_reduce():
        tot = torch.stack([gf.get_partial(b) for gf, b in zip(ranks, bufs)]).sum(0)
        for gf in ranks:
            gf.set_partial(tot)

    for _ in range(opt.num_optimize_iterations):
        for gf in ranks:
            gf.eval_morph()
        if ranks[0].cfg.use_bn_morph:
            all_reduce()
        for gf in ranks:
            gf.eval_losses()
        all_reduce()
        for gf in ranks:
            gf.step()
    dvs = [gf.deform_verts().cpu().numpy() for gf in ranks]
    for d in dvs[1:]:
        np.testing.assert_array_equal(d, dvs[0])           # every rank holds the same parameters
    np.testing.assert_allclose(dvs[0], g[f"gf_{tag}_final"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("tag", ["sgd", "adam", "morph"])
def test_run_loop_continues_where_the_last_run_ended(tag):
    """slm_gf_run's loop keeps no launch of its own for the zeroing and counts its optimiser steps once, behind the loop
    (round 6): two runs of 5 iterations on one bound frame are the 10 iterations of one run -- the step counter
    (SGD's first-step rule, Adam's bias corrections), the momentum buffers and the zeroed state carry over -- and equal
    the stepwise entry points (eval_morph / eval_losses / step), which keep their own zeroing and fold launches."""
    from super_amd import _lib
    from super_amd.deform_mesh import GraphFit
    name = "s60x80_j48_semantic" if tag in GF_SEMANTIC_VARIANTS else "s60x80_j48"
    g, sc, _ = load_golden(name)
    sf, inputs, new_data = _frame(sc)
    full = _opt(tag)
    assert full.num_optimize_iterations == 10
    half = GraphFit(_opt(tag, num_optimize_iterations=5))
    half.bind(inputs, sf, new_data)
    for _ in range(2):
        _lib.check(half.lib.slm_gf_run(half.h, 1, half._st()), "slm_gf_run")
    dv2 = half.deform_verts().cpu().numpy()
    np.testing.assert_allclose(dv2, g[f"gf_{tag}_final"], rtol=0, atol=1e-9)
    steps = GraphFit(full)
    steps.bind(inputs, sf, new_data)
    for _ in range(10):
        steps.eval_morph()
        steps.eval_losses()
        steps.step()
    np.testing.assert_allclose(steps.deform_verts().cpu().numpy(), dv2, rtol=0, atol=1e-12)
