"""The render loss as a term of slm_gf_run (slm_gf_bind_render_loss; GraphFit(opt, native_render_loss=True,
render_in_run=True) and GraphFit.forward_frames) on the 60 x 80 scene of test_gpu_graphfit_render_loss.py: RAD 0.01, weight
0.01, ten iterations.  Needs an MI355X (-m gpu).

Tolerances.  Against the CPU loop and between two GPU runs that evaluate the same term: that file's own, 1e-6 of the update's
size after ten iterations (GraphFit's gradient adds with float64 atomics, so two runs are not bitwise equal).  A slot without
the term against plain GraphFit(opt): atol 1e-9, the bound test_gpu_graphfit.py holds every GraphFit run to against its golden
result (batched against single runs: test_gpu_graphfit_shapes.py; in a mixed batch the slot runs k_gf_data<K, true> with a null
point gradient instead of k_gf_data<K, false>: the same sums in another atomic order).  The guarded render itself is compared with
slm_gf_render + slm_render_backward bitwise."""
import numpy as np
import pytest

import gf_render_run_cases as cases

pytestmark = pytest.mark.gpu


def _perturbed_dv():
    dv = np.zeros((49, 7))
    dv[:, 0] = 1.0
    rng = np.random.default_rng(9)      # the perturbation of test_loss_and_grad_match_the_oracle
    dv[:, :4] += 0.002 * rng.normal(size=(49, 4))
    dv[:, 4:] += 0.0005 * rng.normal(size=(49, 3))
    return dv


@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
def test_single_frame_matches_the_cpu_loop_and_the_stepwise_form(optimizer):
    ref = cases.cpu_loop(optimizer)
    step = cases.step_of(ref)
    o = cases.opt(optimizer=optimizer)
    dv, gf = cases.run_single(o, cases.gpu_frame(), native_render_loss=True, render_in_run=True)
    print("step", step, "err", np.abs(dv - ref).max(), "status", gf.last_render_status, "repeats", gf.render_repeats)
    np.testing.assert_allclose(dv, ref, rtol=0, atol=1e-6 * step)
    assert gf.render_repeats == 0 and gf.last_render_status[0][2] == 0
    assert gf.last_render_kept == gf.last_render_status[0][1] > 50
    stepwise, _ = cases.run_single(o, cases.gpu_frame(), native_render_loss=True)
    print("in-run - stepwise", np.abs(dv - stepwise).max())
    np.testing.assert_allclose(dv, stepwise, rtol=0, atol=1e-6 * step)
    plain, _ = cases.run_single(cases.opt(optimizer=optimizer, render_loss=False), cases.gpu_frame())
    assert np.abs(plain - dv).max() > 1e-3 * step


def test_single_frame_with_per_surfel_radii():
    ref = cases.cpu_loop_radii("SGD")
    step = cases.step_of(ref)
    o = cases.opt_radii()
    dv, gf = cases.run_single(o, cases.radii_gpu_frame(), native_render_loss=True, render_in_run=True)
    print("step", step, "err", np.abs(dv - ref).max(), "status", gf.last_render_status)
    np.testing.assert_allclose(dv, ref, rtol=0, atol=1e-6 * step)
    assert gf.render_repeats == 0 and gf.last_render_kept > 0
    stepwise, _ = cases.run_single(o, cases.radii_gpu_frame(), native_render_loss=True)
    np.testing.assert_allclose(dv, stepwise, rtol=0, atol=1e-6 * step)
    plain, _ = cases.run_single(cases.opt_radii(render_loss=False), cases.radii_gpu_frame())
    assert np.abs(plain - dv).max() > 1e-3 * step


@pytest.mark.parametrize("radii", [False, True])
def test_guarded_forward_and_backward_are_the_existing_ones(radii):
    """One slm_gf_loss_grad with the term bound, at a perturbed deform_verts; the slot's image and point gradient
    (slm_gf_render_loss_read) against slm_gf_render[_radii] + slm_render_ssim_loss + slm_render_backward on a second solver
    and context at the same state."""
    import torch
    from super_amd import _lib
    from super_amd.LM import _dev_ptr
    from super_amd.deform_mesh import GraphFit
    from super_amd.renderer import render_backward, ssim_render_loss_device
    o = cases.opt_radii() if radii else cases.opt()
    sf, inputs, new_data = cases.radii_gpu_frame() if radii else cases.gpu_frame()
    dv = torch.from_numpy(_perturbed_dv()).cuda()
    gf = GraphFit(o, native_render_loss=True, render_in_run=True)
    bf = gf._bind(0, inputs, sf, new_data)
    p = gf._bind_render_term(0, inputs, sf)
    st = gf._st()
    _lib.check(gf.lib.slm_gf_loss_grad(gf.h, 0, _dev_ptr(dv), None, None, st), "slm_gf_loss_grad")
    img = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    gp = torch.empty((bf.c.N, 3), dtype=torch.float64, device="cuda")
    _lib.check(gf.lib.slm_gf_render_loss_read(gf.h, 0, _dev_ptr(img), _dev_ptr(gp), st), "slm_gf_render_loss_read")
    loss, kept, over, _ = gf.render_loss_status(0)
    assert over == 0
    old = GraphFit(o, native_render_loss=True)
    old._bind(0, inputs, sf, new_data)
    _lib.check(old.lib.slm_gf_loss_grad(old.h, 0, _dev_ptr(dv), None, None, old._st()), "slm_gf_loss_grad")
    colors = sf.colors.detach().to(dtype=torch.float32).contiguous()
    img2, p2 = old._render_deformed_hwc(inputs, colors)
    out, gimg = ssim_render_loss_device(img2, inputs[("color", 0)], o.render_loss_weight, with_grad=True)
    gp2 = render_backward(old._render_ctx, p2, gimg)
    loss2, kept2 = out.cpu().tolist()
    print("kept", kept, kept2, "loss", loss, loss2, "|gp|", float(gp.abs().max()))
    assert torch.equal(img, img2)
    assert torch.equal(gp, gp2)
    assert float(gp.abs().max()) > 0.0
    assert loss == loss2 and kept == int(kept2)
    assert kept > 50


def test_batch_of_three_slots_two_with_the_term():
    from super_amd.deform_mesh import GraphFit
    sc, stable, cols, tgt = cases.scene()
    step = cases.step_of(cases.cpu_loop("SGD"))
    o = cases.opt()
    targets = [None, cases.other_target(), None]
    term = [True, True, False]
    singles = []
    for t, has in zip(targets, term):
        if has:
            singles.append(cases.run_single(o, cases.gpu_frame(t), native_render_loss=True, render_in_run=True)[0])
        else:
            singles.append(cases.run_single(cases.opt(render_loss=False), cases.gpu_frame(t))[0])
    assert np.abs(singles[0] - singles[1]).max() > 1e-3 * step      # the two targets pull differently
    gf = GraphFit(o, max_frames=3, native_render_loss=True, render_in_run=True)
    frames = [cases.gpu_frame(t) for t in targets]
    outs = gf.forward_frames([(f[1], f[0], f[2]) for f in frames], render_frames=term)
    outs = [x.cpu().numpy() for x in outs]
    assert len(outs) == 3 and all(x.shape == (sc.J + 1, 7) for x in outs)
    for k in range(3):
        print("slot", k, "err", np.abs(outs[k] - singles[k]).max(), "status", gf.last_render_status[k])
    np.testing.assert_allclose(outs[0], singles[0], rtol=0, atol=1e-6 * step)
    np.testing.assert_allclose(outs[1], singles[1], rtol=0, atol=1e-6 * step)
    np.testing.assert_allclose(outs[2], singles[2], rtol=0, atol=1e-9)
    assert gf.last_render_status[2] is None and gf.last_render_status[0][1] > 50 and gf.last_render_status[1][1] > 50
    # a batch of one on the same solver (max_frames = 3), and the same solver again without any term
    f = cases.gpu_frame()
    one = gf.forward_frames([(f[1], f[0], f[2])])
    assert len(one) == 1
    np.testing.assert_allclose(one[0].cpu().numpy(), singles[0], rtol=0, atol=1e-6 * step)
    f = cases.gpu_frame()
    none = gf.forward_frames([(f[1], f[0], f[2])] * 2, render_frames=[False, False])
    for x in none:
        np.testing.assert_allclose(x.cpu().numpy(), singles[2], rtol=0, atol=1e-9)
    plain = GraphFit(cases.opt(render_loss=False), max_frames=3)
    both = plain.forward_frames([(f[1], f[0], f[2])] * 2)
    for x in both:
        np.testing.assert_allclose(x.cpu().numpy(), singles[2], rtol=0, atol=1e-9)


def test_overflow_empties_the_renders_counts_them_and_forward_repeats():
    """entry_limit = 16, far below the scene's need: all ten renders of the run are empty and counted, the result is that of
    the run without the term, and forward repeats once with a larger limit.

    The largest total.  The status keeps the largest tile-list total of the renders since the bind.  While the renders are empty
    the geometric terms still move the state, and the total moves with it: on this scene the CPU model's boxes give 3027 entries
    at identity and 3027, 3027, 3029, 3032, 3034, 3038, 3040, 3039, 3045, 3045 over the ten iterations, so the largest total is
    that of a later state, not the identity state's.  The test therefore asks for more than the identity state's total: the
    totals of all ten states, each from slm_gf_render's own path, and the status must report their maximum (and the first of
    them must be the identity state's).  How the numbers are obtained: slm_gf_bind_render_loss sizes the lists with one render
    of the slot's CURRENT state through slm_gf_render's path (render_common with its read-back) and enters that total into the
    status record as the largest since the bind; a second solver without the term walks the same ten iterations stepwise
    (eval_morph / eval_losses / step) and, in front of each, binds the term, reads that total and clears the term again."""
    from super_amd import _lib
    from super_amd.deform_mesh import GraphFit
    ref = cases.cpu_loop("SGD")
    step = cases.step_of(ref)
    o = cases.opt()
    sf, inputs, new_data = cases.gpu_frame()
    walk = GraphFit(o, native_render_loss=True, render_in_run=True)
    walk._bind(0, inputs, sf, new_data)
    totals = []
    for _ in range(10):
        walk._bind_render_term(0, inputs, sf)
        _, _, over, total = walk.render_loss_status(0)
        assert over == 0
        totals.append(total)
        _lib.check(walk.lib.slm_gf_bind_render_loss(walk.h, 0, None, None, None, None, 0, None, 0.0, 0, walk._st()),
                   "slm_gf_bind_render_loss")
        walk.eval_morph()
        walk.eval_losses()
        walk.step()
    need = totals[0]                            # the identity state's: slm_gf_bind_frame has just reset the state
    assert need > 1000
    gf = GraphFit(o, native_render_loss=True, render_in_run=True)
    gf._bind(0, inputs, sf, new_data)
    gf._bind_render_term(0, inputs, sf)
    assert gf.render_loss_status(0)[2:] == (0, need)
    gf._bind(0, inputs, sf, new_data)
    gf._bind_render_term(0, inputs, sf, entry_limit=16)
    _lib.check(gf.lib.slm_gf_run(gf.h, 1, gf._st()), "slm_gf_run")
    loss, kept, over, largest = gf.render_loss_status(0)
    print("totals", totals, "status", (loss, kept, over, largest))
    assert over == 10
    assert largest == max(totals) >= need
    assert loss == 0.0 and kept == 0           # a background image keeps no pixel
    dv = gf.deform_verts().cpu().numpy()
    plain, _ = cases.run_single(cases.opt(render_loss=False), cases.gpu_frame())
    np.testing.assert_allclose(dv, plain, rtol=0, atol=1e-6 * step)
    # through Python, the limit injected for the first bind only: one repeat, then the result with the term
    gf2 = GraphFit(o, native_render_loss=True, render_in_run=True)
    gf2._entry_limit_once = 16
    dv2 = gf2(inputs, sf, new_data, None).cpu().numpy()
    print("repeats", gf2.render_repeats, "status", gf2.last_render_status, "err", np.abs(dv2 - ref).max())
    assert gf2.render_repeats == 1 and gf2.last_render_status[0][2] == 0
    np.testing.assert_allclose(dv2, ref, rtol=0, atol=1e-6 * step)
    assert np.abs(dv2 - plain).max() > 1e-3 * step


def test_forward_raises_when_the_repeats_do_not_help(monkeypatch):
    """a status that keeps reporting an overflow: two repeats, then SuperLMError"""
    from super_amd import _lib
    from super_amd.deform_mesh import GraphFit
    sf, inputs, new_data = cases.gpu_frame()
    gf = GraphFit(cases.opt(), native_render_loss=True, render_in_run=True)
    monkeypatch.setattr(gf, "render_loss_status", lambda slot=0: (0.0, 0, 10, 5000))
    with pytest.raises(_lib.SuperLMError, match="after two repeats"):
        gf(inputs, sf, new_data, None)
    assert gf.render_repeats == 2
