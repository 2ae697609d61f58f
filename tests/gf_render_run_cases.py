"""Shared by the tests of the render loss inside slm_gf_run (GraphFit(opt, native_render_loss=True, render_in_run=True)):
the 60 x 80 scene, options and CPU loop of test_gpu_graphfit_render_loss.py, the per-surfel-radii scene of
test_gpu_graphfit_render_radii.py with a CPU loop of its own, and every reference computed once (treat as read-only)."""
import functools

import numpy as np

import render_grad_model as rgm
import render_model as rm
import render_radii_cases as rc
import render_radii_model as rrm
import test_gpu_graphfit_render_loss as base
import test_gpu_graphfit_render_radii as base_radii
from oracle import graphfit_oracle as gfo

RAD, WEIGHT = base.RAD, base.WEIGHT
opt = base._opt
opt_radii = base_radii._opt


@functools.lru_cache(maxsize=None)
def scene():
    return base._scene()


def gpu_frame(tgt=None):
    sc, stable, cols, t0 = scene()
    return base._gpu_frame(sc, stable, cols, t0 if tgt is None else tgt)[:3]


@functools.lru_cache(maxsize=None)
def other_target():
    """a second colour frame for the scene: the model rendered with another shift, plus noise"""
    sc, stable, cols, _ = scene()
    tg = rm.render(sc.sf_points[stable] + np.array([-0.003, 0.003, 0.0]), cols[stable], sc.K, sc.H, sc.W, RAD)["img"]
    return (np.transpose(tg, (2, 0, 1)) + 0.01 * np.random.default_rng(6).normal(size=(3, sc.H, sc.W))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cpu_loop(optimizer):
    sc, stable, cols, tgt = scene()
    return base._cpu_loop(sc, stable, cols, tgt, opt(optimizer=optimizer), False)


def step_of(ref):
    step = np.abs(ref - np.eye(1, 7)).max()
    assert step > 1e-7
    return step


@functools.lru_cache(maxsize=None)
def radii_scene():
    return rc.graphfit_scene()


def radii_gpu_frame():
    return base_radii._gpu_frame(*radii_scene())


@functools.lru_cache(maxsize=None)
def cpu_loop_radii(optimizer="SGD"):
    """base._cpu_loop with the per-point render of tests/render_radii_model.py"""
    import torch
    sc, stable, cols, radii, tgt = radii_scene()
    o = opt_radii(optimizer=optimizer)
    pb = gfo.Problem(sc, stable=stable)
    dv = torch.zeros((pb.J + 1, 7), dtype=torch.float64)
    dv[:, 0] = 1.0
    dv.requires_grad_(True)
    optim = (torch.optim.SGD([dv], lr=o.learning_rate, momentum=0.9) if optimizer == "SGD"
             else torch.optim.Adam([dv], lr=o.learning_rate))
    R = torch.from_numpy(radii[stable])
    C = torch.from_numpy(cols[stable].astype(np.float64))
    for _ in range(o.num_optimize_iterations):
        optim.zero_grad()
        _, P = gfo.deform(pb, dv)
        hits = rrm.hit_sets(P.detach().numpy(), radii[stable], sc.K, sc.H, sc.W)
        img = rrm.blend(P, C, R, hits, sc.K, sc.H, sc.W)
        img32 = img + (img.detach().float().double() - img.detach())
        lr, _, _, _ = rgm.ssim_loss(img32, torch.from_numpy(tgt).double(), o.render_loss_weight)
        loss, _ = gfo.total_loss(pb, dv, o)
        (loss + lr).backward()
        dv.grad[-1] = dv.grad[-1] / pb.J
        optim.step()
    return dv.detach().numpy()


def run_single(o, frame, **kw):
    """one frame through GraphFit(o, **kw).forward -> (deform_verts as numpy, the GraphFit)"""
    from super_amd.deform_mesh import GraphFit
    gf = GraphFit(o, **kw)
    inputs, sf, new_data = frame[1], frame[0], frame[2]
    return gf(inputs, sf, new_data, None).cpu().numpy(), gf
