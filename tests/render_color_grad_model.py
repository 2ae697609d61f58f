"""CPU restatement, in torch float64, of the surfel blend as a differentiable function of the centres AND the colours for
fixed hit sets (include/super_lm.h ``slm_render_backward_ex``: dL/dc_k = sum over the pixels k takes part in of
g w_k / W).  Written from the spec, not from the kernels: test_render_color_grad_model.py pins it against finite
differences and against render_grad_model.blend; test_gpu_render_autograd.py holds the HIP colour gradient and the
autograd renderer against it.

Convention: the blend reads float32-rounded centres and colours (Pulsar gets points.float(); the context keeps a float32
colour copy) and the gradient passes both roundings unchanged.  Hit membership, rho < rad and the n_track cut are
``render_grad_model.hit_sets``, held fixed."""
import numpy as np
import torch

import render_grad_model as rgm
import render_model as rm

F64 = torch.float64


def _round32(t):
    return t + (t.detach().float().double() - t.detach())


def blend(points, colors, hits, K, H, W, rad, view_scale=1.0, bg=(0.0, 0.0, 0.0)):
    """The (h,w,3) float64 image as a torch function of ``points`` (N,3) and ``colors`` (N,3) float64 tensors (either may
    require grad) for the fixed ``hits`` of ``render_grad_model.hit_sets``: with w_k = (1 - rho_k/rad)
    exp((zt_k - zt_max)/gamma) and W = sum w_k + w_bg, the colour (sum w_k c_k + w_bg bg) / W; ``bg`` where nothing is hit.
    zt_max (the first hit's) is held constant: it cancels."""
    P, col = _round32(points), _round32(colors)
    bgt = torch.as_tensor(np.asarray(bg, np.float64))
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    pix, ids, rank = (torch.as_tensor(a) for a in hits)
    img = bgt.repeat(h * w, 1) + 0.0 * col.sum()             # in the graph of the colours even when nothing is hit
    if len(pix) == 0:
        return img.reshape(h, w, 3)
    j, i = (pix % w).double(), torch.div(pix, w, rounding_mode="floor").double()
    d = torch.stack([(j - ccx) / f, (i - ccy) / f, torch.ones_like(j)], 1)
    d = d / d.norm(dim=1, keepdim=True)
    Pk = P[ids]
    v = Pk - (Pk * d).sum(1, keepdim=True) * d
    sq = (v * v).sum(1)
    pos = sq > 0
    rho = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
    zt = (rm.Z_FAR - Pk[:, 2]) / (rm.Z_FAR - rm.Z_NEAR)
    zmax = torch.zeros(h * w, dtype=F64)
    zmax[pix[rank == 0]] = zt.detach()[rank == 0]
    wk = (1.0 - rho / rad) * torch.exp((zt - zmax[pix]) / rm.GAMMA)
    sw = torch.zeros(h * w, dtype=F64).index_add(0, pix, wk)
    sc = torch.zeros(h * w, 3, dtype=F64).index_add(0, pix, wk[:, None] * col[ids])
    hp = torch.unique(pix)
    wbg = torch.exp((rm.BG_EPS - zmax[hp]) / rm.GAMMA)
    img = img.index_put((hp,), (sc[hp] + wbg[:, None] * bgt) / (sw[hp] + wbg)[:, None])
    return img.reshape(h, w, 3)


def render(points, colors, K, H, W, rad, view_scale=1.0, bg=(0.0, 0.0, 0.0), n_track=rm.N_TRACK):
    """blend at the hit sets of ``points``; ``points`` and ``colors`` torch float64 tensors (may require grad)."""
    hits = rgm.hit_sets(points.detach().numpy(), K, H, W, rad, view_scale, n_track)
    return blend(points, colors, hits, K, H, W, rad, view_scale, bg)


def grads(points, colors, g, K, H, W, rad, view_scale=1.0, bg=(0.0, 0.0, 0.0), n_track=rm.N_TRACK):
    """(dL/dpoints, dL/dcolors) numpy float64 (N,3) of L = sum(image * g) for numpy ``points``, ``colors`` and ``g``."""
    P = torch.from_numpy(np.asarray(points, np.float64)).requires_grad_(True)
    Ct = torch.from_numpy(np.asarray(colors, np.float64)).requires_grad_(True)
    img = render(P, Ct, K, H, W, rad, view_scale, bg, n_track)
    (img * torch.from_numpy(np.asarray(g, np.float64))).sum().backward()
    z = np.zeros((len(P), 3))
    return (z if P.grad is None else P.grad.numpy()), Ct.grad.numpy()     # no hit: the points are not in the graph
