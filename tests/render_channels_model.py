"""CPU restatement of the surfel renderer with N-channel features (include/super_lm.h "N-channel features"): the blend of
render_radii_model.py -- ``render``, ``blend``, ``grads`` -- with C columns in place of the three colours,
    out_c = (sum_k w_k f_kc + w_bg bg_c) / (sum_k w_k + w_bg),   bg_c where nothing is hit,
every channel summed on its own.  The geometry is not restated: candidates, hit sets and the rows left out of a gradient
comparison are those of render_radii_model (``_candidates``, ``hit_sets``, ``excluded``), which do not read the features.
test_render_channels_model.py pins this module against render_radii_model at C = 3, channel by channel, and against
finite differences; the GPU tests hold slm_render_points_channels and slm_render_backward_channels against it.

Conventions as in render_radii_model.py: centres, features and radii are read as float32 and widened to float64.
``radius``: one float64 radius for every point instead of ``radii`` (the one-radius forward; it is not rounded)."""
import numpy as np
import torch

import render_model as rm
import render_radii_model as rrm
from render_radii_model import excluded, hit_sets  # noqa: F401  (the geometry, shared)

F64 = torch.float64


def render(points, features, radii, K, H, W, view_scale=1.0, bg=None, n_track=rm.N_TRACK, radius=None):
    """-> dict(img (h,w,C) float64, front (h,w) int, count (h,w) int, near (h,w) bool), as render_radii_model.render."""
    P = np.asarray(points).astype(np.float32).astype(np.float64)
    feat = np.asarray(features, np.float32).astype(np.float64)
    C = feat.shape[1]
    if radius is None:
        R, ok = rrm.radii32(radii)
    else:
        R, ok = np.full(len(P), float(radius)), np.ones(len(P), bool)
    bg = np.zeros(C) if bg is None else np.asarray(bg, np.float64)
    assert bg.shape == (C,)
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    pix_l, id_l, rho_l, near_pix, near_z = [], [], [], [], []
    for ids, ii, jj, r in rrm._candidates(P, R, rrm._live(P, ok), f, ccx, ccy, w, h):
        pix = ii * w + jj
        close = np.abs(r / R[ids] - 1.0) < rm.NEAR
        near_pix.append(pix[close])
        near_z.append(P[ids[close], 2])
        hit = r < R[ids]
        pix_l.append(pix[hit])
        id_l.append(ids[hit])
        rho_l.append(r[hit])
    img = np.tile(bg, (h * w, 1))
    front = -np.ones(h * w, np.int64)
    count = np.zeros(h * w, np.int64)
    near = np.zeros(h * w, bool)
    zcut = np.full(h * w, np.inf)
    if pix_l and sum(len(p) for p in pix_l):
        pix, ids, r = (np.concatenate(a) for a in (pix_l, id_l, rho_l))
        Z = P[ids, 2]
        o = np.lexsort((ids, Z, pix))               # per pixel: front to back, equal depth by row
        pix, ids, Z, r = pix[o], ids[o], Z[o], r[o]
        first = np.r_[0, np.nonzero(np.diff(pix))[0] + 1]
        rank = np.arange(len(pix)) - np.repeat(first, np.diff(np.r_[first, len(pix)]))
        zt = (rm.Z_FAR - Z) / (rm.Z_FAR - rm.Z_NEAR)
        cut = np.nonzero(rank == n_track)[0]
        dz = np.abs(zt[cut - 1] - zt[cut])
        near[pix[cut[(dz > 0) & (dz < rm.NEAR * rm.GAMMA)]]] = True
        keep = rank < n_track
        pix, ids, zt, r, rank = pix[keep], ids[keep], zt[keep], r[keep], rank[keep]
        zmax = np.empty(h * w)
        zmax[pix[rank == 0]] = zt[rank == 0]
        wk = (1.0 - r / R[ids]) * np.exp((zt - zmax[pix]) / rm.GAMMA)
        sw = np.bincount(pix, wk, h * w)
        sc = np.stack([np.bincount(pix, wk * feat[ids, c], h * w) for c in range(C)], 1)
        hitpix = np.unique(pix)
        wbg = np.exp((rm.BG_EPS - zmax[hitpix]) / rm.GAMMA)
        img[hitpix] = (sc[hitpix] + wbg[:, None] * bg) / (sw[hitpix] + wbg)[:, None]
        front[pix[rank == 0]] = ids[rank == 0]
        count = np.bincount(pix, minlength=h * w)
        last = rank == n_track - 1
        zcut[pix[last]] = rm.Z_FAR - zt[last] * (rm.Z_FAR - rm.Z_NEAR)
    if near_pix:
        npix, nz = np.concatenate(near_pix), np.concatenate(near_z)
        near[npix[nz <= zcut[npix] * (1 + 1e-6)]] = True
    return dict(img=img.reshape(h, w, C), front=front.reshape(h, w), count=count.reshape(h, w),
                near=near.reshape(h, w))


def blend(points, features, radii, hits, K, H, W, view_scale=1.0, bg=None):
    """The (h,w,C) float64 image as a torch function of ``points`` (N,3), ``features`` (N,C) and ``radii`` (N,) float64
    tensors (any may require grad) for the fixed ``hits`` of ``hit_sets``; as render_radii_model.blend."""
    P, feat = rrm._round32(points), rrm._round32(features)
    C = feat.shape[1]
    bgt = torch.zeros(C, dtype=F64) if bg is None else torch.as_tensor(np.asarray(bg, np.float64))
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    pix, ids, rank = (torch.as_tensor(a) for a in hits)
    img = bgt.repeat(h * w, 1) + 0.0 * feat.sum()            # in the graph of the features even when nothing is hit
    if len(pix) == 0:
        return img.reshape(h, w, C)
    j, i = (pix % w).double(), torch.div(pix, w, rounding_mode="floor").double()
    d = torch.stack([(j - ccx) / f, (i - ccy) / f, torch.ones_like(j)], 1)
    d = d / d.norm(dim=1, keepdim=True)
    Pk, Rk = P[ids], rrm._round32(radii[ids])
    v = Pk - (Pk * d).sum(1, keepdim=True) * d
    sq = (v * v).sum(1)
    pos = sq > 0
    rho = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
    zt = (rm.Z_FAR - Pk[:, 2]) / (rm.Z_FAR - rm.Z_NEAR)
    zmax = torch.zeros(h * w, dtype=F64)
    zmax[pix[rank == 0]] = zt.detach()[rank == 0]
    wk = (1.0 - rho / Rk) * torch.exp((zt - zmax[pix]) / rm.GAMMA)
    sw = torch.zeros(h * w, dtype=F64).index_add(0, pix, wk)
    sc = torch.zeros(h * w, C, dtype=F64).index_add(0, pix, wk[:, None] * feat[ids])
    hp = torch.unique(pix)
    wbg = torch.exp((rm.BG_EPS - zmax[hp]) / rm.GAMMA)
    img = img.index_put((hp,), (sc[hp] + wbg[:, None] * bgt) / (sw[hp] + wbg)[:, None])
    return img.reshape(h, w, C)


def grads(points, features, radii, g, hits, K, H, W, view_scale=1.0, bg=None):
    """(dL/dpoints (N,3), dL/dfeatures (N,C), dL/dradii (N,)) numpy float64 of L = sum(image * g) at the given hit sets."""
    Pt = torch.from_numpy(np.asarray(points, np.float64)).requires_grad_(True)
    Ft = torch.from_numpy(np.asarray(features, np.float64)).requires_grad_(True)
    Rt = torch.from_numpy(np.asarray(radii, np.float64)).requires_grad_(True)
    img = blend(Pt, Ft, Rt, hits, K, H, W, view_scale, bg)
    (img * torch.from_numpy(np.asarray(g, np.float64))).sum().backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return z(Pt), z(Ft), z(Rt)
