"""CPU restatement, in torch float64, of the render loss of GraphFit: the surfel blend as a differentiable function of the
centres for fixed hit sets (include/super_lm.h ``slm_render_backward``), and monodepth2's SSIM-11 loss with the
reference's mask, selection and weight (``slm_render_ssim_loss``, super/deform_mesh.py:113-123).  Written from the
spec, not from the kernels: the tests pin it against finite differences, ``render_model.render`` and a direct numpy
SSIM (test_render_grad_model.py) and hold the HIP backward, the HIP SSIM loss and GraphFit's render-loss term against
it (test_gpu_render_grad.py, test_gpu_graphfit_render_loss.py).

Convention: the blend reads the float32-rounded centres (Pulsar gets points.float()) and the gradient passes the
rounding unchanged (``round32``: P + (f32(P) - P).detach()).  Hit membership, rho < rad and the n_track cut are
discrete; they are enumerated by ``hit_sets`` at the given centres and held fixed by ``blend``."""
import numpy as np
import torch
import torch.nn.functional as F

import render_model as rm

F64 = torch.float64


def hit_sets(points, K, H, W, rad, view_scale=1.0, n_track=rm.N_TRACK):
    """-> (pix, ids, rank) numpy: the taken hits of every pixel (front to back, equal depth by row, the first n_track),
    from the float32-rounded centres; candidates are the silhouette ranges padded by half a pixel."""
    P = np.asarray(points, np.float64).astype(np.float32).astype(np.float64)
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    live = np.nonzero((P[:, 2] >= rm.Z_NEAR) & (P[:, 2] <= rm.Z_FAR))[0] if len(P) else np.zeros(0, np.int64)
    pix_l, id_l = [], []
    for k in live:
        X, Y, Z = P[k]
        x0, x1 = rm._range(np.array([X]), np.array([Z]), rad, f, ccx, w, 0.5)
        y0, y1 = rm._range(np.array([Y]), np.array([Z]), rad, f, ccy, h, 0.5)
        if x0[0] > x1[0] or y0[0] > y1[0]:
            continue
        ii, jj = np.meshgrid(np.arange(y0[0], y1[0] + 1), np.arange(x0[0], x1[0] + 1), indexing="ij")
        ii, jj = ii.ravel(), jj.ravel()
        r = rm.rho(P[k][None], ii, jj, f, ccx, ccy)
        hit = r < rad
        pix_l.append(ii[hit] * w + jj[hit])
        id_l.append(np.full(int(hit.sum()), k))
    if not pix_l or not sum(len(p) for p in pix_l):
        z = np.zeros(0, np.int64)
        return z, z, z
    pix, ids = np.concatenate(pix_l), np.concatenate(id_l)
    o = np.lexsort((ids, P[ids, 2], pix))
    pix, ids = pix[o], ids[o]
    first = np.r_[0, np.nonzero(np.diff(pix))[0] + 1]
    rank = np.arange(len(pix)) - np.repeat(first, np.diff(np.r_[first, len(pix)]))
    keep = rank < n_track
    return pix[keep], ids[keep], rank[keep]


def hit_sets_fast(points, K, H, W, rad, view_scale=1.0, n_track=rm.N_TRACK, max_candidates=8_000_000):
    """``hit_sets`` without the Python loop over the surfels, for scenes of the driver's size: the candidate pixels of
    a run of surfels (``max_candidates`` at most) are enumerated at once (row-major inside each surfel's range, as the loop does) and pass through
    the same ``rm._range`` / ``rm.rho`` expressions, so every rho is the same float64.  ``hit_sets`` stays the
    definition; test_render_loss_cases.py holds this form identical to it, array by array."""
    P = np.asarray(points, np.float64).astype(np.float32).astype(np.float64)
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    live = np.nonzero((P[:, 2] >= rm.Z_NEAR) & (P[:, 2] <= rm.Z_FAR))[0] if len(P) else np.zeros(0, np.int64)
    X0, X1 = rm._range(P[live, 0], P[live, 2], rad, f, ccx, w, 0.5)
    Y0, Y1 = rm._range(P[live, 1], P[live, 2], rad, f, ccy, h, 0.5)
    NX, NY = np.maximum(X1 - X0 + 1, 0), np.maximum(Y1 - Y0 + 1, 0)
    chunk = np.cumsum(NX * NY) // max_candidates          # surfels whose candidates fit one pass together
    pix_l, id_l = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for c in np.unique(chunk):
        s = chunk == c
        ids, x0, y0, nx, cnt = live[s], X0[s], Y0[s], NX[s], (NX * NY)[s]
        sid = np.repeat(np.arange(len(ids)), cnt)
        k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ii, jj = y0[sid] + k // nx[sid], x0[sid] + k % nx[sid]
        hit = rm.rho(P[ids[sid]], ii, jj, f, ccx, ccy) < rad
        pix_l.append(ii[hit] * w + jj[hit])
        id_l.append(ids[sid[hit]])
    pix, ids = np.concatenate(pix_l), np.concatenate(id_l)
    if not len(pix):
        return pix, pix.copy(), pix.copy()
    o = np.lexsort((ids, P[ids, 2], pix))
    pix, ids = pix[o], ids[o]
    first = np.r_[0, np.nonzero(np.diff(pix))[0] + 1]
    rank = np.arange(len(pix)) - np.repeat(first, np.diff(np.r_[first, len(pix)]))
    keep = rank < n_track
    return pix[keep], ids[keep], rank[keep]


def blend(points, colors, hits, K, H, W, rad, view_scale=1.0, bg=(0.0, 0.0, 0.0), round32=True):
    """The (h,w,3) float64 image as a torch function of ``points`` (N,3) for the fixed ``hits`` of ``hit_sets``:
    w_k = (1 - rho_k/rad) exp((zt_k - zt_max)/gamma), colour = (sum w_k c_k + w_bg bg) / (sum w_k + w_bg).
    zt_max (the first hit's) is held constant: it cancels."""
    P = points
    if round32:
        P = P + (P.detach().float().double() - P.detach())
    col = torch.as_tensor(np.asarray(colors, np.float32).astype(np.float64))
    bgt = torch.as_tensor(np.asarray(bg, np.float64))
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    pix, ids, rank = (torch.as_tensor(a) for a in hits)
    img = bgt.repeat(h * w, 1)
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
    """blend at the hit sets of ``points`` (a torch tensor, may require grad)."""
    hits = hit_sets(points.detach().numpy(), K, H, W, rad, view_scale, n_track)
    return blend(points, colors, hits, K, H, W, rad, view_scale, bg)


def ssim_parts(img_hwc, target_chw):
    """monodepth2's SSIM(kernel=11) (depth/monodepth2/layers.py:217-247) per channel, before the clamp:
    -> (v (1,3,h,w) = (1 - n/d)/2, valid (1,1,h,w) = maxpool11(-min_c img) < 0)."""
    x = img_hwc.permute(2, 0, 1)[None]
    y = torch.as_tensor(target_chw, dtype=F64).reshape(1, 3, *x.shape[-2:])
    xp, yp = F.pad(x, (5, 5, 5, 5), mode="reflect"), F.pad(y, (5, 5, 5, 5), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(xp, 11, 1), F.avg_pool2d(yp, 11, 1)
    sigma_x = F.avg_pool2d(xp ** 2, 11, 1) - mu_x ** 2
    sigma_y = F.avg_pool2d(yp ** 2, 11, 1) - mu_y ** 2
    sigma_xy = F.avg_pool2d(xp * yp, 11, 1) - mu_x * mu_y
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    n = (2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)
    d = (mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2)
    valid = F.max_pool2d(-torch.min(x, dim=1, keepdim=True).values, 11, stride=1, padding=5) < 0
    return (1 - n / d) / 2, valid


def ssim_loss(img_hwc, target_chw, weight):
    """deform_mesh.py:115-121: -> (weight * sum of the kept m, kept count, m (h,w), v (3,h,w)); the mask and the
    m < 0.1 selection are constants."""
    v, valid = ssim_parts(img_hwc, target_chw)
    m = torch.clamp(v, 0, 1).mean(1, True) ** 2
    sel = valid & (m.detach() < 0.1)
    return weight * m[sel].sum(), int(sel.sum()), m[0, 0].detach(), v[0].detach()
