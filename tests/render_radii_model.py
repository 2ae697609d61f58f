"""CPU restatement of the surfel renderer with one radius per point (include/super_lm.h "Per-point radii": sphere k is
hit when rho_k < r_k, w_k = (1 - rho_k/r_k) exp((zt_k - zt_max)/gamma); a radius that is not finite or not > 0 culls its
row), written from the spec and not from the kernels: a numpy float64 forward (``render``), the hit sets (``hit_sets``)
and a torch float64 blend for fixed hit sets that is differentiable in the centres, the colours and the radii (``blend``,
dL/dr_k = sum over the pixels k takes part in of g.(c_k - C)/W e_k rho_k / r_k^2).  test_render_radii_model.py pins it against
``render_model.render`` (all radii equal), a hand-computed scene and finite differences; the GPU tests hold
slm_render_points_radii, slm_gf_render_radii and slm_render_backward_radii against it.

Conventions: centres, colours and radii are read as float32 and widened to float64 (Pulsar gets float32 tensors); the
gradients pass those roundings unchanged.  ``near`` marks a pixel where a decision sits at its threshold, as in
render_model.py, with each sphere's own radius: |rho/r_k - 1| < 1e-4 for a sphere that is not behind the pixel's
n_track-th hit, or an n_track cut between hits whose zt differ by less than 1e-4 gamma without being equal."""
import numpy as np
import torch

import render_model as rm

F64 = torch.float64


def radii32(radii):
    """the float32 radii widened to float64, and which rows they leave alive (finite and > 0)"""
    with np.errstate(over="ignore", invalid="ignore"):      # a float64 radius beyond float32 becomes inf: culled
        r = np.asarray(radii, np.float64).astype(np.float32).astype(np.float64)
    return r, np.isfinite(r) & (r > 0)


def _candidates(P, R, live, f, ccx, ccy, w, h, batch=200_000):
    """for runs of live rows: (ids, pixel rows ii, pixel columns jj, rho) of every pixel of the silhouette ranges padded
    by half a pixel, row-major inside each range (the enumeration of render_model.render)"""
    for b0 in range(0, len(live), batch):
        ids = live[b0:b0 + batch]
        X, Y, Z = P[ids, 0], P[ids, 1], P[ids, 2]
        x0, x1 = rm._range(X, Z, R[ids], f, ccx, w, 0.5)
        y0, y1 = rm._range(Y, Z, R[ids], f, ccy, h, 0.5)
        nx, ny = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
        cnt = nx * ny
        sid = np.repeat(np.arange(len(ids)), cnt)
        k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        jj = x0[sid] + k % nx[sid]
        ii = y0[sid] + k // nx[sid]
        yield ids[sid], ii, jj, rm.rho(P[ids[sid]], ii, jj, f, ccx, ccy)


def _live(P, ok):
    return np.nonzero((P[:, 2] >= rm.Z_NEAR) & (P[:, 2] <= rm.Z_FAR) & ok)[0] if len(P) else np.zeros(0, np.int64)


def render(points, colors, radii, K, H, W, view_scale=1.0, bg=(0.0, 0.0, 0.0), n_track=rm.N_TRACK):
    """-> dict(img (h,w,3) float64, front (h,w) int, count (h,w) int, near (h,w) bool), as render_model.render."""
    P = np.asarray(points).astype(np.float32).astype(np.float64)
    col = np.asarray(colors, np.float32).astype(np.float64)
    R, ok = radii32(radii)
    bg = np.asarray(bg, np.float64)
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    pix_l, id_l, rho_l, near_pix, near_z = [], [], [], [], []
    for ids, ii, jj, r in _candidates(P, R, _live(P, ok), f, ccx, ccy, w, h):
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
        sc = np.stack([np.bincount(pix, wk * col[ids, c], h * w) for c in range(3)], 1)
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
    return dict(img=img.reshape(h, w, 3), front=front.reshape(h, w), count=count.reshape(h, w),
                near=near.reshape(h, w))


def hit_sets(points, radii, K, H, W, view_scale=1.0, n_track=rm.N_TRACK):
    """-> (pix, ids, rank) numpy: the taken hits of every pixel (front to back, equal depth by row, the first n_track)."""
    P = np.asarray(points, np.float64).astype(np.float32).astype(np.float64)
    R, ok = radii32(radii)
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    pix_l, id_l = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for ids, ii, jj, r in _candidates(P, R, _live(P, ok), f, ccx, ccy, w, h):
        hit = r < R[ids]
        pix_l.append(ii[hit] * w + jj[hit])
        id_l.append(ids[hit])
    pix, ids = np.concatenate(pix_l), np.concatenate(id_l)
    if not len(pix):
        return pix, pix.copy(), pix.copy()
    o = np.lexsort((ids, P[ids, 2], pix))
    pix, ids = pix[o], ids[o]
    first = np.r_[0, np.nonzero(np.diff(pix))[0] + 1]
    rank = np.arange(len(pix)) - np.repeat(first, np.diff(np.r_[first, len(pix)]))
    keep = rank < n_track
    return pix[keep], ids[keep], rank[keep]


def _round32(t):
    return t + (t.detach().float().double() - t.detach())


def blend(points, colors, radii, hits, K, H, W, view_scale=1.0, bg=(0.0, 0.0, 0.0)):
    """The (h,w,3) float64 image as a torch function of ``points`` (N,3), ``colors`` (N,3) and ``radii`` (N,) float64
    tensors (any may require grad) for the fixed ``hits`` of ``hit_sets``.  zt_max (the first hit's) is held constant: it
    cancels.  Rows that ``hits`` does not name (culled ones, whatever their radius) are not read."""
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
    Pk, Rk = P[ids], _round32(radii[ids])
    v = Pk - (Pk * d).sum(1, keepdim=True) * d
    sq = (v * v).sum(1)
    pos = sq > 0
    rho = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
    zt = (rm.Z_FAR - Pk[:, 2]) / (rm.Z_FAR - rm.Z_NEAR)
    zmax = torch.zeros(h * w, dtype=F64)
    zmax[pix[rank == 0]] = zt.detach()[rank == 0]
    wk = (1.0 - rho / Rk) * torch.exp((zt - zmax[pix]) / rm.GAMMA)
    sw = torch.zeros(h * w, dtype=F64).index_add(0, pix, wk)
    sc = torch.zeros(h * w, 3, dtype=F64).index_add(0, pix, wk[:, None] * col[ids])
    hp = torch.unique(pix)
    wbg = torch.exp((rm.BG_EPS - zmax[hp]) / rm.GAMMA)
    img = img.index_put((hp,), (sc[hp] + wbg[:, None] * bgt) / (sw[hp] + wbg)[:, None])
    return img.reshape(h, w, 3)


def grads(points, colors, radii, g, hits, K, H, W, view_scale=1.0, bg=(0.0, 0.0, 0.0)):
    """(dL/dpoints (N,3), dL/dcolors (N,3), dL/dradii (N,)) numpy float64 of L = sum(image * g) at the given hit sets."""
    Pt = torch.from_numpy(np.asarray(points, np.float64)).requires_grad_(True)
    Ct = torch.from_numpy(np.asarray(colors, np.float64)).requires_grad_(True)
    Rt = torch.from_numpy(np.asarray(radii, np.float64)).requires_grad_(True)
    img = blend(Pt, Ct, Rt, hits, K, H, W, view_scale, bg)
    (img * torch.from_numpy(np.asarray(g, np.float64))).sum().backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return z(Pt), z(Ct), z(Rt)


def excluded(points, radii, K, H, W, near, view_scale=1.0):
    """rows with a candidate pixel (silhouette box padded by half a pixel) that is ``near``: their gradient hangs on a
    decision at its threshold (test_gpu_render_grad.py's rule, with each row's own radius)"""
    P = np.asarray(points, np.float64).astype(np.float32).astype(np.float64)
    R, ok = radii32(radii)
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    Rs = np.where(ok, R, 1.0)
    x0, x1 = rm._range(P[:, 0], P[:, 2], Rs, f, ccx, w, 0.5)
    y0, y1 = rm._range(P[:, 1], P[:, 2], Rs, f, ccy, h, 0.5)
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(near, 0), 1)
    live = ok & (P[:, 2] >= rm.Z_NEAR) & (P[:, 2] <= rm.Z_FAR) & (x0 <= x1) & (y0 <= y1)
    a, b, c, d = np.clip(y0, 0, h), np.clip(y1 + 1, 0, h), np.clip(x0, 0, w), np.clip(x1 + 1, 0, w)
    return live & (S[b, d] - S[a, d] - S[b, c] + S[a, c] > 0)
