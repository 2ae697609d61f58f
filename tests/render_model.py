"""CPU restatement of the surfel renderer's image (include/super_lm.h "Forward surfel renderer", DESIGN.md
"Renderer"), in numpy float64, written from the spec and not from the kernel: the tests pin it with hand-computed
scenes (test_render_model.py) and hold the HIP renderer against it (test_gpu_render.py, the GraphFit loop of
test_gpu_graphfit_renderimg.py).

For every pixel it also reports whether a decision was close to its threshold: a candidate sphere with
|rho/rad - 1| < 1e-4 (coverage) that is not behind the pixel's n_track-th hit, or a pixel with more than n_track hits whose n_track-th and next hit differ in
zt by less than 1e-4 gamma without being equal (the cut).  Kernel and model may round such a pixel differently."""
import math

import numpy as np

Z_NEAR, Z_FAR, GAMMA, N_TRACK, BG_EPS = 0.01, 15.0, 1e-5, 64, 1e-9
NEAR = 1e-4


def camera(K, H, W, view_scale=1.0):
    """w = int(W s), h = int(H s), f = K[0,0] s, ccx = w/2 + ceil(K[0,2] s - w/2), ccy likewise."""
    K = np.asarray(K, np.float64)
    K = K.reshape(-1, *K.shape[-2:])[0]                      # (3,3), (4,4) or batched
    s = float(view_scale)
    w, h = int(W * s), int(H * s)
    return w, h, float(K[0, 0]) * s, w / 2 + math.ceil(K[0, 2] * s - w / 2), h / 2 + math.ceil(K[1, 2] * s - h / 2)


def rho(P, i, j, f, ccx, ccy):
    """distance of the centres P (n,3) from the line through the camera centre and pixel (i,j): |P x d| / |d|"""
    dx, dy = (np.asarray(j, np.float64) - ccx) / f, (np.asarray(i, np.float64) - ccy) / f
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    cx, cy, cz = Y - Z * dy, Z * dx - X, X * dy - Y * dx
    return np.sqrt(cx * cx + cy * cy + cz * cz) / np.sqrt(dx * dx + dy * dy + 1.0)


def _range(c, z, r, f, cc, n, pad):
    den, disc = z * z - r * r, c * c + z * z - r * r
    ok = (den > 0) & (disc > 0)
    s = r * np.sqrt(np.where(ok, disc, 1.0))
    den = np.where(ok, den, 1.0)
    a = np.where(ok, f * (c * z - s) / den + cc - pad, -1.0)
    b = np.where(ok, f * (c * z + s) / den + cc + pad, float(n))
    lo = np.maximum(np.ceil(np.clip(a, -1.0, n)).astype(np.int64), 0)
    hi = np.minimum(np.floor(np.clip(b, -1.0, n)).astype(np.int64), n - 1)
    return lo, hi


def render(points, colors, K, H, W, rad, view_scale=1.0, bg=(0.0, 0.0, 0.0), n_track=N_TRACK, batch=200_000):
    """-> dict(img (h,w,3) float64, front (h,w) int, count (h,w) int, near (h,w) bool)."""
    P = np.asarray(points).astype(np.float32).astype(np.float64)        # tensor.float(): round to nearest
    col = np.asarray(colors, np.float32).astype(np.float64)
    bg = np.asarray(bg, np.float64)
    w, h, f, ccx, ccy = camera(K, H, W, view_scale)
    n = len(P)
    live = np.nonzero((P[:, 2] >= Z_NEAR) & (P[:, 2] <= Z_FAR))[0] if n else np.zeros(0, np.int64)
    pix_l, id_l, z_l, rho_l, near_pix, near_z = [], [], [], [], [], []
    near = np.zeros(h * w, bool)
    for b0 in range(0, len(live), batch):
        ids = live[b0:b0 + batch]
        X, Y, Z = P[ids, 0], P[ids, 1], P[ids, 2]
        # candidate pixels: the exact silhouette range padded by half a pixel (independent of the kernel's padding)
        x0, x1 = _range(X, Z, rad, f, ccx, w, 0.5)
        y0, y1 = _range(Y, Z, rad, f, ccy, h, 0.5)
        nx, ny = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
        cnt = nx * ny
        sid = np.repeat(np.arange(len(ids)), cnt)
        k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        jj = x0[sid] + k % nx[sid]
        ii = y0[sid] + k // nx[sid]
        r = rho(P[ids[sid]], ii, jj, f, ccx, ccy)
        pix = ii * w + jj
        close = np.abs(r / rad - 1.0) < NEAR
        near_pix.append(pix[close])
        near_z.append(Z[sid[close]])
        hit = r < rad
        pix_l.append(pix[hit])
        id_l.append(ids[sid[hit]])
        z_l.append(Z[sid[hit]])
        rho_l.append(r[hit])
    img = np.tile(bg, (h * w, 1))
    front = -np.ones(h * w, np.int64)
    count = np.zeros(h * w, np.int64)
    if pix_l and sum(len(p) for p in pix_l):
        pix, ids, Z, r = (np.concatenate(a) for a in (pix_l, id_l, z_l, rho_l))
        o = np.lexsort((ids, Z, pix))               # per pixel: front to back, equal depth by row
        pix, ids, Z, r = pix[o], ids[o], Z[o], r[o]
        first = np.r_[0, np.nonzero(np.diff(pix))[0] + 1]
        start = np.repeat(first, np.diff(np.r_[first, len(pix)]))
        rank = np.arange(len(pix)) - start
        zt = (Z_FAR - Z) / (Z_FAR - Z_NEAR)
        # the n_track cut: the n_track-th and the next hit of a pixel
        cut = np.nonzero(rank == n_track)[0]
        dz = np.abs(zt[cut - 1] - zt[cut])
        near[pix[cut[(dz > 0) & (dz < NEAR * GAMMA)]]] = True
        keep = rank < n_track
        pix, ids, zt, r, start = pix[keep], ids[keep], zt[keep], r[keep], start[keep]
        zmax = np.empty(h * w)
        zmax[pix[rank[keep] == 0]] = zt[rank[keep] == 0]
        wk = (1.0 - r / rad) * np.exp((zt - zmax[pix]) / GAMMA)
        sw = np.bincount(pix, wk, h * w)
        sc = np.stack([np.bincount(pix, wk * col[ids, c], h * w) for c in range(3)], 1)
        hitpix = np.unique(pix)
        wbg = np.exp((BG_EPS - zmax[hitpix]) / GAMMA)
        img[hitpix] = (sc[hitpix] + wbg[:, None] * bg) / (sw[hitpix] + wbg)[:, None]
        front[pix[rank[keep] == 0]] = ids[rank[keep] == 0]
        count = np.bincount(pix, minlength=h * w)
    # a coverage decision close to its threshold matters unless the sphere lies behind the pixel's n_track-th hit
    zcut = np.full(h * w, np.inf)
    if pix_l and sum(len(p) for p in pix_l):
        last = rank[keep] == n_track - 1
        zcut[pix[last]] = Z_FAR - zt[last] * (Z_FAR - Z_NEAR)
    if near_pix:
        npix, nz = np.concatenate(near_pix), np.concatenate(near_z)
        near[npix[nz <= zcut[npix] * (1 + 1e-6)]] = True
    return dict(img=img.reshape(h, w, 3), front=front.reshape(h, w), count=count.reshape(h, w),
                near=near.reshape(h, w))
