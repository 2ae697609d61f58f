"""Host-side mirror of the reference's surfel renderer (``renderer/renderer.py:12-78``, pytorch3d's Pulsar) and of
the two ``Surfels`` methods that call it (``super/nodes.py:630-650``), over libsuper_lm.so.

    models.renderer = super_amd.renderer.Pulsar(opt)          # InitNets, utils/shared_functions.py:37-39
    Surfels.render_img = super_amd.renderer.render_img        # the per-frame render at nodes.py:625

The image is the forward blend of Pulsar's paper (Lassner & Zollhoefer, CVPR 2021) at the parameters of the
reference's call; include/super_lm.h and DESIGN.md ("Renderer") state it.  pytorch3d is not available on ROCm, so
parity with Pulsar itself is NOT pinned: every convention that is only a reading of Pulsar is one constant or one
short function below, marked "unpinned".  Forward only: there is no backward pass (``render_loss`` stays
unsupported), and inputs that require grad are refused.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import SlmRenderParams
from .LM import _dev_ptr, _stream_ptr

Z_NEAR = 0.01      # the reference camera's focal_length (renderer.py:31): Pulsar's near plane
Z_FAR = 15.0       # max_depth of the reference's call (renderer.py:74)
GAMMA = 1.0e-5     # Pulsar.gamma (renderer.py:20)
N_TRACK = 64       # n_track of the reference's Renderer (renderer.py:67)
BG_EPS = 1.0e-9    # unpinned: depth of the background in Pulsar's blend, w_bg = exp((BG_EPS - zt_max) / gamma)
DEFAULT_RAD = 2e-4  # opt.renderer_rad (options.py:177-180)


def camera(K, height, width, view_scale=1.0):
    """(w, h, f, ccx, ccy) of the reference's ``get_cam_params`` (renderer.py:22-46).

    One focal length f = K[0,0] s (fy is not used).  The principal point is an integer offset from the image
    centre, ccx = w/2 + ceil(K[0,2] s - w/2) (unpinned: the sign convention of Pulsar's offset).  A camera-frame
    point maps to u = f X/Z + ccx, v = f Y/Z + ccy, and pixel (i,j) casts the ray through (u,v) = (j,i)
    (unpinned: Pulsar's pixel-centre offset; this is pcd2depth's rounding, utils/utils.py:161-184)."""
    K = torch.as_tensor(K).detach()
    K = K.reshape(-1, *K.shape[-2:])[0].double().cpu()      # inputs["K"] (B,4,4); (3,3) accepted
    s = float(view_scale)
    w, h = int(width * s), int(height * s)
    f = float(K[0, 0]) * s
    ccx = w / 2 + math.ceil(float(K[0, 2]) * s - w / 2)
    ccy = h / 2 + math.ceil(float(K[1, 2]) * s - h / 2)
    return w, h, f, ccx, ccy


def render_params(K, height, width, view_scale=1.0, rad=DEFAULT_RAD, bg_col=(0.0, 0.0, 0.0), points_f64=False):
    w, h, f, ccx, ccy = camera(K, height, width, view_scale)
    p = SlmRenderParams()
    p.width, p.height, p.n_track, p.points_f64 = w, h, N_TRACK, int(bool(points_f64))
    p.focal, p.ccx, p.ccy, p.radius = f, ccx, ccy, float(rad)
    p.z_near, p.z_far, p.gamma, p.bg_eps = Z_NEAR, Z_FAR, GAMMA, BG_EPS
    bg = torch.as_tensor(bg_col).detach().float().cpu().reshape(3)
    for c in range(3):
        p.bg[c] = float(bg[c])
    return p


class RenderContext:
    """An ``slm_render`` context (slm_render_create): renders of up to H x W pixels; grows with the point count."""

    def __init__(self, H, W, max_points=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SuperLMError("no HIP device visible: super_amd has no CPU fallback")
        self.H, self.W, self.cap = int(H), int(W), 0
        self.h = C.c_void_p()
        self.reserve(max_points)

    def reserve(self, n):
        if self.h and n <= self.cap:
            return
        self.close()
        cap = max(int(n), 1024, self.cap + self.cap // 2)
        h = C.c_void_p()
        _lib.check(self.lib.slm_render_create(self.H, self.W, cap, C.byref(h)), "slm_render_create")
        self.h, self.cap = h, cap

    def close(self):
        if self.h:
            self.lib.slm_render_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _colors_arg(colors, n, device):
    """(tensor kept alive, row stride in floats): float32 rows with unit column stride are passed in place."""
    c = colors.detach()
    if c.dim() != 2 or c.shape[0] != n or c.shape[1] < 3:
        raise ValueError(f"colors must be (N,3) with N = {n}, got {tuple(c.shape)}")
    if c.dtype != torch.float32 or c.device != device or c.stride(1) != 1 or c.stride(0) < 3:
        c = c[:, :3].to(device=device, dtype=torch.float32).contiguous()
    return c, int(c.stride(0))


def _check_no_grad(*ts):
    for t in ts:
        if torch.is_tensor(t) and t.requires_grad:
            raise RuntimeError("super_amd.renderer: the renderer is forward only (no backward pass); "
                               "pass tensors that do not require grad")


def render_points(ctx, params, points, colors, with_info=False):
    """Render (N,3) ``points`` (float32 or float64) with (N,3) ``colors``: (h,w,3) float32 on the device, and with
    ``with_info`` also the (h,w) int32 front-most row (-1: nothing hit) and hit count (<= n_track)."""
    _check_no_grad(points, colors)
    dev = points.device
    n = int(points.shape[0])
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N,3), got {tuple(points.shape)}")
    pts = points.detach()
    if pts.dtype != torch.float64:
        pts = pts.float()
    pts = pts.contiguous()
    params.points_f64 = int(pts.dtype == torch.float64)
    col, stride = _colors_arg(colors, n, dev)
    ctx.reserve(n)
    img = torch.empty((params.height, params.width, 3), dtype=torch.float32, device=dev)
    fid = cnt = None
    if with_info:
        fid = torch.empty((params.height, params.width), dtype=torch.int32, device=dev)
        cnt = torch.empty_like(fid)
    ptr = lambda t: _dev_ptr(t) if t is not None and t.numel() else None
    _lib.check(ctx.lib.slm_render_points(ctx.h, C.byref(params), n, ptr(pts), ptr(col), stride, _dev_ptr(img),
                                         ptr(fid), ptr(cnt), _stream_ptr(dev)), "slm_render_points")
    return (img, fid, cnt) if with_info else img


class Pulsar:
    """``Pulsar(opt)`` as in the reference: ``forward(inputs, data, colors=None, view_scale=1.0, rad=0.01,
    bg_col=...)`` returns the (h,w,3) float32 image on the device, channels last (callers permute it)."""

    def __init__(self, opt) -> None:
        self.height = opt.height
        self.width = opt.width
        self.gamma = GAMMA
        self._ctx = None

    def to(self, *args, **kwargs):      # models.renderer = Pulsar(opt).to(device) in InitNets
        return self

    def context(self, view_scale=1.0):
        h, w = int(self.height * view_scale), int(self.width * view_scale)
        if self._ctx is None or self._ctx.H < h or self._ctx.W < w:
            H = max(h, self._ctx.H if self._ctx else 0)
            W = max(w, self._ctx.W if self._ctx else 0)
            self._ctx = RenderContext(H, W)
        return self._ctx

    def render(self, inputs, data, colors=None, view_scale=1.0, rad=0.01, bg_col=torch.tensor([0.0, 0.0, 0.0]),
               with_info=False):
        if colors is None:
            colors = data.colors
        with torch.no_grad():
            params = render_params(inputs["K"], self.height, self.width, view_scale, rad, bg_col)
            return render_points(self.context(view_scale), params, data.points, colors, with_info)

    def forward(self, inputs, data, colors=None, view_scale=1.0, rad=0.01, bg_col=torch.tensor([0.0, 0.0, 0.0])):
        return self.render(inputs, data, colors, view_scale, rad, bg_col)

    __call__ = forward


def conf2color(confs):
    """``conf2color`` (utils/utils.py:308-314) on the device: (N,) confidences -> (N,3) float64 ``magma`` colours,
    indexed exactly like ``Colormap.__call__`` on floats (x*256, 1.0 -> the last entry, below 0 -> the first,
    above 1 -> the last, NaN -> black)."""
    assert confs.dim() == 1, f"Point condfidences should be of shape (N,), but got {tuple(confs.shape)}"
    x = confs.detach()
    if not x.is_floating_point():
        x = x.double()
    xa = x * 256                                   # exact in either float dtype
    xa = torch.where(xa == 256, torch.full_like(xa, 255), xa)
    idx = torch.floor(xa).clamp(0, 255).long()
    idx = torch.where(torch.isnan(xa), torch.full_like(idx, 256), idx)
    return _magma_lut(x.device)[idx]


_LUT = {}


def _magma_lut(device):
    """matplotlib's 256-entry ``magma`` table (rgb, float64), read once, plus a black row for NaN."""
    key = str(device)
    if key not in _LUT:
        import matplotlib
        import numpy as np
        cmap = matplotlib.colormaps["magma"]
        assert cmap.N == 256
        lut = np.concatenate([cmap(np.arange(256))[:, :3], np.zeros((1, 3))])   # integer input: the table itself
        _LUT[key] = torch.from_numpy(lut).to(device)
    return _LUT[key]


_DEFAULT = {}


def _renderer_of(sf):
    r = getattr(getattr(sf, "models", None), "renderer", None)
    if isinstance(r, Pulsar):
        return r
    key = (sf.opt.height, sf.opt.width)
    if key not in _DEFAULT:
        _DEFAULT[key] = Pulsar(sf.opt)
    return _DEFAULT[key]


def render_(sf, inputs):
    """(reference ``Surfels.render_``, nodes.py:630-645) sets ``sf.renderImg`` (colours) and
    ``sf.renderImg_conf_heat`` (``magma`` of the confidences), both (1,3,H,W), from the stable surfels."""
    rad = getattr(sf.opt, "renderer_rad", DEFAULT_RAD)
    r = _renderer_of(sf)
    pts = sf.points[sf.isStable]
    cols = sf.colors[sf.isStable]
    heat = conf2color(sf.confs)[sf.isStable]
    data = type("Data", (), {})()
    data.points, data.colors = pts, cols
    sf.renderImg = r(inputs, data, colors=data.colors, rad=rad).permute(2, 0, 1).unsqueeze(0)
    sf.renderImg_conf_heat = r(inputs, data, colors=heat, rad=rad).permute(2, 0, 1).unsqueeze(0)


def render_img(sf, inputs):
    """(reference ``Surfels.render_img``, nodes.py:647-655) ``render_`` under ``no_grad``; bind it with
    ``Surfels.render_img = super_amd.renderer.render_img``."""
    with torch.no_grad():
        render_(sf, inputs)
