"""Host-side mirror of the reference's surfel renderer (``renderer/renderer.py:12-78``, pytorch3d's Pulsar) and of
the two ``Surfels`` methods that call it (``super/nodes.py:630-650``), over libsuper_lm.so.

    models.renderer = super_amd.renderer.Pulsar(opt)          # InitNets, utils/shared_functions.py:37-39
    Surfels.render_img = super_amd.renderer.render_img        # the per-frame render at nodes.py:625

The image is the forward blend of Pulsar's paper (Lassner & Zollhoefer, CVPR 2021) at the parameters of the
reference's call; include/super_lm.h and DESIGN.md ("Renderer") state it.  pytorch3d is not available on ROCm, so
parity with Pulsar itself is NOT pinned: every convention that is only a reading of Pulsar is one constant or one
short function below, marked "unpinned".  ``Pulsar(opt)`` is forward only: inputs that require grad are refused.
``Pulsar(opt, differentiable=True)`` puts the render in the autograd graph (``render_differentiable``): gradients go to
the points and the colours, the exact derivative of THIS blend (``slm_render_backward_ex``), not Pulsar's own backward
(unpinned, hence opt-in).  The context keeps only its last forward; the backward of an earlier render re-renders its
saved inputs first (renders are bitwise reproducible, so the hit sets are the same).

Per-point radii: Pulsar's ``vert_rad`` is a float32 (N,) tensor, which the reference fills with one constant.  Here a
``rad`` of shape (N,) gives every point its own radius (``slm_render_points_radii``; a radius that is not finite or not
> 0 culls its point), and with ``differentiable=True`` an (N,) ``rad`` that requires grad gets dL/drad
(``slm_render_backward_radii``).  ``opt.renderer_surfel_radii`` makes ``render_`` / ``render_img`` and GraphFit render the
surfels with their own radii, ``sf.radii * opt.renderer_radii_scale``.

N-channel features: ``render_channels`` renders an (N,C) feature tensor, 1 <= C <= 8, into an (h,w,C) image in one
geometry pass (``slm_render_points_channels``: every channel is bitwise what a three-channel render gives for the same
column); ``render_backward_channels`` and ``render_channels_differentiable`` give dL/dpoints, dL/dfeatures and dL/dradii,
and ``Pulsar.render_channels`` dispatches between the plain forward and the node like ``Pulsar.render``.
``opt.renderer_one_pass`` makes ``render_`` blend the colours and the confidence heat in one six-channel render.

The render loss of GraphFit (``opt.render_loss``, deform_mesh.py:113-123) has two native pieces here:
``render_backward`` -- dL/dpoints of the last render on a context, the exact derivative of THIS blend (Pulsar's own
backward is not pinned) -- and ``ssim_render_loss`` -- monodepth2's SSIM-11 loss with the reference's mask,
selection and weight, and its image gradient, in float64 (the reference runs float32).  ``GraphFit(opt,
native_render_loss=True)`` chains them.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

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
        self.last_n = 0          # point count of the last render (the rows render_backward writes)
        self.serial = 0          # bumped by every render on this context (render_differentiable's recompute rule)
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


def _radii_arg(radii, n, device):
    """(N,) float32 contiguous radii on ``device`` (Pulsar's vert_rad is float32)"""
    r = radii.detach()
    if r.dim() != 1 or r.shape[0] != n:
        raise ValueError(f"radii must be (N,) with N = {n}, got {tuple(r.shape)}")
    return r.to(device=device, dtype=torch.float32).contiguous()


def _check_no_grad(*ts):
    for t in ts:
        if torch.is_tensor(t) and t.requires_grad:
            raise RuntimeError("super_amd.renderer: the renderer is forward only (no autograd; the render loss's "
                               "gradient is render_backward); pass tensors that do not require grad")


def _ptr(t):
    """the device pointer of a tensor; None for None and for an empty tensor"""
    return _dev_ptr(t) if t is not None and t.numel() else None


def _features_arg(features, n, device):
    """(N,C) float32 features with unit column stride on ``device``, 1 <= C <= 8, and their row stride in floats"""
    f = features.detach()
    if f.dim() != 2 or f.shape[0] != n or not 1 <= f.shape[1] <= _lib.SLM_RENDER_MAX_CHANNELS:
        raise ValueError(f"features must be (N,C) with N = {n} and 1 <= C <= {_lib.SLM_RENDER_MAX_CHANNELS}, "
                         f"got {tuple(f.shape)}")
    if f.dtype != torch.float32 or f.device != device or f.stride(1) != 1 or f.stride(0) < f.shape[1]:
        f = f.to(device=device, dtype=torch.float32).contiguous()
    return f, max(int(f.stride(0)), int(f.shape[1]))     # (an empty tensor's row stride may be anything)


def _bg_arg(bg, c):
    """the C background values as a host float array (zeros by default)"""
    b = torch.zeros(c) if bg is None else torch.as_tensor(bg).detach().float().cpu().reshape(-1)
    if b.numel() != c:
        raise ValueError(f"bg must have C = {c} values, got {b.numel()}")
    return (C.c_float * c)(*b.tolist())


def _forward(ctx, params, points, values, with_info=False, radii=None, bg=None, channels=False):
    """One render on ``ctx``, no check for grad: ``values`` are (N,>=3) colours (``slm_render_points``, with ``radii``
    ``slm_render_points_radii``) or, with ``channels``, (N,C) features with the background ``bg``
    (``slm_render_points_channels``).  Bumps ``ctx.serial``; ``ctx.last_n`` is N once the render has completed."""
    dev = points.device
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N,3), got {tuple(points.shape)}")
    n = int(points.shape[0])
    pts = points.detach()
    if pts.dtype != torch.float64:
        pts = pts.float()
    pts = pts.contiguous()
    params.points_f64 = int(pts.dtype == torch.float64)
    val, stride = (_features_arg if channels else _colors_arg)(values, n, dev)
    c = int(val.shape[1]) if channels else 3
    bgv = _bg_arg(bg, c) if channels else None
    rad = None if radii is None else _radii_arg(radii, n, dev)
    ctx.reserve(n)
    img = torch.empty((params.height, params.width, c), dtype=torch.float32, device=dev)
    fid = cnt = None
    if with_info:
        fid = torch.empty((params.height, params.width), dtype=torch.int32, device=dev)
        cnt = torch.empty_like(fid)
    ctx.last_n = 0
    ctx.serial += 1
    head, tail = (ctx.h, C.byref(params), n, _ptr(pts)), (_dev_ptr(img), _ptr(fid), _ptr(cnt), _stream_ptr(dev))
    if channels:
        _lib.check(ctx.lib.slm_render_points_channels(*head, _ptr(rad), c, _ptr(val), stride, bgv, *tail),
                   "slm_render_points_channels")
    elif rad is None:
        _lib.check(ctx.lib.slm_render_points(*head, _ptr(val), stride, *tail), "slm_render_points")
    else:
        _lib.check(ctx.lib.slm_render_points_radii(*head, _ptr(rad), _ptr(val), stride, *tail), "slm_render_points_radii")
    ctx.last_n = n
    return (img, fid, cnt) if with_info else img


def _backward(ctx, params, grad_image, points, values, radii, entry=None):
    """(dL/dpoints (N,3), dL/dvalues (N,3) or (N,C), dL/dradii (N,)) of the last render on ``ctx``, float64, None where
    not asked: always three entries.  ``entry``: the C entry point; by default ``slm_render_backward_radii`` when the
    radii's gradient is asked and ``slm_render_backward_ex`` otherwise."""
    entry = entry or ("slm_render_backward_radii" if radii else "slm_render_backward_ex")
    channels = entry == "slm_render_backward_channels"
    g = torch.as_tensor(grad_image).detach()
    dev = g.device
    if channels and (g.dim() != 3 or tuple(g.shape[:2]) != (params.height, params.width)):
        raise ValueError(f"grad_image must be ({params.height},{params.width},C), got {tuple(g.shape)}")
    if not channels and tuple(g.shape) != (params.height, params.width, 3):
        raise ValueError(f"grad_image must be ({params.height},{params.width},3), got {tuple(g.shape)}")
    c = int(g.shape[2])
    g = g.to(dtype=torch.float64).contiguous()
    n = ctx.last_n
    gp = torch.empty((n, 3), dtype=torch.float64, device=dev) if points else None
    gv = torch.empty((n, c), dtype=torch.float64, device=dev) if values else None
    gr = torch.empty((n,), dtype=torch.float64, device=dev) if radii else None
    outs = {"slm_render_backward": (gp,), "slm_render_backward_ex": (gp, gv)}.get(entry, (gp, gv, gr))
    _lib.check(getattr(ctx.lib, entry)(ctx.h, C.byref(params), *((c,) if channels else ()), _dev_ptr(g), *map(_ptr, outs),
                                       _stream_ptr(dev)), entry)
    return gp, gv, gr


def render_points(ctx, params, points, colors, with_info=False, radii=None):
    """Render (N,3) ``points`` (float32 or float64) with (N,3) ``colors``: (h,w,3) float32 on the device, and with
    ``with_info`` also the (h,w) int32 front-most row (-1: nothing hit) and hit count (<= n_track).  ``radii`` (N,), read
    as float32: one radius per point instead of ``params.radius`` (``slm_render_points_radii``)."""
    _check_no_grad(points, colors, radii)
    return _forward(ctx, params, points, colors, with_info, radii)


def render_channels(ctx, params, points, features, bg=None, with_info=False, radii=None):
    """Render (N,3) ``points`` with (N,C) ``features``, 1 <= C <= 8: (h,w,C) float32 on the device, every channel the
    blend of ``render_points`` for its column (``slm_render_points_channels``), in one geometry pass.  ``bg``: C
    background values (default zeros; ``params.bg`` is not read).  ``with_info`` and ``radii`` as ``render_points``.
    Forward only: inputs that require grad are refused."""
    _check_no_grad(points, features, radii)
    return _forward(ctx, params, points, features, with_info, radii, bg, channels=True)


def render_backward_channels(ctx, params, grad_image, points=True, features=True, radii=False):
    """(dL/dpoints (N,3) or None, dL/dfeatures (N,C) or None, dL/dradii (N,) or None), float64, of the last render on
    ``ctx``, which must be a ``render_channels`` with ``params`` (``slm_render_backward_channels``); C is
    ``grad_image``'s last dimension.  ``radii`` needs a render with per-point radii."""
    if not (points or features or radii):
        raise ValueError("render_backward_channels: request the points' gradient, the features' or the radii's")
    return _backward(ctx, params, grad_image, points, features, radii, "slm_render_backward_channels")


def render_backward(ctx, params, grad_image):
    """dL/dpoints (N,3) float64 of the last render on ``ctx`` (``render_points`` or GraphFit's ``slm_gf_render``:
    then by surfel row, 0 on unstable rows) for ``grad_image`` = dL/dimage (h,w,3).  ``params`` must be the render's.
    The exact derivative of the blend (include/super_lm.h ``slm_render_backward``): hit sets and the n_track cut are
    the forward's, positions the float32-rounded ones; not Pulsar's own backward (unpinned)."""
    return _backward(ctx, params, grad_image, True, False, False, "slm_render_backward")[0]


def render_backward_ex(ctx, params, grad_image, points=True, colors=True, radii=False):
    """``render_backward`` with the colour gradient: (dL/dpoints or None, dL/dcolors or None), each (N,3) float64, for
    the last render on ``ctx`` (include/super_lm.h ``slm_render_backward_ex``: dL/dc_k = sum over the pixels k takes
    part in of g w_k / W; the gradient passes the float32 cast of the colours).  Rows as ``render_backward``.
    Called with ``radii=True`` (the last render had per-point radii) the result is a triple: dL/dradii (N,) float64
    follows (``slm_render_backward_radii``: sum of g.(c_k - C)/W e_k rho_k / r_k^2), 0 on culled and unstable rows.
    The length of the result follows the caller's own ``radii`` argument, never the data."""
    if not (points or colors or radii):
        raise ValueError("render_backward_ex: request the points' gradient, the colours' or both")
    out = _backward(ctx, params, grad_image, points, colors, radii)
    return out if radii else out[:2]


class _Render(torch.autograd.Function):
    """The render as an autograd node, of colours or (``channels``) of features.  It keeps its inputs
    (``save_for_backward``: autograd's version check catches an in-place change after the forward), a copy of its
    parameters, its context object and the context's serial after its forward.  If another render has run on that
    context since -- any render, on the same handle or on one ``reserve`` recreated -- the backward re-renders the saved
    inputs into it first."""

    @staticmethod
    def forward(fctx, rctx, params, points, values, radii, bg, channels):
        img = _forward(rctx, params, points, values, radii=radii, bg=bg, channels=channels)
        fctx.rctx, fctx.params, fctx.serial = rctx, SlmRenderParams.from_buffer_copy(params), rctx.serial
        fctx.per_point, fctx.bg, fctx.channels = radii is not None, bg, channels
        fctx.save_for_backward(points, values, *(() if radii is None else (radii,)))
        return img

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_image):
        points, values = fctx.saved_tensors[:2]
        radii = fctx.saved_tensors[2] if fctx.per_point else None
        want_p, want_v = fctx.needs_input_grad[2], fctx.needs_input_grad[3]
        want_r = fctx.per_point and fctx.needs_input_grad[4]
        if not (want_p or want_v or want_r):
            return (None,) * 7
        rctx, params = fctx.rctx, fctx.params
        if rctx.serial != fctx.serial:
            _forward(rctx, params, points, values, radii=radii, bg=fctx.bg, channels=fctx.channels)
            fctx.serial = rctx.serial
        gp, gv, gr = _backward(rctx, params, grad_image, want_p, want_v, want_r,
                               "slm_render_backward_channels" if fctx.channels else None)
        if gp is not None:
            gp = gp.to(device=points.device, dtype=points.dtype)
        if gv is not None:          # colours may have more than three columns: those beyond get 0
            full = torch.zeros(values.shape, dtype=values.dtype, device=values.device)
            full[:, :gv.shape[1]] = gv
            gv = full
        if gr is not None:
            gr = gr.to(device=radii.device, dtype=radii.dtype)
        return None, None, gp, gv, gr, None, None


def render_differentiable(ctx, params, points, colors, radii=None):
    """``render_points`` as a node of the autograd graph: (h,w,3) float32 image; gradients to ``points`` (N,3) float32
    or float64, to ``colors`` (N,>=3) of any float dtype (columns beyond 3 get 0) and, when given, to the per-point
    ``radii`` (N,) of any float dtype (the render reads them as float32), each in its input's dtype and
    shape and only where ``needs_input_grad`` asks.  The gradient is ``render_backward_ex``'s, for the grad_image cast
    to float64; computed on the current stream.  ``ctx`` may be shared with other renders (see ``_Render``)."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N,3), got {tuple(points.shape)}")
    if radii is not None and (radii.dim() != 1 or radii.shape[0] != points.shape[0]):
        raise ValueError(f"radii must be (N,) with N = {points.shape[0]}, got {tuple(radii.shape)}")
    return _Render.apply(ctx, params, points, colors, radii, None, False)


def render_channels_differentiable(ctx, params, points, features, bg=None, radii=None):
    """``render_channels`` as a node of the autograd graph: (h,w,C) float32 image; gradients to ``points`` (N,3), to
    ``features`` (N,C) and, when given, to the per-point ``radii`` (N,), each in its input's dtype and only where
    ``needs_input_grad`` asks (``render_backward_channels`` for the grad_image cast to float64).  ``bg`` is a constant.
    ``ctx`` may be shared with other renders (see ``_Render``)."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N,3), got {tuple(points.shape)}")
    n = int(points.shape[0])
    if features.dim() != 2 or features.shape[0] != n or not 1 <= features.shape[1] <= _lib.SLM_RENDER_MAX_CHANNELS:
        raise ValueError(f"features must be (N,C) with N = {n} and 1 <= C <= {_lib.SLM_RENDER_MAX_CHANNELS}, "
                         f"got {tuple(features.shape)}")
    if radii is not None and (radii.dim() != 1 or radii.shape[0] != n):
        raise ValueError(f"radii must be (N,) with N = {n}, got {tuple(radii.shape)}")
    if torch.is_tensor(bg):
        bg = bg.detach().float().cpu()
    return _Render.apply(ctx, params, points, features, radii, bg, True)


def _ssim_args(img_hwc, target_chw):
    img = img_hwc.detach()
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"img_hwc must be (h,w,3), got {tuple(img.shape)}")
    h, w = int(img.shape[0]), int(img.shape[1])
    tgt = target_chw.detach()
    tgt = tgt.reshape(tgt.shape[-3:]) if tgt.dim() == 4 else tgt
    if tuple(tgt.shape) != (3, h, w):
        raise ValueError(f"target_chw must be (3,{h},{w}) or (1,3,{h},{w}), got {tuple(target_chw.shape)}")
    img = img.to(dtype=torch.float32).contiguous()
    tgt = tgt.to(device=img.device, dtype=torch.float32).contiguous()
    return img, tgt, h, w


def ssim_render_loss_device(img_hwc, target_chw, weight, with_grad=True):
    """``ssim_render_loss`` without the read-back: ((2,) float64 device [loss, kept], grad or None)."""
    img, tgt, h, w = _ssim_args(img_hwc, target_chw)
    dev = img.device
    out = torch.empty(2, dtype=torch.float64, device=dev)
    grad = torch.empty((h, w, 3), dtype=torch.float64, device=dev) if with_grad else None
    lib = _lib.load()
    _lib.check(lib.slm_render_ssim_loss(h, w, _dev_ptr(img), _dev_ptr(tgt), float(weight), _dev_ptr(out),
                                        _dev_ptr(grad) if grad is not None else None, _stream_ptr(dev)),
               "slm_render_ssim_loss")
    return out, grad


def ssim_render_loss(img_hwc, target_chw, weight, with_grad=True):
    """The reference's render loss (deform_mesh.py:115-121) of the render ``img_hwc`` (h,w,3) against
    ``target_chw`` (3,h,w) or (1,3,h,w) = inputs[("color",0)]: (weight * sum of the kept m, kept pixel count,
    dL/dimg (h,w,3) float64 or None).  SSIM-11 with reflection padding, m = mean_c(SSIM)^2, kept where the
    border-clipped 11x11 window of the render is > 0 in every channel and m < 0.1; float64 on the float32 inputs."""
    out, grad = ssim_render_loss_device(img_hwc, target_chw, weight, with_grad)
    loss, kept = out.cpu().tolist()
    return loss, int(kept), grad


def _split_rad(rad, n):
    """``rad`` of ``Pulsar.render`` -> (the one radius, None) for a number or a one-element tensor, (DEFAULT_RAD, the
    (N,) tensor) for per-point radii (``params.radius`` must be valid but the per-point render does not read it)."""
    if not torch.is_tensor(rad) or rad.numel() == 1:
        return rad, None
    if rad.dim() == 1 and rad.shape[0] == n:
        return DEFAULT_RAD, rad
    raise ValueError(f"rad must be a number, a one-element tensor or of shape (N,) = ({n},), got {tuple(rad.shape)}")


class Pulsar:
    """``Pulsar(opt)`` as in the reference: ``forward(inputs, data, colors=None, view_scale=1.0, rad=0.01,
    bg_col=...)`` returns the (h,w,3) float32 image on the device, channels last (callers permute it).

    ``rad`` is a number or a one-element tensor (one radius for every point, as the reference calls it) or a tensor of
    shape (N,): one radius per point, Pulsar's ``vert_rad`` (read as float32); any other shape raises ValueError.

    ``Pulsar(opt, differentiable=True)``: with grad enabled and points, colours or an (N,) ``rad`` that require grad,
    the image is in the autograd graph (``render_differentiable``); other inputs take the plain forward.  ``bg_col``
    and a one-element ``rad`` are constants: a tensor of either that requires grad is refused.  Plain ``Pulsar(opt)``
    refuses inputs that require grad (its gradient is this blend's, not Pulsar's own backward, which is unpinned)."""

    def __init__(self, opt, differentiable=False) -> None:
        self.height = opt.height
        self.width = opt.width
        self.gamma = GAMMA
        self.differentiable = bool(differentiable)
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

    def _render(self, inputs, points, values, view_scale, rad, bg, with_info, channels):
        """colours or features, in the graph or plain (see the class)"""
        rad, radii = _split_rad(rad, int(points.shape[0]))
        params = lambda: render_params(inputs["K"], self.height, self.width, view_scale, rad,
                                       *(() if channels else (bg,)))
        if self.differentiable and torch.is_grad_enabled():
            for name, t in (("bg" if channels else "bg_col", bg), ("rad", rad)):
                if torch.is_tensor(t) and t.requires_grad:
                    raise RuntimeError(f"super_amd.renderer.Pulsar: {name} is a constant of the render (no gradient); "
                                       f"pass a {name} that does not require grad")
            if any(torch.is_tensor(t) and t.requires_grad for t in (points, values, radii)):
                if with_info:
                    raise ValueError("super_amd.renderer.Pulsar: with_info is not available for a render in the graph")
                if channels:
                    return render_channels_differentiable(self.context(view_scale), params(), points, values, bg, radii)
                return render_differentiable(self.context(view_scale), params(), points, values, radii)
        if self.differentiable:        # not in the graph: the plain forward of the detached inputs
            points, values = points.detach(), values.detach()
            radii = None if radii is None else radii.detach()
        with torch.no_grad():
            if channels:
                return render_channels(self.context(view_scale), params(), points, values, bg, with_info, radii)
            return render_points(self.context(view_scale), params(), points, values, with_info, radii)

    def render(self, inputs, data, colors=None, view_scale=1.0, rad=0.01, bg_col=torch.tensor([0.0, 0.0, 0.0]),
               with_info=False):
        if colors is None:
            colors = data.colors
        return self._render(inputs, data.points, colors, view_scale, rad, bg_col, with_info, False)

    def render_channels(self, inputs, data, features, view_scale=1.0, rad=0.01, bg=None, with_info=False):
        """``render`` for (N,C) ``features``, 1 <= C <= 8: the (h,w,C) float32 image of ``data.points``, every channel
        blended like a colour channel, in one geometry pass.  ``rad`` as for ``render``; ``bg``: C values, default
        zeros.  In the graph (``render_channels_differentiable``) under the conditions of ``render``."""
        return self._render(inputs, data.points, features, view_scale, rad, bg, with_info, True)

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
    ``sf.renderImg_conf_heat`` (``magma`` of the confidences), both (1,3,H,W), from the stable surfels.  With
    ``opt.renderer_surfel_radii`` the radii are ``sf.radii[sf.isStable] * opt.renderer_radii_scale`` (default 1.0)
    instead of ``opt.renderer_rad``.  With ``opt.renderer_one_pass`` both images come from one six-channel render of
    ``cat(colors, heat)`` (bitwise the two renders'; the context then holds a channels forward, which a later
    ``render_backward`` on it refuses)."""
    rad = getattr(sf.opt, "renderer_rad", DEFAULT_RAD)
    if getattr(sf.opt, "renderer_surfel_radii", False):      # opt-in: every surfel with its own radius
        rad = sf.radii[sf.isStable].detach() * float(getattr(sf.opt, "renderer_radii_scale", 1.0))
    r = _renderer_of(sf)
    pts = sf.points[sf.isStable]
    cols = sf.colors[sf.isStable]
    heat = conf2color(sf.confs)[sf.isStable]
    data = type("Data", (), {})()
    data.points, data.colors = pts, cols
    if getattr(sf.opt, "renderer_one_pass", False):          # opt-in: one geometry pass for both images
        both = r.render_channels(inputs, data, torch.cat([cols.float(), heat.float()], 1), rad=rad)
        sf.renderImg = both[..., :3].contiguous().permute(2, 0, 1).unsqueeze(0)          # the layout of the two renders
        sf.renderImg_conf_heat = both[..., 3:].contiguous().permute(2, 0, 1).unsqueeze(0)
        return
    sf.renderImg = r(inputs, data, colors=data.colors, rad=rad).permute(2, 0, 1).unsqueeze(0)
    sf.renderImg_conf_heat = r(inputs, data, colors=heat, rad=rad).permute(2, 0, 1).unsqueeze(0)


def render_img(sf, inputs):
    """(reference ``Surfels.render_img``, nodes.py:647-655) ``render_`` under ``no_grad``; bind it with
    ``Surfels.render_img = super_amd.renderer.render_img``."""
    with torch.no_grad():
        render_(sf, inputs)
