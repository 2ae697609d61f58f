"""Global rigid pre-alignment of the LM path: ``T_g`` ahead of the node solve (``slm_rigid_*``, include/super_lm.h).

The first-order path carries the reference's global row ``T_g`` (``super/deform_mesh.py:213-223``); the reference's LM
path has none.  ``RigidAlign`` estimates it by the reference's LM loop (``super/LM.py:81-122``) on one node at the origin
with every surfel attached at weight 1 -- seven parameters, the plain point-to-plane term plus the Rot term (always on:
without it ``|q|`` is a free scale) -- and ``rigid_update`` moves the model by it.  The frame is then

    depth -> RigidAlign.align -> rigid_update -> LM_Solver.LM -> nodes.update -> fusion

which ``LM_Solver(opt, global_rigid=True)`` does by itself.  Everything numerical happens in the HIP library.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import SlmFrame, SlmIterRecord, SlmRigidConfig


def _dev_ptr(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise _lib.SuperLMError("super_amd needs tensors on a HIP device (no CPU fallback)")
    return t.data_ptr()


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _as(t, dtype, device):
    return t.detach().to(device=device, dtype=dtype).contiguous()


class RigidFrame:
    """Device-resident, ABI-layout view of what the stage reads from ``sf`` / ``inputs`` / ``new_data``: the surfel
    points and the frame's target.  Holds the tensors alive while the library uses them."""

    def __init__(self, sf, inputs, new_data, state=None):
        from .LM import state_dtype
        dev = sf.points.device
        if dev.type != "cuda":
            raise _lib.SuperLMError("super_amd needs tensors on a HIP device (no CPU fallback)")
        f32, i32 = torch.float32, torch.int32
        self.device = dev
        self.state_dtype = state_dtype(sf, state)
        self.sf_points = _as(sf.points, self.state_dtype, dev)
        self.tgt_points = _as(new_data.points, f32, dev)
        self.tgt_norms = _as(new_data.norms, f32, dev)
        self.index_map = _as(new_data.index_map, i32, dev)
        self.tgt_valid = _as(new_data.valid, torch.uint8, dev)
        H, W = inputs[("color", 0)].shape[-2:]
        Kh = inputs["K"][0].detach().to("cpu", torch.float32)
        fr = SlmFrame()
        fr.N, fr.T = int(self.sf_points.shape[0]), int(self.tgt_points.shape[0])
        fr.J, fr.K, fr.K_ED = 1, 1, 0
        fr.H, fr.W = int(H), int(W)
        fr.fx, fr.fy, fr.cx, fr.cy = float(Kh[0, 0]), float(Kh[1, 1]), float(Kh[0, 2]), float(Kh[1, 2])
        for name in ("sf_points", "tgt_points", "tgt_norms", "index_map", "tgt_valid"):
            t = getattr(self, name)
            setattr(fr, name, _dev_ptr(t) if t.numel() else None)
        fr.state_f64 = 1 if self.state_dtype == torch.float64 else 0
        self.c = fr


class RigidAlign:
    """The rigid stage over ``slm_rigid_*``.  Reads ``opt.num_optimize_iterations``, ``opt.phase``,
    ``opt.sf_point_plane_weight`` and ``opt.mesh_rot_weight`` (the Rot term is on whatever ``opt.mesh_rot`` says)."""

    def __init__(self, opt, max_frames=1):
        if int(max_frames) < 1:
            raise ValueError(f"RigidAlign: max_frames must be >= 1, got {max_frames}")
        self.opt = opt
        self.max_frames = int(max_frames)
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SuperLMError("no HIP device visible: super_amd has no CPU fallback")
        out = C.c_void_p()
        _lib.check(self.lib.slm_rigid_create(self.max_frames, C.byref(out)), "slm_rigid_create")
        self.h = out
        self.last_records = None
        self._kept = None

    def __del__(self):
        try:
            self.lib.slm_rigid_destroy(self.h)
        except Exception:
            pass

    def _config(self, u=10, v=7.5, minimal_loss=1e10):
        o = self.opt
        c = SlmRigidConfig()
        c.num_iterations = int(o.num_optimize_iterations)
        c.phase_test = 1 if o.phase == "test" else 0
        c.w_data = float(getattr(o, "sf_point_plane_weight", 1.0))
        c.w_rot = float(getattr(o, "mesh_rot_weight", 1.0))
        c.u0, c.v, c.minimal_loss0 = float(u), float(v), float(minimal_loss)
        return c

    def align(self, sf, inputs, new_data, u=10, v=7.5, minimal_loss=1e10):
        """``T_g = (q / |q|, t)`` of the frame: a (7,) float64 tensor on ``sf``'s device."""
        return self.align_batch([(sf, inputs, new_data)], u=u, v=v, minimal_loss=minimal_loss)[0]

    def align_batch(self, frames, u=10, v=7.5, minimal_loss=1e10):
        """Many independent frames advanced together in the same launches; a list of (7,) tensors."""
        n = len(frames)
        if n < 1 or n > self.max_frames:
            raise ValueError(f"need 1..{self.max_frames} frames, got {n}")
        state = getattr(self.opt, "slm_state_dtype", None)
        rfs = [RigidFrame(*fr[:3], state=state) for fr in frames]
        dev = rfs[0].device
        st = _stream_ptr(dev)
        cfg = self._config(u, v, minimal_loss)
        arr = (SlmFrame * n)(*[rf.c for rf in rfs])
        _lib.check(self.lib.slm_rigid_run(self.h, C.byref(cfg), n, arr, st), "slm_rigid_run")
        self._kept = rfs                                # read in place by the launches just enqueued
        out = torch.empty((n, 7), dtype=torch.float64, device=dev)
        for i in range(n):
            _lib.check(self.lib.slm_rigid_get(self.h, i, _dev_ptr(out[i]), st), "slm_rigid_get")
        self.last_records = [self.records(i, st) for i in range(n)]
        return [out[i] for i in range(n)]

    def beta(self, slot=0):
        """The raw seven parameters of the slot's last run (the quaternion not normalised)."""
        dev = self._kept[0].device if self._kept else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty(7, dtype=torch.float64, device=dev)
        _lib.check(self.lib.slm_rigid_get_beta(self.h, slot, _dev_ptr(out), _stream_ptr(dev)), "slm_rigid_get_beta")
        return out

    def records(self, slot, stream):
        n = int(self.opt.num_optimize_iterations)
        arr = (SlmIterRecord * max(n, 1))()
        got = C.c_int32(0)
        _lib.check(self.lib.slm_rigid_get_records(self.h, slot, arr, n, C.byref(got), stream), "slm_rigid_get_records")
        return [dict(loss=r.loss, u=r.u, accepted=bool(r.accepted), status=int(r.status),
                     M_grad=int(r.M_grad), M_loss=int(r.M_loss)) for r in arr[:got.value]]

    def assemble(self, sf, inputs, new_data, beta7):
        """(JtJ (7,7), jtl (7,), loss, matched count) of the stage's system at ``beta7`` -- for inspection / parity."""
        rf = RigidFrame(sf, inputs, new_data, state=getattr(self.opt, "slm_state_dtype", None))
        dev = rf.device
        st = _stream_ptr(dev)
        b = _as(torch.as_tensor(beta7), torch.float64, dev).reshape(-1)
        if b.numel() != 7:
            raise ValueError(f"beta7 must have 7 entries, got {tuple(b.shape)}")
        jtj = torch.empty((7, 7), dtype=torch.float64, device=dev)
        jtl = torch.empty(7, dtype=torch.float64, device=dev)
        lm = torch.empty(2, dtype=torch.float64, device=dev)
        cfg = self._config()
        _lib.check(self.lib.slm_rigid_assemble(self.h, C.byref(cfg), C.byref(rf.c), _dev_ptr(b), _dev_ptr(jtj),
                                               _dev_ptr(jtl), _dev_ptr(lm), st), "slm_rigid_assemble")
        lmh = lm.cpu()                                  # (synchronises: rf and b may go afterwards)
        return jtj, jtl, float(lmh[0]), int(lmh[1])


def rigid_transform(points, norms, Tg):
    """In place on contiguous float32 / float64 device tensors (n,3): ``p <- R(q) p + t``, ``n <- normalize(R(q) n)``
    (``F.normalize``: a zero normal stays zero); ``norms`` may be ``None``."""
    lib = _lib.load()
    dev = points.device
    if norms is not None and (norms.dtype != points.dtype or norms.shape != points.shape):
        raise ValueError("rigid_transform: points and norms must agree in dtype and shape")
    if points.dtype not in (torch.float32, torch.float64) or not points.is_contiguous() or \
            (norms is not None and not norms.is_contiguous()):
        raise ValueError("rigid_transform: needs contiguous float32 or float64 tensors")
    tg = _as(Tg, torch.float64, dev).reshape(-1)
    if tg.numel() != 7:
        raise ValueError(f"T_g must have 7 entries, got {tuple(tg.shape)}")
    n = int(points.shape[0])
    _lib.check(lib.slm_rigid_transform(n, _dev_ptr(points) if n else None,
                                       _dev_ptr(norms) if (norms is not None and n) else None,
                                       1 if points.dtype == torch.float64 else 0, _dev_ptr(tg), _stream_ptr(dev)),
               "slm_rigid_transform")


def rigid_update(sf, Tg):
    """Move the model by ``T_g``: ``sf.points`` / ``sf.norms`` and ``sf.ED_nodes.points`` / ``.norms`` are REPLACED by
    moved tensors (out of place, the dtype kept, like ``nodes.update``).  ``knn_indices`` / ``knn_w`` of surfels and
    nodes stay: a rigid motion preserves every distance they were made from."""
    ed = sf.ED_nodes
    dev = sf.points.device
    for obj in (sf, ed):
        sdt = torch.float64 if obj.points.dtype == torch.float64 else torch.float32
        pts, nrm = _as(obj.points, sdt, dev).clone(), _as(obj.norms, sdt, dev).clone()
        rigid_transform(pts, nrm, Tg)
        obj.points, obj.norms = pts.to(obj.points.dtype), nrm.to(obj.norms.dtype)
