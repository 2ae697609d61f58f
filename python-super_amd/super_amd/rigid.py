"""Global rigid pre-alignment of the LM path: ``T_g`` ahead of the node solve (``slm_rigid_*``, include/super_lm.h).

The first-order path carries the reference's global row ``T_g`` (``super/deform_mesh.py:213-223``); the reference's LM
path has none.  ``RigidAlign`` estimates it by the reference's LM loop (``super/LM.py:81-122``) on one node at the origin
with every surfel attached at weight 1 -- seven parameters, the plain point-to-plane term plus the Rot term (always on:
without it ``|q|`` is a free scale) -- and ``rigid_update`` moves the model by it.  Opt-in, the stage carries the node solve's
flow-correspondence rows (``corr_term``) and per-residual data weights (``weighted_data``): ``slm_rigid_set_terms``.  The
frame is then

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
    ``opt.sf_point_plane_weight`` and ``opt.mesh_rot_weight`` (the Rot term is on whatever ``opt.mesh_rot`` says).
    ``corr_term=True`` (needs ``opt.sf_corr``; reads ``sf_corr_weight`` and ``sf_corr_loss_type``) adds the correspondence
    rows of the frames that bring a flow or ``corr_points``; ``weighted_data=True`` puts the weights that
    ``LM_Solver(weighted_data=True)`` reads from ``opt`` on the data rows (``sf.seg``, ``sf.seg_conf`` and
    ``new_data.seg_conf`` of every frame with a semantic weight).  Without them the stage is the plain one."""

    def __init__(self, opt, max_frames=1, corr_term=False, weighted_data=False):
        from .LM import corr_options, data_weight_options
        if int(max_frames) < 1:
            raise ValueError(f"RigidAlign: max_frames must be >= 1, got {max_frames}")
        self.corr_mode, self.corr_weight = corr_options("RigidAlign", opt) if corr_term else (0, 0.0)
        self.seg_mode, self.pp_max = data_weight_options(opt) if weighted_data else (0, 0.0)
        self.opt = opt
        self.max_frames = int(max_frames)
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SuperLMError("no HIP device visible: super_amd has no CPU fallback")
        out = C.c_void_p()
        _lib.check(self.lib.slm_rigid_create(self.max_frames, C.byref(out)), "slm_rigid_create")
        self.h = out
        if self.corr_mode or self.seg_mode or self.pp_max > 0.0:
            _lib.check(self.lib.slm_rigid_set_terms(self.h, self.corr_mode, self.corr_weight, self.seg_mode, self.pp_max),
                       "slm_rigid_set_terms")
        self.last_records = None
        self.last_terms = None                          # per slot of the last run: slm_rigid_get_terms
        self.last_assemble_terms = None                 # the same of the last assemble
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

    @staticmethod
    def _corr_arg(flow, corr_points):
        if flow is not None and corr_points is not None:
            raise ValueError("give flow or corr_points, not both")
        return flow if flow is not None else corr_points

    def _targets(self, rf, flow):
        dev = rf.device
        fl = _as(flow, torch.float32, dev)
        if tuple(fl.shape) != (1, 2, rf.c.H, rf.c.W):
            raise ValueError(f"flow must be (1,2,{rf.c.H},{rf.c.W}), got {tuple(fl.shape)}")
        N = rf.c.N
        pts = torch.zeros((N, 3), dtype=torch.float64, device=dev)
        nrm = torch.zeros((N, 3), dtype=torch.float64, device=dev)
        valid = torch.zeros(N, dtype=torch.uint8, device=dev)
        if N and rf.c.T:
            _lib.check(self.lib.slm_rigid_corr_targets(C.byref(rf.c), _dev_ptr(fl), _dev_ptr(pts), _dev_ptr(nrm),
                                                       _dev_ptr(valid), _stream_ptr(dev)), "slm_rigid_corr_targets")
        rf.flow_keep = fl                               # read by the kernel on the stream
        return pts, nrm, valid

    def corr_targets(self, sf, inputs, new_data, flow):
        """``(pts (N,3), nrm (N,3), valid (N,))`` of the frame from a flow (1,2,H,W): the targets ``LM(..., flow=)`` freezes
        at its bind, built here for the model as it stands (``slm_rigid_corr_targets``)."""
        rf = RigidFrame(sf, inputs, new_data, state=getattr(self.opt, "slm_state_dtype", None))
        out = self._targets(rf, flow)
        torch.cuda.current_stream(rf.device).synchronize()   # (rf may go afterwards)
        return out

    def _set_inputs(self, slot, rf, sf, new_data, corr):
        """Registers the term inputs of ``slot`` for the run that follows (or clears them); ``rf`` keeps them alive."""
        from .LM import corr_tensors, semantic_tensors
        dev = rf.device
        if not self.corr_mode:
            if corr is not None:
                raise ValueError("flow / corr_points need RigidAlign(opt, corr_term=True)")
        elif corr is None or rf.c.N == 0:
            _lib.check(self.lib.slm_rigid_set_corr(self.h, slot, None, None, None), "slm_rigid_set_corr")
        else:
            pts, nrm, valid = self._targets(rf, corr) if torch.is_tensor(corr) else corr_tensors(corr, rf.c.N, dev)
            if nrm is None and self.corr_mode == 2:
                raise ValueError("corr_points: sf_corr_loss_type 'point-plane' needs the target normals")
            rf.corr_keep = (pts, nrm, valid)
            _lib.check(self.lib.slm_rigid_set_corr(self.h, slot, _dev_ptr(pts), None if nrm is None else _dev_ptr(nrm),
                                                   _dev_ptr(valid)), "slm_rigid_set_corr")
        if self.seg_mode:
            seg, sc, tc = semantic_tensors("RigidAlign", sf, new_data, rf.c.N, rf.c.T, dev)
            rf.sem_keep = (seg, sc, tc)
            _lib.check(self.lib.slm_rigid_set_semantic(self.h, slot, int(sc.shape[1]), _dev_ptr(seg), _dev_ptr(sc),
                                                       _dev_ptr(tc)), "slm_rigid_set_semantic")

    def align(self, sf, inputs, new_data, u=10, v=7.5, minimal_loss=1e10, flow=None, corr_points=None):
        """``T_g = (q / |q|, t)`` of the frame: a (7,) float64 tensor on ``sf``'s device.  ``flow`` (1,2,H,W) or
        ``corr_points = (pts, nrm, valid)``: the frame's correspondences (``corr_term=True`` only; none: no such rows)."""
        corr = self._corr_arg(flow, corr_points)
        return self.align_batch([(sf, inputs, new_data, corr)], u=u, v=v, minimal_loss=minimal_loss)[0]

    def align_batch(self, frames, u=10, v=7.5, minimal_loss=1e10):
        """Many independent frames advanced together in the same launches; a list of (7,) tensors.  A fourth element of a
        frame gives its correspondences: a flow, a ``(pts, nrm, valid)`` triple, or ``None``."""
        n = len(frames)
        if n < 1 or n > self.max_frames:
            raise ValueError(f"need 1..{self.max_frames} frames, got {n}")
        state = getattr(self.opt, "slm_state_dtype", None)
        rfs = [RigidFrame(*fr[:3], state=state) for fr in frames]
        for i, (rf, fr) in enumerate(zip(rfs, frames)):
            self._set_inputs(i, rf, fr[0], fr[2], fr[3] if len(fr) > 3 else None)
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
        self.last_terms = [self.terms(i, dev) for i in range(n)]
        return [out[i] for i in range(n)]

    def terms(self, slot, device=None):
        """``(sum w r^2, matched count, sum |r_c|^2, kept count)`` of the sums kept at the slot's beta."""
        dev = device or (self._kept[0].device if self._kept else torch.device("cuda", torch.cuda.current_device()))
        out = torch.empty(4, dtype=torch.float64, device=dev)
        _lib.check(self.lib.slm_rigid_get_terms(self.h, slot, _dev_ptr(out), _stream_ptr(dev)), "slm_rigid_get_terms")
        t = out.cpu()
        return float(t[0]), int(t[1]), float(t[2]), int(t[3])

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

    def assemble(self, sf, inputs, new_data, beta7, flow=None, corr_points=None):
        """(JtJ (7,7), jtl (7,), loss, matched count) of the stage's system at ``beta7`` -- for inspection / parity; the
        split of the loss into its terms goes to ``last_assemble_terms``."""
        rf = RigidFrame(sf, inputs, new_data, state=getattr(self.opt, "slm_state_dtype", None))
        self._set_inputs(self.max_frames, rf, sf, new_data, self._corr_arg(flow, corr_points))
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
        self.last_assemble_terms = self.terms(self.max_frames, dev)
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
