"""Host-side mirror of the reference's ``LM_Solver`` (``super/LM.py:10-122``) over
libsuper_lm.so.

Same names, argument meaning and error behaviour as the reference class, so that
``SuPer.__init__`` / ``SuPer.fusion`` (``super/super.py:18-19,68``) can construct and
call it unchanged when ``--use_derived_gradient`` is set:

    self.lm = LM_Solver(self.opt)
    deform_param = self.lm.LM(self.sf, inputs, sfdata)        # (J,7) float64

Everything numerical happens in the HIP library; this file only hands the caller's tensors to
the C ABI (device pointers) and converts results back.  The model state (``sf.points``,
``sf.knn_w``, ``ED_nodes.points``) is float64 in the reference and is passed AS IS (the library
reads float64 state, ``slm_frame.state_f64``): nothing is rounded between frames.  float32
state tensors are passed as float32 (the compact layout); indices become int32, the per-frame
target tables float32 (exact: the reference widens float32 back-projections,
``utils/data_loader.py:453-462``).  PyTorch is plumbing (device memory, streams).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import SlmConfig, SlmFrame, SlmIterRecord


def _dev_ptr(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise _lib.SuperLMError("super_amd needs tensors on a HIP device (no CPU fallback)")
    return t.data_ptr()


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _as(t, dtype, device):
    return t.detach().to(device=device, dtype=dtype).contiguous()


def state_dtype(sf, override=None):
    """dtype the library reads the model state in: the dtype of ``sf.points`` (float64 in the
    reference) unless ``override`` ("f32" / "f64", ``opt.slm_state_dtype``) forces one."""
    if override in ("f32", "float32", torch.float32):
        return torch.float32
    if override in ("f64", "float64", torch.float64):
        return torch.float64
    return torch.float64 if sf.points.dtype == torch.float64 else torch.float32


class ModelView:
    """The MODEL side of a frame in ABI layout (what ``slm_prepare_model`` reads): ``sf.points``, ``sf.knn_indices``,
    ``sf.knn_w``, ``ED_nodes.points``, ``ED_nodes.knn_indices``.  Remembers which tensors (and which in-place versions
    of them) it was made from, so that the bind of the next frame can tell whether it is still the same model."""

    FIELDS = ("sf_points", "sf_knn_idx", "sf_knn_w", "ed_points", "ed_knn_idx")

    def __init__(self, sf, device=None, state=None):
        dev = device if device is not None else sf.points.device
        if dev.type != "cuda":
            raise _lib.SuperLMError("super_amd needs tensors on a HIP device (no CPU fallback)")
        ed = sf.ED_nodes
        i32 = torch.int32
        sdt = state_dtype(sf, state)
        self.device = dev
        self.state_dtype = sdt
        self.sources = (sf.points, sf.knn_indices, sf.knn_w, ed.points, ed.knn_indices)
        self.stamp = self._stamp(self.sources)
        self.sf_points = _as(sf.points, sdt, dev)          # no copy when already float64 / contiguous
        self.sf_knn_idx = _as(sf.knn_indices, i32, dev)
        self.sf_knn_w = _as(sf.knn_w, sdt, dev)
        self.ed_points = _as(ed.points, sdt, dev)
        self.ed_knn_idx = _as(ed.knn_indices, i32, dev)
        self.J = int(self.ed_points.shape[0])

    @staticmethod
    def _stamp(tensors):
        return tuple((t.data_ptr(), tuple(t.shape), t.dtype, t._version) for t in tensors)

    def matches(self, sf, device, state):
        ed = sf.ED_nodes
        return (self.device == device and self.state_dtype == state_dtype(sf, state) and
                self.stamp == self._stamp((sf.points, sf.knn_indices, sf.knn_w, ed.points, ed.knn_indices)))

    def fill(self, fr: SlmFrame):
        fr.N, fr.J = int(self.sf_points.shape[0]), self.J
        fr.K, fr.K_ED = int(self.sf_knn_idx.shape[1]), int(self.ed_knn_idx.shape[1])
        for name in self.FIELDS:
            setattr(fr, name, _dev_ptr(getattr(self, name)))
        fr.state_f64 = 1 if self.state_dtype == torch.float64 else 0


class BoundFrame:
    """Device-resident, ABI-layout view of what LM reads from ``sf`` / ``inputs`` /
    ``new_data``.  Holds the tensors alive while the library uses them.
    ``model``: a ``ModelView`` of the same ``sf`` made earlier (``LM_Solver.prepare_model``)."""

    def __init__(self, sf, inputs, new_data, device=None, state=None, model=None):
        dev = device if device is not None else sf.points.device
        if dev.type != "cuda":
            raise _lib.SuperLMError("super_amd needs tensors on a HIP device (no CPU fallback)")
        f32, i32 = torch.float32, torch.int32
        mv = model if model is not None else ModelView(sf, dev, state)
        self.model = mv
        self.device = dev
        self.state_dtype = mv.state_dtype
        for name in ModelView.FIELDS:
            setattr(self, name, getattr(mv, name))
        self.tgt_points = _as(new_data.points, f32, dev)
        self.tgt_norms = _as(new_data.norms, f32, dev)
        self.index_map = _as(new_data.index_map, i32, dev)
        self.tgt_valid = _as(new_data.valid, torch.uint8, dev)
        H, W = inputs[("color", 0)].shape[-2:]
        K = inputs["K"]
        Kh = K[0].detach().to("cpu", torch.float32)        # one tiny D2H read per frame
        self.J = mv.J
        fr = SlmFrame()
        mv.fill(fr)
        fr.T = int(self.tgt_points.shape[0])
        fr.H, fr.W = int(H), int(W)
        fr.fx, fr.fy, fr.cx, fr.cy = float(Kh[0, 0]), float(Kh[1, 1]), float(Kh[0, 2]), float(Kh[1, 2])
        for name in ("tgt_points", "tgt_norms", "index_map", "tgt_valid"):
            setattr(fr, name, _dev_ptr(getattr(self, name)))
        self.c = fr


def corr_tensors(corr, N, dev):
    """``corr_points = (pts, nrm, valid)`` as the library reads it: (N,3) float64, (N,3) float64 or ``None``, (N,) uint8"""
    pts, nrm, valid = corr
    pts = _as(pts, torch.float64, dev)
    valid = _as(valid, torch.uint8, dev)
    nrm = None if nrm is None else _as(nrm, torch.float64, dev)
    if tuple(pts.shape) != (N, 3) or tuple(valid.shape) != (N,) or (nrm is not None and tuple(nrm.shape) != (N, 3)):
        raise ValueError(f"corr_points must be ((N,3), (N,3) or None, (N,)) with N = {N}")
    return pts, nrm, valid


def semantic_tensors(who, sf, new_data, N, T, dev):
    """The semantic inputs of a weighted data term as the library reads them: ``sf.seg`` (N,) int32, ``sf.seg_conf`` (N,C)
    and ``new_data.seg_conf`` (T,C) float32; ``who`` names the class in the refusals."""
    got = {}
    for name, obj, attr in (("sf.seg", sf, "seg"), ("sf.seg_conf", sf, "seg_conf"), ("new_data.seg_conf", new_data, "seg_conf")):
        t = getattr(obj, attr, None)
        if t is None:
            raise ValueError(f"{who}(weighted_data=True): {name} is missing")
        got[name] = t
    sc, tc = got["sf.seg_conf"], got["new_data.seg_conf"]
    if got["sf.seg"].numel() != N or got["sf.seg"].dim() > 2:
        raise ValueError(f"{who}(weighted_data=True): sf.seg must be ({N},), got {tuple(got['sf.seg'].shape)}")
    if sc.dim() != 2 or sc.shape[0] != N or not 1 <= sc.shape[1] <= _lib.SLM_MAX_CLASSES:
        raise ValueError(f"{who}(weighted_data=True): sf.seg_conf must be ({N}, C) with C in 1..{_lib.SLM_MAX_CLASSES}, "
                         f"got {tuple(sc.shape)}")
    if tc.dim() != 2 or tuple(tc.shape) != (T, sc.shape[1]):
        raise ValueError(f"{who}(weighted_data=True): new_data.seg_conf must be ({T}, {sc.shape[1]}), got {tuple(tc.shape)}")
    return _as(got["sf.seg"].reshape(-1), torch.int32, dev), _as(sc, torch.float32, dev), _as(tc, torch.float32, dev)


def data_weight_options(opt):
    """(seg_mode, pp_max) that ``weighted_data=True`` reads from ``opt``: soft wins over hard; raft_stereo truncates at 2e-5"""
    soft = bool(getattr(opt, "sf_soft_seg_point_plane", False))
    hard = bool(getattr(opt, "sf_hard_seg_point_plane", False))
    return (2 if soft else (1 if hard else 0)), (2e-5 if getattr(opt, "depth_model", None) == "raft_stereo" else 0.0)


def corr_options(who, opt):
    """(mode, weight) that ``corr_term=True`` reads from ``opt``"""
    if not getattr(opt, "sf_corr", False):
        raise ValueError(f"{who}(corr_term=True) needs opt.sf_corr")
    lt = getattr(opt, "sf_corr_loss_type", "point-point")
    if lt not in ("point-point", "point-plane"):
        raise ValueError(f"sf_corr_loss_type {lt!r}")
    return (1 if lt == "point-point" else 2), float(getattr(opt, "sf_corr_weight", 0.001))


class LM_Solver():
    """Drop-in for ``super.LM.LM_Solver``; see module docstring."""

    def __init__(self, opt, convs=None, max_frames=1, shard_surfels=False, rank=None, world=None,
                 all_reduce=None, broadcast=None, corr_term=False, weighted_data=False, face_term=False,
                 morph_term=False, global_rigid=False, rigid_terms=False):
        """``LM_Solver(opt, convs)`` as in the reference.  ``shard_surfels=True`` (after
        ``torch.distributed.init_process_group``) splits the surfels of ONE large frame over the GPUs
        of a node: every rank evaluates its share, the block-sparse J^T J / J^T r sums and the loss are
        all-reduced, every rank solves and takes rank 0's step.
        ``corr_term=True`` (opt-in; needs ``opt.sf_corr``) adds the flow-correspondence term the reference left commented
        out (``super/LM.py:27-29``): weight ``opt.sf_corr_weight``, form ``opt.sf_corr_loss_type``, targets frozen per
        frame from ``LM(..., flow=)`` or ``LM(..., corr_points=)`` (``slm_enable_corr``, include/super_lm.h).  Without it
        ``opt.sf_corr`` is ignored by this class and nothing changes.
        ``weighted_data=True`` (opt-in) puts the reference's per-residual weights of the first-order path on the
        point-to-plane term (``slm_enable_data_weights``, include/super_lm.h): ``opt.sf_soft_seg_point_plane`` /
        ``opt.sf_hard_seg_point_plane`` (soft wins; the term is then on also without ``opt.sf_point_plane``, whose place the
        reference gives them) read ``sf.seg``, ``sf.seg_conf`` and ``new_data.seg_conf`` of every frame, and
        ``opt.depth_model == "raft_stereo"`` truncates at 2e-5.  Without the flag those options are ignored by this class
        exactly as before.
        ``face_term=True`` (opt-in; needs ``opt.mesh_face``) adds the triangle-area face term of the reference's published
        runs (``super/deform_mesh.py:51-60``, there on the first-order path only) in its Gauss-Newton form
        (``slm_enable_face``, include/super_lm.h): ``sf.ED_nodes.triangles`` (3, F) and ``sf.ED_nodes.triangles_areas`` (F,)
        of every frame, weight ``opt.mesh_face_weight`` on the RESIDUAL (GraphFit weighs the squared sum: its
        ``mesh_face_weight`` = this one squared).  Without the flag ``opt.mesh_face`` is ignored by this class exactly as
        before.
        ``morph_term=True`` (opt-in; needs ``opt.sf_bn_morph``) adds the semantic boundary-morph term of Semantic-SuPer
        (``super/deform_mesh.py:126-194``, there on the first-order path only) in its Gauss-Newton form
        (``slm_enable_morph``, include/super_lm.h): ``inputs[("seg",0)]``, ``inputs[("seg_conf",0)]`` and ``sf.seg`` of every
        frame, ``opt.num_classes`` classes, weight ``opt.sf_bn_morph_weight`` on the RESIDUAL (GraphFit weighs the mean: its
        ``sf_bn_morph_weight`` = this one squared).  Without the flag ``opt.sf_bn_morph`` is ignored by this class exactly as
        before.
        ``global_rigid=True`` (opt-in) runs the global rigid pre-alignment ahead of the node solve (``super_amd.rigid``,
        ``slm_rigid_*`` in include/super_lm.h): ``LM()`` / ``LM_batch()`` first estimate ``T_g`` of every frame
        (``RigidAlign``: the plain, unweighted point-to-plane term plus the Rot term, whatever terms the node solve
        carries -- unless ``rigid_terms``, below), then MOVE ``sf`` BY IT (``rigid_update``: ``sf.points``, ``sf.norms``,
        ``sf.ED_nodes.points`` and ``.norms`` are replaced by the moved tensors), then run exactly what they run without the flag on the moved
        model.  They still return (J,7): ``Surfels.update(deform)`` after them completes the frame.  ``last_rigid`` holds
        the ``T_g`` of the last call.  Not built with ``shard_surfels``; ``prepare_model()`` is refused (the model moves
        after the target arrives: a plan prepared ahead would be sorted from stale points).  Without the flag nothing
        changes.
        ``rigid_terms=True`` (opt-in; needs ``global_rigid`` and at least one of ``corr_term`` / ``weighted_data`` in
        effect) lets the stage carry whichever of those two terms the solver carries (``slm_rigid_set_terms``).  Given a
        flow, the correspondence targets are then built ONCE, on the UNMOVED model (``RigidAlign.corr_targets``), used by
        the stage and handed to the node solve as ``corr_points``: they are points of the target frame and do not move
        with the model.  Without it the stage is the plain one and the node solve samples the flow at the projections of
        the moved model, as before."""
        self.opt = opt
        self.global_rigid = bool(global_rigid)
        self.rigid_terms = bool(rigid_terms)
        if self.rigid_terms and not self.global_rigid:
            raise ValueError("LM_Solver(rigid_terms=True) needs global_rigid=True")
        if self.global_rigid and (shard_surfels or world is not None):
            raise NotImplementedError("LM_Solver: global_rigid with shard_surfels is not built (the stage needs every "
                                      "surfel of the frame on one device)")
        self._rigid = None                           # RigidAlign, made at the first run
        self.last_rigid = None                       # per frame of the last LM / LM_batch: T_g (7,) float64 on the device
        self.last_rigid_records = None
        self.morph_on = False
        if morph_term:
            if not getattr(opt, "sf_bn_morph", False):
                raise ValueError("LM_Solver(morph_term=True) needs opt.sf_bn_morph")
            if shard_surfels or world is not None:
                raise NotImplementedError("LM_Solver: morph_term with shard_surfels is not built (the term needs every "
                                          "surfel of the frame on one device)")
            self.morph_on = True
            self.morph_weight = float(getattr(opt, "sf_bn_morph_weight", 1.0))
            self.morph_classes = int(opt.num_classes)
        self._morph_loss_of = None                   # (n, u, v, minimal_loss) of the last run; its losses once they were asked for
        self._morph_loss = None
        self.last_edge_counts = None                 # per slot: the boundary-list lengths per class of the last bind
        self.face_on = False
        if face_term:
            if not getattr(opt, "mesh_face", False):
                raise ValueError("LM_Solver(face_term=True) needs opt.mesh_face")
            if shard_surfels or world is not None:
                raise NotImplementedError("LM_Solver: face_term with shard_surfels is not built (the term's mesh is not sharded)")
            self.face_on = True
            self.face_weight = float(getattr(opt, "mesh_face_weight", 1.0))
        self._face_sent = {}                         # (handle, slot) -> stamp of the mesh tensors the slot holds
        self._face_loss_of = None                    # (n, u, v, minimal_loss) of the last run; its losses once they were asked for
        self._face_loss = None
        self.seg_mode, self.pp_max = 0, 0.0
        if weighted_data:
            self.seg_mode, self.pp_max = data_weight_options(opt)
        self.weighted = bool(self.seg_mode or self.pp_max > 0.0)
        self.corr_mode = 0
        if corr_term:
            mode, weight = corr_options("LM_Solver", opt)
            if shard_surfels or world is not None:
                raise NotImplementedError("LM_Solver: corr_term with shard_surfels is not built (the term needs every "
                                          "surfel of the frame on one device)")
            self.corr_mode, self.corr_weight = mode, weight
        self.last_corr_kept = None                   # per slot: correspondences kept in the last run (None: slot without)
        if self.rigid_terms and not (self.corr_mode or self.weighted):
            raise ValueError("LM_Solver(rigid_terms=True) needs corr_term=True or weighted_data=True (with a weight that "
                             "opt turns on)")
        self.lib = _lib.load()                       # raises if the HIP library is missing
        self.device = torch.device("cuda", torch.cuda.current_device()) \
            if torch.cuda.is_available() else None
        if self.device is None:
            raise _lib.SuperLMError("no HIP device visible: super_amd has no CPU fallback")
        self.phase = opt.phase
        if self.phase == "train":
            self.convs = convs
        self.max_frames = max_frames
        self._solvers = {}                           # (u, v, minimal_loss) -> handle
        self._bound = [None] * max_frames
        self._prepared = [None] * max_frames         # (handle, ModelView) of a pending slm_prepare_model per slot
        self.last_records = None
        self.rank, self.world = 0, 1
        self.sharded = bool(shard_surfels or world is not None)   # (a world of one rank runs the same protocol)
        self._all_reduce, self._broadcast = all_reduce, broadcast
        if self.sharded:
            import torch.distributed as dist
            if world is None:
                world, rank = dist.get_world_size(), dist.get_rank()
            self.rank, self.world = int(rank), int(world)
            if self._all_reduce is None or self._broadcast is None:
                from .dist import default_collectives
                ar, bc = default_collectives()
                self._all_reduce = self._all_reduce or ar                # sum, in place
                self._broadcast = self._broadcast or bc

    # ---- library handle --------------------------------------------------------------
    def _config(self, u, v, minimal_loss):
        o = self.opt
        c = SlmConfig()
        c.num_iterations = int(o.num_optimize_iterations)
        c.phase_test = 1 if o.phase == "test" else 0
        c.use_data, c.use_arap, c.use_rot = int(bool(o.sf_point_plane) or bool(self.seg_mode)), int(bool(o.mesh_arap)), \
            int(bool(o.mesh_rot))
        c.max_frames = self.max_frames
        c.data_path = int(getattr(o, "slm_data_path", 0))
        c.solver_path = int(getattr(o, "slm_solver_path", 0))
        c.w_data = float(getattr(o, "sf_point_plane_weight", 1.0))
        c.w_arap = float(getattr(o, "mesh_arap_weight", 10.0))
        c.w_rot = float(getattr(o, "mesh_rot_weight", 1.0))
        c.u0, c.v, c.minimal_loss0 = float(u), float(v), float(minimal_loss)
        return c

    def _handle(self, u=10, v=7.5, minimal_loss=1e10):
        key = (float(u), float(v), float(minimal_loss))
        h = self._solvers.get(key)
        if h is None:
            cfg = self._config(*key)
            out = C.c_void_p()
            _lib.check(self.lib.slm_create(C.byref(cfg), C.byref(out)), "slm_create")
            h = out
            if self.corr_mode:
                _lib.check(self.lib.slm_enable_corr(h, self.corr_mode, self.corr_weight), "slm_enable_corr")
            if self.weighted:
                _lib.check(self.lib.slm_enable_data_weights(h, self.seg_mode, self.pp_max), "slm_enable_data_weights")
            if self.face_on:
                _lib.check(self.lib.slm_enable_face(h, self.face_weight), "slm_enable_face")
            if self.morph_on:
                _lib.check(self.lib.slm_enable_morph(h, self.morph_weight), "slm_enable_morph")
            if self.sharded:
                _lib.check(self.lib.slm_set_shard(h, self.rank, self.world), "slm_set_shard")
            self._solvers[key] = h
        return h

    def __del__(self):
        try:
            for h in self._solvers.values():
                self.lib.slm_destroy(h)
        except Exception:
            pass

    def _frame(self, h, slot, sf, inputs, new_data):
        """The ``BoundFrame`` of a slot (no library call yet); settles what becomes of a model prepared ahead."""
        state = getattr(self.opt, "slm_state_dtype", None)
        dev = sf.points.device
        prepared = self._prepared[slot]
        self._prepared[slot] = None                    # a prepared model serves one bind
        mv = None
        if prepared is not None and prepared[0] is h and prepared[1].matches(sf, dev, state):
            mv = prepared[1]                           # same arrays, untouched since: the library only binds the target side
        elif prepared is not None:
            # The model changed after prepare_model (other tensors, or the same buffers rewritten in place: the version
            # counters moved).  The library compares sizes and pointers only -- with no-copy inputs (int32 tables, state
            # dtype, contiguous) it would take the stale plan for this frame's: drop it explicitly.
            _lib.check(self.lib.slm_discard_prepared(prepared[0], slot), "slm_discard_prepared")
        return BoundFrame(sf, inputs, new_data, state=state, model=mv)

    def _face_mesh(self, h, slot, sf):
        """The slot's mesh of the face term, before its bind / ``prepare_model``: sent again when the tensors changed
        (pointer, shape, dtype or version counter), kept by the library otherwise.  The stamp cannot tell a tensor that was
        freed and whose address a NEW tensor of the same shape, dtype and version took over from the old one (``ModelView``
        has the same limit): a caller that rebuilds the mesh tensors per frame and lets the old ones go should keep a
        reference to the previous pair until the next ``LM``, or write into the same tensors in place."""
        if not self.face_on:
            return
        ed = sf.ED_nodes
        tri, areas = getattr(ed, "triangles", None), getattr(ed, "triangles_areas", None)
        if tri is None or areas is None:
            raise ValueError("LM_Solver(face_term=True): sf.ED_nodes.triangles / triangles_areas are missing")
        if tri.dim() != 2 or tri.shape[0] != 3 or areas.numel() != tri.shape[1]:
            raise ValueError(f"LM_Solver(face_term=True): triangles must be (3, F) and triangles_areas (F,), got "
                             f"{tuple(tri.shape)} and {tuple(areas.shape)}")
        stamp = ModelView._stamp((tri, areas))
        if self._face_sent.get((h.value, slot)) == stamp:
            return
        dev = sf.points.device
        t32, a64 = _as(tri, torch.int32, dev), _as(areas.reshape(-1), torch.float64, dev)
        F = int(t32.shape[1])                         # (copied by the library on the stream: t32 / a64 may go afterwards)
        _lib.check(self.lib.slm_set_face_mesh(h, slot, F, _dev_ptr(t32) if F else None, _dev_ptr(a64) if F else None,
                                              _stream_ptr(dev)), "slm_set_face_mesh")
        self._face_sent[(h.value, slot)] = stamp

    @property
    def last_face_loss(self):
        """Per slot of the last ``LM`` / ``LM_batch``: (sum of squared face residuals at the returned beta, triangle count);
        ``None`` without ``face_term`` or before a run.  Evaluated when first read, in one device-to-host copy for all slots:
        a caller that never reads it pays no launch and no host wait per frame."""
        if self._face_loss is None and self._face_loss_of is not None:
            n, u, v, ml = self._face_loss_of
            h, dev = self._handle(u, v, ml), self._bound[0].device
            out = torch.empty((n, 2), dtype=torch.float64, device=dev)
            for i in range(n):
                _lib.check(self.lib.slm_face_loss(h, i, _dev_ptr(out[i]), _stream_ptr(dev)), "slm_face_loss")
            self._face_loss = [(float(a), int(b)) for a, b in out.cpu().tolist()]
        return self._face_loss

    def face_loss(self, slot=0, u=10, v=7.5, minimal_loss=1e10):
        """(sum of squared face residuals at the slot's current beta, triangle count)."""
        h, bf = self._handle(u, v, minimal_loss), self._bound[slot]
        out = torch.empty(2, dtype=torch.float64, device=bf.device)
        _lib.check(self.lib.slm_face_loss(h, slot, _dev_ptr(out), _stream_ptr(bf.device)), "slm_face_loss")
        o = out.cpu()
        return float(o[0]), int(o[1])

    def _bind(self, h, slot, sf, inputs, new_data):
        self._face_mesh(h, slot, sf)
        bf = self._frame(h, slot, sf, inputs, new_data)
        _lib.check(self.lib.slm_bind_frame(h, slot, C.byref(bf.c), _stream_ptr(bf.device)),
                   "slm_bind_frame")
        self._bound[slot] = bf
        return bf

    def _bind_batch(self, h, frames):
        """The frames of a batch bound CONCURRENTLY (``slm_bind_frames``: one host thread, stream and scratch set per frame
        inside the library, forked from and joined into the caller's stream) -- slots 0 .. len(frames) - 1."""
        for i, fr in enumerate(frames):
            self._face_mesh(h, i, fr[0])
        bfs = [self._frame(h, i, *fr) for i, fr in enumerate(frames)]
        arr = (SlmFrame * len(bfs))(*[bf.c for bf in bfs])
        _lib.check(self.lib.slm_bind_frames(h, 0, len(bfs), arr, _stream_ptr(bfs[0].device)), "slm_bind_frames")
        for i, bf in enumerate(bfs):
            self._bound[i] = bf
        return bfs

    def _bind_corr(self, h, slot, bf, corr):
        """The correspondences of a bound slot: a flow (1,2,H,W), a ``(pts, nrm, valid)`` triple, or ``None`` (no term)."""
        if not self.corr_mode:
            if corr is not None:
                raise ValueError("flow / corr_points need LM_Solver(opt, corr_term=True)")
            return
        if corr is None:
            return
        dev, st = bf.device, _stream_ptr(bf.device)
        if torch.is_tensor(corr):
            fl = _as(corr, torch.float32, dev)
            if tuple(fl.shape) != (1, 2, bf.c.H, bf.c.W):
                raise ValueError(f"flow must be (1,2,{bf.c.H},{bf.c.W}), got {tuple(fl.shape)}")
            bf.corr_keep = (fl,)                       # read by the bind's kernel on the stream
            _lib.check(self.lib.slm_bind_corr_flow(h, slot, _dev_ptr(fl), st), "slm_bind_corr_flow")
            return
        pts, nrm, valid = corr_tensors(corr, bf.c.N, dev)
        bf.corr_keep = (pts, nrm, valid)
        _lib.check(self.lib.slm_bind_corr_points(h, slot, _dev_ptr(pts), None if nrm is None else _dev_ptr(nrm),
                                                 _dev_ptr(valid), st), "slm_bind_corr_points")

    def _bind_semantic(self, h, slot, bf, sf, new_data):
        """The semantic inputs of a bound slot (``weighted_data`` with a semantic weight): ``sf.seg`` (N,), ``sf.seg_conf``
        (N,C), ``new_data.seg_conf`` (T,C)."""
        if not self.seg_mode:
            return
        dev = bf.device
        seg, sc, tc = semantic_tensors("LM_Solver", sf, new_data, bf.c.N, bf.c.T, dev)
        bf.sem_keep = (seg, sc, tc)                    # read in place by the library while the slot is used
        _lib.check(self.lib.slm_bind_data_semantic(h, slot, int(sc.shape[1]), _dev_ptr(seg), _dev_ptr(sc), _dev_ptr(tc),
                                                   _stream_ptr(dev)), "slm_bind_data_semantic")

    def _bind_morph(self, h, slot, bf, sf, inputs):
        """The inputs of the boundary-morph term of a bound slot (``morph_term``): ``inputs[("seg",0)]`` (1,1,H,W) -- or
        (1,C,H,W) scores, whose argmax over the channels is taken as ``find_edge_region`` does --, ``inputs[("seg_conf",0)]``
        (1,C,H,W) and ``sf.seg`` (N,).  Returns the boundary-list lengths per class."""
        if not self.morph_on:
            return None
        dev, N, H, W, nc = bf.device, bf.c.N, bf.c.H, bf.c.W, self.morph_classes
        pre = "LM_Solver(morph_term=True): "
        iseg = inputs.get(("seg", 0)) if hasattr(inputs, "get") else None
        iconf = inputs.get(("seg_conf", 0)) if hasattr(inputs, "get") else None
        seg = getattr(sf, "seg", None)
        for name, t in (('inputs[("seg",0)]', iseg), ('inputs[("seg_conf",0)]', iconf), ("sf.seg", seg)):
            if t is None:
                raise ValueError(pre + name + " is missing")
        if iseg.dim() != 4 or tuple(iseg.shape[2:]) != (H, W) or iseg.shape[0] != 1:
            raise ValueError(pre + f'inputs[("seg",0)] must be (1,1,{H},{W}), got {tuple(iseg.shape)}')
        if tuple(iconf.shape) != (1, nc, H, W):
            raise ValueError(pre + f'inputs[("seg_conf",0)] must be (1,{nc},{H},{W}), got {tuple(iconf.shape)}')
        if seg.numel() != N or seg.dim() > 2:
            raise ValueError(pre + f"sf.seg must be ({N},), got {tuple(seg.shape)}")
        if iseg.shape[1] > 1:
            iseg = torch.argmax(iseg, dim=1, keepdim=True)
        iseg = _as(iseg[0, 0], torch.int32, dev)
        iconf = _as(iconf[0], torch.float32, dev)
        seg = _as(seg.reshape(-1), torch.int32, dev)
        bf.morph_keep = (iseg, iconf, seg)             # read in place by the library while the slot is used
        counts = (C.c_int32 * _lib.SLM_MAX_CLASSES)()
        _lib.check(self.lib.slm_bind_morph(h, slot, nc, _dev_ptr(iseg), _dev_ptr(iconf), _dev_ptr(seg), counts,
                                           _stream_ptr(dev)), "slm_bind_morph")
        return list(counts)[:nc]

    @property
    def last_morph_loss(self):
        """Per slot of the last ``LM`` / ``LM_batch``: (the term's loss at the returned beta, kept surfels, candidates);
        ``None`` without ``morph_term`` or before a run.  Evaluated when first read, in one device-to-host copy for all
        slots: a caller that never reads it pays no launch and no host wait per frame."""
        if self._morph_loss is None and self._morph_loss_of is not None:
            n, u, v, ml = self._morph_loss_of
            h, dev = self._handle(u, v, ml), self._bound[0].device
            out = torch.empty((n, 3), dtype=torch.float64, device=dev)
            for i in range(n):
                _lib.check(self.lib.slm_morph_loss(h, i, _dev_ptr(out[i]), _stream_ptr(dev)), "slm_morph_loss")
            self._morph_loss = [(float(a), int(b), int(c)) for a, b, c in out.cpu().tolist()]
        return self._morph_loss

    def morph_targets(self, slot=0, u=10, v=7.5, minimal_loss=1e10):
        """The term's selection of a bound slot at its current beta: (kept (N,) bool, targets (N,2) f64, l_i (N,) f64) on
        the device."""
        h, bf = self._handle(u, v, minimal_loss), self._bound[slot]
        N, dev = bf.c.N, bf.device
        kept = torch.empty(N, dtype=torch.uint8, device=dev)
        tgt = torch.empty((N, 2), dtype=torch.float64, device=dev)
        li = torch.empty(N, dtype=torch.float64, device=dev)
        _lib.check(self.lib.slm_morph_targets(h, slot, _dev_ptr(kept), _dev_ptr(tgt), _dev_ptr(li), _stream_ptr(dev)),
                   "slm_morph_targets")
        return kept.bool(), tgt, li

    def data_weights(self, slot=0, u=10, v=7.5, minimal_loss=1e10):
        """The weights w_i (N,) float64 of a bound slot at its current beta, 0 for unmatched surfels (``weighted_data``)."""
        h, bf = self._handle(u, v, minimal_loss), self._bound[slot]
        w = torch.empty(bf.c.N, dtype=torch.float64, device=bf.device)
        _lib.check(self.lib.slm_data_weights(h, slot, _dev_ptr(w), _stream_ptr(bf.device)), "slm_data_weights")
        return w

    def corr_targets(self, slot=0, u=10, v=7.5, minimal_loss=1e10):
        """The bound targets of a slot: (pts (N,3) f64, nrm (N,3) f64, valid (N,) bool) on the device."""
        h, bf = self._handle(u, v, minimal_loss), self._bound[slot]
        N, dev = bf.c.N, bf.device
        pts = torch.empty((N, 3), dtype=torch.float64, device=dev)
        nrm = torch.empty((N, 3), dtype=torch.float64, device=dev)
        valid = torch.empty(N, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.slm_corr_get_targets(h, slot, _dev_ptr(pts), _dev_ptr(nrm), _dev_ptr(valid), _stream_ptr(dev)),
                   "slm_corr_get_targets")
        return pts, nrm, valid.bool()

    def corr_loss(self, slot=0, u=10, v=7.5, minimal_loss=1e10):
        """(sum of squared correspondence residuals at the slot's current beta, kept count)."""
        h, bf = self._handle(u, v, minimal_loss), self._bound[slot]
        out = torch.empty(2, dtype=torch.float64, device=bf.device)
        _lib.check(self.lib.slm_corr_loss(h, slot, _dev_ptr(out), _stream_ptr(bf.device)), "slm_corr_loss")
        o = out.cpu()
        return float(o[0]), int(o[1])

    def prepare_model(self, sf, slot=0, u=10, v=7.5, minimal_loss=1e10):
        """The model-side half of the NEXT frame's ``loss_term.prepare`` (reference ``super/loss.py:212-220,408-426``),
        ahead of time: call it when the current frame is done with the model -- after ``sf.update`` /
        ``fuseInputData`` / ``prepareStableIndexNSwapAllModel`` (``super/super.py:66-73``) -- and the next ``LM()`` on the
        same, untouched ``sf`` only binds its target (``slm_prepare_model``: the sort, the size read-backs and any
        symbolic analysis run on the library's worker thread and stream while the caller fetches the next frame).
        Optional: ``LM()`` alone does everything, as the reference does.  Not for surfel-sharded solvers' first bind
        order.  When the model changes after all -- other tensors or an in-place write, seen in the tensors' version
        counters -- the next ``LM()`` drops the preparation (``slm_discard_prepared``) and prepares in full."""
        if self.global_rigid:
            raise NotImplementedError("LM_Solver.prepare_model: not with global_rigid (LM() moves the model after the "
                                      "target arrives: a plan prepared ahead would be sorted from stale points)")
        h = self._handle(u, v, minimal_loss)
        self._face_mesh(h, slot, sf)
        mv = ModelView(sf, state=getattr(self.opt, "slm_state_dtype", None))
        fr = SlmFrame()
        mv.fill(fr)
        _lib.check(self.lib.slm_prepare_model(h, slot, C.byref(fr), _stream_ptr(mv.device)), "slm_prepare_model")
        self._prepared[slot] = (h, mv)

    # ---- reference surface -------------------------------------------------------------
    @staticmethod
    def Solver(A, b, method="cholesky"):
        """(reference ``super/LM.py:37-51``) solve A x = b for SPD A on the device; raises
        ``RuntimeError`` when the factorisation fails, like ``torch.linalg.cholesky``."""
        if method == "lu":     # deprecated torch.lu path, never selected by any reference caller
            raise NotImplementedError("super_amd.LM_Solver.Solver: method='lu' is not built (Cholesky only)")
        if method != "cholesky":
            raise ValueError(method)
        lib = _lib.load()
        dev = A.device
        A64 = _as(A, torch.float64, dev)
        b64 = _as(b, torch.float64, dev).reshape(-1)
        P = A64.shape[0]
        x = torch.empty(P, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.slm_solve_dense(P, _dev_ptr(A64), _dev_ptr(b64), _dev_ptr(x),
                                       _dev_ptr(status), _stream_ptr(dev)), "slm_solve_dense")
        if int(status.item()) != 0:
            raise RuntimeError("cholesky: the input is not positive-definite")
        return x.reshape(b.shape).to(b.dtype)

    def prepareCostTerm(self, sf, inputs, new_data, beta, grad=False, flow=None, corr_points=None):
        """(reference ``super/LM.py:54-78``) ``grad=True`` -> (dense JtJ (P,P), jtl (P,1));
        ``grad=False`` -> scalar sum of squared residuals.  For inspection / parity: the LM
        loop itself never materialises the dense matrix.  With ``corr_term`` the correspondence term
        of ``flow`` / ``corr_points`` is included."""
        h = self._handle()
        bf = self._bind(h, 0, sf, inputs, new_data)
        self._bind_corr(h, 0, bf, self._corr_arg(flow, corr_points, required=True))
        self._bind_semantic(h, 0, bf, sf, new_data)
        self._bind_morph(h, 0, bf, sf, inputs)
        st = _stream_ptr(bf.device)
        b64 = _as(beta, torch.float64, bf.device)
        _lib.check(self.lib.slm_set_beta(h, 0, _dev_ptr(b64), st), "slm_set_beta")
        P = 7 * bf.J
        if grad:
            jtj = torch.empty((P, P), dtype=torch.float64, device=bf.device)
            jtl = torch.empty((P, 1), dtype=torch.float64, device=bf.device)
            _lib.check(self.lib.slm_assemble(h, 0, _dev_ptr(jtj), _dev_ptr(jtl), st), "slm_assemble")
            return jtj, jtl
        out = torch.empty(4, dtype=torch.float64, device=bf.device)
        _lib.check(self.lib.slm_loss(h, 0, _dev_ptr(out), st), "slm_loss")
        total = out[:3].sum()
        if self.corr_mode:
            co = torch.empty(2, dtype=torch.float64, device=bf.device)
            _lib.check(self.lib.slm_corr_loss(h, 0, _dev_ptr(co), st), "slm_corr_loss")
            total = total + co[0]
        if self.face_on:
            fo = torch.empty(2, dtype=torch.float64, device=bf.device)
            _lib.check(self.lib.slm_face_loss(h, 0, _dev_ptr(fo), st), "slm_face_loss")
            total = total + fo[0]
        if self.morph_on:
            mo = torch.empty(3, dtype=torch.float64, device=bf.device)
            _lib.check(self.lib.slm_morph_loss(h, 0, _dev_ptr(mo), st), "slm_morph_loss")
            total = total + mo[0]
        return total

    def _corr_arg(self, flow, corr_points, required):
        if flow is not None and corr_points is not None:
            raise ValueError("give flow or corr_points, not both")
        corr = flow if flow is not None else corr_points
        if self.corr_mode and corr is None and required:
            raise ValueError("LM_Solver(corr_term=True): LM() needs flow= (1,2,H,W) or corr_points=(pts, nrm, valid)")
        return corr

    def LM(self, sf, inputs, new_data, u=10, v=7.5, minimal_loss=1e10, flow=None, corr_points=None):
        """(reference ``super/LM.py:81-122``) run ``opt.num_optimize_iterations`` damped
        iterations on the device; returns beta (J,7) float64 on ``sf``'s device.  ``flow`` (1,2,H,W), as
        ``GraphFit.infer_flow`` returns it, or ``corr_points = (pts, nrm, valid)``: the frame's correspondences
        (``corr_term=True`` only, where one of them is required)."""
        corr = self._corr_arg(flow, corr_points, required=True)
        return self.LM_batch([(sf, inputs, new_data, corr)], u=u, v=v, minimal_loss=minimal_loss)[0]

    def LM_batch(self, frames, u=10, v=7.5, minimal_loss=1e10):
        """Many independent frames / hypotheses advanced together in the same launches
        (one slot each).  ``frames`` is a list of ``(sf, inputs, new_data)``; with ``corr_term`` a fourth
        element per frame gives its correspondences: a flow, a ``(pts, nrm, valid)`` triple, or ``None``."""
        n = len(frames)
        if n < 1 or n > self.max_frames:
            raise ValueError(f"need 1..{self.max_frames} frames, got {n}")
        h = self._handle(u, v, minimal_loss)
        corrs = [fr[3] if len(fr) > 3 else None for fr in frames]
        frames = [tuple(fr[:3]) for fr in frames]
        rigid_recs = self._rigid_stage(frames, corrs, u, v, minimal_loss) if self.global_rigid else [None] * n
        bfs = self._bind_batch(h, frames) if n > 1 else [self._bind(h, 0, *frames[0])]
        for i, (bf, corr) in enumerate(zip(bfs, corrs)):
            self._bind_corr(h, i, bf, corr)
            self._bind_semantic(h, i, bf, frames[i][0], frames[i][2])
        if self.morph_on:
            self.last_edge_counts = [self._bind_morph(h, i, bf, frames[i][0], frames[i][1]) for i, bf in enumerate(bfs)]
        dev = bfs[0].device
        st = _stream_ptr(dev)
        if self.sharded:
            self._run_sharded(h, n, dev)
        else:
            _lib.check(self.lib.slm_run(h, n, st), "slm_run")
        betas, self.last_records = [], []
        for i, (bf, fr) in enumerate(zip(bfs, frames)):
            beta = torch.empty((bf.J, 7), dtype=torch.float64, device=dev)
            _lib.check(self.lib.slm_get_beta(h, i, _dev_ptr(beta), st), "slm_get_beta")
            betas.append(beta)
            recs = self.records(h, i, st)
            self.last_records.append(recs)
            self._report(fr[0], fr[1], recs, rigid_recs[i])
        if self.corr_mode:
            self.last_corr_kept = [None if c is None else self.corr_loss(i, u, v, minimal_loss)[1] for i, c in enumerate(corrs)]
        self._face_loss_of, self._face_loss = ((n, u, v, minimal_loss) if self.face_on else None), None
        self._morph_loss_of, self._morph_loss = ((n, u, v, minimal_loss) if self.morph_on else None), None
        return betas

    # ---- one frame sharded over several GPUs ------------------------------------------------
    def exchange_buffer(self, h, slot, what, dev):
        n = C.c_int64(0)
        _lib.check(self.lib.slm_lm_exchange_size(h, slot, what, C.byref(n)), "slm_lm_exchange_size")
        return torch.empty(n.value, dtype=torch.float64, device=dev)

    def exchange_view(self, h, slot, what, dev):
        """The library's exchange buffer itself as a tensor (aliased, not copied)."""
        from .dist import device_view
        ptr, n = C.c_void_p(), C.c_int64(0)
        _lib.check(self.lib.slm_lm_exchange_ptr(h, slot, what, C.byref(ptr), C.byref(n)), "slm_lm_exchange_ptr")
        return device_view(ptr.value, n.value, dev)

    def _exchange(self, h, n, what, op, bufs):
        # the collective runs in place on the library's buffer (kernels and collective share the current stream)
        for i in range(n):
            op(bufs[i])

    def _run_sharded(self, h, n, dev):
        """The LM loop with the three exchanges per iteration (see include/super_lm.h)."""
        for _ in self._sharded_stages(h, n, dev):
            pass

    def _sharded_stages(self, h, n, dev):
        """The stages of ``_run_sharded``, one per ``next()``: a stage is this rank's launches up to and including the
        collective that follows them (a driver that holds several ranks in one process steps them alternately; the
        collectives it injects then see every rank's buffer before the next stage reads it).  The pair records and the data
        loss are exchanged whenever the solver carries the data term -- ``opt.sf_point_plane`` or a semantic weight, which
        puts the term on without it (``_config``: use_data)."""
        st = _stream_ptr(dev)
        lib = self.lib
        data = bool(self.opt.sf_point_plane) or bool(self.seg_mode)
        pair = [self.exchange_view(h, i, _lib.SLM_X_PAIR_BLOCKS, dev) for i in range(n)] if data else []
        delta = [self.exchange_view(h, i, _lib.SLM_X_DELTA, dev) for i in range(n)]
        loss = [self.exchange_view(h, i, _lib.SLM_X_DATA_LOSS, dev) for i in range(n)] if data else []
        for _ in range(int(self.opt.num_optimize_iterations)):
            _lib.check(lib.slm_lm_grad_local(h, n, st), "slm_lm_grad_local")
            if data:
                self._exchange(h, n, _lib.SLM_X_PAIR_BLOCKS, self._all_reduce, pair)
            yield "grad"
            _lib.check(lib.slm_lm_solve(h, n, st), "slm_lm_solve")
            self._exchange(h, n, _lib.SLM_X_DELTA, self._broadcast, delta)
            yield "solve"
            _lib.check(lib.slm_lm_loss_local(h, n, st), "slm_lm_loss_local")
            if data:
                self._exchange(h, n, _lib.SLM_X_DATA_LOSS, self._all_reduce, loss)
            yield "loss"
            _lib.check(lib.slm_lm_accept(h, n, st), "slm_lm_accept")      # (reads the summed loss: behind the yield)

    # ---- helpers -----------------------------------------------------------------------
    def records(self, h, slot, stream):
        n = int(self.opt.num_optimize_iterations)
        arr = (SlmIterRecord * max(n, 1))()
        _lib.check(self.lib.slm_get_records(h, slot, arr, n, stream), "slm_get_records")
        return [dict(loss=r.loss, u=r.u, accepted=bool(r.accepted), status=int(r.status),
                     M_grad=int(r.M_grad), M_loss=int(r.M_loss)) for r in arr[:n]]

    def _rigid_stage(self, frames, corrs, u, v, minimal_loss):
        """The rigid pre-alignment of every frame: ``T_g`` into ``last_rigid``, every ``sf`` moved by its own.  With
        ``rigid_terms`` the stage carries the solver's terms, and a flow in ``corrs`` is REPLACED by the targets built from
        it on the unmoved model (what the node solve is then bound with)."""
        from .rigid import RigidAlign, rigid_update
        if len({id(fr[0]) for fr in frames}) != len(frames):
            raise ValueError("LM_Solver(global_rigid=True): the frames of a batch must not share an sf object (each is "
                             "moved by its own T_g)")
        if self._rigid is None:
            self._rigid = RigidAlign(self.opt, max_frames=self.max_frames,
                                     corr_term=self.rigid_terms and bool(self.corr_mode),
                                     weighted_data=self.rigid_terms and self.weighted)
        stage = frames
        if self.rigid_terms:
            if self.corr_mode:
                for i, (fr, corr) in enumerate(zip(frames, corrs)):
                    if torch.is_tensor(corr):
                        corrs[i] = self._rigid.corr_targets(*fr, corr)
            stage = [fr + (corr if self.corr_mode else None,) for fr, corr in zip(frames, corrs)]
        self.last_rigid = self._rigid.align_batch(stage, u=u, v=v, minimal_loss=minimal_loss)
        self.last_rigid_records = self._rigid.last_records
        for fr, tg in zip(frames, self.last_rigid):
            rigid_update(fr[0], tg)
        return self.last_rigid_records

    def _report(self, sf, inputs, recs, rigid_recs=None):
        for r in recs:
            if r["status"] == _lib.SLM_ITER_SOLVER_FAILED:
                print("\t\tSolver failed: Ill-posed system!")        # super/LM.py:102
            elif r["status"] == _lib.SLM_ITER_SOLVER_TIMEOUT:          # not a property of the matrix: say so
                print("\t\tSolver failed: the task-graph solve timed out (GPU scheduling), beta kept")
        done = [r for r in recs if r["status"] == _lib.SLM_ITER_OK]
        logger = getattr(sf, "logger", None)                         # defect D1: may be absent
        if self.opt.phase == "test" and logger is not None and done:
            fid = inputs["ID"].item() if "ID" in inputs else -1
            rdone = [r for r in (rigid_recs or []) if r["status"] == _lib.SLM_ITER_OK and r["accepted"]]
            stage = f" (rigid stage: {rdone[-1]['loss']})" if rdone else ""
            logger.info(f"{fid} loss: {done[-1]['loss']}{stage}")
