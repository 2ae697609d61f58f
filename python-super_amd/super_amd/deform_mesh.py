"""Host-side mirror of the reference's default per-frame optimiser ``GraphFit``
(``super/deform_mesh.py:10-379``) over libsuper_lm.so.

Same constructor and ``forward(inputs, src, trg, models)`` surface as the reference class,
so ``SuPer.__init__`` / ``SuPer.fusion`` (``super/super.py:20-21,70``) can use it unchanged:

    self.graph_fit = GraphFit(self.opt)
    deform_param = self.graph_fit(inputs, self.sf, sfdata, models)   # (J+1,7) float64

Supported loss flags: ``sf_point_plane``, ``mesh_arap``, ``mesh_rot``, ``mesh_face`` with their
weights, the Semantic-SuPer terms ``sf_soft_seg_point_plane`` / ``sf_hard_seg_point_plane`` /
``sf_bn_morph`` (+ ``sf_bn_morph_weight``, ``num_classes``), the ``max`` clip of the point-plane
term that ``depth_model == "raft_stereo"`` switches on, ``optimizer`` in {"SGD", "Adam"},
``learning_rate``, ``num_optimize_iterations``, and the surfel-correspondence term ``sf_corr``
(+ ``sf_corr_weight``, ``sf_corr_loss_type``): the flow network stays the caller's -- like the reference
(deform_mesh.py:19-23,302-309) ``forward`` calls ``models.optical_flow(src.rgb, inputs[("color",0)])`` once per
frame and hands the (1,2,H,W) flow to the library.  With ``sf_corr_match_renderimg`` (needs ``opt.renderer ==
"pulsar"``, radius ``opt.renderer_rad``) the flow is re-inferred every iteration from the rendered deformed model
instead (deform_mesh.py:292-305): iteration i renders the current deformed stable surfels on the device
(slm_gf_render, super_amd.renderer's blend), calls ``models.optical_flow(render (1,3,H,W), inputs[("color",0)])``,
binds the flow and takes one evaluation and step.  The reference also renders every iteration without that flag (the
``if True:`` at deform_mesh.py:294), but no output depends on that render, so this mirror does not make it: without
the flag (and without the render loss) the path is the single ``infer_flow`` on ``src.rgb`` and one ``slm_gf_run``.

The render loss ``opt.render_loss`` (+ ``render_loss_weight``, default 1e-4; deform_mesh.py:113-123) is opt-in:
``GraphFit(opt, native_render_loss=True)``.  Its gradient is the exact derivative of super_amd.renderer's blend
(slm_render_backward), not Pulsar's own backward, which cannot be pinned without pytorch3d; plain ``GraphFit(opt)``
raises for the flag.  Every iteration renders the deformed stable surfels (slm_gf_render) -- with
``sf_corr_match_renderimg`` that one render also feeds the flow network -- scores the SSIM-11 loss against
``inputs[("color",0)]`` with its image gradient (slm_render_ssim_loss), back-propagates it to the surfels
(slm_render_backward), binds that (slm_gf_bind_point_grad) and takes one evaluation and step.

``GraphFit(opt, native_render_loss=True, render_in_run=True)`` makes the render loss a term of the run instead: the
frame and the term are bound (slm_gf_bind_render_loss: one sizing render fixes the tile lists' entry limit) and ONE
``slm_gf_run`` enqueues every iteration's render, SSIM loss, backward, evaluation and step with no host round trip.  A render
whose tile lists would not fit the limit is empty and counted on the device; ``forward`` reads that status after the run and,
if any render overflowed, binds again with a limit of 1.25 x the largest total + 1024 and repeats the run (the bind resets the
state, so a repeat is a clean repeat; two repeats at most).  ``forward_frames`` runs up to ``max_frames`` frames in one
``slm_gf_run``, with or without the term, one ``RenderContext`` per slot.  ``sf_corr_match_renderimg`` needs the image on the
host side every iteration and is refused with ``render_in_run``.

``opt.renderer_surfel_radii`` (absent or False: nothing changes) renders every surfel with its own radius,
``src.radii * opt.renderer_radii_scale`` (default 1.0) as float32 by surfel row (slm_gf_render_radii), in place of the one
``opt.renderer_rad``: the same render feeds the render loss and ``sf_corr_match_renderimg``.  The radii are not optimised.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import SlmGfConfig, SlmGfFrame, SlmGfSemantic
from .LM import BoundFrame, _as, _dev_ptr, _stream_ptr


class GraphFit:
    """``GraphFit(opt)`` as in the reference.  ``rank`` / ``world`` (default: the
    ``torch.distributed`` rank and world size when ``shard_surfels=True``) split the surfels of
    one large frame over the GPUs of a node: every rank evaluates its block of surfels, the
    partial gradient / loss sums are all-reduced (RCCL) twice per optimiser iteration and every
    rank takes the same step (BASELINE configs[4])."""

    def __init__(self, opt, max_frames=1, shard_surfels=False, rank=None, world=None, all_reduce=None,
                 native_render_loss=False, render_in_run=False):
        self.opt = opt
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SuperLMError("no HIP device visible: super_amd has no CPU fallback")
        self.render_loss = bool(getattr(opt, "render_loss", False))
        if self.render_loss:
            if not native_render_loss:
                raise NotImplementedError(
                    "super_amd.GraphFit: opt.render_loss needs GraphFit(opt, native_render_loss=True): its gradient is "
                    "the exact derivative of super_amd.renderer's blend, not Pulsar's own backward, which is unpinned "
                    "(pytorch3d has no ROCm build)")
            self._refuse_unrenderable("opt.render_loss", shard_surfels or world is not None)
        self.render_loss_weight = float(getattr(opt, "render_loss_weight", 1e-4))
        self.last_render_kept = None
        self.match_render = bool(getattr(opt, "sf_corr", False) and getattr(opt, "sf_corr_match_renderimg", False))
        if self.match_render:
            self._refuse_unrenderable("opt.sf_corr_match_renderimg", shard_surfels or world is not None)
        self.render_in_run = bool(render_in_run)
        if self.render_in_run and self.match_render:
            raise NotImplementedError("super_amd.GraphFit: render_in_run with opt.sf_corr_match_renderimg: the flow network "
                                      "needs the render on the host side every iteration; use the stepwise form")
        self._render_ctx = None
        self._slot_ctx = [None] * max_frames       # render_in_run: one RenderContext per slot
        self._slot_radii = [None] * max_frames
        self._entry_limit_once = 0                 # tests: the entry limit of the next in-run bind of every slot, once
        self.last_render_status = None             # render_in_run: per frame (loss, kept, overflowed renders, largest total)
        self.render_repeats = 0                    # render_in_run: repeats the last forward needed
        # opt-in: the renders of this class give every surfel its own radius, src.radii * renderer_radii_scale
        # (slm_gf_render_radii), instead of opt.renderer_rad; the radii are not optimised (no radius gradient is asked for)
        self.surfel_radii = bool(getattr(opt, "renderer_surfel_radii", False))
        self.radii_scale = float(getattr(opt, "renderer_radii_scale", 1.0))
        self.valid_margin = 1
        self.optim = opt.optimizer
        self.Niter = opt.num_optimize_iterations
        if self.optim not in ("SGD", "Adam"):
            raise NotImplementedError(f"optimizer {self.optim!r}")
        self.max_frames = max_frames
        cfg = SlmGfConfig()
        cfg.num_iterations = int(self.Niter)
        cfg.optimizer = 0 if self.optim == "SGD" else 1
        cfg.use_data = int(bool(opt.sf_point_plane))
        cfg.use_arap = int(bool(opt.mesh_arap))
        cfg.use_rot = int(bool(opt.mesh_rot))
        cfg.use_face = int(bool(getattr(opt, "mesh_face", False)))
        cfg.max_frames = max_frames
        cfg.w_data = float(getattr(opt, "sf_point_plane_weight", 1.0))
        cfg.w_arap = float(getattr(opt, "mesh_arap_weight", 10.0))
        cfg.w_rot = float(getattr(opt, "mesh_rot_weight", 1.0))
        cfg.w_face = float(getattr(opt, "mesh_face_weight", 1.0))
        cfg.lr = float(opt.learning_rate)
        # Semantic-SuPer (deform_mesh.py:76-99,126-194): soft wins over hard (loss.py:384)
        soft = bool(getattr(opt, "sf_soft_seg_point_plane", False))
        hard = bool(getattr(opt, "sf_hard_seg_point_plane", False))
        cfg.seg_mode = 2 if soft else (1 if hard else 0)
        cfg.use_bn_morph = int(bool(getattr(opt, "sf_bn_morph", False)))
        cfg.w_bn_morph = float(getattr(opt, "sf_bn_morph_weight", 0.1))
        cfg.pp_max = 2e-5 if getattr(opt, "depth_model", None) == "raft_stereo" else 0.0
        if getattr(opt, "sf_corr", False):                 # deform_mesh.py:100-109
            lt = getattr(opt, "sf_corr_loss_type", "point-point")
            if lt not in ("point-point", "point-plane"):
                raise ValueError(f"sf_corr_loss_type {lt!r}")
            cfg.corr_mode = 1 if lt == "point-point" else 2
            cfg.w_corr = float(getattr(opt, "sf_corr_weight", 0.001))
        self.semantic = bool(cfg.seg_mode or cfg.use_bn_morph)
        self.flow = None
        self.edge_counts = None
        self.cfg = cfg
        self.h = C.c_void_p()
        _lib.check(self.lib.slm_gf_create(C.byref(cfg), C.byref(self.h)), "slm_gf_create")
        self._keep = [None] * max_frames
        self.rank, self.world, self._all_reduce = 0, 1, all_reduce
        self.sharded = bool(shard_surfels or world is not None)   # (a world of one rank runs the same protocol)
        if self.sharded:
            import torch.distributed as dist
            if world is None:
                world, rank = dist.get_world_size(), dist.get_rank()
            self.rank, self.world = int(rank), int(world)
            if self._all_reduce is None:
                from .dist import default_collectives
                self._all_reduce = default_collectives()[0]         # sum, in place (RCCL on the GPU box; host-staged under gloo)
            _lib.check(self.lib.slm_gf_set_shard(self.h, self.rank, self.world), "slm_gf_set_shard")

    def __del__(self):
        try:
            if self.h:
                self.lib.slm_gf_destroy(self.h)
        except Exception:
            pass

    def _refuse_unrenderable(self, flag, sharded):
        """The refusals of a flag that renders the deformed model: the reference renders with models.renderer, which
        InitNets only builds for opt.renderer == "pulsar", and a render needs every surfel of the frame on one device."""
        renderer = getattr(self.opt, "renderer", None)
        if renderer != "pulsar":
            raise NotImplementedError(f"super_amd.GraphFit: {flag} renders with opt.renderer; "
                                      f"only 'pulsar' is implemented (got {renderer!r})")
        if sharded:
            raise NotImplementedError(f"super_amd.GraphFit: {flag} on surfel-sharded frames")

    def infer_flow(self, models, source_img, target_img):
        """(reference ``deform_mesh.py:19-23``) the caller's flow network; the last element of a list output."""
        flow = models.optical_flow(source_img, target_img)   # x, y
        if isinstance(flow, (list, tuple)):
            flow = flow[-1]
        return flow.detach()

    def _bind(self, slot, inputs, src, trg, models=None, flow=None, defer_flow=False):
        new_data = trg
        if not hasattr(trg, "valid"):            # not read on this path
            trg = type("T", (), {})()
            trg.points, trg.norms, trg.index_map = new_data.points, new_data.norms, new_data.index_map
            trg.valid = torch.zeros(new_data.index_map.numel(), dtype=torch.bool,
                                    device=new_data.points.device)
        bf = BoundFrame(src, inputs, trg, state=getattr(self.opt, "slm_state_dtype", None))
        dev = bf.device
        sdt = bf.state_dtype       # ED_nodes.knn_w / triangle areas follow the dtype of the state
        ed = src.ED_nodes
        fr = SlmGfFrame()
        fr.base = bf.c
        keep = [bf]
        stable = getattr(src, "isStable", None)
        if stable is not None:
            st8 = _as(stable, torch.uint8, dev)
            keep.append(st8)
            fr.sf_stable = _dev_ptr(st8)
        w = _as(ed.knn_w, sdt, dev)
        keep.append(w)
        fr.ed_knn_w = _dev_ptr(w)
        if self.cfg.use_face:
            tri = _as(ed.triangles, torch.int32, dev)
            area = _as(ed.triangles_areas, sdt, dev)
            keep += [tri, area]
            fr.ed_triangles, fr.ed_triangle_areas = _dev_ptr(tri), _dev_ptr(area)
            fr.n_triangles = int(tri.shape[1])
        _lib.check(self.lib.slm_gf_bind_frame(self.h, slot, C.byref(fr), _stream_ptr(dev)),
                   "slm_gf_bind_frame")
        self._keep[slot] = keep      # (what the slot's device pointers refer to; the binds below add to it)
        if self.semantic:
            # src.seg / src.seg_conf (deform_mesh.py:262-264), trg.seg_conf (loss.py:350),
            # inputs[("seg_conf",0)] / inputs[("seg",0)] (deform_mesh.py:136,149)
            sem = SlmGfSemantic()
            nc = int(getattr(self.opt, "num_classes", src.seg_conf.shape[1]))
            sem.num_classes = nc
            seg = _as(src.seg, torch.int32, dev)
            keep.append(seg)
            sem.sf_seg = _dev_ptr(seg)
            if self.cfg.seg_mode:
                sconf = _as(src.seg_conf, torch.float32, dev)
                tconf = _as(new_data.seg_conf, torch.float32, dev)
                if sconf.shape[1] != nc or tconf.shape[1] != nc:
                    raise ValueError("seg_conf must have opt.num_classes columns")
                keep += [sconf, tconf]
                sem.sf_seg_conf, sem.tgt_seg_conf = _dev_ptr(sconf), _dev_ptr(tconf)
            if self.cfg.use_bn_morph:
                iconf = _as(inputs[("seg_conf", 0)][0], torch.float32, dev)
                iseg = inputs[("seg", 0)]
                if iseg.shape[1] > 1:                      # find_edge_region: argmax over channels
                    iseg = torch.argmax(iseg, dim=1, keepdim=True)
                iseg = _as(iseg[0, 0], torch.int32, dev)
                if iconf.shape[0] != nc:
                    raise ValueError('inputs[("seg_conf",0)] must have opt.num_classes channels')
                keep += [iconf, iseg]
                sem.img_seg_conf, sem.img_seg = _dev_ptr(iconf), _dev_ptr(iseg)
            counts = (C.c_int32 * 4)()
            _lib.check(self.lib.slm_gf_bind_semantic(self.h, slot, C.byref(sem), counts, _stream_ptr(dev)),
                       "slm_gf_bind_semantic")
            self.edge_counts = list(counts)[:nc]
        if self.cfg.corr_mode and not defer_flow:
            if flow is None:
                if models is None or not hasattr(models, "optical_flow"):
                    raise ValueError("opt.sf_corr needs models.optical_flow (or flow=...)")   # the reference asserts
                flow = self.infer_flow(models, src.rgb, inputs[("color", 0)])
            self.flow = flow
            self._bind_flow(slot, flow)
        if self.surfel_radii:      # float32 by surfel row, like Pulsar's vert_rad
            radii = (src.radii.detach() * self.radii_scale).to(device=dev, dtype=torch.float32).contiguous()
            if tuple(radii.shape) != (bf.c.N,):
                raise ValueError(f"src.radii must be ({bf.c.N},), got {tuple(src.radii.shape)}")
            keep.append(radii)
            self._slot_radii[slot] = radii
        return bf

    def forward(self, inputs, src, trg, models=None):
        """(reference ``deform_mesh.py:232-247``) returns deform_verts (J+1,7) float64."""
        if getattr(self.opt, "deform_udpate_method", "super_edg") != "super_edg":
            raise NotImplementedError("only deform_udpate_method == 'super_edg'")
        if self.render_loss and self.render_in_run:
            return self.forward_frames([(inputs, src, trg)], models)[0]
        if self.render_loss:
            return self._forward_render_loss(inputs, src, trg, models)
        if self.match_render:
            return self._forward_match_render(inputs, src, trg, models)
        bf = self._bind(0, inputs, src, trg, models)
        if self.sharded:
            self._iterate(part=torch.empty((bf.J + 1) * 7 + _lib.GF_NTERMS, dtype=torch.float64, device=bf.device))
        else:
            _lib.check(self.lib.slm_gf_run(self.h, 1, self._st()), "slm_gf_run")
        return self.deform_verts()

    def _iterate(self, before=None, part=None):
        """The per-iteration loop of every stepwise path: ``before()`` -- what the path binds for this iteration's
        evaluation -- then the two passes of the evaluation and the step.  ``part``: the frame is surfel-sharded and the
        partial sums are exchanged through this buffer behind each pass."""
        for _ in range(int(self.Niter)):
            if before is not None:
                before()
            self.eval_morph()
            if part is not None and self.cfg.use_bn_morph:
                self.exchange_partial(part)      # global kept count before the back-propagation
            self.eval_losses()
            if part is not None:
                self.exchange_partial(part)      # gradient + loss terms
            self.step()

    __call__ = forward

    def _bind_render_term(self, slot, inputs, src, entry_limit=0):
        """Binds the render loss to ``slot`` as a term of the run (slm_gf_bind_render_loss), after ``_bind`` of the same
        frame: the slot's own ``RenderContext``, ``src.colors``, the radii of ``opt.renderer_surfel_radii`` and
        ``inputs[("color",0)]`` as the target.  ``entry_limit`` 0: from the sizing render."""
        bf = self._keep[slot][0]
        dev = bf.device
        # (the frame's bind took the term, and with it the old context, off the slot)
        ctx, p = self._fresh_ctx(self._slot_ctx[slot], bf, inputs)
        self._slot_ctx[slot] = ctx
        tgt = inputs[("color", 0)].detach()
        tgt = tgt.reshape(tgt.shape[-3:]) if tgt.dim() == 4 else tgt
        if tuple(tgt.shape) != (3, p.height, p.width):
            raise ValueError(f'inputs[("color",0)] must be (3,{p.height},{p.width}) or (1,3,{p.height},{p.width}), '
                             f"got {tuple(tgt.shape)}")
        tgt = tgt.to(device=dev, dtype=torch.float32).contiguous()
        colors = self._colors(slot, src)
        radii = self._slot_radii[slot] if self.surfel_radii else None
        self._keep[slot].append(tgt)
        _lib.check(self.lib.slm_gf_bind_render_loss(
            self.h, slot, ctx.h, C.byref(p), _dev_ptr(radii) if radii is not None else None, _dev_ptr(colors),
            int(colors.stride(0)), _dev_ptr(tgt), self.render_loss_weight, int(entry_limit), _stream_ptr(dev)),
            "slm_gf_bind_render_loss")
        return p

    def render_loss_status(self, slot=0):
        """(weighted loss, kept pixels) of the slot's last in-run evaluation, the renders over the entry limit and the
        largest tile-list total since its bind (slm_gf_render_loss_status; synchronises)."""
        out = (C.c_double * 4)()
        _lib.check(self.lib.slm_gf_render_loss_status(self.h, slot, out, self._st()), "slm_gf_render_loss_status")
        return float(out[0]), int(out[1]), int(out[2]), int(out[3])

    def forward_frames(self, frames, models=None, render_frames=None):
        """Up to ``max_frames`` frames, a list of ``(inputs, src, trg)``, in ONE ``slm_gf_run``: the list of their
        deform_verts (J+1,7) float64.  All frames need the same ``num_neighbors``.  With ``opt.render_loss`` (needs
        ``render_in_run=True``) every frame has the term, or those whose entry of ``render_frames`` (a list of bools) is
        true; ``self.last_render_status`` then holds per frame (loss, kept, overflowed renders, largest total) or None.
        If a render overflowed its tile lists' entry limit, the frames are bound again -- that frame with a limit of 1.25 x
        its largest total + 1024 -- and the run is repeated, twice at most."""
        if getattr(self.opt, "deform_udpate_method", "super_edg") != "super_edg":
            raise NotImplementedError("only deform_udpate_method == 'super_edg'")
        n = len(frames)
        if n < 1 or n > self.max_frames:
            raise ValueError(f"forward_frames: {n} frames, max_frames is {self.max_frames}")
        if self.sharded:
            raise NotImplementedError("super_amd.GraphFit: forward_frames on surfel-sharded frames")
        if self.match_render:
            raise NotImplementedError("super_amd.GraphFit: forward_frames with opt.sf_corr_match_renderimg")
        if self.render_loss and not self.render_in_run:
            raise NotImplementedError("super_amd.GraphFit: forward_frames with opt.render_loss needs render_in_run=True")
        term = [self.render_loss] * n if render_frames is None else [bool(t) and self.render_loss for t in render_frames]
        if len(term) != n:
            raise ValueError("forward_frames: render_frames must have one entry per frame")
        limits = [self._entry_limit_once] * n
        self._entry_limit_once = 0
        self.render_repeats = 0
        while True:
            for k, (inputs, src, trg) in enumerate(frames):
                self._bind(k, inputs, src, trg, models)
                if term[k]:
                    self._bind_render_term(k, inputs, src, limits[k])
            _lib.check(self.lib.slm_gf_run(self.h, n, self._st()), "slm_gf_run")
            status = [self.render_loss_status(k) if term[k] else None for k in range(n)]
            over = [k for k in range(n) if status[k] is not None and status[k][2] > 0]
            if not over:
                break
            if self.render_repeats == 2:
                raise _lib.SuperLMError(
                    "super_amd.GraphFit: renders still overflow their tile lists after two repeats (frames "
                    f"{over}, largest totals {[status[k][3] for k in over]}, limits {[limits[k] for k in over]})")
            for k in over:
                limits[k] = status[k][3] + status[k][3] // 4 + 1024
            self.render_repeats += 1
        self.last_render_status = status
        if status[0] is not None:
            self.last_render_kept = status[0][1]
        return [self.deform_verts(k) for k in range(n)]

    def _forward_match_render(self, inputs, src, trg, models):
        """deform_mesh.py:286-330 with sf_corr_match_renderimg: per iteration render -> flow -> bind -> step."""
        if models is None or not hasattr(models, "optical_flow"):
            raise ValueError("opt.sf_corr needs models.optical_flow")   # the reference asserts
        self._bind(0, inputs, src, trg, models, defer_flow=True)
        colors = self._colors(0, src)        # bound once per frame

        def before():
            self.flow = self.infer_flow(models, self.render_deformed(inputs, colors), inputs[("color", 0)])
            self._bind_flow(0, self.flow)

        self._iterate(before)
        return self.deform_verts()

    def _forward_render_loss(self, inputs, src, trg, models):
        """deform_mesh.py:286-330 with opt.render_loss: per iteration render -> (flow of that render, with
        sf_corr_match_renderimg) -> SSIM loss and its image gradient -> renderer backward -> bind -> step."""
        if self.match_render and (models is None or not hasattr(models, "optical_flow")):
            raise ValueError("opt.sf_corr needs models.optical_flow")   # the reference asserts
        # without sf_corr_match_renderimg the flow (sf_corr) is inferred once from src.rgb at the bind (iteration 0)
        bf = self._bind(0, inputs, src, trg, models, defer_flow=self.match_render)
        colors = self._colors(0, src)

        def before():
            img, p = self._render_deformed_hwc(inputs, colors)
            if self.match_render:
                self.flow = self.infer_flow(models, img.permute(2, 0, 1).unsqueeze(0), inputs[("color", 0)])
                self._bind_flow(0, self.flow)
            self._bind_render_grad(bf, inputs, img, p)

        self._iterate(before)
        _lib.check(self.lib.slm_gf_bind_point_grad(self.h, 0, None, _stream_ptr(bf.device)), "slm_gf_bind_point_grad")
        return self.deform_verts()

    def _bind_render_grad(self, bf, inputs, img, p):
        """SSIM loss of the render ``img`` (h,w,3) and its gradient, back through the renderer, bound as the slot's
        point gradient; returns the (2,) device [weighted loss, kept pixels]."""
        from .renderer import render_backward, ssim_render_loss_device
        out, gimg = ssim_render_loss_device(img, inputs[("color", 0)], self.render_loss_weight, with_grad=True)
        gp = render_backward(self._render_ctx, p, gimg)
        self._keep[0].append(gp)         # read by the next evaluation
        _lib.check(self.lib.slm_gf_bind_point_grad(self.h, 0, _dev_ptr(gp), _stream_ptr(bf.device)),
                   "slm_gf_bind_point_grad")
        return out

    def _bind_flow(self, slot, flow):
        bf = self._keep[slot][0]
        fl = _as(flow, torch.float32, bf.device)
        if tuple(fl.shape) != (1, 2, bf.c.H, bf.c.W):
            raise ValueError(f"flow must be (1,2,{bf.c.H},{bf.c.W}), got {tuple(fl.shape)}")
        self._keep[slot].append(fl)      # read by the next evaluation
        _lib.check(self.lib.slm_gf_bind_flow(self.h, slot, _dev_ptr(fl), _stream_ptr(bf.device)), "slm_gf_bind_flow")

    def _colors(self, slot, src):
        """``src.colors`` as the renderer reads them, (N,3) float32 by surfel row, kept alive with the slot."""
        colors = src.colors.detach().to(device=self._keep[slot][0].device, dtype=torch.float32).contiguous()
        self._keep[slot].append(colors)
        return colors

    def _fresh_ctx(self, ctx, bf, inputs):
        """(context, render parameters) for a render of the bound frame ``bf``: ``ctx`` if it holds H x W, else a new
        ``RenderContext``, with room for the frame's surfels and marked fresh (nothing of an earlier render is reused)."""
        from .renderer import DEFAULT_RAD, RenderContext, render_params
        H, W = bf.c.H, bf.c.W
        if ctx is None or ctx.H < H or ctx.W < W:
            ctx = RenderContext(H, W)
        ctx.reserve(bf.c.N)
        ctx.last_n = 0
        ctx.serial += 1
        return ctx, render_params(inputs["K"], H, W, 1.0, getattr(self.opt, "renderer_rad", DEFAULT_RAD))

    def render_deformed(self, inputs, colors):
        """The current deformed stable surfels of the bound frame (deform_source's new_data, global row included)
        rendered like ``models.renderer(inputs, new_data, rad=opt.renderer_rad)``: (1,3,H,W) float32, permuted
        like the reference (deform_mesh.py:295-298).  ``colors`` (N,3) float32 is indexed by surfel row."""
        return self._render_deformed_hwc(inputs, colors)[0].permute(2, 0, 1).unsqueeze(0)

    def _render_deformed_hwc(self, inputs, colors):
        """``render_deformed`` as the (h,w,3) float32 image, with the render parameters.  With
        ``opt.renderer_surfel_radii`` every surfel has its own radius (bound by ``_bind``); ``opt.renderer_rad`` then
        only has to be valid."""
        bf = self._keep[0][0]
        ctx, p = self._fresh_ctx(self._render_ctx, bf, inputs)
        self._render_ctx = ctx
        img = torch.empty((p.height, p.width, 3), dtype=torch.float32, device=bf.device)
        if self.surfel_radii:
            _lib.check(self.lib.slm_gf_render_radii(self.h, 0, ctx.h, C.byref(p), _dev_ptr(self._slot_radii[0]),
                                                    _dev_ptr(colors), int(colors.stride(0)), _dev_ptr(img), None, None,
                                                    _stream_ptr(bf.device)), "slm_gf_render_radii")
        else:
            _lib.check(self.lib.slm_gf_render(self.h, 0, ctx.h, C.byref(p), _dev_ptr(colors), int(colors.stride(0)),
                                              _dev_ptr(img), None, None, _stream_ptr(bf.device)), "slm_gf_render")
        ctx.last_n = bf.c.N
        return img, p

    # ---- stepwise evaluation (surfel-sharded frames; also usable with world == 1) -------------
    def _st(self):
        return _stream_ptr(self._keep[0][0].device)

    def bind(self, inputs, src, trg, models=None, flow=None):
        return self._bind(0, inputs, src, trg, models, flow)

    def eval_morph(self):
        _lib.check(self.lib.slm_gf_eval_morph(self.h, 1, self._st()), "slm_gf_eval_morph")

    def eval_losses(self):
        _lib.check(self.lib.slm_gf_eval_losses(self.h, 1, self._st()), "slm_gf_eval_losses")

    def step(self):
        _lib.check(self.lib.slm_gf_step(self.h, 1, self._st()), "slm_gf_step")

    def get_partial(self, out):
        _lib.check(self.lib.slm_gf_get_partial(self.h, 0, _dev_ptr(out), self._st()), "slm_gf_get_partial")
        return out

    def set_partial(self, buf):
        _lib.check(self.lib.slm_gf_set_partial(self.h, 0, _dev_ptr(buf), self._st()), "slm_gf_set_partial")

    def exchange_partial(self, buf):
        """partial [(J+1)*7 gradient | GF_NTERMS terms] -> sum over the ranks -> back into the slot."""
        self.get_partial(buf)
        self._all_reduce(buf)
        self.set_partial(buf)

    def deform_verts(self, slot=0):
        bf = self._keep[slot][0]
        out = torch.empty((bf.J + 1, 7), dtype=torch.float64, device=bf.device)
        _lib.check(self.lib.slm_gf_get_deform(self.h, slot, _dev_ptr(out), _stream_ptr(bf.device)), "slm_gf_get_deform")
        return out

    def loss_and_grad(self, inputs, src, trg, deform_verts, models=None, flow=None):
        """One evaluation of ``deform_source`` + ``get_losses`` + backward at ``deform_verts``:
        returns (dict of weighted loss terms, matched count, gradient (J+1,7) with the global
        row divided by J).  With the render loss (``native_render_loss``) the dict also holds ``render_loss``
        (weighted; the render is made at ``deform_verts`` from ``src.colors``), the gradient includes it and
        ``self.last_render_kept`` is its kept pixel count."""
        bf = self._bind(0, inputs, src, trg, models, flow)
        st = _stream_ptr(bf.device)
        dv = _as(deform_verts, torch.float64, bf.device)
        terms = torch.zeros(_lib.GF_NTERMS, dtype=torch.float64, device=bf.device)
        grad = torch.zeros((bf.J + 1, 7), dtype=torch.float64, device=bf.device)
        rl = None
        if self.render_loss:
            # a first evaluation puts deform_verts into the slot, where slm_gf_render reads it
            _lib.check(self.lib.slm_gf_loss_grad(self.h, 0, _dev_ptr(dv), None, None, st), "slm_gf_loss_grad")
            img, p = self._render_deformed_hwc(inputs, self._colors(0, src))
            rl = self._bind_render_grad(bf, inputs, img, p)
        _lib.check(self.lib.slm_gf_loss_grad(self.h, 0, _dev_ptr(dv), _dev_ptr(terms), _dev_ptr(grad), st),
                   "slm_gf_loss_grad")
        if rl is not None:
            _lib.check(self.lib.slm_gf_bind_point_grad(self.h, 0, None, st), "slm_gf_bind_point_grad")
        t = terms.cpu().tolist()
        d = dict(face_losses=t[0], arap_loss=t[1], rot_loss=t[2], point_plane_loss=t[3])
        if self.cfg.use_bn_morph and t[7] != 0.0:       # the reference only adds the key when a class contributes
            d["sf_bn_morph_loss"] = t[5]
        self.last_bn_morph_kept = int(t[6])
        if self.cfg.corr_mode:
            d["corr_loss"] = t[8]
            self.last_corr_kept = int(t[9])
        if rl is not None:
            loss, kept = rl.cpu().tolist()
            d["render_loss"] = loss
            self.last_render_kept = int(kept)
        return d, int(t[4]), grad

    def edge_points(self, class_id):
        """Boundary pixels (x,y) of ``class_id`` extracted at the last bind (``self.edge_pts`` of the
        reference, deform_mesh.py:145-165), float32 (E,2) on the device."""
        n = self.edge_counts[class_id]
        dev = self._keep[0][0].device
        out = torch.empty((n, 2), dtype=torch.float32, device=dev)
        _lib.check(self.lib.slm_gf_get_edge_points(self.h, 0, class_id, _dev_ptr(out), n, _stream_ptr(dev)),
                   "slm_gf_get_edge_points")
        return out
