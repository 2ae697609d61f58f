"""Timing: one surfel render (slm_render_points) at 480x640 for 300 k make_scene surfels at the default radius
(opt.renderer_rad = 2e-4) and at 10x, and one GraphFit frame (10 SGD iterations, sf_corr) with and without
sf_corr_match_renderimg, the flow network an identity stand-in (returns a zero flow at once).  The render loss: at
both radii one forward + SSIM loss with its image gradient + renderer backward (and the loss + backward alone, after
a forward), the same with the colour gradient as well (slm_render_backward_ex), one differentiable render + backward
through torch (Pulsar(opt, differentiable=True), gradients to the points and the colours), and one GraphFit frame
(10 SGD iterations) with opt.render_loss (native_render_loss=True).

    python tools/time_render.py [--reps 30] [--out gpu_out.json]
    python tools/time_render.py --radii [--reps 30] [--out gpu_out.json]
    python tools/time_render.py --channels 6 [--radii] [--reps 30] [--out gpu_out.json]

``--radii`` times the per-point render instead (slm_render_points_radii): the same 300 k surfels at 480x640 with the
radii of the reference's formula, Z / (sqrt(2) f clamp(|n_z|, 0.26, 1)); beside the two one-radius forwards it reports
the per-point forward, forward + SSIM loss + backward (the point gradient; with the radius gradient as well), the loss +
backward alone, and the fractions of pixels hit and kept.

``--channels C`` times the N-channel render (slm_render_points_channels) on the same scene at 2e-4, at 2e-3 and, with
``--radii``, with the formula's radii: the C-channel forward, the same columns as ceil(C/3) three-channel renders (what
the C channels cost before), and the channels backward (points and features; with the radii as well under ``--radii``) for a
random dL/dimage, after one forward.

``--in-run`` times one GraphFit frame at C2 (200 k surfels, 2 000 nodes, 10 SGD iterations) four ways, interleaved in one
process, at renderer_rad 2e-4, at 2e-3 and with the formula's per-surfel radii: without the render loss (``plain``), with it
stepwise (``native_render_loss=True``), with it inside the run (``render_in_run=True``), and ``--frames B`` (default 8) such
frames in one ``slm_gf_run`` (``forward_frames``; reported per frame).  Every timed call is the whole ``forward``, binds
included.  ``--no-in-run-forms`` leaves the two in-run forms out (a library without them: SLM_LIB names another build).

HIP events around each call after warm-up; median and maximum over --reps runs.  A render synchronises once
inside (the tile-list total is read back), so a timed call includes that round trip.  Kernel times: run it under
``rocprofv3 --kernel-trace --stats -- python tools/time_render.py``."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-super_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return {"median_us": float(np.median(ts)), "max_us": float(np.max(ts)), "reps": reps}


def _time_interleaved(fns, reps, warm=2):
    """{name: fn} -> {name: median / min / max in us}: the calls take turns, rep by rep, in one process"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v)), "reps": reps}
            for k, v in ts.items()}


def in_run_mode(a):
    from helpers import torch_frame
    from oracle import graphfit_oracle as gfo
    from super_amd import synth
    from super_amd.deform_mesh import GraphFit
    B, res = a.frames, {}
    gsc = synth.make_scene(seed=0, **synth.WORKLOADS["C2"])
    sf, ginputs, new_data = torch_frame(gsc)
    sf.colors = torch.rand(gsc.N, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    sf.rgb = torch.zeros(1, 3, gsc.H, gsc.W, device="cuda")
    nz = np.clip(np.abs(gsc.sf_norms[:, 2].astype(np.float64)), 0.26, 1.0)
    sf.radii = torch.from_numpy(gsc.sf_points[:, 2].astype(np.float64) / (np.sqrt(2.0) * gsc.K[0, 0] * nz)).cuda()
    ginputs = dict(ginputs)
    ginputs[("color", 0)] = torch.zeros(1, 3, gsc.H, gsc.W, device="cuda")

    def opt_of(rad, radii, loss):
        o = gfo.default_opt(renderer="pulsar", renderer_rad=rad, render_loss=loss, render_loss_weight=1e-4)
        o.deform_udpate_method = "super_edg"
        o.renderer_surfel_radii = radii
        return o

    for key, rad, radii in (("rad2e-4", 2e-4, False), ("rad2e-3", 2e-3, False), ("radii", 2e-4, True)):
        step = GraphFit(opt_of(rad, radii, True), native_render_loss=True)
        step._bind(0, ginputs, sf, new_data)              # the colour frame: the render at identity, brightened
        inp = dict(ginputs)
        inp[("color", 0)] = (step.render_deformed(inp, sf.colors.float().contiguous()) + 0.01).contiguous()
        plain = GraphFit(opt_of(rad, radii, False))
        fns = {"plain": lambda: plain(inp, sf, new_data, None), "stepwise": lambda: step(inp, sf, new_data, None)}
        if not a.no_in_run_forms:
            one = GraphFit(opt_of(rad, radii, True), native_render_loss=True, render_in_run=True)
            many = GraphFit(opt_of(rad, radii, True), max_frames=B, native_render_loss=True, render_in_run=True)
            plain_many = GraphFit(opt_of(rad, radii, False), max_frames=B)
            fns["in_run"] = lambda: one(inp, sf, new_data, None)
            fns[f"in_run_b{B}"] = lambda: many.forward_frames([(inp, sf, new_data)] * B)
            fns[f"plain_b{B}"] = lambda: plain_many.forward_frames([(inp, sf, new_data)] * B)
        t = _time_interleaved(fns, a.reps)
        for k, v in t.items():
            if k.endswith(f"_b{B}"):
                v["per_frame_median_us"] = v["median_us"] / B
            res[f"graphfit_{k}_{key}"] = v
        if not a.no_in_run_forms:
            res[f"graphfit_in_run_{key}"]["status"] = one.last_render_status[0]
            res[f"graphfit_in_run_{key}"]["repeats"] = one.render_repeats
    res["graphfit_surfels"], res["frames"] = gsc.N, B
    return res


def radii_mode(a):
    from types import SimpleNamespace

    from super_amd import synth
    from super_amd.renderer import (DEFAULT_RAD, Pulsar, render_backward, render_backward_ex, render_params,
                                    ssim_render_loss_device)
    res = {}
    sc = synth.make_scene(N=300_000, J=512, H=480, W=640, seed=5, src_border=2)
    pts = torch.from_numpy(sc.sf_points).cuda()
    cols = torch.from_numpy(np.random.default_rng(2).uniform(size=(sc.N, 3)).astype(np.float32)).cuda()
    nz = np.clip(np.abs(sc.sf_norms[:, 2].astype(np.float64)), 0.26, 1.0)
    radii = torch.from_numpy((sc.sf_points[:, 2].astype(np.float64) / (np.sqrt(2.0) * sc.K[0, 0] * nz)).astype(np.float32)).cuda()
    inputs = {"K": torch.from_numpy(sc.K).float()[None].cuda()}
    r = Pulsar(SimpleNamespace(height=sc.H, width=sc.W))
    data = SimpleNamespace(points=pts, colors=cols)
    gen = torch.Generator("cuda").manual_seed(3)
    for name, rad in (("render_rad2e-4", 2e-4), ("render_rad2e-3", 2e-3), ("render_radii", radii)):
        res[name] = _time(lambda: r(inputs, data, rad=rad), a.reps)
        img, _, cnt = r.render(inputs, data, rad=rad, with_info=True)
        tgt = (img.permute(2, 0, 1) + 0.01 * torch.randn(3, sc.H, sc.W, device="cuda", generator=gen)).contiguous()
        out, _ = ssim_render_loss_device(img, tgt, 1e-4, with_grad=False)
        res[name]["pixels_hit"] = float((cnt > 0).float().mean())
        res[name]["pixels_kept"] = float(out[1]) / (sc.H * sc.W)
        res[name]["hits_per_pixel_mean"] = float(cnt.float().mean())
        res[name]["hits_per_pixel_max"] = int(cnt.max())
        ctx = r.context()
        p = render_params(inputs["K"], sc.H, sc.W, 1.0, DEFAULT_RAD if torch.is_tensor(rad) else rad)
        key = name[len("render_"):]

        def loss_bwd():
            _, g = ssim_render_loss_device(loss_bwd.img, tgt, 1e-4)
            return render_backward(ctx, p, g)

        def fwd_loss_bwd():
            loss_bwd.img = r(inputs, data, rad=rad)
            return loss_bwd()

        fwd_loss_bwd()
        res["render_fwd_ssim_bwd_" + key] = _time(fwd_loss_bwd, a.reps)
        fwd_loss_bwd()
        res["render_ssim_bwd_" + key] = _time(loss_bwd, a.reps)
        if torch.is_tensor(rad):
            def loss_bwd_all():
                _, g = ssim_render_loss_device(loss_bwd.img, tgt, 1e-4)
                return render_backward_ex(ctx, p, g, radii=True)

            fwd_loss_bwd()
            res["render_ssim_bwd_points_colors_radii_" + key] = _time(loss_bwd_all, a.reps)
    res["render_points"] = sc.N
    res["radii_px"] = [float((radii * sc.K[0, 0] / pts[:, 2]).min()), float((radii * sc.K[0, 0] / pts[:, 2]).max())]
    return res


def channels_mode(a):
    from super_amd import synth
    from super_amd.renderer import (DEFAULT_RAD, RenderContext, render_backward_channels, render_channels, render_params,
                                    render_points)
    nch, res = a.channels, {}
    sc = synth.make_scene(N=300_000, J=512, H=480, W=640, seed=5, src_border=2)
    pts = torch.from_numpy(sc.sf_points).cuda()
    feat = torch.from_numpy(np.random.default_rng(2).uniform(size=(sc.N, nch)).astype(np.float32)).cuda()
    groups = []                                    # the same columns, three at a time, padded with zeros
    for c0 in range(0, nch, 3):
        cols = torch.zeros((sc.N, 3), dtype=torch.float32, device="cuda")
        cols[:, :min(3, nch - c0)] = feat[:, c0:c0 + 3]
        groups.append(cols)
    K = torch.from_numpy(sc.K).float()[None]
    cases = [("rad2e-4", 2e-4, None), ("rad2e-3", 2e-3, None)]
    if a.radii:
        nz = np.clip(np.abs(sc.sf_norms[:, 2].astype(np.float64)), 0.26, 1.0)
        radii = (sc.sf_points[:, 2].astype(np.float64) / (np.sqrt(2.0) * sc.K[0, 0] * nz)).astype(np.float32)
        cases.append(("radii", DEFAULT_RAD, torch.from_numpy(radii).cuda()))
    ctx = RenderContext(sc.H, sc.W, sc.N)
    g = torch.randn((sc.H, sc.W, nch), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    for key, rad, radii in cases:
        p = render_params(K, sc.H, sc.W, 1.0, rad)
        res[f"channels{nch}_fwd_{key}"] = _time(lambda: render_channels(ctx, p, pts, feat, radii=radii), a.reps)
        res[f"three_channel_x{len(groups)}_fwd_{key}"] = _time(
            lambda: [render_points(ctx, p, pts, cols, radii=radii) for cols in groups], a.reps)
        res[f"three_channel_x1_fwd_{key}"] = _time(lambda: render_points(ctx, p, pts, groups[0], radii=radii), a.reps)
        _, _, cnt = render_channels(ctx, p, pts, feat, with_info=True, radii=radii)
        res[f"channels{nch}_fwd_{key}"]["pixels_hit"] = float((cnt > 0).float().mean())
        res[f"channels{nch}_fwd_{key}"]["hits_per_pixel_mean"] = float(cnt.float().mean())
        res[f"channels{nch}_bwd_points_features_{key}"] = _time(lambda: render_backward_channels(ctx, p, g), a.reps)
        if radii is not None:
            res[f"channels{nch}_bwd_points_features_radii_{key}"] = _time(
                lambda: render_backward_channels(ctx, p, g, radii=True), a.reps)
    res["render_points"] = sc.N
    res["channels"] = nch
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--radii", action="store_true", help="time the per-point render (see the module's docstring)")
    ap.add_argument("--channels", type=int, default=0, help="time the N-channel render with this many channels (1..8)")
    ap.add_argument("--in-run", action="store_true", help="time the GraphFit render-loss frame stepwise and inside the run")
    ap.add_argument("--frames", type=int, default=8, help="--in-run: frames per slm_gf_run of the batched form")
    ap.add_argument("--no-in-run-forms", action="store_true", help="--in-run: only the plain and the stepwise frame")
    a = ap.parse_args()
    if a.in_run or a.channels or a.radii:
        res = in_run_mode(a) if a.in_run else (channels_mode(a) if a.channels else radii_mode(a))
        print(json.dumps(res, indent=1))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    from types import SimpleNamespace

    from helpers import torch_frame
    from oracle import graphfit_oracle as gfo
    from super_amd import synth
    from super_amd.deform_mesh import GraphFit
    from super_amd.renderer import Pulsar, render_backward, render_backward_ex, render_params, ssim_render_loss_device

    res = {}
    sc = synth.make_scene(N=300_000, J=512, H=480, W=640, seed=5, src_border=2)
    pts = torch.from_numpy(sc.sf_points).cuda()
    cols = torch.from_numpy(np.random.default_rng(2).uniform(size=(sc.N, 3)).astype(np.float32)).cuda()
    inputs = {"K": torch.from_numpy(sc.K).float()[None].cuda(), ("color", 0): torch.zeros(1, 3, sc.H, sc.W, device="cuda")}
    r = Pulsar(SimpleNamespace(height=sc.H, width=sc.W))
    data = SimpleNamespace(points=pts, colors=cols)
    for name, rad in (("render_rad2e-4", 2e-4), ("render_rad2e-3", 2e-3)):
        res[name] = _time(lambda: r(inputs, data, rad=rad), a.reps)
        _, _, cnt = r.render(inputs, data, rad=rad, with_info=True)
        res[name]["pixels_hit"] = float((cnt > 0).float().mean())
        res[name]["hits_per_pixel_max"] = int(cnt.max())
    res["render_points"] = sc.N
    # the render loss: the colour frame is the render itself plus noise (an SSIM loss with kept pixels)
    gen = torch.Generator("cuda").manual_seed(3)
    for name, rad in (("rad2e-4", 2e-4), ("rad2e-3", 2e-3)):
        tgt = (r(inputs, data, rad=rad).permute(2, 0, 1) + 0.01 * torch.randn(3, sc.H, sc.W, device="cuda",
                                                                              generator=gen)).contiguous()
        ctx = r.context()
        p = render_params(inputs["K"], sc.H, sc.W, 1.0, rad)

        def loss_bwd():
            img = loss_bwd.img
            _, g = ssim_render_loss_device(img, tgt, 1e-4)
            return render_backward(ctx, p, g)

        def fwd_loss_bwd():
            loss_bwd.img = r(inputs, data, rad=rad)
            return loss_bwd()

        fwd_loss_bwd()
        res["render_fwd_ssim_bwd_" + name] = _time(fwd_loss_bwd, a.reps)
        fwd_loss_bwd()
        res["render_ssim_bwd_" + name] = _time(loss_bwd, a.reps)
        def loss_bwd_colors():
            _, g = ssim_render_loss_device(loss_bwd.img, tgt, 1e-4)
            return render_backward_ex(ctx, p, g)

        fwd_loss_bwd()
        res["render_ssim_bwd_colors_" + name] = _time(loss_bwd_colors, a.reps)
        img = loss_bwd.img
        res["render_ssim_" + name] = _time(lambda: ssim_render_loss_device(img, tgt, 1e-4), a.reps)
        # through torch: Pulsar(opt, differentiable=True), the SSIM image gradient as the image's grad
        rd = Pulsar(SimpleNamespace(height=sc.H, width=sc.W), differentiable=True)
        pts_g, cols_g = pts.clone().requires_grad_(True), cols.clone().requires_grad_(True)
        _, g_img = ssim_render_loss_device(img, tgt, 1e-4)
        g_img32 = g_img.float()

        def autograd_fwd_bwd():
            out = rd(inputs, SimpleNamespace(points=pts_g, colors=cols_g), rad=rad)
            out.backward(g_img32)

        res["render_autograd_fwd_bwd_colors_" + name] = _time(autograd_fwd_bwd, a.reps)
        out, _ = ssim_render_loss_device(img, tgt, 1e-4, with_grad=False)
        res["render_ssim_" + name]["kept"] = int(out[1])
    # algorithmic bytes: positions (f64) + colours read, one 8-byte key per tile entry written and read, image written
    res["algorithmic_bytes_rad2e-4"] = sc.N * (24 + 12) + sc.H * sc.W * 12

    gsc = synth.make_scene(seed=0, **synth.WORKLOADS["C2"])
    sf, ginputs, new_data = torch_frame(gsc)
    sf.colors = torch.rand(gsc.N, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    sf.rgb = torch.zeros(1, 3, gsc.H, gsc.W, device="cuda")
    zero = torch.zeros(1, 2, gsc.H, gsc.W, device="cuda")
    models = SimpleNamespace(optical_flow=lambda x, y: zero)
    for name, flag in (("graphfit_corr", False), ("graphfit_corr_match_renderimg", True)):
        opt = gfo.default_opt(sf_corr=True, sf_corr_weight=0.05, sf_corr_match_renderimg=flag, renderer="pulsar",
                              renderer_rad=2e-4)
        opt.deform_udpate_method = "super_edg"
        gf = GraphFit(opt)
        res[name] = _time(lambda: gf(ginputs, sf, new_data, models), max(5, a.reps // 3))
    ginputs = dict(ginputs)
    for name, rad in (("graphfit_render_loss_rad2e-4", 2e-4), ("graphfit_render_loss_rad2e-3", 2e-3)):
        opt = gfo.default_opt(renderer="pulsar", renderer_rad=rad, render_loss=True, render_loss_weight=1e-4)
        opt.deform_udpate_method = "super_edg"
        gf = GraphFit(opt, native_render_loss=True)
        gf._bind(0, ginputs, sf, new_data, models)      # the colour frame: the render at identity, brightened
        ginputs[("color", 0)] = (gf.render_deformed(ginputs, sf.colors.float().contiguous()) + 0.01).contiguous()
        res[name] = _time(lambda: gf(ginputs, sf, new_data, models), max(5, a.reps // 3))
    res["graphfit_surfels"] = gsc.N
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
