"""Timing: the global rigid pre-alignment stage of the LM path (``slm_rigid_run``, include/super_lm.h) at C2 (200 k
surfels, 480 x 640) by default, one and eight frames per run, the model rigidly displaced against its target (0.01 rad,
2 / -1 / 3 mm).  Four measurements, interleaved in one process:

    rigid     one ``slm_rigid_run`` of 10 iterations (22 launches + the set-up launch), per stage
    floor     the same with a model of 256 surfels: what the 22 launches and the one-wave steps cost with no surfel work --
              ``rigid`` minus ``floor`` is the eleven passes' own time
    lm        one ``slm_run`` of 10 iterations of the node solve on the same scene (2 000 nodes), per LM iteration: the stage
              it precedes, from the same session
    onenode   the same one-node, K = 1 problem through the node solver itself where it accepts it (data_path 1: per-entry
              atomics, solver_path 1: band; every surfel's 7 x 7 block lands on the same 49 addresses), one frame, or the
              refusal text

    python tools/time_rigid.py [--workload C2] [--frames 1 8] [--reps 10] [--only rigid lm] [--out FILE]
                               [--corr MODE] [--weights {hard,soft,trunc}]

``--corr 1|2`` / ``--weights`` put the stage's opt-in terms (``slm_rigid_set_terms``) on ``rigid`` and ``floor``: point-point /
point-plane correspondence rows with targets built from a smooth synthetic flow by ``slm_rigid_corr_targets`` (weight 1),
and the hard / soft semantic weight (a scene with semantic fields) or the 2e-5 truncation on the data rows.

HIP events around every timed call after a warm-up call, median and maximum over --reps.  The frames of a run are the same
scene in every slot.  Kernel times: run it under ``rocprofv3 --kernel-trace --stats -- python tools/time_rigid.py --only
rigid --frames 8 --reps 3`` (k_rg_pass, k_rg_step), in a run of its own."""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-super_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = ["rigid", "floor", "lm", "onenode"]
ITERS = 10


def displaced(points, angle=0.01, axis=(0.3, -0.5, 0.8), trans=(0.002, -0.001, 0.003)):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    w, v = np.cos(angle / 2), np.sin(angle / 2) * a
    c = np.cross(v, points)
    return points + 2.0 * w * c + 2.0 * np.cross(v, c) + np.asarray(trans, np.float64)


def timed(call, reps):
    ts = []
    for rep in range(reps + 1):                               # (rep 0 warms up)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        if rep:
            ts.append(t0.elapsed_time(t1))
    return float(np.median(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=["C1", "C2", "C4", "tiny"])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", nargs="+", default=CONFIGS, choices=CONFIGS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--corr", type=int, default=0, choices=[0, 1, 2], metavar="MODE")
    ap.add_argument("--weights", default=None, choices=["hard", "soft", "trunc"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rigid.py needs a HIP device (no CPU fallback)")
    from super_amd import _lib, synth
    from super_amd.engine import DeviceFrame, Engine
    dims = dict(N=3000, J=48, H=60, W=80, src_border=5, tgt_border=3) if a.workload == "tiny" else dict(synth.WORKLOADS[a.workload])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    semantic = a.weights in ("hard", "soft")
    sc = synth.make_scene(seed=0, **dims, **(dict(semantic=True, num_classes=3) if semantic else {}))
    sc = dataclasses.replace(sc, sf_points=displaced(sc.sf_points.astype(np.float64)).astype(np.float32))
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    cfg = _lib.SlmRigidConfig(num_iterations=ITERS, phase_test=1, w_data=1.0, w_rot=1.0, u0=10.0, v=7.5, minimal_loss0=1e10)
    out = {"workload": a.workload, "N": sc.N, "J": sc.J, "H": sc.H, "W": sc.W, "iterations": ITERS, "corr": a.corr,
           "weights": a.weights, "results": {}}
    seg_mode = {"hard": 1, "soft": 2}.get(a.weights, 0)
    pp_max = 2e-5 if a.weights == "trunc" else 0.0
    keep = []                                                  # the term inputs, read in place by the runs

    def set_terms(h, cs):
        """the stage's opt-in terms of every slot: targets from a smooth flow, the scene's semantic fields"""
        if not (a.corr or seg_mode or pp_max):
            return
        _lib.check(lib.slm_rigid_set_terms(h, a.corr, 1.0, seg_mode, pp_max), "slm_rigid_set_terms")
        t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)
        for slot, c in enumerate(cs):
            if a.corr:
                flow = t(synth.smooth_flow(sc.H, sc.W, 11, amp=(2.0, 1.5)), torch.float32)
                pts = torch.zeros((sc.N, 3), dtype=torch.float64, device=dev)
                nrm, valid = torch.zeros_like(pts), torch.zeros(sc.N, dtype=torch.uint8, device=dev)
                full = _lib.SlmFrame()
                C.memmove(C.byref(full), C.byref(c), C.sizeof(full))
                full.N = sc.N                                  # (floor: the arrays cover the whole model)
                _lib.check(lib.slm_rigid_corr_targets(C.byref(full), flow.data_ptr(), pts.data_ptr(), nrm.data_ptr(),
                                                      valid.data_ptr(), stream()), "slm_rigid_corr_targets")
                _lib.check(lib.slm_rigid_set_corr(h, slot, pts.data_ptr(), nrm.data_ptr(), valid.data_ptr()), "slm_rigid_set_corr")
                keep.append((flow, pts, nrm, valid))
            if seg_mode:
                seg, scf, tcf = t(sc.sf_seg, torch.int32), t(sc.sf_seg_conf, torch.float32), t(sc.tgt_seg_conf, torch.float32)
                _lib.check(lib.slm_rigid_set_semantic(h, slot, int(scf.shape[1]), seg.data_ptr(), scf.data_ptr(), tcf.data_ptr()),
                           "slm_rigid_set_semantic")
                keep.append((seg, scf, tcf))
        torch.cuda.synchronize()

    def rigid_records(h, slot):
        arr, got = (_lib.SlmIterRecord * ITERS)(), C.c_int32(0)
        _lib.check(lib.slm_rigid_get_records(h, slot, arr, ITERS, C.byref(got), stream()), "slm_rigid_get_records")
        return [dict(loss=r.loss, accepted=bool(r.accepted), status=int(r.status), M=int(r.M_grad)) for r in arr[:got.value]]

    for n in a.frames:
        frames = [DeviceFrame.from_scene(sc, dev) for _ in range(n)]
        for name in [c for c in ("rigid", "floor") if c in a.only]:
            cs = [f.c_struct() for f in frames]
            if name == "floor":
                for c in cs:
                    c.N = min(c.N, 256)
            arr = (_lib.SlmFrame * n)(*cs)
            h = C.c_void_p()
            _lib.check(lib.slm_rigid_create(n, C.byref(h)), "slm_rigid_create")
            set_terms(h, cs)
            med, mx = timed(lambda: _lib.check(lib.slm_rigid_run(h, C.byref(cfg), n, arr, stream()), "slm_rigid_run"), a.reps)
            recs = rigid_records(h, 0)
            out["results"][f"{name}_b{n}"] = {
                "ms_per_stage": med, "max_ms_per_stage": mx, "ms_per_stage_per_frame": med / n, "reps": a.reps,
                "frames_per_run": n, "surfels": int(cs[0].N), "launches": 2 * (ITERS + 1) + (n + 7) // 8,
                "accepted": sum(r["accepted"] for r in recs), "matched": recs[0]["M"],
                "first_loss": recs[0]["loss"], "final_loss": min(r["loss"] for r in recs if r["accepted"])}
            if a.corr or seg_mode or pp_max:
                t4 = torch.empty(4, dtype=torch.float64, device=dev)
                _lib.check(lib.slm_rigid_get_terms(h, 0, t4.data_ptr(), stream()), "slm_rigid_get_terms")
                out["results"][f"{name}_b{n}"]["terms"] = t4.cpu().tolist()
            lib.slm_rigid_destroy(h)
        if "lm" in a.only:
            e = Engine(dev, max_frames=n, num_iterations=ITERS)
            e.bind_batch(frames) if n > 1 else e.bind(0, frames[0])
            ident = torch.zeros((sc.J, 7), dtype=torch.float64, device=dev)
            ident[:, 0] = 1.0
            ts = []
            for rep in range(a.reps + 1):
                for i in range(n):                             # (outside the timed region)
                    _lib.check(lib.slm_set_beta(e.h, i, ident.data_ptr(), e.stream), "slm_set_beta")
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                e.run(n)
                t1.record()
                t1.synchronize()
                if rep:
                    ts.append(t0.elapsed_time(t1) / ITERS)
            recs = e.records(0)
            out["results"][f"lm_b{n}"] = {"ms_per_iteration": float(np.median(ts)), "max_ms_per_iteration": float(np.max(ts)),
                                          "ms_per_iteration_per_frame": float(np.median(ts)) / n, "reps": a.reps,
                                          "frames_per_launch": n, "accepted": sum(r["accepted"] for r in recs),
                                          "final_loss": recs[-1]["loss"]}
            e.close()
    if "onenode" in a.only:
        # one node at the origin, K = 1, every surfel attached to it: the node solver's per-entry-atomics path + band solver
        f = DeviceFrame.from_scene(sc, dev)
        f.sf_knn_idx = torch.zeros((sc.N, 1), dtype=torch.int32, device=dev)
        f.sf_knn_w = torch.ones((sc.N, 1), dtype=torch.float32, device=dev)
        f.ed_points = torch.zeros((1, 3), dtype=torch.float32, device=dev)
        f.ed_norms = torch.zeros((1, 3), dtype=torch.float32, device=dev)
        f.ed_knn_idx = torch.zeros((1, 1), dtype=torch.int32, device=dev)
        try:
            e = Engine(dev, max_frames=1, num_iterations=ITERS, use_arap=False, use_rot=True, data_path=1, solver_path=1)
            e.bind(0, f)
            ident = torch.tensor([[1.0, 0, 0, 0, 0, 0, 0]], dtype=torch.float64, device=dev)

            def call():
                _lib.check(lib.slm_set_beta(e.h, 0, ident.data_ptr(), e.stream), "slm_set_beta")
                e.run(1)
            med, mx = timed(call, min(a.reps, 3))
            recs = e.records(0)
            out["results"]["onenode_b1"] = {"ms_per_stage": med, "max_ms_per_stage": mx, "reps": min(a.reps, 3),
                                            "accepted": sum(r["accepted"] for r in recs),
                                            "final_loss": min(r["loss"] for r in recs if r["accepted"])}
            e.close()
        except _lib.SuperLMError as err:
            out["results"]["onenode_b1"] = {"refused": str(err)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
