"""Timing: what the semantic boundary-morph term of the LM path costs (``slm_enable_morph``, include/super_lm.h), at C2
(200 k surfels, 2 000 nodes, num_neighbors 4, three classes, the target segmentation moved 6 px) by default, one and eight
frames per launch.  Three solvers, interleaved in one process:

    tuple     the default: the tuple-sorted form of the data term (what bench.py times)
    pairs     the term enabled, no inputs bound: prices the pair-record form at num_neighbors 4 (plus the term's fold, the one
              launch per loss pass an enabled solver always runs)
    morph     the term enabled with the scene's semantic inputs in every slot

    python tools/time_lm_morph.py [--workload C2] [--frames 1 8] [--reps 10] [--only morph] [--out FILE]

The comparison that matters is ``morph`` against ``pairs`` (and ``pairs`` against the same figure of tools/time_lm_face.py, whose
enabled solver runs the pair-record form without this term's fold).  Every timed call is one ``slm_run`` of 10 LM iterations
from the identity (the slots' beta is reset outside the timed region), HIP events around it after a warm-up run; reported as ms
per LM iteration (median and maximum over --reps), the kept and candidate counts at identity and the boundary-list lengths.
The frames of a launch are the same scene in every slot.  The weight is computed so that the term's largest J^T J entry is
about the data term's: in pixel units the term swamps the data term at weight 1, and the iteration count of the
accept / reject loop would not be a frame's.  Kernel times: run it under
``rocprofv3 --kernel-trace --stats -- python tools/time_lm_morph.py --only morph --frames 8 --reps 3`` (k_morph_select,
k_morph_fold, k_morph_grad_pairs; k_data_grad_pairs beside them), in a run of its own."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-super_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = ["tuple", "pairs", "morph"]
ITERS = 10


def default_weight(sc, kept):
    """sqrt(largest diagonal entry of the data term's J^T J / largest of the term's at weight 1), both estimated: a node
    carries sum_i w_ik^2 over its surfels of the former's translation block; of the latter's, (fx / Z)^2 / n times that sum
    over its KEPT surfels -- up to about half of a node's surfels where the node sits on a class boundary"""
    fx = float(sc.K[0, 0])
    z = float(sc.sf_points.astype(np.float64)[:, 2].mean())
    return float(np.sqrt(max(kept, 1) / (0.5 * (fx / z) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=["C1", "C2", "C4", "tiny"])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--weight", type=float, default=None)
    ap.add_argument("--only", nargs="+", default=CONFIGS, choices=CONFIGS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lm_morph.py needs a HIP device (no CPU fallback)")
    from super_amd import _lib, synth
    from super_amd.engine import DeviceFrame, Engine
    dims = dict(N=3000, J=48, H=60, W=80, src_border=5, tgt_border=3) if a.workload == "tiny" else dict(synth.WORKLOADS[a.workload])
    dev = torch.device("cuda", 0)
    sc = synth.make_scene(seed=0, semantic=True, num_classes=3, **dims)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt).contiguous()
    img_seg, img_conf, sf_seg = t(sc.img_seg, torch.int32), t(sc.img_seg_conf, torch.float32), t(sc.sf_seg, torch.int32)
    ident = torch.zeros((sc.J, 7), dtype=torch.float64, device=dev)
    ident[:, 0] = 1.0

    def bind_inputs(e, slot):
        counts = (C.c_int32 * _lib.SLM_MAX_CLASSES)()
        _lib.check(e.lib.slm_bind_morph(e.h, slot, sc.num_classes, img_seg.data_ptr(), img_conf.data_ptr(), sf_seg.data_ptr(), counts,
                                        e.stream), "slm_bind_morph")
        return list(counts)[:sc.num_classes]

    def counts_at_identity(e):
        res = torch.zeros(3, dtype=torch.float64, device=dev)
        _lib.check(e.lib.slm_morph_loss(e.h, 0, res.data_ptr(), e.stream), "slm_morph_loss")
        return int(res[1].item()), int(res[2].item())

    # the kept count at identity does not depend on the weight: a probe solver counts, the weight follows
    probe = Engine(dev, max_frames=1, num_iterations=ITERS)
    _lib.check(probe.lib.slm_enable_morph(probe.h, 1.0), "slm_enable_morph")
    probe.bind(0, DeviceFrame.from_scene(sc, dev))
    edges = bind_inputs(probe, 0)
    kept, cand = counts_at_identity(probe)
    probe.close()
    weight = a.weight if a.weight is not None else default_weight(sc, kept)
    out = {"workload": a.workload, "N": sc.N, "J": sc.J, "K": int(sc.sf_knn_idx.shape[1]), "classes": int(sc.num_classes),
           "boundary_lists": edges, "kept": kept, "candidates": cand, "iterations": ITERS, "weight": weight, "results": {}}
    for n in a.frames:
        engines = {}
        for name in a.only:
            e = Engine(dev, max_frames=n, num_iterations=ITERS)
            if name != "tuple":
                _lib.check(e.lib.slm_enable_morph(e.h, weight), "slm_enable_morph")
            frames = [DeviceFrame.from_scene(sc, dev) for _ in range(n)]
            e.bind_batch(frames) if n > 1 else e.bind(0, frames[0])
            if name == "morph":
                for i in range(n):
                    bind_inputs(e, i)
            engines[name] = (e, e.plan_info(0)["pairs"])

        def reset(e):
            for i in range(n):
                _lib.check(e.lib.slm_set_beta(e.h, i, ident.data_ptr(), e.stream), "slm_set_beta")

        ts = {name: [] for name in engines}
        for rep in range(a.reps + 1):                     # (rep 0 warms up)
            for name, (e, _) in engines.items():
                reset(e)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                e.run(n)
                t1.record()
                t1.synchronize()
                if rep:
                    ts[name].append(t0.elapsed_time(t1) / ITERS)
        for name, (e, pairs) in engines.items():
            recs = e.records(0)
            end = counts_at_identity(e) if name == "morph" else (0, 0)      # (at the run's final beta)
            out["results"][f"{name}_b{n}"] = {
                "ms_per_iteration": float(np.median(ts[name])), "max_ms_per_iteration": float(np.max(ts[name])),
                "ms_per_iteration_per_frame": float(np.median(ts[name])) / n, "reps": a.reps, "frames_per_launch": n,
                "kept_at_end": end[0], "candidates_at_end": end[1], "coupled_pairs": int(pairs),
                "accepted": sum(r["accepted"] for r in recs), "final_loss": recs[-1]["loss"]}
            e.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
