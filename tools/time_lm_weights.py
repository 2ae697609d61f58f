"""Timing: what the per-residual weights of the LM path's point-to-plane term cost (``slm_enable_data_weights``,
include/super_lm.h), at C2 (200 k surfels, 2 000 nodes, num_neighbors 4) by default, one and eight frames per launch.
Five solvers, interleaved in one process:

    tuple     the default: the tuple-sorted form of the data term (what bench.py times)
    pairs     the unweighted pair-record form at num_neighbors 4 (slm_enable_corr, nothing bound): the baseline of the three below
    trunc     the weights enabled with the truncation only (seg_mode 0, pp_max 2e-5)
    hard      the hard semantic weight (seg_mode 1)
    soft      the soft semantic weight (seg_mode 2)

    python tools/time_lm_weights.py [--workload C2] [--frames 1 8] [--reps 10] [--only hard soft] [--classes 4] [--out FILE]

Every timed call is one ``slm_run`` of 10 LM iterations from the identity (the slots' beta is reset outside the timed
region), HIP events around it after a warm-up run; reported as ms per LM iteration (median and maximum over --reps) and
the share of matched surfels whose weight is 0 at the identity.  The frames of a launch are the same scene in every slot.
Kernel times: run it under ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_lm_weights.py --only pairs trunc hard soft
--frames 8 --reps 3`` (k_data_grad_pairs<4> against k_data_grad_pairs<4, DataWArgs>, k_data_loss likewise), in a run of its
own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-super_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {"tuple": None, "pairs": "corr", "trunc": (0, 2e-5), "hard": (1, 0.0), "soft": (2, 0.0)}
ITERS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=["C1", "C2", "C4", "tiny"])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--only", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lm_weights.py needs a HIP device (no CPU fallback)")
    from super_amd import _lib, synth
    from super_amd.engine import DeviceFrame, Engine
    dims = dict(N=3000, J=48, H=60, W=80, src_border=5, tgt_border=3) if a.workload == "tiny" else dict(synth.WORKLOADS[a.workload])
    dev = torch.device("cuda", 0)
    sc = synth.make_scene(seed=0, semantic=True, num_classes=a.classes, **dims)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
    seg, seg_conf, tgt_conf = t(sc.sf_seg, torch.int32), t(sc.sf_seg_conf, torch.float32), t(sc.tgt_seg_conf, torch.float32)
    ident = torch.zeros((sc.J, 7), dtype=torch.float64, device=dev)
    ident[:, 0] = 1.0
    out = {"workload": a.workload, "N": sc.N, "J": sc.J, "K": int(sc.sf_knn_idx.shape[1]), "classes": a.classes, "iterations": ITERS,
           "results": {}}
    for n in a.frames:
        engines = {}
        for name in a.only:
            cfg = CONFIGS[name]
            e = Engine(dev, max_frames=n, num_iterations=ITERS)
            if cfg == "corr":
                _lib.check(e.lib.slm_enable_corr(e.h, 1, 0.5), "slm_enable_corr")
            elif cfg is not None:
                _lib.check(e.lib.slm_enable_data_weights(e.h, cfg[0], cfg[1]), "slm_enable_data_weights")
            frames = [DeviceFrame.from_scene(sc, dev) for _ in range(n)]
            e.bind_batch(frames) if n > 1 else e.bind(0, frames[0])
            zero_share = 0.0
            if isinstance(cfg, tuple):
                if cfg[0]:
                    for i in range(n):
                        _lib.check(e.lib.slm_bind_data_semantic(e.h, i, a.classes, seg.data_ptr(), seg_conf.data_ptr(), tgt_conf.data_ptr(),
                                                                e.stream), "slm_bind_data_semantic")
                w = torch.zeros(sc.N, dtype=torch.float64, device=dev)
                m = torch.zeros(sc.N, dtype=torch.uint8, device=dev)
                _lib.check(e.lib.slm_data_weights(e.h, 0, w.data_ptr(), e.stream), "slm_data_weights")
                _lib.check(e.lib.slm_data_residuals(e.h, 0, None, m.data_ptr(), None, e.stream), "slm_data_residuals")
                zero_share = float(((w == 0) & (m != 0)).sum().item()) / max(int(m.sum().item()), 1)
            engines[name] = (e, zero_share)

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
        for name, (e, zero_share) in engines.items():
            recs = e.records(0)
            out["results"][f"{name}_b{n}"] = {
                "ms_per_iteration": float(np.median(ts[name])), "max_ms_per_iteration": float(np.max(ts[name])),
                "ms_per_iteration_per_frame": float(np.median(ts[name])) / n, "reps": a.reps, "frames_per_launch": n,
                "zero_weight_share": zero_share, "accepted": sum(r["accepted"] for r in recs), "final_loss": recs[-1]["loss"]}
            e.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
