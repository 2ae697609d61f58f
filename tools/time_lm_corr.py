"""Timing: what the flow-correspondence term of the LM path costs (``slm_enable_corr``, include/super_lm.h), at C2
(200 k surfels, 2 000 nodes, num_neighbors 4) by default, one and eight frames per launch.  Four solvers, interleaved
in one process:

    tuple     the default: the tuple-sorted form of the data term (what bench.py times)
    pairs     the term enabled, no correspondences bound: prices the pair-record form at num_neighbors 4
    corr_pp   the term in mode 1 'point-point', targets from a smooth synthetic flow
    corr_pl   the term in mode 2 'point-plane'

    python tools/time_lm_corr.py [--workload C2] [--frames 1 8] [--reps 10] [--only corr_pp corr_pl] [--out FILE]

Every timed call is one ``slm_run`` of 10 LM iterations from the identity (the slots' beta is reset outside the timed
region), HIP events around it after a warm-up run; reported as ms per LM iteration (median and maximum over --reps) and
the share of surfels with a correspondence.  The frames of a launch are the same scene in every slot.  Kernel times: run it
under ``rocprofv3 --kernel-trace --stats -- python tools/time_lm_corr.py --only corr_pp corr_pl --frames 8 --reps 3``
(k_corr_grad_pairs, k_corr_loss), in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-super_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {"tuple": 0, "pairs": None, "corr_pp": 1, "corr_pl": 2}   # name -> mode (0: never enabled, None: enabled, nothing bound)
ITERS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=["C1", "C2", "C4", "tiny"])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--only", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lm_corr.py needs a HIP device (no CPU fallback)")
    from super_amd import _lib, synth
    from super_amd.engine import DeviceFrame, Engine
    dims = dict(N=3000, J=48, H=60, W=80, src_border=5, tgt_border=3) if a.workload == "tiny" else dict(synth.WORKLOADS[a.workload])
    dev = torch.device("cuda", 0)
    sc = synth.make_scene(seed=0, **dims)
    flow = torch.from_numpy(synth.smooth_flow(sc.H, sc.W, 7, amp=(2.5, 1.8))).to(dev).contiguous()
    ident = torch.zeros((sc.J, 7), dtype=torch.float64, device=dev)
    ident[:, 0] = 1.0
    out = {"workload": a.workload, "N": sc.N, "J": sc.J, "K": int(sc.sf_knn_idx.shape[1]), "iterations": ITERS, "weight": a.weight,
           "results": {}}
    for n in a.frames:
        engines = {}
        for name in a.only:
            mode = CONFIGS[name]
            e = Engine(dev, max_frames=n, num_iterations=ITERS)
            if mode != 0:
                _lib.check(e.lib.slm_enable_corr(e.h, mode or 1, a.weight), "slm_enable_corr")
            frames = [DeviceFrame.from_scene(sc, dev) for _ in range(n)]
            e.bind_batch(frames) if n > 1 else e.bind(0, frames[0])
            kept = 0
            if mode:
                res = torch.zeros(2, dtype=torch.float64, device=dev)
                for i in range(n):
                    _lib.check(e.lib.slm_bind_corr_flow(e.h, i, flow.data_ptr(), e.stream), "slm_bind_corr_flow")
                _lib.check(e.lib.slm_corr_loss(e.h, 0, res.data_ptr(), e.stream), "slm_corr_loss")
                kept = int(res[1].item())
            engines[name] = (e, kept)

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
        for name, (e, kept) in engines.items():
            recs = e.records(0)
            out["results"][f"{name}_b{n}"] = {
                "ms_per_iteration": float(np.median(ts[name])), "max_ms_per_iteration": float(np.max(ts[name])),
                "ms_per_iteration_per_frame": float(np.median(ts[name])) / n, "reps": a.reps, "frames_per_launch": n,
                "kept_share": kept / sc.N, "accepted": sum(r["accepted"] for r in recs), "final_loss": recs[-1]["loss"]}
            e.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
