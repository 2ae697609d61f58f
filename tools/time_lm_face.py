"""Timing: what the triangle-area face term of the LM path costs (``slm_enable_face``, include/super_lm.h), at C2
(200 k surfels, 2 000 nodes, num_neighbors 4, ~3 800 grid triangles) by default, one and eight frames per launch.  Three
solvers, interleaved in one process:

    tuple     the default: the tuple-sorted form of the data term (what bench.py times)
    pairs     the term enabled, no mesh set: prices the pair-record form at num_neighbors 4
    face      the term enabled with the scene's own mesh in every slot

    python tools/time_lm_face.py [--workload C2] [--frames 1 8] [--reps 10] [--only face] [--out FILE]

The comparison that matters is ``face`` against ``pairs``.  Every timed call is one ``slm_run`` of 10 LM iterations from
the identity (the slots' beta is reset outside the timed region), HIP events around it after a warm-up run; reported as ms
per LM iteration (median and maximum over --reps), the triangle count and the coupled pairs of the slot's plan.  The frames
of a launch are the same scene in every slot.  The weight is computed so that the term's largest J^T J entry is about the
data term's (edge length 0.2 m, ~100 surfels per node): at weight 1 it would be lost, and the iteration count of the
accept / reject loop would not be the term's.  Kernel times: run it under
``rocprofv3 --kernel-trace --stats -- python tools/time_lm_face.py --only face --frames 8 --reps 3`` (k_face_grad,
k_face_loss; k_reg_grad_nd beside them), in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-super_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = ["tuple", "pairs", "face"]
ITERS = 10


def default_weight(sc):
    """sqrt(largest diagonal entry of the data term's J^T J / largest of the face term's at weight 1), both estimated: a node
    carries sum_i w_ik^2 <= its surfel count of the former's translation block and ~6 triangles x (edge / 2)^2 of the latter's"""
    per_node = np.bincount(sc.sf_knn_idx.reshape(-1), weights=(sc.sf_knn_w.astype(np.float64) ** 2).reshape(-1), minlength=sc.J)
    e = sc.ed_points.astype(np.float64)
    edge = np.linalg.norm(e[sc.ed_triangles[1]] - e[sc.ed_triangles[0]], axis=1).mean()
    return float(np.sqrt(per_node.max() / (6.0 * (0.5 * edge) ** 2)))


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
        raise SystemExit("time_lm_face.py needs a HIP device (no CPU fallback)")
    from super_amd import _lib, synth
    from super_amd.engine import DeviceFrame, Engine
    dims = dict(N=3000, J=48, H=60, W=80, src_border=5, tgt_border=3) if a.workload == "tiny" else dict(synth.WORKLOADS[a.workload])
    dev = torch.device("cuda", 0)
    sc = synth.make_scene(seed=0, **dims)
    weight = a.weight if a.weight is not None else default_weight(sc)
    tri = torch.from_numpy(np.ascontiguousarray(sc.ed_triangles)).to(device=dev, dtype=torch.int32).contiguous()
    areas = torch.from_numpy(np.ascontiguousarray(sc.ed_triangle_areas)).to(device=dev, dtype=torch.float64).contiguous()
    ident = torch.zeros((sc.J, 7), dtype=torch.float64, device=dev)
    ident[:, 0] = 1.0
    out = {"workload": a.workload, "N": sc.N, "J": sc.J, "K": int(sc.sf_knn_idx.shape[1]), "triangles": int(tri.shape[1]),
           "iterations": ITERS, "weight": weight, "results": {}}
    for n in a.frames:
        engines = {}
        for name in a.only:
            e = Engine(dev, max_frames=n, num_iterations=ITERS)
            if name != "tuple":
                _lib.check(e.lib.slm_enable_face(e.h, weight), "slm_enable_face")
            if name == "face":
                for i in range(n):
                    _lib.check(e.lib.slm_set_face_mesh(e.h, i, int(tri.shape[1]), tri.data_ptr(), areas.data_ptr(), e.stream),
                               "slm_set_face_mesh")
            frames = [DeviceFrame.from_scene(sc, dev) for _ in range(n)]
            e.bind_batch(frames) if n > 1 else e.bind(0, frames[0])
            n_tri = 0
            if name == "face":
                res = torch.zeros(2, dtype=torch.float64, device=dev)
                _lib.check(e.lib.slm_face_loss(e.h, 0, res.data_ptr(), e.stream), "slm_face_loss")
                n_tri = int(res[1].item())
            engines[name] = (e, n_tri, e.plan_info(0)["pairs"])

        def reset(e):
            for i in range(n):
                _lib.check(e.lib.slm_set_beta(e.h, i, ident.data_ptr(), e.stream), "slm_set_beta")

        ts = {name: [] for name in engines}
        for rep in range(a.reps + 1):                     # (rep 0 warms up)
            for name, (e, _, _) in engines.items():
                reset(e)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                e.run(n)
                t1.record()
                t1.synchronize()
                if rep:
                    ts[name].append(t0.elapsed_time(t1) / ITERS)
        for name, (e, n_tri, pairs) in engines.items():
            recs = e.records(0)
            out["results"][f"{name}_b{n}"] = {
                "ms_per_iteration": float(np.median(ts[name])), "max_ms_per_iteration": float(np.max(ts[name])),
                "ms_per_iteration_per_frame": float(np.median(ts[name])) / n, "reps": a.reps, "frames_per_launch": n,
                "triangles": n_tri, "coupled_pairs": int(pairs), "accepted": sum(r["accepted"] for r in recs),
                "final_loss": recs[-1]["loss"]}
            e.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
