"""Golden vectors of the depth-preprocessing edge cases (tests/depth_edge_cases.py): the REFERENCE's ``depth_preprocessing``
(``utils/data_loader.py:333-523``, unmodified, through ``ref_shim``, driven by ``make_golden_depth.run_reference``) on every
case the reference can run.

    python tests/golden/make_golden_depth_edges.py        ->  tests/golden/dp_edges.npz

Recorded per case: a digest of the inputs (``depth_edge_cases.build`` regenerates them) and the outputs in the layout of
``depth_edge_cases.Packer`` / ``expand_golden``.  Nothing is lost: this script checks that the expansion gives the reference's
arrays back bit for bit, dtypes included, before it writes them.  A case the reference raises on must be listed in
``depth_edge_cases.ORACLE_ONLY``; its exception is printed.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "python-super_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import depth_edge_cases as dec  # noqa: E402
import ref_shim  # noqa: E402
from make_golden_depth import run_reference  # noqa: E402
from make_golden_fusion_edges import save_npz  # noqa: E402


def reference_outputs(ref, name):
    base, okw = dec.build(name)
    if "valid_mask" in base:
        # the reference reads the mask with cv2.imread(path, 0) (data_loader.py:377-383); the shim's cv2 is an empty stub
        sys.modules["cv2"].imread = lambda path, flag: base["valid_mask"].astype(np.uint8) * 255
    with np.errstate(all="ignore"):
        return base, run_reference(ref, base, okw)


def main():
    torch.set_num_threads(1)
    ref = ref_shim.install_data_loader()
    packer = dec.Packer()
    outs, raised = {}, {}
    for name in dec.CASES:
        try:
            base, out = reference_outputs(ref, name)
        except Exception as e:                                      # noqa: BLE001 -- whatever the reference raises
            raised[name] = f"{type(e).__name__}: {e}"
            print(f"{name}: reference raises {raised[name]}")
            continue
        H, W = dec.CASES[name]["size"]
        T = int(out["valid"].sum())
        # what expand_golden derives from the inputs really is what the reference returned
        for k, v in dec.derived(base, name, out["valid"].reshape(H, W)).items():
            assert v.dtype == out[k].dtype and v.tobytes() == np.ascontiguousarray(out[k]).tobytes(), (name, k)
        for k, (dt, tail) in dec.REF_LAYOUT.items():
            if k in out:
                assert out[k].dtype == dt and out[k].shape[0] == T and (tail is None or out[k].shape[1:] == tail), (name, k)
        packer.add(name, base, out)
        outs[name] = (base, out)
        print(f"{name}: valid {T} of {H * W}, inval {int(out['inval'].sum())}")
    assert raised == dec.ORACLE_ONLY, (raised, dec.ORACLE_ONLY)
    g = packer.arrays()
    gold = type("G", (dict,), {"files": property(lambda s: list(s))})(g)
    for name, (base, out) in outs.items():
        back = dec.expand_golden(gold, name, base)
        for k, v in out.items():
            assert back[k].dtype == v.dtype and back[k].shape == v.shape, (name, k, back[k].dtype, v.dtype, back[k].shape, v.shape)
            assert back[k].tobytes() == np.ascontiguousarray(v).tobytes(), (name, k)
    path = os.path.join(HERE, "dp_edges.npz")
    save_npz(path, g)
    print(path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
