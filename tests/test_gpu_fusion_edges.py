"""HIP surfel fusion at its edges, through super_amd.fusion: more than 16 surfels on a pixel, merge chains, every
num_neighbors, node counts around the 64-node runs of the candidate search, tie orders, a power-of-two image, degenerate
calls, the cached context reused across different calls, and device state carried from one fused frame into the next.
Scenes: fusion_edge_cases.py; references: the reference's own recording tests/golden/fu_edges.npz, and the NumPy oracle where
the reference pins nothing (test_fusion_edge_cases.py checks the oracle against the recording, and that no discrete decision
of a scene sits on a knife edge, which is why isStable / knn_indices / time_stamp / seg are compared bit for bit here).
Needs an MI355X (-m gpu)."""
from types import SimpleNamespace

import numpy as np
import pytest

import fusion_edge_cases as fec
from test_fusion_edge_cases import GOLD, run_oracle
from test_gpu_fusion import _check, _objects

pytestmark = pytest.mark.gpu


def _start(name, b=None):
    b0, okw, _ = fec.build(name)
    b = b0 if b is None else b
    sf, inputs, sfdata = _objects(b, okw, seg="sf_seg" in b)
    if "track_id" in b:
        import torch
        sf.track_pts, sf.evaluate_tracking = {}, False
        sf.track_id = torch.from_numpy(b["track_id"].copy()).cuda()
        inputs["filename"] = ["%06d" % int(b["time"])]
    return b, okw, sf, inputs, sfdata


def _fuse_and_swap(name, ref, prefix, sf, inputs, sfdata):
    """fuseInputData then prepareStableIndexNSwapAllModel, each compared with ``ref[prefix + "fuse_*" / "swap_*"]``."""
    from super_amd import fusion
    fusion.fuseInputData(sf, inputs, sfdata)
    _check(sf, ref, prefix + "fuse_")
    if hasattr(sf, "track_id"):
        np.testing.assert_array_equal(sf.track_id.cpu().numpy(), ref[prefix + "fuse_track_id"])
        sf.evaluate_tracking = True
    fusion.prepareStableIndexNSwapAllModel(sf, inputs, sfdata)
    _check(sf, ref, prefix + "swap_")
    if hasattr(sf, "track_id"):
        np.testing.assert_array_equal(sf.track_id.cpu().numpy(), ref[prefix + "swap_track_id"])
    assert sf.surfel_num == int(ref[prefix + "swap_isStable"].sum())


def _golden_run(name):
    b, _, sf, inputs, sfdata = _start(name)
    _fuse_and_swap(name, fec.expand_golden(np.load(GOLD), name, b), name + "_", sf, inputs, sfdata)
    return sf


def _oracle_ref(name, frames=1):
    steps, tids = run_oracle(name, frames=frames)
    ref = fec.Gold()
    for i, (s, t) in enumerate(zip(steps, tids)):
        prefix = f"f{i // 2}_" + ("fuse_", "swap_")[i % 2]
        ref.update({prefix + k: v for k, v in s.items()})
        if t is not None:
            ref[prefix + "track_id"] = t
    return ref


@pytest.mark.parametrize("name", fec.RECORDED)
def test_edge_scene_matches_the_reference_recording(name):
    _golden_run(name)


@pytest.mark.parametrize("name", list(fec.ORACLE_ONLY))
def test_tie_orders_match_the_oracle(name):
    """Equal confidences on a pixel and ED nodes at bit-identical positions in different node runs: lower index first."""
    _, _, sf, inputs, sfdata = _start(name)
    _fuse_and_swap(name, _oracle_ref(name), "f0_", sf, inputs, sfdata)


def _state(sf):
    names = fec.OUT_FIELDS + (fec.OUT_SEG_FIELDS if hasattr(sf, "seg") else ())
    return {k: getattr(sf, k).cpu().numpy().copy() for k in names}


def test_cached_context_is_reused_across_different_calls():
    """One process, one (H, W): semantic and plain calls, K = 3 / 8 / 1 / 4, J = 35 / 129 / 70 / 4, merges of existing surfels
    on and off alternate on the cached context; a model too large for it forces its re-creation in between.  Every run equals
    its recording, and the second ``sem_k3`` the first bit for bit."""
    import torch
    from super_amd import fusion
    first = _state(_golden_run("sem_k3"))
    _golden_run("k8_j129")
    # the same scene with 1500 more (unstable, hence inert) surfels: more rows than the context holds
    b, okw, _ = fec.build("k8_j129")
    big = dict(b)
    pad = np.arange(1500) % len(b["sf_points"])
    for k in fec.MODEL_FIELDS:
        big[k] = np.concatenate([b[k], b[k][pad]])
    big["sf_isStable"] = np.concatenate([b["sf_isStable"], np.zeros(1500, bool)])
    key = (int(b["H"]), int(b["W"]), str(torch.device("cuda", torch.cuda.current_device())))
    before = fusion._ctx[key]
    need = len(big["sf_points"]) + len(big["new_points"])
    _, _, sf, inputs, sfdata = _start("k8_j129", big)
    fusion.fuseInputData(sf, inputs, sfdata)
    after = fusion._ctx[key]
    assert after[1] >= need and (before[1] >= need or after[1] != before[1])
    g = fec.expand_golden(np.load(GOLD), "k8_j129", b)
    n0 = len(b["sf_points"])
    rows = torch.cat([torch.arange(n0), torch.arange(n0 + 1500, len(sf.points))]).cuda()   # the scene's own and the appended rows
    _check(SimpleNamespace(**{k: getattr(sf, k)[rows] for k in fec.OUT_FIELDS}), g, "k8_j129_fuse_")
    assert not bool(sf.isStable[n0:n0 + 1500].any())
    fusion.prepareStableIndexNSwapAllModel(sf, inputs, sfdata)
    _check(sf, g, "k8_j129_swap_")
    for name in ("k1", "hard_k4_j70", "k4_j4", "nomerge_exist"):
        _golden_run(name)
    again = _state(_golden_run("sem_k3"))
    for k, v in first.items():
        assert v.tobytes() == again[k].tobytes() and v.shape == again[k].shape, k


@pytest.mark.parametrize("name", list(fec.CARRIED))
def test_two_frames_carried_on_the_device_match_the_oracle(name):
    """Fuse + swap, then a second frame at time 42 fused into what the device itself produced (the oracle likewise carries its
    own state): compared after each of the four steps."""
    b, _, sf, inputs, sfdata = _start(name)
    ref = _oracle_ref(name, frames=2)
    _fuse_and_swap(name, ref, "f0_", sf, inputs, sfdata)
    _, inputs2, sfdata2 = _objects(dict(b, **fec.second_frame(b)), fec.build(name)[1], seg="sf_seg" in b)
    assert int(inputs2["time"]) == 42 and sfdata2.time == 42
    _fuse_and_swap(name, ref, "f1_", sf, inputs2, sfdata2)
    assert len(sf.points) > 200 and bool(sf.isStable.all())


def _assert_reference_layout(sf, K, C=None):
    """dtype and trailing shape of every field as the reference holds them (also with 0 rows)."""
    import torch
    n = int(sf.points.shape[0])
    want = {"points": (torch.float64, (3,)), "norms": (torch.float64, (3,)), "colors": (torch.float32, (3,)),
            "radii": (torch.float64, ()), "confs": (torch.float32, ()), "time_stamp": (torch.float32, ()),
            "isStable": (torch.bool, ()), "knn_indices": (torch.long, (K,)), "knn_w": (torch.float64, (K,)),
            "projdata": (torch.float32, (2,))}
    if C is not None:
        want.update(seg=(torch.long, ()), seg_conf=(torch.float64, (C,)), dist2edge=(torch.float64, ()))
    for k, (dt, tail) in want.items():
        t = getattr(sf, k)
        assert t.dtype == dt and tuple(t.shape) == (n,) + tail, (k, t.dtype, tuple(t.shape))


@pytest.mark.parametrize("name", fec.DEGENERATE)
def test_degenerate_calls_match_the_oracle(name):
    """An empty model, an empty frame, a model of which nothing projects into the image, a swap that keeps nothing (followed by
    the next frame fused into the n = 0 model): the oracle's rows, the reference's dtypes and shapes, no exception."""
    frames = 2 if name == "all_dropped" else 1
    b, okw, sf, inputs, sfdata = _start(name)
    ref = _oracle_ref(name, frames=frames)
    K = int(b["num_neighbors"])
    _fuse_and_swap(name, ref, "f0_", sf, inputs, sfdata)
    _assert_reference_layout(sf, K)
    if frames == 2:
        assert len(sf.points) == 0 and sf.surfel_num == 0
        _, inputs2, sfdata2 = _objects(dict(b, **fec.second_frame(b)), okw)
        _fuse_and_swap(name, ref, "f1_", sf, inputs2, sfdata2)
        _assert_reference_layout(sf, K)
        assert len(sf.points) == 0


@pytest.mark.parametrize("seg", [False, True])
def test_empty_model_and_empty_frame_together(seg):
    """n = 0 and T = 0 in one call (no row to give any buffer): the empty model comes back unchanged, fields in the reference's
    dtypes and shapes."""
    from super_amd import fusion
    b, okw, _ = fec.build("carry_sem_k7" if seg else "k5")
    for k in fec.MODEL_FIELDS + (fec.SEG_FIELDS if seg else ()):
        b[k] = b[k][:0]
    for k in [k for k in b if k.startswith("new_") and k not in ("new_valid", "new_index_map")]:
        b[k] = b[k][:0]
    b["new_valid"] = np.zeros_like(b["new_valid"])
    b["new_index_map"] = -np.ones_like(b["new_index_map"])
    sf, inputs, sfdata = _objects(b, okw, seg=seg)
    fusion.fuseInputData(sf, inputs, sfdata)
    _assert_reference_layout(sf, int(b["num_neighbors"]), fec.NUM_CLASSES if seg else None)
    fusion.prepareStableIndexNSwapAllModel(sf, inputs, sfdata)
    _assert_reference_layout(sf, int(b["num_neighbors"]), fec.NUM_CLASSES if seg else None)
    assert len(sf.points) == 0 and sf.surfel_num == 0 and sf.time == int(b["time"])
