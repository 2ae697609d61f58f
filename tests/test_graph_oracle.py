"""Pin the NumPy restatement of the reference's ED-graph construction against
golden vectors recorded from the reference itself.  CPU only."""
import os

import numpy as np
import pytest

from oracle import graph_oracle as gro

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gr_60x80.npz")
VARIANTS = {"step6": 6, "step9": 9, "step4": 4}
SEM_VARIANTS = {"sem6": dict(step=6, hard_seg=False), "hard6": dict(step=6, hard_seg=True),
                "hard4": dict(step=4, hard_seg=True)}


def check(out, g, tag):
    assert out["num"] == int(g[f"{tag}_num"])
    np.testing.assert_array_equal(out["edge_index"], g[f"{tag}_edge_index"])
    np.testing.assert_array_equal(out["triangles"], g[f"{tag}_triangles"])
    np.testing.assert_array_equal(out["points"], g[f"{tag}_points"])
    np.testing.assert_array_equal(out["norms"], g[f"{tag}_norms"])
    np.testing.assert_allclose(out["edges_lens"], g[f"{tag}_edges_lens"], rtol=1e-14)
    np.testing.assert_allclose(out["radii"], g[f"{tag}_radii"], rtol=1e-13)
    np.testing.assert_allclose(out["triangles_areas"], g[f"{tag}_triangles_areas"], rtol=1e-12)
    if f"{tag}_seg" in g.files:
        np.testing.assert_array_equal(out["seg"], g[f"{tag}_seg"])
        np.testing.assert_array_equal(out["seg_conf"], g[f"{tag}_seg_conf"])


@pytest.mark.parametrize("tag", list(SEM_VARIANTS))
def test_semantic_graph_matches_reference(tag):
    g = np.load(GOLD)
    kw = SEM_VARIANTS[tag]
    out = gro.direct_deform_graph(g["in_valid"], g["in_index_map"], g["in_points"], g["in_norms"], kw["step"],
                                  seg_conf=g["in_seg_conf"], prune_class_edges=kw["hard_seg"])
    check(out, g, tag)
    if kw["hard_seg"]:
        s = out["seg"]
        assert (s[out["edge_index"][0]] == s[out["edge_index"][1]]).all()
        assert out["edge_index"].shape[1] < g["sem6_edge_index"].shape[1] or kw["step"] != 6
        assert len(np.unique(s)) == 3


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_graph_matches_reference(tag):
    g = np.load(GOLD)
    out = gro.direct_deform_graph(g["in_valid"], g["in_index_map"], g["in_points"], g["in_norms"], VARIANTS[tag])
    check(out, g, tag)
    assert out["num"] > 20 and out["edge_index"].shape[1] > out["num"]


# ---- degenerate grids (built directly, no reference recording): the oracle is known to run on them here; test_gpu_graph.py
# compares the device with it.  name -> (H, W, step, which grid points are valid anchors, J, E, F, radii that stay NaN)
DEGENERATE_GRIDS = {
    "no_anchor": (9, 13, 4, "none", 0, 0, 0, 0),
    "one_anchor": (9, 13, 4, "one", 1, 0, 0, 1),
    "even_only": (17, 25, 4, "even", 6, 0, 0, 6),       # no two anchors are neighbours: k_gr_fix_nan divides 0 by 0
    "exact_multiple": (17, 25, 4, "all", 24, 68, 30, 0),   # W - 1 and H - 1 are multiples of the step: no anchor on the last column / row
    "step_exceeds_image": (9, 13, 20, "all", 1, 0, 0, 1),   # a 1 x 1 grid
    "step_1": (5, 6, 1, "all", 20, 55, 24, 0),
}


def degenerate_grid(name, seed=0):
    """(valid (H*W,), index_map (H,W), points, norms, seg_conf, H, W, step) of a degenerate grid: every pixel off the anchor grid
    is valid, the grid points are as the table says."""
    H, W, step, anchors = DEGENERATE_GRIDS[name][:4]
    rng = np.random.default_rng(seed)
    valid = np.ones((H, W), bool)
    gy, gx = np.meshgrid(np.arange(0, H, step), np.arange(0, W, step), indexing="ij")
    on = {"none": np.zeros(gy.shape, bool), "one": (gy == step) & (gx == 2 * step), "all": np.ones(gy.shape, bool),
          "even": ((gy // step) % 2 == 0) & ((gx // step) % 2 == 0)}[anchors]
    valid[gy, gx] = on
    T = int(valid.sum())
    index_map = -np.ones((H, W), np.int64)
    index_map[valid] = rng.permutation(T)               # rows in no particular order
    points = rng.uniform(-1, 1, (T, 3)) + np.array([0.0, 0.0, 3.0])
    norms = rng.normal(size=(T, 3))
    norms /= np.linalg.norm(norms, axis=1, keepdims=True)
    conf = rng.uniform(0.05, 1, (T, 3))
    return valid.reshape(-1), index_map, points, norms, conf / conf.sum(1, keepdims=True), H, W, step


@pytest.mark.parametrize("sem", ["plain", "sem", "hard"])
@pytest.mark.parametrize("name", list(DEGENERATE_GRIDS))
def test_oracle_runs_on_degenerate_grids(name, sem):
    valid, index_map, points, norms, conf, H, W, step = degenerate_grid(name)
    J, E, F, n_nan = DEGENERATE_GRIDS[name][4:]
    with np.errstate(invalid="ignore"), pytest.warns(RuntimeWarning) if n_nan else _no_warning():
        out = gro.direct_deform_graph(valid, index_map, points, norms, step, seg_conf=None if sem == "plain" else conf,
                                      prune_class_edges=sem == "hard")
    assert out["num"] == J == len(out["points"]) and out["points"].shape == (J, 3)
    assert out["edge_index"].shape[0] == 2 and out["edge_index"].dtype == np.int64
    assert out["triangles"].shape[0] == 3 and out["triangles"].dtype == np.int64
    if sem == "hard":
        s = out["seg"]
        assert out["edge_index"].shape[1] <= E and out["triangles"].shape[1] <= F
        assert (s[out["edge_index"][0]] == s[out["edge_index"][1]]).all()
        if E:
            assert 0 < out["edge_index"].shape[1] < E        # the pruning bites and leaves something
    else:
        assert out["edge_index"].shape[1] == E and out["triangles"].shape[1] == F
        assert int(np.isnan(out["radii"]).sum()) == n_nan
    if name == "exact_multiple":                             # no anchor at u = W - 1 or v = H - 1
        assert valid.reshape(H, W)[H - 1, ::step].all() and valid.reshape(H, W)[::step, W - 1].all()    # valid, yet no anchors
        np.testing.assert_array_equal(out["points"], points[index_map[0:H - 1:step, 0:W - 1:step].reshape(-1)])


def _no_warning():
    import contextlib
    return contextlib.nullcontext()
