"""What test_gpu_fusion_edges.py relies on, pinned on the CPU: the fusion oracle reproduces what the reference itself gave on
every edge scene of fusion_edge_cases.py (tests/golden/fu_edges.npz, test_fusion_oracle.check's tolerances), every scene
exercises what it claims (the 16-layer overflow, the boundary pixels, merge chains, merged / appended / rejected new points,
neighbours across node runs, tie orders, tracked ids), and no discrete decision of any scene sits on a knife edge: the
oracle's isStable / knn_indices / seg / row counts do not move when th_dist, th_cosine_ang or the node radii move by 1e-9.
A seed that fails the last gets replaced (fusion_edge_cases.SEEDS), never tolerated: it is what lets the device test demand
bit-exact discrete results."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import fusion_edge_cases as fec
from oracle import fusion_oracle as fuo
from test_fusion_oracle import check

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fu_edges.npz")
FULL = fec.RECORDED + tuple(fec.ORACLE_ONLY) + tuple(fec.CARRIED)          # scenes with pixels A-D and a full frame
DISCRETE = ("isStable", "knn_indices", "seg")


@functools.lru_cache(maxsize=None)
def scene(name):
    return fec.build(name)


def oracle_model(b, seg):
    kw = dict(seg=b["sf_seg"], seg_conf=b["sf_seg_conf"], dist2edge=b["sf_dist2edge"], ed_seg=b["ed_seg"],
              ed_seg_conf=b["ed_seg_conf"]) if seg else {}
    return fuo.Model(b["sf_points"], b["sf_norms"], b["sf_colors"], b["sf_radii"], b["sf_confs"], b["sf_time_stamp"],
                     b["sf_isStable"], b["sf_knn_idx"], b["sf_knn_w"], b["ed_points"], b["ed_radii"], **kw)


def oracle_frame(f, seg):
    new = SimpleNamespace(points=f["new_points"], norms=f["new_norms"], colors=f["new_colors"], radii=f["new_radii"],
                          confs=f["new_confs"], valid=f["new_valid"])
    if seg:
        new.seg, new.seg_conf, new.dist2edge = f["new_seg"], f["new_seg_conf"], f["new_dist2edge"]
    return new


def oracle_opt(b, okw, dist=1.0, cos=0.0, **more):
    opt = fuo.default_opt(height=int(b["H"]), width=int(b["W"]), num_neighbors=int(b["num_neighbors"]), **dict(okw, **more))
    opt.th_dist, opt.th_cosine_ang = opt.th_dist * dist, opt.th_cosine_ang + cos
    return opt


def snapshot(m):
    names = fec.OUT_FIELDS + (fec.OUT_SEG_FIELDS if m.seg is not None else ())
    return {k: np.array(getattr(m, k), copy=True) for k in names}


def run_oracle(name, dist=1.0, cos=0.0, radii=1.0, frames=1, track=None, **more):
    """Fuse + swap (``frames`` = 2: then the second frame at time 42 on the carried model) in the oracle.  Returns the list of
    snapshots after every step, and the track ids after every step (or None)."""
    b, okw, _ = scene(name)
    seg = "sf_seg" in b
    m = oracle_model(b, seg)
    m.ed_radii = m.ed_radii * radii
    opt = oracle_opt(b, okw, dist, cos, **more)
    tid = np.array(track, np.int64) if track is not None else b["track_id"].copy() if "track_id" in b else None
    steps, tids = [], []
    for f in [b, fec.second_frame(b)][:frames]:
        fuo.fuse_input_data(m, opt, b["K"], oracle_frame(f, seg), int(f["time"]), track_id=tid)
        steps.append(snapshot(m))
        tids.append(None if tid is None else tid.copy())
        fuo.swap_stable(m, opt, int(f["time"]), track_id=tid)
        steps.append(snapshot(m))
        tids.append(None if tid is None else tid.copy())
    return steps, tids


# ------------------------------------------------------------------------------------------- the oracle against the reference
@pytest.mark.parametrize("name", fec.RECORDED)
def test_oracle_reproduces_the_reference_on_the_edge_scenes(name):
    b, okw, _ = scene(name)
    g = fec.expand_golden(np.load(GOLD), name, b)
    seg = "sf_seg" in b
    m = oracle_model(b, seg)
    opt = oracle_opt(b, okw)
    tid = b["track_id"].copy() if name == "track" else None
    fuo.fuse_input_data(m, opt, b["K"], oracle_frame(b, seg), int(b["time"]), track_id=tid)
    check(m, g, f"{name}_fuse_")
    if tid is not None:
        np.testing.assert_array_equal(tid, g["track_fuse_track_id"])
    fuo.swap_stable(m, opt, int(b["time"]), track_id=tid)
    check(m, g, f"{name}_swap_")
    if tid is not None:
        np.testing.assert_array_equal(tid, g["track_swap_track_id"])


def test_golden_file_is_small_and_holds_every_recorded_case():
    assert os.path.getsize(GOLD) < 1 << 20
    g = np.load(GOLD)
    assert {k.split("_in_digest")[0] for k in g.files if k.endswith("_in_digest")} == set(fec.RECORDED)


# --------------------------------------------------------------------------------------- every scene exercises what it claims
def layer_overflow(b, rows):
    """Of the stable surfels ``rows`` (one pixel): those past the 16 maps, by descending confidence, lower index first."""
    rows = rows[b["sf_isStable"][rows]]
    order = rows[np.argsort(-b["sf_confs"][rows].astype(np.float64), kind="stable")]
    return order[fuo.MAP_NUM:]


@pytest.mark.parametrize("name", FULL)
def test_scene_overflows_the_layer_maps_and_chains_merges(name):
    b, okw, groups = scene(name)
    H, W = int(b["H"]), int(b["W"])
    _, _, coords, ok = fuo.project(b["sf_points"], b["K"], H, W)
    for p, (cnt, _, _) in fec.GROUP.items():                     # the groups are what the docstring says they are
        u, v = fec.PIX[p]
        on = np.nonzero(ok & b["sf_isStable"] & (coords == v * W + u))[0]
        np.testing.assert_array_equal(on, groups[p])
        assert len(on) == cnt and bool(b["sf_isStable"][on].all())
    (fused, _), _ = run_oracle(name)
    lost = {p: groups[p][b["sf_isStable"][groups[p]] & ~fused["isStable"][groups[p]]] for p in fec.GROUP}
    print(name, "lost per pixel", {p: len(v) for p, v in lost.items()})
    if okw.get("disable_merging_exist_surfels"):
        assert all(len(v) == 0 for v in lost.values())           # (a) overflow present, nothing dropped
        assert len(layer_overflow(b, groups["A"])) == 24
        return
    assert len(lost["A"]) >= 24 and set(layer_overflow(b, groups["A"])) <= set(lost["A"])      # (a)
    assert len(lost["C"]) == 0 and len(layer_overflow(b, groups["C"])) == 0                      # (b)
    np.testing.assert_array_equal(lost["D"], layer_overflow(b, groups["D"]))
    assert len(lost["D"]) == 1
    # (c) pixel B: some surfel absorbed two or more others (ids tracked on B's surfels move to their absorbers)
    _, (tid, _) = run_oracle(name, track=groups["B"])
    moved = (tid >= 0) & (tid != groups["B"])
    absorbers, times = np.unique(tid[moved], return_counts=True)
    print(name, "pixel B: absorbers", dict(zip(absorbers.tolist(), times.tolist())))
    assert times.max() >= 2 and np.isin(absorbers, groups["B"]).all()


@pytest.mark.parametrize("name", [n for n in FULL if n not in ("nomerge_new", "noadd")])
def test_scene_merges_appends_and_rejects_new_points(name):
    """(d).  Merged points are counted with the merges of existing surfels switched off: every merged point then changes the
    confidence of a surfel of its own."""
    b, okw, _ = scene(name)
    n0, T = len(b["sf_points"]), len(b["new_points"])
    (only_new, _), _ = run_oracle(name, disable_merging_exist_surfels=True, disable_adding_new_surfels=True)
    merged = int((only_new["confs"] != b["sf_confs"]).sum())
    (fused, _), _ = run_oracle(name)
    appended = len(fused["points"]) - n0
    rejected = T - merged - appended
    print(name, "new points", T, "merged", merged, "appended", appended, "rejected", rejected)
    assert merged >= 0.3 * T and appended >= 20 and rejected >= 10
    idx = fused["knn_indices"][n0:]
    if name in fec.MULTI_RUN:                                    # (e)
        runs = idx // 64
        assert len(np.unique(runs)) == (len(b["ed_points"]) + 63) // 64
        mixed = int((runs != runs[:, :1]).any(1).sum())             # (k5_j65: the tail run is node 64 alone)
        print(name, "appended rows with neighbours from two runs", mixed)
        assert mixed >= 1
    if name.startswith("knn_ties"):                              # (f)
        P, pairs = b["ed_points"], scene(name)[2]["knn_pairs"]
        np.testing.assert_array_equal(P[pairs[:, 0]], P[pairs[:, 1]])
        assert (pairs[:, 0] // 64 != pairs[:, 1] // 64).all() and len(pairs) == 18 and {128, 129} <= set(pairs[:, 1])
        low = np.array([sum(1 for lo, hi in pairs if lo in r and hi not in r) for r in idx])
        both = np.array([sum(1 for lo, hi in pairs if lo in r and hi in r) for r in idx])
        print(name, "appended rows with the lower node of a pair only", int((low > 0).sum()), "with a whole pair", int((both > 0).sum()))
        assert (low > 0).sum() >= 10 and (both > 0).sum() >= 10
        assert not any(hi in r and lo not in r for r in idx for lo, hi in pairs)     # never the higher one alone
        # the search meets the higher index first: rows with a pair of the shared column whose point is strictly nearer to the
        # bounding box of run 1 than to that of run 0 (k_fu_candidates scans the nearest run first)
        def box_d2(p, nodes):
            d = np.maximum(np.maximum(nodes.min(0) - p, p - nodes.max(0)), 0.0)
            return (d * d).sum(-1)
        pts = fused["points"][n0:]
        run1_first = box_d2(pts, P[64:128]) < box_d2(pts, P[:64])
        shared = np.array([any(lo in r for lo, hi in pairs[:16]) for r in idx])
        print(name, "rows with a shared-column pair scanned higher index first", int((run1_first & shared).sum()))
        assert (run1_first & shared).sum() >= 10


def test_tie_scene_has_the_ties():
    b, _, groups = scene("ties")
    assert len(np.unique(b["sf_confs"][groups["B"]])) == 1
    a = b["sf_confs"][groups["A"]]
    np.testing.assert_array_equal(a[0::2], a[1::2])
    assert len(np.unique(a)) == 20


def test_tracked_ids_end_as_the_reference_says():
    """(g) overflow -> -2, absorbed -> the absorber's id, the absorber / an unstable / a stale surfel keep theirs (and are kept
    alive by the swap), -1 stays."""
    b, _, groups = scene("track")
    tid0 = b["track_id"]
    (fused, swapped), (tid1, tid2) = run_oracle("track")
    over_a = layer_overflow(b, groups["A"])
    assert set(tid0[:2]) <= set(over_a) and (tid1[:2] == -2).all()
    tb0, tb1 = tid0[2:22], tid1[2:22]
    np.testing.assert_array_equal(tb0, groups["B"])
    over_b = np.isin(tb0, layer_overflow(b, groups["B"]))
    assert (tb1[over_b] == -2).all() and (tb1[~over_b] >= 0).all()
    moved = ~over_b & (tb1 != tb0)
    absorbers = np.unique(tb1[moved])
    assert moved.sum() >= 2 and len(absorbers) >= 1
    assert not fused["isStable"][tb0[moved]].any() and fused["isStable"][absorbers].all()
    assert all(tb1[tb0 == a][0] == a for a in absorbers)         # the absorber keeps its own id
    np.testing.assert_array_equal(tid1[22:24], np.concatenate([groups["track_unstable"], groups["track_stale"]]))
    assert not b["sf_isStable"][tid0[22]] and _age(b, tid0[23]) >= 30
    assert (tid1[24:] == -1).all() and (tid2[24:] == -1).all()
    # after the swap every live id points at the row its surfel moved to
    live = tid2 >= 0
    np.testing.assert_array_equal(live, tid1 >= 0)
    np.testing.assert_array_equal(swapped["points"][tid2[live]], fused["points"][tid1[live]])
    assert live[22] and live[23]                                 # kept although unstable / stale


def _age(b, row):
    return float(b["time"]) - float(b["sf_time_stamp"][row])


def test_degenerate_scenes_are_degenerate():
    b, _, _ = scene("empty_model")
    assert len(b["sf_points"]) == 0 and b["sf_knn_idx"].shape == (0, 4) and len(b["new_points"]) > 100
    b, _, _ = scene("empty_frame")
    assert len(b["new_points"]) == 0 and not b["new_valid"].any()
    b, _, _ = scene("none_project")
    assert not fuo.project(b["sf_points"], b["K"], int(b["H"]), int(b["W"]))[3].any()
    (fused, swapped), _ = run_oracle("none_project")
    assert len(fused["points"]) == len(b["sf_points"])           # nothing added ...
    np.testing.assert_array_equal(fused["confs"], b["sf_confs"])   # ... nothing merged
    np.testing.assert_array_equal(fused["isStable"], b["sf_isStable"])
    assert 0 < len(swapped["points"]) < len(fused["points"])
    steps, _ = run_oracle("all_dropped", frames=2)
    assert [len(s["points"]) for s in steps] == [len(scene("all_dropped")[0]["sf_points"]), 0, 0, 0]
    assert steps[3]["knn_indices"].shape == (0, 4) and steps[3]["projdata"].shape == (0, 2)


# --------------------------------------------------------------------------------------------- no decision on a knife edge
PERTURBATIONS = [dict(dist=1 + 1e-9), dict(dist=1 - 1e-9), dict(cos=1e-9), dict(cos=-1e-9), dict(radii=1 + 1e-9),
                 dict(radii=1 - 1e-9)]


@pytest.mark.parametrize("name", FULL + fec.DEGENERATE)
def test_no_decision_on_a_knife_edge(name):
    frames = 2 if name in fec.CARRIED or name == "all_dropped" else 1
    base, _ = run_oracle(name, frames=frames)
    for p in PERTURBATIONS:
        steps, _ = run_oracle(name, frames=frames, **p)
        for i, (s, s0) in enumerate(zip(steps, base)):
            assert len(s["points"]) == len(s0["points"]), (name, p, i)
            for k in DISCRETE:
                if k in s0:
                    np.testing.assert_array_equal(s[k], s0[k], err_msg=f"{name} {p} step {i} {k}")
