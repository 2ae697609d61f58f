"""The facts about the fixtures of tests/rigid_terms_cases.py that the GPU tests of the rigid stage's opt-in terms
(tests/test_gpu_rigid_terms.py) rely on, pinned on the CPU with the project's own models.  No GPU, no library."""
import numpy as np
import pytest

import lm_corr_model as lcm
import lm_weight_model as lwm
import rigid_model as rm
import rigid_terms_cases as rc
from oracle import lm_oracle as orc


def margins(trace, minimal_loss=1e10):
    """per iteration |loss - best| / best, best = the smallest accepted loss before it"""
    out, best = [], minimal_loss
    for t in trace:
        out.append(abs(t["loss"] - best) / best)
        if t["accepted"] and t["loss"] < best:
            best = t["loss"]
    return out


def test_the_pan_along_the_surface_is_fixed_by_point_point_rows_only():
    """the issue's table: RMS distance (mm) of the moved model from its true place after ten iterations"""
    got = {"before": rc.rms_mm("issue", rm.IDENTITY)}
    for label, c in (("plain", rc.Case("issue", True, 0)), ("pp_w1", rc.Case("issue", True, 1, "none", 1.0, "exact")),
                     ("pp_w3", rc.Case("issue", True, 1, "none", 3.0, "exact")),
                     ("pp_w10", rc.Case("issue", True, 1, "none", 10.0, "exact")),
                     ("plane_w1", rc.Case("issue", True, 2, "none", 1.0, "exact"))):
        got[label] = rc.rms_mm("issue", rc.loop(c, 10)[0])
    print(got)
    for k, want in rc.KNOWN_WARP.items():
        assert abs(got[k] - want) <= 0.006 * max(1.0, want), (k, got[k], want)       # the table's rounding
    assert got["plain"] > got["before"]                 # the loss falls, the model slides
    assert got["pp_w3"] < 1.0
    # the plain case is the oracle's own loop: the weight model without weights and without targets adds nothing
    want, _ = rm.run(rc.frame("issue"), rc.opt(10))
    assert np.abs(rc.loop(rc.Case("issue", True, 0), 10)[0] - want).max() < 1e-12


@pytest.mark.parametrize("c", rc.LOOP_CASES + [rc.TRAIN_CASE] + rc.EDGE_LOOP_CASES, ids=lambda c: c.id)
def test_loop_cases_meet_the_conditions_at_every_point_and_decide_clearly(c):
    phase = "train" if c is rc.TRAIN_CASE else "test"
    for n_iter in ((4,) if phase == "train" else (4, 10)):
        beta, trace, visited = rc.loop(c, n_iter, phase)
        assert len(trace) == n_iter and len(visited) == 2 * n_iter
        for ww in visited:
            lwm.check_conditions(ww, *c.seg)
        if phase == "test":
            m = margins(trace)
            print(c.id, n_iter, "".join(str(int(t["accepted"])) for t in trace), "smallest margin %.2e" % min(m))
            assert min(m) > 1e-9, m
    assert trace[0]["M_grad"] > 0
    if c in rc.LOOP_CASES:
        assert int(c.corr[0][2].sum()) > 0


def test_no_valid_correspondence_is_the_plain_model():
    a, b = rc.loop(rc.NONE_CASE, 4), rc.loop(rc.PLAIN_CASE, 4)
    assert a[0].tobytes() == b[0].tobytes() and [t["loss"] for t in a[1]] == [t["loss"] for t in b[1]]


def test_the_default_damping_brings_rejects_and_the_weights_bite():
    rejected = [c for c in rc.LOOP_CASES if not all(t["accepted"] for t in rc.loop(c, 10)[1])]
    assert rejected and all(c.weights == "trunc" for c in rejected)
    for c in rc.LOOP_CASES:
        w = rc.loop(c, 4)[2][0].w
        if c.weights in ("hard", "trunc"):
            assert 0 < int((w == 0).sum()) < len(w), c.id                # some rows switched off, not all
        elif c.weights == "soft":
            assert ((w > 0) & (w < 1)).all() and w.std() > 0.0, c.id


@pytest.mark.parametrize("name,f64", [("n3000", True), ("n3000", False), ("n65", True), ("n257", True), ("big", True)])
@pytest.mark.parametrize("weights", ["hard", "trunc"])
def test_assembly_points_meet_the_conditions(name, f64, weights):
    fr, s = rc.frame(name, f64), rc.sem(name)
    for beta in (rm.IDENTITY, rm.displaced_beta()):
        lwm.check_conditions(lwm.weights(fr, s, beta[None, :], *rc.WEIGHTS[weights]), *rc.WEIGHTS[weights])


def test_holes_scene_has_surfels_with_one_term_only():
    fr = rc.frame("holes")
    o, n, valid = rc.targets("holes")
    matched = np.zeros(len(valid), bool)
    matched[orc.data_term(fr, rm.IDENTITY[None, :], 1.0).match] = True
    print("valid but unmatched", int((valid & ~matched).sum()), "matched but invalid", int((matched & ~valid).sum()))
    assert (valid & ~matched).sum() >= 1 and (matched & ~valid).sum() >= 1


def test_flow_ties_are_a_handful():
    sc = rc.issue_scene()
    fr = rm.frame_of_scene(sc)
    fl = rc.synth.smooth_flow(60, 80, 11, amp=(2.0, 1.5))
    tie = lcm.tie_distance(fr, fl) <= 1e-4
    assert int(tie.sum()) == 1 and int(lcm.targets_from_flow(fr, fl)[2].sum()) == 1117
    for name, f64 in (("n3000", True), ("n3000", False), ("issue", True), ("holes", True)):
        tie = lcm.tie_distance(rc.frame(name, f64), rc.flow(name)) <= 1e-4
        print(name, f64, "ties", int(tie.sum()), "valid", int(rc.targets(name, f64)[2].sum()))
        assert tie.sum() <= 5 and rc.targets(name, f64)[2].sum() > 0.5 * len(tie)


def test_every_matched_surfel_can_be_switched_off_beside_valid_correspondences():
    """the hard weight with every surfel labelled a class its target never wins: w = 0 everywhere, the match set stays"""
    fr, s = rc.frame("n257"), rc.sem("n257")
    ww = lwm.weights(fr, s, rm.IDENTITY[None, :], 1, 0.0)
    lwm.check_conditions(ww, 1, 0.0)
    w2 = lwm.weights(fr, rc.sem("n257", "off"), rm.IDENTITY[None, :], 1, 0.0)
    assert len(w2.w) == len(ww.w) > 0 and (w2.w == 0).all()
    c = rc.Case("n257", True, 1, "hard", 1.0, labels="off", **rc.SLOW)
    beta, trace, visited = rc.loop(c, 4)
    assert all(t["M_grad"] > 0 and t["M_loss"] > 0 for t in trace) and all((v.w == 0).all() for v in visited)
    assert min(margins(trace)) > 1e-9
