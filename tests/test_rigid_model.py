"""The one-node construction of tests/rigid_model.py does what the rigid stage's definition claims of it (CPU; this guards
the fixture, not the feature): on a rigidly displaced model the oracle loop brings the loss below a tenth of its value at
identity within four iterations, every surfel matches, and with the Rot term on |q| stays at 1."""
import numpy as np

import rigid_model as rm
from oracle import lm_oracle as orc
from super_amd import synth


def _scene():
    sc = synth.make_scene(N=3000, J=64, H=96, W=128, seed=3)
    return sc, rm.frame_of_scene(sc, rm.displace(sc.sf_points.astype(np.float64)))


def test_the_one_node_loop_removes_a_rigid_displacement():
    sc, fr1 = _scene()
    opt = rm.rigid_opt(num_optimize_iterations=4)
    loss0, M0 = orc.total_loss(fr1, rm.IDENTITY[None, :], opt)
    beta, trace = rm.run(fr1, opt)
    assert M0 == sc.N
    assert len(trace) == 4 and all(t["M_grad"] == sc.N and t["M_loss"] == sc.N for t in trace)
    best = min(t["loss"] for t in trace if t["accepted"])
    assert best < 0.1 * loss0, (loss0, [t["loss"] for t in trace])
    assert abs(np.linalg.norm(beta[:4]) - 1.0) < 1e-4


def test_the_rot_term_is_what_holds_the_quaternion_norm():
    _, fr1 = _scene()
    beta, _ = rm.run(fr1, rm.rigid_opt(num_optimize_iterations=10))
    assert abs(np.linalg.norm(beta[:4]) - 1.0) < 1e-4


def test_moved_is_a_rigid_motion_and_keeps_zero_normals():
    rng = np.random.default_rng(0)
    p, n = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[7] = 0.0
    Tg = rm.normalised(rm.displaced_beta())
    q, nq = rm.moved(p, n, Tg)
    d0 = np.linalg.norm(p[:, None] - p[None], axis=-1)
    d1 = np.linalg.norm(q[:, None] - q[None], axis=-1)
    np.testing.assert_allclose(d1, d0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(np.delete(nq, 7, 0), axis=1), 1.0, rtol=0, atol=1e-12)
    assert (nq[7] == 0.0).all()
    # a rotation by 0.004 rad turns no direction by more than that
    assert ((np.delete(nq, 7, 0) * np.delete(n, 7, 0)).sum(1) >= np.cos(0.004) - 1e-12).all()
