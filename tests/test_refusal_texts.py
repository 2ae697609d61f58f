"""The refusal texts of the C ABI, byte for byte: every stage host reports through one error channel
(csrc/slm_host.h), and slm_last_error() is part of the ABI.  Each call below is refused on its arguments,
before any device call, so this runs without a GPU."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from super_amd import build, _lib
    build.build()
    return _lib.load()


def _cases():
    from super_amd._lib import SlmConfig, SlmGfConfig
    INVALID, UNSUPPORTED = 1, 5
    out = C.c_void_p()
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    bad_gf = SlmGfConfig(max_frames=0)
    bad_lm = SlmConfig(num_iterations=10, max_frames=1, v=7.5, solver_path=5)
    return [
        ("slm_fuse_create", (4, 64, 1000, C.byref(out)), INVALID, b"slm_fuse_create: bad argument"),
        ("slm_fuse_bind_semantic", (None, None), INVALID, b"slm_fuse_bind_semantic: null handle"),
        ("slm_depth_create", (4, 64, C.byref(out)), INVALID, b"slm_depth_create: bad argument"),
        ("slm_gf_create", (C.byref(bad_gf), C.byref(out)), INVALID, b"slm_gf_create: bad argument"),
        ("slm_gf_bind_frame", (None, 0, None, None), INVALID, b"slm_gf_bind_frame: null argument"),
        ("slm_gf_set_shard", (None, 0, 1), INVALID, b"slm_gf_set_shard: bad rank/world"),
        ("slm_gf_bind_semantic", (None, 0, None, None, None), INVALID, b"slm_gf_bind_semantic: null argument"),
        ("slm_gf_bind_flow", (None, 0, None, None), INVALID, b"slm_gf_bind_flow: null argument"),
        ("slm_gf_bind_point_grad", (None, 0, None, None), INVALID, b"slm_gf_bind_point_grad: null argument"),
        ("slm_gf_get_edge_points", (None, 0, 0, None, 0, None), INVALID, b"slm_gf_get_edge_points: bad argument"),
        ("slm_gf_eval_morph", (None, 1, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_gf_eval_losses", (None, 1, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_gf_step", (None, 1, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_gf_run", (None, 1, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_gf_get_partial", (None, 0, None, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_gf_set_partial", (None, 0, None, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_gf_get_deform", (None, 0, None, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_gf_loss_grad", (None, 0, None, None, None, None), INVALID, b"slm_gf: slot range out of bounds"),
        ("slm_apply_update_gf", (0, 1, 9, None, None, None, None, one, one, one, None), UNSUPPORTED,
         b"slm_apply_update_gf: num_neighbors must be in 1..8"),
        ("slm_apply_update_gf_f64", (0, 0, 4, None, None, None, None, one, one, one, None), INVALID,
         b"slm_apply_update_gf: bad argument"),
        ("slm_render_create", (0, 64, 10, C.byref(out)), INVALID, b"slm_render_create: bad argument"),
        ("slm_render_points", (None, None, 0, None, None, 3, None, None, None, None), INVALID,
         b"slm_render_points: null argument"),
        ("slm_render_backward", (None, None, None, None, None), INVALID, b"slm_render_backward: null argument"),
        ("slm_render_ssim_loss", (16, 16, None, None, 1.0, None, None, None), INVALID,
         b"slm_render_ssim_loss: null argument"),
        ("slm_render_ssim_loss", (5, 16, one, one, 1.0, one, None, None), INVALID,
         b"slm_render_ssim_loss: h and w must be >= 6"),
        ("slm_graph_init", (1, 64, 4, None, None, None, None, None, None, None), INVALID, b"slm_graph_init: bad argument"),
        ("slm_graph_init_semantic", (48, 64, 4, None, None, None, None, 5, None, 0, None, None, None, None, None), INVALID,
         b"slm_graph_init_semantic: bad argument (1..4 classes, seg_conf and both node outputs)"),
        ("slm_knn", (0, 4, 9, 1, None, one, one, one, None), INVALID, b"slm_knn: bad argument (K + skip_self <= 9)"),
        ("slm_knn", (0, 2, 4, 0, None, one, one, one, None), INVALID, b"slm_knn: fewer nodes than K (+ self)"),
        ("slm_create", (C.byref(bad_lm), C.byref(out)), INVALID, b"slm_create: solver_path must be 0..4"),
        ("slm_debug_counters", (None,), INVALID, b"slm_debug_counters: null output"),
        # the LM host, unit by unit: bind ...
        ("slm_bind_frame", (None, 0, None, None), INVALID, b"slm_bind_frame: null argument"),
        ("slm_bind_frames", (None, 0, 1, None, None), INVALID, b"slm_bind_frames: null argument"),
        ("slm_prepare_model", (None, 0, None, None), INVALID, b"slm_prepare_model: null argument"),
        ("slm_discard_prepared", (None, 0), INVALID, b"slm_discard_prepared: null argument"),
        # ... the LM step ...
        ("slm_run", (None, 1, None), INVALID, b"null solver"),
        ("slm_set_shard", (None, 0, 1), INVALID, b"slm_set_shard: bad rank/world"),
        ("slm_lm_exchange_size", (None, 0, 0, None), INVALID, b"slm_lm_exchange_size: null output"),
        ("slm_lm_exchange_ptr", (None, 0, 0, None, None), INVALID, b"slm_lm_exchange_ptr: null output"),
        ("slm_lm_grad_local", (None, 1, None), INVALID, b"null solver"),
        ("slm_assemble", (None, 0, None, None, None), INVALID, b"null solver"),
        ("slm_loss", (None, 0, None, None), INVALID, b"null solver"),
        ("slm_solve", (None, 0, 1.0, None, None, None), INVALID, b"null solver"),
        # ... the solver's getters, setters and diagnostics, and the stateless wrappers
        ("slm_profile_enable", (None, 1), INVALID, b"slm_profile_enable: null solver"),
        ("slm_profile_read", (None, None, None), INVALID, b"slm_profile_read: null argument"),
        ("slm_get_beta", (None, 0, None, None), INVALID, b"null solver"),
        ("slm_get_records", (None, 0, None, 0, None), INVALID, b"null solver"),
        ("slm_debug_read", (None, 0, 0, None, 0, None, None), INVALID, b"slm_debug_read: bad argument"),
        ("slm_debug_read_plan", (None, 0, 0, None, 0, None, None), INVALID, b"slm_debug_read_plan: bad argument"),
        ("slm_debug_dag_trace", (None, 0, 1, None), INVALID, b"slm_debug_dag_trace: bad argument"),
        ("slm_debug_dag_abort", (None, 1, None), INVALID, b"null solver"),
        ("slm_debug_dag_timeout", (-1,), INVALID, b"slm_debug_dag_timeout: negative"),
        ("slm_solve_dense", (0, None, None, None, None, None), INVALID, b"slm_solve_dense: bad argument"),
        ("slm_data_residuals", (None, 0, None, None, None, None), INVALID, b"null solver"),
        ("slm_apply_update", (0, 0, 4, None, None, None, None, one, one, one, None), INVALID,
         b"slm_apply_update: bad argument"),
        ("slm_knn_weights", (0, 10, 0, one, one, one, one, None, None), INVALID, b"slm_knn_weights: bad argument"),
        ("slm_knn_f64", (0, 2, 4, 0, None, one, None, None, one, one, None), INVALID,
         b"slm_knn_f64: fewer nodes than K (+ self)"),
        ("slm_knn_weights_f64", (0, 10, 0, one, one, one, 0, None, None, one, None, None), INVALID,
         b"slm_knn_weights_f64: bad argument"),
    ]


def test_refusal_texts_are_exact(lib):
    for name, args, code, text in _cases():
        rc = getattr(lib, name)(*args)
        got = lib.slm_last_error()
        print(name, rc, got)
        assert rc == code, (name, rc, got)
        assert got == text, (name, got)


def test_a_refusal_replaces_the_previous_text(lib):
    # one channel for every translation unit: the text is that of the LAST refusal, whichever file it came from
    assert lib.slm_fuse_bind_semantic(None, None) != 0
    assert lib.slm_debug_counters(None) != 0
    assert lib.slm_last_error() == b"slm_debug_counters: null output"
    assert lib.slm_gf_set_shard(None, 0, 1) != 0
    assert lib.slm_last_error() == b"slm_gf_set_shard: bad rank/world"
