"""The refusal texts of the N-channel entry points of the renderer, byte for byte, after the pattern of
test_refusal_texts_radii.py: each call is refused on its arguments, before any device call, so this runs without a GPU."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from super_amd import build, _lib
    build.build()
    return _lib.load()


def _cases():
    from super_amd._lib import SlmRenderParams
    INVALID = 1
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    p = C.byref(SlmRenderParams())
    bg = (C.c_float * 8)()
    fwd, bwd = "slm_render_points_channels", "slm_render_backward_channels"
    # (r, p, N, points, radii, C, features, feature_stride, bg, image, front_id, hit_count, stream)
    return [
        (fwd, (None, None, 0, None, None, 3, None, 3, None, None, None, None, None), INVALID, fwd.encode() + b": null argument"),
        (fwd, (one, p, 1, one, None, 3, one, 3, bg, None, None, None, None), INVALID, fwd.encode() + b": null argument"),  # image
        (fwd, (one, p, 1, one, None, 3, one, 3, None, one, None, None, None), INVALID, fwd.encode() + b": null argument"),  # bg
        (fwd, (one, p, 1, one, None, 0, one, 3, bg, one, None, None, None), INVALID, fwd.encode() + b": channels must be 1..8"),
        (fwd, (one, p, 1, one, None, 9, one, 9, bg, one, None, None, None), INVALID, fwd.encode() + b": channels must be 1..8"),
        (fwd, (one, p, 1, one, None, -1, one, 3, bg, one, None, None, None), INVALID, fwd.encode() + b": channels must be 1..8"),
        (fwd, (one, p, 1, one, None, 4, one, 3, bg, one, None, None, None), INVALID, fwd.encode() + b": feature_stride < channels"),
        (fwd, (one, p, 1, one, one, 8, None, 8, bg, one, None, None, None), INVALID, fwd.encode() + b": null features"),
        # (r, p, C, grad_image, grad_points, grad_features, grad_radii, stream)
        (bwd, (None, None, 3, None, None, None, None, None), INVALID, bwd.encode() + b": null argument"),
        (bwd, (one, p, 3, None, one, one, one, None), INVALID, bwd.encode() + b": null argument"),          # no grad_image
        (bwd, (one, p, 0, one, one, one, one, None), INVALID, bwd.encode() + b": channels must be 1..8"),
        (bwd, (one, p, 9, one, one, one, one, None), INVALID, bwd.encode() + b": channels must be 1..8"),
    ]


def test_refusal_texts_are_exact(lib):
    for name, args, code, text in _cases():
        rc = getattr(lib, name)(*args)
        got = lib.slm_last_error()
        print(name, rc, got)
        assert rc == code, (name, rc, got)
        assert got == text, (name, got)


def test_the_new_entries_are_exported():
    from super_amd import _lib
    for name in ("slm_render_points_channels", "slm_render_backward_channels"):
        assert name in _lib.EXPORTS
    assert _lib.SLM_RENDER_MAX_CHANNELS == 8
