"""The refusal texts of the per-point-radius entry points of the renderer, byte for byte, after the pattern of
test_refusal_texts.py: each call is refused on its arguments, before any device call, so this runs without a GPU."""
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
    p = SlmRenderParams()
    return [
        ("slm_render_points_radii", (None, None, 0, None, None, None, 3, None, None, None, None), INVALID,
         b"slm_render_points_radii: null argument"),
        ("slm_render_points_radii", (one, C.byref(p), 1, one, one, one, 3, None, None, None, None), INVALID,
         b"slm_render_points_radii: null argument"),                                       # no image
        ("slm_render_points_radii", (one, C.byref(p), 1, one, None, one, 3, one, None, None, None), INVALID,
         b"slm_render_points_radii: null radii"),
        ("slm_gf_render_radii", (None, 0, None, None, None, None, 3, None, None, None, None), INVALID,
         b"slm_gf_render_radii: null argument"),
        ("slm_gf_render_radii", (one, 0, one, C.byref(p), None, one, 3, one, None, None, None), INVALID,
         b"slm_gf_render_radii: null radii"),
        ("slm_render_backward_radii", (None, None, None, None, None, None, None), INVALID,
         b"slm_render_backward_radii: null argument"),
        ("slm_render_backward_radii", (one, C.byref(p), None, one, one, one, None), INVALID,
         b"slm_render_backward_radii: null argument"),                                     # no grad_image
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
    for name in ("slm_render_points_radii", "slm_gf_render_radii", "slm_render_backward_radii"):
        assert name in _lib.EXPORTS
