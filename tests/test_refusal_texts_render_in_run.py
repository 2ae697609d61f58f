"""The refusal texts of slm_gf_bind_render_loss, slm_gf_render_loss_status and slm_gf_render_loss_read, byte for byte, after the
pattern of test_refusal_texts_radii.py, and the exports, signatures and ABI version of the new entry points.  What is refused
on the arguments alone, and the export checks, run without a GPU; the refusals that need a solver (slm_gf_create needs a
device) are marked gpu."""
import ctypes as C
import os
import re

import pytest

INVALID, UNBOUND, UNSUPPORTED = 1, 4, 5
NEW = ("slm_gf_bind_render_loss", "slm_gf_render_loss_status", "slm_gf_render_loss_read")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "super_lm.h")


@pytest.fixture(scope="module")
def lib():
    from super_amd import build, _lib
    build.build()
    return _lib.load()


def _refused(lib, name, args, code, text):
    rc = getattr(lib, name)(*args)
    got = lib.slm_last_error()
    print(name, rc, got)
    assert rc == code, (name, rc, got)
    assert got == text, (name, got)


def test_null_solver_is_refused(lib):
    from super_amd._lib import SlmRenderParams
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    p = SlmRenderParams()
    out = (C.c_double * 4)()
    _refused(lib, "slm_gf_bind_render_loss", (None, 0, one, C.byref(p), None, one, 3, one, 1.0, 0, None), INVALID,
             b"slm_gf_bind_render_loss: null argument")
    _refused(lib, "slm_gf_render_loss_status", (None, 0, out, None), INVALID, b"slm_gf_render_loss_status: null argument")
    _refused(lib, "slm_gf_render_loss_read", (None, 0, None, None, None), INVALID, b"slm_gf_render_loss_read: null argument")


def _declaration(name):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_exports_signatures_and_abi_version(lib):
    from super_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(raw, name)                                   # the built library exports it
    assert _declaration("slm_gf_bind_render_loss") == [
        "slm_gf* g", "int32_t slot", "slm_render* r", "const slm_render_params* p", "const float* radii", "const float* colors",
        "int32_t color_stride", "const float* target_chw", "double weight", "int64_t entry_limit", "void* stream"]
    assert _declaration("slm_gf_render_loss_status") == ["slm_gf* g", "int32_t slot", "double out_host[4]", "void* stream"]
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.slm_gf_bind_render_loss.argtypes == [vp, i32, vp, C.POINTER(_lib.SlmRenderParams), vp, vp, i32, vp, C.c_double,
                                                    C.c_int64, vp]
    assert lib.slm_gf_render_loss_status.argtypes == [vp, i32, C.POINTER(C.c_double), vp]
    assert lib.slm_gf_render_loss_read.argtypes == [vp, i32, vp, vp, vp]
    for name in NEW:
        assert getattr(lib, name).restype == C.c_int
    assert re.search(r"#define\s+SLM_ABI_VERSION\s+3\b", open(HEADER).read())
    assert _lib.SLM_ABI_VERSION == 3 and lib.slm_abi_version() == 3


@pytest.mark.gpu
def test_refusal_texts_with_a_solver(lib):
    import torch
    import gf_render_run_cases as cases
    from super_amd.LM import _dev_ptr
    from super_amd.deform_mesh import GraphFit
    from super_amd.renderer import RenderContext, render_params
    sf, inputs, new_data = cases.gpu_frame()
    gf = GraphFit(cases.opt(render_loss=False), max_frames=2)
    sc = cases.scene()[0]
    N = sc.N
    ctx, small = RenderContext(sc.H, sc.W, N), RenderContext(sc.H, sc.W, 0)      # small holds 1024 points
    colors = sf.colors.float().contiguous()
    tgt = inputs[("color", 0)][0].float().contiguous()
    grad = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    out = (C.c_double * 4)()

    def params(**kw):
        p = render_params(inputs["K"], sc.H, sc.W, 1.0, cases.RAD)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def bind(slot=0, r=ctx, p=None, col=_dev_ptr(colors), stride=3, target=_dev_ptr(tgt), weight=0.01, limit=0, g=gf):
        p = params() if p is None else p
        return ("slm_gf_bind_render_loss",
                (g.h, slot, r.h if r is not None else None, C.byref(p) if p is not False else None, None, col, stride, target,
                 weight, limit, None))

    pre = b"slm_gf_bind_render_loss: "
    _refused(lib, *bind(slot=2), INVALID, pre + b"bad slot")
    _refused(lib, *bind(slot=-1), INVALID, pre + b"bad slot")
    _refused(lib, *bind(p=False), INVALID, pre + b"null argument")
    _refused(lib, *bind(target=None), INVALID, pre + b"null argument")
    _refused(lib, *bind(), UNBOUND, pre + b"slm_gf_bind_frame first")
    _refused(lib, "slm_gf_render_loss_status", (gf.h, 2, out, None), INVALID, b"slm_gf_render_loss_status: bad slot")
    _refused(lib, "slm_gf_render_loss_status", (gf.h, 0, out, None), UNBOUND,
             b"slm_gf_render_loss_status: slm_gf_bind_render_loss first")
    _refused(lib, "slm_gf_render_loss_read", (gf.h, 2, None, None, None), INVALID, b"slm_gf_render_loss_read: bad slot")
    _refused(lib, "slm_gf_render_loss_read", (gf.h, 0, None, None, None), UNBOUND,
             b"slm_gf_render_loss_read: slm_gf_bind_render_loss first")
    gf._bind(0, inputs, sf, new_data)
    gf._bind(1, inputs, sf, new_data)
    _refused(lib, *bind(weight=float("nan")), INVALID, pre + b"weight must be finite")
    _refused(lib, *bind(limit=-1), INVALID, pre + b"entry_limit must be 0 (from a sizing render) or 1..2^31")
    _refused(lib, *bind(limit=(1 << 31) + 1), INVALID, pre + b"entry_limit must be 0 (from a sizing render) or 1..2^31")
    _refused(lib, *bind(p=params(width=sc.W + 1)), INVALID, pre + b"image size outside the context's H x W")
    _refused(lib, *bind(p=params(n_track=0)), INVALID, pre + b"n_track must be 1..64")
    _refused(lib, *bind(p=params(focal=0.0)), INVALID, pre + b"bad camera or blend parameters")
    _refused(lib, *bind(r=small), INVALID, pre + b"more points than the context holds")
    _refused(lib, *bind(col=None), INVALID, pre + b"null points / colours or color_stride < 3")
    _refused(lib, *bind(stride=2), INVALID, pre + b"null points / colours or color_stride < 3")
    _refused(lib, *bind(p=params(height=5)), INVALID, pre + b"height and width must be >= 6 (the SSIM window)")
    # a point gradient and the term exclude each other, in both orders
    assert lib.slm_gf_bind_point_grad(gf.h, 0, _dev_ptr(grad), None) == 0
    _refused(lib, *bind(), INVALID,
             pre + b"a point gradient is bound to the slot (slm_gf_bind_point_grad): clear it first")
    assert lib.slm_gf_bind_point_grad(gf.h, 0, None, None) == 0
    name, args = bind()
    assert getattr(lib, name)(*args) == 0, lib.slm_last_error()
    _refused(lib, "slm_gf_bind_point_grad", (gf.h, 0, _dev_ptr(grad), None), INVALID,
             b"slm_gf_bind_point_grad: the render loss is bound to the slot (slm_gf_bind_render_loss), which owns its point "
             b"gradient: clear it first")
    _refused(lib, "slm_gf_render_loss_status", (gf.h, 0, None, None), INVALID, b"slm_gf_render_loss_status: null argument")
    # one context serves one slot
    _refused(lib, *bind(slot=1), INVALID, pre + b"the context is bound to another slot; one context serves one slot")
    name, args = bind(r=None)                               # cleared: the context is free again, and so is the point gradient
    assert getattr(lib, name)(*args) == 0
    name, args = bind(slot=1)
    assert getattr(lib, name)(*args) == 0, lib.slm_last_error()
    assert lib.slm_gf_bind_point_grad(gf.h, 0, _dev_ptr(grad), None) == 0
    # slm_gf_bind_frame clears the term
    gf._bind(1, inputs, sf, new_data)
    _refused(lib, "slm_gf_render_loss_status", (gf.h, 1, out, None), UNBOUND,
             b"slm_gf_render_loss_status: slm_gf_bind_render_loss first")
    # sharded surfels
    sh = GraphFit(cases.opt(render_loss=False), rank=0, world=2, all_reduce=lambda t: None)
    sh._bind(0, inputs, sf, new_data)
    _refused(lib, *bind(g=sh), UNSUPPORTED,
             pre + b"surfels are sharded; the render loss needs every surfel of the frame on one device")


@pytest.mark.gpu
def test_python_refusals():
    import gf_render_run_cases as cases
    from super_amd.deform_mesh import GraphFit
    with pytest.raises(NotImplementedError, match="render_in_run with opt.sf_corr_match_renderimg"):
        GraphFit(cases.opt("corr", sf_corr_match_renderimg=True), native_render_loss=True, render_in_run=True)
    gf = GraphFit(cases.opt(), native_render_loss=True)
    sf, inputs, new_data = cases.gpu_frame()
    with pytest.raises(NotImplementedError, match="needs render_in_run=True"):
        gf.forward_frames([(inputs, sf, new_data)])
    with pytest.raises(ValueError, match="max_frames is 1"):
        GraphFit(cases.opt(render_loss=False)).forward_frames([(inputs, sf, new_data)] * 2)
