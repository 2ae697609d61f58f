"""HIP depth_preprocessing at its edges, through super_amd.data_loader: image sizes off the 256-thread block down to 8 x 8, frames
without a valid pixel, NaN / inf / threshold depths, warps that leave the image, every dilation kernel on all four borders,
deleted / absent / out-of-range / four classes, the cached context reused across variants and sizes, input forms, refusals.
Cases: depth_edge_cases.py; references: the reference's own recording tests/golden/dp_edges.npz, and the NumPy oracle where the
reference cannot run (test_depth_edge_cases.py pins the oracle against the recording).  Checks and tolerances are
test_gpu_depth._check's.  Needs an MI355X (-m gpu)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import depth_edge_cases as dec
from test_depth_edge_cases import case, reference
from test_gpu_depth import _check, _run_gpu

pytestmark = pytest.mark.gpu

FLOATS = ("points", "norms", "radii", "confs", "disp_conf", "seg_conf", "dist2edge")
ARRAYS = FLOATS + ("colors", "seg", "valid", "index_map", "inval", "depth_after")


def _compare(out, ref):
    """Non-finite values by position, then test_gpu_depth._check on the finite rest."""
    out, ref = dict(out), dict(ref)
    for k in FLOATS:
        if k in ref:
            np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)
            np.testing.assert_array_equal(np.isinf(out[k]), np.isinf(ref[k]), err_msg=k)
            odd = ~np.isfinite(ref[k])
            if odd.any():
                np.testing.assert_array_equal(np.signbit(out[k][odd]), np.signbit(ref[k][odd]), err_msg=k)
                out[k], ref[k] = np.where(odd, 0, out[k]), np.where(odd, 0, ref[k])
    _check(out, ref, "")


def _run(name, mutate=None):
    base, okw = case(name)
    return _run_gpu(base, okw, mutate)


def _same_bits(a, b):
    for k in ARRAYS:
        assert (k in a) == (k in b), k
        if k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", list(dec.CASES))
def test_edge_case_matches_its_reference(name):
    import torch
    base, okw = case(name)
    out, ref = _run(name), reference(name)
    _compare(out, ref)
    H, W = dec.CASES[name]["size"]
    T = int(ref["valid"].sum())
    assert out["valid"].dtype == np.bool_ and out["index_map"].dtype == np.int64 and out["index_map"].shape == (H, W)
    np.testing.assert_array_equal(out["valid_map"], ref["valid_map"])
    np.testing.assert_array_equal(out["index_map"].reshape(-1)[out["valid"]], np.arange(T))
    # the fields in the reference's dtypes and shapes (also with no row at all)
    for k, (dt, tail) in dec.REF_LAYOUT.items():
        if k in ref:
            tail = (int(okw.get("num_classes", 3)),) if k == "seg_conf" else tail
            assert out[k].dtype == dt and out[k].shape == (T,) + tail, (k, out[k].dtype, out[k].shape)
    assert ("seg" in out) == ("seg_conf" in out) == ("dist2edge" in out) == dec.is_seg(name)
    assert ("disp_conf" in out) == dec.is_ssim(name)
    # the reference's side effects on ``inputs``
    inputs = out["_inputs"]
    np.testing.assert_array_equal(np.isnan(out["depth_after"]), out["inval"] | np.isnan(base["depth"]))
    np.testing.assert_array_equal(np.isnan(inputs[("disp", 0)][0, 0].cpu().numpy()), out["inval"])
    assert ("valid_map" in inputs) == (okw["data"] == "superv1")
    if "valid_map" in inputs:
        assert inputs["valid_map"].dtype == torch.bool and tuple(inputs["valid_map"].shape) == (1, 1, H, W)
        np.testing.assert_array_equal(inputs["valid_map"][0, 0].cpu().numpy(), ~out["inval"])
    if name in dec.EMPTY:
        assert T == 0 and not out["valid"].any() and (out["index_map"] == -1).all()


REUSE = ("s37x53_v1dil", "sem_stripes", "s37x53_v2ssim", "s37x53_v1", "s37x53_v1dil")
REUSE_TWO_SIZES = ("s37x53_v1dil", "s61x83_v1seg", "sem_stripes", "s61x83_v2ssim", "s37x53_v2ssim", "s61x83_v1", "raft_k5",
                   "s61x83_v1n8", "s37x53_v1dil", "s61x83_v1seg")


@pytest.mark.parametrize("order", [REUSE, REUSE_TWO_SIZES], ids=["one_size", "two_sizes"])
def test_cached_context_carries_nothing_over(order):
    """One context per (H, W) holds the invalid-map pair, the warp, the SSIM map and the semantic scratch across calls: a
    segmentation with few boundary pixels, then one whose every interior pixel is one (``sel`` / ``edge_xy`` grow), then the
    stereo confidence, then a plain call, an empty frame, and the first again.  Every run matches its reference, and a
    repeated case its first run bit for bit."""
    from super_amd import data_loader
    first = {}
    for name in order:
        out = _run(name)
        _compare(out, reference(name))
        if name in first:
            _same_bits(out, first[name])
        first.setdefault(name, out)
    assert len(first) < len(order)
    sizes = {dec.CASES[n]["size"] for n in order}
    assert sizes <= {(H, W) for H, W, _ in data_loader._ctx}


FORM_CASE = "s37x53_v1n8"          # the colour image enters the normals here


def _form_float64(inputs):
    inputs[("depth", 0)] = inputs[("depth", 0)].double()


def _form_cpu(inputs):
    inputs[("depth", 0)] = inputs[("depth", 0)].cpu()
    inputs[("color", 0)] = inputs[("color", 0)].cpu()


def _form_permuted(inputs):
    c = inputs[("color", 0)]
    inputs[("color", 0)] = c.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not inputs[("color", 0)].is_contiguous() and bool((inputs[("color", 0)] == c).all())


@pytest.mark.parametrize("form", [_form_float64, _form_cpu, _form_permuted, "stream"], ids=["float64", "cpu", "permuted", "stream"])
def test_input_forms_give_the_same_bits(form):
    import torch
    plain = _run(FORM_CASE)
    _compare(plain, reference(FORM_CASE))
    if form == "stream":
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            assert torch.cuda.current_stream() != torch.cuda.default_stream()
            out = _run(FORM_CASE)
        stream.synchronize()
    else:
        out = _run(FORM_CASE, form)
    _same_bits({k: v for k, v in out.items() if k != "depth_after"}, {k: v for k, v in plain.items() if k != "depth_after"})
    # the side effect reaches the caller's tensor in its own dtype and on its own device
    after = out["_inputs"][("depth", 0)]
    assert after.dtype == (torch.float64 if form is _form_float64 else torch.float32)
    assert after.is_cuda == (form is not _form_cpu)
    np.testing.assert_array_equal(np.isnan(out["depth_after"]), out["inval"])


# ------------------------------------------------------------------------------------------------------------------ refusals
def _lib():
    from super_amd import _lib
    return _lib, _lib.load()


@pytest.mark.parametrize("size", [(7, 8), (8, 7), (7, 7)])
def test_create_refuses_images_below_8(size):
    _l, lib = _lib()
    h = C.c_void_p()
    assert lib.slm_depth_create(size[0], size[1], C.byref(h)) == _l.SLM_ERR_INVALID and not h.value
    assert lib.slm_last_error() == b"slm_depth_create: bad argument"


def _context_call(cfg_edit, with_seg=False):
    """slm_depth_preprocess on the 37 x 53 context with a config edited by ``cfg_edit``: (return code, message, T)."""
    import torch
    from super_amd import data_loader
    _l, lib = _lib()
    H, W = 37, 53
    ctx = data_loader._context(lib, H, W, torch.device("cuda", torch.cuda.current_device()))
    cfg = _l.SlmDepthConfig()
    cfg.H, cfg.W, cfg.num_classes = H, W, 3
    cfg_edit(cfg)
    depth, color = torch.zeros(H, W, device="cuda"), torch.zeros(3, H, W, device="cuda")
    seg = torch.zeros(H, W, dtype=torch.int32, device="cuda")
    inp = _l.SlmDepthInputs()
    inp.depth, inp.color = depth.data_ptr(), color.data_ptr()
    if with_seg:
        inp.seg = seg.data_ptr()
    T = C.c_int32(-7)
    rc = lib.slm_depth_preprocess(ctx, C.byref(cfg), C.byref(inp), C.byref(_l.SlmDepthOutputs()), C.byref(T), None)
    return rc, lib.slm_last_error(), T.value


def test_preprocess_refuses_a_size_that_is_not_the_context_s():
    _l, _ = _lib()
    for edit in (lambda c: setattr(c, "W", 54), lambda c: setattr(c, "H", 36), lambda c: (setattr(c, "H", 53), setattr(c, "W", 37))):
        rc, msg, T = _context_call(edit)
        assert rc == _l.SLM_ERR_INVALID and msg == b"slm_depth_preprocess: image size differs from slm_depth_create" and T == -7


def test_preprocess_refuses_four_deleted_classes_and_five_classes():
    _l, _ = _lib()
    rc, msg, T = _context_call(lambda c: setattr(c, "n_del_classes", 4), with_seg=True)
    assert rc == _l.SLM_ERR_INVALID and msg == b"slm_depth_preprocess: del_seg_classes needs the segmentation image" and T == -7
    rc, msg, T = _context_call(lambda c: setattr(c, "n_del_classes", 1))           # a deleted class and no segmentation
    assert rc == _l.SLM_ERR_INVALID and T == -7
    for n in (0, 5):
        rc, msg, T = _context_call(lambda c: setattr(c, "num_classes", n), with_seg=True)
        assert rc == _l.SLM_ERR_UNSUPPORTED and msg == b"slm_depth_preprocess: num_classes must be 1..4" and T == -7


def _python_call(okw, channels=3):
    import torch
    from super_amd.data_loader import depth_preprocessing
    base, _ = case("s37x53_v1seg")
    H, W = 37, 53
    opt = SimpleNamespace(height=H, width=W, data="superv1", load_valid_mask=False, depth_model="monodepth2",
                          dilate_invalid_kernel=0, normal_model="naive", phase="test", load_depth=True, num_classes=3)
    for k, v in okw.items():
        setattr(opt, k, v)
    inputs = {("depth", 0): torch.from_numpy(base["depth"].copy())[None, None].cuda(), ("disp", 0): torch.zeros(1, 1, H, W).cuda(),
              "inv_K": torch.from_numpy(base["inv_K"])[None], "K": torch.from_numpy(base["K"])[None],
              ("color", 0): torch.from_numpy(base["color"].copy())[None].cuda(), "divterm": float(base["divterm"]),
              "filename": ["000001"], ("seg", 0): torch.from_numpy(base["seg"])[None, None].cuda(),
              ("seg_conf", 0): torch.zeros(1, channels, H, W, dtype=torch.float64).cuda()}
    before = inputs[("depth", 0)].clone()
    try:
        depth_preprocessing(opt, None, inputs)
    finally:
        assert bool((inputs[("depth", 0)] == before).all()) and "valid_map" not in inputs     # nothing ran


def test_python_refuses_what_the_library_would():
    from super_amd._lib import SuperLMError
    with pytest.raises(ValueError, match="at most 3 del_seg_classes"):
        _python_call(dict(del_seg_classes=[0, 1, 2, 0]))
    with pytest.raises(ValueError, match="must have opt.num_classes channels"):
        _python_call(dict(), channels=2)
    with pytest.raises(ValueError, match="must have opt.num_classes channels"):
        _python_call(dict(num_classes=4))
    with pytest.raises(SuperLMError, match="num_classes must be 1..4"):
        _python_call(dict(num_classes=5), channels=5)
