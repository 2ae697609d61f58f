"""The refusal texts of the older GraphFit entry points that need a solver (slm_gf_create needs a device), byte for byte:
the slot checks of the three binds, the slot-range checks every evaluation entry point shares, and the null outputs.
Their null-handle forms run without a GPU in test_refusal_texts.py."""
import ctypes as C

import pytest

from helpers import GF_SEMANTIC_VARIANTS, load_golden, torch_frame
from oracle import graphfit_oracle as gfo

pytestmark = pytest.mark.gpu

INVALID, UNBOUND, UNSUPPORTED = 1, 4, 5


def _refused(lib, name, args, code, text):
    rc = getattr(lib, name)(*args)
    got = lib.slm_last_error()
    print(name, rc, got)
    assert rc == code, (name, rc, got)
    assert got == text, (name, got)


def _opt(**kw):
    o = gfo.default_opt(**kw)
    o.deform_udpate_method, o.num_classes = "super_edg", 3
    return o


def test_refusal_texts_with_a_solver():
    import torch
    from super_amd._lib import SlmGfSemantic
    from super_amd.LM import _dev_ptr
    from super_amd.deform_mesh import GraphFit
    _, sc, _ = load_golden("s60x80_j48")
    sf, inputs, new_data = torch_frame(sc)
    gf = GraphFit(_opt(), max_frames=2)
    lib, h = gf.lib, gf.h
    sem = SlmGfSemantic(num_classes=3)
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    binds = [("slm_gf_bind_semantic", lambda slot: (h, slot, C.byref(sem), None, None)),
             ("slm_gf_bind_flow", lambda slot: (h, slot, one, None)),
             ("slm_gf_bind_point_grad", lambda slot: (h, slot, None, None))]
    for name, args in binds:
        _refused(lib, name, args(2), INVALID, name.encode() + b": bad slot")
        _refused(lib, name, args(-1), INVALID, name.encode() + b": bad slot")
        _refused(lib, name, args(1), UNBOUND, name.encode() + b": slm_gf_bind_frame first")
    _refused(lib, "slm_gf_run", (h, 3, None), INVALID, b"slm_gf: slot range out of bounds")
    _refused(lib, "slm_gf_run", (h, 1, None), UNBOUND, b"slm_gf: slot used before slm_gf_bind_frame")
    gf._bind(0, inputs, sf, new_data)
    _refused(lib, "slm_gf_run", (h, 2, None), UNBOUND, b"slm_gf: slot used before slm_gf_bind_frame")
    dv = torch.zeros((sc.J + 1, 7), dtype=torch.float64, device="cuda")
    _refused(lib, "slm_gf_get_partial", (h, 0, None, None), INVALID, b"slm_gf_get_partial: null output")
    _refused(lib, "slm_gf_get_deform", (h, 0, None, None), INVALID, b"slm_gf_get_deform: null output")
    _refused(lib, "slm_gf_loss_grad", (h, 0, None, None, _dev_ptr(dv), None), INVALID, b"slm_gf_loss_grad: null dv")
    # two slots of different num_neighbors
    _, sc6, _ = load_golden("s60x80_j48_k6")
    sf6, inputs6, new_data6 = torch_frame(sc6)
    gf._bind(1, inputs6, sf6, new_data6)
    _refused(lib, "slm_gf_run", (h, 2, None), UNSUPPORTED,
             b"slm_gf: the frames of one batch must have the same num_neighbors")
    # semantic terms enabled, the frame bound without its semantic inputs
    gs = GraphFit(_opt(**GF_SEMANTIC_VARIANTS["hard"]), max_frames=2)
    gs.semantic = False          # _bind then binds the frame alone
    gs._bind(0, inputs, sf, new_data)
    _refused(lib, "slm_gf_run", (gs.h, 1, None), UNBOUND,
             b"slm_gf: semantic terms enabled but slm_gf_bind_semantic was not called")
    _refused(lib, "slm_gf_eval_losses", (gs.h, 1, None), UNBOUND,
             b"slm_gf: semantic terms enabled but slm_gf_bind_semantic was not called")


def test_loss_grad_refuses_the_morph_term_on_a_sharded_handle():
    """One rank cannot evaluate the term's mean: the kept count it divides by is global only behind the first exchange."""
    import torch
    import gf_shape_cases as cases
    from super_amd.LM import _dev_ptr
    from super_amd._lib import GF_NTERMS, SuperLMError
    from super_amd.deform_mesh import GraphFit
    case = cases.Case("morph", 257, 12, 4, 84, semantic=True)
    frame = cases.case_frame(case)
    text = (b"slm_gf_loss_grad: surfels are sharded and the boundary-morph term is on; its mean needs the global kept "
            b"count: drive slm_gf_eval_morph / eval_losses with an all-reduce of slm_gf_get_partial behind each (null "
            b"terms and grad only set deform_verts)")
    dv = torch.from_numpy(cases.perturbed_dv(case)).cuda()
    terms = torch.zeros(GF_NTERMS, dtype=torch.float64, device="cuda")
    grad = torch.zeros_like(dv)
    gf = GraphFit(cases.opt_of("morph"), rank=1, world=2, all_reduce=lambda t: None)
    gf.bind(*frame)
    lib, h = gf.lib, gf.h
    _refused(lib, "slm_gf_loss_grad", (h, 0, _dev_ptr(dv), _dev_ptr(terms), _dev_ptr(grad), None), UNSUPPORTED, text)
    _refused(lib, "slm_gf_loss_grad", (h, 0, _dev_ptr(dv), _dev_ptr(terms), None, None), UNSUPPORTED, text)
    _refused(lib, "slm_gf_loss_grad", (h, 0, _dev_ptr(dv), None, _dev_ptr(grad), None), UNSUPPORTED, text)
    with pytest.raises(SuperLMError, match="surfels are sharded and the boundary-morph term is on"):
        gf.loss_and_grad(*frame, dv)
    # the form that only sets deform_verts stays
    assert lib.slm_gf_loss_grad(h, 0, _dev_ptr(dv), None, None, None) == 0
    torch.testing.assert_close(gf.deform_verts(), dv, rtol=0, atol=0)
    # allowed: a world of one rank (the same protocol, the whole sums), and more ranks without the term
    one = GraphFit(cases.opt_of("morph"), rank=0, world=1, all_reduce=lambda t: None)
    t, matched, _ = one.loss_and_grad(*frame, dv)
    assert matched > 0 and "sf_bn_morph_loss" in t
    hard = GraphFit(cases.opt_of("hard"), rank=1, world=2, all_reduce=lambda t: None)
    assert hard.loss_and_grad(*frame, dv)[1] > 0
