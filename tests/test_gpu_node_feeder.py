"""The model-side node feeder at its edges (csrc/slm_nodes.hip through super_amd.nodes): the search across the LDS tile
boundary with exact ties, in float32, float64 and by class; the weights at dist == radius, K = 1 and K = 9, with zero class
probabilities; Surfels.update for K = 1, 4, 8 with and without the global row, N = 0, and an exactly-zero blended normal.
The inputs and the oracle's answers are node_feeder_cases.py.  Needs an MI355X (-m gpu)."""
import types

import numpy as np
import pytest

import node_feeder_cases as nfc

pytestmark = pytest.mark.gpu

TOL_W = {False: 1e-12, True: 1e-6}       # weights: float64 / float32 storage (test_knn_feeder_matches_reference_golden)
TOL_UPD = {False: 1e-12, True: 2e-7}     # update: float64 / float32 state (test_update_matches_reference_golden)
# distances: sqrt of an exact d2, within an ulp or two of float64; float32 storage rounds that once more (2^-24)
RTOL_D = {False: 1e-15, True: 1.2e-7}


def _t(a, f32=False):
    import torch
    t = torch.from_numpy(np.array(a))             # (a copy: the cached cases are read-only)
    if t.dtype == torch.float64 and f32:
        t = t.float()
    return t.cuda()


def _search(q, nodes, K, skip, f32, want_d, want_i, **kw):
    from super_amd import nodes as fd
    d, i = fd.find_knn(_t(q, f32), _t(nodes, f32), k=K, skip_self=bool(skip), **kw)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)                      # bit-exact, ties included
    np.testing.assert_allclose(d.cpu().numpy(), want_d, rtol=RTOL_D[f32], atol=0)
    return d, i


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("K,skip", [(1, 0), (1, 1), (4, 0), (4, 1), (8, 0), (8, 1)])
def test_search_around_the_tile_boundary_is_bit_exact(K, skip, f32):
    """The lattice makes equal distances common (every query of the small-span cases has a tie among its nine nearest).  The
    search kernels before slm_nodes.hip missed this in 10 of the 12 cases (all but K = 1 without skip_self; e.g. 87 of 1028 ids
    at K = 4, float64) and in the by-class case at K = 8 (2 of 480): when a nearer node arrived later, the entry it pushed down
    the list stopped in front of no entry at its own distance and so ended BEHIND a higher index.  k_knn shifts the tail
    unconditionally."""
    for Nn, Nq in nfc.search_sizes(K, skip):
        nodes, q, d9, i9 = nfc.search_case(Nn, Nq)
        _search(q, nodes, K, skip, f32, *nfc.expected_search(d9, i9, K, skip))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_search_tie_across_the_tile_edge_and_a_duplicate_in_the_second_tile(f32):
    nodes, q, d, i = nfc.tile_edge_case()
    T = nfc.KNN_TILE
    for K in (1, 2, 4):
        dd, ii = _search(q, nodes, K, 0, f32, d[:, :K], i[:, :K])
        assert int(ii[0, 0]) == T - 1 and float(dd[0, 0]) == 1.0                # the tie goes to the lower index, K = 1 too
    assert float(dd[0, 2]) == 5.0                                               # the 3-4-5 triple: sqrt(25) exactly
    dd, ii = _search(q, nodes, 4, 1, f32, d[:, 1:], i[:, 1:])
    assert int(ii[3, 0]) == T + 1 and int(ii[T + 1, 0]) == T + 1 and float(dd[3, 0]) == 0.0


@pytest.mark.parametrize("K", [1, 4, 8])
def test_search_by_class_across_the_tile_boundary(K):
    from super_amd._lib import SuperLMError
    nodes, seg, q, q_seg, d, i = nfc.class_case(K)
    _search(q, nodes, K, 0, False, d, i, num_classes=3, seg1=_t(q_seg), seg2=_t(seg))
    nodes, seg, q, q_seg, _, _ = nfc.class_case(K, short=True)
    with pytest.raises(SuperLMError) as e:
        _search(q, nodes, K, 0, False, None, None, num_classes=4, seg1=_t(q_seg), seg2=_t(seg))
    assert nfc.SHORT_CLASS_TEXT in str(e.value)


@pytest.mark.parametrize("K,radius_mode,C,f32", [
    (1, 0, 0, False), (1, 1, 0, True), (9, 0, 0, False), (9, 1, 0, False), (9, 0, 0, True), (9, 1, 0, True),
    (4, 0, 0, True), (4, 1, 0, False), (1, 0, 1, False), (9, 0, 1, False), (4, 0, 4, False), (9, 1, 4, False), (8, 0, 4, False)])
def test_weights_at_the_radius_and_with_zero_class_probabilities(K, radius_mode, C, f32):
    from super_amd import nodes as fd
    c = nfc.weights_case(K, radius_mode, C, f32)
    for stable in (c["stable"], None):
        if f32:
            w, st = fd._weights(_t(c["idx"]), _t(c["dist"]), _t(c["radii"]), radius_mode, stable=None if stable is None else _t(stable))
        else:
            conf = dict(q_conf=_t(c["q_conf"]), node_conf=_t(c["node_conf"])) if C else {}
            w, st = fd._weights64(_t(c["idx"]), _t(c["dist"]), _t(c["radii"]), radius_mode,
                                  stable=None if stable is None else _t(stable), **conf)
        w = w.cpu().numpy()
        assert w.dtype == (np.float32 if f32 else np.float64)
        np.testing.assert_allclose(w, c["w"], rtol=0, atol=TOL_W[f32])
        if K == 1:
            assert (w == 1.0).all()
        if stable is None:
            assert st is None
        else:
            np.testing.assert_array_equal(st.cpu().numpy().astype(bool), c["stable_out"])   # row 0 kept, rows 1 and 2 cleared


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("with_global", [False, True], ids=["J", "J+1"])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_update_with_and_without_the_global_row(K, with_global, f32):
    from super_amd import nodes as fd
    for N in (0, 1, 257):
        c = nfc.update_case(K, N, with_global, f32)
        ed = types.SimpleNamespace(points=_t(c["ed_points"], f32), norms=_t(c["ed_norms"], f32))
        sf = types.SimpleNamespace(points=_t(c["points"], f32), norms=_t(c["norms"], f32), knn_indices=_t(c["knn_idx"]),
                                   knn_w=_t(c["knn_w"], f32), ED_nodes=ed)
        fd.update(sf, _t(c["deform"]))
        got = (sf.points, sf.norms, ed.points, ed.norms)
        for mine, want in zip(got, c["want"]):
            assert mine.dtype == sf.points.dtype and tuple(mine.shape) == want.shape
            np.testing.assert_allclose(mine.cpu().numpy(), want, rtol=0, atol=TOL_UPD[f32])
        if N:
            assert (sf.norms[0].cpu().numpy() == 0.0).all()                     # the 1e-12 floor: 0 / 1e-12, not 0 / 0
