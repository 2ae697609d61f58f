"""Inputs of the N-channel renderer tests (test_gpu_render_channels.py, test_gpu_render_channels_python.py) on the scenes of
render_radii_cases.py, and what the float64 model render_channels_model.py says about them, computed once and shared.
Features are uniform in [0,1) from a seed, the background C distinct values; nothing here reads a kernel's output.  Hit sets,
`near` pixels and the rows left out of a gradient comparison do not depend on the features: they are those of
render_radii_cases.facts, whose caps test_render_radii_cases.py proves on the CPU."""
import functools

import numpy as np

import render_channels_model as rcm
import render_radii_cases as rc

ONE_RADIUS = 2e-3      # the one-radius forward on `link`: covers pixels, unlike the default 2e-4


def bg(C):
    return (0.1 + 0.1 * np.arange(C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def features(name, C):
    """(N,C) float32, uniform in [0,1) (treat as read-only)"""
    n = len(rc.facts(name)["scene"]["P"])
    return np.random.default_rng(100 * C + n).uniform(size=(n, C)).astype(np.float32)


def _geo(s):
    return s["K"], s["H"], s["W"], s["view_scale"]


@functools.lru_cache(maxsize=None)
def want(name, C, one_radius=False):
    """the model's render of the scene with features(name, C) and bg(C), with its own radii or ONE_RADIUS"""
    s = rc.facts(name)["scene"]
    return rcm.render(s["P"], features(name, C), s["radii"], *_geo(s), bg=bg(C), n_track=s["n_track"],
                      radius=ONE_RADIUS if one_radius else None)


@functools.lru_cache(maxsize=None)
def grad_facts(name, C):
    """-> dict(g (h,w,C) a dL/dimage, grads: the model's (dL/dP, dL/df, dL/dr) for it); the rows left out are
    render_radii_cases.facts(name)["ex"]"""
    f = rc.facts(name)
    s = f["scene"]
    h, w = f["want"]["near"].shape
    g = np.random.default_rng(len(s["P"]) + C).normal(size=(h, w, C))
    return dict(g=g, grads=rcm.grads(s["P"], features(name, C), s["radii"], g, f["hits"], *_geo(s), bg=bg(C)))
