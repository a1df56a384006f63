"""Shaded-relief rendering, host side (no GPU): the product's colormap table and Gaussian weights against the ones the reference's libraries
produced (tests/golden/relief.npz, tests/golden/make_relief_golden.py), the NumPy twin against every recorded case, and the argument checks
of get_relief_map that must refuse before any engine is touched."""
import json

import numpy as np
import pytest

import _relief_twin as twin


def _cases(golden):
    g = golden("relief")
    for c in json.loads(str(g["cases"])):
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c["kwargs"].items()}
        yield c["name"], g[c["input"]], kw, g["out_" + c["name"]]


def test_terrain_lut_and_gaussian_weights_match_the_recorded_ones(golden):
    from terrain_diffusion_amd.relief import gaussian_weights, terrain_lut
    g = golden("relief")
    lut = terrain_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.float32
    assert np.abs(lut.astype(np.float64) - g["terrain_lut"]).max() < 1e-7
    for sigma in (6.0, 1.2, 3.0, 0.8):
        w, r = gaussian_weights(sigma)
        ref = g[f"impulse_{sigma}"]
        assert r == int(4 * sigma + 0.5) and w.shape == ref.shape, sigma
        assert np.array_equal(w, ref.astype(np.float32)), sigma                # the fp64 weights, rounded once to fp32
    assert gaussian_weights(6.0)[1] == 24 and gaussian_weights(1.2)[1] == 5


def test_twin_matches_every_recorded_case(golden):
    names = []
    for name, elev, kw, want in _cases(golden):
        got = twin.relief(elev, **kw)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        msg = twin.compare(got, want, tol=5e-5, step_frac=0.0)
        assert msg is None, (name, msg)
        names.append(name)
    assert len(names) == 11


def test_recorded_cases_cover_the_branches(golden):
    c = {name: (elev, kw, out) for name, elev, kw, out in _cases(golden)}
    assert (c["all_land"][0] > 0).all()                                     # automatic vmin above 0: the non-offset colormap branch
    e, kw, out = c["explicit_range"]
    assert (e > 0).any() and (e[e > 0] < kw["vmin"]).any() and (e > kw["vmax"]).any()
    assert ((out == 0).all(axis=-1) & (e > 0)).any()                        # land below vmin: the colormap's bad colour
    assert np.isnan(c["nan_pos_median"][2]).any() and np.nanmedian(c["nan_pos_median"][0]) > 0
    e, _, out = c["nan_neg_median"]
    assert np.isnan(e).any() and np.nanmedian(e) < 0 and not np.isnan(out).any()   # ocean colour replaces the NaN
    assert np.ptp(c["constant"][0]) == 0 and (c["all_ocean"][0] < 0).all()
    assert c["tiny_7x5"][0].shape == (7, 5) and c["tiny_2x9"][0].shape == (2, 9) and c["narrow_31x97"][0].shape == (31, 97)


@pytest.mark.parametrize("arg", ["biome", "flow", "rgb"])
def test_get_relief_map_refuses_unsupported_inputs(arg):
    from terrain_diffusion_amd import get_relief_map
    e = np.zeros((8, 8), np.float32)
    kw = {"biome": None, "flow": None}
    if arg == "rgb":
        with pytest.raises(NotImplementedError, match="rgb"):
            get_relief_map(e, None, None, None, rgb=np.zeros((8, 8, 3), np.float32))
    else:
        kw[arg] = np.zeros((8, 8), np.float32)
        with pytest.raises(NotImplementedError, match=arg):
            get_relief_map(e, None, kw["biome"], kw["flow"])


@pytest.mark.parametrize("shape", [(1, 8), (8, 1), (1, 1), (8,), (2, 3, 4)])
def test_get_relief_map_refuses_images_below_2x2(shape):
    from terrain_diffusion_amd import get_relief_map
    with pytest.raises(ValueError):
        get_relief_map(np.zeros(shape, np.float32), None, None, None)


def test_relief_library_exports_what_its_header_declares():
    import ctypes
    import os
    import re
    import __graft_entry__ as ge
    from terrain_diffusion_amd import relief
    ge.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ge.ROOT, "include", "td_relief.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(td_[a-z0-9_]+)\s*\(", text))
    assert declared == set(relief.EXPORTS) == {"td_relief_last_error", "td_relief_map"}
    lib = ctypes.CDLL(relief.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
