"""The shaded-relief kernels on the MI355X, element by element, against their float64 twin (tests/_relief_ops_twin.py).

Every committed case goes through td.relief_map and is held to criterion A on every element against the nearer of the one or two LUT rows the twin admits, to
criterion B, the cap on the bound's median, the two-candidate share and exact NaN positions.  One printed line per case; a failure names the worst pixel and the
bounding box of the pixels outside E.  Three cases also go through td_relief_map with tables, fill and scalars made on the host by the twin, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _relief_ops_twin as rw
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


def _kw(kw):
    return {("azimuths" if k == "azimuth" else k): ((v,) if k == "azimuth" else v) for k, v in kw.items()}


def render(td, e, kw):
    return td.relief_map(torch.from_numpy(np.ascontiguousarray(e)).cuda(), **_kw(kw)).cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    return rw.cases()


@pytest.fixture(scope="module")
def results(td, cases):
    """every committed case once; the twin's references are computed here, once, and shared"""
    res = {}
    for name, (e, kw) in cases.items():
        tw = rw.relief_ref(e, **kw)
        got = render(td, e, kw)
        res[name] = (got, tw, rw.judge(got, tw))
    return res


def test_every_case_elementwise(results, cases):
    assert len(results) == rw.N_CASES                           # every committed case ran, nothing skipped
    bad = []
    print()
    for name, (got, tw, st) in results.items():
        e = cases[name][0]
        print(rw.line(name, "x".join(str(s) for s in e.shape), st))
        assert got.shape == e.shape + (3,) and got.dtype == np.float32 and st["elements"] == 3 * e.size
        v = rw.verdict(st)
        if v:
            bad.append(f"{name}: " + "; ".join(v) + " -- " + rw.failures(st))
    assert not bad, "\n".join(bad)


def test_exact_elements_are_exact(results):
    """relief = 0 leaves the LUT row itself on the land (E = 0 there); the bad colour is 0; NaN pixels of the input are NaN unless the fill makes them ocean"""
    got, tw, st = results["scalars: relief 0 (the colormap alone), 160x224"]
    exact = (tw["refs"][0][1] == 0) & (tw["refs"][1][1] == 0) & np.isfinite(tw["refs"][0][0])
    assert exact.mean() > 0.5
    near = np.where(np.abs(got - tw["refs"][0][0]) <= np.abs(got - tw["refs"][1][0]), tw["refs"][0][0], tw["refs"][1][0])
    assert np.array_equal(got[exact].astype(np.float64), near[exact])
    got, tw, st = results["range: all NaN but one ocean pixel, 9x12"]
    assert np.isfinite(got).all()
    got, tw, st = results["range: all NaN, 9x12"]
    assert np.isnan(got).all()


@pytest.mark.parametrize("name", rw.HOST_TABLE_CASES)
def test_host_made_tables_give_the_same_bits(td, results, cases, name):
    """td_relief_map with the LUT, the two weight tables, the radii, the fill and the scalars the twin makes: the tables the kernel reads are the twin's"""
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.relief import check, lib
    e, kw = cases[name]
    k = dict(rw.DEFAULTS, **kw)
    lut, wl, rl, ws, rs = rw.tables(k["sigma_large"], k["sigma_small"])
    filled, nan, has_fill, fill = rw.fill_of(e)
    eng = get_engine("cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    d_e, d_lut, d_wl, d_ws = dev(e), dev(lut), dev(wl), dev(ws)
    out = torch.full(e.shape + (3,), 777.0, device="cuda")
    dp = lambda t: C.c_void_p(t.data_ptr())
    has_range = k["vmin"] is not None and k["vmax"] is not None
    torch.cuda.synchronize()
    check(lib().td_relief_map(C.c_void_p(eng.stream), dp(d_e), e.shape[0], e.shape[1], dp(d_lut), dp(d_wl), rl, dp(d_ws), rs, float(k["azimuth"]), float(k["resolution"]),
                              float(k["relief"]), int(has_range), float(k["vmin"] or 0.0), float(k["vmax"] or 0.0), int(has_fill), float(fill), dp(out), 1))
    got = out.cpu().numpy()
    assert np.array_equal(got, results[name][0], equal_nan=True)
    st = rw.judge(got, results[name][1])
    print("\n" + rw.line(name + " [host-made tables]", "x".join(str(s) for s in e.shape), st))
    assert not rw.verdict(st), rw.verdict(st)
