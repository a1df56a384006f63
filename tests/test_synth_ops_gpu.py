"""The synthetic conditioning map on the MI355X, element by element, against its float64 twin (tests/_synth_twin.py).

Every committed case goes through td_perlin_map on the tables the twin file makes and is held to criterion A on every element, criterion B and the cap on the
bound's median.  One printed line per case.  Beside them: the probe kernel that measures the device's fast sine and cosine at the 128 gradient angles (the one
measured quantity in the bound), and the factory's own tables, all five channels, on today's 50x70 window."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _synth_twin as sw
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
U = sw.U
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def eng():
    import terrain_diffusion_amd  # noqa: F401
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return get_engine("cuda")


def perlin_map(eng, args, src, dst):
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import ptr
    rows, cols, i1, j1, seed, freq, octaves, lac, gain = args
    src, dst = np.ascontiguousarray(src, dtype=np.float32), np.ascontiguousarray(dst, dtype=np.float32)
    out = torch.full((rows, cols), 777.0, device="cuda")
    check(lib().td_perlin_map(eng._h, rows, cols, int(i1), int(j1), int(seed), float(freq), int(octaves), float(lac), float(gain),
                              C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data), len(src), ptr(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _report(name, got, ref, E, st):
    """the worst element and the bounding box of the elements outside E"""
    bad = np.argwhere(np.abs(got - ref) > E)
    if not bad.size:
        return ""
    r, c = st["at"]
    (r0, c0), (r1, c1) = bad.min(axis=0), bad.max(axis=0)
    return f"{name}: {len(bad)} elements outside E, rows {r0}..{r1}, columns {c0}..{c1}; worst at ({r}, {c}): hip {got[r, c]!r}, ref {ref[r, c]!r}, E {E[r, c]:.3g}"


@pytest.fixture(scope="module")
def results(eng):
    """every committed case once; the twin's references are computed here, once, and shared"""
    res = []
    for name, shape, got, ref, E, info in sw.run_cases(lambda name, cs: perlin_map(eng, cs["args"], cs["src"], cs["dst"])):
        res.append((name, shape, sw.judge(got, ref, E), got, ref, E, info))
    return res


def test_every_case_elementwise(results):
    assert len(results) == sw.N_CASES                           # every committed case ran, nothing skipped
    bad = []
    print()
    for name, shape, st, got, ref, E, info in results:
        print(sw.line(name, "x".join(str(s) for s in shape), st))
        assert st["elements"] == int(np.prod(shape)) and got.shape == ref.shape
        bad += [f"{name}: {v}" for v in sw.verdict(st)]
        rep = _report(name, got.astype(np.float64), ref, E, st)
        if rep:
            bad.append(rep)
    assert not bad, "\n".join(bad)


def test_clamped_and_lattice_elements_are_exact(results):
    seen = 0
    for name, shape, st, got, ref, E, info in results:
        exact = E == 0
        assert np.array_equal(got[exact].astype(np.float64), ref[exact]), name
        if "narrower" in name:
            assert exact.mean() > 0.1
            seen += 1
    assert seen == 1


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/sincos_probe.hip built with the engine's flags -> (angle, cos, sin) fp32 from the device"""
    so = str(tmp_path_factory.mktemp("probe") / "libsincos_probe.so")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *os.environ.get("TD_EXTRA_HIPCC_FLAGS", "").split(),
                           "-o", so, os.path.join(HERE, "sincos_probe.hip")])
    lib = C.CDLL(so)
    lib.sincos_probe.restype = C.c_int
    lib.sincos_probe.argtypes = [C.c_void_p] * 3
    bufs = [torch.zeros(128, device="cuda") for _ in range(3)]
    assert lib.sincos_probe(*(b.data_ptr() for b in bufs)) == 0
    return [b.cpu().numpy() for b in bufs]


def test_fast_sine_and_cosine_at_the_128_angles(probe, golden):
    """exhaustive: the kernel can form no other angle.  Not the kernel under test: the two intrinsics alone, against float64."""
    angle, c, s = probe
    assert np.array_equal(angle, sw.angles(fused=True)), "the build no longer contracts k c1 + c2: the twin's angle chain is not the device's"
    a = angle.astype(np.float64)
    ec, es = np.abs(c - np.cos(a)), np.abs(s - np.sin(a))
    rec = golden("sincos_gfx950")
    same = np.array_equal(c, rec["cos"]) and np.array_equal(s, rec["sin"])
    print(f"\n__cosf: max |error| {ec.max():.3e} at k = {int(ec.argmax())}; __sinf: {es.max():.3e} at k = {int(es.argmax())}; recorded EPS_SINCOS {sw.EPS_SINCOS:.3e}, "
          f"E uses x {sw.SINCOS_MARGIN:g}; the table {'is' if same else 'IS NOT'} the recorded one bit for bit")
    assert max(ec.max(), es.max()) <= sw.SINCOS_MARGIN * sw.EPS_SINCOS          # what E relies on


def test_factory_tables_all_five_channels(eng):
    """the factory's own statistics (its noise quantiles measured on the device): today's window and origin, every channel, through the factory's `_channel`"""
    from terrain_diffusion_amd.synthetic_map import make_synthetic_map_factory
    f = make_synthetic_map_factory(eng, frequency_mult=[1.5, 3, 3, 3, 3], seed=77)
    bad = []
    print()
    for ch in range(5):
        fr, o, l, g = f.params[ch]
        src, dst = f.stats["noise_quantile_tables"][ch].astype(np.float32), f.stats["data_quantile_tables"][ch].astype(np.float32)
        got = f._channel(ch, -37, 1200, 50, 70).cpu().numpy()
        ref, E, _ = sw.fbm_ref(50, 70, -37, 1200, f.seeds[ch], fr, o, l, g, src, dst)
        st = sw.judge(got, ref, E)
        print(sw.line(f"factory channel {ch}, 50x70 at (-37, 1200)", "50x70", st))
        bad += [f"channel {ch}: {v}" for v in sw.verdict(st)]
    assert not bad, "\n".join(bad)
