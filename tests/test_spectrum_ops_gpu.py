"""The spectrum kernels (spectrum_csrc/spectrum_kernels.hip) element by element on the GPU.  The library is built with contraction off and
sums through fixed trees, so its fp32 results are a function of the inputs alone and tests/_spectrum_twin.py restates them in NumPy fp32:

  half spectrum   the int32 view of fft2's output equals fft2_fp32's at EVERY coefficient: the committed cases, every side 8 .. 4096 on each
                  axis, 512 and 2048 on both, and batches whose column tiles cross a plane stride;
  against float64 |F_gpu - F64| <= E at every coefficient of the same planes, E the running bound of fft2_bound: independent of the
                  restatement, so either side being wrong shows;
  log|F|          every position of the new shapes against float64 0.5 log(re^2 + im^2) of the device's own spectrum, one fp32 rounding, the
                  mirrored half taken from row (H - r) % H, column W - k;
  decode          bits equal decode_fp32's at every element, the count of v <= 0 exact: the score cases, sizes off the tile, identity taps,
                  -0.0, an exact cancellation, a NaN in either input;
  ring means      every mean against the float64 mean of the device's own plane over host_bin_map's ring, within the summation bound and one
                  fp32 rounding; counts exact; an empty ring 0.0.

Measured on an MI355X: see DESIGN.md, "How the spectrum kernels are checked"."""
import numpy as np
import pytest
import torch

import _beauty_twin as twin
import _spectrum_twin as st
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F = np.float32
RING_BINS = (1, 4, 7, 64)


@pytest.fixture(scope="module")
def bt():
    from terrain_diffusion_amd import beauty
    assert torch.cuda.is_available()
    return beauty


def summation_bound(n):
    """the relative bound on a float64 sum of n terms in any order, the device's and NumPy's together (tests/test_dataset_gpu.py's form)"""
    return 4.0 * n * 2.0 ** -53


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def planes():
    return st.all_planes()


@pytest.fixture(scope="module")
def device_spectra(bt, planes):
    """{name: (half complex64, logabs fp32)} as NumPy arrays: one call per plane or batch, both outputs, made once and left unchanged"""
    out = {}
    for name, x in planes.items():
        half, logabs = bt.fft2(dev(x), spectrum=True, logabs=True)
        assert half.dtype == torch.complex64 and tuple(half.shape) == x.shape[:-1] + (x.shape[-1] // 2 + 1,)
        assert logabs.dtype == torch.float32 and tuple(logabs.shape) == x.shape
        out[name] = (half.cpu().numpy(), logabs.cpu().numpy())
    return out


def singles(planes, device_spectra):
    """[(name, x, half, logabs)] plane by plane, the members of a batch as name[i]"""
    for name, x in planes.items():
        half, logabs = device_spectra[name]
        if x.ndim == 2:
            yield name, x, half, logabs
        else:
            for i in range(x.shape[0]):
                yield f"{name}[{i}]", x[i], half[i], logabs[i]


@pytest.fixture(scope="module")
def float64_side(planes):
    """{name: (F64 half spectrum, E)} of every single plane, computed once"""
    return {name: (twin.half_of(twin.spectrum(x)), st.fft2_bound(x)) for name, x in st.single_planes(planes)}


# ------------------------------------------------------------------------------------------------------------------------------ spectrum
def test_half_spectrum_bits_equal_the_restatement_at_every_coefficient(planes, device_spectra, float64_side):
    failures, total = [], 0
    for name, x, half, _ in singles(planes, device_spectra):
        want = st.fft2_fp32(x)
        assert half.shape == want.shape
        differ = (st.int_view(half) != st.int_view(want)).any(-1)
        total += half.size
        print(f"bits {name:18s} {half.size:7d} coefficients  differing {int(differ.sum())}")
        if differ.any():
            f64, E = float64_side[name]
            first = tuple(int(v) for v in np.argwhere(differ)[0])
            ulps = int(np.maximum(st.ulp_distance(half.real, want.real), st.ulp_distance(half.imag, want.imag)).max())
            inside = bool((np.abs(half.astype(np.complex128) - f64) <= E)[differ].all())
            failures.append(f"{name}: {int(differ.sum())} of {half.size} coefficients differ, first at {first} (device {half[first]!r}, restatement "
                            f"{want[first]!r}), largest distance {ulps} ulp, device within E of float64 at all of them: {inside}")
    print(f"bits: {total} coefficients compared over {len(float64_side)} planes")
    assert not failures, "\n".join(failures)


def test_every_coefficient_within_E_of_float64(planes, device_spectra, float64_side):
    worst = {}
    for name, x, half, _ in singles(planes, device_spectra):
        f64, E = float64_side[name]
        err = np.abs(half.astype(np.complex128) - f64)
        worst[name] = float((err / E).max())
        print(f"float64 {name:18s} {half.size:7d} coefficients  worst err / E {worst[name]:.4f}")
        assert (err <= E).all(), (name, worst[name], tuple(int(v) for v in np.argwhere(err > E)[0]))
    print(f"float64: largest err / E over {len(worst)} planes {max(worst.values()):.4f}")
    assert max(worst.values()) >= 0.01                     # the bound decides something (tests/test_spectrum_ops_cpu.py says what)


def test_logabs_every_position_of_the_new_shapes(planes, device_spectra):
    new = set(st.new_planes())
    for name, x, half, la in singles(planes, device_spectra):
        if name.split("[")[0] not in new:
            continue
        H, W = x.shape
        re, im = half.real.astype(np.float64), half.imag.astype(np.float64)
        with np.errstate(divide="ignore"):
            own_half = 0.5 * np.log(re * re + im * im)     # of the device's own spectrum: the kernel rounds it once
        own = np.empty((H, W))
        own[:, :W // 2 + 1] = own_half
        k = np.arange(W // 2 + 1, W)
        own[:, W // 2 + 1:] = own_half[(H - np.arange(H)) % H][:, W - k]
        zero = np.isneginf(own)
        assert np.array_equal(np.isneginf(la), zero), name                 # -inf at an exact zero and nowhere else
        assert (zero.sum() == H * W - 1) == name.endswith("batch5_16x32[4]")  # the flat plane
        ok = ~zero
        # one rounding to fp32, and 2^-52 of |F|^2 either way in float64, which the logarithm hands on as it is
        slack = twin.ulp32(own[ok]) + 2.0 ** -50 * np.maximum(1.0, np.abs(own[ok]))
        assert np.isfinite(own[ok]).all() and (np.abs(la.astype(np.float64)[ok] - own[ok]) <= slack).all(), name
        # the mirrored half is the same fp32 value, written once more: columns 0 and W / 2 have no mirror
        mirror = la[(H - np.arange(H)) % H][:, W - k]
        assert np.array_equal(la[:, W // 2 + 1:].view(np.int32), np.ascontiguousarray(mirror).view(np.int32)), name


# ------------------------------------------------------------------------------------------------------------------------------ decode
def test_decode_bits_equal_the_restatement_and_the_count_is_exact(bt):
    failures = []
    for name, (low, res) in st.decode_cases().items():
        want, nonpos = st.decode_fp32(low, res)
        got, stats = bt.decode_terrain(dev(low), dev(res), return_stats=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == res.shape
        g = got.cpu().numpy()
        differ = g.view(np.int32) != want.view(np.int32)
        count = int(stats["nonpos"].cpu())
        print(f"decode {name:18s} {g.size:6d} elements  differing {int(differ.sum())}  nonpos {count} (restatement {nonpos})")
        if differ.any() or count != nonpos:
            first = tuple(int(v) for v in np.argwhere(differ)[0]) if differ.any() else None
            failures.append(f"{name}: {int(differ.sum())} of {g.size} elements differ, first at {first}"
                            + (f" (device {g[first]!r}, restatement {want[first]!r}, {int(st.ulp_distance(g, want)[differ].max())} ulp at most)" if first else "")
                            + f"; nonpos {count}, restatement {nonpos}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------------------ ring means
def _ring_planes(device_spectra):
    """[(name, fp32 (H, W))]: a log|F| plane the device produced, and planes of values spread over +-30 whose sizes leave a ragged tail"""
    yield "logabs_terrain_1024", device_spectra["terrain_1024"][1]
    for i, (H, W) in enumerate(((8, 8), (24, 40), (300, 257))):
        yield f"spread_{H}x{W}", ((twin.uniform(300 + i, H * W).reshape(H, W) - 0.5) * 60.0).astype(F)


def test_ring_means_within_the_summation_bound_of_the_devices_own_plane(bt, device_spectra):
    empty = 0
    for name, plane in _ring_planes(device_spectra):
        H, W = plane.shape
        v = plane.astype(np.float64)
        assert np.isfinite(v).all()
        for bins in RING_BINS:
            ring = bt.host_bin_map(H, W, bins).numpy()
            counts, means = bt.radial_bins(dev(plane)[None], bins)
            assert means.dtype == torch.float32 and tuple(means.shape) == (1, bins) and tuple(counts.shape) == (1, bins)
            c, m = counts.cpu().numpy()[0], means.cpu().numpy()[0].astype(np.float64)
            assert np.array_equal(c, np.bincount(ring.ravel(), minlength=256)[:bins]), (name, bins)
            worst = 0.0
            for b in range(bins):
                members = v[ring == b]
                if members.size == 0:
                    assert m[b] == 0.0 and not np.signbit(m[b])
                    empty += 1
                    continue
                want = float(members.mean())
                sums = summation_bound(members.size) * float(np.abs(members).mean())
                bound = sums + 0.5 * float(twin.ulp32(abs(want) + sums))       # the sum's order, then one rounding of the mean to fp32
                worst = max(worst, abs(m[b] - want) / bound)
                assert abs(m[b] - want) <= bound, (name, bins, b, m[b], want, bound)
            print(f"ring means {name:20s} bins {bins:2d}: worst |gpu - mean64| / bound {worst:.3f}")
    assert empty > 40                                       # 64 rings over 8 x 8: most are empty
