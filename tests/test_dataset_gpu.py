"""The dataset preparation on the GPU (include/td_dataset.h, dataset_csrc/dataset_kernels.hip): the void fill and the block median bit for bit
against the NumPy twin (tests/_dataset_twin.py) and the fixture (tests/golden/dataset.npz), the residual element by element against the float64
twin within its derived bound, laplacian_encode end to end (the low band by the criterion of tests/_tile_twin.py for td_resample2d), the land
counts exactly, the moments within the float64 summation bound and bit-identical between two calls, calculate_stats_welford against the
reference's recorded outputs, the chunk routine, prepare_and_encode against encode_dihedral, the enqueue-only stream mode and the C-ABI's
refusals."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _dataset_twin as twin
import _tile_twin as tw
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F = np.float32
RADII = (1, 5, 32, 64)


@pytest.fixture(scope="module")
def ds():
    from terrain_diffusion_amd import dataset
    assert torch.cuda.is_available()
    return dataset


@pytest.fixture(scope="module")
def eng():
    from terrain_diffusion_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def voids():
    """every committed case with its exact distance transform, computed once"""
    return {name: (dem, base, twin.edt(np.isnan(dem)) if not np.isnan(dem).all() else None) for name, (dem, base) in twin.void_cases().items()}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def summation_bound(n):
    return 4.0 * n * 2.0 ** -53


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ------------------------------------------------------------------------------------------------------------------------------ void fill
@pytest.mark.parametrize("radius", RADII)
def test_fill_voids_bit_for_bit(ds, voids, radius):
    assert len(voids) == 8
    for name, (dem, base, distance) in voids.items():
        want, n_voids = twin.fill_voids(dem, base, radius, False, distance)
        got, count = ds.fill_voids(dem, base, radius, return_count=True)
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == dem.shape
        g = got.cpu().numpy()
        valid = ~np.isnan(dem)
        assert np.array_equal(bits(g[valid]), bits(dem[valid])), (name, "valid pixels")
        assert np.array_equal(bits(g), bits(want)), (name, radius, int((bits(g) != bits(want)).sum()))
        assert int(count) == n_voids == int((~valid).sum()), name
        # the signed square root of the filled value; zeros by value (np.sign(-0.0) * 0.0 is +0.0)
        s = ds.fill_voids(dev(dem), dev(base), radius, True).cpu().numpy()
        ws = twin.signed_sqrt(want)
        assert np.array_equal(s, ws) and np.array_equal(bits(s[ws != 0]), bits(ws[ws != 0])), (name, radius, "signed_sqrt")
    dem, base, _ = voids["all_void_30x40"]
    assert np.array_equal(bits(ds.fill_voids(dem, base, radius).cpu().numpy()), bits(base))          # elevation_dataset.py:233
    dem, base, _ = voids["no_void_40x50"]
    assert np.array_equal(bits(ds.fill_voids(dem, base, radius).cpu().numpy()), bits(dem))


# ------------------------------------------------------------------------------------------------------------------------------ block median
@pytest.mark.parametrize("r", twin.MEDIAN_RS)
def test_block_median_bit_for_bit_against_np_median(ds, golden, r):
    g = golden("dataset")
    x, want = g["median_in"], g[f"median_r{r}"]
    got = ds.block_median(x, r)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (96 // r, 192 // r)
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), (r, int((bits(got) != bits(want)).sum()))
    assert int(np.isnan(got).sum()) == 1
    if r == 3:                                               # 340 blocks in a row, 113 to a group of the kernel: the last group holds one
        y = np.tile(x, (1, 6))[:, :1020]
        assert np.array_equal(bits(ds.block_median(y, 3).cpu().numpy()), bits(twin.block_median(y, 3)))


# ------------------------------------------------------------------------------------------------------------------------------ residual
RESIDUAL_SHAPES = [((256, 256), (32, 32)), ((96, 160), (12, 20)), ((7, 5), (1, 1)), ((37, 1031), (5, 130))]


def residual_inputs(shape, low_shape, seed):
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    x = (40.0 * np.sin(ii / 9.0) * np.cos(jj / 13.0) + rng.standard_normal(shape) * 3.0 - 12.0).astype(F)
    low = (rng.standard_normal(low_shape) * 25.0 - 10.0).astype(F)
    return x, low


@pytest.mark.parametrize("shape,low_shape", RESIDUAL_SHAPES)
def test_residual_every_element_within_the_derived_bound(ds, shape, low_shape):
    x, low = residual_inputs(shape, low_shape, shape[1])
    ref, E = twin.residual_ref(x, low)
    got = ds.residual(x, low)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    ratio = np.abs(got.cpu().numpy().astype(np.float64) - ref) / E
    print(f"\nresidual {shape} <- {low_shape}: worst err / E {ratio.max():.3f}, median E / |ref| {np.median(E / np.abs(ref)) / twin.U:.2f} u")
    assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (shape, float(ratio.max()), np.unravel_index(ratio.argmax(), shape))
    # in place
    a = dev(x)
    assert ds.residual(a, low, out=a) is a and torch.equal(a, got)


# ------------------------------------------------------------------------------------------------------------------------------ laplacian_encode
def test_laplacian_encode_end_to_end(ds, eng):
    from terrain_diffusion_amd import composition as cp
    x, _ = residual_inputs((96, 160), (1, 1), 77)
    sigma, size = 2.0, 24
    h, w = cp._resize_int_size(96, 160, size)
    assert (h, w) == (24, 40)
    # the low band in its two resampler calls, each by the criterion td_resample2d is held to
    small = cp.resize_bilinear(eng, dev(x), (h, w))
    ref, E = tw.resample_ref(x[None], cp.bilinear_aa_taps(96, h), cp.bilinear_aa_taps(160, w))
    st = tw.judge(small.cpu().numpy()[None], ref, E)
    print("\n" + tw.line("resample", "laplacian_encode: anti-aliased shrink", "96x160->24x40", st))
    assert tw.verdict("resample", st) == []
    low = cp.gaussian_blur(eng, small, sigma)
    ref, E = tw.resample_ref(small.cpu().numpy()[None], cp.gaussian_taps(h, sigma), cp.gaussian_taps(w, sigma))
    st = tw.judge(low.cpu().numpy()[None], ref, E)
    print(tw.line("resample", "laplacian_encode: gaussian blur", "24x40", st))
    assert tw.verdict("resample", st) == []
    res, lowres = ds.laplacian_encode(dev(x), size, sigma)
    assert tuple(res.shape) == (96, 160) and tuple(lowres.shape) == (24, 40) and torch.equal(lowres, low)
    # the residual by its bound, with the GPU's own low band as input
    ref, E = twin.residual_ref(x, lowres.cpu().numpy())
    ratio = np.abs(res.cpu().numpy().astype(np.float64) - ref) / E
    print(f"laplacian_encode residual: worst err / E {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    # and the whole against the CPU statement of the operator (oracle/compose.py; PARITY-UNPINNED against torchvision): both parts agree to fp32
    # rounding.  Each side rounds once per tap at most, at the magnitude of the largest input since every tap table sums to 1: 9 + 9 taps of the
    # shrink, 5 + 5 of the blur and 4 of the upsampling on either side, 2 x 32 u in all
    from oracle import compose
    ores, olow = compose.laplacian_encode(torch.from_numpy(x), size, sigma)
    assert float((lowres.cpu() - olow).abs().max()) <= 64 * twin.U * float(olow.abs().max())
    assert float((res.cpu() - ores).abs().max()) <= 64 * twin.U * float(torch.from_numpy(x).abs().max())
    assert ds.laplacian_encode(x, (24, 40), sigma)[0].equal(res)


# ------------------------------------------------------------------------------------------------------------------------------ land counts
@pytest.mark.parametrize("num_chunks", [1, 2, 3])
def test_land_counts_are_exact(ds, num_chunks):
    rng = np.random.default_rng(3)
    for shape in ((13, 20), (64, 64), (97, 301)):
        low = (rng.standard_normal(shape) * 5.0).astype(F)
        low[rng.random(shape) < 0.1] = 0.0
        low[rng.random(shape) < 0.05] = -0.0
        low[rng.random(shape) < 0.05] = np.nan
        low[0, 0], low[-1, -1] = np.nan, np.inf
        want = twin.land_counts(low, num_chunks)
        got = ds.land_counts(low, num_chunks)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (shape, num_chunks)
        share = ds.land_share(low, num_chunks)
        assert share.dtype == torch.float64
        assert np.array_equal(share.cpu().numpy(), want / float((shape[0] // num_chunks) * (shape[1] // num_chunks)))


# ------------------------------------------------------------------------------------------------------------------------------ moments
def moment_cases():
    rng = np.random.default_rng(11)
    one = (rng.standard_normal((250, 262)) * 3.0 + 1.5).astype(F)
    one.reshape(-1)[5::701] = np.nan
    three = (rng.standard_normal((3, 100, 131)) * np.array([2.0, 50.0, 0.1], F)[:, None, None] + np.array([1.0, -300.0, 0.05], F)[:, None, None]).astype(F)
    three[1].reshape(-1)[3::53] = np.nan
    many = (rng.standard_normal((19, 40, 33)) * 4.0 + np.arange(1, 20, dtype=F)[:, None, None]).astype(F)
    many[7].reshape(-1)[::17] = np.nan
    long = (rng.standard_normal(140000) * 2.0 - 7.0).astype(F)           # more than 512 blocks of 256: the strided loop of a block
    long[1000:1100] = np.nan
    return {"C1_250x262": one, "C3_100x131": three, "C19_40x33": many, "C1_140000": long}


@pytest.mark.parametrize("name", list(moment_cases()))
def test_moments_within_the_summation_bound_and_reproducible(ds, name):
    x = moment_cases()[name]
    n, mean, m2 = twin.moments(x)
    count, gm, g2 = ds.moments(x)
    assert count.dtype == torch.int64 and gm.dtype == g2.dtype == torch.float64 and tuple(gm.shape) == tuple(g2.shape) == (mean.size,)
    assert int(count) == n and 0 < n < x.size // mean.size
    bound = summation_bound(x.size // mean.size)
    print(f"\nmoments {name}: mean {rel(gm.cpu().numpy(), mean):.2e}, m2 {rel(g2.cpu().numpy(), m2):.2e} relative (bound {bound:.2e})")
    assert rel(gm.cpu().numpy(), mean) <= bound and rel(g2.cpu().numpy(), m2) <= bound
    again = ds.moments(dev(x))
    assert torch.equal(again[0], count) and np.array_equal(again[1].cpu().numpy().view(np.uint64), gm.cpu().numpy().view(np.uint64))
    assert np.array_equal(again[2].cpu().numpy().view(np.uint64), g2.cpu().numpy().view(np.uint64))


def test_moments_of_nothing_are_zero(ds):
    x = np.full((3, 5, 7), 2.0, F)
    x[1] = np.nan
    count, mean, m2 = ds.moments(x)
    assert int(count) == 0 and mean.cpu().tolist() == [0.0] * 3 and m2.cpu().tolist() == [0.0] * 3
    count, mean, m2 = ds.moments(np.array([[3.0]], F))
    assert int(count) == 1 and mean.cpu().tolist() == [3.0] and m2.cpu().tolist() == [0.0]


def test_calculate_stats_welford_against_the_reference_outputs(ds, golden):
    g = golden("dataset")
    info = json.loads(str(g["stats"]))
    group = twin.stats_group()
    assert twin.group_crc(group) == info["crc"]
    bound = summation_bound(info["n"]) * info["chunks"]
    for name in ("residual", "climate"):
        for tag, pct in (("p0", 0.0), ("p4", 0.4)):
            m64, s64 = g[f"stats_{name}_f64_{tag}_means"], g[f"stats_{name}_f64_{tag}_stds"]
            m32, s32 = g[f"stats_{name}_f32_{tag}_means"], g[f"stats_{name}_f32_{tag}_stds"]
            means, stds = ds.calculate_stats_welford(group, name, pct)
            assert np.shape(means) == m64.shape and np.asarray(means).dtype == np.float64
            print(f"\nwelford {name} {tag}: vs float64-fed reference {rel(means, m64):.2e} / {rel(stds, s64):.2e} (bound {bound:.2e}); "
                  f"the float32-fed reference is {rel(m32, m64):.2e} / {rel(s32, s64):.2e} from its float64 run")
            assert rel(means, m64) <= bound and rel(stds, s64) <= bound, (name, tag)
            # the float32-fed reference runs its 2-D path in float32: it is held only to its own recorded distance from its float64 run
            assert rel(means, m32) <= (rel(m32, m64) + bound) * (1 + 1e-6) and rel(stds, s32) <= (rel(s32, s64) + bound) * (1 + 1e-6), (name, tag)
    with pytest.raises(ValueError, match="No elevation data"):
        ds.calculate_stats_welford(group, "elevation")


# ------------------------------------------------------------------------------------------------------------------------------ the chunk routine
def chunk_inputs(size=96):
    dem, base = twin.void_cases()["hole_150x170"]
    return np.ascontiguousarray(dem[:size, :size]), np.ascontiguousarray(base[:size, :size])


@pytest.mark.parametrize("num_chunks,edge_margin", [(1, 0), (2, 0), (3, 1)])
def test_prepare_chunks_is_the_device_forms_in_the_references_order(ds, num_chunks, edge_margin):
    dem, base = chunk_inputs()
    chunks = ds.prepare_chunks(dem, base, 12, 2.0, num_chunks, edge_margin, chunk_id="17")
    want = twin.prepare_chunks(dem, base, 12, 2.0, num_chunks, edge_margin, chunk_id="17")
    assert len(chunks) == len(want) == num_chunks ** 2
    m = edge_margin * 8
    d, b = (dem[m:-m, m:-m], base[m:-m, m:-m]) if m else (dem, base)
    filled = ds.fill_voids(d, b, 32, True)
    res, low = ds.laplacian_encode(filled, 12 - 2 * edge_margin, 2.0)
    counts = twin.land_counts(low.cpu().numpy(), num_chunks).reshape(-1)
    _, boxes = twin.reference_boxes(96, 12, num_chunks, edge_margin)
    for k, (c, w, (sub, (h0, h1, w0, w1), (l0, l1, m0, m1))) in enumerate(zip(chunks, want, boxes)):
        assert set(c) == {"residual", "lowfreq", "lowres_exact", "pct_land", "chunk_id", "subchunk_id"} and "climate" not in c
        assert (c["chunk_id"], c["subchunk_id"]) == ("17", sub) == (w["chunk_id"], w["subchunk_id"])
        assert all(c[key].is_cuda and c[key].dtype == torch.float32 and tuple(c[key].shape) == w[key].shape for key in ("residual", "lowfreq", "lowres_exact"))
        # the fill and the square root are exact, so the block median equals the CPU routine's bit for bit
        assert np.array_equal(bits(c["lowres_exact"].cpu().numpy()), bits(w["lowres_exact"])), sub
        assert torch.equal(c["residual"], res[h0:h1, w0:w1]) and torch.equal(c["lowfreq"], low[l0:l1, m0:m1])
        assert isinstance(c["pct_land"], float) and c["pct_land"] == counts[k] / float((l1 - l0) * (m1 - m0))
        assert float((c["residual"].cpu() - torch.from_numpy(w["residual"])).abs().max()) <= 64 * twin.U * float(np.abs(filled.cpu().numpy()).max())


def test_prepare_and_encode_gives_encode_dihedrals_bits(ds):
    import terrain_diffusion_amd as td
    import _ae_twin as T
    cfg = dict(T.TINY, in_channels=1, direct_skips=[0])     # the tiny config of tests/test_autoencoder_gpu.py with the residual's one channel
    m = td.EDMAutoencoder(**cfg, dtype="fp32").load_state_dict(T.synth_ae_state_dict(cfg, seed=81))
    try:
        dem, base = chunk_inputs()
        mean, std = 0.11, 1.1678
        got = ds.prepare_and_encode(m, dem, base, 12, 2.0, mean, std, num_chunks=2, chunk_id="5")
        chunks = ds.prepare_chunks(dem, base, 12, 2.0, num_chunks=2, chunk_id="5")
        assert len(got) == 4
        for a, b in zip(got, chunks):
            assert torch.equal(a["residual"], b["residual"]) and a["subchunk_id"] == b["subchunk_id"]
            want = m.encode_dihedral(b["residual"][None].contiguous(), mean, std)
            assert a["latents"].dtype == torch.float16 and tuple(a["latents"].shape) == (8, 6, 24, 24) and a["latents"].is_cuda
            assert torch.equal(a["latents"].view(torch.int16), want.view(torch.int16))
        assert not torch.equal(got[0]["latents"], got[3]["latents"])
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------------------------ the library as a whole
def _everything(ds, inputs):
    dem, base, x3 = inputs
    filled, count = ds.fill_voids(dem, base, 32, True, return_count=True)
    med = ds.block_median(filled[:144, :168], 8)
    res, low = ds.laplacian_encode(filled, 24, 2.0)
    return [filled, count, med, res, low, ds.land_counts(low, 2), *ds.moments(x3)]


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(ds, eng, voids):
    dem, base, _ = voids["hole_150x170"]
    inputs = [dev(dem), dev(base), dev(moment_cases()["C3_100x131"])]
    ref = _everything(ds, inputs)
    again = _everything(ds, inputs)
    for a, b in zip(ref, again):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = [t.clone() for t in inputs]                   # produced on the caller's stream, consumed there without a host sync
        got = [t.clone() for t in _everything(ds, x)]     # read on that stream after the calls
    torch.cuda.current_stream().synchronize()
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def test_c_abi_argument_errors(ds, eng):
    from terrain_diffusion_amd._lib import TdError
    st = C.c_void_p(eng.stream)
    l = ds.lib()
    dp = lambda t: C.c_void_p(t.data_ptr())
    plane, out, low = torch.zeros(8, 8, device="cuda"), torch.empty(8, 8, device="cuda"), torch.zeros(2, 2, device="cuda")
    cnt = torch.empty(4, dtype=torch.int32, device="cuda")
    n64, d64 = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.float64, device="cuda")
    host, hosti = torch.zeros(8, 8), torch.zeros(4, dtype=torch.int32)
    big = 16385
    bad = [
        lambda: l.td_dataset_fill_voids(st, dp(plane), dp(plane), 0, 8, 32, 0, dp(out), dp(cnt), 1),
        lambda: l.td_dataset_fill_voids(st, dp(plane), dp(plane), 8, big, 32, 0, dp(out), dp(cnt), 1),
        lambda: l.td_dataset_fill_voids(st, dp(plane), dp(plane), 8, 8, 0, 0, dp(out), dp(cnt), 1),
        lambda: l.td_dataset_fill_voids(st, dp(plane), dp(plane), 8, 8, 65, 0, dp(out), dp(cnt), 1),
        lambda: l.td_dataset_fill_voids(st, None, dp(plane), 8, 8, 32, 0, dp(out), dp(cnt), 1),
        lambda: l.td_dataset_fill_voids(st, dp(plane), dp(plane), 8, 8, 32, 0, dp(out), None, 1),
        lambda: l.td_dataset_fill_voids(st, dp(host), dp(plane), 8, 8, 32, 0, dp(out), dp(cnt), 1),
        lambda: l.td_dataset_fill_voids(st, dp(plane), dp(plane), 8, 8, 32, 0, dp(out), dp(hosti), 1),
        lambda: l.td_dataset_fill_voids(st, dp(plane), dp(plane), 8, 8, 32, 0, dp(plane), dp(cnt), 1),
        lambda: l.td_dataset_block_median(st, dp(plane), 8, 8, 0, dp(out), 1),
        lambda: l.td_dataset_block_median(st, dp(plane), 8, 8, 33, dp(out), 1),
        lambda: l.td_dataset_block_median(st, dp(plane), 8, 8, 3, dp(out), 1),
        lambda: l.td_dataset_block_median(st, dp(plane), big, 8, 1, dp(out), 1),
        lambda: l.td_dataset_block_median(st, dp(plane), 8, 8, 2, None, 1),
        lambda: l.td_dataset_block_median(st, dp(plane), 8, 8, 2, dp(host), 1),
        lambda: l.td_dataset_block_median(st, dp(plane), 8, 8, 2, dp(plane), 1),
        lambda: l.td_dataset_residual(st, dp(plane), dp(low), 8, 8, 0, 2, dp(out), 1),
        lambda: l.td_dataset_residual(st, dp(plane), dp(low), 8, big, 2, 2, dp(out), 1),
        lambda: l.td_dataset_residual(st, dp(plane), None, 8, 8, 2, 2, dp(out), 1),
        lambda: l.td_dataset_residual(st, dp(plane), dp(host), 8, 8, 2, 2, dp(out), 1),
        lambda: l.td_dataset_residual(st, dp(plane), dp(low), 4, 8, 2, 2, C.c_void_p(plane.data_ptr() + 64), 1),
        lambda: l.td_dataset_residual(st, dp(plane), dp(plane), 8, 8, 2, 2, dp(plane), 1),
        lambda: l.td_dataset_land_counts(st, dp(plane), 8, 8, 0, dp(cnt), 1),
        lambda: l.td_dataset_land_counts(st, dp(plane), 8, 8, 9, dp(cnt), 1),
        lambda: l.td_dataset_land_counts(st, dp(plane), 8, 8, 65, dp(cnt), 1),
        lambda: l.td_dataset_land_counts(st, dp(plane), 8, 8, 2, dp(hosti), 1),
        lambda: l.td_dataset_land_counts(st, None, 8, 8, 2, dp(cnt), 1),
        lambda: l.td_dataset_moments(st, dp(plane), 0, 64, dp(n64), dp(d64), dp(d64), 1),
        lambda: l.td_dataset_moments(st, dp(plane), 1025, 64, dp(n64), dp(d64), dp(d64), 1),
        lambda: l.td_dataset_moments(st, dp(plane), 1, 0, dp(n64), dp(d64), dp(d64), 1),
        lambda: l.td_dataset_moments(st, dp(plane), 1, (1 << 30) + 1, dp(n64), dp(d64), dp(d64), 1),
        lambda: l.td_dataset_moments(st, dp(plane), 8, 1 << 30, dp(n64), dp(d64), dp(d64), 1),
        lambda: l.td_dataset_moments(st, dp(plane), 1, 64, None, dp(d64), dp(d64), 1),
        lambda: l.td_dataset_moments(st, dp(host), 1, 64, dp(n64), dp(d64), dp(d64), 1),
        lambda: l.td_dataset_moments(st, dp(plane), 1, 64, C.c_void_p(n64.data_ptr() + 4), dp(d64), dp(d64), 1),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(TdError):
            ds.check(fn())
        assert l.td_dataset_last_error().decode().startswith("td_dataset_"), k
    # what is allowed: the residual in place
    ds.check(l.td_dataset_residual(st, dp(plane), dp(low), 8, 8, 2, 2, dp(plane), 1))
    assert bool((plane == 0).all())
