"""libtd_batch.so on the GPU (include/td_batch.h, batch_csrc/batch_kernels.hip) element by element at its edges, on the inputs of
tests/_train_data_shapes.py and against its independent references (tests/test_train_data_ops_cpu.py shows, without a GPU, that they and
the twin agree and that the inputs tell the wrong variants apart): every transform of rectangular views that overhang every side of planes of
unlike sides, through the C ABI; the affine at its arithmetic edges; the half exponential on all 65536 logvars; rectangular and hand-placed
latent draws; the designed 32 x 32 blocks against numpy.quantile and math.fsum under all 8 transforms; odd cond-image grids with the dropout
and noise edges; the cond vector's centre window at g = 4 .. 7.  Every comparison asks for the same bits, NaN for NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import _train_data_shapes as sh
import _train_data_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F, H = np.float32, np.float16
same, where = sh.same_values, sh.first_difference
GUARD = 256                              # elements past the end of an output of a C-ABI call, which must stay as they were
SENTINEL = 12288.0                       # exact in half too


@pytest.fixture(scope="module")
def td_():
    from terrain_diffusion_amd import train_data
    assert torch.cuda.is_available()
    return train_data


@pytest.fixture(scope="module")
def place(td_):
    return td_.DeviceGroups(sh.TREE(), sh.PLACE_KEYS, sh.ALL_PLANES)


@pytest.fixture(scope="module")
def partial(td_):
    """the placement groups without lowres_exact, climate and latent: null pointers in the group table"""
    return td_.DeviceGroups(sh.TREE(), sh.PLACE_KEYS, ("lowfreq", "residual"))


@pytest.fixture(scope="module")
def edge(td_):
    return td_.DeviceGroups(sh.TREE(), sh.EDGE_KEYS, ("latent", "lowfreq"))


@pytest.fixture(scope="module")
def design(td_):
    return td_.DeviceGroups(sh.TREE(), sh.DESIGN_KEYS, ("lowres_exact", "climate"))


def P(t):
    return C.c_void_p(t.data_ptr())


def c_views(td_, groups, items, plane, origin, offset, h, w):
    """td_batch_views through the C ABI (the Python form only takes squares): (N, h, w), the guard behind the output checked"""
    from terrain_diffusion_amd._plumbing import call
    eng, dev = groups.resolve()
    it = torch.as_tensor(items, dtype=torch.int32).to(dev).contiguous()
    n = it.shape[0] * h * w
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    call(td_._LIB, "td_batch_views", eng, dev, P(groups.table()), len(groups), P(it), it.shape[0], td_.PLANES[plane], origin, offset, h, w, 0, 0.0, 1.0,
         1.0, P(out), ordered=True)
    host = out.cpu().numpy()
    assert (host[n:] == F(SENTINEL)).all(), "a write past the end of the output"
    return host[:n].reshape(it.shape[0], h, w)


# ------------------------------------------------------------------------------------------------------------------------------ 1. views
@pytest.mark.parametrize("h,w", sh.VIEW_SHAPES)
def test_rectangular_views_equal_the_loop_on_every_side_of_every_plane(td_, place, h, w):
    compared = 0
    for plane in sh.VIEW_PLANES:
        for origin in (0, 1):
            items = sh.view_items(h, w, plane, origin)
            got = c_views(td_, place, items, plane, origin, sh.VIEW_OFFSETS[origin], h, w)
            want = sh.views_ref(plane, items, origin, h, w)
            assert same(got, want), (plane, origin, where(got, want))
            compared += got.size
    print(f"\n({h}, {w}): {compared} elements, 8 transforms x 7 window positions x 3 planes x 2 origins, the same bits")


def test_a_plane_the_groups_do_not_hold_gives_nan_views_zero_latents_and_a_masked_cond_image(td_, partial):
    from terrain_diffusion_amd._plumbing import call
    items = sh.view_items(5, 9, "lowfreq", 0)
    assert np.isnan(c_views(td_, partial, items, "lowres_exact", 0, -1, 5, 9)).all()
    got, want = c_views(td_, partial, items, "lowfreq", 0, -1, 5, 9), sh.views_ref("lowfreq", items, 0, 5, 9)
    assert same(got, want), where(got, want)
    eng, dev = partial.resolve()
    it = torch.as_tensor(sh.rect_items(3, 5), dtype=torch.int32).to(dev)
    for mode, dtype in ((0, torch.float32), (1, torch.float16)):
        n = it.shape[0] * sh.PLACE_LC * 15 * (64 if mode else 1)
        out = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=dev)
        noise = torch.ones((it.shape[0], sh.PLACE_LC, 3, 5), dtype=dtype, device=dev)
        stat = torch.ones(sh.PLACE_LC, dtype=torch.float32, device=dev)
        call(td_._LIB, "td_batch_latents", eng, dev, P(partial.table()), len(partial), P(it), it.shape[0], sh.PLACE_LC, 3, 5, mode, P(noise), P(stat), P(stat),
             0.5, P(out), ordered=True)
        host = out.cpu().numpy()
        assert (host[:n] == 0).all() and not np.signbit(host[:n]).any() and (host[n:] == SENTINEL).all(), mode
    img = td_.cond_image(partial, sh.CROPS[96], 96).cpu().numpy()
    assert np.isnan(img[:, :6]).all() and (img[:, 6] == 0).all()


def test_the_affine_rounds_each_operation_once_at_its_edges(td_, edge):
    x = sh.AFFINE_X.reshape(4, 4)
    items = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, 6, 0, 0]], np.int32)
    for abc in sh.AFFINE_ABC:
        got = td_.views(edge, items, "lowfreq", 4, affine=abc).cpu().numpy()
        y = sh.affine_ref(x, *abc)
        want = np.stack([y, sh.view_loop(y, 0, 0, 4, 4, 6)])
        assert same(got, want), (abc, where(got, want))


# ------------------------------------------------------------------------------------------------------------------------------ 2. latents
def test_the_half_exponential_on_all_65536_logvars_in_every_slab(td_):
    groups = td_.DeviceGroups(sh.TREE(), sh.EXP_KEYS, ("latent",))
    table = sh.exp_table()
    with np.errstate(all="ignore"):
        e = twin.half_std(table)                                                             # (8, 256, 256)
    items = np.array([[0, 0, 0, t, 0, 0] for t in range(8)], np.int32)
    got = td_.sample_latents(groups, items, torch.ones(8, 1, sh.EXP_S, sh.EXP_S), mode=0, mean=[0.0], std=[1.0], sigma_data=1.0).cpu().numpy()[:, 0]
    nan_in = np.isnan(table)
    bad = ~same_elements(got, e.astype(F))
    print(f"\nmode 0: {got.size} exponentials ({int(nan_in.sum())} NaN logvars, {int(np.isinf(e).sum())} inf, {int((e == 0).sum())} zero); {int(bad.sum())} differ"
          + "".join(f"\n  logvar {table[i]!r}: gpu {got[i]!r}, twin {e[i]!r}" for i in list(zip(*np.nonzero(bad)))[:8]))
    assert got.size == 8 * 65536 and np.array_equal(np.isnan(got), nan_in) and not bad.any()
    # mode 1: 16 rows of every slab, each value over its 8 x 8 pixels
    rows = np.array([[0, 32 * t + 5, 0, t, 0, 0] for t in range(8)], np.int32)
    got1 = td_.sample_latents(groups, rows, torch.ones(8, 1, 16, sh.EXP_S, dtype=torch.float16), mode=1).cpu().numpy()[:, 0]
    assert got1.shape == (8, 128, 8 * sh.EXP_S) and got1.dtype == H
    want1 = np.stack([e[t, 32 * t + 5:32 * t + 21] for t in range(8)])
    cells = got1.reshape(8, 16, 8, sh.EXP_S, 8)
    assert same(cells, np.broadcast_to(want1[:, :, None, :, None], cells.shape).copy()), where(cells[:, :, 0, :, 0], want1)


def same_elements(a, b):
    """per element: the same bits, or NaN on both sides"""
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("h,w", sh.RECT_SHAPES)
def test_rectangular_latent_windows_that_leave_the_latent(td_, place, h, w):
    items = sh.rect_items(h, w)
    for mode in (0, 1):
        noise = sh.rect_noise(h, w, mode)
        kw = dict(mean=sh.RECT_MEAN, std=sh.RECT_STD, sigma_data=sh.RECT_SIGMA) if mode == 0 else {}
        got = td_.sample_latents(place, items, torch.from_numpy(noise), mode=mode, **kw).cpu().numpy()
        assert got.shape == ((len(items), sh.PLACE_LC, 8 * h, 8 * w) if mode else (len(items), sh.PLACE_LC, h, w))
        for n, (g, i, j, t, _, _) in enumerate(items.tolist()):
            lat = sh.arrays(sh.PLACE_KEYS[g])["latent"]
            want = sh.latents_window(lat, t, i, j, h, w, noise[n], mode, sh.latent_draw_ref, **kw)
            assert same(got[n], want), (mode, n, where(got[n], want))                         # +0 outside: the bits are compared
            assert same(got[n], sh.latents_window(lat, t, i, j, h, w, noise[n], mode, sh.twin_draw, **kw)), (mode, n)
            if mode:
                cells = got[n].reshape(sh.PLACE_LC, h, 8, w, 8)
                assert same(cells, np.broadcast_to(cells[:, :, :1, :, :1], cells.shape).copy()), n       # every 8 x 8 replica is constant


def test_the_latent_arithmetic_at_its_edges(td_, edge):
    lat = sh.arrays(sh.EDGE_KEYS[0])["latent"]
    items = np.array([[0, 0, 0, 0, 0, 0]], np.int32)
    for mode in (0, 1):
        kw = dict(mean=sh.EDGE_MEAN, std=sh.EDGE_STD, sigma_data=sh.EDGE_SIGMA) if mode == 0 else {}
        got = td_.sample_latents(edge, items, torch.from_numpy(sh.edge_noise(mode)), mode=mode, **kw).cpu().numpy()[0]
        want = sh.latent_draw_ref(lat[0, :2], lat[0, 2:], sh.edge_noise(mode)[0], mode, **kw)
        got = got.reshape(2, 4, 8, 4, 8)[:, :, 0, :, 0] if mode else got
        assert same(got, want), (mode, where(got, want))
        if mode:
            flat = got.reshape(2, 16)
            assert flat[0, 4] == 1 and flat[0, 5] == H(1 + 2.0 ** -9) and flat[0, 8] == 1 and np.isinf(flat[0, 9])       # ties to even


# ------------------------------------------------------------------------------------------------------------------------------ 3. cond image
def test_the_designed_blocks_equal_numpy_quantile_and_math_fsum_under_every_transform(td_, design):
    items = sh.design_items()
    raw = td_.cond_image(design, items, 64).cpu().numpy()
    norm = td_.cond_image(design, items, 64, mean=sh.NORM_MEAN, std=sh.NORM_STD).cpu().numpy()
    assert raw.shape == (24, 7, 4, 4)
    for k, (n, _, _, t, _, _) in enumerate(items.tolist()):
        want = sh.design_raw_ref(n, t)
        names = np.array(sh.DESIGN_LAYOUT[n]).reshape(4, 4)
        bad = ~same_elements(raw[k], want)
        assert not bad.any(), (n, t, where(raw[k], want), "blocks of the untransformed plane:", sorted(set(sh.view_loop(np.arange(16, dtype=F).reshape(4, 4), 0, 0, 4, 4, t)[bad.any(0)].astype(int).tolist())), names.tolist())
        assert same(norm[k], sh.normalise_ref(want)), (n, t, where(norm[k], sh.normalise_ref(want)))
        a = sh.arrays(sh.DESIGN_KEYS[n])
        with np.errstate(all="ignore"):
            assert same(raw[k], twin.cond_image(a["lowres_exact"], a["climate"], 32, 32, 64, t, raw=True)), (n, t)
    zeros = [raw[t, 1].reshape(-1)[np.flatnonzero(sh.view_loop(np.arange(16, dtype=F).reshape(4, 4), 0, 0, 4, 4, t).reshape(-1) == s)[0]]
             for t in range(8) for s in (8, 9, 10)]
    assert all(z == 0 and not np.signbit(z) for z in zeros)                                  # -0 / +0 at the ranks: +0 by the kernel's arithmetic


@pytest.mark.parametrize("crop", sorted(sh.CROPS))
def test_other_crops_with_the_dropout_and_noise_edges(td_, place, crop):
    items, d = sh.CROPS[crop], sh.crop_draws(crop)
    g = (crop + 64) // 32
    raw = td_.cond_image(place, items, crop).cpu().numpy()
    assert raw.shape == (3, 7, g, g) and same(raw, sh.crop_raw_ref(crop)), where(raw, sh.crop_raw_ref(crop))
    kw = dict(u_drop=d["u_drop"], dropout=sh.DROPOUT_P, u_noise=d["u_noise"], max_noise=sh.MAX_NOISE, z_mean=d["z_mean"], z_p5=d["z_p5"])
    full_raw = td_.cond_image(place, items, crop, **kw).cpu().numpy()
    assert same(full_raw, sh.crop_twin(crop, raw=True)), where(full_raw, sh.crop_twin(crop, raw=True))
    assert np.isnan(full_raw[0, 0, 1, 1]) and not np.isnan(full_raw[0, 0, 1, 2]) and np.isnan(full_raw[0, 0, 2, 1])      # == p drops, above p keeps, NaN drops
    full = td_.cond_image(place, items, crop, mean=sh.NORM_MEAN, std=sh.NORM_STD, **kw).cpu().numpy()
    assert same(full, sh.crop_twin(crop)), where(full, sh.crop_twin(crop))
    std = list(sh.NORM_STD)
    std[3] = np.nan
    bad_std = td_.cond_image(place, items, crop, mean=sh.NORM_MEAN, std=std, **kw).cpu().numpy()
    assert same(bad_std, sh.crop_twin(crop, norm_std=std)) and np.isnan(bad_std[:, 3]).all()


# ------------------------------------------------------------------------------------------------------------------------------ cond vector
@pytest.mark.parametrize("g", sh.VECTOR_GS)
def test_the_cond_vector_reads_the_centre_window_in_the_stated_order(td_, g):
    d = sh.vector_inputs(g)
    img = torch.from_numpy(d["img"]).cuda()
    for z in (None, d["z_replace"]):
        vec, flags = td_.cond_vector(img, d["hist"], d["noise_level"], z)
        vec, flags = vec.cpu().numpy(), flags.cpu().numpy()
        assert vec.shape == (sh.VECTOR_N, 58) and flags.shape == (sh.VECTOR_N, 4)
        for n in range(sh.VECTOR_N):
            want, wf = sh.cond_vector_ref(d["img"][n], d["hist"][n], d["noise_level"][n], None if z is None else z[n])
            assert same(vec[n], want) and np.array_equal(flags[n], wf), (g, n, z is None, where(vec[n], want), flags[n], wf)
    assert flags.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0]]
