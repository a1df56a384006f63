"""libtd_objective.so on the GPU (include/td_objective.h, objective_csrc/objective_kernels.hip) against the twin (tests/_objective_twin.py) and
the fixture (tests/golden/objective.npz: the reference's own train_step, calc_loss and _normalize_and_process_terrain).

Shapes are the smallest at which each kernel can go wrong: H x W in 1 x 1, 17 x 19 (odd rows: no 16-byte alignment, the 4-byte path),
64 x 64, 3 x 1366 (4098 elements) and 2 x 129 (258 = the 256-thread span of a reduction pass plus two); N in 1, 3, 33; C in 1, 5; Cc in 0, 2;
K in 1, 64, 128, 130; a base pointer 4 bytes off a 16-byte boundary; an all-equal plane; a plane with one NaN; one value with scale_sigma.

Criteria (the issue's): levels within 1 fp32 ulp of the float64 twin and within e_ref + 1 ulp of the recorded values; x and v bit for bit the
NumPy fp32 twin on the device's own table, and within the table's differences carried through the formula of the recorded ones; logvar within
the bound of tests/_emb_twin.py for a 'float' input row, whose median over |ref| stays below that file's cap; S within HW 2^-52 S of the exact
sum; the loss within 8 x 2^-52 (float64) and 1 ulp (fp32) of the twin on the device's own S, and within e_ref + 1 ulp, carried, of the
recorded loss when fed the recorded model_output; the uint8 images exactly; two runs and the enqueue-only mode the same bits throughout.

End to end: validation_loss on the engine against the same loop over oracle.unet.OracleUnet and the float64 twin, with the same draws.  The
project states its per-forward bound against the oracle as a relative RMS b (fp32 5e-6, bf16 2e-2: README, tests/test_gpu_parity.py), that is
||out - out_ref||_2 <= b ||out_ref||_2 over the batch.  The loss is quadratic in out, loss(out + D) - loss(out) = g . D + sum a_n D_n^2 with
g = dloss / dout = -2 d / (N C HW exp(lv_n) sd) and a_n = 1 / (N C HW exp(lv_n)), so
    |loss - loss_ref| <= ||g||_2 b ||out_ref||_2 + max_n a_n (b ||out_ref||_2)^2 + sum_n |dloss / dlv_n| E_n
(Cauchy-Schwarz; E_n the logvar bound), every term computed by the test from the data.  Measured on an MI355X, |loss - loss_ref| over this margin:
see DESIGN.md section 6.
"""
import ctypes as C
import json
import math
import zlib

import numpy as np
import pytest
import torch

import _objective_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
same_bits, within, ulp32 = twin.same_bits, twin.within, twin.ulp32
# (N, C, Cc, H, W)
COMBOS = ((1, 1, 0, 1, 1), (3, 5, 2, 17, 19), (33, 5, 2, 64, 64), (3, 1, 2, 3, 1366), (1, 5, 0, 2, 129), (33, 1, 0, 17, 19), (3, 5, 0, 64, 64))
B_FORWARD = {"fp32": 5e-6, "bf16": 2e-2}           # the project's stated per-forward rel-RMS bounds against the oracle


@pytest.fixture(scope="module")
def ob():
    from terrain_diffusion_amd import objective
    assert torch.cuda.is_available()
    return objective


@pytest.fixture(scope="module")
def fx(golden):
    return golden("objective")


@pytest.fixture(scope="module")
def cases(fx):
    return json.loads(str(fx["cases"]))


def get(fx, case, key):
    k = f"{case['name']}_{key}"
    return fx[k] if k in fx.files else None


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def off4(a):
    """a device copy of `a` whose base address is 4 bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=F)
    buf = torch.empty(a.size + 5, dtype=torch.float32, device="cuda")
    k = 1 + (-(buf.data_ptr() // 4) % 4)           # the first element at a 16-byte boundary, plus one
    t = buf[k:k + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def three_runs(fn):
    """fn(**extra) twice and once only enqueued: the first result (numpy, or a tuple of them), after asserting that all three have the same bits"""
    outs = []
    for extra in ({}, {}, {"enqueue_only": True}):
        r = fn(**extra)
        r = r if isinstance(r, tuple) else (r,)
        outs.append(tuple(host(t) for t in r))
    for o in outs[1:]:
        assert all(same_bits(a, b) for a, b in zip(o, outs[0]))
    return outs[0] if len(outs[0]) > 1 else outs[0][0]


def data(N, Cn, Cc, H, W, seed=3):
    rng = np.random.default_rng(seed + N + 7 * Cn + 13 * H + W)
    d = dict(image=(rng.standard_normal((N, Cn, H, W)) * 0.6).astype(F), noise=rng.standard_normal((N, Cn, H, W)).astype(F),
             z=rng.standard_normal(N).astype(F), out=rng.standard_normal((N, Cn, H, W)).astype(F))
    d["cond"] = rng.standard_normal((N, Cc, H, W)).astype(F) if Cc else None
    return d


def head(K, seed=9):
    """the logvar head's tensors as MPFourier and MPConv make them, the weight folded by the host's fold"""
    import _conv_twin as ct
    rng = np.random.default_rng(seed + K)
    f, p = (2 * np.pi * rng.standard_normal(K)).astype(F), (2 * np.pi * rng.random(K)).astype(F)
    w = rng.standard_normal((1, K)).astype(F)
    return f, p, w, ct.fold_host(torch.from_numpy(w), 1).numpy().reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------------ levels
def check_table(got, want):
    for j, k in enumerate(twin.LEVEL_COLS):
        assert within(got[:, j], want[k], ulp32(want[k])), (k, got[:, j], want[k])


@pytest.mark.parametrize("N", (1, 3, 33))
def test_levels_within_one_ulp_of_float64(ob, N):
    rng = np.random.default_rng(N)
    z = (rng.standard_normal(N) * 1.3).astype(F)
    got = three_runs(lambda **kw: ob.noise_levels(dev(z), sigma_data=0.5, P_mean=-0.4, P_std=1.2, **kw))
    assert got.shape == (N, 6) and got.dtype == F
    check_table(got, twin.levels64(z, "draw", 0.5, -0.4, 1.2))
    sig = np.exp(rng.uniform(math.log(0.002), math.log(80.0), N)).astype(F)
    check_table(three_runs(lambda **kw: ob.noise_levels(dev(sig), mode="sigma", sigma_data=0.5, **kw)), twin.levels64(sig, "sigma", 0.5))
    t = np.linspace(1e-3, 1.5705, N, dtype=F) if N > 1 else np.array([0.7853], F)
    got = three_runs(lambda **kw: ob.noise_levels(dev(t), mode="t", sigma_data=1.0, **kw))
    check_table(got, twin.levels64(t, "t", 1.0))
    assert same_bits(got[:, 1], t)


@pytest.mark.parametrize("combo", COMBOS)
def test_levels_with_scale_sigma(ob, combo):
    N, Cn, Cc, H, W = combo
    d = data(*combo)
    ch = [0, 1, 2, 3] if Cn == 5 else [0]
    if N > 1:
        d["image"][1, ch] *= F(0.02)                # below the eps floor
    img = off4(d["image"]) if H in (17, 64) else dev(d["image"])
    got = three_runs(lambda **kw: ob.noise_levels(dev(d["z"]), sigma_data=0.5, P_mean=-0.4, P_std=1.0, images=img, scale_channels=ch, eps=0.05, **kw))
    want = twin.levels64(d["z"], "draw", 0.5, -0.4, 1.0, d["image"], ch, 0.05)
    check_table(got, want)
    if Cn * H * W == 1:                             # one value: torch.std is NaN and propagates through the max
        assert np.isnan(got[:, [0, 1, 2, 3, 4, 5]]).all()
    else:
        assert np.isfinite(got).all() and (N == 1 or want["std"][1] / 0.5 < 0.05 < want["std"][0] / 0.5)


def test_levels_one_nan_propagates(ob):
    d = data(3, 5, 0, 17, 19)
    d["image"][1, 2, 5, 7] = np.nan
    got = three_runs(lambda **kw: ob.noise_levels(dev(d["z"]), sigma_data=0.5, images=dev(d["image"]), scale_channels=[0, 1, 2, 3], **kw))
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()
    check_table(got, twin.levels64(d["z"], "draw", 0.5, 0.0, 1.0, d["image"], [0, 1, 2, 3], 0.05))


def device_table(ob, fx, c):
    return ob.noise_levels(dev(get(fx, c, "d_z")), sigma_data=c["sigma_data"], P_mean=c["P_mean"], P_std=c["P_std"],
                           images=dev(get(fx, c, "image")) if c["scale"] else None, scale_channels=c["channels"], eps=c["eps"])


def test_levels_against_the_recorded_reference(ob, fx, cases):
    for c in cases:
        got = host(device_table(ob, fx, c))
        refs = dict(sigma=get(fx, c, "ratio").astype(D) * float(F(c["sigma_data"])), t=get(fx, c, "t"), cos=get(fx, c, "cos"), sin=get(fx, c, "sin"))
        if c["scale"]:
            refs["std"] = get(fx, c, "std")
        for k, r in refs.items():
            assert within(got[:, twin.LEVEL_COLS.index(k)], r, get(fx, c, "eref_" + k) + ulp32(r)), (c["name"], k)


# ------------------------------------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("misaligned", (False, True))
def test_noise_equals_the_twin_bit_for_bit(ob, combo, misaligned):
    N, Cn, Cc, H, W = combo
    d = data(*combo)
    table = ob.noise_levels(dev(d["z"]), sigma_data=0.5, P_mean=-0.4, P_std=1.2)
    put = off4 if misaligned else dev
    img, nz, cond = put(d["image"]), put(d["noise"]), (put(d["cond"]) if Cc else None)
    x, v = three_runs(lambda **kw: ob.add_noise(img, nz, table, sigma_data=0.5, cond_img=cond, **kw))
    wx, wv = twin.add_noise32(d["image"], d["noise"], host(table), 0.5, d["cond"])
    assert x.shape == (N, Cn + Cc, H, W) and v.shape == (N, Cn, H, W)
    assert same_bits(x, wx) and same_bits(v, wv)
    if Cc:
        assert same_bits(x[:, Cn:], d["cond"])


def test_noise_one_nan_propagates_as_in_torch(ob):
    d = data(3, 5, 2, 64, 64)
    d["image"][1, 2, 5, 7] = np.nan
    d["noise"][2, 0, 0, 0] = np.nan
    table = ob.noise_levels(dev(d["z"]), sigma_data=0.5)
    x, v = three_runs(lambda **kw: ob.add_noise(dev(d["image"]), dev(d["noise"]), table, sigma_data=0.5, cond_img=dev(d["cond"]), **kw))
    wx, wv = twin.add_noise32(d["image"], d["noise"], host(table), 0.5, d["cond"])
    assert np.array_equal(x, wx, equal_nan=True) and np.array_equal(v, wv, equal_nan=True)
    assert np.isnan(x).sum() == 2 and np.isnan(v).sum() == 2


def test_noise_against_the_recorded_reference(ob, fx, cases):
    for c in cases:
        table = device_table(ob, fx, c)
        image, noise, cond = get(fx, c, "image"), get(fx, c, "d_noise"), get(fx, c, "cond_img")
        x, v = (host(t) for t in ob.add_noise(dev(image), dev(noise), table, sigma_data=c["sigma_data"], cond_img=None if cond is None else dev(cond)))
        tb = host(table).astype(D)
        dc, ds = np.abs(tb[:, 2] - get(fx, c, "cos")), np.abs(tb[:, 3] - get(fx, c, "sin"))     # the table's differences, carried through the formula
        bx, bv = twin.noise_carry(dc, ds, image, noise, c["sigma_data"])
        xr = get(fx, c, "x")
        assert within(x[:, :c["C"]], xr[:, :c["C"]], bx) and same_bits(x[:, c["C"]:], xr[:, c["C"]:]), c["name"]
        assert within(v, get(fx, c, "v_t"), bv), c["name"]
        assert float(np.max(bx)) <= 64 * twin.U * float(np.max(np.abs(xr))) and float(np.max(bv)) <= 64 * twin.U * float(np.max(np.abs(xr)))


# ------------------------------------------------------------------------------------------------------------------------------ logvar
@pytest.mark.parametrize("K", (1, 64, 128, 130))
@pytest.mark.parametrize("N", (1, 3, 33))
def test_logvar_within_the_float_row_bound(ob, K, N):
    f, p, _, wf = head(K)
    t = np.linspace(1e-3, 1.5705, N, dtype=F) if N > 1 else np.array([0.7853], F)
    table = ob.noise_levels(dev(t), mode="t", sigma_data=1.0)
    got = three_runs(lambda **kw: ob.logvar(table, dev(f), dev(p), dev(wf), **kw))
    ref, E = twin.logvar64(host(table)[:, 4], f, p, wf)
    assert got.shape == (N,) and within(got, ref, E), (got, ref, E)
    assert float(np.median(E / np.abs(ref))) <= twin.CAP, float(np.median(E / np.abs(ref))) / twin.U


def test_logvar_against_the_recorded_reference(ob, fx, cases):
    for c in cases:
        table = device_table(ob, fx, c)
        f, p, wf = get(fx, c, "lv_freqs"), get(fx, c, "lv_phases"), get(fx, c, "lv_wfold").reshape(-1)
        got = host(ob.logvar(table, dev(f), dev(p), dev(wf)))
        xlv = host(table)[:, 4]
        _, E = twin.logvar64(xlv, f, p, wf)
        want = twin.levels64(get(fx, c, "d_z"), "draw", c["sigma_data"], c["P_mean"], c["P_std"], get(fx, c, "image"), c["channels"], c["eps"])
        dx = np.abs(xlv.astype(D) - want["table"][:, 4].astype(D))                 # 0 unless the device's x_lv rounds the other way
        y = np.abs(np.outer(xlv.astype(D), f.astype(D))) + np.abs(p.astype(D))[None, :]
        carried = np.where(dx[:, None] > 0, dx[:, None] * np.abs(f.astype(D))[None, :] + 2 * ulp32(y), 0.0) @ np.abs(wf.astype(D)) * math.sqrt(2.0)
        r = get(fx, c, "logvar")
        assert within(got, r, get(fx, c, "eref_logvar") + ulp32(r) + E + carried), c["name"]


# ------------------------------------------------------------------------------------------------------------------------------ sqerr, loss
@pytest.mark.parametrize("combo", COMBOS)
def test_sqerr_and_the_three_losses(ob, combo):
    N, Cn, Cc, H, W = combo
    d = data(*combo)
    v = (d["noise"] * F(0.7)).astype(F)
    out, vv = (off4(d["out"]), off4(v)) if H in (17, 64) else (dev(d["out"]), dev(v))
    S = three_runs(lambda **kw: ob.squared_error(out, vv, sigma_data=0.5, **kw))
    want = twin.sqerr64(d["out"], v, 0.5)
    assert S.dtype == D and S.shape == (N, Cn) and within(S, want, H * W * 2.0 ** -52 * want)
    lv = (np.random.default_rng(N).standard_normal(N) * 0.8).astype(F)
    for form, groups in (("weighted", None), ("plain", None), ("grouped", [1, 4] if Cn == 5 else [1])):
        kw0 = dict(sigma_data=0.5, form=form, loss_groups=groups, logvar=dev(lv) if form == "weighted" else None)
        items, l64, l32 = three_runs(lambda **kw: ob.v_loss(dev(S, torch.float64), H, W, **kw0, **kw)[1:])
        wi, wl = twin.loss64(S, H * W, 0.5, lv, form, groups)
        terms = np.abs(wi - lv) + np.abs(lv) if form == "weighted" else np.abs(wi)           # an item is m / (exp(lv) sd^2) + lv
        assert within(items, wi, 8 * 2.0 ** -52 * terms), form
        assert within(l64, wl, 8 * 2.0 ** -52 * abs(wl)), (form, l64, wl)
        assert within(l32, wl, ulp32(wl)) and l32[0] == F(l64[0]) and l32.dtype == F
        assert ob.v_loss(dev(S, torch.float64), H, W, **kw0).value == float(l64[0])


def test_loss_takes_more_items_than_a_block_has_threads(ob):
    """300 items: a thread of the one block takes two.  logvar >= 0 here, so that no item is a difference of nearly equal terms and the relative
    criterion means what it says (exp is the device's float64 one, good to an ulp or two of ITS result, not of the item's)."""
    rng = np.random.default_rng(4)
    S, lv = rng.random((300, 5)) * 40.0, np.abs(rng.standard_normal(300) * 0.5).astype(F)
    items, l64, l32 = three_runs(lambda **kw: ob.v_loss(dev(S, torch.float64), 17, 19, sigma_data=1.0, logvar=dev(lv), **kw)[1:])
    wi, wl = twin.loss64(S, 17 * 19, 1.0, lv, "weighted")
    assert within(items, wi, 8 * 2.0 ** -52 * np.abs(wi)), float(np.max(np.abs(items - wi) / np.abs(wi))) * 2.0 ** 52
    assert within(l64, wl, 8 * 2.0 ** -52 * abs(wl)), (l64, wl)
    assert within(l32, wl, ulp32(wl))


def test_sqerr_one_nan_stays_in_its_plane(ob):
    d = data(3, 5, 0, 17, 19)
    d["out"][1, 2, 5, 7] = np.nan
    S = three_runs(lambda **kw: ob.squared_error(dev(d["out"]), dev(d["noise"]), sigma_data=0.5, **kw))
    bad = np.zeros((3, 5), bool)
    bad[1, 2] = True
    assert np.array_equal(np.isnan(S), bad)
    r = ob.v_loss(dev(S, torch.float64), 17, 19, sigma_data=0.5, form="plain")
    assert math.isnan(r.value) and np.array_equal(np.isnan(host(r.items)), bad.any(axis=1))


def test_loss_against_the_recorded_reference_on_the_recorded_model_output(ob, fx, cases):
    for c in cases:
        sd, HW = c["sigma_data"], c["H"] * c["W"]
        table = device_table(ob, fx, c)
        image, noise, cond = get(fx, c, "image"), get(fx, c, "d_noise"), get(fx, c, "cond_img")
        _, v = ob.add_noise(dev(image), dev(noise), table, sigma_data=sd, cond_img=None if cond is None else dev(cond))
        lv = ob.logvar(table, dev(get(fx, c, "lv_freqs")), dev(get(fx, c, "lv_phases")), dev(get(fx, c, "lv_wfold").reshape(-1)))
        out = get(fx, c, "model_output")                    # the recorded model_output: the U-Net is not in the way
        S = ob.squared_error(dev(out), v, sigma_data=sd)
        r = ob.v_loss(S, c["H"], c["W"], sigma_data=sd, logvar=lv)
        # the tolerance, from the fixture alone: cos, sin and logvar lie within e_ref + 1 ulp of the reference's (asserted above), carried on
        dc, ds = (get(fx, c, "eref_" + k) + ulp32(get(fx, c, k)) for k in ("cos", "sin"))
        _, bv = twin.noise_carry(dc, ds, image, noise, sd)
        vr, lvr = get(fx, c, "v_t"), get(fx, c, "logvar")
        _, E = twin.logvar64(host(table)[:, 4], get(fx, c, "lv_freqs"), get(fx, c, "lv_phases"), get(fx, c, "lv_wfold"))
        dlv = get(fx, c, "eref_logvar") + ulp32(lvr) + E
        Sr = twin.sqerr64(out, vr, sd)
        tol = get(fx, c, "eref_loss") + ulp32(get(fx, c, "loss")) + twin.loss_carry(Sr, twin.sq_carry(out, vr, bv, sd), HW, sd, lvr, dlv, "weighted")
        print(f"{c['name']}: loss {r.value:.9g} / fp32 {float(host(r.loss32)[0]):.9g}, recorded {float(get(fx, c, 'loss')[0]):.9g}, tolerance {float(tol[0]):.2e}")
        assert within(host(r.loss32), get(fx, c, "loss"), tol), c["name"]
        assert float(tol[0]) <= 2e-3 * abs(float(get(fx, c, "loss")[0])) + 1e-4
    c0 = cases[0]
    S = ob.squared_error(dev(get(fx, c0, "model_output")), dev(get(fx, c0, "v_t")), sigma_data=c0["sigma_data"])
    for key, form, groups in (("plain", "plain", None), ("g14", "grouped", [1, 4]), ("g23", "grouped", [2, 3])):
        r = ob.v_loss(S, c0["H"], c0["W"], sigma_data=c0["sigma_data"], form=form, loss_groups=groups)
        ref = fx["curve_" + key]
        assert within(host(r.loss32), ref, fx["curve_" + key + "_eref"] + ulp32(ref)), key


# ------------------------------------------------------------------------------------------------------------------------------ terrain_u8
def test_terrain_bytes_equal_the_recorded_ones(ob, fx):
    got = three_runs(lambda **kw: ob.terrain_uint8(dev(fx["terrain"]), **kw))
    assert got.dtype == np.uint8 and np.array_equal(got, fx["terrain_u8"])


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("misaligned", (False, True))
def test_terrain_bytes_equal_the_twin(ob, combo, misaligned):
    N, Cn, Cc, H, W = combo
    rng = np.random.default_rng(H + W)
    t = (rng.standard_normal((N, Cn, H, W)) * 700.0 + 200.0).astype(F)          # ranges above 255: the extremes land on 0 and 255
    if N > 1:
        t[1] = F(-37.25)                                                          # an all-equal item: the range is floored at 255
    if N > 2:
        t[2] = (rng.random((Cn, H, W)) * 90.0).astype(F)                           # a narrow item, floored too
        t[N - 1, 0, 0, 0] = np.nan                                                # one NaN: amin / amax make the whole item NaN; bytes 0 here
    x = off4(t) if misaligned else dev(t)                                         # H W % 4 == 0 with a base off 16 bytes: the one-pixel path
    got = three_runs(lambda **kw: ob.terrain_uint8(x, **kw))
    want, _ = twin.terrain_u8(t)
    assert got.shape == (N, 3 * Cn, H, W) and np.array_equal(got, want)
    if N > 1:
        assert (got[1] == 127).all()
    if N > 2:
        assert (got[N - 1] == 0).all() and got[0].max() == 255 and got[0].min() == 0


@pytest.mark.parametrize("combo", (COMBOS[2], COMBOS[3]))
def test_terrain_bytes_into_an_output_off_a_four_byte_boundary(ob, combo):
    """H W % 4 == 0 and an aligned input, but `out` one byte past a 4-byte boundary: the C ABI takes the one-pixel path; the bytes before and
    after the output stay as they were"""
    from terrain_diffusion_amd._plumbing import engine_for
    N, Cn, Cc, H, W = combo
    rng = np.random.default_rng(H)
    t = (rng.standard_normal((N, Cn, H, W)) * 700.0 + 200.0).astype(F)
    x = dev(t)
    size = N * 3 * Cn * H * W
    buf = torch.full((size + 8,), 201, dtype=torch.uint8, device="cuda")
    k = 1 + (-buf.data_ptr() % 4)
    assert (buf.data_ptr() + k) % 4 == 1
    engine, _ = engine_for(x, None)
    torch.cuda.synchronize()
    with torch.cuda.device(x.device):
        rc = ob.lib().td_objective_terrain_u8(C.c_void_p(engine.stream), C.c_void_p(x.data_ptr()), N, Cn, H, W, C.c_void_p(buf.data_ptr() + k), 1)
    assert rc == 0, ob._LIB.error_text()
    got = host(buf)
    assert np.array_equal(got[k:k + size].reshape(N, 3 * Cn, H, W), twin.terrain_u8(t)[0])
    assert (got[:k] == 201).all() and (got[k + size:] == 201).all()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_the_c_abi_refuses_with_a_status(ob):
    from terrain_diffusion_amd._plumbing import engine_for
    engine, _ = engine_for(None, None)
    l, st = ob.lib(), C.c_void_p(engine.stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    z, table, img = dev(np.zeros(3, F)), dev(np.zeros((3, 6), F)), dev(np.zeros((3, 5, 4, 4), F))
    x, v, S = dev(np.zeros((3, 5, 4, 4), F)), dev(np.zeros((3, 5, 4, 4), F)), dev(np.zeros((3, 5)), torch.float64)
    l64, l32, u8 = dev(np.zeros(1), torch.float64), dev(np.zeros(1, F)), dev(np.zeros((3, 15, 4, 4), np.uint8), torch.uint8)
    hz = np.zeros(3, F)
    H_ = C.c_void_p(hz.ctypes.data)
    ch = np.array([0, 5], np.int32)
    gr = np.array([2, 2], np.int32)
    refused = {
        "host in": lambda: l.td_objective_levels(st, 0, H_, 3, 0.0, 1.0, 0.5, None, 0, 0, 0, None, 0, 0.05, P(table), 1),
        "host table": lambda: l.td_objective_levels(st, 0, P(z), 3, 0.0, 1.0, 0.5, None, 0, 0, 0, None, 0, 0.05, H_, 1),
        "N 0": lambda: l.td_objective_levels(st, 0, P(z), 0, 0.0, 1.0, 0.5, None, 0, 0, 0, None, 0, 0.05, P(table), 1),
        "channel >= C": lambda: l.td_objective_levels(st, 0, P(z), 3, 0.0, 1.0, 0.5, P(img), 5, 4, 4, C.c_void_p(ch.ctypes.data), 2, 0.05, P(table), 1),
        "H 0": lambda: l.td_objective_noise(st, P(img), P(img), None, P(table), 3, 5, 0, 0, 4, 0.5, P(x), P(v), 1),
        "C 0": lambda: l.td_objective_noise(st, P(img), P(img), None, P(table), 3, 0, 0, 4, 4, 0.5, P(x), P(v), 1),
        "host images": lambda: l.td_objective_noise(st, H_, P(img), None, P(table), 3, 5, 0, 4, 4, 0.5, P(x), P(v), 1),
        "K 1025": lambda: l.td_objective_logvar(st, P(table), 3, P(img), P(img), P(img), 1025, 1, P(z), 1),
        "K 0": lambda: l.td_objective_logvar(st, P(table), 3, P(img), P(img), P(img), 0, 1, P(z), 1),
        "n_logvar 2": lambda: l.td_objective_logvar(st, P(table), 3, P(img), P(img), P(img), 16, 2, P(z), 1),
        "W 0": lambda: l.td_objective_sqerr(st, P(x), P(v), 3, 5, 4, 0, 0.5, P(S), 1),
        "host S": lambda: l.td_objective_sqerr(st, P(x), P(v), 3, 5, 4, 4, 0.5, H_, 1),
        "groups sum": lambda: l.td_objective_loss(st, P(S), None, 3, 5, 4, 4, 0.5, 2, C.c_void_p(gr.ctypes.data), 2, P(S), P(l64), P(l32), 1),
        "no logvar": lambda: l.td_objective_loss(st, P(S), None, 3, 5, 4, 4, 0.5, 0, None, 0, P(S), P(l64), P(l32), 1),
        "host terrain": lambda: l.td_objective_terrain_u8(st, H_, 3, 5, 4, 4, P(u8), 1),
        "N 65537": lambda: l.td_objective_terrain_u8(st, P(img), 65537, 5, 4, 4, P(u8), 1),
    }
    with torch.cuda.device(0):
        for what, f in refused.items():
            rc = f()
            assert rc == -1 and ob._LIB.error_text().startswith("td_objective_"), (what, rc, ob._LIB.error_text())
    torch.cuda.synchronize()


def test_python_refuses_as_the_other_libraries_do(ob):
    table = dev(np.zeros((3, 6), F))
    big = dev(np.zeros(1025, F))
    with pytest.raises(ValueError, match="1 .. 1024"):
        ob.logvar(table, big, big, big)
    with pytest.raises(NotImplementedError, match="n_logvar"):
        ob.logvar(table, big[:8], big[:8], big[:8], n_logvar=3)
    with pytest.raises(ValueError, match="sum to C"):
        ob.v_loss(dev(np.ones((3, 5)), torch.float64), 4, 4, sigma_data=0.5, form="grouped", loss_groups=[2, 2])
    with pytest.raises(ValueError, match="outside 0 .. 4"):
        ob.noise_levels(dev(np.zeros(3, F)), sigma_data=0.5, images=dev(np.zeros((3, 5, 4, 4), F)), scale_channels=[0, 5])
    with pytest.raises(ValueError, match="empty"):
        ob.squared_error(dev(np.zeros((3, 5, 0, 4), F)), dev(np.zeros((3, 5, 0, 4), F)), sigma_data=0.5)
    with pytest.raises(ValueError, match="device tensor"):
        ob.terrain_uint8(np.zeros((1, 1, 4, 4), F))


# ------------------------------------------------------------------------------------------------------------------------------ the model
def with_head(sd, K, seed=5):
    f, p, w, wf = head(K, seed)
    sd = dict(sd)
    sd.update({"logvar_fourier.freqs": torch.from_numpy(f), "logvar_fourier.phases": torch.from_numpy(p), "logvar_linear.weight": torch.from_numpy(w)})
    return sd, (f, p, wf)


@pytest.fixture(scope="module")
def tiny():
    import terrain_diffusion_amd as td
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    sd, hd = with_head(synth_state_dict(cfg, seed=77), 130)
    models = {d: td.EDMUnet2D(**cfg, logvar_channels=130, dtype=d).load_state_dict(sd) for d in ("fp32", "bf16")}
    return cfg, sd, hd, models


def test_return_logvar_leaves_the_output_bit_for_bit(ob, tiny):
    import terrain_diffusion_amd as td
    from oracle.unet import synth_state_dict
    cfg, sd, (f, p, wf), models = tiny
    rng = np.random.default_rng(2)
    x, cond = dev(rng.standard_normal((3, 5, 16, 16)).astype(F)), dev(rng.standard_normal((3, 58)).astype(F))
    t = torch.tensor([1.2, 0.3, 0.9])
    for m in models.values():
        plain = host(m(x, t, [cond]))
        out, lv = m(x, t, [cond], return_logvar=True)
        assert same_bits(host(out), plain) and same_bits(host(m(x, t, [cond])), plain)
        assert tuple(lv.shape) == (3, 1, 1, 1) and lv.is_cuda and lv.dtype == torch.float32
        ref, E = twin.logvar64(twin.levels64(t.numpy(), "t", 1.0)["table"][:, 4], f, p, wf)
        assert within(host(lv).reshape(-1), ref, E + ulp32(ref))
    bare = td.EDMUnet2D(**cfg, dtype="fp32").load_state_dict(synth_state_dict(cfg, seed=77))
    with pytest.raises(KeyError, match="logvar"):
        bare(x, t, [cond], return_logvar=True)
    assert same_bits(host(bare(x, t, [cond])), host(models["fp32"](x, t, [cond])))
    bare.close()


def test_the_recorded_step_on_the_rebuilt_state(ob, fx, cases):
    """the state dict the reference's forward used, rebuilt as w0 / den and checked by CRC: the engine's fp32 forward gives the recorded
    model_output within the project's per-forward bound, and the recorded logvar within its bound"""
    import terrain_diffusion_amd as td
    from conftest import rel_rms
    from oracle.unet import synth_state_dict
    c = cases[0]
    sd0, sd = synth_state_dict(c["cfg"], seed=c["seed"]), {}
    for k, den, crc in zip(c["state_names"], get(fx, c, "state_den"), get(fx, c, "state_crc")):
        w0 = torch.as_tensor(sd0[k]).to(torch.float32).numpy()
        w = np.asarray(w0 / F(den), dtype=F).reshape(w0.shape)
        assert zlib.crc32(w.tobytes()) == int(crc), k
        sd[k] = torch.from_numpy(w.copy())
    sd.update({"logvar_fourier.freqs": torch.from_numpy(get(fx, c, "lv_freqs")), "logvar_fourier.phases": torch.from_numpy(get(fx, c, "lv_phases")),
               "logvar_linear.weight": torch.from_numpy(get(fx, c, "lv_weight"))})
    m = td.EDMUnet2D(**c["cfg"], logvar_channels=c["K"], dtype="fp32").load_state_dict(sd)
    out, lv = m(dev(get(fx, c, "x")), torch.from_numpy(get(fx, c, "t")), [dev(get(fx, c, "cond_inputs"))], return_logvar=True)
    e = rel_rms(host(out), get(fx, c, "model_output"))
    print(f"engine fp32 vs the recorded model_output: rel-RMS {e:.3e}")
    assert e <= B_FORWARD["fp32"]
    xlv = twin.levels64(get(fx, c, "t"), "t", 1.0)["table"][:, 4]
    _, E = twin.logvar64(xlv, get(fx, c, "lv_freqs"), get(fx, c, "lv_phases"), get(fx, c, "lv_wfold"))
    r = get(fx, c, "logvar")
    assert within(host(lv).reshape(-1), r, get(fx, c, "eref_logvar") + ulp32(r) + E)
    m.close()


# ------------------------------------------------------------------------------------------------------------------------------ end to end
def make_batches(n_batches=2, seed=21):
    rng = np.random.default_rng(seed)
    return [{"image": dev((rng.standard_normal((3, 5, 16, 16)) * 0.5).astype(F)), "cond_inputs": [dev(rng.standard_normal((3, 58)).astype(F))]} for _ in range(n_batches)]


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_validation_loss_end_to_end_against_the_oracle_loop(ob, tiny, dtype):
    from oracle.unet import OracleUnet
    cfg, sd, (f, p, wf), models = tiny
    m = models[dtype]
    sdat, P_mean, P_std, b = 0.5, -0.4, 1.0, B_FORWARD[dtype]
    batches = make_batches()
    got = ob.validation_loss(m, batches, sigma_data=sdat, P_mean=P_mean, P_std=P_std, generator=torch.Generator().manual_seed(5))
    again = ob.validation_loss(m, batches, sigma_data=sdat, P_mean=P_mean, P_std=P_std, generator=torch.Generator().manual_seed(5))
    assert got == again
    oracle = OracleUnet(cfg, {k: v for k, v in sd.items() if not k.startswith("logvar_")})
    gen = torch.Generator().manual_seed(5)
    refs, margins = [], []
    for batch in batches:
        image = host(batch["image"])
        N, Cn, H, W = image.shape
        z, noise = torch.randn(N, generator=gen), torch.randn(image.shape, generator=gen)          # the reference's order
        table = host(ob.noise_levels(z.cuda(), sigma_data=sdat, P_mean=P_mean, P_std=P_std))      # the device's own table (checked above)
        x, v = twin.add_noise32(image, noise.numpy(), table, sdat)
        with torch.no_grad():
            out = oracle(torch.from_numpy(x), torch.from_numpy(table[:, 1].copy()), [batch["cond_inputs"][0].cpu()]).numpy()
        lv, E = twin.logvar64(table[:, 4], f, p, wf)
        S = twin.sqerr64(out, v, sdat)
        _, loss = twin.loss64(S, H * W, sdat, lv, "weighted")
        refs.append(loss)
        d = twin.diff32(out, v, sdat).astype(D)
        cnt = N * Cn * H * W
        g = 2.0 * d / (cnt * np.exp(lv).reshape(-1, 1, 1, 1) * sdat)
        dn = b * float(np.sqrt((out.astype(D) ** 2).sum()))                                         # ||out - out_ref||_2 under the stated bound
        mn = S.sum(axis=1) / (Cn * H * W)
        dl = np.abs(1.0 - mn / (np.exp(lv) * sdat ** 2)) / N
        margins.append(float(np.sqrt((g ** 2).sum())) * dn + float(np.max(1.0 / (cnt * np.exp(lv)))) * dn ** 2 + float((dl * E).sum()))
    ref, margin = float(np.mean(refs)), float(np.mean(margins))
    print(f"validation_loss [{dtype}]: engine {got:.9g}, oracle loop {ref:.9g}, |difference| {abs(got - ref):.3e}, margin {margin:.3e}, ratio {abs(got - ref) / margin:.3f}")
    assert abs(got - ref) <= margin
    assert margin <= 40.0 * b * max(1.0, abs(ref))            # the margin is the bound carried, a few b of the loss's scale: not vacuous


def test_noise_loss_curve_is_the_loop_of_the_device_forms(ob, tiny):
    cfg, sd, hd, models = tiny
    m = models["fp32"]
    batches = make_batches(1)
    sig, losses = ob.noise_loss_curve(m, batches, [0.05, 2.0], sigma_data=0.5, generator=torch.Generator().manual_seed(8))
    sg, lg = ob.noise_loss_curve(m, batches, torch.tensor([0.05, 2.0]), sigma_data=0.5, loss_groups=[1, 4], generator=torch.Generator().manual_seed(8))
    assert sig.dtype == D and losses.shape == (2,) and np.array_equal(sig, np.array([0.05, 2.0], F).astype(D)) and np.array_equal(sg, sig)
    gen = torch.Generator().manual_seed(8)
    img = batches[0]["image"]
    for i, s in enumerate(sig):
        table = ob.noise_levels(torch.full((3,), float(s), device="cuda"), mode="sigma", sigma_data=0.5)
        x, v = ob.add_noise(img, torch.randn(tuple(img.shape), generator=gen).cuda(), table, sigma_data=0.5)
        S = ob.squared_error(m(x, table[:, 1].cpu(), batches[0]["cond_inputs"]), v, sigma_data=0.5)
        assert ob.v_loss(S, 16, 16, sigma_data=0.5, form="plain").value == losses[i]
        assert ob.v_loss(S, 16, 16, sigma_data=0.5, form="grouped", loss_groups=[1, 4]).value == lg[i]
    assert np.isfinite(losses).all() and losses[0] != losses[1]
