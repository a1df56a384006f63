"""The inputs of tests/_train_data_shapes.py without a GPU: the synthetic trees are taken by DeviceGroups unchanged; on every input the twin
(tests/_train_data_twin.py) and the independent references agree bit for bit -- the per-element view loop with twin.views and np.rot90 /
np.flip, the float64-and-round affine and latent arithmetic with the twin's fp32 expressions, numpy.quantile and math.fsum with the twin's
block statistics --; the exhaustive half exponential is measured against mpmath and torch's own half exp; and each wrong restatement
(shapes.VARIANTS) changes at least one designed output, every design being separated by at least one of them."""
import numpy as np
import pytest
import torch

import _train_data_shapes as sh
import _train_data_twin as twin
from terrain_diffusion_amd import train_data as td_

F, H = np.float32, np.float16
same = sh.same_values


# ------------------------------------------------------------------------------------------------------------------------------ the trees
def test_device_groups_takes_the_synthetic_trees_unchanged():
    place = td_.DeviceGroups(sh.TREE(), sh.PLACE_KEYS, sh.ALL_PLANES)
    assert place.sides == [128, 33, 256] and place.residual_sides == [1024, 40, 16] and place.latent_channels == sh.PLACE_LC
    assert any(r != 8 * s for s, r in zip(place.sides, place.residual_sides))
    partial = td_.DeviceGroups(sh.TREE(), sh.PLACE_KEYS, ("lowfreq", "residual"))
    assert partial.sides == place.sides and partial.latent_channels is None
    assert td_.DeviceGroups(sh.TREE(), sh.EXP_KEYS, ("latent",)).latent_channels == 1
    assert td_.DeviceGroups(sh.TREE(), sh.EDGE_KEYS, ("latent", "lowfreq")).sides == [sh.EDGE_S]
    assert td_.DeviceGroups(sh.TREE(), sh.DESIGN_KEYS, ("lowres_exact", "climate")).sides == [128] * 3
    for key in sh.PLACE_KEYS + sh.DESIGN_KEYS:
        c = sh.arrays(key)["climate"]
        others = [ch for ch in range(15) if ch not in sh.KEPT]
        assert c.shape[0] == 15 and (c[others] == sh.POISON).all() and not (c[list(sh.KEPT)] == sh.POISON).any()
    a = sh.arrays(sh.PLACE_KEYS[1])
    assert a["lowfreq"][7, 5] == 7 * 33 + 5 and a["residual"][7, 5] == -(7 * 40 + 5) - 1 and a["lowres_exact"][32, 32] == 32 * 33 + 32 + 0.5


# ------------------------------------------------------------------------------------------------------------------------------ 1. views
@pytest.mark.parametrize("h,w", sh.VIEW_SHAPES)
def test_the_view_loop_the_twin_and_numpy_agree_on_overhanging_rectangles(h, w):
    seen = set()
    for plane in sh.VIEW_PLANES:
        for origin in (0, 1):
            it = sh.view_items(h, w, plane, origin)
            ref = sh.views_ref(plane, it, origin, h, w)
            assert ref.shape == (len(it), h, w) and {int(t) for t in it[:, 3]} == set(range(8)) and {int(g) for g in it[:, 0]} == {0, 1, 2}
            for n, (g, i, j, t, li, lj) in enumerate(it.tolist()):
                a = sh.arrays(sh.PLACE_KEYS[g])[plane]
                r0, c0 = (np.array((i, j) if origin else (li, lj)) + sh.VIEW_OFFSETS[origin]).tolist()
                assert same(ref[n], twin.views(a, r0, c0, h, w, t)), (plane, origin, n)
                hh, ww = (w, h) if t % 2 else (h, w)
                win = twin.window(a, r0, c0, hh, ww)
                assert same(ref[n], np.ascontiguousarray(np.rot90(np.flip(win, -1) if t // 4 else win, t % 4))), (plane, origin, n)
                nan = np.isnan(ref[n])
                seen.add((t, "outside" if nan.all() else "inside" if not nan.any() else "partial"))
    kinds = {"outside", "inside"} | ({"partial"} if h * w > 1 else set())
    assert seen == {(t, k) for t in range(8) for k in kinds}, sorted(seen)


def test_the_affine_reference_equals_the_twin_on_the_edge_operands():
    results = {}
    for abc in sh.AFFINE_ABC:
        with np.errstate(all="ignore"):
            want, tw = sh.affine_ref(sh.AFFINE_X, *abc), twin.affine(sh.AFFINE_X, *abc)
        assert same(want, tw), abc
        results[abc] = want
    tiny = float(np.finfo(F).tiny)
    flat = np.concatenate(list(results.values()))
    assert ((flat != 0) & (np.abs(flat) < tiny)).sum() >= 2                                  # denormal quotients, kept and halved
    x_is_a = int(np.flatnonzero(sh.AFFINE_X == F(1.25))[0])
    assert results[sh.AFFINE_ABC[0]][x_is_a] == 0 and not np.signbit(results[sh.AFFINE_ABC[0]][x_is_a])
    assert results[sh.AFFINE_ABC[1]][x_is_a] == 0 and np.signbit(results[sh.AFFINE_ABC[1]][x_is_a])   # 0 / -3 = -0
    finite_in = np.isfinite(sh.AFFINE_X)
    assert np.isinf(results[sh.AFFINE_ABC[4]][finite_in]).any() and np.isinf(results[sh.AFFINE_ABC[5]][finite_in]).any()   # overflow
    assert all(np.isnan(r[np.isnan(sh.AFFINE_X)]).all() and np.isinf(r[np.isinf(sh.AFFINE_X)]).all() for k, r in results.items() if k[1] != 0.0)


# ------------------------------------------------------------------------------------------------------------------------------ 2. latents
def test_the_half_exponential_over_all_65536_inputs_against_mpmath_and_torch():
    """The measured counts (also in DESIGN.md): of the 63488 finite logvars 891 give a subnormal half, 11178 give 0 and 11892 give inf; the
    library's float64 -> fp32 -> half rounding differs from ONE rounding of the exact exponential on 2 inputs (hv = 0.007298 and 0.02269, one
    half ulp each); torch's CPU half exp, which the reference runs, equals the twin on all 65536; the exact exponential stays 2^-49.0 relative
    (1.776e-15, eight float64 ulps or more) away from every fp32 rounding midpoint, asserted as 2^-50, so a device exp within four float64
    ulps cannot differ from NumPy's."""
    table = sh.exp_table()
    assert all(np.array_equal(np.sort(t.reshape(-1).view(np.uint16)), np.arange(65536, dtype=np.uint16)) for t in table)
    assert len({t.tobytes() for t in table}) == 8
    v = table[0].reshape(-1)
    with np.errstate(all="ignore"):
        hv = (v.astype(F) * F(0.5)).astype(H)
        e = twin.half_std(v)
    finite = np.isfinite(v)
    ef = e[finite]
    counts = (int(finite.sum()), int(((ef != 0) & (ef < H(2.0 ** -14))).sum()), int((ef == 0).sum()), int(np.isinf(ef).sum()))
    single = sh.single_rounded_half(hv)
    ok = np.isfinite(hv)
    want = np.array([single[int(b)] for b in hv[ok].view(np.uint16)], np.uint16)
    double_rounded = int((e[ok].view(np.uint16) != want).sum())
    with torch.no_grad():
        te = torch.exp(torch.from_numpy(v.copy()) * 0.5).numpy()
    torch_differs = int((~((te.view(np.uint16) == e.view(np.uint16)) | (np.isnan(te) & np.isnan(e)))).sum())
    away = sh.fp32_midpoint_distance(hv)
    print(f"\nfinite, subnormal, zero, inf = {counts}; double vs single rounding: {double_rounded}; torch half exp vs twin: {torch_differs}; "
          f"exact exp from an fp32 midpoint: 2^{np.log2(away):.1f}")
    assert np.isnan(e[np.isnan(v)]).all() and e[v == H(np.inf)] == H(np.inf) and e[v == H(-np.inf)] == 0
    assert counts == (63488, 891, 11178, 11892) and double_rounded == 2 and torch_differs == 0 and away >= 2.0 ** -50


def edge_draws(mode, variant=None):
    lat = sh.arrays(sh.EDGE_KEYS[0])["latent"]
    kw = dict(mean=sh.EDGE_MEAN, std=sh.EDGE_STD, sigma_data=sh.EDGE_SIGMA) if mode == 0 else {}
    with np.errstate(all="ignore"):
        ref = sh.latent_draw_ref(lat[0, :2], lat[0, 2:], sh.edge_noise(mode)[0], mode, variant=variant, **kw)
        tw = sh.twin_draw(lat[0, :2], lat[0, 2:], sh.edge_noise(mode)[0], mode, **kw)
    return ref, tw


def test_the_latent_edges_give_what_they_were_placed_for():
    r0, t0 = edge_draws(0)
    r1, t1 = edge_draws(1)
    assert same(r0, t0) and same(r1, t1)
    a, b = r0.reshape(2, 16), r1.reshape(2, 16)
    tiny = float(np.finfo(F).tiny)
    assert np.isnan(a[:, 0]).all() and 0 < a[0, 1] < tiny and a[0, 2] == np.inf and a[0, 3] == -np.inf and np.isnan(a[:, 10]).all()
    assert np.isfinite(a[0, 14]) and np.isinf(a[1, 14])                                       # the tiny std overflows the quotient
    assert np.isnan(b[0, 0]) and b[0, 4] == 1 and b[0, 5] == H(1 + 2.0 ** -9) and b[0, 8] == 1          # ties to even
    assert b[0, 6] == np.inf and 0 < b[0, 7] < H(2.0 ** -14) and b[0, 9] == np.inf and b[0, 11] == 0 and np.signbit(b[0, 11])
    assert b[0, 1] == H(2.0 ** -24) and np.isnan(b[0, 12]) and np.isnan(b[0, 13])


@pytest.mark.parametrize("h,w", sh.RECT_SHAPES)
def test_rectangular_latent_windows_leave_the_latent_on_every_side(h, w):
    items = sh.rect_items(h, w)
    kinds = set()
    for mode in (0, 1):
        noise = sh.rect_noise(h, w, mode)
        kw = dict(mean=sh.RECT_MEAN, std=sh.RECT_STD, sigma_data=sh.RECT_SIGMA) if mode == 0 else {}
        for n, (g, i, j, t, _, _) in enumerate(items.tolist()):
            lat, S = sh.arrays(sh.PLACE_KEYS[g])["latent"], sh.PLACE[g][1]
            a = sh.latents_window(lat, t, i, j, h, w, noise[n], mode, sh.latent_draw_ref, **kw)
            b = sh.latents_window(lat, t, i, j, h, w, noise[n], mode, sh.twin_draw, **kw)
            assert same(a, b) and a.shape == ((sh.PLACE_LC, 8 * h, 8 * w) if mode else (sh.PLACE_LC, h, w)), (mode, n)
            rr, cc = np.meshgrid(np.arange(i, i + h), np.arange(j, j + w), indexing="ij")
            out = (rr < 0) | (rr >= S) | (cc < 0) | (cc >= S)
            kinds.add("outside" if out.all() else "inside" if not out.any() else "partial")
            cell = a.reshape(sh.PLACE_LC, h, 8, w, 8)[:, :, 0, :, 0] if mode else a
            assert (cell[:, out] == 0).all() and not np.signbit(cell[:, out]).any() and (cell[:, ~out] != 0).all(), (mode, n)
    assert kinds == {"outside", "inside", "partial"} and (items[:, 1:3] < 0).any()


# ------------------------------------------------------------------------------------------------------------------------------ 3. cond image
def slot_of(name, plane):
    return [s for s, d in enumerate(sh.DESIGN_LAYOUT[plane]) if d == name]


def test_the_designed_blocks_give_what_they_were_designed_for():
    grids = [np.stack(sh.design_grids(n)) for n in range(3)]
    cell = lambda n, name, ch: grids[n][ch].reshape(-1)[slot_of(name, n)[0]]
    for name in ("zeros_mp", "zeros_pm", "zeros_mm"):                                        # +0 whatever the signs and the placement
        assert cell(0, name, 1) == 0 and not np.signbit(cell(0, name, 1)), name
    s = np.sort(sh.design_block(0, slot_of("copies52", 0)[0]))
    assert s[51] == F(-3.5) and s[52] > 1 and cell(0, "copies52", 1) > F(-3.5) and cell(0, "copies53", 1) == F(-3.5) == cell(0, "copies54", 1)
    assert cell(0, "copies51", 1) > 1 and cell(0, "equal", 1) == F(7.25) == cell(0, "equal", 0)
    assert cell(0, "sign_change", 1) == F(F(-0.5) + F(F(0.75) * F(F(1023) * F(0.05) - F(51))))
    tiny = float(np.finfo(F).tiny)
    assert 0 < abs(cell(0, "denormal_signs", 1)) < tiny and 0 < cell(0, "denormal_gap", 1) < tiny
    assert np.isnan(cell(1, "ninf53", 1)) and cell(1, "ninf53", 0) == -np.inf and np.isnan(cell(1, "ninf52", 1)) and cell(1, "ninf52", 0) == -np.inf
    assert np.isfinite(cell(1, "pinf_top", 1)) and cell(1, "pinf_top", 0) == np.inf
    assert cell(1, "big_diff", 1) == np.inf and np.isfinite(cell(1, "big_diff", 0))
    perm = {cell(1, name, ch).tobytes() for name in ("ascending", "descending", "last_slot") for ch in (1,)}
    assert len(perm) == 1 and len({cell(1, name, 0).tobytes() for name in ("ascending", "descending", "last_slot")}) == 1
    b = sh.design_block(1, slot_of("last_slot", 1)[0])
    assert b[1023] == np.sort(b)[51]
    for k in (0, 255, 256, 1023):
        slot = slot_of(f"nan{k}", 2)[0]
        assert np.isnan(sh.design_block(2, slot)[k]) and np.isnan(sh.design_block(2, slot)).sum() == 1
        by, bx = divmod(slot, 4)
        for ny, nx in ((by - 1, bx), (by + 1, bx), (by, bx - 1), (by, bx + 1)):
            if 0 <= ny < 4 and 0 <= nx < 4:
                assert np.isfinite(grids[2][:2, ny, nx]).all(), (k, ny, nx)
    assert np.isnan(grids[2][0]).sum() == 4 and np.isnan(grids[2][2:]).sum() == 1           # one climate block of one channel holds a NaN
    for n in range(3):                                                                      # low and top byte: the degenerate passes
        for name in ("low_byte", "top_byte"):
            for slot in slot_of(name, n):
                k = sh.keys_of(sh.design_block(n, slot))
                varying = [shift for shift in (24, 16, 8, 0) if np.unique((k >> np.uint32(shift)) & np.uint32(255)).size > 1]
                assert varying == ([0] if name == "low_byte" else [24]), (name, varying)


@pytest.mark.parametrize("n", range(len(sh.DESIGN_LAYOUT)))
def test_numpy_quantile_math_fsum_the_restated_select_and_the_twin_agree_on_every_design(n):
    a = sh.arrays(sh.DESIGN_KEYS[n])
    assert same(sh.design_grids(n, "as_the_kernel")[1], sh.design_grids(n)[1])               # the select restated for the variants == numpy.quantile
    outputs = set()
    for t in range(8):
        want = sh.design_raw_ref(n, t)
        with np.errstate(all="ignore"):
            raw = twin.cond_image(a["lowres_exact"], a["climate"], 32, 32, 64, t, raw=True)
            norm = twin.cond_image(a["lowres_exact"], a["climate"], 32, 32, 64, t, norm_mean=sh.NORM_MEAN, norm_std=sh.NORM_STD)
        assert same(want, raw), (t, sh.first_difference(want, raw))
        assert same(sh.normalise_ref(want), norm), (t, sh.first_difference(sh.normalise_ref(want), norm))
        outputs.add(want.tobytes())
    assert len(outputs) == 8                                                                # the output cell moves with the transform
    if n == 1:
        norm = sh.normalise_ref(sh.design_raw_ref(1, 0))
        big = slot_of("big_diff", 1)[0]
        fmax = np.finfo(F).max
        assert norm[1].reshape(-1)[big] == F((np.float64(fmax) - np.float64(F(sh.NORM_MEAN[1]))) / np.float64(F(sh.NORM_STD[1])))
        assert norm[1].reshape(-1)[slot_of("ninf53", 1)[0]] == 0 and norm[6].reshape(-1)[slot_of("ninf53", 1)[0]] > 0


@pytest.mark.parametrize("crop", sorted(sh.CROPS))
def test_other_crops_and_the_draw_edges(crop):
    g = (crop + 64) // 32
    raw = sh.crop_twin(crop, draws=False, raw=True)
    assert raw.shape == (3, 7, g, g) and same(raw, sh.crop_raw_ref(crop)), sh.first_difference(raw, sh.crop_raw_ref(crop))
    nan_share = np.isnan(raw[:, 0]).reshape(3, -1).mean(1)
    assert nan_share[0] == 0 and (0 < nan_share[1:]).all() and (nan_share[1:] < 1).all()     # one item inside, the others partly off the plane
    full = sh.crop_twin(crop, raw=True)
    d = sh.crop_draws(crop)
    whole = ~np.isnan(raw[:, 0])
    assert whole[0, 1, 1] and whole[0, 1, 2] and whole[0, 2, 1]
    assert np.isnan(full[0, 0, 1, 1]) and full[0, 6, 1, 1] == 0                              # u_drop == p drops: the comparison is a strict >
    assert not np.isnan(full[0, 0, 1, 2]) and full[0, 6, 1, 2] == 1                          # the fp32 number above p keeps
    assert np.isnan(full[0, 0, 2, 1]) and full[0, 6, 2, 1] == 0                              # a NaN uniform drops
    kept = whole[0] & (full[0, 6] == 1)
    assert d["u_noise"][0] == 0 and same(full[0, :2][:, kept], raw[0, :2][:, kept])          # u_noise = 0 adds +-0
    assert not same(full[1, 0][full[1, 6] == 1], raw[1, 0][full[1, 6] == 1])
    assert not same(sh.crop_twin(crop, raw=True, variant="dropout_ge"), full)
    std = list(sh.NORM_STD)
    std[3] = np.nan
    out = sh.crop_twin(crop, norm_std=std)
    assert np.isnan(out[:, 3]).all() and not np.isnan(out[:, [0, 1, 6]]).any()


# ------------------------------------------------------------------------------------------------------------------------------ cond vector
@pytest.mark.parametrize("g", sh.VECTOR_GS)
def test_the_cond_vector_reference_equals_the_twin_and_finds_the_centre(g):
    d = sh.vector_inputs(g)
    f = twin.mp_factors()
    assert np.unique(sh.vector_inputs(g)["img"][0]).size == 7 * g * g and sh.VECTOR_N * td_.COND_LEN > 256
    for n in range(sh.VECTOR_N):
        for z in (None, d["z_replace"][n]):
            want, flags = sh.cond_vector_ref(d["img"][n], d["hist"][n], d["noise_level"][n], z)
            tw, tf = twin.cond_vector(d["img"][n], d["hist"][n], d["noise_level"][n], z)
            assert same(want, tw) and np.array_equal(flags, tf), (n, z is None)
        assert flags.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0]][n], n
        if n == 1:
            assert (want[32:36] == F(F(0.25) * f[2])).all()                                  # only ((x00 + x01) + x10) + x11 gives 1
        if n == 0:
            c = g // 2
            assert want[0] == F(F(10 * (c - 2) + (c - 2)) * f[0]) and want[31] == F(F(1000 + 10 * (c + 1) + (c + 1)) * f[1])
        if n == 4:
            assert np.isnan(want[32:36]).sum() == 0 and np.isnan(want[:16]).sum() == 0 and np.isnan(sh.vector_inputs(g)["img"][4]).sum() == 1


# ------------------------------------------------------------------------------------------------------------------------------ 4. the inputs decide
def separated(variant):
    """the designed outputs the wrong variant changes"""
    out = []
    if variant in ("ranks_50_51", "ranks_52_53", "k1_min_gt", "k1_prefix", "unsigned_keys", "nan_wave0_only", "nan_first_value_only", "fp32_sum"):
        for n in range(3):
            good, bad = np.stack(sh.design_grids(n)).reshape(6, 16), np.stack(sh.design_grids(n, variant)).reshape(6, 16)
            chans = (0,) if variant == "fp32_sum" else (1,)
            out += [sh.DESIGN_LAYOUT[n][s] for s in range(16) if not same(good[chans, s], bad[chans, s])]
            if variant == "fp32_sum":
                out += ["climate"] * int(sum(not same(good[2:, s], bad[2:, s]) for s in range(16)))
    elif variant == "halo31":
        for n in range(3):
            a = sh.arrays(sh.DESIGN_KEYS[n])
            with np.errstate(all="ignore"):
                bad = twin.cond_image(a["lowres_exact"], a["climate"], 32, 32, 64, 0, raw=True, variant="halo31")
            out += [sh.DESIGN_LAYOUT[n][s] for s in range(16) if not same(bad.reshape(7, 16)[:, s], sh.design_raw_ref(n, 0).reshape(7, 16)[:, s])]
    elif variant in ("residual_side_as_side", "no_swap"):
        for h, w in sh.VIEW_SHAPES:
            it = sh.view_items(h, w, "residual", 0)
            good, bad = sh.views_ref("residual", it, 0, h, w), sh.views_ref("residual", it, 0, h, w, variant=variant)
            out += [(h, w, n) for n in range(len(it)) if not same(good[n], bad[n])]
    elif variant == "half_truncates":
        good, bad = edge_draws(1)[0].reshape(2, 16), edge_draws(1, variant)[0].reshape(2, 16)
        out += [k for k in range(16) if not same(good[:, k], bad[:, k])]
        assert 5 in out and 4 not in out                     # 1 + 2^-10 + 2^-11 needs the tie to go up; 1 + 2^-11 truncates to the same 1
    elif variant == "c0_up":
        for g in sh.VECTOR_GS:
            d = sh.vector_inputs(g)
            diff = [not same(sh.cond_vector_ref(d["img"][n], d["hist"][n], d["noise_level"][n])[0],
                             sh.cond_vector_ref(d["img"][n], d["hist"][n], d["noise_level"][n], variant=variant)[0]) for n in range(sh.VECTOR_N)]
            assert all(diff) if g % 2 else not any(diff), g  # only an odd g tells the two roundings apart
            out += [g] * any(diff)
    else:
        raise AssertionError(variant)
    return out


@pytest.mark.parametrize("variant", sh.VARIANTS)
def test_a_wrong_variant_changes_a_designed_output(variant):
    out = separated(variant)
    print(f"\n{variant}: changes {len(out)} designed outputs: {sorted(set(map(str, out)))[:24]}")
    assert out, variant
    if variant == "no_swap":
        assert not any(h == w for h, w, _ in out) and {(h, w) for h, w, _ in out} == {s for s in sh.VIEW_SHAPES if s[0] != s[1]}
    if variant == "residual_side_as_side":
        it = sh.view_items(5, 9, "residual", 0)
        assert {int(it[n, 0]) for h, w, n in out if (h, w) == (5, 9)} == {0, 1, 2}           # R = 1024, 40 and 16 beside S = 128, 33 and 256
    if variant == "k1_min_gt":
        assert {"copies53", "copies54", "equal"} <= set(out) and "copies52" not in out
    if variant == "k1_prefix":
        assert {"copies51", "copies52"} <= set(out) and "copies53" not in out
    if variant == "nan_wave0_only":
        assert set(out) == {"nan255", "nan1023"}
    if variant == "nan_first_value_only":
        assert set(out) == {"nan256", "nan1023"}
    if variant == "fp32_sum":
        assert "cancel" in out and out.count("climate") == 48


def test_no_design_is_dead_weight():
    """every design but the filler is changed by at least one wrong variant; nan0, which every NaN-blind variant still sees, is their control"""
    hit = set()
    for variant in sh.VARIANTS[:9]:
        hit |= {d for d in separated(variant) if isinstance(d, str)}
    names = {d for layout in sh.DESIGN_LAYOUT for d in layout}
    assert names - hit - {"nan0"} == set(), sorted(names - hit)
