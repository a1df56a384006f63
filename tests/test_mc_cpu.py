"""Minecraft terrain, host side (no GPU): the NumPy twin (tests/_mc_twin.py) against every case recorded from the reference's own
minecraft_api.py and api.py (tests/golden/mc.npz, tests/golden/make_mc_golden.py), the fixtures' coverage of the classifier's ids, the payload's
byte layout and round trip, and the refusals that come before any launch."""
import json

import numpy as np
import pytest

import _mc_twin as twin

F = np.float32


def cases(golden):
    g = golden("mc")
    for c in json.loads(str(g["cases"])):
        n = c["name"]
        wins = []
        for k in range(len(c["gets"])):
            cl = f"win{k}_climate_{n}"
            wins.append((g[f"win{k}_elev_{n}"], g[cl] if cl in g.files else None))
        yield c, wins, g


def ulps_of(scale):
    return np.spacing(np.asarray(scale, F)).astype(np.float64)


def upsample_close(got, want, native, s, r0, c0):
    """|got - want| <= 2 ulp of the largest native sample each pixel interpolates."""
    H, W = got.shape[-2:]
    tol = 2 * ulps_of(twin.upsample_scale(native, s, r0, c0, H, W))
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return bool(np.all((d <= tol) | (np.isnan(got) & np.isnan(want)))), tol


def check_case(c, wins, g, elev, biome, smooth=None, padded=None, climate=None, payload=None):
    """The bounds of the recorded-case comparison (shared with the GPU test): upsampled fields to 2 ulp of their native samples, elev to 1e-3 m
    except where the land mask may flip, payload int16 except within 1e-3 of an integer, biome ids wherever the twin's margin exceeds 4 ulp.
    Returns the number of margin-exempt pixels."""
    n, s, (i1, j1, i2, j2) = c["name"], c["scale"], c["box"]
    H, W = i2 - i1, j2 - j1
    planes = g["noise_" + n]
    nan_case = c["kind"] == "nan"
    tol_smooth = np.zeros((H, W))
    if s > 1:
        r0, c0 = twin.crop_origin(i1, j1, s, 2)
        en, cn = wins[0]
        ok, tol_pad = upsample_close(padded, g["elev_padded_" + n], en, s, r0 - 1, c0 - 1)
        assert ok or nan_case, n
        tol_smooth = tol_pad[1:-1, 1:-1]
        assert np.array_equal(smooth, padded[1:-1, 1:-1], equal_nan=True), n
        if cn is not None:
            ok, _ = upsample_close(climate, g["climate_" + n], cn, s, r0, c0)
            assert ok or nan_case, n
        grad = twin.gradient(padded)
        base = smooth
        clim = climate
    else:
        (pad, _), (base, clim) = wins
        grad = twin.gradient(pad)
        assert np.array_equal(elev, g["elev_" + n], equal_nan=True), n
    if not nan_case:
        want = g["elev_" + n]
        d = np.abs(elev.astype(np.float64) - want.astype(np.float64))
        flip = np.abs(g["elev_smooth_" + n].astype(np.float64)) <= 2 * tol_smooth if s > 1 else np.zeros((H, W), bool)
        assert np.all((d <= 1e-3) | flip), (n, float(d.max()))
        if payload is not None:
            got16 = np.frombuffer(payload, "<i2")[:H * W].reshape(H, W)
            want16 = g["payload_" + n].view("<i2")[:H * W].reshape(H, W)
            near = np.abs(elev - np.round(elev)) <= 1e-3
            assert np.all((got16 == want16) | near | flip), n
    pix = c["native_resolution"] / s
    m = twin.margin(base, clim, grad, pix, planes)
    want_b = g["biome_" + n]
    exempt = int((m <= 4).sum())
    assert np.array_equal(biome[m > 4], want_b[m > 4]), (n, int((biome != want_b).sum()))
    if payload is not None:
        assert payload[2 * H * W:] == want_b.astype("<i2").tobytes() or exempt, n
    return exempt


def test_twin_matches_every_recorded_case(golden):
    seen, exempt = {"mc": 0, "api": 0}, 0
    for c, wins, g in cases(golden):
        n, s, (i1, j1, i2, j2) = c["name"], c["scale"], c["box"]
        H, W = i2 - i1, j2 - j1
        nr = c["native_resolution"]
        planes = g["noise_" + n]
        assert planes.shape == (7, H, W) and np.array_equal(planes, twin.noise_planes(i1, j1, H, W)), n
        if c["fn"] == "api":
            assert c["gets"] == [[*twin.native_box(i1, j1, i2, j2, s, 1 if s > 1 else 0), True]], n
            en, cn = wins[0]
            if s == 1:
                got = {"elev": en, "climate": cn}
            else:
                got = twin.get_terrain(en, cn, i1, j1, i2, j2, s)
            r0, c0 = twin.crop_origin(i1, j1, s, 1) if s > 1 else (0, 0)
            assert upsample_close(got["elev"], g["elev_" + n], en, s, r0, c0)[0], n
            assert (got["climate"] is None) == (f"climate_{n}" not in g.files), n
            if got["climate"] is not None:
                assert upsample_close(got["climate"], g["climate_" + n], cn, s, r0, c0)[0], n
        elif s == 1:
            assert c["gets"] == [[i1 - 1, j1 - 1, i2 + 1, j2 + 1, False], [i1, j1, i2, j2, True]], n
            elev, biome = twin.minecraft_terrain(wins, i1, j1, i2, j2, s, c["noise"], nr, planes)
            exempt += check_case(c, wins, g, elev, biome, payload=twin.payload(elev, biome))
        else:
            assert c["gets"] == [[*twin.native_box(i1, j1, i2, j2, s, 2), True]], n
            en, cn = wins[0]
            up = twin.get_upsampled(en, cn, i1, j1, i2, j2, s, c["noise"], nr / s, nr, planes)
            _, biome = twin.minecraft_terrain(wins, i1, j1, i2, j2, s, c["noise"], nr, planes)
            exempt += check_case(c, wins, g, up["elev"], biome, up["elev_smooth"], up["elev_padded"], up["climate"],
                                 twin.payload(up["elev"], biome))
        seen[c["fn"]] += 1
    print(f"margin-exempt pixels over all recorded cases: {exempt}")
    assert seen == {"mc": 24, "api": 6}


def test_recorded_cases_cover_every_biome_id_and_the_edges(golden):
    g = golden("mc")
    cs = {c["name"]: c for c in json.loads(str(g["cases"]))}
    ids = set()
    for n, c in cs.items():
        if c["fn"] == "mc":
            ids |= {int(v) for v in np.unique(g["biome_" + n])}
    assert ids == set(twin.BIOME_IDS)
    assert {c["scale"] for c in cs.values() if c["fn"] == "mc"} == {1, 2, 3, 4, 8}
    assert {c["noise"] for c in cs.values() if c["scale"] in (2, 4, 8)} >= {0.0, 1.0, 2.5}
    assert any(c["box"][0] < 0 and c["box"][0] % c["scale"] for c in cs.values())         # negative, scale-misaligned origins
    assert {(c["box"][2] - c["box"][0], c["box"][3] - c["box"][1]) for c in cs.values()} >= {(1, 9), (9, 1), (7, 5)}
    assert np.all(g["biome_clim_none"] == 1) and np.all(g["biome_clim3"] == 1) and np.all(g["biome_clim3_x1"] == 1)
    assert np.all(g["win0_elev_ocean"] < 0) and set(np.unique(g["biome_ocean"])) <= {41, 44, 46, 48}
    assert np.isnan(g["elev_nan_x1"]).any() and np.isnan(g["elev_nan_x2"]).any()
    assert not np.array_equal(g["elev_x2_n10"], g["elev_x2_n00"]) and not np.array_equal(g["elev_x2_n25"], g["elev_x2_n10"])
    assert str(g["torch_version"]) and str(g["numpy_version"]).split(".")[0] == "2"


def test_payload_layout_and_round_trip():
    from terrain_diffusion_amd.minecraft import parse_minecraft_payload
    elev = np.array([[-0.5, 0.0, 1.999], [40000.0, -40000.0, -32768.5]], F)
    biome = np.array([[1, 48, 116], [3, 5, 6]], np.int16)
    body = twin.payload(elev, biome)
    assert len(body) == 2 * 2 * 6
    assert np.frombuffer(body[:12], "<i2").tolist() == [-1, 0, 1, 32767, -32768, -32768]
    assert np.frombuffer(body[12:], "<i2").tolist() == biome.ravel().tolist()
    e16, b16 = parse_minecraft_payload(body, {"X-Height": "2", "X-Width": "3", "X-Dtype": "int16-le"})
    assert e16.dtype == np.int16 and e16.tolist() == [[-1, 0, 1], [32767, -32768, -32768]] and np.array_equal(b16, biome)
    e16, b16 = parse_minecraft_payload(body[:12], {"X-Height": "2", "X-Width": "3", "X-Dtype": "int16-le"})
    assert b16 is None and e16.shape == (2, 3)
    with pytest.raises(ValueError):
        parse_minecraft_payload(body[:10], {"X-Height": "2", "X-Width": "3", "X-Dtype": "int16-le"})
    with pytest.raises(ValueError):
        parse_minecraft_payload(body, {"X-Height": "2", "X-Width": "3", "X-Dtype": "float32"})


class _NoWorld:
    native_resolution = 90.0

    def get(self, *a, **k):
        raise AssertionError("world.get must not be called for a refused request")


def test_refusals_before_any_launch():
    from terrain_diffusion_amd import minecraft as mc
    w = _NoWorld()
    for fn in (lambda: mc.minecraft_terrain(w, 0, 0, 8, 8, scale=0), lambda: mc.get_upsampled(w, 0, 0, 8, 8, 0),
               lambda: mc.get_terrain(w, 0, 0, 8, 8, -2), lambda: mc.minecraft_terrain(w, 5, 0, 5, 8, scale=2),
               lambda: mc.get_upsampled(w, 0, 8, 8, 3, 4), lambda: mc.get_terrain(w, 3, 3, 2, 9, 2),
               lambda: mc.minecraft_terrain(w, 0, 0, 1 << 14, 1 << 14, scale=4), lambda: mc.minecraft_terrain(w, 0, 0, 8, 8, scale=2.5)):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):   # climate that does not match the elevation
        mc.classify_biome(np.zeros((4, 5), F), np.zeros((5, 4, 6), F), 0, 0, np.zeros((6, 7), F))
    with pytest.raises(ValueError):   # elev_padded must be (H + 2, W + 2)
        mc.classify_biome(np.zeros((4, 5), F), np.zeros((5, 4, 5), F), 0, 0, np.zeros((6, 6), F))
    with pytest.raises(ValueError):
        mc.minecraft_payload(np.zeros((4, 5), F), np.zeros((4, 6), np.int16))
    assert mc.MAX_PIXELS == 1 << 26 and set(mc.EXPORTS) == {"td_mc_last_error", "td_mc_upsample", "td_mc_finish", "td_mc_noise", "td_mc_payload"}
    assert mc.NOISE_NAMES == twin.NAMES
