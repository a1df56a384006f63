"""Hydrology on structured terrain, host side (no GPU): the NumPy twin against every case the reference's postprocessing.py gave on the
closed-form terrains of tests/_hydro_shapes.py (tests/golden/hydro_structured.npz, tests/golden/make_hydro_structured_golden.py), and the
conditions that make those terrains worth running on the GPU -- tied slopes, chain length, fan-in, fill depth -- checked on the inputs and
the recorded results alone.

Ties: `more than half of the land cells attain their largest prefer slope at two or more k` holds on steps (0.669 with the default tol,
0.982 with tol = 0.5), checkerboard and flat (1.0 each).  It cannot hold on the other five surfaces, whatever the kernel does: in the open
quadrants of pit_l1 the diagonal slope 2 / sqrt 2 beats both cardinal slopes of 1, in the wedges of pit_linf and peak_linf_sea the one
cardinal slope of 1 beats the two diagonal ones of 1 / sqrt 2, and on plane NW (3 / sqrt 2) beats W (2).  Measured: pit_l1, pit_linf and
plane 0.001 (one cell), saddle 0.087, peak_linf_sea 0.184 (the cells beside the sea ring, +inf at three or more k).  Those five are kept
for what they do give -- a maximum on a diagonal, whose slope is the one divided by fl32(sqrt 2), eight donors at one cell, +inf ties on a
coast -- and each of those is asserted below instead."""
import json

import numpy as np
import pytest

import _hydro_shapes as shapes
import _hydro_twin as twin

N_TIE = 33
MOSTLY_TIED = ("steps", "checkerboard", "flat")


def _cases(golden):
    g = golden("hydro_structured")
    for c in json.loads(str(g["cases"])):
        yield c["name"], c["fn"], g[c["input"]], c["kwargs"], g


@pytest.fixture(scope="module")
def twin_fills(golden):
    """(filled, Jacobi iterations) of the twin for every recorded fill case, computed once."""
    return {name: twin.fill(z, **kw) for name, fn, z, kw, _ in _cases(golden) if fn == "fill"}


def test_inputs_are_what_the_generators_give(golden):
    g = golden("hydro_structured")
    assert str(g["numpy_version"]).split(".")[0] == "2"                      # NEP 50: fl32(tol), fl32(eps)
    want = {"serp64": shapes.serpentine(64, 64), "serp64x65": shapes.serpentine(64, 65), "serp65x64": shapes.serpentine(65, 64),
            "serp130": shapes.serpentine(130, 130), "pit_linf257": shapes.pit_linf(257), "comb": shapes.comb(),
            "ramp64": shapes.ramp_serpentine(64, 64), "ramp130": shapes.ramp_serpentine(130, 130), "serp64_filled": g["out_fill_serp64"]}
    want.update({f"{n}{N_TIE}": make(N_TIE) for n, make in shapes.TIE_SURFACES.items()})
    assert {k[3:] for k in g.files if k.startswith("in_")} == set(want)
    for k, z in want.items():
        assert g["in_" + k].dtype == np.float32 and np.array_equal(g["in_" + k], z), k


def test_serpentine_is_one_closed_channel():
    for H, W in ((64, 64), (64, 65), (65, 64), (130, 130)):
        z = shapes.serpentine(H, W)
        r, c = shapes.serpentine_path(H, W)
        assert len(r) == len(set(zip(r.tolist(), c.tolist()))) == int((z == 1).sum())                     # the path is the floor, each cell once
        assert (np.abs(np.diff(r)) + np.abs(np.diff(c)) == 1).all() and (r[0], c[0]) == (1, 1)             # 4-connected, from the outlet's side
        assert z[1, 0] == 10 and (np.delete(np.concatenate([z[0], z[-1], z[:, 0], z[:, -1]]), 2 * W + 1) == 1000).all()   # walled in but for the outlet
        assert len(r) >= (H // 2 - 1) * (W - 2)


def test_twin_matches_every_recorded_case(golden, twin_fills):
    seen = {"fill": 0, "d8": 0, "acc": 0, "indicator": 0}
    for name, fn, z, kw, g in _cases(golden):
        if fn == "fill":
            got, _ = twin_fills[name]
            assert got.dtype == np.float32 and np.array_equal(got, g["out_" + name], equal_nan=True), name
            assert twin.fill_fixed_point_violations(z, g["out_" + name], **kw) == 0, name
        elif fn == "d8":
            r, k, s = twin.d8(z, **kw)
            assert np.array_equal(r, g["receiver_" + name]) and np.array_equal(k, g["kmax_" + name]) and np.array_equal(s, g["sink_" + name]), name
        elif fn == "acc":
            r, _, s = twin.d8(z, **kw)                                          # an acc case's kwargs are its d8's
            assert twin.uphill_edges(z, r, s) == 0, name
            assert np.array_equal(twin.accumulate(z, r, s), g["out_" + name]), name
            assert twin.accumulation_ok(z, r, s, g["out_" + name]), name
        else:
            r, _, s = twin.d8(z)
            assert np.array_equal(twin.indicator(twin.accumulate(z, r, s), kw.get("max_pool_kernel", 1)), g["out_" + name]), name
        seen[fn] += 1
    assert seen == {"fill": 8, "d8": 14, "acc": 14, "indicator": 2}


def test_tied_slopes(golden):
    g = golden("hydro_structured")
    frac = {n: shapes.tie_fraction(g[f"in_{n}{N_TIE}"]) for n in shapes.TIE_SURFACES}
    frac["steps_tol05"] = shapes.tie_fraction(g[f"in_steps{N_TIE}"], 0.5)
    print("tied land cells:", {n: round(f, 3) for n, f in frac.items()})
    for n in MOSTLY_TIED + ("steps_tol05",):
        assert frac[n] > 0.5, (n, frac[n])
    # tol = 0.5 on steps: a cardinal step down is exactly tol and stays, the diagonal one falls below; the default tol keeps both
    z = g[f"in_steps{N_TIE}"]
    down = z[1:, :] - z[:-1, :]
    assert set(np.unique(down).tolist()) == {0.0, 0.5} and np.float32(0.5) / twin.SQRT2_F32 < np.float32(0.5)
    assert not np.array_equal(g[f"kmax_d8_steps{N_TIE}"], g[f"kmax_d8_steps{N_TIE}_tol05"])
    assert g[f"sink_d8_steps{N_TIE}_tol05"].sum() > g[f"sink_d8_steps{N_TIE}"].sum()
    # a first maximum that is not k = 0: among tied cells the recorded argmax takes the first of the tied k, on every surface that ties
    for n in ("checkerboard", "steps"):
        k = g[f"kmax_d8_{n}{N_TIE}"]
        assert len(np.unique(k)) >= 2, n
    # the five surfaces with (nearly) unique maxima: what they cover instead
    for n in ("pit_l1", "pit_linf", "peak_linf_sea", "saddle", "plane"):
        assert 0 < frac[n] <= 0.5, (n, frac[n])
        if n != "peak_linf_sea":                                               # (there a cardinal beats the diagonals everywhere)
            assert (g[f"kmax_d8_{n}{N_TIE}"] >= 4).any(), n                    # a diagonal wins somewhere: the division by fl32(sqrt 2) decides
    assert frac["peak_linf_sea"] > 0.15                                        # +inf into the sea at three or more k along the ring
    assert len(np.unique(g[f"kmax_d8_pit_linf{N_TIE}"])) == 8 and len(np.unique(g[f"kmax_d8_pit_l1{N_TIE}"])) == 8
    assert g[f"sink_d8_flat{N_TIE}"].all() and (g[f"out_acc_flat{N_TIE}"] == 1).all()


def test_chains_and_fan_in(golden):
    g = golden("hydro_structured")
    got = {}
    for n in ("ramp64", "ramp130", "pit_linf257", f"pit_linf{N_TIE}", "comb"):
        got[n] = shapes.longest_chain(g["in_" + n], g["receiver_d8_" + n], g["sink_d8_" + n]) + (int(g["out_acc_" + n].max()),)
    print("(longest chain, max fan-in, largest count):", got)
    assert got["ramp64"][0] >= 1800 and got["ramp130"][0] >= 8000
    assert got["ramp64"] == (1892, 4, 4027) and got["ramp130"] == (8129, 4, 16765)
    assert got["pit_linf257"] == (128, 8, 257 * 257) and got[f"pit_linf{N_TIE}"][1] == 8
    assert got["comb"][2] == 2721 and int((g["in_comb"] > 0).sum()) == 2760
    # the comb's trunk: 35 teeth (the even columns); all but the one beside the sea deliver a tooth and its ridge cells to the row H - 2
    acc = g["out_acc_comb"]
    assert int((acc[-3, :-1] >= 30).sum()) == 34 and (np.diff(acc[-2, :-1]) > 0).all()
    # the filled serpentine routes on slopes of about eps = fl32(1e-3) against tol = fl32(1e-3): both outcomes occur along the channel
    f = g["in_serp64_filled"]
    ch = shapes.serpentine(64, 64) == 1
    assert g["sink_d8_serp64_filled"][ch].any() and (~g["sink_d8_serp64_filled"][ch]).any()
    assert np.array_equal(f[~ch], shapes.serpentine(64, 64)[~ch]) and (f[ch] > 10).all()


def test_fill_depth(golden, twin_fills):
    its = {name: it for name, (_, it) in twin_fills.items()}
    print("twin Jacobi iterations:", its)
    assert its["fill_serp64"] >= 1800 and its["fill_serp130"] >= 8000
    assert its["fill_serp64x65"] >= 1800 and its["fill_serp65x64"] >= 1800 and its["fill_serp64_conn4"] > its["fill_serp64"]
    g = golden("hydro_structured")
    out = g["out_fill_serp64"]
    for other in ("fill_serp64_conn4", "fill_serp64_eps0", "fill_serp64_eps001"):
        assert not np.array_equal(out, g["out_" + other]), other
    ch = shapes.serpentine(64, 64) == 1
    assert (g["out_fill_serp64_eps0"][ch] == 10).all()                       # eps 0: the channel fills level with its outlet
    pit, filled = g["in_pit_linf257"], g["out_fill_pit_linf257"]             # one basin over 5 x 5 tiles: filled from the rim (129) inwards
    assert (filled[1:-1, 1:-1] > pit[1:-1, 1:-1]).all() and np.array_equal(filled[0], pit[0]) and 129.1 < filled[128, 128] < 129.2
