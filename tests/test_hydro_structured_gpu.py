"""Hydrology on the GPU (libtd_hydro.so, hydro_csrc/hydro_kernels.hip) on structured terrain: every case the reference's postprocessing.py
gave on the closed-form terrains of tests/_hydro_shapes.py (tests/golden/hydro_structured.npz).  Noise-like canvases never reach the paths
these reach:
  * fill -- a one-cell channel advances one column per in-tile sweep, so a tile stops at FILL_MAX_SWEEPS = 128 and has to continue in the
    next pass, td_hydro_fill goes through several FILL_BATCH = 8 batches of passes, and on the 130^2 canvas the channel crosses every tile
    border back and forth, so tiles go idle and are woken again and again;
  * accumulation -- one chain of 8129 cells for a single walker, eight donors at one cell, a trunk that 34 walkers reach together;
  * d8 -- surfaces on which most cells' largest slope is attained at two or more neighbours, and slopes exactly equal to tol.
The conditions on `passes` below are conditions, not measurements: with one tile a pass ends either converged or at the sweep cap, and a
converged first pass gives passes == 2, so passes >= 3 proves the cap-and-continue path ran; passes > 8 proves a second batch was entered.

Measured on an MI355X (passes, the last no-change pass included):
    serpentine 64 x 64: 16 (connectivity 4: 17, epsilon 0: 16, epsilon 0.01: 16)     64 x 65: 16     65 x 64: 17     130 x 130: 132
    pit_linf 257 x 257: 3 (no condition: a wide basin converges fast)
the same counts on a second call.  A Jacobi emulation of the tile scheme on the host gives 16, 17 (64 x 65) and 132.
"""
import json

import numpy as np
import pytest
import torch

import _hydro_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

SINGLE_TILE = ("fill_serp64", "fill_serp64_conn4", "fill_serp64_eps0", "fill_serp64_eps001")
SECOND_BATCH = SINGLE_TILE + ("fill_serp64x65", "fill_serp65x64", "fill_serp130")


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available()
    return t


def _cases(golden, fn):
    g = golden("hydro_structured")
    cases = json.loads(str(g["cases"]))
    assert len(cases) == 38
    return g, [(c["name"], g[c["input"]], c["kwargs"]) for c in cases if c["fn"] == fn]


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def test_fill_reaches_the_sweep_cap_and_a_second_batch_and_matches_the_reference(td, golden):
    g, cases = _cases(golden, "fill")
    assert len(cases) == 8
    passes = {}
    for name, z, kw in cases:
        filled, passes[name] = td.fill_depressions(torch.from_numpy(z).cuda(), return_passes=True, **kw)
        filled = filled.cpu().numpy()
        print(f"{name} {z.shape}: passes = {passes[name]}")
        assert filled.dtype == np.float32 and np.array_equal(filled, g["out_" + name], equal_nan=True), (name, passes[name])
        assert twin.fill_fixed_point_violations(z, filled, **kw) == 0, name
    for name in SINGLE_TILE:
        assert g["in_serp64"].shape == (64, 64) and passes[name] >= 3, (name, passes[name])     # stopped at the cap, went on in the next pass
    for name in SECOND_BATCH:
        assert passes[name] > 8, (name, passes[name])                                           # entered a second batch of passes


def test_fill_twice_and_from_host_or_device_is_bit_identical(td, golden):
    g, cases = _cases(golden, "fill")
    for name, z, kw in cases:
        if name not in ("fill_serp64", "fill_serp64x65", "fill_serp130"):
            continue
        zd = torch.from_numpy(z).cuda()
        a, pa = td.fill_depressions(zd, return_passes=True, **kw)
        b, pb = td.fill_depressions(zd, return_passes=True, **kw)
        host = td.fill_depressions_priority_flood(z, **kw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert isinstance(host, np.ndarray) and np.array_equal(host, a.cpu().numpy(), equal_nan=True), name
        assert np.array_equal(host, g["out_" + name], equal_nan=True), name
        print(f"{name}: passes = {pa}, {pb}")


def test_d8_on_tied_slopes_matches_the_reference_and_the_twin(td, golden):
    g, cases = _cases(golden, "d8")
    assert len(cases) == 14
    for name, z, kw in cases:
        receiver, kmax, sink = (t.cpu().numpy() for t in td.flow_directions(torch.from_numpy(z).cuda(), **kw))
        assert np.array_equal(receiver, g["receiver_" + name]), name
        assert np.array_equal(kmax, g["kmax_" + name]) and np.array_equal(sink, g["sink_" + name]), name
        r, k, s = twin.d8(z, **kw)
        assert np.array_equal(receiver, r) and np.array_equal(kmax, k) and np.array_equal(sink, s), name
        rr, cc, sk, km = td.d8_flow(z, **kw)                                 # the drop-in, from a host array
        assert np.array_equal(rr * z.shape[1] + cc, r) and np.array_equal(km, k) and np.array_equal(sk, s), name


def test_accumulation_over_long_chains_and_full_fan_in_matches_the_reference(td, golden):
    g, cases = _cases(golden, "acc")
    assert len(cases) == 14
    for name, z, kw in cases:
        zd = torch.from_numpy(z).cuda()
        receiver, _, sink = td.flow_directions(zd, **kw)                       # an acc case's kwargs are its d8's
        acc = td.flow_accumulation_map(zd, receiver, sink)
        again = td.flow_accumulation_map(zd, receiver, sink)
        got, want = acc.cpu().numpy(), g["out_" + name]
        print(f"{name} {z.shape}: largest count = {int(got.max())} (recorded {int(want.max())})")
        assert got.max() >= want.max(), name                                   # a truncated walk
        assert got.dtype == np.float32 and np.array_equal(got, want), name
        assert twin.accumulation_ok(z, receiver.cpu().numpy(), sink.cpu().numpy(), got), name
        assert torch.equal(acc, again), name


def test_indicator_matches_the_reference_to_one_ulp(td, golden):
    g, cases = _cases(golden, "indicator")
    assert len(cases) == 2
    for name, z, kw in cases:
        want = g["out_" + name]
        for got in (td.plot_flow_indicator(z, **kw), td.flow_indicator(torch.from_numpy(z).cuda(), **kw).cpu().numpy()):
            assert got.dtype == np.float32 and got.shape == want.shape, name
            assert _ulps(got, want) <= 1, (name, _ulps(got, want))
