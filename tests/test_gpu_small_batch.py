"""GPU tests of the small-batch conv flavour (conv_sb.hip, engine option "sb", default on): K split over the four waves of a workgroup and
reduced through LDS instead of fp32 partial planes in HBM + a reduce launch (BASELINE configs[1]: one 64x64 latent tile; the 1-16-window batches
of the cascade's latent stage).  It replaces conv_glds wherever that would have split K over workgroups; its K order differs, so its results differ
from conv_glds in bf16 rounding and are held to the same bounds against the reference: 2e-2 (bf16) / 4e-3 (fp16) rel-RMS per forward.
"""
import numpy as np
import pytest
import torch

from conftest import rel_rms
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def orc():
    from oracle import rng, unet
    return dict(rng=rng, unet=unet)


@pytest.fixture(scope="module")
def base(td, orc):
    cfg = dict(orc["unet"].BASE_CONFIG)
    sd = orc["unet"].synth_state_dict(cfg, seed=1234)
    return {d: td.EDMUnet2D(**cfg, dtype=d).load_state_dict(sd) for d in ("bf16", "fp16")}


def _inputs(orc, n):
    x = torch.from_numpy(orc["rng"].standard_normal(7, (n, 5, 64, 64))).cuda()
    c = torch.from_numpy(orc["rng"].standard_normal(8, (n, 58))).cuda()
    return x, torch.full((n,), 1.1), [c]


def _flavours(eng, model, args):
    """flavour tag ('f4m2n2', 'f2s', ...) of every conv launch of one forward, from the engine's profile labels"""
    import re
    with pinned(eng, profile=1):
        eng.profile_read(reset=True)
        try:
            model(*args)
            rows = eng.profile_ops()
        finally:
            eng.profile_read(reset=True)
    return {r[0].split(" [")[0]: re.search(r" (f\d\w*) bn", r[0]).group(1) for r in rows if " [" in r[0]}


@pytest.mark.parametrize("dtype,tol", [("bf16", 2e-2), ("fp16", 4e-3)])
def test_single_tile_forward_runs_on_the_small_batch_flavour_and_matches_the_reference(td, orc, golden, base, dtype, tol):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    args = _inputs(orc, 1)
    m = base[dtype]
    y = m(*args)
    err = rel_rms(y.cpu().numpy(), golden("unet")["base_out"])
    fl = _flavours(eng, m, args)
    n4 = sum(v.startswith(("f4", "f5")) for v in fl.values())
    n5 = sum(v.startswith("f5") for v in fl.values())
    print(f"batch 1 {dtype}: {n4} of {len(fl)} conv launches on the small-batch flavours ({n5} of them on the 64 px x 16 cout one); rel-RMS vs reference {err:.3e}")
    assert err < tol
    assert n4 >= 70, fl   # every conv that used to split K over workgroups (78 of 79 at batch 1)
    assert n5 >= 15, fl   # round 5: the 16x16 level (19 convs) no longer splits K over workgroups (at 8x8 that stays the faster plan: 48 workgroups of 16 couts lose)
    with pinned(eng, sb=0):   # the same forward with the flavour switched off: conv_glds + split-K, same bound, and the two agree to bf16 rounding
        y0 = m(*args)
        assert not any(v.startswith(("f4", "f5")) for v in _flavours(eng, m, args).values())
    assert rel_rms(y0.cpu().numpy(), golden("unet")["base_out"]) < tol
    assert rel_rms(y.cpu().numpy(), y0.cpu().numpy()) < tol


@pytest.mark.parametrize("mt,nt", [(2, 2), (2, 1), (1, 2), (1, 1), (4, 1)])
def test_every_tile_shape_of_the_small_batch_flavour(td, orc, golden, base, mt, nt):
    """test hooks sb_mt / sb_nt force one tile shape on every layer (64 / 32 pixels x 64 / 32 couts, 16-wide and 8-wide maps): each must hold
    the reference bound on its own"""
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    args = _inputs(orc, 1)
    with pinned(eng, sb_mt=mt, sb_nt=nt):
        y = base["bf16"](*args)
        fl = _flavours(eng, base["bf16"], args)
    tag = f"f4m{mt}n{nt}"
    # (the 128-pixel tile of round 5 exists on 16-wide maps only: the 8x8 level keeps the planner's tile there)
    assert sum(v == tag for v in fl.values()) >= (50 if mt == 4 else 70), fl
    err = rel_rms(y.cpu().numpy(), golden("unet")["base_out"])
    print(f"sb tile m{mt} n{nt}: rel-RMS vs reference {err:.3e}")
    assert err < 2e-2


def _split_k_launches(eng, model, args):
    """conv launches of one forward that split K over workgroups (ks > 1 in the profile label: each has a reduce launch behind it)"""
    import re
    with pinned(eng, profile=1):
        eng.profile_read(reset=True)
        try:
            model(*args)
            rows = eng.profile_ops()
        finally:
            eng.profile_read(reset=True)
    return [r[0] for r in rows if (m_ := re.search(r" ks(\d+) ", r[0])) and int(m_.group(1)) > 1]


@pytest.mark.parametrize("dtype,tol", [("bf16", 2e-2), ("fp16", 4e-3)])
def test_deep_level_flavour_everywhere_and_no_reduce_launch_in_a_single_tile_forward(td, orc, golden, base, dtype, tol):
    """conv_s16.hip (64 px x 16 couts on 16x16x32 MFMAs, K split over the waves of the workgroup only).  (1) default plan of a single tile: the 16x16
    level no longer splits K over workgroups (44 reduce launches per forward in round 4, 25 now: the 8x8 level keeps them -- measured faster there,
    profiles/r05_conv_s16_deep_levels.txt); (2) option s16 = 2 forces it on every layer the small-batch
    flavours apply to (3x3 + fused 1x1 segments, pixel-norm prologue, every epilogue, the fp32 output conv with the generic epilogue): the
    reference bound holds on its own; (3) s16 = 0 restores the round-4 plan."""
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    args = _inputs(orc, 1)
    m = base[dtype]
    sk = _split_k_launches(eng, m, args)
    # (the two 384-cout convs of the 16x16 level's down block give 96 workgroups of 16 couts: below "s16_min_wgs", they keep their split-K plan too)
    assert 0 < len(sk) <= 26 and all("8x8" in l or "128x128_down" in l for l in sk), sk
    with pinned(eng, s16=2):
        y = m(*args)
        fl = _flavours(eng, m, args)
    assert sum(v == "f5c16" for v in fl.values()) >= 70, fl
    err = rel_rms(y.cpu().numpy(), golden("unet")["base_out"])
    print(f"s16 everywhere, {dtype}: rel-RMS vs reference {err:.3e}")
    assert err < tol
    with pinned(eng, s16=0):
        y0 = m(*args)
        assert not any(v.startswith("f5") for v in _flavours(eng, m, args).values())
        assert len(_split_k_launches(eng, m, args)) >= 40
    assert rel_rms(y0.cpu().numpy(), golden("unet")["base_out"]) < tol


def test_small_batches_match_the_single_tile_results(td, orc, base):
    """a window's result must not depend on what shares its batch beyond bf16 rounding (batches 2 ... 6 mix small-batch and throughput launches)"""
    m = base["bf16"]
    x, t, c = _inputs(orc, 6)
    y6 = m(x, t, c)
    for i in (0, 3, 5):
        yi = m(x[i:i + 1].contiguous(), t[i:i + 1], [c[0][i:i + 1].contiguous()])
        e = rel_rms(y6[i:i + 1].cpu().numpy(), yi.cpu().numpy())
        assert e < 1e-2, (i, e)


def test_ragged_map_and_workgroup_order(td, orc):
    """maps that are not a multiple of the tile (72x72 -> 36, 18, 9 wide levels), both workgroup orders (sb_order), against the per-tap flavour
    run of the same bf16 model (glds = 0, splitk = 0: no LDS-DMA kernel, no split-K)"""
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg = orc["unet"].tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(orc["unet"].synth_state_dict(cfg, seed=77))
    n_cond = 58   # BASE_CONFIG's one tensor input
    x = torch.from_numpy(orc["rng"].standard_normal(17, (2, cfg["in_channels"], 72, 72))).cuda()
    c = torch.from_numpy(orc["rng"].standard_normal(18, (2, n_cond))).cuda()
    t = torch.full((2,), 0.9)
    with pinned(eng, glds=0, splitk=0):
        ref = m(x, t, [c])
    for order, s16 in ((0, 1), (1, 1), (0, 2), (1, 2)):   # s16 = 2: the 64 px x 16 cout flavour on every eligible layer (ragged 36 / 18 / 9-wide maps)
        with pinned(eng, sb_order=order, s16=s16):   # (on exit: back to the planner's choice)
            y = m(x, t, [c])
            fl = _flavours(eng, m, (x, t, [c]))
        assert any(v.startswith("f4" if s16 == 1 else "f5") for v in fl.values()), fl
        e = rel_rms(y.cpu().numpy(), ref.cpu().numpy())
        print(f"ragged 72x72, sb_order {order}, s16 {s16}: rel-RMS vs the per-tap flavour {e:.3e}")
        assert e < 1e-2, (order, s16, e)
    m.close()
