"""The 16x16x32-MFMA form of the wide conv tile (csrc/conv_glds_wide16.hip, engine option glds_wide_mfma16 = 1): the 96-cout, pure-3x3 launches of the
wide tile on one 32-deep MFMA step per half K-step, with a lane -> pixel map, weight-slot order and epilogue ownership of its own.

  * every conv op of a forward that runs on it, element by element against the float64 twin of the op on the op's own stored inputs (tests/_conv_twin.py:
    |hip - ref| <= half_ulp_T(ref) + E), every sum-of-squares plane included -- on 40x40 maps (40 -> 20 -> 10 -> 5: the 16x16 tiles hang over the edge at
    every level, the smallest maps on which the clamped out-of-image columns can go wrong) in bf16 and on 64x64 in fp16;
  * the profile labels say which launches took it: ` x16` on at least ten, on none with a 1x1 segment or another cout tile, on none with the option off;
  * the same forward twice gives the same bits; the network output with the option on against off stays inside the 2e-2 rel-RMS bound the suite holds
    two tile families to (tests/test_gpu_bench_config.py, test_wide_tile_*), for a forward and for a two-step td_sample_edm_img call (the fused solver
    epilogue downstream of the new kernel)."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_twin as ct
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (autouse: every test here starts and ends on the shipped options)
from conftest import rel_rms

pytestmark = pytest.mark.gpu

# glds_wide = 2 puts a launch on the wide tile "wherever it is legal", and a launch that splits K is not: at these batch sizes (2 - 4 windows) every
# level's grid is small enough for the planner to split K, which left ONE wide launch in the forward.  glds_splitk = 0 keeps K whole, so that the wide
# tile really is forced on every 16-wide level, as the arms of test_conv_ops_gpu.py get it from a larger batch.
ON = dict(glds_wide=2, glds_splitk=0, glds_wide_mfma16=1)
OFF = dict(glds_wide=2, glds_splitk=0, glds_wide_mfma16=0)


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def zoo(td):
    """the base model and its twin per storage type, built on first use"""
    from oracle.unet import BASE_CONFIG, synth_state_dict
    cfg = dict(BASE_CONFIG)
    sd = synth_state_dict(cfg, seed=1234)
    models, twins = {}, {}

    def get(T):
        if T not in models:
            models[T] = td.EDMUnet2D(**cfg, dtype=T).load_state_dict(sd)
            twins[T] = ct.Twin(cfg, sd, T, "cuda")
        return cfg, models[T], twins[T]

    yield get
    for m in models.values():
        m.close()


def _inputs(cfg, n, H, W, seed=7):
    from oracle import rng
    x = torch.from_numpy(rng.standard_normal(seed, (n, cfg["in_channels"], H, W)))
    cond = [torch.from_numpy(rng.standard_normal(seed + 1 + i, (n, c[1]))).cuda() for i, c in enumerate(cfg.get("conditional_inputs", []))]
    return x, torch.full((n,), 1.1), cond


def _forward(eng, m, x, t, cond, **opts):
    """(output, profile labels of the conv launches) of one forward under `opts`"""
    with pinned(eng, **opts):
        with pinned(eng, profile=1):
            eng.profile_read(reset=True)
            y = m(x.cuda(), t, cond).clone()
            torch.cuda.synchronize()
            labels = [r[0] for r in eng.profile_ops() if " [" in r[0]]
        eng.profile_read(reset=True)
    return y, labels


def _x16(label):
    return re.search(r" x16\]", label) is not None


@pytest.mark.parametrize("T,n,hw", [("bf16", 3, 40), ("fp16", 2, 64)])
def test_every_conv_op_on_the_mfma16_tile_against_its_float64_twin(td, zoo, T, n, hw):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg, m, tw = zoo(T)
    x, t, cond = _inputs(cfg, n, hw, hw)
    with pinned(eng, **ON):
        with pinned(eng, profile=1):
            eng.profile_read(reset=True)
            y = m(x.cuda(), t, cond)
            torch.cuda.synchronize()
            labels = [r[0] for r in eng.profile_ops() if " [" in r[0]]
        eng.profile_read(reset=True)
        fl = {}
        for l in labels:
            lab, tag, ks = ct.flavour_of(l)
            fl[lab] = (tag, ks)
        assert set(fl) == set(tw.by_label), set(fl) ^ set(tw.by_label)
        on16 = [l for l in labels if _x16(l)]
        print(f"\n{T} n{n} {hw}x{hw}: {len(on16)} of {len(labels)} conv launches on the 16x16x32 tile, {sum(' f2w ' in l for l in labels)} on the wide tile")
        assert len(on16) >= 10, labels
        for l in labels:
            lab = ct.flavour_of(l)[0]
            tail = any(s["taps"] == 1 for s in tw.by_label[lab]["segs"])
            bn = int(re.search(r" bn(\d+) ", l).group(1))
            if tail or bn != 96:
                assert not _x16(l), l
            if _x16(l):
                assert " f2w " in l, l      # the flavour tag stays f2w
        stats, nss = ct.check_forward(m, tw, x, t, cond, T, fl)     # every op, every sum-of-squares plane, at the twin's own bound
        assert len(stats) == len(tw.ops) and nss == sum(o["sumsq"] for o in tw.ops)
        print(ct.summary_line(f"mfma16 {T} n{n} {hw}x{hw}", stats, nss, 0.0))
        assert torch.isfinite(y).all()


def test_same_forward_twice_same_bits_and_option_off_within_the_tile_family_bound(td, zoo):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg, m, _ = zoo("bf16")
    x, t, cond = _inputs(cfg, 3, 40, 40, seed=23)
    y1, l1 = _forward(eng, m, x, t, cond, **ON)
    y2, _ = _forward(eng, m, x, t, cond, **ON)
    assert sum(_x16(l) for l in l1) >= 10
    assert torch.equal(y1, y2), float((y1 - y2).abs().max())
    y0, l0 = _forward(eng, m, x, t, cond, **OFF)
    assert not any(_x16(l) for l in l0), [l for l in l0 if _x16(l)]
    assert torch.isfinite(y0).all() and float(y0.abs().mean()) > 1e-4
    e = rel_rms(y1.cpu().numpy(), y0.cpu().numpy())
    print(f"\nmfma16 on vs off, network output rel-RMS {e:.2e}")
    assert e < 2e-2, e


def test_two_step_sampler_call_on_against_off(td, zoo):
    """td_sample_edm_img, 4 windows of 64x64, 2 steps, wide tile forced: the solver step fused behind the output conv consumes what the new kernel wrote"""
    from oracle import rng, schedule
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import get_engine, ptr
    eng = get_engine("cuda")
    cfg, m, _ = zoo("bf16")
    n, H, W, steps = 4, 64, 64, 2
    sig = schedule.karras_sigmas(steps)[0].contiguous()
    x0 = (torch.from_numpy(rng.standard_normal(17, (n, cfg["out_channels"], H, W))) * float(sig[0])).contiguous()
    conds = [torch.from_numpy(rng.standard_normal(18 + i, (n, c[1]))) for i, c in enumerate(cfg.get("conditional_inputs", []))]
    cond = m.cond_rows(conds, n, "cuda") if conds else None
    xf, tf, cf = _inputs(cfg, n, H, W, seed=29)
    _, labels = _forward(eng, m, xf, tf, cf, **ON)      # the plan of an n = 4 forward under these options: what each step of the call below launches
    assert sum(_x16(l) for l in labels) >= 10, labels
    outs = {}
    for k, o in (("on", ON), ("off", OFF)):
        x = x0.clone().cuda()
        with pinned(eng, **o):
            check(lib().td_sample_edm_img(m._h, n, H, W, steps, ptr(sig), 0.5, ptr(cond), None, 0, ptr(x)))
            torch.cuda.synchronize()
        assert torch.isfinite(x).all() and float(x.abs().mean()) > 1e-4
        outs[k] = x.cpu()
    e = rel_rms(outs["on"].numpy(), outs["off"].numpy())
    print(f"\nmfma16 on vs off, 2-step sampler call rel-RMS {e:.2e}")
    assert e < 2e-2, e
