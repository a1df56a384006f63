"""GPU: td.EDMAutoencoder (the encoder-only and skip-less decoder graphs of the engine and the kernels around them) against the outputs the
reference's own EDMAutoencoder recorded (tests/golden/autoencoder.npz), and the new kernels element by element."""
import numpy as np
import pytest
import torch

import _ae_twin as T
from conftest import rel_rms
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

BOUNDS = {"fp32": 5e-6, "bf16": 2e-2, "fp16": 4e-3}   # the project's per-forward bounds (tests/test_gpu_parity.py: test_unet_base_forward)
F16_ROUND = 2.0 ** -11                                  # storage rounding of a binary16 value, relative
# four levels of 64 channels: a cheap model whose bottleneck is 8 x smaller than its input (direct-skip blocks of 8 x 8)
DEEP = dict(image_size=16, in_channels=2, model_channels=64, model_channel_mults=[1, 1, 1, 1], layers_per_block=1, midblock_attention=False,
            latent_channels=2, direct_skips=[1])


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    return t


@pytest.fixture(scope="module")
def tiny(td):
    sd = T.synth_ae_state_dict(T.TINY, seed=77)
    ms = {d: td.EDMAutoencoder(**T.TINY, dtype=d).load_state_dict(sd) for d in ("fp32", "bf16", "fp16")}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def released(td):
    sd = T.synth_ae_state_dict(T.RELEASED, seed=78)
    ms = {d: td.EDMAutoencoder(**T.RELEASED, dtype=d).load_state_dict(sd) for d in ("bf16", "fp16")}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def deep(td):
    m = td.EDMAutoencoder(**DEEP, dtype="fp32").load_state_dict(T.synth_ae_state_dict(DEEP, seed=79))
    yield m
    m.close()


def _recorded_shapes(g, tag):
    return {str(n): tuple(int(v) for v in s if v >= 0) for n, s in zip(g[f"names_{tag}"], g[f"shapes_{tag}"])}


def _rng(seed, shape):
    from oracle import rng
    return torch.from_numpy(rng.standard_normal(seed, shape))


def test_expected_parameters_and_checkpoint_refusals(td, golden):
    from terrain_diffusion_amd._lib import ae_lib as lib
    g = golden("autoencoder")
    for tag, cfg in (("tiny", T.TINY), ("released", T.RELEASED)):
        m = td.EDMAutoencoder(**cfg, dtype="bf16")
        want = {k: v for k, v in _recorded_shapes(g, tag).items() if not T.is_ignored(k)}
        assert m.expected_parameters() == want
        if tag == "tiny":
            with pytest.raises(RuntimeError):                           # run before weights
                m.preencode(torch.zeros(1, 2, 16, 16))
            sd = T.synth_ae_state_dict(cfg, seed=77)
            bad = dict(sd); bad.pop("encoder.out_gain")
            with pytest.raises(KeyError):                               # missing parameter
                m.load_state_dict(bad)
            bad = dict(sd); bad["decoder_conv.weight"] = torch.zeros(128, 4, 1, 2)
            with pytest.raises(ValueError):                             # wrong shape
                m.load_state_dict(bad)
            bad = dict(sd); bad["decoder.0.emb_linear.weight"] = torch.zeros(128, 128)
            with pytest.raises(KeyError):                               # a key the model does not have (the ignored ones are not such keys)
                m.load_state_dict(bad)
            assert lib().td_ae_set_param(m._h, b"no.such.param", None, 0) != 0 and b"unknown parameter" in lib().td_last_error()
        m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_tiny_model_matches_the_reference(tiny, golden, dtype):
    g, m, tol = golden("autoencoder"), tiny[dtype], BOUNDS[dtype]
    L = T.TINY["latent_channels"]
    xa, xb = torch.from_numpy(g["tiny_x_a"]), torch.from_numpy(g["tiny_x_b"])
    cases = [("a", xa, g["tiny_means_a"], g["tiny_logvars_a"]),
             ("odd", torch.cat([xa, xa[:1]]), np.concatenate([g["tiny_means_a"], g["tiny_means_a"][:1]]), np.concatenate([g["tiny_logvars_a"], g["tiny_logvars_a"][:1]])),
             ("b", xb, g["tiny_means_b"], g["tiny_logvars_b"])]
    for tag, x, rm, rl in cases:
        means, logvars = m.preencode(x.cuda())
        assert means.is_cuda and means.shape == rm.shape and logvars.shape == rl.shape
        em, el = rel_rms(means[:, :L].cpu().numpy(), rm[:, :L]), rel_rms(logvars[:, :L].cpu().numpy(), rl[:, :L])
        print(f"tiny {dtype} preencode {tag}: means {em:.3e} logvars {el:.3e}")
        assert em < tol and el < tol, (tag, em, el)
        hm, hl = m.preencode(x)                                         # host pointers: the same bits
        assert not hm.is_cuda and torch.equal(hm, means.cpu()) and torch.equal(hl, logvars.cpu())
    for tag in ("a", "b"):
        z = torch.from_numpy(g[f"tiny_means_{tag}"])
        y = m.decode(z.cuda())
        e = rel_rms(y[:, :1].cpu().numpy(), g[f"tiny_decode_{tag}"][:, :1])     # channel 1 is a direct skip
        print(f"tiny {dtype} decode {tag}: {e:.3e}")
        assert y.shape == g[f"tiny_decode_{tag}"].shape and e < tol, (tag, e)
        assert torch.equal(m.decode(z), y.cpu())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_released_model_dataset_latents_and_decode(released, golden, dtype):
    g, m, tol = golden("autoencoder"), released[dtype], BOUNDS[dtype]
    stack = m.encode_dihedral(torch.from_numpy(g["rel_chunk"]).cuda())      # residual_mean 0, residual_std 1.1678: build_encoded_dataset.py's defaults
    assert stack.dtype == torch.float16 and tuple(stack.shape) == g["rel_latent_f16"].shape == (8, 8, 8, 8)
    e = rel_rms(stack.float().cpu().numpy(), g["rel_latent_f16"].astype(np.float32))
    print(f"released {dtype} encode_dihedral: {e:.3e}")
    assert e < tol + F16_ROUND
    y = m.decode(torch.from_numpy(g["rel_means"]).cuda())
    e = rel_rms(y.cpu().numpy(), g["rel_decode"])
    print(f"released {dtype} decode: {e:.3e}")
    assert y.shape == g["rel_decode"].shape and e < tol


def _direct_mean_check(x_norm_views, means, L, s):
    """direct mean channel against the float64 block mean of the fp32-normalised input: |gpu - D64| <= n u mean_block|x|, n = s^2, u = 2^-24
    (an fp32 sum of n terms in any order plus the rounding of the division)"""
    v = x_norm_views[:, 1].double()
    n, H, W = v.shape
    blocks = v.reshape(n, H // s, s, W // s, s)
    d64, mabs = blocks.mean(dim=(2, 4)), blocks.abs().mean(dim=(2, 4))
    err = (means[:, L].double().cpu() - d64).abs()
    bound = (s * s) * 2.0 ** -24 * mabs
    print(f"direct mean s={s}: worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("S", [16, 48])
def test_dihedral_views_and_latent_head_are_exact(tiny, S):
    """fp32 model.  The one-call dihedral form equals preencode of the 8 views built with torch.flip / torch.rot90 on the normalised chunk -- the same
    batch on the same plan -- bit for bit; 48 is no multiple of 32 and the data has no symmetry."""
    m, L = tiny["fp32"], T.TINY["latent_channels"]
    x = _rng(500 + S, (2, S, S)) * 1.3 + 0.2
    mean, std = 0.3, 1.7
    means, logvars, packed = m.preencode_dihedral(x.cuda(), mean, std)
    xn = ((x - mean) / std).float()                                     # on the CPU: one subtraction, one true division (build_encoded_dataset.py:69)
    views = torch.stack(T.dihedral_views(xn))
    rm, rl = m.preencode(views.cuda())
    assert means.shape == (8, 3, S // 2, S // 2)
    assert torch.equal(means, rm) and torch.equal(logvars, rl)
    assert torch.equal(packed, torch.cat([means, logvars], dim=1).to(torch.float16))
    assert torch.equal(m.encode_dihedral(x.cuda(), mean, std), packed)
    assert bool((logvars[:, L:] == -20.0).all())
    _direct_mean_check(views, means, L, 2)
    # identity normalisation: the staged input is the plain one
    a, b = m.preencode(views.cuda())
    c, d, _ = m._preencode(views.cuda(), 0.0, 1.0, False, False)
    assert torch.equal(a, c) and torch.equal(b, d)


def test_direct_mean_over_8x8_blocks(deep):
    m, L = deep, DEEP["latent_channels"]
    x = _rng(611, (2, 48, 48)) * 2.1 - 0.4
    mean, std = -0.1, 1.1678
    means, logvars, _ = m.preencode_dihedral(x.cuda(), mean, std)
    views = torch.stack(T.dihedral_views(((x - mean) / std).float()))
    assert means.shape == (8, 3, 6, 6) and bool((logvars[:, L:] == -20.0).all())
    _direct_mean_check(views, means, L, 8)
    rm, _ = m.preencode(views.cuda())
    assert torch.equal(means, rm)


def test_decode_direct_channels_and_denormalisation(tiny):
    m, L = tiny["fp32"], T.TINY["latent_channels"]
    z = _rng(620, (2, 3, 5, 7)).cuda()
    y = m.decode(z)
    assert y.shape == (2, 2, 10, 14)
    up = z[:, L].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(y[:, 1], up)
    assert torch.equal(y[:, 1], torch.nn.functional.interpolate(z[:, L:L + 1], size=(10, 14), mode="nearest")[:, 0])
    std, mean = 1.1678, 0.25
    yd = m.decode(z, std=std, mean=mean)
    assert torch.equal(yd.cpu(), y.cpu() * std + mean)


def test_postencode_formula_noise_and_mode(td, tiny):
    m = tiny["fp32"]
    shape = (4, 3, 8, 8)
    means, eps = _rng(630, shape), _rng(631, shape)
    from oracle import rng
    u = rng.pcg_stream(632, int(np.prod(shape))).astype(np.float64) / 4294967296.0
    logvars = torch.from_numpy((-20.0 + 24.0 * u).astype(np.float32)).reshape(shape)
    z = m.postencode(means.cuda(), logvars.cuda(), eps=eps.cuda())
    sigma = torch.exp(0.5 * logvars.double())
    prod = eps.double().abs() * sigma
    d64 = means.double() + eps.double() * sigma
    ulp = lambda t: torch.from_numpy(np.spacing(t.abs().numpy().astype(np.float32)).astype(np.float64))
    bound = 2 * ulp(prod) + ulp(d64)
    err = (z.double().cpu() - d64).abs()
    print(f"postencode: worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(m.postencode(means, logvars, eps=eps), z.cpu())     # host pointers
    zs = m.postencode(means.cuda(), logvars.cuda(), seed=4242)
    noise = td.standard_normal(4242, shape, as_torch=True)
    assert torch.equal(zs, m.postencode(means.cuda(), logvars.cuda(), eps=noise)) and not torch.equal(zs, z)
    mc = means.cuda()
    assert m.postencode(mc, logvars.cuda(), use_mode=True) is mc
    with pytest.raises(ValueError):
        m.postencode(mc, logvars.cuda())


def test_save_and_load_round_trip(td, tiny, tmp_path):
    m = tiny["bf16"]
    m.save_pretrained(str(tmp_path / "ae"))
    m2 = td.EDMAutoencoder.from_pretrained(str(tmp_path / "ae"), dtype="bf16")
    assert m2.config == m.config and set(m2.state_dict()) == set(m.state_dict())
    x = _rng(640, (2, 2, 16, 16)).cuda()
    (a, b), (c, d) = m.preencode(x), m2.preencode(x)
    assert torch.equal(a, c) and torch.equal(b, d)
    out, lv = m2.decode(a, include_logvar=True)
    assert torch.equal(out, m.decode(a)) and lv.shape == (1, 1, 1, 1) and float(lv) == 0.25
    m2.close()


def test_unet_on_the_same_engine_after_an_autoencoder(td, golden):
    from oracle import rng
    from oracle.unet import synth_state_dict, tiny_config
    ae = td.EDMAutoencoder(**T.TINY, dtype="bf16").load_state_dict(T.synth_ae_state_dict(T.TINY, seed=77))
    z, _ = ae.preencode(_rng(650, (1, 2, 16, 16)).cuda())
    ae.decode(z)
    ae.close()
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="fp32").load_state_dict(synth_state_dict(cfg, seed=77))
    x = torch.from_numpy(rng.standard_normal(7, (2, 5, 16, 16)))
    cond = torch.from_numpy(rng.standard_normal(8, (2, 58)))
    y = m(x.cuda(), noise_labels=torch.tensor([1.2, 0.3]), conditional_inputs=[cond.cuda()])
    assert rel_rms(y.cpu().numpy(), golden("unet")["tiny_out"]) < 5e-6
    m.close()
