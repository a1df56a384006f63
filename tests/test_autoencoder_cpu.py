"""CPU: the float64 twin of the reference's EDMAutoencoder (tests/_ae_twin.py) against the outputs the reference itself recorded
(tests/golden/autoencoder.npz, written by tests/golden/make_autoencoder_golden.py), the parameter list, the constructor refusals of
td.EDMAutoencoder and the td_ae_* declarations.  No engine is created here."""
import os
import re

import numpy as np
import pytest
import torch

import _ae_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 5e-6   # the project's fp32-vs-reference bound (tests/test_gpu_parity.py: fp32 forward)


def _recorded_shapes(g, tag):
    return {str(n): tuple(int(v) for v in s if v >= 0) for n, s in zip(g[f"names_{tag}"], g[f"shapes_{tag}"])}


def test_twin_reproduces_the_recorded_reference_outputs(golden):
    g = golden("autoencoder")
    tw = T.AETwin(T.TINY, T.synth_ae_state_dict(T.TINY, seed=77))
    for tag in ("a", "b"):
        taps = {}
        means, logvars = tw.preencode(torch.from_numpy(g[f"tiny_x_{tag}"]), taps)
        dec = tw.decode(torch.from_numpy(g[f"tiny_means_{tag}"]), taps)
        for name, got in (("means", means), ("logvars", logvars), ("decode", dec)):
            err = T.rel_rms(got, g[f"tiny_{name}_{tag}"])
            print(f"tiny {tag} {name}: {err:.3e}")
            assert got.shape == g[f"tiny_{name}_{tag}"].shape and err < TOL, (tag, name, err)
        assert np.all(g[f"tiny_logvars_{tag}"][:, 2:] == -20.0)
        if tag == "a":
            keys = [k for k in g.files if k.startswith("tiny_tap_")]
            assert len(keys) == len(tw.plan["enc"]) + len(tw.plan["dec"])
            for k in keys:
                err = T.rel_rms(taps[k[len("tiny_tap_"):]][:1, ::2], g[k])
                assert err < TOL, (k, err)
    tw = T.AETwin(T.RELEASED, T.synth_ae_state_dict(T.RELEASED, seed=78))
    x = (torch.from_numpy(g["rel_chunk"]) - 0.0) / 1.1678
    views = torch.stack(T.dihedral_views(x.float()))
    means, logvars = tw.preencode(views)
    stack = torch.cat([means, logvars], dim=1)
    ref = torch.from_numpy(g["rel_latent_f16"].astype(np.float32))
    # the recorded stack is fp16: the twin, rounded the same way, differs from it in the few elements that sit on a rounding boundary
    err = T.rel_rms(stack.to(torch.float16).float(), ref)
    print(f"released latent stack (fp16): {err:.3e}")
    assert stack.shape == ref.shape == (8, 8, 8, 8) and err < 2.0 ** -11
    assert T.rel_rms(means, g["rel_means"]) < TOL
    err = T.rel_rms(tw.decode(torch.from_numpy(g["rel_means"])), g["rel_decode"])
    print(f"released decode: {err:.3e}")
    assert err < TOL


def test_param_shapes_equal_the_reference_state_dict(golden):
    g = golden("autoencoder")
    for tag, cfg in (("tiny", T.TINY), ("released", T.RELEASED)):
        rec = _recorded_shapes(g, tag)
        assert any(T.is_ignored(k) for k in rec)
        want = {k: v for k, v in rec.items() if not T.is_ignored(k)}
        assert dict(T.ae_param_shapes(cfg)) == want
        sd = T.synth_ae_state_dict(cfg)
        assert set(sd) <= set(rec) and all(tuple(sd[k].shape) == rec[k] or sd[k].numel() == int(np.prod(rec[k])) for k in sd)


def test_autoencoder_class_refuses_before_any_engine_is_created(monkeypatch):
    import terrain_diffusion_amd as td
    from terrain_diffusion_amd import autoencoder as A
    assert td.EDMAutoencoder is A.EDMAutoencoder

    def no_engine(*a, **k):
        raise AssertionError("the engine was touched before the refusal")
    monkeypatch.setattr(A, "get_engine", no_engine)
    base = dict(image_size=16, in_channels=2, model_channels=64, model_channel_mults=[1, 2], layers_per_block=1, latent_channels=2, direct_skips=[1])
    for bad in (dict(block_kwargs={"dropout": 0.1}), dict(conditional_inputs=[["float", 64, 1.0]]), dict(latent_channels=None), dict(latent_channels=5),
                dict(in_channels=32, direct_skips=[]), dict(out_channels=9), dict(model_channels=48), dict(direct_skips=[2]),
                dict(latent_channels=4, direct_skips=[0] * 8 + [1] * 20)):
        with pytest.raises(NotImplementedError):
            td.EDMAutoencoder(**{**base, **bad})
    with pytest.raises(AssertionError, match="engine was touched"):     # a valid configuration does go on to the engine
        td.EDMAutoencoder(**base)


def test_unet_wrapper_still_refuses_the_autoencoder_topologies():
    import terrain_diffusion_amd as td
    base = dict(image_size=64, in_channels=5, model_channels=64, conditional_inputs=[["tensor", 58, 1.0]], fourier_scale="pos")
    for bad in (dict(encode_only=True), dict(noise_emb_dims=0)):
        with pytest.raises(NotImplementedError):
            td.EDMUnet2D(**{**base, **bad})


def test_header_declares_the_autoencoder_entry_points():
    """include/td_engine.h declares the td_ae_* entry points by including include/td_ae.h, the header that spells them out (td_engine.h's own text keeps
    the declarations it had: tests/test_sampler_args_cpu.py counts them); either header alone compiles as C99 and declares all of it; the library
    exports every one and terrain_diffusion_amd/_lib.py binds every one."""
    import ctypes
    import subprocess
    import tempfile
    import __graft_entry__ as ge
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    eng = strip(open(os.path.join(ROOT, "include", "td_engine.h")).read())
    assert re.search(r'^#include "td_ae.h"$', eng, flags=re.M), "include/td_engine.h does not include td_ae.h"
    text = strip(open(os.path.join(ROOT, "include", "td_ae.h")).read())
    declared = set(re.findall(r"\b(td_ae_[a-z0-9_]+)\s*\(", text))
    assert declared == {"td_ae_create", "td_ae_destroy", "td_ae_num_params", "td_ae_param_info", "td_ae_set_param", "td_ae_set_prefolded", "td_ae_finalize",
                        "td_ae_preencode", "td_ae_postencode", "td_ae_decode", "td_ae_read_activation"}
    assert "typedef struct td_ae_config" in text
    with tempfile.TemporaryDirectory() as d:
        for hdr in ("td_engine.h", "td_ae.h"):
            src = os.path.join(d, "t.c")
            with open(src, "w") as f:
                f.write(f'#include "{hdr}"\nint main(void) {{ td_ae_config c; c.latent_channels = td_version(); return td_ae_decode(0, 1, 1, 1, 0, 1.f, 0.f, 0) + c.latent_channels; }}\n')
            subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])
    ge.build()
    from terrain_diffusion_amd._lib import AE_EXPORTS, LIB_PATH
    assert set(AE_EXPORTS) == declared
    l = ctypes.CDLL(LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} declared in include/td_ae.h but not exported"
    assert os.path.join(ROOT, "include", "td_ae.h") in ge.ENGINE_HEADERS     # an edit of it moves the library's build id
