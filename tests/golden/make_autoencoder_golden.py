"""Writes tests/golden/autoencoder.npz: outputs of the reference's own EDMAutoencoder (terrain_diffusion/models/edm_autoencoder.py) on the synthetic
checkpoints of tests/_ae_twin.py, run on the CPU under make_golden's import shim.  Needs the reference checkout; the tests only read the file.

  names_<cfg> / shapes_<cfg>   the reference's state-dict names and shapes, both configs
  tiny_*                       preencode on (2,2,16,16) and on a non-square (1,2,32,16), decode of those means, per-block forward-hook taps
                               (first image, every other channel)
  rel_*                        the released config at (1,1,64,64): the 8-view dihedral latent stack as build_encoded_dataset.py:74-94 makes it (fp16)
                               and decode of the 8 fp32 means
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from oracle import rng  # noqa: E402
import _ae_twin as T  # noqa: E402

RES_MEAN, RES_STD = 0.0, 1.1678   # build_encoded_dataset.py's defaults


def _model(cfg, sd):
    from terrain_diffusion.models.edm_autoencoder import EDMAutoencoder
    m = EDMAutoencoder(**cfg).eval()
    ref_sd = m.state_dict()
    full = {k: (sd[k].reshape(v.shape) if k in sd else v) for k, v in ref_sd.items()}
    missing = [k for k in sd if k not in ref_sd]
    assert not missing, missing
    m.load_state_dict(full, strict=True)
    return m, ref_sd


def _names(out, tag, ref_sd):
    keys = list(ref_sd)
    out[f"names_{tag}"] = np.array(keys)
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        shapes[i, :ref_sd[k].dim()] = list(ref_sd[k].shape)
    out[f"shapes_{tag}"] = shapes


def _save_deterministic(path, arrays):
    """np.savez with fixed member timestamps, so that regenerating gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    make_golden.install_shim()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    out = {}
    # ---- tiny
    sd = T.synth_ae_state_dict(T.TINY, seed=77)
    m, ref_sd = _model(T.TINY, sd)
    _names(out, "tiny", ref_sd)
    taps = {}
    for name, mod in list(m.encoder.enc.items()):
        mod.register_forward_hook(lambda _m, _i, o, n="encoder.enc." + name: taps.__setitem__(n, o.detach().clone()))
    for i, mod in enumerate(m.decoder):
        mod.register_forward_hook(lambda _m, _i, o, n=f"decoder.{i}": taps.__setitem__(n, o.detach().clone()))
    xa = torch.from_numpy(rng.standard_normal(4101, (2, 2, 16, 16)))
    xb = torch.from_numpy(rng.standard_normal(4102, (1, 2, 32, 16)))
    for tag, x in (("a", xa), ("b", xb)):
        taps.clear()
        means, logvars = m.preencode(x, conditional_inputs=[])
        dec = m.decode(means)
        out[f"tiny_x_{tag}"], out[f"tiny_means_{tag}"], out[f"tiny_logvars_{tag}"], out[f"tiny_decode_{tag}"] = x.numpy(), means.numpy(), logvars.numpy(), dec.numpy()
        if tag == "a":
            for k, v in taps.items():
                out["tiny_tap_" + k] = v[:1, ::2].numpy()   # first image, every other channel: keeps the file small
    # ---- released config, 64 x 64 chunk through the loop of build_encoded_dataset.py:68-94
    sd = T.synth_ae_state_dict(T.RELEASED, seed=78)
    m, ref_sd = _model(T.RELEASED, sd)
    _names(out, "released", ref_sd)
    chunk = rng.standard_normal(4103, (1, 64, 64)) * np.float32(1.7)
    residual = torch.from_numpy(chunk)
    residual = (residual - RES_MEAN) / RES_STD
    input_data = residual.float()
    stack, means8 = [], []
    for horiz_flip in [False, True]:
        for rot_deg in [0, 90, 180, 270]:
            t = input_data
            if horiz_flip:
                t = torch.flip(t, dims=[-1])
            if rot_deg != 0:
                t = torch.rot90(t, k=rot_deg // 90, dims=[-2, -1])
            mu, lv = m.preencode(t[None], conditional_inputs=[])
            stack.append(torch.cat([mu, lv], dim=1)[0].numpy())
            means8.append(mu[0])
    out["rel_chunk"] = chunk
    out["rel_latent_f16"] = np.stack(stack).astype(np.float16)
    means8 = torch.stack(means8)
    out["rel_means"] = means8.numpy()
    out["rel_decode"] = m.decode(means8).numpy()
    path = os.path.join(HERE, "autoencoder.npz")
    _save_deterministic(path, out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
