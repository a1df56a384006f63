"""EDMAutoencoder with the reference's call signature, executed by the HIP engine.

Mirrors terrain_diffusion/models/edm_autoencoder.py:13-158: same constructor kwargs, same state-dict names (diffusers layout),
`preencode` / `postencode` / `decode`, plus `encode_dihedral`, the body of data/preprocessing/build_encoded_dataset.py:68-94 for one chunk
as one engine call.  The encoder-only and the skip-less decoder stacks are two graph kinds of the engine (include/td_ae.h, td_ae_*);
`EDMUnet2D` itself keeps refusing `encode_only` / `noise_emb_dims=0`.
"""
import ctypes as C
import json
import os

import torch

from ._lib import AeConfig, ae_lib as lib, ae_check as check
from .engine import get_engine, ptr, f32
from .unet import DTYPES, EDMUnet2D

_IGNORED_EXACT = ("logvar",)


def _ignored(name):
    """state-dict entries inference never reads: the blocks' unused `emb_gain` (unet_block.py:72 with emb_channels=0), the training-only
    `logvar` (edm_autoencoder.py:105) and the encoder's `logvar_*` (edm_unet.py:142-143)"""
    return name.endswith(".emb_gain") or name in _IGNORED_EXACT or name.startswith("encoder.logvar_")


class EDMAutoencoder:
    def __init__(self, image_size, in_channels, out_channels=None, model_channels=128, model_channel_mults=None, layers_per_block=3,
                 layers_per_block_decoder=None, attn_resolutions=None, midblock_attention=True, logvar_channels=128, block_kwargs=None,
                 conditional_inputs=(), latent_channels=None, n_logvar=1, direct_skips=(),
                 *, dtype="bf16", device="cuda"):
        # refusals first: nothing below may touch the engine before they have fired
        if block_kwargs:
            raise NotImplementedError("block_kwargs are not on the accelerated path")
        if conditional_inputs is not None and len(conditional_inputs) > 0:
            raise NotImplementedError("autoencoder conditional_inputs are not on the accelerated path (the released configs have none)")
        if latent_channels is None:
            raise NotImplementedError("latent_channels must be specified (edm_autoencoder.py:64)")
        mults = list(model_channel_mults or [1, 2, 3, 4])
        lpb = [layers_per_block] * len(mults) if isinstance(layers_per_block, int) else list(layers_per_block)
        lpbd = layers_per_block_decoder or lpb
        lpbd = [lpbd] * len(mults) if isinstance(lpbd, int) else list(lpbd)
        ar = list(attn_resolutions or [])
        ds = [int(c) for c in (direct_skips or [])]
        out_channels = out_channels or in_channels
        L, D = int(latent_channels), len(ds)
        if len(mults) > 8 or len(lpb) != len(mults) or len(lpbd) != len(mults) or len(ar) > 8:
            raise NotImplementedError("at most 8 levels / attention resolutions, one layers_per_block entry per level")
        if not 1 <= L <= 4:
            raise NotImplementedError("latent_channels must be 1..4 (the encoder's output conv writes 2 * latent_channels <= 8 channels)")
        if D > 8 or L + D + 1 > 32:
            raise NotImplementedError("latent_channels + len(direct_skips) + 1 must be <= 32, with at most 8 direct skips")
        if in_channels + 1 > 32:
            raise NotImplementedError("in_channels + 1 must be <= 32")
        if out_channels > 8:
            raise NotImplementedError("out_channels must be <= 8")
        if any(c < 0 or c >= in_channels or c >= out_channels for c in ds):
            raise NotImplementedError("direct_skips must name channels of both the input and the output")
        if any((model_channels * m) % 64 for m in mults):
            raise NotImplementedError("block channels (model_channels * mult) must be multiples of 64")
        self.config = dict(image_size=image_size, in_channels=in_channels, out_channels=out_channels, model_channels=model_channels,
                           model_channel_mults=mults, layers_per_block=lpb, layers_per_block_decoder=lpbd, attn_resolutions=ar,
                           midblock_attention=bool(midblock_attention), logvar_channels=logvar_channels, conditional_inputs=[],
                           latent_channels=L, n_logvar=n_logvar, direct_skips=ds)
        self.dtype = dtype
        self.down = 2 ** (len(mults) - 1)
        self._h = C.c_void_p()
        self._finalized = False
        self.engine = get_engine(device)
        self.device = torch.device("cuda", self.engine.device_id)
        cfg = AeConfig()
        cfg.image_size, cfg.in_channels, cfg.out_channels = image_size, in_channels, out_channels
        cfg.model_channels, cfg.n_levels = model_channels, len(mults)
        for i, m in enumerate(mults):
            cfg.channel_mults[i], cfg.layers_per_block[i], cfg.layers_per_block_decoder[i] = m, lpb[i], lpbd[i]
        cfg.n_attn_resolutions = len(ar)
        for i, r in enumerate(ar):
            cfg.attn_resolutions[i] = r
        cfg.midblock_attention = int(bool(midblock_attention))
        cfg.latent_channels, cfg.n_direct_skips = L, D
        for i, c in enumerate(ds):
            cfg.direct_skips[i] = c
        check(lib().td_ae_create(self.engine._h, C.byref(cfg), DTYPES[dtype], C.byref(self._h)))

    # ---- checkpoint interface
    def expected_parameters(self):
        out = {}
        for i in range(lib().td_ae_num_params(self._h)):
            name, ndim, shape = C.c_char_p(), C.c_int32(), (C.c_int64 * 4)()
            check(lib().td_ae_param_info(self._h, i, C.byref(name), C.byref(ndim), C.byref(shape)))
            out[name.value.decode()] = tuple(shape[k] for k in range(ndim.value))
        return out

    def load_state_dict(self, state_dict, strict=True, fold="reference"):
        """Reference parameter names (EDMAutoencoder.state_dict()).  `*.emb_gain`, `logvar` and `encoder.logvar_*` are accepted and ignored.
        fold: as EDMUnet2D.load_state_dict ("reference": the host folds with the reference's fp32 arithmetic; "engine": fp64 inside the engine);
        gains: encoder.out_gain for encoder.out_conv.weight, out_gain for out_conv.weight, 1 elsewhere."""
        exp = self.expected_parameters()
        missing = [k for k in exp if k not in state_dict]
        unexpected = [k for k in state_dict if k not in exp and not _ignored(k)]
        if strict and (missing or unexpected):
            raise KeyError(f"state dict mismatch: missing {missing[:5]} unexpected {unexpected[:5]}")
        if missing:
            raise ValueError(f"state dict lacks {len(missing)} parameter(s) the model needs, e.g. {missing[:5]}: the engine cannot run on uninitialised weights")
        check(lib().td_ae_set_prefolded(self._h, int(fold == "reference")))
        gains = {"encoder.out_conv.weight": "encoder.out_gain", "out_conv.weight": "out_gain"}
        for k, shape in exp.items():
            w = torch.as_tensor(state_dict[k]).detach().to("cpu", torch.float32).contiguous()
            if tuple(w.shape) != tuple(shape):
                raise ValueError(f"{k}: shape {tuple(w.shape)} != {shape}")
            if fold == "reference" and k.endswith(".weight"):
                gain = torch.as_tensor(state_dict[gains[k]]).to(torch.float32) if k in gains else 1
                w = EDMUnet2D._fold_reference(w, gain).contiguous()
            check(lib().td_ae_set_param(self._h, k.encode(), C.c_void_p(w.data_ptr()), w.numel()))
        check(lib().td_ae_finalize(self._h))
        self._finalized = True
        self._state = {k: state_dict[k] for k in state_dict if k in exp or _ignored(k)}
        return self

    def state_dict(self):
        """The parameters this model was loaded from, under the reference's names (raw values, as a checkpoint holds them)."""
        self._need()
        return dict(self._state)

    def save_pretrained(self, save_directory, **_ignored_kw):
        """diffusers ModelMixin layout: <dir>/config.json with the constructor arguments + <dir>/diffusion_pytorch_model.safetensors."""
        from safetensors.torch import save_file
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(dict(self.config, _class_name="EDMAutoencoder"), f, indent=2, sort_keys=True)
        save_file({k: torch.as_tensor(v).detach().to("cpu", torch.float32).contiguous() for k, v in self.state_dict().items()},
                  os.path.join(save_directory, "diffusion_pytorch_model.safetensors"))

    @classmethod
    def from_pretrained(cls, path, *, dtype="bf16", device="cuda"):
        from safetensors.torch import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
        files = [f for f in os.listdir(path) if f.endswith(".safetensors")]
        if len(files) != 1:
            raise FileNotFoundError(f"expected exactly one .safetensors in {path}")
        m = cls(**cfg, dtype=dtype, device=device)
        return m.load_state_dict(load_file(os.path.join(path, files[0])))

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def close(self):
        if self._h:
            lib().td_ae_destroy(self._h)
            self._h = C.c_void_p()

    def _need(self):
        if not self._finalized or not self._h:
            raise RuntimeError("load_state_dict first")

    # ---- model methods
    def _preencode(self, x, mean, std, dihedral, packed):
        self._need()
        x = f32(x)
        if x.dim() != 4 or x.shape[1] != self.config["in_channels"]:
            raise ValueError(f"x must be (n, {self.config['in_channels']}, H, W), got {tuple(x.shape)}")
        n_src, _, H, W = x.shape
        if H % self.down or W % self.down:
            raise ValueError(f"H and W must be divisible by {self.down}")
        if dihedral and H != W:
            raise ValueError("the dihedral views need a square input")
        n = 8 * n_src if dihedral else n_src
        LD = self.config["latent_channels"] + len(self.config["direct_skips"])
        shape = (n, LD, H // self.down, W // self.down)
        means = torch.empty(shape, dtype=torch.float32, device=x.device)
        logvars = torch.empty(shape, dtype=torch.float32, device=x.device)
        pk = torch.empty((n, 2 * LD) + shape[2:], dtype=torch.float16, device=x.device) if packed else None
        check(lib().td_ae_preencode(self._h, n_src, H, W, ptr(x), float(mean), float(std), int(bool(dihedral)), ptr(means), ptr(logvars), ptr(pk)))
        return means, logvars, pk

    def preencode(self, x, conditional_inputs=None):
        """edm_autoencoder.py:107-123 -> (means, logvars), each (n, latent_channels + len(direct_skips), H / 2^(levels-1), W / 2^(levels-1))."""
        if conditional_inputs is not None and len(conditional_inputs) > 0:
            raise NotImplementedError("autoencoder conditional_inputs are not on the accelerated path")
        m, lv, _ = self._preencode(x, 0.0, 1.0, False, False)
        return m, lv

    def postencode(self, means, logvars, use_mode=False, *, eps=None, seed=None):
        """edm_autoencoder.py:125-130.  The noise is the caller's `eps`, or the package's portable generator keyed by `seed` (noise.standard_normal:
        the same on every machine, which randn_like is not); one of the two is required unless use_mode."""
        if use_mode:
            return means
        if eps is None and seed is None:
            raise ValueError("postencode needs eps=<tensor> or seed=<int>: there is no silent fall-back to torch.randn")
        self._need()
        means, logvars = f32(means), f32(logvars)
        if means.shape != logvars.shape:
            raise ValueError("means and logvars differ in shape")
        if eps is None:
            from .noise import standard_normal
            eps = standard_normal(seed, tuple(means.shape), device=self.device, as_torch=True)
        eps = f32(eps, means.device)
        if eps.shape != means.shape:
            raise ValueError("eps and means differ in shape")
        z = torch.empty_like(means)
        if means.numel():
            check(lib().td_ae_postencode(self._h, means.numel(), ptr(means), ptr(logvars), ptr(eps), ptr(z)))
        return z

    def decode(self, z, include_logvar=False, *, std=1.0, mean=0.0):
        """edm_autoencoder.py:132-158; `std` / `mean` additionally de-normalise the output as `y * std + mean` (two roundings, as torch's)."""
        self._need()
        z = f32(z)
        LD = self.config["latent_channels"] + len(self.config["direct_skips"])
        if z.dim() != 4 or z.shape[1] != LD:
            raise ValueError(f"z must be (n, {LD}, h, w), got {tuple(z.shape)}")
        n, _, h, w = z.shape
        out = torch.empty((n, self.config["out_channels"], h * self.down, w * self.down), dtype=torch.float32, device=z.device)
        check(lib().td_ae_decode(self._h, n, h, w, ptr(z), float(std), float(mean), ptr(out)))
        if include_logvar:
            if "logvar" not in self._state:
                raise KeyError("the loaded checkpoint holds no `logvar`")
            return out, torch.as_tensor(self._state["logvar"]).to(torch.float32).reshape(-1, 1, 1, 1)
        return out

    def read_activation(self, stack, n, H, W, label, max_elems=1 << 26):
        """Debug/test: what `EDMUnet2D.read_activation` gives, on one of the two stacks (1 the encoder, 2 the decoder), from the last preencode / decode
        with this batch and map.  H, W are that stack's own input map (the image for the encoder, the latent for the decoder); `label` is a conv or
        attention op, "sumsq:<label>" or "@xin".  NCHW fp32 (host)."""
        import numpy as np
        self._need()
        buf = np.empty(max_elems, dtype=np.float32)
        dims = (C.c_int32 * 4)()
        check(lib().td_ae_read_activation(self._h, int(stack), n, H, W, label.encode(), C.c_void_p(buf.ctypes.data), buf.size, C.byref(dims)))
        shape = tuple(dims)
        return torch.from_numpy(buf[:int(np.prod(shape))].reshape(shape).copy())

    def preencode_dihedral(self, residual, residual_mean=0.0, residual_std=1.1678):
        """The 8 dihedral views of one chunk through preencode in one engine call -> (means, logvars, packed): fp32 (8, L + D, h, w) twice and
        cat(means, logvars) as float16."""
        x = f32(residual)
        while x.dim() < 4:
            x = x[None]
        if x.dim() != 4 or x.shape[0] != 1:
            raise ValueError("one chunk: (C, S, S)")
        return self._preencode(x.contiguous(), residual_mean, residual_std, True, True)

    def encode_dihedral(self, residual, residual_mean=0.0, residual_std=1.1678):
        """build_encoded_dataset.py:68-94 for one chunk: (C, S, S) or (1, C, S, S) fp32 residual -> (8, 2 (L + D), S / down, S / down) float16, the 8
        views 4 * flip + r of the normalised chunk through preencode, cat(means, logvars), rounded to fp16 -- one engine call on a batch of 8.
        HDF5 reading and writing stay with the caller."""
        return self.preencode_dihedral(residual, residual_mean, residual_std)[2]
