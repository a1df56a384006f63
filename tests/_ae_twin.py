"""Float64 restatement of the reference's EDMAutoencoder (terrain_diffusion/models/edm_autoencoder.py:13-158) for the tests: parameter shapes,
a seeded synthetic state dict, preencode / postencode / decode.  Folded weights and the block arithmetic come from oracle.unet."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rng
from oracle.unet import _name_seed, fold_weight, mp_silu, mp_sum2, normalize

TINY = dict(image_size=16, in_channels=2, model_channels=64, model_channel_mults=[1, 2], layers_per_block=1, midblock_attention=True,
            latent_channels=2, direct_skips=[1])
RELEASED = dict(image_size=512, in_channels=1, out_channels=1, model_channels=64, model_channel_mults=[1, 2, 4, 4], layers_per_block=2,
                attn_resolutions=[], midblock_attention=False, latent_channels=4, conditional_inputs=[],
                direct_skips=[])   # configs/autoencoder/autoencoder_x8.cfg:43-59


def is_ignored(name):
    """state-dict entries inference never reads (unet_block.py:72 without an embedding; edm_autoencoder.py:105; edm_unet.py:142-143)"""
    return name.endswith(".emb_gain") or name == "logvar" or name.startswith("encoder.logvar_")


def _lists(cfg):
    mults = list(cfg.get("model_channel_mults") or [1, 2, 3, 4])
    lpb = cfg.get("layers_per_block", 3)
    lpb = [lpb] * len(mults) if isinstance(lpb, int) else list(lpb)
    lpbd = cfg.get("layers_per_block_decoder") or lpb
    lpbd = [lpbd] * len(mults) if isinstance(lpbd, int) else list(lpbd)
    return mults, lpb, lpbd


def ae_plan(cfg):
    """Blocks in execution order: edm_unet.py:107-121 (encode_only) and edm_autoencoder.py:87-101, under the state-dict prefixes."""
    mults, lpb, lpbd = _lists(cfg)
    mc, size, attn_res = cfg["model_channels"], cfg["image_size"], cfg.get("attn_resolutions") or []
    chans = [mc * m for m in mults]
    enc, dec = [], []
    cout = cfg["in_channels"] + 1
    for level, (ch, nb) in enumerate(zip(chans, lpb)):
        res = size // 2 ** level
        if level == 0:
            enc.append(dict(name=f"encoder.enc.{res}x{res}_conv", kind="conv", cin=cout, cout=ch))
            cout = ch
        else:
            enc.append(dict(name=f"encoder.enc.{res}x{res}_down", kind="block", mode="enc", cin=cout, cout=cout, resample="down", attn=False))
        for idx in range(nb):
            cin, cout = cout, ch
            enc.append(dict(name=f"encoder.enc.{res}x{res}_block{idx}", kind="block", mode="enc", cin=cin, cout=cout, resample="keep", attn=res in attn_res))
    enc_c = cout
    cout = chans[-1]

    def push(cin, co, resample, attn):
        dec.append(dict(name=f"decoder.{len(dec)}", kind="block", mode="dec", cin=cin, cout=co, resample=resample, attn=attn))
    for level, (ch, nb) in reversed(list(enumerate(zip(chans, lpbd)))):
        res = size // 2 ** level
        if level == len(chans) - 1:
            push(cout, cout, "keep", bool(cfg.get("midblock_attention", True)))
            push(cout, cout, "keep", False)
        else:
            push(cout, cout, "up", False)
        for _ in range(nb + 1):
            push(cout, ch, "keep", res in attn_res)
            cout = ch
    return dict(enc=enc, dec=dec, enc_c=enc_c, dec_c0=chans[-1], final_c=cout, down=2 ** (len(mults) - 1))


def ae_param_shapes(cfg):
    """Ordered {name: shape} of every tensor inference reads (the reference's state-dict names without the ignored keys)."""
    plan = ae_plan(cfg)
    L, D = cfg["latent_channels"], len(cfg.get("direct_skips") or [])
    sh = OrderedDict()

    def block(b):
        n = b["name"]
        if b["kind"] == "conv":
            sh[n + ".weight"] = (b["cout"], b["cin"], 3, 3)
            return
        sh[n + ".conv_res0.weight"] = (b["cout"], b["cout"] if b["mode"] == "enc" else b["cin"], 3, 3)
        sh[n + ".conv_res1.weight"] = (b["cout"], b["cout"], 3, 3)
        if b["cin"] != b["cout"]:
            sh[n + ".conv_skip.weight"] = (b["cout"], b["cin"], 1, 1)
        if b["attn"]:
            sh[n + ".attn_qkv.weight"] = (3 * b["cout"], b["cout"], 1, 1)
            sh[n + ".attn_proj.weight"] = (b["cout"], b["cout"], 1, 1)
    for b in plan["enc"]:
        block(b)
    sh["encoder.out_conv.weight"] = (2 * L, plan["enc_c"], 3, 3)
    sh["encoder.out_gain"] = ()
    sh["decoder_conv.weight"] = (plan["dec_c0"], L + D + 1, 1, 1)
    for b in plan["dec"]:
        block(b)
    sh["out_conv.weight"] = (cfg.get("out_channels") or cfg["in_channels"], plan["final_c"], 3, 3)
    sh["out_gain"] = ()
    return sh


def synth_ae_state_dict(cfg, seed=77, enc_out_gain=0.8, out_gain=0.3, emb_gain=0.37):
    """Seeded synthetic checkpoint from the portable rng (as oracle.unet.synth_state_dict): non-trivial gains, and the keys inference must IGNORE
    present with non-zero values (every block's emb_gain, logvar) so that a build which wrongly uses them is caught."""
    sd = OrderedDict()
    for name, shape in ae_param_shapes(cfg).items():
        if name == "encoder.out_gain":
            sd[name] = torch.tensor(float(enc_out_gain))
        elif name == "out_gain":
            sd[name] = torch.tensor(float(out_gain))
        else:
            sd[name] = torch.from_numpy(rng.standard_normal(_name_seed(name, seed), shape))
    plan = ae_plan(cfg)
    for b in plan["enc"] + plan["dec"]:
        if b["kind"] == "block":
            sd[b["name"] + ".emb_gain"] = torch.tensor(float(emb_gain))
    sd["logvar"] = torch.tensor([0.25])
    return sd


class AETwin:
    """Folded-weight functional EDMAutoencoder in `dtype` (float64 for the bounds, float32 for a like-for-like look)."""

    def __init__(self, cfg, state_dict, dtype=torch.float64):
        self.cfg, self.plan, self.dtype = cfg, ae_plan(cfg), dtype
        self.L, self.ds = cfg["latent_channels"], list(cfg.get("direct_skips") or [])
        gains = {"encoder.out_conv.weight": "encoder.out_gain", "out_conv.weight": "out_gain"}
        self.w = {}
        for name in ae_param_shapes(cfg):
            if name.endswith(".weight"):
                g = float(state_dict[gains[name]]) if name in gains else 1.0
                self.w[name[:-len(".weight")]] = fold_weight(torch.as_tensor(state_dict[name]), g).to(dtype)

    # unet_block.py:102-108
    def _attn(self, x, n):
        heads = x.shape[1] // 64
        y = F.conv2d(x, self.w[n + ".attn_qkv"])
        y = y.reshape(y.shape[0], heads, -1, 3, y.shape[2] * y.shape[3])
        q, k, v = normalize(y, dim=2).unbind(3)
        w = torch.einsum("nhcq,nhck->nhqk", q, k / np.sqrt(q.shape[2])).softmax(dim=3)
        y = torch.einsum("nhqk,nhck->nhcq", w, v)
        return F.conv2d(y.reshape(*x.shape), self.w[n + ".attn_proj"])

    # unet_block.py:116-156 with emb_linear None (:133-134): y = mp_silu(y)
    def _block(self, b, x):
        n = b["name"]
        if b["resample"] == "down":
            x = x[:, :, ::2, ::2]      # mp_layers.resample 'down' as oracle.unet restates it
        elif b["resample"] == "up":
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        if b["mode"] == "enc":
            if b["cin"] != b["cout"]:
                x = F.conv2d(x, self.w[n + ".conv_skip"])
            x = normalize(x, dim=1)
        y = F.conv2d(mp_silu(x), self.w[n + ".conv_res0"], padding=1)
        y = mp_silu(y)
        y = F.conv2d(y, self.w[n + ".conv_res1"], padding=1)
        if b["mode"] == "dec" and b["cin"] != b["cout"]:
            x = F.conv2d(x, self.w[n + ".conv_skip"])
        x = mp_sum2(x, y, 0.3)
        if b["attn"]:
            x = mp_sum2(x, self._attn(x, n), 0.3)
        return torch.clip(x, -256, 256)

    # edm_autoencoder.py:107-123
    def preencode(self, x, taps=None):
        x = torch.as_tensor(x).to(self.dtype)
        y = torch.cat([x, torch.ones_like(x[:, :1])], dim=1)
        for b in self.plan["enc"]:
            y = F.conv2d(y, self.w[b["name"]], padding=1) if b["kind"] == "conv" else self._block(b, y)
            if taps is not None:
                taps[b["name"]] = y
        enc = F.conv2d(y, self.w["encoder.out_conv"], padding=1)
        means, logvars = enc[:, :self.L], enc[:, self.L:]
        s = self.plan["down"]
        pooled = [x[:, c:c + 1].reshape(x.shape[0], 1, x.shape[2] // s, s, x.shape[3] // s, s).mean(dim=(3, 5)) for c in self.ds]
        means = torch.cat([means] + pooled, dim=1)
        logvars = torch.cat([logvars, torch.full((x.shape[0], len(self.ds)) + tuple(logvars.shape[2:]), -20.0, dtype=self.dtype)], dim=1)
        return means, logvars

    # edm_autoencoder.py:125-130 with the noise as an argument
    @staticmethod
    def postencode(means, logvars, eps):
        means, logvars, eps = (torch.as_tensor(t).to(torch.float64) for t in (means, logvars, eps))
        return means + eps * torch.exp(logvars * 0.5)

    # edm_autoencoder.py:132-158
    def decode(self, z, taps=None):
        z = torch.as_tensor(z).to(self.dtype)
        direct = z[:, self.L:]
        y = F.conv2d(torch.cat([z, torch.ones_like(z[:, :1])], dim=1), self.w["decoder_conv"])
        for b in self.plan["dec"]:
            y = self._block(b, y)
            if taps is not None:
                taps[b["name"]] = y
        out = F.conv2d(y, self.w["out_conv"], padding=1).clone()
        s = self.plan["down"]
        for i, c in enumerate(self.ds):
            out[:, c] = direct[:, i].repeat_interleave(s, dim=1).repeat_interleave(s, dim=2)
        return out


def dihedral_views(x):
    """build_encoded_dataset.py:75-81: the 8 views of x (..., S, S), view 4 * flip + r = rot90(flip(x, [-1]) if flip else x, k=r)"""
    out = []
    for flip in (False, True):
        for r in range(4):
            t = torch.flip(x, dims=[-1]) if flip else x
            out.append(torch.rot90(t, k=r, dims=[-2, -1]) if r else t)
    return out


def rel_rms(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
