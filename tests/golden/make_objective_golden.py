"""Generates tests/golden/objective.npz by RUNNING THE REFERENCE'S OWN CODE: DiffusionTrainer.train_step itself
(terrain_diffusion/training/trainers/diffusion.py) on a stand-in `self` around the reference's EDMUnet2D, the nested calc_loss of
training/dev_utils/noise_loss_curve.py, and DiffusionTrainer._normalize_and_process_terrain.

Needs a checkout of the reference and torch; the fixture needs neither.  trainers/diffusion.py, models/edm_unet.py, unet_block.py and
mp_layers.py are loaded by path; ema_pytorch, torchmetrics, tqdm, diffusers and the rest of the reference's package are stub modules in
sys.modules, as make_train_data_golden.py and make_golden.py do.  The stand-in's accelerator is a no-op, backward and step are stubs, the
model is the reference's EDMUnet2D with the oracle's tiny_config, its weights oracle.unet.synth_state_dict's.  torch.randn / randn_like are
wrapped to record every draw in order; the model's forward and _calc_loss are wrapped to record x, cnoise, model_output, logvar, pred_v_t, v_t
and the loss; torch.atan, cos, sin and std are wrapped to record the locals sigma / sigma_data, cos t, sin t and the std.  calc_loss is taken
out of noise_loss_curve.py's AST (the module's imports need click, confection, matplotlib) and run on a recorded pred_v_t, v_t with and
without loss_groups.  Only inputs, draws, outputs and library versions are stored, never source text:

    python tests/golden/make_objective_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

train_step puts the model in train mode, which re-normalises every weight in place (mp_layers.py:206-208) before the forward uses it: the
state dict AFTER the step is the one the forward used.  The whole dict is 40 MB, so it is stored as what rebuilds it from
synth_state_dict(cfg, seed): every re-normalised tensor is w0 / den with one fp32 scalar den per tensor (asserted here bit for bit), and the
fixture keeps den and the CRC-32 of the result; the logvar head's three tensors are stored whole, with the folded weight the forward used.

Arrays (cases json lists name, Cc, scale, sigma_data, K, seed, P_mean, P_std, eps, channels, N, C, H, W):
  <c>_image, _cond_img, _cond_inputs        the batch;            <c>_d_z, _d_noise      the draws, in order
  <c>_ratio, _t, _cos, _sin, _std           the reference's sigma / sigma_data, cnoise, cos t, sin t, std (fp32)
  <c>_x, _model_output, _logvar, _pred_v_t, _v_t, _loss          what forward and _calc_loss saw and returned
  <c>_lv_freqs, _lv_phases, _lv_weight, _lv_wfold                the logvar head after the step, and its folded weight
  <c>_state_den, _state_crc (cases[c]["state_names"])            the rest of the state dict after the step
  <c>_f64_<q>, <c>_eref_<q>                 the float64 companion of q in sigma, t, cos, sin, std, logvar, loss and e_ref = |reference - float64|
  curve_plain, curve_g14, curve_g23 (+ _f64, _eref)               calc_loss on case c0's pred_v_t, v_t
  terrain, terrain_u8                       _normalize_and_process_terrain's input and bytes
  versions json.

The generator asserts what the tests lean on: no uint8 pre-truncation value within 2 ulp of an integer; std / sigma_data not within 1 ulp of
eps; every e_ref small (the reference is fp32: a criterion of e_ref + 1 ulp would be vacuous otherwise); the twin's bytes equal the
reference's on a wide-range terrain too (not stored: its extremes sit on 0 and 255).
"""
import argparse
import ast
import contextlib
import importlib.util
import json
import math
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _objective_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "objective.npz")
F, D = np.float32, np.float64
N, C, H, W = 3, 5, 16, 16
P_MEAN, P_STD, EPS = -0.4, 1.0, 0.05
CHANNELS = [0, 1, 2, 3]
CASES = (dict(name="c0", Cc=2, scale=False, sigma_data=0.5, K=128, seed=101),
         dict(name="c1", Cc=0, scale=True, sigma_data=1.0, K=130, seed=102),
         dict(name="c2", Cc=2, scale=True, sigma_data=0.5, K=130, seed=103),
         dict(name="c3", Cc=0, scale=False, sigma_data=1.0, K=128, seed=104))


# ------------------------------------------------------------------------------------------------------------------------------ the reference
def install_stubs(torch):
    import functools
    import inspect

    class _Cfg(dict):
        __getattr__ = dict.get

    class ConfigMixin:
        config = property(lambda self: self._cfg)

    def register_to_config(init):
        @functools.wraps(init)
        def wrap(self, *a, **kw):
            ba = inspect.signature(init).bind(self, *a, **kw)
            ba.apply_defaults()
            self.__dict__.setdefault("_cfg", _Cfg()).update({k: v for k, v in ba.arguments.items() if k != "self"})
            init(self, *a, **kw)
        return wrap

    class ModelMixin(torch.nn.Module):
        pass

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("diffusers", ConfigMixin=ConfigMixin)
    mod("diffusers.configuration_utils", ConfigMixin=ConfigMixin, register_to_config=register_to_config)
    mod("diffusers.models")
    mod("diffusers.models.modeling_utils", ModelMixin=ModelMixin)
    mod("tqdm", tqdm=lambda it=None, **kw: it)
    mod("ema_pytorch", PostHocEMA=object)
    mod("torchmetrics")
    mod("torchmetrics.image")
    mod("torchmetrics.image.kid", KernelInceptionDistance=object)
    for name in ("terrain_diffusion", "terrain_diffusion.models", "terrain_diffusion.training", "terrain_diffusion.training.trainers", "terrain_diffusion.data"):
        mod(name)
    mod("terrain_diffusion.training.trainers.trainer", Trainer=object)
    mod("terrain_diffusion.models.edm_autoencoder", EDMAutoencoder=object)
    mod("terrain_diffusion.data.laplacian_encoder", laplacian_denoise=None, laplacian_decode=None)
    mod("terrain_diffusion.training.utils", recursive_to=None, temporary_ema_to_model=None)
    mod("terrain_diffusion.training.datasets", LongDataset=object)


def load(reference, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(reference, "terrain_diffusion", *rel))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class Recorder:
    """wraps functions of the torch module while a step runs: every call's result (and for atan its argument) is kept in order"""

    NAMES = ("randn", "randn_like", "atan", "cos", "sin", "std")

    def __init__(self, torch):
        self.torch, self.calls = torch, []
        self.orig = {n: getattr(torch, n) for n in self.NAMES}

    def __enter__(self):
        for n in self.NAMES:
            setattr(self.torch, n, self.wrap(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.torch, n, f)
        return False

    def wrap(self, name):
        def f(*a, **k):
            r = self.orig[name](*a, **k)
            self.calls.append((name, a[0].detach().clone() if name == "atan" else None, r.detach().clone()))
            return r
        return f

    def first(self, name, arg=False):
        for n, a, r in self.calls:
            if n == name:
                return (a if arg else r).numpy()
        return None


class NoOpAccelerator:
    sync_gradients = False
    is_main_process = False

    def accumulate(self, model):
        return contextlib.nullcontext()

    def autocast(self):
        return contextlib.nullcontext()

    def backward(self, loss):
        pass


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def ulps(e, ref):
    return float(np.max(np.asarray(e, dtype=D) / twin.ulp32(ref)))


# ------------------------------------------------------------------------------------------------------------------------------ one case
def run_case(torch, ref, case, out):
    from oracle.unet import synth_state_dict, tiny_config
    name, Cc, sd, K = case["name"], case["Cc"], case["sigma_data"], case["K"]
    cfg = tiny_config(64, 1, in_channels=C + Cc, out_channels=C)
    rng = np.random.default_rng(case["seed"])
    image = (rng.standard_normal((N, C, H, W)) * 0.6).astype(F)
    if case["scale"]:
        image[2, :4] *= F(0.02)                   # std / sigma_data below eps: the floor holds for this item
    batch = {"image": torch.from_numpy(image), "cond_inputs": [torch.from_numpy(rng.standard_normal((N, 58)).astype(F))]}
    if Cc:
        batch["cond_img"] = torch.from_numpy(rng.standard_normal((N, Cc, H, W)).astype(F))
    torch.manual_seed(case["seed"])
    model = ref["unet"].EDMUnet2D(**cfg, logvar_channels=K)
    sd0 = synth_state_dict(cfg, seed=case["seed"])
    missing, unexpected = model.load_state_dict(sd0, strict=False)
    assert not unexpected and all(k.startswith("logvar_") for k in missing), (missing, unexpected)
    rec = {}
    fwd = model.forward

    def forward(x, noise_labels, conditional_inputs, return_logvar=False, **kw):
        r = fwd(x, noise_labels=noise_labels, conditional_inputs=conditional_inputs, return_logvar=return_logvar, **kw)
        rec.update(x=x.detach().clone(), cnoise=noise_labels.detach().clone(), model_output=r[0].detach().clone(), logvar=r[1].detach().clone())
        return r
    model.forward = forward
    Trainer = ref["diffusion"].DiffusionTrainer
    this = types.SimpleNamespace()

    def calc_loss(self_, pred_v_t, v_t, logvar, sigma_data):
        loss = Trainer._calc_loss(self_, pred_v_t, v_t, logvar, sigma_data)
        rec.update(pred_v_t=pred_v_t.detach().clone(), v_t=v_t.detach().clone(), loss=loss.detach().clone())
        return loss
    training = {"P_std": P_STD, "P_mean": P_MEAN}
    if case["scale"]:
        training.update(scale_sigma=True, scaling_channels=CHANNELS, sigma_scale_eps=EPS)
    this.accelerator, this.config, this.model = NoOpAccelerator(), {"training": training}, model
    this.scheduler = types.SimpleNamespace(config=types.SimpleNamespace(sigma_data=sd))
    this.resolved = {"lr_sched": types.SimpleNamespace(get=lambda seen: 1e-4)}
    this.optimizer = types.SimpleNamespace(param_groups=[{}], zero_grad=lambda: None, step=lambda: None)
    this.ema = types.SimpleNamespace(update=lambda: None)
    this._calc_loss = types.MethodType(calc_loss, this)
    with Recorder(torch) as r:
        res = Trainer.train_step(this, {"seen": 0, "step": 0}, batch)
    draws = [c for c in r.calls if c[0] in ("randn", "randn_like")]
    assert [c[0] for c in draws] == ["randn", "randn_like"] and tuple(draws[0][2].shape) == (N,) and tuple(draws[1][2].shape) == (N, C, H, W)
    assert res["loss"] == float(rec["loss"])
    z, noise = draws[0][2].numpy(), draws[1][2].numpy()
    ratio = r.first("atan", arg=True).reshape(-1)
    q = dict(image=image, cond_inputs=batch["cond_inputs"][0].numpy(), d_z=z, d_noise=noise, ratio=ratio, t=rec["cnoise"].numpy(),
             cos=r.first("cos").reshape(-1), sin=r.first("sin").reshape(-1), x=rec["x"].numpy(), model_output=rec["model_output"].numpy(),
             logvar=rec["logvar"].numpy().reshape(-1), pred_v_t=rec["pred_v_t"].numpy(), v_t=rec["v_t"].numpy(), loss=rec["loss"].numpy().reshape(1))
    if Cc:
        q["cond_img"] = batch["cond_img"].numpy()
    if case["scale"]:
        q["std"] = r.first("std").reshape(-1)
    assert q["t"].dtype == F and q["loss"].dtype == F
    # ---- the state after the step
    post = {k: v.detach().clone() for k, v in model.state_dict().items()}
    names, den, crcs = [], [], []
    for k, w0 in sd0.items():
        w0 = torch.as_tensor(w0).to(torch.float32)
        if torch.equal(post[k], w0):
            d = 1.0
        else:
            norm = torch.add(1e-4, torch.linalg.vector_norm(w0), alpha=np.sqrt(1 / w0.numel()))
            assert torch.equal(post[k], w0 / norm) and np.array_equal((w0.numpy() / F(norm)).astype(F), post[k].numpy()), k
            d = float(norm)
        names.append(k); den.append(d); crcs.append(crc(post[k].numpy()))
    q.update(state_den=np.array(den, dtype=F), state_crc=np.array(crcs, dtype=np.uint32))
    lw = post["logvar_linear.weight"]
    wfold = ref["mp"].normalize(lw.to(torch.float32)) * (1 / np.sqrt(lw[0].numel()))
    q.update(lv_freqs=post["logvar_fourier.freqs"].numpy(), lv_phases=post["logvar_fourier.phases"].numpy(), lv_weight=lw.numpy(), lv_wfold=wfold.numpy())
    # ---- float64 companions, by this file's own arithmetic (not the twin's)
    sd64, z64 = float(F(sd)), z.astype(D)
    sigma = np.exp(z64 * float(F(P_STD)) + float(F(P_MEAN)))
    f64 = {}
    if case["scale"]:
        std = np.empty(N)
        for n in range(N):
            v = [float(a) for a in image[n, CHANNELS].reshape(-1)]
            m = math.fsum(v) / len(v)
            std[n] = math.sqrt(math.fsum((a - m) ** 2 for a in v) / (len(v) - 1))
        f64["std"] = std
        rr = std / sd64
        assert np.all(np.abs(rr - float(F(EPS))) > twin.ulp32(rr)), "std / sigma_data within 1 ulp of eps: change the seed"
        assert (rr < float(F(EPS))).any() and (rr > float(F(EPS))).any(), "both sides of the floor must occur"
        sigma = sigma * np.maximum(rr, float(F(EPS)))
    t32 = np.arctan(sigma / sd64).astype(F)
    t64 = t32.astype(D)
    f64.update(sigma=sigma, t=np.arctan(sigma / sd64), cos=np.cos(t64), sin=np.sin(t64))
    xlv32 = np.log(np.tan(t64) / 8.0).astype(F)
    y = ((xlv32[:, None] * q["lv_freqs"][None, :]).astype(F) + q["lv_phases"][None, :]).astype(F)
    f64["logvar"] = np.array([math.fsum(r_) for r_ in np.cos(y.astype(D)) * math.sqrt(2.0) * q["lv_wfold"].astype(D).reshape(1, -1)])
    d = (q["pred_v_t"] - q["v_t"]).astype(F).astype(D)                     # the reference's own fp32 difference; its square is exact in float64
    lv = q["logvar"].astype(D)
    per = [math.fsum(float(a) ** 2 for a in d[n].reshape(-1)) / (C * H * W) / (math.exp(lv[n]) * sd64 ** 2) + lv[n] for n in range(N)]
    f64["loss"] = np.array([math.fsum(per) / N])
    refs = dict(sigma=ratio.astype(D) * sd64, t=q["t"], cos=q["cos"], sin=q["sin"], logvar=q["logvar"], loss=q["loss"])
    if case["scale"]:
        refs["std"] = q["std"]
    for k, v in f64.items():
        e = np.abs(np.asarray(refs[k], dtype=D) - v)
        q["f64_" + k], q["eref_" + k] = v, e
        limit = {"logvar": 4096.0, "sigma": 64.0}.get(k, 16.0)            # logvar: an ulp of x_lv times |f| up to 20, over sum |w| about sqrt(K)
        assert ulps(e, v) <= limit, (name, k, ulps(e, v))
        print(f"  {name} e_ref({k}) <= {ulps(e, v):.2f} ulp")
    for k, v in q.items():
        out[f"{name}_{k}"] = v
    return dict(case, P_mean=P_MEAN, P_std=P_STD, eps=EPS, channels=CHANNELS if case["scale"] else None, N=N, C=C, H=H, W=W, state_names=names, cfg=cfg), q


# ------------------------------------------------------------------------------------------------------------------------------ calc_loss
def curve_losses(torch, reference, q, sd, out):
    path = os.path.join(reference, "terrain_diffusion", "training", "dev_utils", "noise_loss_curve.py")
    tree = ast.parse(open(path).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "calc_loss")
    pred, v = torch.from_numpy(q["pred_v_t"]), torch.from_numpy(q["v_t"])
    d = (q["pred_v_t"] - q["v_t"]).astype(F).astype(D)
    S = np.array([[math.fsum(float(a) ** 2 for a in d[n, c].reshape(-1)) for c in range(C)] for n in range(N)])
    sd2 = float(F(sd)) ** 2
    for key, groups in (("plain", None), ("g14", [1, 4]), ("g23", [2, 3])):
        ns = {"torch": torch, "config": {"training": {} if groups is None else {"loss_groups": groups}}}
        exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
        r = ns["calc_loss"](pred, v, None, sd).numpy().reshape(1)
        if groups is None:
            f = math.fsum(S.reshape(-1)) / (N * C * H * W) / sd2
        else:
            c, g = 0, []
            for k in groups:
                g.append(math.fsum(S[:, c:c + k].reshape(-1)) / (N * k * H * W) / sd2)
                c += k
            f = math.fsum(g) / len(g)
        out["curve_" + key], out["curve_" + key + "_f64"], out["curve_" + key + "_eref"] = r, np.array([f]), np.abs(r.astype(D) - f)
        assert ulps(np.abs(r.astype(D) - f), f) <= 16.0, key
        print(f"  calc_loss {key}: {float(r[0]):.7g}, e_ref {ulps(np.abs(r.astype(D) - f), f):.2f} ulp")


# ------------------------------------------------------------------------------------------------------------------------------ terrain
def terrain_case(torch, ref, out, seed=7):
    rng = np.random.default_rng(seed)
    t = np.empty((4, 1, H, W), dtype=F)
    t[0] = (rng.random((1, H, W)) * 100.0 + 20.0).astype(F)              # range 100: floored at 255
    t[1] = (rng.standard_normal((1, H, W)) * 30.0 - 400.0).astype(F)      # negative elevations, range about 200
    t[2] = F(1234.5)                                                     # all equal: range 0, every byte 127
    t[3] = (rng.random((1, H, W)) * 254.0).astype(F)                      # range just below the floor
    fn = ref["diffusion"].DiffusionTrainer._normalize_and_process_terrain
    got = fn(None, torch.from_numpy(t)).numpy()
    mine, pre = twin.terrain_u8(t)
    assert got.dtype == np.uint8 and got.shape == (4, 3, H, W) and np.array_equal(mine, got)
    near = np.abs(pre - np.rint(pre)) <= 2.0 * twin.ulp32(np.maximum(np.abs(pre), np.abs(np.rint(pre))))
    assert not near.any(), "a pre-truncation value within 2 ulp of an integer: change the seed"
    assert all(float(t[n].max() - t[n].min()) < 255.0 for n in range(4))
    wide = (rng.standard_normal((2, 2, H, W)) * 900.0 + 300.0).astype(F)   # range above 255, two channels: checked here, not stored
    assert np.array_equal(twin.terrain_u8(wide)[0], fn(None, torch.from_numpy(wide)).numpy())
    out["terrain"], out["terrain_u8"] = t, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference PATH (or TD_REFERENCE) is required")
    import torch
    torch.set_num_threads(1)
    install_stubs(torch)
    ref = {"mp": load(args.reference, ("models", "mp_layers.py"), "terrain_diffusion.models.mp_layers")}
    load(args.reference, ("models", "unet_block.py"), "terrain_diffusion.models.unet_block")
    ref["unet"] = load(args.reference, ("models", "edm_unet.py"), "terrain_diffusion.models.edm_unet")
    ref["diffusion"] = load(args.reference, ("training", "trainers", "diffusion.py"), "terrain_diffusion.training.trainers.diffusion")
    out, cases, first = {}, [], None
    for case in CASES:
        print(case["name"])
        meta, q = run_case(torch, ref, case, out)
        cases.append(meta)
        first = first or (q, case["sigma_data"])
    curve_losses(torch, args.reference, first[0], first[1], out)
    terrain_case(torch, ref, out)
    out["cases"] = np.array(json.dumps(cases))
    out["versions"] = np.array(json.dumps({"torch": torch.__version__, "numpy": np.__version__, "python": sys.version.split()[0]}))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
