"""The validation objective on the GPU: what the reference does with a batch and a checkpoint, forward half only.

The reference computes its training objective in three places -- DiffusionTrainer.train_step and .evaluate (training/trainers/diffusion.py:
103-171, 371-407), training/dev_utils/noise_loss_curve.py:69-133 and _normalize_and_process_terrain (diffusion.py:173-182).  Here the trigflow
noising in front of the U-Net, the model's return_logvar head and the uncertainty-weighted v-loss behind the U-Net are launches of
libtd_objective.so (include/td_objective.h, objective_csrc/) on the engine's stream; the U-Net between them is td_unet_forward.  There is no
CPU fallback.  Backward passes, the optimizer, EMA and the Inception network of KID are not here.

  device forms   noise_levels, add_noise, logvar, squared_error, v_loss, terrain_uint8: device tensors in and out; only v_loss's scalar is
                 read back;
  the model      EDMUnet2D.__call__(..., return_logvar=True) returns (out, logvar) with logvar shaped (n, 1, 1, 1);
  drop-ins       validation_loss (the loop of evaluate, `val/loss`) and noise_loss_curve (the arrays; it does not plot).

Read-backs.  td_unet_forward takes noise_labels from the host, so a drop-in reads the column t of the level table back once per batch (4 N
bytes), and the scalar loss once per batch (8 bytes), as the reference's loss.item() does.  Nothing else leaves the device.

Stated, not reproduced:
  * fp32 only: under autocast the reference runs the logvar linear in bf16; that rounding is not reproduced.
  * n_logvar != 1 raises NotImplementedError: the reference's reshape(-1, 1, 1, 1) only broadcasts for 1.
  * The caller supplies the draws (or a torch.Generator the drop-ins draw from in the reference's order: randn(N) for sigma, then
    randn(images.shape)); the portable generator is not used here.
  * The bound the logvar head is tested against takes sinf / cosf at 4 ulp: that is the OpenCL full-profile SPECIFICATION of the device math
    library, not a measurement.
"""
import collections
import collections.abc
import ctypes as C

import numpy as np
import torch

from ._lib import Library
from ._plumbing import call, engine_for as _engine_for

_P = C.c_void_p
_F = C.c_float
_I = C.c_int
_SIGS = {
    "td_objective_last_error": (C.c_char_p, []),
    "td_objective_levels": (_I, [_P, _I, _P, _I, _F, _F, _F, _P, _I, _I, _I, _P, _I, _F, _P, _I]),
    "td_objective_noise": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _I]),
    "td_objective_logvar": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _P, _I]),
    "td_objective_sqerr": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _I]),
    "td_objective_loss": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _I, _P, _P, _P, _I]),
    "td_objective_terrain_u8": (_I, [_P, _P, _I, _I, _I, _I, _P, _I]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_objective.so", _SIGS, "td_objective_last_error", "td_objective")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

LEVEL_COLS = 6              # include/td_objective.h TD_OBJECTIVE_LEVEL_COLS: sigma, t, cos t, sin t, x_lv, std
MAX_ITEMS = 65536           # TD_OBJECTIVE_MAX_ITEMS
MAX_CHANNELS = 1024         # TD_OBJECTIVE_MAX_CHANNELS
MAX_SIDE = 65536            # TD_OBJECTIVE_MAX_SIDE
MAX_LOGVAR = 1024           # TD_OBJECTIVE_MAX_LOGVAR
MAX_LIST = 64               # TD_OBJECTIVE_MAX_LIST
MODES = {"draw": 0, "sigma": 1, "t": 2}                         # TD_OBJECTIVE_MODE_*
FORMS = {"weighted": 0, "plain": 1, "grouped": 2}               # TD_OBJECTIVE_LOSS_*

VLoss = collections.namedtuple("VLoss", "value items loss64 loss32")


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(x, what, dtype=torch.float32):
    """a contiguous device tensor of `dtype`; the device forms take no host arrays"""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise ValueError(f"{what} must be a device tensor (the device forms take no host arrays)")
    return x.detach().to(dtype).contiguous()


def _nchw(x, what):
    x = _dev(x, what)
    if x.dim() != 4:
        raise ValueError(f"{what} must be (N, C, H, W), got {tuple(x.shape)}")
    N, Cn, H, W = (int(d) for d in x.shape)
    if N < 1 or Cn < 1 or H < 1 or W < 1:
        raise ValueError(f"empty {what}: {tuple(x.shape)}")
    if N > MAX_ITEMS or Cn > MAX_CHANNELS or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what} {tuple(x.shape)} beyond the library's limit (N <= {MAX_ITEMS}, C <= {MAX_CHANNELS}, H, W <= {MAX_SIDE})")
    return x


def _table(table, N=None):
    table = _dev(table, "table")
    if table.dim() != 2 or table.shape[1] != LEVEL_COLS or (N is not None and table.shape[0] != N):
        raise ValueError(f"table must be ({'N' if N is None else N}, {LEVEL_COLS}), got {tuple(table.shape)}")
    return table


def _int_list(values, what):
    a = np.ascontiguousarray(np.asarray(list(values), dtype=np.int64).reshape(-1))
    if not 1 <= a.size <= MAX_LIST:
        raise ValueError(f"{what} must list 1 .. {MAX_LIST} entries, got {a.size}")
    return a.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------ device forms
@torch.no_grad()
def noise_levels(values, *, mode="draw", sigma_data, P_mean=0.0, P_std=1.0, images=None, scale_channels=None, eps=0.05, engine=None,
                 enqueue_only=False):
    """The level table (N, 6) fp32 -- sigma, t, cos t, sin t, x_lv = log(tan(t) / 8), std -- from `values` (N):
      mode 'draw'   normals z: sigma = exp(z P_std + P_mean) (train_step, evaluate); with `scale_channels` (the reference's scale_sigma and
                    scaling_channels) times max(std(images[n, scale_channels]) / sigma_data, eps), torch's unbiased std;
      mode 'sigma'  sigma itself (noise_loss_curve);        mode 't'  t itself (what return_logvar starts from).
    Float64 device arithmetic on the fp32 inputs, every column rounded once; cos, sin and x_lv are taken of the ROUNDED t."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    z = _dev(values, "values").reshape(-1)
    N = int(z.numel())
    if not 1 <= N <= MAX_ITEMS:
        raise ValueError(f"values must hold 1 .. {MAX_ITEMS} entries, got {N}")
    img, ch, Cn, H, W = None, None, 0, 0, 0
    if scale_channels is not None:
        if mode != "draw":
            raise ValueError("scale_channels goes with mode 'draw'")
        img = _nchw(images, "images")
        if img.shape[0] != N:
            raise ValueError(f"images has {img.shape[0]} items, values {N}")
        Cn, H, W = (int(d) for d in img.shape[1:])
        ch = _int_list(scale_channels, "scale_channels")
        if ch.min() < 0 or ch.max() >= Cn:
            raise ValueError(f"scale_channels {ch.tolist()} outside 0 .. {Cn - 1}")
    engine, dev = _engine_for(z, engine)
    table = torch.empty((N, LEVEL_COLS), dtype=torch.float32, device=dev)
    call(_LIB, "td_objective_levels", engine, dev, MODES[mode], _dp(z), N, float(P_mean), float(P_std), float(sigma_data), _dp(img), Cn, H, W,
         None if ch is None else C.c_void_p(ch.ctypes.data), 0 if ch is None else int(ch.size), float(eps), _dp(table), enqueue_only=enqueue_only,
         ordered=True)
    return table


@torch.no_grad()
def add_noise(images, noise, table, *, sigma_data, cond_img=None, engine=None, enqueue_only=False):
    """(x, v) in one pass, with nz = noise sigma_data: the model input x (N, C + Cc, H, W) = (cos t images + sin t nz) / sigma_data followed
    by cond_img's channels copied, and the target v (N, C, H, W) = cos t nz - sin t images.  fp32, in the reference's order of operations."""
    img = _nchw(images, "images")
    N, Cn, H, W = (int(d) for d in img.shape)
    nz = _dev(noise, "noise")
    if tuple(nz.shape) != tuple(img.shape):
        raise ValueError(f"noise must be {tuple(img.shape)}, got {tuple(nz.shape)}")
    table = _table(table, N)
    cond, Cc = None, 0
    if cond_img is not None:
        cond = _dev(cond_img, "cond_img")
        if cond.dim() != 4 or cond.shape[0] != N or tuple(cond.shape[2:]) != (H, W) or cond.shape[1] < 1:
            raise ValueError(f"cond_img must be ({N}, Cc, {H}, {W}), got {tuple(cond.shape)}")
        Cc = int(cond.shape[1])
    if Cn + Cc > MAX_CHANNELS or N * (Cn + Cc) * H * W >= 2 ** 31:
        raise ValueError(f"x ({N}, {Cn + Cc}, {H}, {W}) beyond the library's limit ({MAX_CHANNELS} channels, 2^31 elements)")
    engine, dev = _engine_for(img, engine)
    x = torch.empty((N, Cn + Cc, H, W), dtype=torch.float32, device=dev)
    v = torch.empty((N, Cn, H, W), dtype=torch.float32, device=dev)
    call(_LIB, "td_objective_noise", engine, dev, _dp(img), _dp(nz), _dp(cond), _dp(table), N, Cn, Cc, H, W, float(sigma_data), _dp(x), _dp(v),
         enqueue_only=enqueue_only, ordered=True)
    return x, v


@torch.no_grad()
def logvar(table, freqs, phases, weight, *, n_logvar=1, engine=None, enqueue_only=False):
    """(N) fp32: the head of edm_unet.py:181-183, weight . (sqrt2 cos(x_lv freqs + phases)), from the table's x_lv.  `weight` (K) is
    logvar_linear.weight ALREADY FOLDED (EDMUnet2D._fold_reference(w, 1)).  fp32; the reference's bf16 autocast is not reproduced."""
    if int(n_logvar) != 1:
        raise NotImplementedError(f"n_logvar={n_logvar}: the reference's reshape(-1, 1, 1, 1) only broadcasts for 1")
    table = _table(table)
    f, p, w = (_dev(a, what).reshape(-1) for a, what in ((freqs, "freqs"), (phases, "phases"), (weight, "weight")))
    K = int(f.numel())
    if not 1 <= K <= MAX_LOGVAR:
        raise ValueError(f"logvar_channels must be in 1 .. {MAX_LOGVAR}, got {K}")
    if p.numel() != K or w.numel() != K:
        raise ValueError(f"freqs, phases and weight must hold {K} entries each, got {p.numel()} and {w.numel()}")
    engine, dev = _engine_for(table, engine)
    N = int(table.shape[0])
    out = torch.empty((N,), dtype=torch.float32, device=dev)
    call(_LIB, "td_objective_logvar", engine, dev, _dp(table), N, _dp(f), _dp(p), _dp(w), K, 1, _dp(out), enqueue_only=enqueue_only, ordered=True)
    return out


@torch.no_grad()
def squared_error(model_output, v, *, sigma_data, engine=None, enqueue_only=False):
    """S (N, C) float64: the sum over H x W of (fl32(-sigma_data model_output) - v)^2, the difference in fp32 as the reference forms it, the
    square and the sum in float64 through a fixed tree."""
    out = _nchw(model_output, "model_output")
    vv = _dev(v, "v")
    if tuple(vv.shape) != tuple(out.shape):
        raise ValueError(f"v must be {tuple(out.shape)}, got {tuple(vv.shape)}")
    N, Cn, H, W = (int(d) for d in out.shape)
    engine, dev = _engine_for(out, engine)
    S = torch.empty((N, Cn), dtype=torch.float64, device=dev)
    call(_LIB, "td_objective_sqerr", engine, dev, _dp(out), _dp(vv), N, Cn, H, W, float(sigma_data), _dp(S), enqueue_only=enqueue_only, ordered=True)
    return S


@torch.no_grad()
def v_loss(S, H, W, *, sigma_data, logvar=None, form="weighted", loss_groups=None, engine=None, enqueue_only=False):
    """The scalar loss from S (N, C) and H, W, in one of the reference's three forms:
      'weighted'  mean_n(mean_c(S / HW) / (exp(logvar_n) sigma_data^2) + logvar_n)       (_calc_loss);
      'plain'     mean(S / HW) / sigma_data^2                                            (noise_loss_curve without loss_groups);
      'grouped'   the mean over `loss_groups` (channel counts summing to C) of each group's mean.
    Returns VLoss(value, items, loss64, loss32): the per-item losses (N) float64 and the scalar as float64 and rounded once to fp32 stay on
    the device; `value` is the float64 scalar read back (None when only enqueued)."""
    if form not in FORMS:
        raise ValueError(f"form must be one of {sorted(FORMS)}, got {form!r}")
    S = _dev(S, "S", torch.float64)
    if S.dim() != 2 or S.shape[0] < 1 or S.shape[1] < 1:
        raise ValueError(f"S must be (N, C), got {tuple(S.shape)}")
    N, Cn = (int(d) for d in S.shape)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or N > MAX_ITEMS or Cn > MAX_CHANNELS or H > MAX_SIDE or W > MAX_SIDE or N * Cn * H * W >= 2 ** 31:
        raise ValueError(f"({N}, {Cn}, {H}, {W}) is empty or beyond the library's limit")
    lv = groups = None
    if form == "weighted":
        if logvar is None:
            raise ValueError("the weighted form needs logvar")
        lv = _dev(logvar, "logvar").reshape(-1)
        if lv.numel() != N:
            raise ValueError(f"logvar must hold {N} entries, got {lv.numel()}")
    if form == "grouped":
        if loss_groups is None:
            raise ValueError("the grouped form needs loss_groups")
        groups = _int_list(loss_groups, "loss_groups")
        if groups.min() < 1 or int(groups.sum()) != Cn:
            raise ValueError(f"loss_groups {groups.tolist()} must be positive and sum to C = {Cn}")
    engine, dev = _engine_for(S, engine)
    items = torch.empty((N,), dtype=torch.float64, device=dev)
    l64 = torch.empty((1,), dtype=torch.float64, device=dev)
    l32 = torch.empty((1,), dtype=torch.float32, device=dev)
    call(_LIB, "td_objective_loss", engine, dev, _dp(S), _dp(lv), N, Cn, H, W, float(sigma_data), FORMS[form],
         None if groups is None else C.c_void_p(groups.ctypes.data), 0 if groups is None else int(groups.size), _dp(items), _dp(l64), _dp(l32),
         enqueue_only=enqueue_only, ordered=True)
    return VLoss(None if enqueue_only else float(l64.item()), items, l64, l32)


@torch.no_grad()
def terrain_uint8(terrain, *, engine=None, enqueue_only=False):
    """_normalize_and_process_terrain: terrain (N, C, H, W) -> uint8 (N, 3 C, H, W), per item centred on the middle of its range, the range
    floored at 255, clamped, truncated, repeated three times.  A NaN pixel (the reference's conversion is undefined there) gives 0."""
    x = _nchw(terrain, "terrain")
    N, Cn, H, W = (int(d) for d in x.shape)
    if 3 * Cn > MAX_CHANNELS or N * 3 * Cn * H * W >= 2 ** 31:
        raise ValueError(f"output ({N}, {3 * Cn}, {H}, {W}) beyond the library's limit ({MAX_CHANNELS} channels, 2^31 elements)")
    engine, dev = _engine_for(x, engine)
    out = torch.empty((N, 3 * Cn, H, W), dtype=torch.uint8, device=dev)
    call(_LIB, "td_objective_terrain_u8", engine, dev, _dp(x), N, Cn, H, W, _dp(out), enqueue_only=enqueue_only, ordered=True)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ drop-ins
def _draw(shape, generator, dev):
    """torch.randn(shape) as the reference draws it: on the generator's own device (the default generator of `dev` without one)"""
    if generator is None:
        return torch.randn(shape, device=dev)
    return torch.randn(shape, generator=generator, device=generator.device).to(dev)


def _batch_parts(batch, dev):
    images = torch.as_tensor(batch["image"]).to(device=dev, dtype=torch.float32)
    cond_img = batch.get("cond_img")
    if cond_img is not None:
        cond_img = torch.as_tensor(cond_img).to(device=dev, dtype=torch.float32)
    return images, cond_img, batch.get("cond_inputs")


def _forward(model, images, cond_img, cond_inputs, table, noise, sigma_data, with_logvar):
    """noising, the U-Net, the squared error, and the logvar head from the x_lv the batch's table already holds: (S, logvar (N) or None)"""
    ops = model.logvar_operands() if with_logvar else None      # a checkpoint without the head fails before anything is launched
    x, v = add_noise(images, noise, table, sigma_data=sigma_data, cond_img=cond_img, engine=model.engine)
    t = table[:, 1].cpu()                                       # the one read-back of a batch: td_unet_forward takes noise_labels from the host
    out = model(x, t, cond_inputs)
    lv = logvar(table, *ops, engine=model.engine) if with_logvar else None
    return squared_error(out, v, sigma_data=sigma_data, engine=model.engine), lv


@torch.no_grad()
def validation_loss(model, batches, *, sigma_data, P_mean, P_std, generator=None, scale_sigma=None):
    """`val/loss`: the loop of DiffusionTrainer.evaluate (diffusion.py:372-407) over `batches`, each the dict a get_batch returns or any mapping
    with `image` and optionally `cond_img` and `cond_inputs`.  Per batch the draws are the reference's, in its order -- randn(N) for sigma,
    then randn(images.shape) --, the loss is _calc_loss; the batches' losses are averaged.  scale_sigma (train_step's option): None, a list of
    channels, or a mapping with `channels` and optionally `eps` (the reference's sigma_scale_eps, 0.05)."""
    dev = model.device
    channels, eps = None, 0.05
    if scale_sigma is not None:
        if isinstance(scale_sigma, collections.abc.Mapping):
            channels, eps = scale_sigma["channels"], scale_sigma.get("eps", 0.05)
        else:
            channels = scale_sigma
    losses = []
    for batch in batches:
        images, cond_img, cond_inputs = _batch_parts(batch, dev)
        z = _draw((images.shape[0],), generator, dev)
        noise = _draw(tuple(images.shape), generator, dev)
        table = noise_levels(z, mode="draw", sigma_data=sigma_data, P_mean=P_mean, P_std=P_std, images=images if channels is not None else None,
                             scale_channels=channels, eps=eps, engine=model.engine)
        S, lv = _forward(model, images, cond_img, cond_inputs, table, noise, sigma_data, True)
        losses.append(v_loss(S, images.shape[2], images.shape[3], sigma_data=sigma_data, logvar=lv, form="weighted", engine=model.engine).value)
    if not losses:
        raise ValueError("no batches")
    return float(np.mean(losses))


@torch.no_grad()
def noise_loss_curve(model, batches, sigmas, *, sigma_data, loss_groups=None, generator=None):
    """The loss-versus-sigma curve of training/dev_utils/noise_loss_curve.py:105-133 over a fixed list of batches: (sigmas, losses) as float64
    arrays, losses[i] the mean over the batches of the plain loss -- or of the grouped one with loss_groups -- at sigmas[i], with fresh
    noise per (sigma, batch) as there.  It does not plot."""
    batches = list(batches)
    if not batches:
        raise ValueError("no batches")
    dev = model.device
    sig = np.asarray(torch.as_tensor(sigmas).detach().cpu(), dtype=np.float32).reshape(-1)
    form = "plain" if loss_groups is None else "grouped"
    losses = []
    for s in sig:
        per = []
        for batch in batches:
            images, cond_img, cond_inputs = _batch_parts(batch, dev)
            table = noise_levels(torch.full((images.shape[0],), float(s), dtype=torch.float32, device=dev), mode="sigma", sigma_data=sigma_data,
                                 engine=model.engine)
            noise = _draw(tuple(images.shape), generator, dev)
            S, _ = _forward(model, images, cond_img, cond_inputs, table, noise, sigma_data, False)
            per.append(v_loss(S, images.shape[2], images.shape[3], sigma_data=sigma_data, form=form, loss_groups=loss_groups, engine=model.engine).value)
        losses.append(np.mean(per))
    return sig.astype(np.float64), np.asarray(losses, dtype=np.float64)
