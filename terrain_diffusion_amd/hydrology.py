"""Hydrology of generated terrain on the GPU: the reference's d8_flow, flow_accumulation, plot_flow_indicator and
fill_depressions_priority_flood (terrain_diffusion/inference/postprocessing.py), with the reference's results bit for bit (the indicator's
log1p to 1 ulp of numpy's).

The work runs in hydro_csrc/hydro_kernels.hip through include/td_hydro.h (libtd_hydro.so), on the engine's stream.  Two surfaces:
  * device forms -- flow_directions, flow_accumulation_map, flow_indicator, fill_depressions: device tensors in and out, no host copy of an
    image (the accumulation reads back one 4-byte count of uphill edges; the fill reads its convergence flags);
  * drop-ins with the reference's names, signatures and return dtypes, taking numpy arrays or tensors and returning numpy arrays.
The contract is fp32 elevation (what WorldPipeline.get returns).  Other dtypes are cast to fp32 first; where the reference would have computed
in float64, its result can differ.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import Library
from ._plumbing import call, engine_for as _engine_for, f32 as _f32
from .engine import ptr

_P = C.c_void_p
_SIGS = {
    "td_hydro_last_error": (C.c_char_p, []),
    "td_hydro_d8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, C.c_int]),
    "td_hydro_accumulate": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int]),
    "td_hydro_indicator": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "td_hydro_fill": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, _P, C.POINTER(C.c_int)]),
}
EXPORTS = tuple(_SIGS)
MAX_SIDE = 1 << 20          # d8 and fill: H, W <= 2^20, H * W < 2^31
MAX_CELLS_ACC = 1 << 24     # accumulation and indicator: upstream counts stay exact in fp32
_LIB = Library("libtd_hydro.so", _SIGS, "td_hydro_last_error", "td_hydro")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check


def _check_shape(shape, max_cells):
    if len(shape) != 2:
        raise ValueError(f"elevation must be (H, W), got shape {tuple(shape)}")
    H, W = int(shape[0]), int(shape[1])
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE or H * W > max_cells:
        raise ValueError(f"elevation (H, W) = {(H, W)} outside 1 <= H, W <= 2^20, H * W <= {max_cells}")
    return H, W


@torch.no_grad()
def flow_directions(z, tol=1e-3, *, engine=None):
    """D8 receivers of a 2-D elevation (tensor or array) -> (receiver int32 (H, W) flat index r * W + c, kmax uint8 (H, W), is_sink bool (H, W)),
    device tensors.  The reference's d8_flow rule for rule: slopes in fp32, fl32(tol), ocean = NaN or <= 0, the first maximum."""
    H, W = _check_shape(z.shape, (1 << 31) - 1)
    engine, dev = _engine_for(z, engine)
    e = _f32(z, dev)
    receiver = torch.empty((H, W), dtype=torch.int32, device=dev)
    kmax = torch.empty((H, W), dtype=torch.uint8, device=dev)
    sink = torch.empty((H, W), dtype=torch.uint8, device=dev)
    call(_LIB, "td_hydro_d8", engine, dev, ptr(e), H, W, float(tol), ptr(receiver), ptr(kmax), ptr(sink))
    return receiver, kmax, sink.view(torch.bool)


@torch.no_grad()
def flow_accumulation_map(z, receiver, is_sink, *, engine=None):
    """Upstream cell count (float32 (H, W) device tensor, 0 on ocean) over the receivers of flow_directions (int32 flat indices, or anything
    torch converts to them) and its sink mask.  Raises ValueError when a counted edge is not strictly downhill: the reference's result then
    depends on how its sort orders equal elevations.  That check reads one 4-byte count back (a host sync)."""
    H, W = _check_shape(z.shape, MAX_CELLS_ACC)
    engine, dev = _engine_for(z, engine)
    e = _f32(z, dev)
    r = torch.as_tensor(receiver).to(device=dev, dtype=torch.int32).contiguous()
    s = torch.as_tensor(is_sink).to(device=dev, dtype=torch.bool).contiguous()
    if tuple(r.shape) != (H, W) or tuple(s.shape) != (H, W):
        raise ValueError(f"receiver {tuple(r.shape)} and is_sink {tuple(s.shape)} must have the elevation's shape {(H, W)}")
    acc = torch.empty((H, W), dtype=torch.float32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    call(_LIB, "td_hydro_accumulate", engine, dev, ptr(e), H, W, ptr(r), ptr(s.view(torch.uint8)), ptr(acc), ptr(bad))
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f"flow_accumulation: {n_bad} counted edge(s) are not strictly downhill (or point outside the image); the reference's "
                         "result would depend on the order its sort gives to equal elevations")
    return acc


@torch.no_grad()
def _indicator_of(acc, max_pool_kernel, engine, dev):
    H, W = int(acc.shape[0]), int(acc.shape[1])
    k = int(max_pool_kernel) if max_pool_kernel > 1 else 1
    Ho, Wo = H // k, W // k
    out = torch.empty((Ho, Wo), dtype=torch.float32, device=dev)
    if Ho == 0 or Wo == 0:
        return out
    call(_LIB, "td_hydro_indicator", engine, dev, ptr(acc), H, W, k, ptr(out))
    return out


@torch.no_grad()
def flow_indicator(z, max_pool_kernel=1, *, tol=1e-3, engine=None):
    """log1p of the upstream cell count after a non-overlapping max_pool_kernel^2 max-pool (cropped to a multiple of it; none when <= 1):
    the river map of plot_flow_indicator, as a float32 device tensor."""
    _check_shape(z.shape, MAX_CELLS_ACC)
    engine, dev = _engine_for(z, engine)
    e = _f32(z, dev)
    receiver, _, sink = flow_directions(e, tol, engine=engine)
    acc = flow_accumulation_map(e, receiver, sink, engine=engine)
    return _indicator_of(acc, max_pool_kernel, engine, dev)


def _check_epsilon(epsilon):
    eps = float(epsilon)
    if not eps >= 0.0:
        raise ValueError(f"epsilon must be >= 0, got {epsilon}: with a negative one the reference's result depends on its heap order")
    return eps


@torch.no_grad()
def fill_depressions(height, epsilon=1e-3, connectivity=8, nodata=None, *, return_passes=False, engine=None):
    """Priority-Flood+epsilon depression fill (max_raise None) of a 2-D elevation -> float32 device tensor; with return_passes=True,
    (filled, passes) where passes counts the relaxation passes until one changed nothing.  Invalid cells (NaN, <= 0, == nodata) keep their
    value; connectivity 4, anything else means 8; epsilon >= 0, added in fp32.  Synchronises the engine's stream (convergence check)."""
    H, W = _check_shape(height.shape, (1 << 31) - 1)
    eps = _check_epsilon(epsilon)
    engine, dev = _engine_for(height, engine)
    h = _f32(height, dev)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    passes = C.c_int(0)
    with torch.cuda.device(dev):   # no synchronize argument: td_hydro_fill always synchronises
        check(lib().td_hydro_fill(C.c_void_p(engine.stream), ptr(h), H, W, eps, int(connectivity), int(nodata is not None),
                                  float(nodata) if nodata is not None else 0.0, ptr(out), C.byref(passes)))
    return (out, passes.value) if return_passes else out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Drop-ins: the reference's names, signatures and return dtypes.

def _as_input(z):
    return z.detach() if torch.is_tensor(z) else np.asarray(z)


def d8_flow(z, tol=1e-3, *, engine=None):
    """Drop-in for the reference's d8_flow -> (rr, cc, is_sink, kmax): rr, cc, kmax int64, is_sink bool, numpy arrays."""
    z = _as_input(z)
    _check_shape(z.shape, (1 << 31) - 1)
    receiver, kmax, sink = flow_directions(z, tol, engine=engine)
    W = int(z.shape[1])
    r = receiver.to(torch.int64)
    return (r // W).cpu().numpy(), (r % W).cpu().numpy(), sink.cpu().numpy(), kmax.to(torch.int64).cpu().numpy()


def flow_accumulation(z, rr, cc, is_sink, *, engine=None):
    """Drop-in for the reference's flow_accumulation -> float32 numpy array.  Receivers outside the image raise IndexError (as indexing does in
    the reference); uphill or level counted edges raise ValueError (see flow_accumulation_map)."""
    z = _as_input(z)
    H, W = _check_shape(z.shape, MAX_CELLS_ACC)
    rr = torch.as_tensor(np.asarray(rr) if not torch.is_tensor(rr) else rr).to(torch.int64)
    cc = torch.as_tensor(np.asarray(cc) if not torch.is_tensor(cc) else cc).to(torch.int64)
    if tuple(rr.shape) != (H, W) or tuple(cc.shape) != (H, W):
        raise ValueError(f"rr {tuple(rr.shape)} and cc {tuple(cc.shape)} must have the elevation's shape {(H, W)}")
    if bool(((rr < 0) | (rr >= H) | (cc < 0) | (cc >= W)).any()):
        raise IndexError("flow_accumulation: rr / cc point outside the image")
    sink = torch.as_tensor(np.asarray(is_sink) if not torch.is_tensor(is_sink) else is_sink).to(torch.bool)
    return flow_accumulation_map(z, (rr * W + cc).to(torch.int32), sink, engine=engine).cpu().numpy()


def plot_flow_indicator(z, max_pool_kernel=1, *, engine=None):
    """Drop-in for the reference's plot_flow_indicator (d8_flow with its default tol, flow_accumulation, max-pool, log1p) -> float32 numpy."""
    z = _as_input(z)
    return flow_indicator(z, max_pool_kernel, engine=engine).cpu().numpy()


def fill_depressions_priority_flood(height, epsilon=1e-3, max_raise=None, connectivity=8, in_place=False, nodata=None, *, engine=None):
    """Drop-in for the reference's fill_depressions_priority_flood with max_raise None -> float32 numpy array.  A max_raise other than None
    raises NotImplementedError (the reference's result then depends on its heap order).  in_place=True also writes the result into `height`
    when that is a float32 numpy array (the reference's behaviour; any other input is left as it is)."""
    if max_raise is not None:
        raise NotImplementedError("fill_depressions_priority_flood: only max_raise=None is supported (with a limit the result depends on heap order)")
    _check_epsilon(epsilon)
    h = _as_input(height)
    out = fill_depressions(h, epsilon, connectivity, nodata, engine=engine).cpu().numpy()
    if in_place and isinstance(height, np.ndarray) and height.dtype == np.float32:
        height[...] = out
        return height
    return out
