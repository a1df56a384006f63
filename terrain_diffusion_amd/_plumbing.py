"""What the bindings of the side libraries (relief, hydrology, minecraft, explorer) share around their calls: the engine and device of an
input, the fp32 device form of an array, the shape checks of the per-call limit, and the call itself on the engine's stream."""
import contextlib
import ctypes as C

import numpy as np
import torch

from .engine import _SHARED_STREAM, get_engine

MAX_SIDE = 1 << 16          # per call of libtd_mc.so and libtd_explorer.so: 1 <= H, W <= 2^16 ...
MAX_PIXELS = 1 << 26        # ... and H * W <= 2^26 pixels (include/td_mc.h, include/td_explorer.h)


def engine_for(x, engine):
    """(engine, its device): the given engine, else the one of x's GPU, else GPU 0's."""
    if engine is None:
        engine = get_engine(x.device if (torch.is_tensor(x) and x.is_cuda) else None)
    return engine, torch.device("cuda", engine.device_id)


def f32(x, dev):
    """Contiguous fp32 device tensor of a numpy array or tensor (no copy when it already is one)."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    return x.detach().to(device=dev, dtype=torch.float32).contiguous()


def sync_flag(engine, enqueue_only=False):
    """The `synchronize` argument of an entry point: 0 when the caller only enqueues or the engine is in enqueue-only mode (option "async")."""
    return 0 if (enqueue_only or engine._async) else 1


def shape(x):
    return tuple(int(d) for d in x.shape)


def hw(H, W, noun):
    """(H, W) within the per-call limit; `noun` is what the messages call the image ("box", "field")."""
    if H < 1 or W < 1:
        raise ValueError(f"empty {noun}: {H} x {W} pixels")
    if H > MAX_SIDE or W > MAX_SIDE or H * W > MAX_PIXELS:
        raise ValueError(f"{noun} {H} x {W} beyond the library's limit (H, W <= 2^16, H * W <= 2^26 pixels)")
    return H, W


class _Ordered:
    """Orders the engine's stream with torch's current stream WITHOUT a host synchronisation: on entry the engine's stream waits for what
    torch has enqueued (the inputs), on exit torch's stream waits for the engine's (the outputs).  Nothing to do when the engine already
    launches on torch's current stream (Engine.on_stream)."""

    def __init__(self, engine, dev):
        cur = torch.cuda.current_stream(dev)
        self.cur, self.ext = cur, None
        if _SHARED_STREAM.get(engine.device_id) != cur.cuda_stream:
            self.ext = torch.cuda.ExternalStream(int(engine.stream), device=dev)

    def __enter__(self):
        if self.ext is not None:
            self.ext.wait_stream(self.cur)
        return self

    def __exit__(self, *exc):
        if self.ext is not None:
            self.cur.wait_stream(self.ext)
        return False


_UNORDERED = contextlib.nullcontext()


def call(library, name, engine, dev, *args, enqueue_only=False, ordered=False):
    """One entry point `name` of a _lib.Library with `dev` current: the engine's stream first, then args, the synchronize flag last; checked.
    ordered=True orders the engine's stream with torch's current one (_Ordered) for callers that take pointers without engine.ptr's host
    synchronisation."""
    with torch.cuda.device(dev), (_Ordered(engine, dev) if ordered else _UNORDERED):
        library.check(getattr(library.lib(), name)(C.c_void_p(engine.stream), *args, sync_flag(engine, enqueue_only)))
