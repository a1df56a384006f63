"""GPU: how every C-ABI call of the engine ENDS (csrc/engine.hip: struct Call).  Under engine option "async" a call whose caller buffers are all device
memory only enqueues on the engine's stream; one host pointer among them, a host table too large for the pinned ring, "async" = 0, or one of the four
entry points that never honoured the option make it wait for the stream.  DESIGN.md has the table; this file records it from the library.

Method: the engine runs on a torch stream `s` (Engine.on_stream); a chain of 4096 x 4096 matmuls is queued on `s` in front of the call and `s.query()` is
read right after it: still busy = the call only enqueued, drained = it waited.  The chain is at least 20 times as long as the call itself takes (both
measured here, per entry point), so host jitter cannot make an enqueue-only call look synchronous, and every case first asserts that the chain
alone leaves `s` busy.  Every case's results are compared bit for bit with the same call made synchronously on the engine's own stream."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

SD = 0.5
N, HW, STEPS = 2, 16, 3


def _dev(seed, shape, scale=1.0):
    from oracle import rng
    return (torch.from_numpy(rng.standard_normal(seed, shape)) * scale).cuda().contiguous()


class Case:
    """One entry point on fixed inputs.  make() -> {name: fresh device tensor}; call(b) makes the C call on those buffers (a test may have moved some to
    the host); `ptrs`: the caller pointers that must be device memory for the call to end enqueue-only; `outs`: what the call writes."""

    def __init__(self, name, make, call, ptrs, outs, always_sync=False):
        self.name, self.make, self.call, self.ptrs, self.outs, self.always_sync = name, make, call, tuple(ptrs), tuple(outs), always_sync
        self.ref = self.units = None


class Bench:
    """the stream, the delay chain and the per-case calibration"""

    def __init__(self, eng):
        self.eng, self.s = eng, torch.cuda.Stream()
        self.a = torch.randn(4096, 4096, device="cuda") / 64.0
        self.b = torch.empty_like(self.a)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            self.delay(4)                                   # warm-up: the first matmul loads its kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.s)
            self.delay(8)
            e1.record(self.s)
        torch.cuda.synchronize()
        self.unit_s = e0.elapsed_time(e1) * 1e-3 / 8

    def delay(self, units):
        """`units` matmuls on torch's current stream"""
        for _ in range(units):
            torch.mm(self.a, self.a, out=self.b)

    def prepare(self, case):
        """the synchronous reference of the case and the length of its delay chain"""
        if case.ref is not None:
            return
        b = case.make()
        torch.cuda.synchronize()
        case.call(b)                                        # engine's own stream, "async" = 0: complete on return (and plans / graphs exist from here on)
        torch.cuda.synchronize()
        case.ref = {k: b[k].cpu() for k in case.outs}
        b = case.make()
        torch.cuda.synchronize()
        with self.eng.on_stream(self.s, asynchronous=False):
            case.call(b)
            t0 = time.perf_counter()
            case.call(b)
            dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        case.units = max(8, math.ceil(20 * dt / self.unit_s))

    def run(self, case, asynchronous, host=()):
        """-> was `s` still busy when the call returned?  (the results are checked against the synchronous reference on the way)"""
        return self.run_seq([case], asynchronous, host)[0]

    def run_seq(self, seq, asynchronous, host=()):
        """the cases of `seq` one after the other inside ONE on_stream block, each behind a delay of its own -> [busy, ...]"""
        for case in seq:
            self.prepare(case)
        bufs = [case.make() for case in seq]
        for b in bufs:
            for k in host:
                b[k] = b[k].cpu()
        torch.cuda.synchronize()
        busy = []
        with self.eng.on_stream(self.s, asynchronous=asynchronous):
            for case, b in zip(seq, bufs):
                self.delay(case.units)
                assert not self.s.query(), f"{case.name}: a delay of {case.units} matmuls ({case.units * self.unit_s * 1e3:.1f} ms) is over before the call is made"
                case.call(b)
                busy.append(not self.s.query())
                self.s.synchronize()
        torch.cuda.synchronize()
        for case, b in zip(seq, bufs):
            for k in case.outs:
                assert torch.equal(b[k].cpu(), case.ref[k]), f"{case.name} (async={asynchronous}, host={host}): {k} differs from the synchronous call"
        return busy


@pytest.fixture(scope="module")
def cases():
    """every entry point of the end-of-call table on the smallest shapes, models built once"""
    import terrain_diffusion_amd as td
    from terrain_diffusion_amd._lib import lib, check, ae_lib, ae_check, EdmExt, GridBatch
    from terrain_diffusion_amd.engine import get_engine, ptr
    from oracle.unet import synth_state_dict, tiny_config
    from oracle import schedule
    import _ae_twin
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    eng = get_engine("cuda")
    L, E = lib(), eng._h
    cfg = tiny_config(64, 1)
    cfg_img = tiny_config(64, 1, in_channels=6, out_channels=5)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=77))
    guide = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=78))
    mi = td.EDMUnet2D(**cfg_img, dtype="bf16").load_state_dict(synth_state_dict(cfg_img, seed=79))
    ae = td.EDMAutoencoder(**_ae_twin.TINY, dtype="bf16").load_state_dict(_ae_twin.synth_ae_state_dict(_ae_twin.TINY, seed=77))
    sig = schedule.karras_sigmas(STEPS)[0].contiguous()
    t = np.arctan(sig[:STEPS].numpy().astype(np.float32) / np.float32(SD))
    cs = np.ascontiguousarray(np.stack([np.cos(t), np.sin(t)], 1).astype(np.float32))
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    out = []

    def add(name, make, call, ptrs=(), outs=("out",), always_sync=False):
        out.append(Case(name, make, call, ptrs, outs, always_sync))

    # ---- samplers
    def mk_edm(img):
        def make():
            b = dict(x=_dev(12, (N, 5, HW, HW), 80.0), cond=_dev(13, (N, 58)))
            if img:
                b["cond_img"] = _dev(14, (N, 1, HW, HW))
            return b
        return make
    add("td_sample_edm", mk_edm(False), lambda b: check(L.td_sample_edm(m._h, N, HW, HW, STEPS, ptr(sig), SD, ptr(b["cond"]), ptr(b["x"]))), ("x", "cond"), ("x",))
    add("td_sample_edm_img", mk_edm(True), lambda b: check(L.td_sample_edm_img(mi._h, N, HW, HW, STEPS, ptr(sig), SD, ptr(b["cond"]), ptr(b["cond_img"]), 1, ptr(b["x"]))),
        ("x", "cond", "cond_img"), ("x",))
    add("td_sample_edm_guided", mk_edm(False), lambda b: check(L.td_sample_edm_guided(m._h, guide._h, 1.3, N, HW, HW, STEPS, ptr(sig), SD, ptr(b["cond"]), ptr(b["x"]))),
        ("x", "cond"), ("x",))

    def call_ext(b):
        a = EdmExt(n=N, H=HW, W=HW, n_steps=STEPS, sigmas_host=ptr(sig), sigma_data=SD, cond=ptr(b["cond"]), x=ptr(b["x"]), cond_img=ptr(b["cond_img"]), cimg_channels=1,
                   guide=None, guidance_scale=1.0, score_scaling=0.9, score_cs_host=vp(cs))
        check(L.td_sample_edm_ext(mi._h, C.byref(a)))
    add("td_sample_edm_ext", mk_edm(True), call_ext, ("x", "cond", "cond_img"), ("x",))

    def mk_cons(img):
        def make():
            b = dict(out=torch.zeros(N, 5, HW, HW, device="cuda"), z=_dev(15, (N, 5, HW, HW)), sample=_dev(16, (N, 5, HW, HW)), cond=_dev(13, (N, 58)))
            if img:
                b["cond_img"] = _dev(14, (N, 1, HW, HW))
            return b
        return make
    add("td_sample_consistency", mk_cons(False),
        lambda b: check(L.td_sample_consistency(m._h, N, HW, HW, 1.1, SD, ptr(b["sample"]), ptr(b["z"]), ptr(b["cond"]), ptr(b["out"]))), ("out", "z", "sample", "cond"))
    add("td_sample_consistency_img", mk_cons(True),
        lambda b: check(L.td_sample_consistency_img(mi._h, N, HW, HW, 1.1, SD, ptr(b["sample"]), ptr(b["z"]), ptr(b["cond"]), ptr(b["cond_img"]), 1, ptr(b["out"]))),
        ("out", "z", "sample", "cond", "cond_img"))

    # ---- tiling: 2 x 2 windows of 16, one channel, on a 24 x 24 canvas
    org = np.ascontiguousarray(np.array([[0, 0], [0, 8], [8, 0], [8, 8]], dtype=np.int64))
    starts = np.array([0, 8], dtype=np.int32)
    wi, wj = np.array([0, 0, 1, 1], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32)
    add("td_noise_patches", lambda: dict(out=torch.zeros(4, 1, HW, HW, device="cuda")),
        lambda b: check(L.td_noise_patches(E, 99, 4, vp(org), HW, HW, 1, 64, 64, 1.5, ptr(b["out"]))), ("out",))
    mk_blend = lambda: dict(canvas=_dev(20, (2, 24, 24)).abs() + 1.0, tiles=_dev(21, (4, 1, HW, HW)), window=_dev(22, (HW, HW)).abs() + 0.1)   # noqa: E731
    add("td_blend_windows", mk_blend, lambda b: check(L.td_blend_windows(E, ptr(b["canvas"]), 1, 24, 24, HW, 2, vp(starts), 2, vp(starts), 4, vp(wi), vp(wj), ptr(b["tiles"]), 1)),
        ("canvas", "tiles"), ("canvas",))
    add("td_blend_windows_w", mk_blend,
        lambda b: check(L.td_blend_windows_w(E, ptr(b["canvas"]), 1, 24, 24, HW, 2, vp(starts), 2, vp(starts), 4, vp(wi), vp(wj), ptr(b["tiles"]), 0, ptr(b["window"]))),
        ("canvas", "tiles"), ("canvas",))
    add("td_blend_normalize", lambda: dict(canvas=_dev(20, (2, 24, 24)).abs() + 1.0, out=torch.zeros(1, 24, 24, device="cuda")),
        lambda b: check(L.td_blend_normalize(E, ptr(b["canvas"]), 1, 24, 24, 2.0, ptr(b["out"]))), ("canvas", "out"))
    # one 24 x 24 region under the four windows (each listed with the position of its first pixel relative to the region)
    desc = np.ascontiguousarray(np.array([[[k, int(org[k, 0]), int(org[k, 1])] for k in range(4)]], dtype=np.int32))

    def call_gather(b):
        ptrs = np.array([b["tiles"][k].data_ptr() for k in range(4)], dtype=np.uint64)
        ptr(b["tiles"])
        check(L.td_gather_regions(E, 1, HW, 1, 24, 24, 4, vp(desc), 4, vp(ptrs), ptr(b["out"])))
    add("td_gather_regions", lambda: dict(tiles=_dev(21, (4, 1, HW, HW)), out=torch.zeros(1, 2, 24, 24, device="cuda")), call_gather)

    # ---- conditioning rows and the grid batch
    means, stds = np.linspace(-0.5, 0.5, 7).astype(np.float32), np.linspace(0.5, 1.5, 7).astype(np.float32)
    hist = np.array([0.11, -0.42, 0.93, 0.27, -0.08], dtype=np.float32)
    pos = np.ascontiguousarray(np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.int32))
    add("td_cond_rows", lambda: dict(grid=_dev(30, (7, 5, 5)), out=torch.zeros(4, 58, device="cuda")),
        lambda b: check(L.td_cond_rows(E, ptr(b["grid"]), 5, 5, 4, vp(pos), vp(means), vp(stds), vp(hist), 5, 0.3, ptr(b["out"]))), ("grid", "out"))

    def mk_grid(rows):
        def make():
            b = dict(canvas=torch.zeros(6, 24, 24, device="cuda"), windows=torch.zeros(4, 5, HW, HW, device="cuda"))
            b.update(cond_rows=_dev(31, (4, 58))) if rows else b.update(cond_grid=_dev(30, (7, 5, 5)))
            return b

        def call(b):
            g = GridBatch(noise_seed=99, n=4, H=HW, W=HW, tile_h=64, tile_w=64, noise_scale=float(sig[0]), origins_host=vp(org), n_steps=STEPS, sigma_data=SD,
                          sigmas_host=ptr(sig), canvas=ptr(b["canvas"]), Hc=24, Wc=24, size=HW, n_rows=2, n_cols=2, accumulate=1, row_starts_host=vp(starts),
                          col_starts_host=vp(starts), wi_host=vp(wi), wj_host=vp(wj), windows_out=ptr(b["windows"]))
            if rows:
                g.cond_rows = ptr(b["cond_rows"])
            else:
                g.cond_grid, g.grid_rows, g.grid_cols, g.cond_pos_host = ptr(b["cond_grid"]), 5, 5, vp(pos)
                g.cond_means_host, g.cond_stds_host, g.hist_host, g.n_hist, g.noise_level = vp(means), vp(stds), vp(hist), 5, 0.3
            check(L.td_sample_grid_batch(m._h, C.byref(g)))
        return make, call
    add("td_sample_grid_batch[rows]", *mk_grid(True), ("cond_rows",), ("canvas", "windows"))
    add("td_sample_grid_batch[grid]", *mk_grid(False), ("cond_grid",), ("canvas", "windows"))

    # ---- output composition
    iy = np.ascontiguousarray(np.array([[min(y // 2, 15), min(y // 2 + 1, 15)] for y in range(24)], dtype=np.int32))
    wy = np.ascontiguousarray(np.tile(np.array([0.75, 0.25], dtype=np.float32), (24, 1)))
    add("td_resample2d", lambda: dict(src=_dev(40, (1, HW, HW)), out=torch.zeros(1, 24, 24, device="cuda")),
        lambda b: check(L.td_resample2d(E, ptr(b["src"]), 1, HW, HW, 24, 24, vp(iy), vp(wy), 2, vp(iy), vp(wy), 2, ptr(b["out"]))), ("src", "out"))
    mk_packed = lambda: dict(packed=_dev(41, (2, HW, HW)), low=_dev(42, (HW, HW)), out=torch.zeros(HW, HW, device="cuda"))   # noqa: E731
    add("td_residual_plus", mk_packed, lambda b: check(L.td_residual_plus(E, ptr(b["packed"]), ptr(b["low"]), HW, HW, 0.1, 1.2, ptr(b["out"]))))
    add("td_elev_finish", lambda: dict(packed=_dev(41, (2, HW, HW)), low=_dev(42, (HW, HW)), out=torch.zeros(8, 8, device="cuda")),
        lambda b: check(L.td_elev_finish(E, ptr(b["packed"]), ptr(b["low"]), HW, HW, 3, 4, 8, 8, 0.1, 1.2, ptr(b["out"]))))
    add("td_ddim_cfg_step", lambda: dict(lat=_dev(43, (1024,)), pu=_dev(44, (1024,)), pc=_dev(45, (1024,)), out=torch.zeros(1024, device="cuda")),
        lambda b: check(L.td_ddim_cfg_step(E, ptr(b["lat"]), ptr(b["pu"]), ptr(b["pc"]), 1024, 7.5, 0.5, 0.6, ptr(b["out"]))))
    add("td_climate_finish", lambda: dict(feats=_dev(46, (5, 4, 4)), elev=_dev(47, (HW, HW)), out=torch.zeros(5, HW, HW, device="cuda")),
        lambda b: check(L.td_climate_finish(E, ptr(b["feats"]), 4, 4, ptr(b["elev"]), 0, 0, HW, HW, 8.0, 0, 0, ptr(b["out"]))))

    # ---- autoencoder (TINY: two levels, latent + direct skip = 3 channels)
    A = ae_lib()
    add("td_ae_preencode", lambda: dict(x=_dev(50, (1, 2, HW, HW)), means=torch.zeros(1, 3, 8, 8, device="cuda"), logvars=torch.zeros(1, 3, 8, 8, device="cuda"),
                                        packed_f16=torch.zeros(1, 6, 8, 8, device="cuda", dtype=torch.float16)),
        lambda b: ae_check(A.td_ae_preencode(ae._h, 1, HW, HW, ptr(b["x"]), 0.0, 1.0, 0, ptr(b["means"]), ptr(b["logvars"]), ptr(b["packed_f16"]))),
        ("x", "means", "logvars", "packed_f16"), ("means", "logvars", "packed_f16"))
    add("td_ae_postencode", lambda: dict(means=_dev(51, (192,)), logvars=_dev(52, (192,)), eps=_dev(53, (192,)), z=torch.zeros(192, device="cuda")),
        lambda b: ae_check(A.td_ae_postencode(ae._h, 192, ptr(b["means"]), ptr(b["logvars"]), ptr(b["eps"]), ptr(b["z"]))), ("means", "logvars", "eps", "z"), ("z",))
    add("td_ae_decode", lambda: dict(z=_dev(54, (1, 3, 8, 8)), out=torch.zeros(1, 2, HW, HW, device="cuda")),
        lambda b: ae_check(A.td_ae_decode(ae._h, 1, 8, 8, ptr(b["z"]), 1.0, 0.0, ptr(b["out"]))), ("z", "out"))

    # ---- the four entry points that wait for the stream whatever "async" says
    tt = np.full(N, 1.1, dtype=np.float32)
    add("td_unet_forward", lambda: dict(x=_dev(60, (N, 5, HW, HW)), cond=_dev(13, (N, 58)), out=torch.zeros(N, 5, HW, HW, device="cuda")),
        lambda b: check(L.td_unet_forward(m._h, N, HW, HW, ptr(b["x"]), vp(tt), ptr(b["cond"]), ptr(b["out"]))), always_sync=True)
    add("td_standard_normal", lambda: dict(out=torch.zeros(4096, device="cuda")), lambda b: check(L.td_standard_normal(E, 7, 4096, ptr(b["out"]))), always_sync=True)
    q = np.linspace(-1.0, 1.0, 9).astype(np.float32)
    add("td_perlin_map", lambda: dict(out=torch.zeros(HW, HW, device="cuda")),
        lambda b: check(L.td_perlin_map(E, HW, HW, 3, 5, 11, 0.05, 3, 2.0, 0.5, vp(q), vp(q), 9, ptr(b["out"]))), always_sync=True)
    add("td_attention", lambda: dict(q=_dev(61, (1, 2, 16, 64)), k=_dev(62, (1, 2, 16, 64)), v=_dev(63, (1, 2, 16, 64)), out=torch.zeros(1, 2, 16, 64, device="cuda")),
        lambda b: check(L.td_attention(E, ptr(b["q"]), ptr(b["k"]), ptr(b["v"]), 1, 2, 16, 16, 64, 0.125, 1, ptr(b["out"]))), always_sync=True)

    # ---- td_resample2d with a row-tap table of Hout * Ky * 4 = 2 129 920 bytes: more than half the pinned ring (2 MiB), so the upload reads the caller's array
    big_iy = np.ascontiguousarray((np.arange(8192 * 65, dtype=np.int32) % 4).reshape(8192, 65))
    big_wy = np.full((8192, 65), 1.0 / 65, dtype=np.float32)
    one_i, one_w = np.zeros((1, 1), dtype=np.int32), np.ones((1, 1), dtype=np.float32)
    big = Case("td_resample2d[row taps > half the ring]", lambda: dict(src=_dev(70, (1, 4, 1)), out=torch.zeros(1, 8192, 1, device="cuda")),
               lambda b: check(L.td_resample2d(E, ptr(b["src"]), 1, 4, 1, 8192, 1, vp(big_iy), vp(big_wy), 65, vp(one_i), vp(one_w), 1, ptr(b["out"]))), ("src", "out"), ("out",))
    yield eng, Bench(eng), {c.name: c for c in out}, big
    for mod in (m, guide, mi, ae):
        mod.close()


def _table(cases):
    return [c for c in cases[2].values() if not c.always_sync]


def test_all_device_calls_only_enqueue_under_async(cases):
    _, bench, _, _ = cases
    waited = [c.name for c in _table(cases) if not bench.run(c, True)]
    assert not waited, f"waited for the stream although every pointer was device memory: {waited}"


def test_async_off_every_call_is_synchronous(cases):
    _, bench, all_cases, _ = cases
    left = [c.name for c in all_cases.values() if bench.run(c, False)]
    assert not left, f'returned with work in flight under "async" = 0: {left}'


def test_one_host_pointer_makes_the_call_synchronous(cases):
    """each listed pointer of each row moved to the host in turn: the call reads or writes caller memory, so it must be complete on return"""
    _, bench, _, _ = cases
    left = [f"{c.name}:{p}" for c in _table(cases) for p in c.ptrs if bench.run(c, True, host=(p,))]
    assert not left, f"returned with work in flight although a caller buffer was host memory: {left}"


def test_the_four_always_synchronous_entry_points(cases):
    _, bench, all_cases, _ = cases
    sync = [c for c in all_cases.values() if c.always_sync]
    assert [c.name for c in sync] == ["td_unet_forward", "td_standard_normal", "td_perlin_map", "td_attention"]
    left = [c.name for c in sync if bench.run(c, True)]
    assert not left, f"returned with work in flight: {left}"


def test_table_too_large_for_the_ring_ends_synchronously_and_the_next_call_enqueues_again(cases):
    _, bench, all_cases, big = cases
    assert big.make()["out"].shape[1] * 65 * 4 > 2 << 20
    first, after = bench.run_seq([big, all_cases["td_resample2d"]], True)
    assert not first, "returned while an upload was still reading the caller's tap table"
    assert after, "the call after it waited for the stream"
