"""The three arguments the bounded samplers used to refuse, on the MI355X: autoguidance on a model with conditioning-image channels, score scaling
(`_scale_score`), custom blend windows.  Against the reference's own outputs (tests/golden/sampler_args.npz, made by make_sampler_args_golden.py), against the
float64 twin (tests/_sampler_args_twin.py) element by element and step by step, and bit for bit against the entry points that existed before.

bf16 end to end, alpha != 1 (printed by test_reference_parity_bf16, not asserted; the per-step test holds those cases): see DESIGN.md."""
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_args_twin as sa   # noqa: E402
import _sampler_twin as tw        # noqa: E402
import _tile_twin as tt           # noqa: E402
from _engine_opts import engine_options_guard, pinned  # noqa: F401,E402  (autouse guard: every test starts and ends on the shipped options)
from conftest import rel_rms      # noqa: E402

pytestmark = pytest.mark.gpu

SD = 0.5
LABELS = ("@x", "@m1", "@m2", "@xin")
DEC_CASES = {"plain": (1.0, 1.0), "guided": (1.5, 1.0), "alpha1p1": (1.0, 1.1), "alpha1p3": (1.0, 1.3), "guided_alpha1p1": (1.5, 1.1)}   # (guidance, alpha)


def window_constant(size, device, dtype):
    return torch.ones(1, 1, size, size, device=device, dtype=dtype)


def window_sin2(size, device, dtype):
    i = torch.arange(size, device=device, dtype=dtype)
    r = torch.sin(math.pi * (i + 0.5) / size) ** 2 + 0.05
    return (r[:, None] * r[None, :])[None, None]


WINDOWS = {"const": window_constant, "sin2": window_sin2}


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def zoo(td):
    """models, built on first use and shared.  dec / dec_guide: the golden generator's decoder pair; *_twin: same-width pairs for every storage type"""
    from oracle.unet import DECODER_CONFIG, synth_state_dict, tiny_config
    dec = dict(DECODER_CONFIG, layers_per_block=1)
    cfgs = {"dec": (dec, 11), "dec_guide": (dict(dec, model_channel_mults=[1, 2, 2, 2]), 12), "dec_guide64": (dec, 13), "base": (tiny_config(64, 1), 77), "base_guide": (tiny_config(64, 1), 78),
            "decoder_full": (dict(DECODER_CONFIG), 2468)}
    sds, models = {}, {}

    def get(which, T):
        cfg, seed = cfgs[which]
        if which not in sds:
            sds[which] = synth_state_dict(cfg, seed=seed)
        if (which, T) not in models:
            models[(which, T)] = td.EDMUnet2D(**cfg, dtype=T).load_state_dict(sds[which])
        return cfg, models[(which, T)]

    yield get
    for m in models.values():
        m.close()


def _sched(td):
    return td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=SD)


def _dec_inputs():
    from oracle import rng
    return torch.from_numpy(rng.standard_normal(921, (2, 1, 32, 32))) * 80.0, torch.from_numpy(rng.standard_normal(922, (2, 4, 32, 32)))


# ------------------------------------------------------------------------------------------------------------------ 1. reference parity
@pytest.mark.parametrize("case", list(DEC_CASES))
def test_reference_parity_fp32_decoder_diffusion(td, zoo, golden, case):
    g = golden("sampler_args")
    (_, m), (_, guide) = zoo("dec", "fp32"), zoo("dec_guide", "fp32")
    noise, cimg = _dec_inputs()
    gs, alpha = DEC_CASES[case]
    got = td.sample_decoder_diffusion_tiled(m, _sched(td), cimg, noise, num_steps=5, guidance_model=guide, guidance_scale=gs, score_scaling=alpha).cpu().numpy()
    e = rel_rms(got, g["dec_diffusion:" + case])
    print(f"\ndecoder diffusion {case} (guidance {gs}, alpha {alpha}), fp32 mode: rel-RMS vs the reference {e:.2e} (reference fp32 vs float64: {float(g['e_ref:' + case]):.2e})")
    assert e < 1e-5
    if case != "plain":       # the arguments matter: the same call without them is far from this golden
        plain = td.sample_decoder_diffusion_tiled(m, _sched(td), cimg, noise, num_steps=5, guidance_model=guide, guidance_scale=1.0, score_scaling=1.0).cpu().numpy()
        off = rel_rms(plain, g["dec_diffusion:" + case])
        print(f"  without the arguments: {off:.2e}")
        assert off > 1e-4


def test_reference_parity_bf16(td, zoo, golden):
    """guided, alpha = 1 against the project's guided bf16 bound (3e-2); the alpha != 1 cases are printed only (the per-step test holds them)"""
    g = golden("sampler_args")
    (_, m), (_, guide) = zoo("dec", "bf16"), zoo("dec_guide", "bf16")
    noise, cimg = _dec_inputs()
    figs = {}
    for case, (gs, alpha) in DEC_CASES.items():
        got = td.sample_decoder_diffusion_tiled(m, _sched(td), cimg, noise, num_steps=5, guidance_model=guide, guidance_scale=gs, score_scaling=alpha).cpu().numpy()
        figs[case] = rel_rms(got, g["dec_diffusion:" + case])
        assert np.all(np.isfinite(got))
    print("\ndecoder diffusion, bf16 mode, rel-RMS vs the reference: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert figs["guided"] < 3e-2


@pytest.mark.parametrize("wname", list(WINDOWS))
def test_reference_parity_fp32_decoder_consistency_windows(td, zoo, golden, wname):
    from oracle import rng
    g = golden("sampler_args")
    _, m = zoo("dec", "fp32")
    cn, cc = torch.from_numpy(rng.standard_normal(925, (2, 1, 40, 56))), torch.from_numpy(rng.standard_normal(926, (2, 4, 40, 56)))
    sch = _sched(td)
    sch.set_timesteps(20)
    one = td.sample_decoder_consistency_tiled(m, sch, cc, cn, 32, 24, weight_window_fn=WINDOWS[wname]).cpu().numpy()
    three = td.sample_decoder_consistency_tiled(m, sch, cc, cn, 32, 24, intermediate_t=[float(np.arctan(0.35 / 0.5)), 0.2], weight_window_fn=WINDOWS[wname]).cpu().numpy()
    e1, e3 = rel_rms(one, g[f"dec_consistency_1step:{wname}"]), rel_rms(three, g[f"dec_consistency_3step:{wname}"])
    lin = td.sample_decoder_consistency_tiled(m, sch, cc, cn, 32, 24).cpu().numpy()
    off = rel_rms(lin, g[f"dec_consistency_1step:{wname}"])
    print(f"\ndecoder consistency, window {wname}: rel-RMS vs the reference {e1:.2e} (1 step), {e3:.2e} (3 steps); the linear window against this golden {off:.2e}")
    assert e1 < 1e-5 and e3 < 1e-5 and off > 1e-4


def test_reference_parity_fp32_base_samplers_windows(td, zoo, golden):
    from oracle import tiling
    g = golden("sampler_args")
    _, m = zoo("base", "fp32")
    kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5))
    cond = tiling.synthetic_cond_grid(3, 3)
    y = td.sample_base_diffusion(m, _sched(td), (1, 5, 32, 32), cond, steps=6, tile_size=16, noise_seed=42 + 5819, weight_window_fn=window_sin2, **kw).cpu().numpy()
    lin = td.sample_base_diffusion(m, _sched(td), (1, 5, 32, 32), cond, steps=6, tile_size=16, noise_seed=42 + 5819, **kw).cpu().numpy()
    e, off = rel_rms(y, g["base_diffusion:sin2"]), rel_rms(lin, g["base_diffusion:sin2"])
    yc = td.sample_base_consistency(m, _sched(td), (1, 5, 32, 32), cond, intermediate_t=float(np.arctan(0.35 / 0.5)), tile_size=16, weight_window_fn=window_constant, **kw).cpu().numpy()
    linc = td.sample_base_consistency(m, _sched(td), (1, 5, 32, 32), cond, intermediate_t=float(np.arctan(0.35 / 0.5)), tile_size=16, **kw).cpu().numpy()
    ec, offc = rel_rms(yc, g["base_consistency_2phase:const"]), rel_rms(linc, g["base_consistency_2phase:const"])
    print(f"\nbase diffusion, sin2 window: {e:.2e} (linear window against it {off:.2e}); base consistency 2 phases, constant window: {ec:.2e} (linear {offc:.2e})")
    assert e < 1e-5 and ec < 1e-5 and off > 1e-4 and offc > 1e-4


# ------------------------------------------------------------------------------------------------------------------ the engine call
class Run:
    """one sampler case through td_sample_edm_ext; run(k) = the state after k steps ("sampler_stop_after" = k)"""

    def __init__(self, cfg, m, T, n, H, W, n_steps, order, guide=None, gscale=1.3, alpha=1.0, seed=7):
        from oracle import rng, schedule
        from terrain_diffusion_amd.engine import get_engine
        self.eng, self.m, self.T, self.n, self.H, self.W, self.n_steps, self.order, self.guide, self.gscale, self.alpha = get_engine("cuda"), m, T, n, H, W, n_steps, order, guide, gscale, alpha
        self.C, self.Cin = cfg["out_channels"], cfg["in_channels"]
        self.sig = schedule.karras_sigmas(n_steps)[0].contiguous()
        self.table = tw.engine_table(self.sig.numpy(), SD, order, True)
        self.cs = sa.score_table(self.sig, SD)
        s0 = np.float32(self.sig[0].item())
        self.c_in0 = np.float32(1.0) / np.sqrt(s0 * s0 + np.float32(SD) * np.float32(SD))
        self.x0 = (torch.from_numpy(rng.standard_normal(seed, (n, self.C, H, W))) * float(s0)).contiguous()
        self.img = torch.from_numpy(rng.standard_normal(seed + 1, (n, self.Cin - self.C, H, W))).contiguous() if self.Cin > self.C else None
        conds = [torch.from_numpy(rng.standard_normal(seed + 2 + i, (n, c[1]))) for i, c in enumerate(cfg.get("conditional_inputs", []))]
        self.cond = m.cond_rows(conds, n, "cuda") if conds else None
        self.chunk = tw.CHUNK[T]

    def sample(self, k=None, rows=None, alpha=None, via="ext", **opts):
        from terrain_diffusion_amd._lib import lib, check, EdmExt
        from terrain_diffusion_amd.engine import ptr
        sl = rows or slice(0, self.n)
        x = self.x0[sl].clone().cuda()
        cond = self.cond[sl].contiguous() if self.cond is not None else None
        img = self.img[sl].contiguous().cuda() if self.img is not None else None
        n, cimg = x.shape[0], self.Cin - self.C
        alpha = self.alpha if alpha is None else alpha
        torch.cuda.synchronize()
        with pinned(self.eng, solver_order=self.order, sampler_stop_after=-1 if k is None else k, **opts):
            if via == "ext":
                a = EdmExt(n=n, H=self.H, W=self.W, n_steps=self.n_steps, sigmas_host=ptr(self.sig), sigma_data=SD, cond=ptr(cond), x=ptr(x), cond_img=ptr(img), cimg_channels=cimg,
                           guide=self.guide._h if self.guide is not None else None, guidance_scale=float(self.gscale), score_scaling=float(alpha),
                           score_cs_host=C.c_void_p(self.cs.ctypes.data) if alpha != 1.0 else None)
                check(lib().td_sample_edm_ext(self.m._h, C.byref(a)))
            elif via == "img":
                check(lib().td_sample_edm_img(self.m._h, n, self.H, self.W, self.n_steps, ptr(self.sig), SD, ptr(cond), ptr(img), cimg, ptr(x)))
            elif via == "plain":
                check(lib().td_sample_edm(self.m._h, n, self.H, self.W, self.n_steps, ptr(self.sig), SD, ptr(cond), ptr(x)))
            else:
                check(lib().td_sample_edm_guided(self.m._h, self.guide._h, float(self.gscale), n, self.H, self.W, self.n_steps, ptr(self.sig), SD, ptr(cond), ptr(x)))
            torch.cuda.synchronize()
        return x.cpu()

    def read(self, label, m=None):
        return (m or self.m).read_activation(self.n, self.H, self.W, label, max_elems=self.n * max(self.chunk, 8) * self.H * self.W).numpy()

    def run(self, k):
        x = self.sample(k)
        S = {l[1:]: self.read(l) for l in LABELS}
        S["F"] = self.read("out_conv")[:, :self.C] if k >= 1 else None
        S["Fg"] = self.read("out_conv", self.guide)[:, :self.C] if k >= 1 and self.guide is not None else None
        S["xin_g"] = self.read("@xin", self.guide) if self.guide is not None else None
        assert np.array_equal(x.numpy(), S["x"]), f"k = {k}: the sample the call returns is not the plan's @x"
        return S


# ------------------------------------------------------------------------------------------------------------------ 2. per step, every element
# A covering design of the issue's settings (shape x storage type x order x guide x alpha): every storage type meets both shapes, every order, both guide
# settings and every alpha; every alpha meets every order and both guide settings.  n = 3, 16 x 16, 4 steps each.
STEP_CASES = [(shape, T, order, guided, alpha)
              for shape in ("dec", "base")
              for ti, T in enumerate(("fp32", "bf16", "fp16"))
              for j, alpha in enumerate(sa.ALPHAS)
              for order, guided in [(1 + (j + ti + (shape == "base")) % 3, (j + ti) % 2 == 0), (1 + (j + ti + 1 + (shape == "base")) % 3, (j + ti) % 2 == 1)]]


@pytest.mark.parametrize("shape,T,order,guided,alpha", STEP_CASES, ids=[f"{s}-{T}-order{o}-{'guided' if g else 'plain'}-alpha{a}" for s, T, o, g, a in STEP_CASES])
def test_every_scaled_step_elementwise(zoo, shape, T, order, guided, alpha):
    t0 = time.time()
    cfg, m = zoo(shape, T)
    guide = zoo({"dec": "dec_guide64", "base": "base_guide"}[shape], T)[1] if guided else None
    r = Run(cfg, m, T, 3, 16, 16, 4, order, guide, 1.3, alpha)
    assert (r.C, r.Cin) == {"dec": (1, 5), "base": (5, 5)}[shape]
    img = r.img.numpy() if r.img is not None else None
    S = r.run(0)
    viol = [f"k=0 exact {n}: {c} elements differ" for n, c in tw.check_start(S, r.x0.numpy(), r.c_in0, T, r.C, r.Cin, img).items()]
    stats = []
    for i in range(r.n_steps):
        S1 = r.run(i + 1)
        k = tw.row(r.table, i)
        st = sa.judge_step(k, (alpha, r.cs[i][0], r.cs[i][1], SD), S, S1, S1["Fg"], r.gscale if guided else None)
        stats.append(st)
        viol += [f"step {i} (order {st['order']}): {v}" for v in sa.verdict(st)]
        ex = tw.check_step(k, S, S1, T, r.C, r.Cin, order == 3, img, r.gscale if guided else None)["exact_bad"]       # the hand-offs of the plain step, unchanged
        viol += [f"step {i}: exact {n}: {c} elements differ ({tw.WHERE.get(n, '')})" for n, c in ex.items()]
        S = S1
    a, b = max(max(s["A_x"], s["A_m0"]) for s in stats), max(max(s["B_x"], s["B_m0"]) for s in stats)
    med = max(max(s["median_x"], s["median_m0"]) for s in stats)
    print(f"\n{shape} {T} order {order} {'guided 1.3' if guided else 'plain'} alpha {alpha}: {stats[0]['elements']} elements x {len(stats)} steps; worst err / E {a:.3f}, "
          f"B {b / sa.U:.2f} u (<= {(sa.C_RMS_SS_GUIDED if guided else sa.C_RMS_SS) / sa.U:.1f}), max median E / scale {med / sa.U:.1f} u (cap {sa.CAP_SS / sa.U:.1f}); {time.time() - t0:.1f} s")
    assert stats[0]["elements"] == 3 * r.C * 256 and len(stats) == 4
    assert not viol, "\n".join(viol[:12])


# ------------------------------------------------------------------------------------------------------------------ 3. unchanged paths
def test_ext_equals_the_entry_points_it_generalises(zoo):
    cfg, m = zoo("base", "bf16")
    _, guide = zoo("base_guide", "bf16")
    r = Run(cfg, m, "bf16", 3, 16, 16, 5, 2)
    assert torch.equal(r.sample(via="ext"), r.sample(via="plain"))
    rg = Run(cfg, m, "bf16", 3, 16, 16, 5, 2, guide, 1.4)
    a, b = rg.sample(via="ext"), rg.sample(via="guided")
    assert torch.equal(a, b) and not torch.equal(a, r.sample(via="plain"))
    cfgd, md = zoo("dec", "bf16")
    rd = Run(cfgd, md, "bf16", 3, 16, 16, 5, 2)
    assert torch.equal(rd.sample(via="ext"), rd.sample(via="img"))
    assert torch.isfinite(a).all()


def _blend_args(Hc, Wc, size, stride):
    rows, cols = tt.tile_starts(Hc, size, stride), tt.tile_starts(Wc, size, stride)
    idx = [(a, b) for a in range(len(rows)) for b in range(len(cols))]
    return np.asarray(rows, np.int32), np.asarray(cols, np.int32), np.asarray([a for a, _ in idx], np.int32), np.asarray([b for _, b in idx], np.int32)


def _blend(eng, tiles, C_, Hc, Wc, size, rows, cols, wi, wj, accumulate, prior, window, entry):
    """td_blend_windows (entry "old") / td_blend_windows_w with `window` (None, host array or device tensor); returns the canvas (C + 1, Hc, Wc) on the host"""
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import ptr
    canvas = (torch.from_numpy(prior).clone() if accumulate else torch.full((C_ + 1, Hc, Wc), 7.0)).cuda()
    t = torch.from_numpy(tiles).cuda()
    torch.cuda.synchronize()
    args = (eng._h, ptr(canvas), C_, Hc, Wc, size, len(rows), ptr(rows), len(cols), ptr(cols), len(wi), ptr(wi), ptr(wj), ptr(t), int(accumulate))
    if entry == "old":
        check(lib().td_blend_windows(*args))
    else:
        check(lib().td_blend_windows_w(*args, ptr(window)))
    torch.cuda.synchronize()
    return canvas.cpu().numpy()


def test_blend_w_with_the_linear_window_is_td_blend_windows(td):
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.sampling import _linear_weight_window
    eng = get_engine("cuda")
    rs = np.random.RandomState(11)
    C_, Hc, Wc, size = 5, 24, 40, 16           # ragged: 40 = 16 + 8 + 8 + 8, the last start clamped
    rows, cols, wi, wj = _blend_args(Hc, Wc, size, 8)
    tiles = rs.standard_normal((len(wi), C_, size, size)).astype(np.float32)
    prior = rs.standard_normal((C_ + 1, Hc, Wc)).astype(np.float32)
    lin = _linear_weight_window(size)[0, 0].contiguous()
    for accumulate in (0, 1):
        old = _blend(eng, tiles, C_, Hc, Wc, size, rows, cols, wi, wj, accumulate, prior, None, "old")
        for window in (None, lin, lin.cpu().numpy()):
            new = _blend(eng, tiles, C_, Hc, Wc, size, rows, cols, wi, wj, accumulate, prior, window, "w")
            assert np.array_equal(old, new), (accumulate, type(window))


# ------------------------------------------------------------------------------------------------------------------ 4. windows, every element
def _border_zero(size):
    w = np.zeros((size, size), np.float32)
    w[2:-2, 2:-2] = tt.weight_window(size)[2:-2, 2:-2]
    return w


@pytest.mark.parametrize("size,Hc,Wc,stride", [(16, 24, 40, 8), (32, 40, 56, 24)])
@pytest.mark.parametrize("wname", ["const", "sin2", "zero border"])
def test_windowed_blend_elementwise(td, size, Hc, Wc, stride, wname):
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.sampling import blend_normalize
    eng = get_engine("cuda")
    rs = np.random.RandomState(size + len(wname))
    C_ = 5
    rows, cols, wi, wj = _blend_args(Hc, Wc, size, stride)
    if wname == "zero border":       # one window only: its border stays uncovered
        rows, cols, wi, wj = rows[:1], cols[:1], wi[:1], wj[:1]
        window = _border_zero(size)
    else:
        window = WINDOWS[wname](size, "cpu", torch.float32)[0, 0].contiguous().numpy()
    tiles = rs.standard_normal((len(wi), C_, size, size)).astype(np.float32)
    got = _blend(eng, tiles, C_, Hc, Wc, size, rows, cols, wi, wj, 0, None, window, "w")
    ref, E = sa.blend_ref(tiles, window, C_, Hc, Wc, size, rows, cols, wi, wj)
    st = tt.judge(got, ref, E)
    print("\n" + tt.line("blend", f"window {wname}, tile {size}", got.shape, st))
    assert not tt.verdict("blend", st), tt.verdict("blend", st)
    out = blend_normalize(eng, torch.from_numpy(got).cuda(), 1.0).cpu().numpy()
    zero_w = ref[C_] == 0
    assert np.array_equal(np.isnan(out), np.broadcast_to(zero_w, out.shape)), "NaN exactly where the summed weight is 0"
    assert bool(zero_w.any()) == (wname == "zero border")


# ------------------------------------------------------------------------------------------------------------------ 5. stale graph
def test_a_captured_graph_is_not_replayed_with_another_alpha(zoo):
    cfg, m = zoo("dec", "bf16")
    r = Run(cfg, m, "bf16", 3, 16, 16, 5, 2)
    a, b, c = r.sample(alpha=1.1), r.sample(alpha=1.0), r.sample(alpha=1.1)
    assert torch.equal(a, c) and torch.equal(b, r.sample(via="img")) and not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ 6. two lanes
def test_two_lanes_guided_with_cond_img(zoo):
    cfg, m = zoo("dec", "bf16")
    _, guide = zoo("dec_guide64", "bf16")
    r = Run(cfg, m, "bf16", 5, 16, 16, 4, 2, guide, 1.5, 1.1)
    both = r.sample(dual_stream=1, dual_stream_min_batch=4)
    halves = torch.cat([r.sample(rows=slice(0, 2), dual_stream=0), r.sample(rows=slice(2, 5), dual_stream=0)])
    assert torch.isfinite(both).all()
    assert torch.equal(both[:2], halves[:2]) and torch.equal(both[2:], halves[2:])


# ------------------------------------------------------------------------------------------------------------------ 7. few-cout output conv under the fused solver
def test_fewcout_output_conv_fused_equals_unfused(zoo):
    """decoder-shaped model, n = 2, 128 x 128, 3 steps: the fused solver epilogue of the few-cout output conv gives the bits of the separate step kernel"""
    cfg, m = zoo("decoder_full", "bf16")
    r = Run(cfg, m, "bf16", 2, 128, 128, 3, 2)
    fused, unfused = r.sample(via="img", fuse_solver=1), r.sample(via="img", fuse_solver=0)
    assert torch.isfinite(fused).all() and torch.equal(fused, unfused)
    f0, u0 = r.sample(via="img", fuse_solver=1, fewcout=0), r.sample(via="img", fuse_solver=0, fewcout=0)
    assert torch.equal(f0, u0)
