"""The solver step and the sampler's hand-offs on the MI355X, element by element, against their float64 twin (tests/_sampler_twin.py).

Trajectories: with the engine option "sampler_stop_after" = k the state after k steps is read back ("@x", "@m1", "@m2", "@xin", "out_conv"); runs k and k + 1 give the
inputs and outputs of step k, and every step of every case is held to criterion A on every element, criterion B, the cap on the bound's median and the exact hand-offs.
The engine's determinism, which that rests on, is asserted itself.  The consistency sampler's two kernels likewise.

The fused epilogue (EPI_DPM_STEP): for every arm -- kernel flavour / tile shape / storage type / map shape of the output conv -- the state after every k of a 4-step
third-order run (lower_order_final = 0: orders 1, 2, 3, 1, so that every branch of dpm_update runs in the epilogue) is bit-identical to the separate kernel's, and the
flavour that carried `out_conv` is read from the profile labels.  The planner does give `out_conv` ks > 1 (ks 3 on the per-tap kernel at n = 1 and 2 and on conv_glds
with sb = 0, ks 6 in fp32 mode), so the split-K reduce kernel's epilogue is among the arms; the closing test asserts it.  One printed line per case."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_twin as tw
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

SD = 0.5
LABELS = ("@x", "@m1", "@m2", "@xin")
FUSED_SEEN = {}        # arm -> (flavour tag, ksplit) of the fused out_conv: read by the closing test
SUMMARY = []


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def zoo(td):
    """models, built on first use and shared"""
    from oracle.unet import BASE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    cfgs = {"tiny": (tiny_config(64, 1), 77), "tiny_guide": (tiny_config(64, 1), 78), "tiny_img": (tiny_config(64, 1, in_channels=7, out_channels=5), 79),
            "base": (dict(BASE_CONFIG), 1234), "decoder": (dict(DECODER_CONFIG), 2468)}
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


class Run:
    """one sampler case on the engine: run(k) = the state after k steps, as tests/_sampler_twin.py's check_trajectory takes it"""

    def __init__(self, cfg, m, T, n, H, W, n_steps, order, lof=1, guide=None, gscale=1.3, seed=7):
        from oracle import rng, schedule
        from terrain_diffusion_amd.engine import get_engine
        self.eng, self.m, self.T, self.n, self.H, self.W, self.n_steps, self.order, self.lof, self.guide, self.gscale = get_engine("cuda"), m, T, n, H, W, n_steps, order, lof, guide, gscale
        self.C, self.Cin = cfg["out_channels"], cfg["in_channels"]
        self.sig = schedule.karras_sigmas(n_steps)[0].contiguous()
        self.table = tw.engine_table(self.sig.numpy(), SD, order, bool(lof))
        s0 = np.float32(self.sig[0].item())
        self.c_in0 = np.float32(1.0) / np.sqrt(s0 * s0 + np.float32(SD) * np.float32(SD))
        self.x0 = (torch.from_numpy(rng.standard_normal(seed, (n, self.C, H, W))) * float(s0)).contiguous()
        self.img = torch.from_numpy(rng.standard_normal(seed + 1, (n, self.Cin - self.C, H, W))).contiguous() if self.Cin > self.C else None
        conds = [torch.from_numpy(rng.standard_normal(seed + 2 + i, (n, c[1]))) for i, c in enumerate(cfg.get("conditional_inputs", []))]
        self.cond = m.cond_rows(conds, n, "cuda") if conds else None
        self.chunk = tw.CHUNK[T]

    def sample(self, k, fuse=0, rows=None):
        """the engine call: sampler_stop_after = k (None: unset), fuse_solver = fuse; returns the x the call hands back.  rows: a slice of the batch"""
        from terrain_diffusion_amd._lib import lib, check
        from terrain_diffusion_amd.engine import ptr
        e, sl = self.eng, rows or slice(0, self.n)
        x = self.x0[sl].clone().cuda()
        cond = self.cond[sl].contiguous() if self.cond is not None else None
        img = self.img[sl].contiguous().cuda() if self.img is not None else None
        n = x.shape[0]
        with pinned(e, solver_order=self.order, lower_order_final=self.lof, fuse_solver=fuse, sampler_stop_after=-1 if k is None else k):
            if self.guide is not None:
                check(lib().td_sample_edm_guided(self.m._h, self.guide._h, float(self.gscale), n, self.H, self.W, self.n_steps, ptr(self.sig), SD, ptr(cond), ptr(x)))
            else:
                check(lib().td_sample_edm_img(self.m._h, n, self.H, self.W, self.n_steps, ptr(self.sig), SD, ptr(cond), ptr(img), self.Cin - self.C, ptr(x)))
            torch.cuda.synchronize()
        return x.cpu()

    def read(self, label, m=None):
        m = m or self.m
        return m.read_activation(self.n, self.H, self.W, label, max_elems=self.n * max(self.chunk, 8) * self.H * self.W).numpy()

    def state(self, with_F):
        S = {l[1:]: self.read(l) for l in LABELS}
        S["F"] = self.read("out_conv")[:, :self.C] if with_F else None
        S["Fg"] = self.read("out_conv", self.guide)[:, :self.C] if with_F and self.guide is not None else None
        S["xin_g"] = self.read("@xin", self.guide) if self.guide is not None else None
        return S

    def run(self, k):
        x = self.sample(k, fuse=0)
        S = self.state(with_F=k >= 1)
        assert np.array_equal(x.numpy(), S["x"]), f"k = {k}: the sample the call returns is not the plan's @x"
        return S


# name -> (model, T, n, H, W, n_steps, solver_order, lower_order_final, guided)
TRAJ = {
    "fp32 order 3, 6 steps, n3 16x16": ("tiny", "fp32", 3, 16, 16, 6, 3, 1, False),
    "bf16 order 3, 6 steps, n3 16x16": ("tiny", "bf16", 3, 16, 16, 6, 3, 1, False),
    "fp16 order 3, 6 steps, n3 16x16": ("tiny", "fp16", 3, 16, 16, 6, 3, 1, False),
    "bf16 order 1, 6 steps, n3 16x16": ("tiny", "bf16", 3, 16, 16, 6, 1, 1, False),
    "bf16 order 2, 6 steps, n3 16x16": ("tiny", "bf16", 3, 16, 16, 6, 2, 1, False),
    "bf16 order 3 without lower_order_final, 6 steps, n3 16x16": ("tiny", "bf16", 3, 16, 16, 6, 3, 0, False),
    "bf16 order 3, 6 steps, n2 24x40": ("tiny", "bf16", 2, 24, 40, 6, 3, 1, False),
    "fp32 order 2, 6 steps, n2 24x40": ("tiny", "fp32", 2, 24, 40, 6, 2, 1, False),
    "bf16 order 3, 16 steps, n3 16x16": ("tiny", "bf16", 3, 16, 16, 16, 3, 1, False),
    "bf16 autoguided 1.3, order 3, 6 steps, n3 16x16": ("tiny", "bf16", 3, 16, 16, 6, 3, 1, True),
    "fp32 autoguided 1.3, order 2, 6 steps, n2 24x40": ("tiny", "fp32", 2, 24, 40, 6, 2, 1, True),
    "bf16 conditioning image (7 in, 5 out), order 3, 6 steps, n3 16x16": ("tiny_img", "bf16", 3, 16, 16, 6, 3, 1, False),
    "fp16 conditioning image (7 in, 5 out), order 2, 6 steps, n2 24x40": ("tiny_img", "fp16", 2, 24, 40, 6, 2, 1, False),
    "fp32 conditioning image (7 in, 5 out), order 3, 6 steps, n2 24x40": ("tiny_img", "fp32", 2, 24, 40, 6, 3, 1, False),
}
ORDERS = {(3, 1, 6): "123321", (3, 0, 6): "123331", (1, 1, 6): "111111", (2, 1, 6): "122221", (3, 1, 16): "12" + "3" * 13 + "1"}


@pytest.mark.parametrize("name", list(TRAJ))
def test_every_step_elementwise(zoo, name):
    which, T, n, H, W, n_steps, order, lof, guided = TRAJ[name]
    t0 = time.time()
    cfg, m = zoo(which, T)
    guide = zoo("tiny_guide", T)[1] if guided else None
    r = Run(cfg, m, T, n, H, W, n_steps, order, lof, guide)
    assert "".join(str(int(v)) for v in r.table[:, 11]) == ORDERS[(order, lof, n_steps)]
    img = r.img.numpy() if r.img is not None else None
    stats, viol = tw.check_trajectory(r.run, r.table, T, r.C, r.Cin, order == 3, r.x0.numpy(), r.c_in0, img, r.gscale if guided else None)
    print("\n" + tw.line(name, stats, time.time() - t0))
    SUMMARY.append((name, stats, time.time() - t0))
    assert stats[0]["elements"] == n * r.C * H * W and len(stats) == n_steps        # every element of every step, nothing skipped
    assert not viol, "\n".join(viol[:12])


def test_the_engine_is_deterministic_at_every_read_back_label(zoo):
    """two runs at the same k agree bit for bit on "@x", "@m1", "@m2", "@xt", "@xin" (what pairing run k with run k + 1 rests on), after other calls in between"""
    cfg, m = zoo("tiny", "bf16")
    r = Run(cfg, m, "bf16", 3, 16, 16, 6, 3)
    for k in (1, 3, 6):
        r.sample(k)
        a = {l: r.read(l) for l in LABELS + ("@xt",)}
        r.sample(6 if k < 6 else 2)                    # leaves another history behind
        r.sample(k)
        for l in a:
            assert np.array_equal(a[l], r.read(l)), (k, l)


def test_without_the_option_the_run_is_the_whole_trajectory(zoo):
    cfg, m = zoo("tiny", "bf16")
    r = Run(cfg, m, "bf16", 3, 16, 16, 6, 3)
    full = r.sample(None)
    assert torch.equal(full, r.sample(6)) and torch.equal(full, r.sample(9)) and not torch.equal(full, r.sample(5))
    assert torch.equal(full, r.sample(None, fuse=1))


# ------------------------------------------------------------------------------------------------------------------ consistency sampler
@pytest.mark.parametrize("which,T,with_sample,t", [("tiny", "bf16", True, 1.1), ("tiny", "bf16", False, 1.5607), ("tiny", "fp32", True, 0.3), ("tiny_img", "fp16", True, 1.1),
                                                   ("tiny_img", "bf16", False, 1.5607)])
def test_consistency_sampler_elementwise(zoo, which, T, with_sample, t):
    from oracle import rng
    from terrain_diffusion_amd.sampling import consistency_step
    t0 = time.time()
    cfg, m = zoo(which, T)
    n, H, W, C, Cin = 2, 24, 40, cfg["out_channels"], cfg["in_channels"]
    sample = torch.from_numpy(rng.standard_normal(21, (n, C, H, W))).contiguous() if with_sample else None
    z = torch.from_numpy(rng.standard_normal(22, (n, C, H, W))).contiguous()
    img = torch.from_numpy(rng.standard_normal(23, (n, Cin - C, H, W))).contiguous() if Cin > C else None
    cond = m.cond_rows([torch.from_numpy(rng.standard_normal(24, (n, 58)))], n, "cuda")
    out = consistency_step(m, t, SD, sample.cuda() if with_sample else None, z.cuda(), cond=cond, cond_img=img.cuda() if img is not None else None)
    torch.cuda.synchronize()
    rd = lambda l: m.read_activation(n, H, W, l, max_elems=n * 64 * H * W).numpy()
    xt, xin, F = rd("@xt"), rd("@xin"), rd("out_conv")[:, :C]
    smp = sample.numpy() if with_sample else np.zeros((n, C, H, W), np.float32)
    st = tw.check_consistency(t, SD, smp, z.numpy(), xt, xin, F, out.cpu().numpy(), T, C, Cin, img.numpy() if img is not None else None)
    print(f"\nconsistency {which} {T} sample={with_sample} t={t}: {st['elements']} elements; x_t worst err / E {st['A_xt']:.3f}, B {st['B_xt'] / tw.U:.2f} u; out worst err / E "
          f"{st['A_out']:.3f}, B {st['B_out'] / tw.U:.2f} u; median E / |ref| {st['median_xt'] / tw.U:.1f} / {st['median_out'] / tw.U:.1f} u; {time.time() - t0:.1f} s")
    assert st["elements"] == n * C * H * W
    assert not tw.verdict_consistency(st), tw.verdict_consistency(st)


# ------------------------------------------------------------------------------------------------------------------ the fused epilogue
ANY = ("f0", "f2", "f4", "f5")     # the planner's choice for the 5-cout output conv under the arm's options: recorded, and judged over all arms by the closing test
# name -> (model, T, n, H, W, engine options (as in test_conv_ops_gpu.ARMS), flavour families the fused out_conv may be carried by)
FUSED = {
    "base bf16 n1 default plan": ("base", "bf16", 1, 64, 64, {}, ANY),
    "base bf16 n1 sb tile m2n2": ("base", "bf16", 1, 64, 64, dict(sb_mt=2, sb_nt=2), ANY),
    "base bf16 n1 sb tile m2n1": ("base", "bf16", 1, 64, 64, dict(sb_mt=2, sb_nt=1), ANY),
    "base bf16 n1 sb tile m1n2": ("base", "bf16", 1, 64, 64, dict(sb_mt=1, sb_nt=2), ANY),
    "base bf16 n1 sb tile m1n1": ("base", "bf16", 1, 64, 64, dict(sb_mt=1, sb_nt=1), ANY),
    "base bf16 n1 sb tile m4n1": ("base", "bf16", 1, 64, 64, dict(sb_mt=4, sb_nt=1), ANY),
    "base bf16 n1 s16 everywhere": ("base", "bf16", 1, 64, 64, dict(s16=2), ANY),
    "base bf16 n1 sb0 split-K": ("base", "bf16", 1, 64, 64, dict(sb=0, glds_splitk=1), ANY),
    "base bf16 n1 sb0 no split-K": ("base", "bf16", 1, 64, 64, dict(sb=0, glds_splitk=0), ANY),
    "base bf16 n2 per-tap kernel": ("base", "bf16", 2, 64, 64, dict(glds=0), ("f0",)),
    "base bf16 n1 per-tap kernel": ("base", "bf16", 1, 64, 64, dict(glds=0), ("f0",)),
    "base bf16 n8 default plan": ("base", "bf16", 8, 64, 64, {}, ANY),
    # the plan that ships: with dual_stream = 1 a 64-window batch of the grid sampler runs as two lanes of N = 32, each on this plan.  A 32-row call of its own
    # would itself split into two lanes of 16 (dual_stream_min_batch = 32), so the arm runs single-lane: one lane of the shipped 64-window call, on its own.
    "base bf16 n32 default plan": ("base", "bf16", 32, 64, 64, dict(dual_stream=0), ANY),
    "base bf16 n3 56x88": ("base", "bf16", 3, 56, 88, {}, ANY),
    "base bf16 n3 40x40": ("base", "bf16", 3, 40, 40, {}, ANY),
    "base fp16 n1 default plan": ("base", "fp16", 1, 64, 64, {}, ANY),
    "base fp32 n1": ("base", "fp32", 1, 64, 64, {}, ("f0",)),
    "decoder bf16 n2 128x128 fewcout": ("decoder", "bf16", 2, 128, 128, dict(fewcout=1), ("f6",)),
    "decoder bf16 n2 136x152 fewcout": ("decoder", "bf16", 2, 136, 152, dict(fewcout=1), ("f6",)),
    "decoder bf16 n2 136x152 no fewcout": ("decoder", "bf16", 2, 136, 152, dict(fewcout=0), ("f2", "f4")),
}


def _out_conv_flavour(eng):
    import _conv_twin as ct
    for r in eng.profile_ops():
        if r[0].startswith("out_conv ["):
            _, tag, ks = ct.flavour_of(r[0])
            return tag, ks
    raise AssertionError("no out_conv launch in the profile")


def _state(r, opts, k, fuse, profile=True):
    """one run under the arm's options: ({label: array}, (flavour tag, ksplit) of out_conv or None).  Read back under the same options: they are part of the plan's key"""
    eng = r.eng
    with pinned(eng, **opts):
        with pinned(eng, profile=int(profile)):
            eng.profile_read(reset=True)
            x = r.sample(k, fuse=fuse)
            tag = _out_conv_flavour(eng) if profile and k >= 1 else None
        eng.profile_read(reset=True)
        got = {l: r.read(l) for l in LABELS}
        assert np.array_equal(x.numpy(), got["@x"]) and np.all(np.isfinite(got["@x"]))
    return got, tag


def _differences(a, b, k, what):
    """[(k, label, differing elements, elements, largest |a - b| / rms(b))] over the four labels"""
    out = []
    for l in LABELS:
        d = int(np.count_nonzero(a[l] != b[l]))
        if d:
            out.append((k, l, d, a[l].size, float(np.abs(a[l].astype(np.float64) - b[l]).max() / np.sqrt(np.mean(b[l].astype(np.float64) ** 2))), what))
    return out


def _fused_against_unfused(r, opts, graph_too=False):
    """states after every k, fused (profile mode: eager, flavour from the labels) against the separate kernel; returns
    ((tag, ks) fused, (tag, ks) unfused, differences)"""
    tags, diffs = {}, []
    for k in range(r.n_steps + 1):
        sep, t0_ = _state(r, opts, k, 0)
        fus, t1_ = _state(r, opts, k, 1)
        tags[0], tags[1] = t0_ or tags.get(0), t1_ or tags.get(1)
        diffs += _differences(fus, sep, k, "fused")
        if graph_too:
            diffs += _differences(_state(r, opts, k, 1, profile=False)[0], sep, k, "graph-replayed fused")
    return tags[1], tags[0], diffs


def _say(diffs):
    return "; ".join(f"k = {k}, {l}: {d} of {size} elements of the {what} run differ from the separate kernel's (largest difference {rel:.2e} of the rms)" for k, l, d, size, rel, what in diffs[:6])


@pytest.mark.parametrize("arm", list(FUSED))
def test_fused_epilogue_is_bit_identical_on_every_flavour(zoo, arm):
    """The decoder arms are the input that failed first: the fused step of the few-cout output conv used to run on conv_glds's 128-pixel MFMA tile, whose fp32 sums
    are taken in another order than the VALU few-cout flavour's (f6) of the separate-kernel run, so F -- and with it @x, @m1, @xin -- differed in the last bits
    (k = 1: 5540 of 32768 elements at 128 x 128, 6839 of 41344 at 136 x 152).  conv_fewcout.hip now runs the shared solver epilogue itself: fused and
    unfused are both f6, on its ragged 16 x 16 tiles too; with `fewcout` = 0 both run the planner's MFMA kernel (ragged 16 x 8 tiles of conv_glds at 136 x 152)."""
    which, T, n, H, W, opts, families = FUSED[arm]
    t0 = time.time()
    cfg, m = zoo(which, T)
    r = Run(cfg, m, T, n, H, W, 4, 3, lof=0)
    assert "".join(str(int(v)) for v in r.table[:, 11]) == "1231"
    fused, unfused, diffs = _fused_against_unfused(r, opts, graph_too=arm in ("base bf16 n8 default plan", "decoder bf16 n2 136x152 fewcout"))
    FUSED_SEEN[arm] = fused
    print(f"\n{arm}: fused out_conv on {fused[0]} (ks {fused[1]}), unfused on {unfused[0]} (ks {unfused[1]}); @x, @m1, @m2, @xin of {n * cfg['out_channels'] * H * W} elements "
          + ("bit-identical after each of the 4 steps" if not diffs else "DIFFER: " + _say(diffs)) + f"; {time.time() - t0:.1f} s")
    assert fused[0].startswith(families), f"{arm}: the fused out_conv ran on {fused[0]}, meant {families}"
    if which == "decoder":                         # the VALU few-cout flavour with and without the solver step, or neither
        assert (unfused[0] == "f6") == bool(opts["fewcout"]) and unfused == fused, (unfused, fused)
    assert not diffs, _say(diffs)


def test_two_lanes_equal_the_single_lane_runs_of_their_halves(zoo):
    """dual_stream_min_batch lowered to 2, n = 3: lane one takes the first n / 2 = 1 tile, lane two the other 2; the sample equals single-lane runs of the halves"""
    cfg, m = zoo("base", "bf16")
    r = Run(cfg, m, "bf16", 3, 64, 64, 4, 3, lof=0)
    eng = r.eng
    with pinned(eng, dual_stream=1, dual_stream_min_batch=2):
        both = r.sample(None, fuse=1)
        with pinned(eng, dual_stream=0):
            halves = torch.cat([r.sample(None, fuse=1, rows=slice(0, 1)), r.sample(None, fuse=1, rows=slice(1, 3))])
    d = int((both != halves).sum())
    print(f"\ntwo lanes (1 + 2 tiles) against single-lane runs of the halves: {d} of {both.numel()} elements differ")
    assert torch.isfinite(both).all() and d == 0


def test_the_shipped_lane_threshold(zoo):
    """On the options that ship (dual_stream = 1, dual_stream_min_batch = 32, nothing pinned but the case's own solver order): a batch of n = 33 runs as lanes of
    n / 2 = 16 and 17 rows and equals, bit for bit, single-lane runs of rows [0, 16) and [16, 33); n = 31 stays below the threshold and equals the unsplit run."""
    from _engine_opts import SHIPPED
    assert SHIPPED["dual_stream"] == 1 and SHIPPED["dual_stream_min_batch"] == 32
    cfg, m = zoo("tiny", "bf16")
    r = Run(cfg, m, "bf16", 33, 16, 16, 4, 3, lof=0)
    assert r.eng.get_option("dual_stream", 1) == 1 and r.eng.get_option("dual_stream_min_batch", 32) == 32
    both = r.sample(None, fuse=1)
    with pinned(r.eng, dual_stream=0):
        halves = torch.cat([r.sample(None, fuse=1, rows=slice(0, 16)), r.sample(None, fuse=1, rows=slice(16, 33))])
        whole = r.sample(None, fuse=1)
    d = int((both != halves).sum())
    r31 = Run(cfg, m, "bf16", 31, 16, 16, 4, 3, lof=0)
    below = r31.sample(None, fuse=1)
    with pinned(r.eng, dual_stream=0):
        unsplit = r31.sample(None, fuse=1)
    d31 = int((below != unsplit).sum())
    print(f"\nshipped lane threshold: n = 33 against single-lane runs of rows [0, 16) and [16, 33): {d} of {both.numel()} elements differ "
          f"({int((both != whole).sum())} from the unsplit 33-row run); n = 31 against the unsplit run: {d31} of {below.numel()} differ")
    assert torch.isfinite(both).all() and torch.isfinite(below).all()
    assert d == 0 and d31 == 0


def test_every_flavour_carried_a_fused_output_conv():
    """reads what the arms recorded (belongs to a run of the whole file): the per-tap kernel, conv_glds, some conv_sb tile, conv_s16 and the few-cout kernel each
    ran the fused solver epilogue, and so did the split-K reduce kernel (an arm whose out_conv has ks > 1) behind the per-tap kernel and behind conv_glds."""
    assert len(FUSED_SEEN) == len(FUSED), f"only {len(FUSED_SEEN)} of {len(FUSED)} arms ran: run the whole file"
    tags = {t for t, _ in FUSED_SEEN.values()}
    print("\nfused out_conv flavours: " + ", ".join(sorted(tags)) + "; arms with ks > 1: " + (", ".join(a for a, (_, ks) in FUSED_SEEN.items() if ks > 1) or "none"))
    assert "f0" in tags and any(t.startswith("f2") for t in tags) and any(t.startswith("f4") for t in tags) and "f5c16" in tags and "f6" in tags, tags
    assert any(t == "f0" and ks > 1 for t, ks in FUSED_SEEN.values()) and any(t.startswith("f2") and ks > 1 for t, ks in FUSED_SEEN.values()), FUSED_SEEN


def test_summary():
    for name, stats, wall in SUMMARY:
        print(tw.line(name, stats, wall))
