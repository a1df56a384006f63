"""Every fused conv op of the network, element by element, against the float64 twin of the same op on the op's own stored inputs (tests/_conv_twin.py):
|hip - ref| <= half_ulp_T(ref) + E for EVERY element of every op (`attn_proj` from the stored attention output, like any 1x1 conv), and the sum-of-squares planes of every op that writes them
against the float64 sum of squares of the stored output.  One arm per kernel flavour / tile shape / storage type / map shape; each arm asserts from the
profile labels that the intended flavour really ran, and prints one line: ops, elements, worst (|err| - half_ulp) / E, share of elements whose stored value
is not RNE_T(ref), wall time.  A failure names the op, the flavour, the worst element and the bounding box of the failing ones."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_twin as ct
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

SEEN = {}          # arm -> {label: (tag, ksplit)}: which flavours were exercised, for the coverage test at the end of the file


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def zoo(td):
    """models and twins, built on first use and shared by the arms"""
    from oracle.unet import BASE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    cfgs = {"base": (dict(BASE_CONFIG), 1234), "decoder": (dict(DECODER_CONFIG), 2468), "tiny_attn": (tiny_config(64, 2, attn_resolutions=[128]), 77)}
    sds, models, twins = {}, {}, {}

    def get(which, T):
        cfg, seed = cfgs[which]
        if which not in sds:
            sds[which] = synth_state_dict(cfg, seed=seed)
        if (which, T) not in models:
            models[(which, T)] = td.EDMUnet2D(**cfg, dtype=T).load_state_dict(sds[which])
            twins[(which, T)] = ct.Twin(cfg, sds[which], T, "cuda")
        return cfg, models[(which, T)], twins[(which, T)]

    yield get
    for m in models.values():
        m.close()


def _tail_on_wide(tw, fl):
    return [l for l, (tag, _) in fl.items() if tag == "f2w" and any(s["taps"] == 1 for s in tw.by_label[l]["segs"])]


def _count(fl, *prefixes):
    return sum(tag.startswith(prefixes) for tag, _ in fl.values())


# name -> (model, T, n, H, W, engine options, check of the flavours that ran: f(flavours, twin) -> bool)
ARMS = {
    "base bf16 n64 default plan": ("base", "bf16", 64, 64, 64, {}, lambda fl, tw: _count(fl, "f2w") >= 10 and _count(fl, "f2b", "f2s") >= 10 and len({tag for tag, _ in fl.values()}) >= 3),
    # the plan that ships: with dual_stream = 1 a 64-window batch of the grid sampler runs as two lanes of N = 32 (LANE_ARMS below)
    "base bf16 n32 default plan": ("base", "bf16", 32, 64, 64, {}, lambda fl, tw: len(fl) == 79),
    "base bf16 n64 wide forced": ("base", "bf16", 64, 64, 64, dict(glds_wide=2), lambda fl, tw: _count(fl, "f2w") >= 40 and len(_tail_on_wide(tw, fl)) >= 4),
    "base bf16 n5 72x72 wide forced": ("base", "bf16", 5, 72, 72, dict(glds_wide=2), lambda fl, tw: _count(fl, "f2w") >= 20 and len(_tail_on_wide(tw, fl)) >= 2),
    "base bf16 n8 sb0 split-K": ("base", "bf16", 8, 64, 64, dict(sb=0, glds_splitk=1), lambda fl, tw: _count(fl, "f4", "f5") == 0 and sum(ks > 1 for _, ks in fl.values()) >= 10),
    "base bf16 n1 sb0 split-K": ("base", "bf16", 1, 64, 64, dict(sb=0, glds_splitk=1), lambda fl, tw: _count(fl, "f4", "f5") == 0 and sum(ks > 1 for _, ks in fl.values()) >= 40),
    "base bf16 n8 sb0 no split-K": ("base", "bf16", 8, 64, 64, dict(sb=0, glds_splitk=0), lambda fl, tw: _count(fl, "f4", "f5") == 0 and all(ks == 1 or tag == "f0" for tag, ks in fl.values())),
    "base bf16 n1 sb0 no split-K": ("base", "bf16", 1, 64, 64, dict(sb=0, glds_splitk=0), lambda fl, tw: _count(fl, "f4", "f5") == 0 and all(ks == 1 or tag == "f0" for tag, ks in fl.values())),
    "base bf16 n1 default plan": ("base", "bf16", 1, 64, 64, {}, lambda fl, tw: _count(fl, "f4", "f5") >= 70 and _count(fl, "f5") >= 15),
    "base bf16 n1 sb tile m2n2": ("base", "bf16", 1, 64, 64, dict(sb_mt=2, sb_nt=2), lambda fl, tw: _count(fl, "f4m2n2") >= 70),
    "base bf16 n1 sb tile m2n1": ("base", "bf16", 1, 64, 64, dict(sb_mt=2, sb_nt=1), lambda fl, tw: _count(fl, "f4m2n1") >= 70),
    "base bf16 n1 sb tile m1n2": ("base", "bf16", 1, 64, 64, dict(sb_mt=1, sb_nt=2), lambda fl, tw: _count(fl, "f4m1n2") >= 70),
    "base bf16 n1 sb tile m1n1": ("base", "bf16", 1, 64, 64, dict(sb_mt=1, sb_nt=1), lambda fl, tw: _count(fl, "f4m1n1") >= 70),
    "base bf16 n1 sb tile m4n1": ("base", "bf16", 1, 64, 64, dict(sb_mt=4, sb_nt=1), lambda fl, tw: _count(fl, "f4m4n1") >= 50),
    "base bf16 n1 s16 everywhere": ("base", "bf16", 1, 64, 64, dict(s16=2), lambda fl, tw: _count(fl, "f5c16") >= 70),
    "base bf16 n2 per-tap kernel": ("base", "bf16", 2, 64, 64, dict(glds=0), lambda fl, tw: all(tag == "f0" for tag, _ in fl.values())),
    "base bf16 n3 56x88": ("base", "bf16", 3, 56, 88, {}, lambda fl, tw: len(fl) == 79),
    "base bf16 n3 40x40": ("base", "bf16", 3, 40, 40, {}, lambda fl, tw: len(fl) == 79),
    "base fp16 n64 default plan": ("base", "fp16", 64, 64, 64, {}, lambda fl, tw: _count(fl, "f2") >= 40),
    "base fp16 n32 default plan": ("base", "fp16", 32, 64, 64, {}, lambda fl, tw: len(fl) == 79),
    "base fp16 n1 default plan": ("base", "fp16", 1, 64, 64, {}, lambda fl, tw: _count(fl, "f4", "f5") >= 70),
    "base fp32 n1": ("base", "fp32", 1, 64, 64, {}, lambda fl, tw: all(tag == "f0" for tag, _ in fl.values())),
    "decoder bf16 n2 256x256 fewcout": ("decoder", "bf16", 2, 256, 256, dict(fewcout=1), lambda fl, tw: fl["out_conv"][0] == "f6" and any(tw.by_label[l]["cout"] == 64 for l in _tail_on_wide(tw, fl))),
    "decoder bf16 n3 144x176 no fewcout": ("decoder", "bf16", 3, 144, 176, dict(fewcout=0), lambda fl, tw: fl["out_conv"][0] != "f6"),
    "tiny attention bf16 n3 32x32": ("tiny_attn", "bf16", 3, 32, 32, {}, lambda fl, tw: sum(l.endswith(".attn_proj") for l in fl) >= 3),
}


# arms whose flavour map must be the one a 64-window td_sample_edm_img call launches, lane by lane, on the shipped options
LANE_ARMS = ("base bf16 n32 default plan", "base fp16 n32 default plan")


def _labels_of(rows):
    """{op label: {(full profile label, launches)}} of the conv launches among Engine.profile_ops() rows"""
    out = {}
    for r in rows:
        if " [" in r[0]:
            out.setdefault(ct.flavour_of(r[0])[0], set()).add((r[0], r[2]))
    return out


def _two_lane_sampler_labels(eng, cfg, m, n=64, H=64, W=64, steps=3):
    """Profile rows of one td_sample_edm_img call of `n` windows on the shipped options.  Profile mode: the two lanes run one after the other on the plans they
    run concurrently without it; fuse_solver = 0: the output conv is the plain launch a forward makes (profile mode and fuse_solver are not part of a plan's key)."""
    from oracle import rng, schedule
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import ptr
    assert cfg["in_channels"] == cfg["out_channels"]
    assert eng.get_option("dual_stream", 1) == 1 and n >= eng.get_option("dual_stream_min_batch", 32)    # the call splits
    sig = schedule.karras_sigmas(steps)[0].contiguous()
    x = (torch.from_numpy(rng.standard_normal(17, (n, cfg["out_channels"], H, W))) * float(sig[0])).contiguous().cuda()
    conds = [torch.from_numpy(rng.standard_normal(18 + i, (n, c[1]))) for i, c in enumerate(cfg.get("conditional_inputs", []))]
    cond = m.cond_rows(conds, n, "cuda") if conds else None
    with pinned(eng, profile=1, fuse_solver=0):
        eng.profile_read(reset=True)
        check(lib().td_sample_edm_img(m._h, n, H, W, steps, ptr(sig), 0.5, ptr(cond), None, 0, ptr(x)))
        torch.cuda.synchronize()
        rows = eng.profile_ops()
    eng.profile_read(reset=True)
    assert torch.isfinite(x).all()
    return rows


@pytest.mark.parametrize("arm", list(ARMS))
def test_every_conv_op_elementwise_against_its_float64_twin(td, zoo, arm):
    from oracle import rng
    from terrain_diffusion_amd.engine import get_engine
    which, T, n, H, W, opts, intended = ARMS[arm]
    eng = get_engine("cuda")
    cfg, m, tw = zoo(which, T)
    x = torch.from_numpy(rng.standard_normal(7, (n, cfg["in_channels"], H, W)))
    cond = [torch.from_numpy(rng.standard_normal(8 + i, (n, c[1]))).cuda() for i, c in enumerate(cfg.get("conditional_inputs", []))]
    t = torch.full((n,), 1.1)
    t0 = time.time()
    with pinned(eng, **opts):
        with pinned(eng, profile=1):
            eng.profile_read(reset=True)
            y = m(x.cuda(), t, cond)
            torch.cuda.synchronize()
            rows = eng.profile_ops()
        eng.profile_read(reset=True)
        fl = {}
        for r in rows:
            if " [" in r[0]:
                lab, tag, ks = ct.flavour_of(r[0])
                fl[lab] = (tag, ks)
        SEEN[arm] = fl
        assert set(fl) == set(tw.by_label), set(fl) ^ set(tw.by_label)      # the twin describes exactly the ops the engine launched
        assert intended(fl, tw), f"{arm}: the intended flavours did not run: {sorted(set(v for v in fl.values()))}"
        stats, nss = ct.check_forward(m, tw, x, t, cond, T, fl)
        out = m.read_activation(n, H, W, "out_conv")                          # (under the arm's options: they are part of the plan's key)
        assert torch.equal(out[:, :cfg["out_channels"]], y.cpu())            # the output conv's stored tensor is what forward() returned
    if arm in LANE_ARMS:
        # the plan checked element-wise above is the plan the two-lane sampler launches: same flavour, tile and split-K for every op -- the whole profile label,
        # workgroup count included, which only an N = 32 launch gives -- and every op launched once per lane and step
        steps = 3
        lanes = _labels_of(_two_lane_sampler_labels(eng, cfg, m, n=2 * n, H=H, W=W, steps=steps))
        fl_s = {}
        for lab, seen in lanes.items():
            assert len(seen) == 1, f"{arm}: the two lanes launched {lab} on different plans: {sorted(seen)}"
            (full, launches), = seen
            assert launches == 2 * steps, f"{arm}: {full} ran {launches} times in a {steps}-step two-lane call"
            fl_s[lab] = ct.flavour_of(full)[1:]
        diff = {l: (fl.get(l), fl_s.get(l)) for l in set(fl) | set(fl_s) if fl.get(l) != fl_s.get(l)}
        assert not diff, f"{arm}: the N = {n} forward and the lanes of the {2 * n}-window sampler call chose different flavours (forward, sampler): {diff}"
        assert {r[0] for r in rows if " [" in r[0]} == {full for seen in lanes.values() for full, _ in seen}
        # ... and which ops the N = 32 plan carries otherwise than the N = 64 plan does, where that arm ran before this one
        for other in ("base bf16 n64 default plan", "base fp16 n64 default plan"):
            if other in SEEN and other.split()[1] == T:
                d = {l: (fl[l], SEEN[other][l]) for l in fl if fl[l] != SEEN[other][l]}
                print(f"\n{arm}: {len(d)} of {len(fl)} ops differ in (flavour, ksplit) from '{other}'" + (": " + ", ".join(f"{l} {a[0]}/ks{a[1]} vs {b[0]}/ks{b[1]}" for l, (a, b) in sorted(d.items())) if d else ""))
    tags = {}
    for tag, ks in fl.values():
        key = tag + (" ks>1" if ks > 1 else "")
        tags[key] = tags.get(key, 0) + 1
    print("\n" + ct.summary_line(arm, stats, nss, time.time() - t0) + "   flavours " + " ".join(f"{k}:{v}" for k, v in sorted(tags.items())))
    assert len(stats) == len(tw.ops) and nss == sum(o["sumsq"] for o in tw.ops)


def test_every_flavour_was_exercised_by_some_arm():
    """f2b, f2s, f2w, the small-batch tiles, f5, f6, the per-tap flavour and split-K launches each ran in at least one arm above (this test reads what the
    arms recorded: it belongs to a run of the whole file)"""
    assert len(SEEN) == len(ARMS), f"only {len(SEEN)} of {len(ARMS)} arms recorded their flavours: run the whole file"
    tags = {tag for fl in SEEN.values() for tag, _ in fl.values()}
    assert {"f2b", "f2s", "f2w", "f5c16", "f6", "f0"} <= tags and any(t.startswith("f4") for t in tags), tags
    assert any(ks > 1 for fl in SEEN.values() for _, ks in fl.values())
