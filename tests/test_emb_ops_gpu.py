"""The embedding and modulation kernels (emb_kernel; cvec_kernel / cvec_mfma_kernel<1> / cvec_mfma_kernel<4>; cvec_norm_kernel), element by element, against their
float64 twin (tests/_emb_twin.py): every row a forward or a sampler call computed ("@emb:rows" / "@cvec:rows"), on all three dispatch arms of compute_cvecs (the arm
is asserted from the config by restating its rule), every kind of conditional-input list, the (step, tile) layout with the diagonal copy of a forward with
differing t, both samplers and the three storage types.  Condition A on every element, condition B, the cap and the honesty condition per case.  Every model is
tiny_config(64, 1, ...) on a 16 x 16 map: the forward is only the vehicle.  One line per case."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _emb_twin as et
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

H = W = 16
C_TOTAL = 3392          # tiny_config(64, 1): the couts of its 20 blocks, 64 .. 256
LINES, STATS = [], []
CASES = {c[0]: c for c in et.gpu_cases()}
ARM_OF_EMB_CH = {None: "<4>", 768: "<4>", 80: "<1>", 16: "<1>", 100: "scalar", 37: "scalar"}


def dispatch(cfg):
    """engine.hip, compute_cvecs(): the matrix-core form needs emb_ch % 16 == 0, c_total % 4 == 0 and block couts in whole 16s; <4> needs emb_ch % 64 == 0"""
    from oracle.unet import build_plan
    plan = build_plan(cfg)
    couts = [b["cout"] for b in plan["enc"] + plan["dec"]]
    c_total = sum(b["cout"] for b in plan["enc"] + plan["dec"] if b["kind"] != "conv")
    e = plan["emb_channels"]
    c16 = e % 16 == 0 and c_total % 4 == 0 and all(c % 16 == 0 for c in couts)
    return "<4>" if c16 and e % 64 == 0 else ("<1>" if c16 else "scalar")


def _model(case, T="bf16"):
    import terrain_diffusion_amd as td
    return td.EDMUnet2D(**case["cfg"], dtype=T).load_state_dict(case["sd"])


def _call(m, case):
    """runs the case's forward / sampler call on a 16 x 16 map; returns (emb rows, cvec rows) as "@emb:rows" / "@cvec:rows" give them"""
    from oracle import rng
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import ptr
    from terrain_diffusion_amd.sampling import consistency_step
    n, kind = case["n"], case["kind"]
    x = torch.from_numpy(rng.standard_normal(7, (n, 5, H, W))).cuda()
    cond = [c.cuda() for c in case["cond"]]
    if kind in ("forward", "uniform"):
        m(x, case["t"] if kind == "forward" else case["t"].expand(n).contiguous(), cond)
    elif kind == "edm":
        x = (x * 80.0).contiguous()
        with pinned(m.engine, solver_order=2):
            check(lib().td_sample_edm(m._h, n, H, W, 5, ptr(case["sigmas"].contiguous()), float(case["sigma_data"]), ptr(m.cond_rows(cond, n, "cuda")), ptr(x)))
    else:
        consistency_step(m, float(case["t"][0]), 0.5, None, x, cond=m.cond_rows(cond, n, "cuda"))
    torch.cuda.synchronize()
    R = case["step"].numel()
    emb_ch = m.config["emb_channels"] or 64 * 4
    emb = m.read_activation(n, H, W, "@emb:rows", max_elems=R * emb_ch)
    cv = m.read_activation(n, H, W, "@cvec:rows", max_elems=R * C_TOTAL)
    assert emb.shape == (R, emb_ch, 1, 1) and cv.shape == (R, C_TOTAL, 1, 1), (tuple(emb.shape), tuple(cv.shape), R)
    return emb.reshape(R, -1), cv.reshape(R, -1)


@pytest.mark.parametrize("name", list(CASES))
def test_every_row_elementwise(name):
    t0 = time.time()
    nm, kind, n, kw = CASES[name]
    case = et.make_case(nm, kind, n, kw)
    want = ARM_OF_EMB_CH[kw.get("emb_channels")]
    assert dispatch(case["cfg"]) == want == et.arm_of(case["cfg"]), f"{name}: the config runs arm {dispatch(case['cfg'])}, the test meant {want}"
    m = _model(case)
    try:
        emb, cv = _call(m, case)
        # the old labels: the first n rows, unchanged
        assert torch.equal(m.read_activation(n, H, W, "@emb").reshape(n, -1), emb[:n]) and torch.equal(m.read_activation(n, H, W, "@cvec").reshape(n, -1), cv[:n])
    finally:
        m.close()
    st = et.check(case, emb, cv)
    st["wall"] = time.time() - t0
    STATS.append(st)
    LINES.append(et.line(st) + f"; {st['wall']:.1f} s")
    print(LINES[-1])


def test_storage_type_does_not_reach_the_embedding_path():
    """@emb:rows and @cvec:rows are bit-identical between the fp32, bf16 and fp16 models of the same weights: the path is fp32 whatever the storage type"""
    nm, kind, n, kw = CASES["forward n9 emb80 mixed8"]
    case = et.make_case(nm, kind, n, kw)
    got = {}
    for T in ("fp32", "bf16", "fp16"):
        m = _model(case, T)
        try:
            got[T] = _call(m, case)
        finally:
            m.close()
    for T in ("bf16", "fp16"):
        assert torch.equal(got[T][0], got["fp32"][0]) and torch.equal(got[T][1], got["fp32"][1]), T
    print(et.line(et.check(case, *got["fp32"])) + " (fp32 = bf16 = fp16, bit for bit)")


def test_nine_conditional_inputs_are_refused_at_construction():
    import terrain_diffusion_amd as td
    cfg = et.tiny_config(64, 1, conditional_inputs=[["float", 4, 0.1]] * 9)
    with pytest.raises(NotImplementedError, match="up to 8"):
        td.EDMUnet2D(**cfg, dtype="bf16")


def test_rows_are_refused_before_anything_was_computed():
    from terrain_diffusion_amd._lib import TdError
    nm, kind, n, kw = CASES["forward n1 emb256 tensor58"]
    case = et.make_case(nm, kind, n, kw)
    m = _model(case)
    try:
        with pytest.raises(TdError, match="no embedding rows"):
            m.read_activation(2, H, W, "@emb:rows", max_elems=1 << 16)
    finally:
        m.close()


def test_summary():
    """worst figures per dispatch arm (the lines DESIGN.md quotes)"""
    for arm in ("<4>", "<1>", "scalar"):
        ss = [s for s in STATS if s["arm"] == arm]
        if not ss:
            continue
        assert any(s["rows"] == 289 for s in ss), f"no 289-row case ran on arm {arm}"
        print(f"ARM {arm}: {len(ss)} cases, {sum(s['rows'] for s in ss)} rows; emb worst err / E {max(s['emb_worst'] for s in ss):.3f}, B {max(s['emb_rms'] for s in ss) / et.U:.2f} u; "
              f"cvec worst err / E {max(s['cvec_worst'] for s in ss):.3f}, B {max(s['cvec_rms'] for s in ss) / et.U:.2f} u; wall {min(s['wall'] for s in ss):.1f} .. {max(s['wall'] for s in ss):.1f} s")
