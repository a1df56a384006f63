"""The model graph (csrc/model_graph.h) on the CPU: tests/model_graph_harness.cpp, a host program, prints the parameter list and the fused-op list of a
config; both must equal, in order and field for field, what the engine stated in three places before the graph existed (tests/golden/model_graph.npz,
recorded from that commit's own library on an MI355X by tests/golden/make_model_graph_golden.py).  No tolerance anywhere: floats are bit patterns."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS_A = ("kind", "chunk", "image_size", "in_channels", "out_channels", "model_channels", "n_levels")
ARRAYS_A = ("channel_mults", "layers_per_block", "layers_per_block_decoder")
SCALARS_B = ("midblock_attention", "concat_balance_bits", "noise_emb_dims", "emb_channels", "n_cond")
TD_ERR_ARG, TD_ERR_UNSUPPORTED = -1, -4


def harness_input(c):
    """the harness's stdin for a config dict (keys: SCALARS_A, ARRAYS_A, n_attn_resolutions, attn_resolutions, SCALARS_B, cond_type, cond_dims; lists may be short)"""
    def arr(k):
        v = list(c.get(k, []))
        return v + [0] * (8 - len(v))
    vals = [c[k] for k in SCALARS_A] + sum((arr(k) for k in ARRAYS_A), []) + [c["n_attn_resolutions"]] + arr("attn_resolutions") + [c[k] for k in SCALARS_B] \
        + arr("cond_type") + arr("cond_dims")
    return " ".join(str(int(v)) for v in vals) + "\n"


def level_dim(v, level):
    """a map side at `level` halvings (negative: doublings) of the input's, with build_plan's arithmetic"""
    for _ in range(max(level, 0)):
        v = (v + 1) // 2
    return v << max(-level, 0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on PATH")
    exe = str(tmp_path_factory.mktemp("mgraph") / "model_graph")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "terrain_diffusion_amd", "csrc"), os.path.join(ROOT, "tests", "model_graph_harness.cpp"), "-o", exe])
    return lambda cfg: subprocess.run([exe], input=harness_input(cfg).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()


def load_golden():
    """{model name: dict(config, shape, lines)} (the layout: make_model_graph_golden.save)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "model_graph.npz"))
    lines, off = [str(l) for l in g["lines"]], g["offsets"].tolist()
    return {str(n): dict(config=json.loads(str(c)), shape=s.tolist(), lines=lines[off[i]:off[i + 1]]) for i, (n, c, s) in enumerate(zip(g["names"], g["configs"], g["shapes"]))}


GOLDEN = load_golden()


def test_golden_holds_every_model_the_graph_is_checked_on():
    want = {f"{m}_{dt}" for dt in ("fp32", "bf16") for m in ("coarse", "base", "decoder", "tiny", "tiny_attn", "ae_tiny_enc", "ae_tiny_dec", "ae_released_enc", "ae_released_dec")}
    assert set(GOLDEN) == want
    for name, g in GOLDEN.items():
        assert g["config"]["chunk"] == (32 if name.endswith("fp32") else 64)
    # attention in encoder and decoder blocks, with and without a channel change (decoder: the mid block keeps its channels, every concat block changes them)
    lines = GOLDEN["tiny_attn_fp32"]["lines"]
    params = {l.split()[1] for l in lines if l.startswith("param ")}
    attn = [l.split()[1][:-len(".attn")] for l in lines if l.startswith("attn ")]
    for side in ("enc.", "dec."):
        assert {(b + ".conv_skip.weight") in params for b in attn if b.startswith(side)} == {True, False}


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_parameters_and_ops_are_the_recorded_ones(harness, name):
    g = GOLDEN[name]
    _, H, W = g["shape"]
    got = []
    for line in harness(g["config"]):
        f = line.split(" ")
        assert f[0] != "error", line
        if f[0] in ("conv", "attn"):   # the golden has the map the op ran on; the graph has its level
            f[2:3] = [str(level_dim(H, int(f[2]))), str(level_dim(W, int(f[2])))]
        if f[0] in ("param", "conv", "seg", "attn"):
            got.append(" ".join(f))
    want = g["lines"]
    n_ops = sum(l.startswith(("conv ", "attn ")) for l in want)
    assert n_ops > 3 and sum(l.startswith("param ") for l in want) > 3
    bad = [f"line {i}: got {a!r}, recorded {b!r}" for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad and len(got) == len(want), f"{len(bad)} of {len(want)} lines differ ({len(got)} printed):\n" + "\n".join(bad[:10])


def test_tensors_are_written_before_they_are_read(harness):
    for name, g in GOLDEN.items():
        lines = [l.split(" ") for l in harness(g["config"])]
        n_tensors = sum(f[0] == "tensor" for f in lines)
        written = {0}
        for i, f in enumerate(lines):
            if f[0] == "conv":
                nseg, res, out = int(f[13]), int(f[6]), int(f[12])
                reads = [int(s[9]) for s in lines[i + 1:i + 1 + nseg]] + ([res] if res >= 0 else [])
            elif f[0] == "attn":
                reads, out = [int(f[4])], int(f[5])
            else:
                continue
            assert all(r in written for r in reads), (name, f)
            assert out == len(written) < n_tensors + 1 and out not in written, (name, f)
            written.add(out)
        assert len(written) == n_tensors


BAD = [
    (0, dict(n_levels=0), TD_ERR_ARG, "n_levels out of range"),
    (0, dict(n_levels=9), TD_ERR_ARG, "n_levels out of range"),
    (0, dict(n_cond=9), TD_ERR_ARG, "n_cond out of range"),
    (0, dict(cond_type=[2]), TD_ERR_UNSUPPORTED, "conditional input type (embedding tables are not on the accelerated path)"),
    (0, dict(model_channels=96), TD_ERR_UNSUPPORTED, "block channels must be multiples of 64: enc.512x512_block0"),
    (0, dict(in_channels=32), TD_ERR_UNSUPPORTED, "in_channels+1 must fit one K chunk (<=32)"),
    (0, dict(out_channels=9), TD_ERR_UNSUPPORTED, "out_channels must be <= 8"),
    (1, dict(n_levels=0), TD_ERR_ARG, "n_levels out of range"),
    (1, dict(model_channels=96), TD_ERR_UNSUPPORTED, "block channels must be multiples of 64: encoder.enc.16x16_block0"),
    (2, dict(n_levels=9), TD_ERR_ARG, "n_levels out of range"),
    (2, dict(model_channels=96), TD_ERR_UNSUPPORTED, "block channels must be multiples of 64: decoder.5"),   # (decoder.0 .. 4 run on 2 x 96 channels)
]


@pytest.mark.parametrize("kind,change,code,text", BAD, ids=[f"kind{k}-{'-'.join(f'{a}={b}' for a, b in c.items())}".replace(" ", "") for k, c, _, _ in BAD])
def test_a_config_the_engine_refused_is_refused_with_the_same_code_and_text(harness, kind, change, code, text):
    """the checks of the former build_blocks / build_blocks_ae (csrc/engine.hip), in their order: texts and codes are those of that source"""
    cfg = dict(GOLDEN[("tiny_fp32", "ae_tiny_enc_fp32", "ae_tiny_dec_fp32")[kind]]["config"])
    assert cfg["kind"] == kind
    cfg.update(change)
    assert harness(cfg) == [f"error {code} {text}"]
