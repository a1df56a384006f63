"""The conv kernel / tile / split-K selector (csrc/conv_select.h) on the CPU: tests/conv_select_harness.cpp, a host program, replays every decision the
plan builder made before the selector existed (tests/golden/conv_select.npz, recorded on an MI355X by tests/golden/make_conv_select_golden.py)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _engine_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("PerTap", "Glds", "GldsWide", "GldsWide16", "Sb", "S16", "FewCout")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on PATH")
    exe = str(tmp_path_factory.mktemp("csel") / "conv_select")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "terrain_diffusion_amd", "csrc"), os.path.join(ROOT, "tests", "conv_select_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "conv_select.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def rows(golden):
    """the recorded decisions as one dict of columns (inputs, options and results by name, `tag`)"""
    c = {}
    for names, arr in (("input_names", "inputs"), ("option_names", "options"), ("result_names", "results")):
        for i, n in enumerate(golden[names]):
            c[str(n)] = golden[arr][:, i].astype(np.int64)
    c["tag"] = golden["tags"][golden["tag_index"]]
    c["kernel_name"] = np.array(KERNELS)[c["kernel"]]
    return c


def test_every_recorded_decision_replays_exactly(harness, golden):
    fin, fopt, fout = (l.split() for l in subprocess.check_output([harness, "--fields"]).decode().splitlines())
    assert fin == list(golden["input_names"]) and fopt == list(golden["option_names"]) and fout == list(golden["result_names"])
    cases = np.concatenate([golden["inputs"], golden["options"]], axis=1)
    text = "\n".join(" ".join(str(v) for v in r) for r in cases.tolist()) + "\n"
    out = subprocess.run([harness], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases) > 1000
    want_tags = golden["tags"][golden["tag_index"]]
    bad = []
    for i, (line, want, tag) in enumerate(zip(out, golden["results"].tolist(), want_tags)):
        f = line.split(" ", len(fout))
        if [int(v) for v in f[:len(fout)]] != want or f[len(fout)] != str(tag):
            bad.append(f"row {i}: inputs {dict(zip(fin, golden['inputs'][i].tolist()))} options off default "
                       f"{ {n: int(v) for n, v, d in zip(fopt, golden['options'][i], golden['options'][0]) if v != d} }: got {line!r}, recorded {want} {tag!r}")
    assert not bad, f"{len(bad)} of {len(out)} decisions differ:\n" + "\n".join(bad[:10])


def test_golden_covers_the_decision_space(rows):
    r = rows
    k = r["kernel_name"]

    def some(mask, what):
        assert bool(mask.any()), f"no recorded row with {what}"
    for bn in (64, 96, 128):
        some((k == "PerTap") & (r["bn"] == bn), f"PerTap bn {bn}")
    some((k == "PerTap") & (r["ksplit"] > 1), "PerTap split-K")
    for v in (0, 1, 2):
        some((k == "Glds") & (r["glds_variant"] == v), f"Glds variant {v}")
    some((k == "Glds") & (r["ksplit"] > 1), "Glds split-K")
    for d in (0, 1):
        some((k == "Glds") & (r["dma1x1"] == d), f"Glds dma1x1 {d}")
    tail = ((r["s0_taps"] == 1) & (r["nseg"] >= 1)) | ((r["s1_taps"] == 1) & (r["nseg"] >= 2)) | ((r["s2_taps"] == 1) & (r["nseg"] >= 3))
    for bn in (64, 96):
        some((k == "GldsWide") & (r["bn"] == bn), f"GldsWide bn {bn}")
    some((k == "GldsWide") & tail, "GldsWide with a 1x1 tail")
    some((k == "GldsWide") & (r["persist"] > 0), "GldsWide persistent")
    assert bool((np.char.startswith(r["tag"][r["persist"] > 0], "f2wp")).all())
    some(k == "GldsWide16", "GldsWide16")
    assert bool((np.char.endswith(r["tag"][k == "GldsWide16"], " x16")).all()) and not bool(np.char.endswith(r["tag"][k != "GldsWide16"], " x16").any())
    for mt, nt in ((1, 1), (2, 1), (2, 2), (4, 1)):
        some((k == "Sb") & (r["sb_mt"] == mt) & (r["sb_nt"] == nt), f"Sb tile ({mt}, {nt})")
    some((k == "Sb") & (r["ksplit"] > 1), "Sb split-K")
    for o in (0, 1):
        some((k == "Sb") & (r["sb_order"] == o), f"Sb order {o}")
    some(k == "S16", "S16")
    some(k == "FewCout", "FewCout")
    some(r["narrow"] == 1, "narrow tiles")
    inv = r["batch_invariant"] != 0
    some(inv, "batch_invariant = 1")
    assert not bool((inv & (np.isin(k, ("Sb", "S16", "GldsWide", "GldsWide16")) | (r["ksplit"] > 1))).any())
    assert sorted(set(k)) == sorted(KERNELS)
    for dt in (0, 1, 2):
        some(r["dt"] == dt, f"dtype {dt}")


def test_option_list_is_the_plan_builder_section_of_the_known_options(harness):
    fopt = subprocess.check_output([harness, "--fields"]).decode().splitlines()[1].split()
    with open(_engine_opts.ENGINE_HIP) as f:
        raw = f.read()
    m = re.search(r"kKnownOptions\s*\[\s*\]\s*=\s*\{(.*?)\}\s*;", raw, flags=re.S)   # the table _engine_opts.parse_shipped reads; here with its section comments
    section = m.group(1).split("// plan builder", 1)[1]
    plan = re.findall(r'"([^"]+)"', _engine_opts._strip_comments(section.split("\n", 1)[1]))
    assert fopt == ["batch_invariant"] + plan
    assert set(fopt) <= set(_engine_opts.SHIPPED)
    # each is read exactly once in engine.hip (read_plan_options), with a literal default
    src = _engine_opts._strip_comments(raw)
    for name in fopt:
        assert len(re.findall(r'\boption\(\s*"%s"\s*,' % re.escape(name), src)) == 1, name
