"""The validation objective without a GPU: the twin (tests/_objective_twin.py) against what the reference's own train_step, calc_loss and
_normalize_and_process_terrain recorded (tests/golden/objective.npz) -- within e_ref + 1 ulp, carried through the later operations by the
twin's rules; the uint8 images exactly --, eight wrong variants of the twin that must each fail on the same inputs, the refusals that happen
before an engine exists, the build table and the header against the binding."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _objective_twin as twin
from terrain_diffusion_amd import objective as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
within, ulp32 = twin.within, twin.ulp32


@pytest.fixture(scope="module")
def fx(golden):
    return golden("objective")


@pytest.fixture(scope="module")
def cases(fx):
    return json.loads(str(fx["cases"]))


def get(fx, case, key):
    k = f"{case['name']}_{key}"
    return fx[k] if k in fx.files else None


def twin_levels(fx, case, variant=None):
    return twin.levels64(get(fx, case, "d_z"), "draw", case["sigma_data"], case["P_mean"], case["P_std"], get(fx, case, "image"), case["channels"],
                         case["eps"], variant=variant)


def table_slack(fx, case):
    """(dc, ds): how far the twin's cos t and sin t may lie from the reference's, from the fixture alone"""
    return tuple(get(fx, case, "eref_" + k) + ulp32(get(fx, case, k)) for k in ("cos", "sin"))


def check_case(fx, case, variant=None):
    """what differs between the twin (or a wrong variant of it) and the reference's recorded step"""
    bad = []
    sd = case["sigma_data"]
    lv_ = twin_levels(fx, case, variant)
    refs = dict(sigma=get(fx, case, "ratio").astype(D) * float(F(sd)), t=get(fx, case, "t"), cos=get(fx, case, "cos"), sin=get(fx, case, "sin"))
    if case["scale"]:
        refs["std"] = get(fx, case, "std")
    for k, r in refs.items():
        if not within(lv_["table"][:, twin.LEVEL_COLS.index(k)], r, get(fx, case, "eref_" + k) + ulp32(r)):
            bad.append(k)
    image, noise, cond = get(fx, case, "image"), get(fx, case, "d_noise"), get(fx, case, "cond_img")
    x, v = twin.add_noise32(image, noise, lv_["table"], sd, cond, variant=variant)
    dc, ds = table_slack(fx, case)
    bx, bv = twin.noise_carry(dc, ds, image, noise, sd)
    xr = get(fx, case, "x")
    if x.shape != xr.shape or not within(x[:, :case["C"]], xr[:, :case["C"]], bx):
        bad.append("x")
    if cond is not None and not twin.same_bits(x[:, case["C"]:], xr[:, case["C"]:]):
        bad.append("x cond channels")
    if not within(v, get(fx, case, "v_t"), bv):
        bad.append("v")
    lvr = get(fx, case, "logvar")
    lv, _ = twin.logvar64(lv_["table"][:, 4], get(fx, case, "lv_freqs"), get(fx, case, "lv_phases"), get(fx, case, "lv_wfold"))
    dlv = get(fx, case, "eref_logvar") + ulp32(lvr)
    if not within(lv, lvr, dlv):
        bad.append("logvar")
    out = get(fx, case, "model_output")                       # the recorded model_output: the U-Net is not in the way
    S = twin.sqerr64(out, v, sd)
    HW = case["H"] * case["W"]
    _, loss = twin.loss64(S, HW, sd, lv, "weighted", variant=variant)
    dS = twin.sq_carry(out, v, bv, sd)
    lr = get(fx, case, "loss")
    tol = get(fx, case, "eref_loss") + ulp32(lr) + twin.loss_carry(S, dS, HW, sd, lv, dlv, "weighted")
    if not within(loss, lr, tol):
        bad.append("loss")
    return bad, dict(tol=float(tol[0]), loss=float(lr[0]), eref=float(get(fx, case, "eref_loss")[0]))


def check_curve(fx, cases, variant=None):
    c0 = cases[0]
    S = twin.sqerr64(get(fx, c0, "model_output"), get(fx, c0, "v_t"), c0["sigma_data"])
    bad = []
    for key, form, groups in (("plain", "plain", None), ("g14", "grouped", [1, 4]), ("g23", "grouped", [2, 3])):
        _, loss = twin.loss64(S, c0["H"] * c0["W"], c0["sigma_data"], None, form, groups, variant=variant)
        r = fx["curve_" + key]
        if not within(loss, r, fx["curve_" + key + "_eref"] + ulp32(r)):
            bad.append(key)
    return bad


# ------------------------------------------------------------------------------------------------------------------------------ the fixture
def test_the_fixture_holds_the_cases_the_issue_names(fx, cases):
    assert {(c["Cc"], c["scale"]) for c in cases} == {(2, False), (0, True), (2, True), (0, False)}
    assert {c["sigma_data"] for c in cases} == {0.5, 1.0} and {c["K"] for c in cases} == {128, 130}
    for c in cases:
        assert (c["N"], c["C"], c["H"], c["W"]) == (3, 5, 16, 16)
        assert get(fx, c, "lv_freqs").shape == (c["K"],) and get(fx, c, "lv_weight").shape == (1, c["K"])
        assert get(fx, c, "x").shape == (3, 5 + c["Cc"], 16, 16) and get(fx, c, "logvar").shape == (3,)
        for k in ("sigma", "t", "cos", "sin", "logvar", "loss") + (("std",) if c["scale"] else ()):
            assert get(fx, c, "eref_" + k).dtype == D and get(fx, c, "f64_" + k).dtype == D
            assert float(np.max(get(fx, c, "eref_" + k) / ulp32(get(fx, c, "f64_" + k)))) <= (4096.0 if k == "logvar" else 64.0), (c["name"], k)
        if c["scale"]:
            r = get(fx, c, "f64_std") / c["sigma_data"]
            assert (r < c["eps"]).any() and (r > c["eps"]).any()          # the floor holds for one item and not for another
        assert len(c["state_names"]) == get(fx, c, "state_den").size == get(fx, c, "state_crc").size
    assert set(json.loads(str(fx["versions"]))) == {"torch", "numpy", "python"}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "objective.npz")) < 1 << 20
    _, pre = twin.terrain_u8(fx["terrain"])
    assert not (np.abs(pre - np.rint(pre)) <= 2.0 * ulp32(np.maximum(np.abs(pre), np.abs(np.rint(pre))))).any()


def test_the_folded_logvar_weight_is_the_hosts_fold(fx, cases):
    import _conv_twin as ct
    from terrain_diffusion_amd.unet import EDMUnet2D
    for c in cases:
        w = torch.from_numpy(get(fx, c, "lv_weight"))
        assert twin.same_bits(ct.fold_host(w, 1).numpy(), get(fx, c, "lv_wfold")), c["name"]
        assert twin.same_bits(EDMUnet2D._fold_reference(w, 1).numpy(), get(fx, c, "lv_wfold")), c["name"]


# ------------------------------------------------------------------------------------------------------------------------------ twin vs reference
def test_twin_reproduces_the_recorded_train_steps(fx, cases):
    for c in cases:
        bad, st = check_case(fx, c)
        print(f"{c['name']}: loss {st['loss']:.7g}, e_ref {st['eref']:.2e}, tolerance {st['tol']:.2e}")
        assert not bad, (c["name"], bad)
        assert st["tol"] <= 2e-3 * abs(st["loss"]) + 1e-4, (c["name"], st)          # the carried tolerance stays far below what a wrong formula moves


def test_twin_reproduces_the_recorded_curve_losses(fx, cases):
    assert not check_curve(fx, cases)
    assert abs(float(fx["curve_g14"][0]) - float(fx["curve_plain"][0])) > 1e-3     # the grouped and the plain form part on these inputs


def test_twin_terrain_bytes_equal_the_recorded_ones(fx):
    got, _ = twin.terrain_u8(fx["terrain"])
    assert got.dtype == np.uint8 and np.array_equal(got, fx["terrain_u8"])
    assert (fx["terrain_u8"][2] == 127).all()                                       # the all-equal plane: range floored at 255, every value 127.5


WRONG = {"cos_sin_swapped": ("x", "v"), "noise_unscaled": ("x", "v"), "v_sign": ("v",), "biased_std": ("std",), "mean_nhw": ("loss",),
         "logvar_not_added": ("loss",)}


@pytest.mark.parametrize("variant", twin.VARIANTS)
def test_each_wrong_variant_of_the_twin_fails(fx, cases, variant):
    if variant == "group_weighted":
        assert set(check_curve(fx, cases, variant)) == {"g14", "g23"}
        return
    if variant == "range_not_floored":
        got, _ = twin.terrain_u8(fx["terrain"], variant=variant)
        assert all(not np.array_equal(got[n], fx["terrain_u8"][n]) for n in range(got.shape[0]))
        return
    hit = [c for c in cases if (variant != "noise_unscaled" or c["sigma_data"] != 1.0) and (variant != "biased_std" or c["scale"])]
    assert hit
    for c in hit:
        bad, _ = check_case(fx, c, variant)
        assert set(WRONG[variant]) <= set(bad), (variant, c["name"], bad)


# ------------------------------------------------------------------------------------------------------------------------------ refusals before an engine
def test_refusals_that_need_no_engine():
    z = torch.zeros(3)
    with pytest.raises(ValueError, match="device tensor"):
        ob.noise_levels(z, sigma_data=0.5)
    with pytest.raises(ValueError, match="mode must be"):
        ob.noise_levels(z, mode="x", sigma_data=0.5)
    with pytest.raises(ValueError, match="device tensor"):
        ob.add_noise(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2), torch.zeros(1, 6), sigma_data=0.5)
    with pytest.raises(NotImplementedError, match="n_logvar"):
        ob.logvar(torch.zeros(1, 6), z, z, z, n_logvar=2)
    with pytest.raises(ValueError, match="device tensor"):
        ob.squared_error(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2), sigma_data=0.5)
    with pytest.raises(ValueError, match="form must be"):
        ob.v_loss(torch.zeros(1, 1), 2, 2, sigma_data=0.5, form="x")
    with pytest.raises(ValueError, match="device tensor"):
        ob.terrain_uint8(torch.zeros(1, 1, 2, 2))
    with pytest.raises(ValueError, match="no batches"):
        ob.noise_loss_curve(None, [], [1.0], sigma_data=0.5)


def test_the_model_call_accepts_return_logvar():
    from terrain_diffusion_amd.unet import EDMUnet2D
    p = inspect.signature(EDMUnet2D.__call__).parameters
    assert list(p)[:4] == ["self", "x", "noise_labels", "conditional_inputs"] and p["return_logvar"].default is False
    assert EDMUnet2D.forward is EDMUnet2D.__call__ and callable(EDMUnet2D.logvar) and callable(EDMUnet2D.logvar_operands)


def test_the_twins_constants_are_the_embedding_twins():
    import _emb_twin as et
    assert (twin.TRIG_ULP, twin.CAP, twin.U) == (et.TRIG_ULP, et.CAP, et.U)


# ------------------------------------------------------------------------------------------------------------------------------ the header
def test_header_entry_points_exports_and_the_build_tables():
    import terrain_diffusion_amd as td
    import __graft_entry__ as ge
    text = open(os.path.join(ROOT, "include", "td_objective.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = set(re.findall(r"\b(td_objective_\w+)\s*\(", code))
    stated = {"td_objective_last_error", "td_objective_levels", "td_objective_noise", "td_objective_logvar", "td_objective_sqerr", "td_objective_loss",
              "td_objective_terrain_u8"}
    assert declared == set(ob.EXPORTS) == stated
    for name in stated - {"td_objective_last_error"}:
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")
        assert len(params) == len(ob._SIGS[name][1]), name
        assert params[0].strip() == "void* hip_stream" and params[-1].strip() == "int synchronize", name
        for p, ctype in zip(params, ob._SIGS[name][1]):
            assert ("*" in p) == (ctype is ob._P), (name, p)
            assert (p.strip().startswith("float ")) == (ctype is ob._F), (name, p)
    for macro, value in (("LEVEL_COLS", 6), ("MAX_ITEMS", 65536), ("MAX_CHANNELS", 1024), ("MAX_SIDE", 65536), ("MAX_LOGVAR", 1024), ("MAX_LIST", 64)):
        assert re.search(rf"#define TD_OBJECTIVE_{macro} {value}\b", text) and getattr(ob, macro) == value
    for name, value in ob.MODES.items():
        assert re.search(rf"#define TD_OBJECTIVE_MODE_{name.upper()} {value}\b", text)
    for name, value in ob.FORMS.items():
        assert re.search(rf"#define TD_OBJECTIVE_LOSS_{name.upper()} {value}\b", text)
    have = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", ob.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert stated <= have and not {n for n in have if n.startswith("td_") and n not in stated}
    ob.lib()     # binds every entry point
    for name in ("noise_levels", "add_noise", "logvar", "squared_error", "v_loss", "terrain_uint8", "validation_loss", "noise_loss_curve"):
        assert getattr(td, name) is getattr(ob, name), name
    assert callable(ob.logvar)
    assert ge.OBJECTIVE_LIBS == (("objective", "objective_csrc", "objective.hip", "td_objective.h", ("-ffp-contract=off",), "objective"),)
    assert [r[0] for r in ge.SIDE_LIBS] == ["relief", "hydro", "mc", "explorer", "custom", "rivers", "dataset"]
    assert ge.DATA_LIBS == (("coarse", "coarse_csrc", "coarse.hip", "td_coarse.h", ("-ffp-contract=off",), "coarse_dataset"),)
    assert ge.SPECTRUM_LIBS == (("spectrum", "spectrum_csrc", "spectrum.hip", "td_spectrum.h", ("-ffp-contract=off",), "beauty"),)
    assert ge.ALL_SIDE_LIBS == ge.SIDE_LIBS + ge.DATA_LIBS + ge.SPECTRUM_LIBS and len(ge.ALL_SIDE_LIBS) == 9
    assert ge.BATCH_LIBS == (("batch", "batch_csrc", "batch.hip", "td_batch.h", ("-ffp-contract=off",), "train_data"),)
    assert "objective" not in {r[0] for r in ge.ALL_SIDE_LIBS + ge.BATCH_LIBS}
    deps = ge.side_deps("objective", "objective_csrc", "td_objective.h")
    assert {os.path.basename(d) for d in deps} == {"objective.hip", "objective_kernels.hip", "td_objective.h", "td_side_host.h"}
