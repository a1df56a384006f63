"""Training items without a GPU: the NumPy twin (tests/_train_data_twin.py) against what the reference's own three dataset classes recorded
(tests/golden/train_data.npz) -- bit for bit for the views, both latent modes, p5, the mask, histogram_raw and noise_level, and within
e_ref + 1 ulp, carried through the later operations by the twin's rule, for every value that descends from a block mean --, six wrong variants
of the twin that must each fail on the same inputs, the host planners against the recorded draws, the key lists, the refusals, which happen
before an engine exists, and the header against the binding."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _train_data_twin as twin
from terrain_diffusion_amd import train_data as td_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CLASSES = {"latents": td_.H5LatentsDataset, "decoder": td_.H5DecoderTerrainDataset, "autoencoder": td_.H5AutoencoderDataset}


@pytest.fixture(scope="module")
def fx(golden):
    return golden("train_data")


@pytest.fixture(scope="module")
def cases(fx):
    return json.loads(str(fx["cases"]))


def draws_of(fx, item):
    return {key: fx[f"{item['name']}_d_{key}"] for _, _, key, _ in item["draws"] if key is not None}


same_bits, equal_nan, within = twin.same_bits, twin.equal_nan, twin.within


def latents_twin(fx, cases, item, variant=None):
    args = cases["configs"][item["config"]]["args"]
    dr = draws_of(fx, item)
    return twin.latents_item(args, item["path"], item["i"], item["j"], item["t"], dr, e_mean=fx[item["name"] + "_eref"], variant=variant,
                             with_latent="noise" in dr)


# ------------------------------------------------------------------------------------------------------------------------------ the fixture
def test_the_committed_inputs_are_the_recorded_ones(cases):
    assert twin.tree_crc() == cases["tree_crc"]
    its = cases["items"]
    for cls in ("latents", "decoder", "autoencoder"):
        assert {e["t"] for e in its if e["cls"] == cls and e["forced"]} == set(range(8)), cls
    run = [e for e in its if e["name"].startswith("runLA_")]
    assert len(run) >= 12 and {bool(e["nan_centres"]) for e in run} == {True, False}
    assert {twin.TREE()[e["path"]]["lowfreq"].shape[0] for e in its if e["cls"] == "latents"} == set(twin.SIDES)


# ------------------------------------------------------------------------------------------------------------------------------ twin vs reference
def test_views_equal_the_reference_bit_for_bit(fx, cases):
    seen = 0
    for e in cases["items"]:
        args = cases["configs"][e["config"]]["args"]
        if e["cls"] == "latents":
            key = "_image" if e["full"] else "_lowfreq" if e["forced"] else None
            if key is None:
                continue
            want = fx[e["name"] + key]
            got = latents_twin(fx, cases, e)["lowfreq"]
            assert same_bits(got, want[-1] if e["full"] else want), e["name"]
        elif e["cls"] == "decoder":
            got = twin.decoder_item(args, e["path"], e["i"], e["j"], e["t"], fx[e["name"] + "_d_noise"])
            for key in ("image", "lowfreq", "lowfreq_padded"):
                assert same_bits(got[key], fx[f"{e['name']}_{key}"]), (e["name"], key)
        else:
            assert same_bits(twin.autoencoder_item(args, e["path"], e["i"], e["j"], e["t"]), fx[e["name"] + "_image"]), e["name"]
        seen += 1
    assert seen >= 40


def test_latent_draws_equal_the_reference_bit_for_bit(fx, cases):
    full = [e for e in cases["items"] if e["cls"] == "latents" and e["full"]]
    assert len(full) >= 2
    for e in full:
        assert same_bits(latents_twin(fx, cases, e)["latent"], fx[e["name"] + "_image"][:-1]), e["name"]
    dec = [e for e in cases["items"] if e["cls"] == "decoder"]
    assert len(dec) >= 12
    for e in dec:
        args = cases["configs"][e["config"]]["args"]
        got = twin.decoder_item(args, e["path"], e["i"], e["j"], e["t"], fx[e["name"] + "_d_noise"])["cond_img"]
        assert got.dtype == np.float16 and same_bits(got, fx[e["name"] + "_cond_img"]), e["name"]
    for path in cases["tree_crc"]:
        assert twin.exp_midpoint_distance(twin.TREE()[path]["latent"].array[:, twin.LC:]) > 2.0 ** -20


def check_cond(fx, cases, e, variant=None):
    """the list of what differs between the twin (or a wrong variant of it) and the recorded item"""
    got = latents_twin(fx, cases, e, variant)
    img, vec = fx[e["name"] + "_cond_inputs_img"], fx[e["name"] + "_cond_inputs"]
    bad = []
    for ch in (1, 6):                                                       # p5 and the mask: bit for bit
        if not equal_nan(got["cond_img"][ch], img[ch]):
            bad.append(f"cond_img[{ch}]")
    if not within(got["cond_img"], img, got["d_img"]):
        bad.append("cond_img")
    exact = np.r_[16:32, 36:58]                                             # p5, mask, histogram, noise level
    if not equal_nan(got["cond_vector"][exact], vec[exact]):
        bad.append("cond_vector exact parts")
    if not within(got["cond_vector"], vec, got["d_vector"]):
        bad.append("cond_vector")
    if int(got["flags"].sum()) != e["nan_centres"]:
        bad.append("nan centres")
    return bad


def test_cond_image_and_vector_against_the_reference(fx, cases):
    lat = [e for e in cases["items"] if e["cls"] == "latents"]
    assert len(lat) >= 30
    finite = 0
    for e in lat:
        assert check_cond(fx, cases, e) == [], e["name"]
        dr = draws_of(fx, e)
        assert same_bits(fx[e["name"] + "_histogram_raw"], dr["histogram_raw"])
        assert same_bits(fx[e["name"] + "_noise_level"], dr["u_noise"] if "u_noise" in dr else np.zeros(1, F))
        # the reference's own raw statistics of the window: p5 and the mask exactly, the means within e_ref + 1 ulp of the twin's
        g = twin.TREE()[e["path"]]
        crop = cases["configs"][e["config"]]["args"]["crop_size"]
        li, lj = twin.inverse_offsets(e["i"], e["j"], crop, crop, e["t"], g["lowfreq"].shape[0])
        raw, d = twin.cond_image(g["lowres_exact"].array, g["climate"].array, li, lj, crop, e["t"], raw=True, e_mean=fx[e["name"] + "_eref"])
        want = fx[e["name"] + "_raw"]
        assert equal_nan(raw[1], want[1]) and equal_nan(raw[6], want[6]) and within(raw, want, d), e["name"]
        # the twin's mean is the correctly rounded float64 mean
        m64 = fx[e["name"] + "_m64"]
        assert equal_nan(raw[[0, 2, 3, 4, 5]], m64.astype(F)), e["name"]
        finite += int(np.isfinite(raw[1]).sum())
    assert finite >= 100                                                    # p5 was compared on real values, not on NaN alone


@pytest.mark.parametrize("variant", twin.VARIANTS)
def test_a_wrong_variant_of_the_twin_fails_on_the_committed_inputs(fx, cases, variant):
    assert len(twin.VARIANTS) >= 6
    lat = [e for e in cases["items"] if e["cls"] == "latents"]
    failing = [e["name"] for e in lat if check_cond(fx, cases, e, variant)]
    print(f"\n{variant}: {len(failing)} of {len(lat)} items fail")
    assert failing, variant


# ------------------------------------------------------------------------------------------------------------------------------ planners, keys
def build(cases, name, **extra):
    cfg = cases["configs"][name]
    return CLASSES[cfg["cls"]](**dict(cfg["args"], h5_file=twin.TREE(), **extra))


def test_key_lists_and_buckets_equal_the_recorded_ones(cases):
    for name, want in cases["keys"].items():
        ds = build(cases, name)
        assert json.loads(json.dumps(ds.keys)) == want, name
        assert len(ds) == (100000 if cases["configs"][name]["cls"] == "latents" else max(len(k) for k in want))
    assert td_.beauty_class(2.5000001) == 2 and td_.beauty_class(2.5) == 1


def test_planners_reproduce_the_recorded_draws(fx, cases):
    recorded = json.loads(str(fx["versions"]))["torch"]
    if torch.__version__ != recorded:
        pytest.skip(f"the draws were recorded with torch {recorded}; torch {torch.__version__} is installed and its generator's stream is not pinned across versions")
    by_name = {e["name"]: e for e in cases["items"]}
    for run, spec in cases["runs"].items():
        ds = build(cases, spec["config"])
        ds.set_seed(spec["seed"])
        for name in spec["items"]:
            e = by_name[name]
            p = ds.plan_item()
            if e["cls"] == "latents":
                p["z_replace"] = ds.draw_replacements(e["nan_centres"])
            assert (p["path"], p["i"], p["j"], p["t"], p["subset"]) == (e["path"], e["i"], e["j"], e["t"], e["subset"]), name
            for fn, shape, key, crc in e["draws"]:
                if key in ("histogram_raw", "noise", "u_drop", "u_noise", "z_mean", "z_p5", "z_replace"):
                    got = p[key].numpy()
                    assert list(got.shape) == shape and twin.crc(got) == crc, (name, key)
                    assert got.dtype == (np.float16 if (e["cls"], key) == ("decoder", "noise") else np.float32)


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_happen_before_any_engine_is_touched(cases, monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(td_, "_engine_for", no_engine)
    with pytest.raises(NotImplementedError, match="val_dset"):
        build(cases, "LA", val_dset=True)
    with pytest.raises(NotImplementedError, match="signed_sqrt"):
        build(cases, "AA", signed_sqrt=False)
    with pytest.raises(NotImplementedError, match="residual_mean"):
        build(cases, "DA", residual_mean=None)
    with pytest.raises(NotImplementedError, match="clip_edges"):
        build(cases, "DA", clip_edges=False)
    for crop in (32, 48, 80, 0):
        with pytest.raises(ValueError, match="multiple of 32"):
            build(cases, "LA", crop_size=crop)
    with pytest.raises(ValueError, match="side 66 is below 98"):
        build(cases, "LA", crop_size=96)
    with pytest.raises(ValueError, match="divisible by 8"):
        build(cases, "DA", crop_size=12)
    tree = twin.TREE()
    g = tree["90/c0/s0"]
    odd = twin.Node({"90": twin.Node({"c0": twin.Node({"s0": twin.Node(dict(g, lowfreq=twin.Dataset(g["lowfreq"].array[:, :100], **g["lowfreq"].attrs)))})})})
    odd["90/c0/s0"].attrs.update(g.attrs)
    with pytest.raises(ValueError, match="square"):
        td_.H5LatentsDataset(**dict(cases["configs"]["LA"]["args"], h5_file=odd))
    f32 = twin.Node({"90": twin.Node({"c0": twin.Node({"s0": twin.Node(dict(g, latent=twin.Dataset(g["latent"].array.astype(F), **g["latent"].attrs)))})})})
    f32["90/c0/s0"].attrs.update(g.attrs)
    with pytest.raises(ValueError, match="float16"):
        td_.H5LatentsDataset(**dict(cases["configs"]["LA"]["args"], h5_file=f32))
    ds = build(cases, "LA")                                  # constructing, seeding and planning need no engine
    ds.set_seed(3)
    assert set(ds.plan_item()) >= {"path", "i", "j", "t", "li", "lj", "noise", "u_drop", "u_noise", "z_mean", "z_p5", "histogram_raw"}
    with pytest.raises(ValueError, match="plane must be"):
        td_.views(ds.groups, np.zeros((1, 6)), "climate", 8)
    with pytest.raises(ValueError, match="multiple of 32"):
        td_.cond_image(ds.groups, np.zeros((1, 6)), 80)
    with pytest.raises(ValueError, match="device tensor"):
        td_.cond_vector(torch.zeros(1, 7, 4, 4), torch.zeros(1, 5), torch.zeros(1))
    assert ds.denormalize_lowfreq(torch.tensor(1.0)).item() == pytest.approx(38.6 - 31.4)


# ------------------------------------------------------------------------------------------------------------------------------ the header
def test_header_entry_points_exports_and_the_build_table():
    import terrain_diffusion_amd as td
    import __graft_entry__ as ge
    text = open(os.path.join(ROOT, "include", "td_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = set(re.findall(r"\b(td_batch_\w+)\s*\(", code))
    stated = {"td_batch_last_error", "td_batch_views", "td_batch_latents", "td_batch_cond_image", "td_batch_cond_vector"}
    assert declared == set(td_.EXPORTS) == stated
    for name in stated - {"td_batch_last_error"}:
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code).group(1).split(",")
        assert len(params) == len(td_._SIGS[name][1]), name
        assert params[0].strip() == "void* hip_stream" and params[-1].strip() == "int synchronize", name
        for p, ctype in zip(params, td_._SIGS[name][1]):
            assert ("*" in p) == (ctype is td_._P), (name, p)
            assert (p.strip().startswith("float ")) == (ctype is td_._F), (name, p)
    for macro, value in (("ITEM_FIELDS", 6), ("MAX_ITEMS", 65536), ("MAX_CROP", 4096), ("HALO", 32), ("COND_CHANNELS", 7), ("COND_LEN", 58)):
        assert re.search(rf"#define TD_BATCH_{macro} {value}\b", text) and getattr(td_, macro) == value
    for name, value in td_.PLANES.items():
        assert re.search(rf"#define TD_BATCH_PLANE_{name.upper()} {value}\b", text)
    have = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", td_.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert stated <= have and not {n for n in have if n.startswith("td_") and n not in stated}
    td_.lib()     # binds every entry point
    for name in ("DeviceGroups", "views", "sample_latents", "cond_image", "cond_vector", "H5LatentsDataset", "H5DecoderTerrainDataset",
                 "H5AutoencoderDataset"):
        assert getattr(td, name) is getattr(td_, name), name
    assert ge.BATCH_LIBS == (("batch", "batch_csrc", "batch.hip", "td_batch.h", ("-ffp-contract=off",), "train_data"),)
    assert len(ge.ALL_SIDE_LIBS) == 9 and "batch" not in {r[0] for r in ge.ALL_SIDE_LIBS}
    assert [float(F(f)) for f in td_.mp_concat_factors()] == [float(f) for f in twin.mp_factors()]
