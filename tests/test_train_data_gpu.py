"""libtd_batch.so on the GPU (include/td_batch.h, batch_csrc/batch_kernels.hip) against the NumPy twin (tests/_train_data_twin.py) and the
fixture (tests/golden/train_data.npz: the reference's own three dataset classes on the committed tree): every entry point on N = 33 items
over groups of three sides in one call -- exact where the twin is exact, the block means bit-equal to the twin's tree and within 1 ulp of
the correctly rounded float64 mean --, the seeded __getitem__ sequences item by item against what the reference recorded, by the CPU file's
criteria, get_batch against the twin fed its plan, the same bits from a second run and from the enqueue-only mode, and the C-ABI's refusals."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import _train_data_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
same_bits, equal_nan, within = twin.same_bits, twin.equal_nan, twin.within
F = np.float32
N = 33
PATHS = ("90/c0/s0", "90/c1/s0", "90/c1/s1", "90/c0/s1")            # sides 112, 130, 66, 112
KEYS = [("c0", 90, "s0"), ("c1", 90, "s0"), ("c1", 90, "s1"), ("c0", 90, "s1")]
NORM_MEAN = [13.36, 10.03, 16.17, 612.99, 869.73, 71.64, 0.674]
NORM_STD = [22.22, 22.13, 10.23, 453.81, 797.71, 34.23, 0.460]


@pytest.fixture(scope="module")
def td_():
    from terrain_diffusion_amd import train_data
    assert torch.cuda.is_available()
    return train_data


@pytest.fixture(scope="module")
def fx(golden):
    return golden("train_data")


@pytest.fixture(scope="module")
def cases(fx):
    return json.loads(str(fx["cases"]))


@pytest.fixture(scope="module")
def groups(td_):
    return td_.DeviceGroups(twin.TREE(), KEYS, ("latent", "lowfreq", "lowres_exact", "climate", "residual"))


@pytest.fixture(scope="module")
def batch():
    """33 items at crop 64 over the four groups, every transform, windows against every side; the draws the calls need"""
    rng = np.random.default_rng(5)
    rows = []
    for n in range(N):
        g = n % 4
        S = twin.TREE()[PATHS[g]]["lowfreq"].shape[0]
        i, j = (int(rng.integers(0, S - 64 + 1)) for _ in range(2))
        if n < 8:
            i, j = ((0, 0), (S - 64, S - 64), (0, S - 64), (S - 64, 0))[n % 4]
        t = n % 8
        rows.append([g, i, j, t, *twin.inverse_offsets(i, j, 64, 64, t, S)])
    gen = torch.Generator().manual_seed(11)
    d = {"items": np.array(rows, np.int32), "noise": torch.randn((N, 4, 64, 64), generator=gen), "noise16": torch.randn((N, 4, 8, 8), generator=gen).half(),
         "u_drop": torch.rand((N, 4, 4), generator=gen), "u_noise": torch.rand(N, generator=gen), "z_mean": torch.randn((N, 4, 4), generator=gen),
         "z_p5": torch.randn((N, 4, 4), generator=gen), "hist": torch.randn((N, 5), generator=gen), "z_replace": torch.randn((N, 4), generator=gen)}
    return d


def arrays(path):
    return {k: v.array for k, v in twin.TREE()[path].items()}


def build(cases, name, **extra):
    from terrain_diffusion_amd import train_data as t
    cfg = cases["configs"][name]
    cls = {"latents": t.H5LatentsDataset, "decoder": t.H5DecoderTerrainDataset, "autoencoder": t.H5AutoencoderDataset}[cfg["cls"]]
    return cls(**dict(cfg["args"], h5_file=twin.TREE(), **extra))


# ------------------------------------------------------------------------------------------------------------------------------ entry points
def test_views_equal_the_twin_bit_for_bit(td_, groups, batch):
    it = batch["items"]
    calls = {
        "lowfreq": (dict(plane="lowfreq", size=64, affine=(twin.LOWFREQ_MEAN, twin.LOWFREQ_STD, 0.5)), lambda a, r: twin.views(a["lowfreq"], r[4], r[5], 64, 64, r[3], (twin.LOWFREQ_MEAN, twin.LOWFREQ_STD, 0.5))),
        "padded": (dict(plane="lowfreq", size=66, offset=-1), lambda a, r: twin.views(a["lowfreq"], r[4] - 1, r[5] - 1, 66, 66, r[3])),
        "own": (dict(plane="residual", size=40, origin="own", affine=(0.05, 1.17, 1.0)), lambda a, r: twin.views(a["residual"], r[1], r[2], 40, 40, r[3], (0.05, 1.17, 1.0))),
        "overhang": (dict(plane="lowres_exact", size=128, offset=-32), lambda a, r: twin.views(a["lowres_exact"], r[4] - 32, r[5] - 32, 128, 128, r[3])),
    }
    for name, (kw, ref) in calls.items():
        got = td_.views(groups, it, **kw)
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (N, kw["size"], kw["size"])
        g = got.cpu().numpy()
        for n, r in enumerate(it):
            assert equal_nan(g[n], ref(arrays(PATHS[r[0]]), [int(v) for v in r])), (name, n)
        for extra in ({}, {"enqueue_only": True}):
            again = td_.views(groups, it, **kw, **extra)
            torch.cuda.synchronize()
            assert same_bits(again.cpu().numpy(), g), (name, extra)
    assert np.isnan(td_.views(groups, it, "lowres_exact", 128, offset=-32).cpu().numpy()).any()


def test_latent_draws_equal_the_twin_bit_for_bit(td_, groups, batch):
    it = batch["items"]
    mean, std = [0.1, -0.2, 0.05, 0.0], [1.1, 0.9, 1.3, 0.7]
    got0 = td_.sample_latents(groups, it, batch["noise"], mode=0, mean=mean, std=std, sigma_data=0.5)
    it8 = it.copy()
    it8[:, 1:3] = np.minimum(it8[:, 1:3], 50)                # an 8 x 8 latent window inside every group
    got1 = td_.sample_latents(groups, it8, batch["noise16"], mode=1)
    assert got0.dtype == torch.float32 and tuple(got0.shape) == (N, 4, 64, 64) and got1.dtype == torch.float16 and tuple(got1.shape) == (N, 4, 64, 64)
    g0, g1 = got0.cpu().numpy(), got1.cpu().numpy()
    for n in range(N):
        lat = arrays(PATHS[it[n, 0]])["latent"]
        assert same_bits(g0[n], twin.latents(lat, int(it[n, 3]), int(it[n, 1]), int(it[n, 2]), 64, 64, batch["noise"][n].numpy(), 0, mean, std, 0.5)), n
        assert same_bits(g1[n], twin.latents(lat, int(it8[n, 3]), int(it8[n, 1]), int(it8[n, 2]), 8, 8, batch["noise16"][n].numpy(), 1)), n
    for extra in ({}, {"enqueue_only": True}):
        a0 = td_.sample_latents(groups, it, batch["noise"], mode=0, mean=mean, std=std, sigma_data=0.5, **extra)
        a1 = td_.sample_latents(groups, it8, batch["noise16"], mode=1, **extra)
        torch.cuda.synchronize()
        assert same_bits(a0.cpu().numpy(), g0) and same_bits(a1.cpu().numpy(), g1), extra


def exact_means(v):
    b = twin.blocks_of(v.astype(np.float64))
    out = np.full(b.shape[:-1], np.nan)
    for idx in np.ndindex(*out.shape):
        if not np.isnan(b[idx]).any():
            out[idx] = math.fsum(b[idx]) / 1024.0
    return out


def test_cond_image_and_vector_equal_the_twin(td_, groups, batch):
    it = batch["items"]
    kw = dict(u_drop=batch["u_drop"], dropout=0.2, u_noise=batch["u_noise"], max_noise=0.1, z_mean=batch["z_mean"], z_p5=batch["z_p5"])
    raw = td_.cond_image(groups, it, 64)
    img = td_.cond_image(groups, it, 64, mean=NORM_MEAN, std=NORM_STD, **kw)
    plain = td_.cond_image(groups, it, 64, mean=NORM_MEAN, std=NORM_STD)
    vec, flags = td_.cond_vector(img, batch["hist"], batch["u_noise"], batch["z_replace"])
    vec0, flags0 = td_.cond_vector(img, batch["hist"], batch["u_noise"])
    assert tuple(raw.shape) == tuple(img.shape) == (N, 7, 4, 4) and tuple(vec.shape) == (N, 58) and flags.dtype == torch.int32 and tuple(flags.shape) == (N, 4)
    r, g, pl, v, fl, v0 = (x.cpu().numpy() for x in (raw, img, plain, vec, flags, vec0))
    finite, worst = 0, 0.0
    for n in range(N):
        a = arrays(PATHS[it[n, 0]])
        li, lj, t = int(it[n, 4]), int(it[n, 5]), int(it[n, 3])
        tk = {k: (x[n].numpy() if k not in ("dropout", "max_noise") else x) for k, x in kw.items()}
        tk["dropout_p"] = tk.pop("dropout")
        want_raw = twin.cond_image(a["lowres_exact"], a["climate"], li, lj, 64, t, raw=True)
        assert equal_nan(r[n], want_raw), n                                                     # the means through the same tree: the same bits
        lo = twin.view(twin.window(a["lowres_exact"], li - 32, lj - 32, 128, 128), t)
        cl = twin.view(twin.window(a["climate"][list(twin.CLIMATE_CHANNELS)], li - 32, lj - 32, 128, 128), t)
        m64 = np.concatenate([exact_means(lo)[None], exact_means(cl)])
        got_means = r[n][[0, 2, 3, 4, 5]]
        assert np.array_equal(np.isnan(got_means), np.isnan(m64)), n
        ok = ~np.isnan(m64)
        worst = max(worst, float(np.max(np.abs(got_means[ok].astype(np.float64) - m64[ok]) / twin.ulp(m64[ok].astype(F))))) if ok.any() else worst
        finite += int(np.isfinite(r[n][1]).sum())
        assert equal_nan(g[n], twin.cond_image(a["lowres_exact"], a["climate"], li, lj, 64, t, norm_mean=NORM_MEAN, norm_std=NORM_STD, **tk)), n
        assert equal_nan(pl[n], twin.cond_image(a["lowres_exact"], a["climate"], li, lj, 64, t, norm_mean=NORM_MEAN, norm_std=NORM_STD)), n
        wv, wf = twin.cond_vector(g[n], batch["hist"][n].numpy(), batch["u_noise"][n].numpy(), batch["z_replace"][n].numpy())
        assert equal_nan(v[n], wv) and np.array_equal(fl[n], wf), n
        assert equal_nan(v0[n], twin.cond_vector(g[n], batch["hist"][n].numpy(), batch["u_noise"][n].numpy())[0]), n
    print(f"\nblock means: worst |gpu - float64 mean| = {worst:.3f} ulp; {finite} finite p5 values compared; NaN centres in {int(fl.any(1).sum())} of {N} items")
    assert worst <= 1.0 and finite >= 60 and 0 < int(fl.any(1).sum()) < N
    assert np.array_equal(flags0.cpu().numpy(), fl)
    for extra in ({}, {"enqueue_only": True}):
        a = td_.cond_image(groups, it, 64, mean=NORM_MEAN, std=NORM_STD, **kw, **extra)
        b, _ = td_.cond_vector(a, batch["hist"], batch["u_noise"], batch["z_replace"], **extra)
        torch.cuda.synchronize()
        assert same_bits(a.cpu().numpy(), g) and same_bits(b.cpu().numpy(), v), extra


# ------------------------------------------------------------------------------------------------------------------------------ the recorded items
def test_getitem_sequences_equal_the_recorded_ones_item_by_item(td_, fx, cases):
    recorded = json.loads(str(fx["versions"]))["torch"].split("+")[0]
    if torch.__version__.split("+")[0] != recorded:
        pytest.skip(f"the sequences were recorded with torch {recorded}; torch {torch.__version__} is installed and its generator's stream is not pinned across versions")
    by_name = {e["name"]: e for e in cases["items"]}
    smallest = set()
    for run, spec in cases["runs"].items():
        cfg = cases["configs"][spec["config"]]
        ds = build(cases, spec["config"])
        ds.set_seed(spec["seed"])
        for k, name in enumerate(spec["items"]):
            e, out = by_name[name], ds[k]
            host = {key: (v.cpu().numpy() if torch.is_tensor(v) else v) for key, v in out.items()}
            label = host["cond_inputs"][-1] if e.get("label") is not None else None
            assert (None if label is None else int(label)) == e["label"], name
            if cfg["cls"] == "latents":
                assert host["path"] == e["path"] and twin.crc(host["image"]) == e["image_crc"] and host["image"].dtype == F, name
                args = cfg["args"]
                dr = {key: fx[f"{name}_d_{key}"] for _, _, key, _ in e["draws"] if key is not None}
                tw = twin.latents_item(args, e["path"], e["i"], e["j"], e["t"], dr, e_mean=fx[name + "_eref"], with_latent=False)
                img, vec = host["cond_inputs_img"], host["cond_inputs"][0].cpu().numpy()
                assert equal_nan(img, tw["cond_img"]) and equal_nan(vec, tw["cond_vector"]), name       # the twin's bits
                want_img, want_vec = fx[name + "_cond_inputs_img"], fx[name + "_cond_inputs"]
                exact = np.r_[16:32, 36:58]
                assert equal_nan(img[[1, 6]], want_img[[1, 6]]) and within(img, want_img, tw["d_img"]), name
                assert equal_nan(vec[exact], want_vec[exact]) and within(vec, want_vec, tw["d_vector"]), name
                assert same_bits(host["histogram_raw"], fx[name + "_histogram_raw"]), name
                assert same_bits(host["noise_level"].reshape(1), fx[name + "_noise_level"]) and host["noise_level"].shape == ((1,) if args.get("cond_input_max_noise") else ()), name
                smallest.add((twin.TREE()[e["path"]]["lowfreq"].shape[0], args["crop_size"], bool(args["clip_edges"])))
            elif cfg["cls"] == "decoder":
                assert host["path"] == e["path"] and host["cond_img"].dtype == np.float16, name
                for key in ("image", "cond_img", "lowfreq", "lowfreq_padded"):
                    assert same_bits(host[key], fx[f"{name}_{key}"]), (name, key)
                smallest.add(("decoder", cfg["args"]["crop_size"]))
            else:
                assert same_bits(host["image"], fx[name + "_image"]), name
    assert (66, 64, True) in smallest and ("decoder", 64) in smallest


def test_get_batch_equals_the_twin_fed_its_plan(td_, cases):
    ds = build(cases, "LA")
    ds.set_seed(2024)
    b = ds.get_batch(N)
    assert tuple(b["image"].shape) == (N, 5, 64, 64) and tuple(b["cond_inputs"][0].shape) == (N, 58) and len(b["path"]) == N
    args = cases["configs"]["LA"]["args"]
    image, vec, img = b["image"].cpu().numpy(), b["cond_inputs"][0].cpu().numpy(), b["cond_inputs_img"].cpu().numpy()
    for n, p in enumerate(b["plan"]):
        dr = {k: v.numpy() for k, v in p.items() if torch.is_tensor(v)}
        tw = twin.latents_item(args, p["path"], p["i"], p["j"], p["t"], dr)
        assert same_bits(image[n, :4], tw["latent"]) and equal_nan(image[n, 4], tw["lowfreq"]), n
        assert equal_nan(img[n], tw["cond_img"]) and equal_nan(vec[n], tw["cond_vector"]), n
    assert len({p["path"] for p in b["plan"]}) >= 3 and len({p["t"] for p in b["plan"]}) == 8
    dec = build(cases, "DA")
    dec.set_seed(9)
    d = dec.get_batch(N)
    for n, p in enumerate(d["plan"]):
        tw = twin.decoder_item(cases["configs"]["DA"]["args"], p["path"], p["i"], p["j"], p["t"], p["noise"].numpy())
        for key in ("image", "cond_img", "lowfreq", "lowfreq_padded"):
            assert same_bits(d[key][n].cpu().numpy(), tw[key]), (n, key)
    ae = build(cases, "AB")
    ae.set_seed(9)
    a = ae.get_batch(N)
    for n, p in enumerate(a["plan"]):
        assert same_bits(a["image"][n].cpu().numpy(), twin.autoencoder_item(cases["configs"]["AB"]["args"], p["path"], p["i"], p["j"], p["t"])), n
    assert a["cond_inputs"][0].tolist() == [4] * N


def test_cond_input_stats_follow_the_reference_expressions(td_, cases):
    ds = build(cases, "LB", cond_input_mean=None, cond_input_std=None)
    assert len(ds.cond_input_mean) == len(ds.cond_input_std) == 7 and np.isfinite(ds.cond_input_mean).all() and (np.asarray(ds.cond_input_std) > 0).all()
    assert 0.0 < ds.cond_input_mean[6] < 1.0                 # the mask's mean is the share of blocks without NaN


# ------------------------------------------------------------------------------------------------------------------------------ the C ABI
def test_the_c_abi_refuses_bad_arguments(td_, groups):
    eng, dev = groups.resolve()
    l, st = td_.lib(), C.c_void_p(eng.stream)
    tab, items = groups.table(), torch.zeros((1, 6), dtype=torch.int32, device=dev)
    out = torch.empty(7 * 16 + 64, dtype=torch.float32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    host = np.zeros(64, F)
    bad = [
        l.td_batch_views(st, P(tab), 4, P(items), 1, 3, 0, 0, 8, 8, 0, 0.0, 1.0, 1.0, P(out), 1),            # plane 3
        l.td_batch_views(st, P(tab), 4, P(items), 1, 0, 0, 0, 0, 8, 0, 0.0, 1.0, 1.0, P(out), 1),            # h = 0
        l.td_batch_views(st, P(tab), 4, P(items), 0, 0, 0, 0, 8, 8, 0, 0.0, 1.0, 1.0, P(out), 1),            # N = 0
        l.td_batch_views(st, P(tab), 4, P(items), 1, 0, 0, 0, 8, 8, 0, 0.0, 1.0, 1.0, host.ctypes.data_as(C.c_void_p), 1),      # a host buffer
        l.td_batch_cond_image(st, P(tab), 4, P(items), 1, 80, 0.0, None, 0.0, None, None, None, None, None, 1, P(out), 1),      # crop 80
        l.td_batch_cond_image(st, P(tab), 4, P(items), 1, 64, 0.0, None, 0.0, None, None, None, None, None, 0, P(out), 1),      # no statistics
        l.td_batch_latents(st, P(tab), 4, P(items), 1, 4, 8, 8, 2, P(out), None, None, 0.5, P(out), 1),                           # mode 2
        l.td_batch_cond_vector(st, P(out), 1, 3, P(out), P(out), None, 3.4641016, 1, 1, 1, 1, 1, 1, P(out), P(items), 1),         # g = 3
    ]
    assert all(rc == -1 for rc in bad), bad
    assert b"td_batch_cond_vector" in l.td_batch_last_error()
    # an item whose group or transform is out of range reads nothing: NaN views, a zero latent draw
    wild = torch.tensor([[9, 0, 0, 0, 0, 0], [0, 0, 0, 8, 0, 0], [-1, 0, 0, 0, 0, 0]], dtype=torch.int32)
    assert torch.isnan(td_.views(groups, wild, "lowfreq", 8)).all()
    assert (td_.sample_latents(groups, wild, torch.ones(3, 4, 8, 8), mode=0, mean=[0.0] * 4, std=[1.0] * 4) == 0).all()
