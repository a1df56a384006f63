"""NumPy restatement of libtd_batch.so (include/td_batch.h, batch_csrc/batch_kernels.hip) in the kernels' own arithmetic, the committed inputs
of tests/golden/train_data.npz, and the rule that carries a block mean's error through the operations that follow it.

The inputs: TREE() builds an in-memory mapping shaped like the reference's HDF5 file, res / chunk / subchunk / {latent, lowfreq, lowres_exact,
climate, residual} with .attrs, from seeded NumPy draws; the fixture records their CRC-32.  Groups have sides 66, 112 and 130; lowres_exact and
climate carry NaN rectangles that cross block edges and the 2 x 2 centre of the cond image.

The twin, written from the header's definitions:
  view            flip(dims=[-1]) if t // 4 == 1, then rot90(k = t % 4)
  window          a window of a plane with NaN outside it
  latents         e = fp16(exp(fp16(0.5 v))) with the float64 exponential rounded to fp32 and then to half; mode 0 in fp32, mode 1 in half
  block_sums      the kernels' float64 tree: a thread adds its four values, 64 lanes combine by xor-shuffles 32 .. 1, four waves pairwise
  cond_image      means, the all-fp32 `linear` 0.05 quantile over the exact order statistics 51 and 52, mask, dropout, noise, nan_to_num, the
                  normalisation; `variant` names a deliberately WRONG restatement (VARIANTS), each of which the CPU test must see fail
  cond_vector     build_cond_inputs with mp_concat's factors as fp32 computes them

The bound (the second result of cond_image and the third of cond_vector): the twin's block mean is the correctly rounded float64 mean M up to
the float64 sum's own error (below 2^-43 of sum|x| / 1024: nothing in fp32), the reference's fp32 mean is within its recorded e_ref of M, so
the two differ by at most d0 = e_ref + ulp(M).
Every later operation f is the same rounded fp32 operation on both sides, and |fl(f(a)) - fl(f(b))| <= L |a - b| + ulp(result) for an f that
is L-Lipschitz, rounding being monotone: an addition of the same term keeps d and adds one ulp of the sum, a division by s divides d by |s|
and adds one ulp of the quotient, a product with a factor multiplies d.  Values that are NaN on both sides, or replaced by the same constant,
carry d = 0.  Nothing in the bound is measured.
"""
import zlib

import numpy as np

F = np.float32
H = np.float16
HALO = 32
RANK = 51
CLIMATE_CHANNELS = (0, 3, 11, 14)
LOWFREQ_MEAN, LOWFREQ_STD = -31.4, 38.6
SIDES = (66, 112, 130)
LC = 4
SEED = 20240607
VARIANTS = ("rot_sense", "rot_before_flip", "halo31", "f64_index", "climate13", "dropout_ge")


# ------------------------------------------------------------------------------------------------------------------------------ the inputs
class Dataset:
    """an array with .attrs, .shape and h5py's slicing (a list on the first axis and slices on the rest included)"""

    def __init__(self, array, **attrs):
        self.array, self.attrs = array, dict(attrs)

    shape = property(lambda self: self.array.shape)
    dtype = property(lambda self: self.array.dtype)

    def __getitem__(self, idx):
        return self.array[idx]

    def __array__(self, dtype=None, copy=None):
        return self.array if dtype is None else self.array.astype(dtype)


class Node(dict):
    """a group: a dict with .attrs whose [] also walks 'a/b/c' paths"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.attrs = {}

    def __getitem__(self, key):
        node = self
        for part in str(key).split("/"):
            node = dict.__getitem__(node, part)
        return node

    def __contains__(self, key):
        try:
            self[key]
            return True
        except KeyError:
            return False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# (res, chunk, subchunk, side, pct_land, split, beauty_score): three sides, both splits, every beauty class but one, a pct_land below 0.01
GROUPS = (
    ("90", "c0", "s0", 112, 0.80, "train", 3.2),
    ("90", "c0", "s1", 112, 0.55, "train", 2.4),
    ("90", "c1", "s0", 130, 0.95, "train", 4.6),
    ("90", "c1", "s1", 66, 0.30, "train", 1.2),
    ("90", "c2", "s0", 112, 0.005, "train", 1.0),
    ("90", "c2", "s1", 130, 0.70, "val", 3.6),
    ("90", "c3", "s0", 66, 0.65, "train", 2.5000001),
    ("30", "c0", "s0", 112, 0.90, "train", 5.4),
)
# NaN rectangles (r0, r1, c0, c1) by side: across block edges (multiples of 32 once the halo is added), over the centre, along a border
NAN_RECTS = {66: ((30, 37, 28, 40),), 112: ((20, 45, 60, 70), (52, 60, 50, 58), (100, 112, 0, 9)), 130: ((60, 70, 62, 66), (0, 3, 90, 130))}
# climate: (r0, r1, c0, c1, channels or None for all): some crops keep a NaN-free centre, and the four centre means differ in which are NaN
CLIMATE_RECTS = {66: ((31, 35, 31, 35, (0, 3)),), 112: ((0, 20, 80, 112, None), (90, 112, 0, 30, (0, 11)), (30, 34, 100, 112, (3,))),
                 130: ((64, 66, 64, 66, (14,)), (100, 130, 0, 40, None))}


def group_arrays(index):
    """the five arrays of GROUPS[index]"""
    S = GROUPS[index][3]
    rng = np.random.default_rng(SEED + index)
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    base = 40.0 * np.sin(yy / 17.0 + index) * np.cos(xx / 23.0) + 12.0 * rng.standard_normal((S, S))
    lowfreq = (base - 20.0).astype(F)
    lowres = (base + 3.0 * rng.standard_normal((S, S)) - 18.0).astype(F)
    lowres[rng.random((S, S)) < 0.02] = F(0.0)                                          # exact zeros of both signs among both signs
    lowres[rng.random((S, S)) < 0.01] = F(-0.0)
    climate = (rng.standard_normal((15, S, S)) * np.array([10, 1, 1, 400, 1, 1, 1, 1, 1, 1, 1, 800, 1, 50, 30.0])[:, None, None]
               + np.arange(15)[:, None, None] * 7.0).astype(F)
    for r0, r1, c0, c1 in NAN_RECTS[S]:
        lowres[r0:r1, c0:c1] = np.nan
    for r0, r1, c0, c1, chans in CLIMATE_RECTS[S]:
        climate[slice(None) if chans is None else list(chans), r0:r1, c0:c1] = np.nan
    latent = np.concatenate([rng.standard_normal((8, LC, S, S)), -2.0 + 1.5 * rng.standard_normal((8, LC, S, S))], axis=1).astype(H)
    logvar = latent[:, LC:]
    for _ in range(16):         # no exp(fp16(0.5 v)) within 2^-19 relative of a rounding midpoint of half: a rounding of the exponential decides nothing
        close = exp_midpoint_rel(logvar) <= 2.0 ** -19
        if not close.any():
            break
        logvar[close] = np.nextafter(logvar[close], H(np.inf))
    residual = (1.5 * rng.standard_normal((8 * S, 8 * S))).astype(F)
    return {"latent": latent, "lowfreq": lowfreq, "lowres_exact": lowres, "climate": climate, "residual": residual}


_TREE = []


def TREE():
    """the committed tree (built once)"""
    if not _TREE:
        root = Node()
        for index, (res, chunk, sub, S, pct, split, beauty) in enumerate(GROUPS):
            g = Node({k: Dataset(v, pct_land=pct, split=split) for k, v in group_arrays(index).items()})
            g.attrs["beauty_score"] = beauty
            dict.setdefault(root, res, Node())
            dict.setdefault(dict.__getitem__(root, res), chunk, Node())
            root[res][chunk][sub] = g
        _TREE.append(root)
    return _TREE[0]


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def tree_crc():
    t = TREE()
    return {f"{res}/{chunk}/{sub}": crc(*(t[f"{res}/{chunk}/{sub}"][k].array for k in ("latent", "lowfreq", "lowres_exact", "climate", "residual")))
            for res, chunk, sub, *_ in GROUPS}


# ------------------------------------------------------------------------------------------------------------------------------ views
def view(a, t, variant=None):
    """the dihedral view of the last two axes"""
    flip, k = t // 4 == 1, t % 4
    if variant == "rot_sense":
        k = -k
    if variant == "rot_before_flip":
        a = np.rot90(a, k, axes=(-2, -1))
        return np.flip(a, -1) if flip else a
    if flip:
        a = np.flip(a, -1)
    return np.rot90(a, k, axes=(-2, -1))


def inverse_offsets(i, j, h, w, t, side):
    """(li, lj): h5_latents_dataset.py:299-303"""
    li, lj = i, j
    for _ in range(t % 4):
        li, lj = lj, side - li - h
    if t // 4 == 1:
        lj = side - lj - w
    return li, lj


def window(plane, r0, c0, h, w):
    """plane[..., r0 : r0 + h, c0 : c0 + w] with NaN outside the plane"""
    S0, S1 = plane.shape[-2:]
    out = np.full(plane.shape[:-2] + (h, w), np.nan, F)
    a0, a1, b0, b1 = max(0, r0), min(S0, r0 + h), max(0, c0), min(S1, c0 + w)
    if a1 > a0 and b1 > b0:
        out[..., a0 - r0:a1 - r0, b0 - c0:b1 - c0] = plane[..., a0:a1, b0:b1]
    return out


def affine(x, a, b, c):
    return ((x - F(a)) / F(b)) * F(c)


def views(plane, r0, c0, h, w, t, abc=None):
    """td_batch_views for one item: the view of the (h, w) -- (w, h) for an odd rotation -- window at (r0, c0)"""
    hh, ww = (w, h) if t % 2 else (h, w)
    v = np.ascontiguousarray(view(window(plane, r0, c0, hh, ww), t))
    return affine(v, *abc) if abc is not None else v


# ------------------------------------------------------------------------------------------------------------------------------ latents
def half_std(logvar):
    hv = (logvar.astype(F) * F(0.5)).astype(H)
    return np.exp(hv.astype(np.float64)).astype(F).astype(H)


def latents(latent, t, i, j, h, w, noise, mode, mean=None, std=None, sigma_data=0.5):
    lc = latent.shape[1] // 2
    m, lv = latent[t, :lc, i:i + h, j:j + w], latent[t, lc:, i:i + h, j:j + w]
    e = half_std(lv)
    if mode == 0:
        x = noise.astype(F) * e.astype(F) + m.astype(F)
        return ((x - np.asarray(mean, F).reshape(-1, 1, 1)) / np.asarray(std, F).reshape(-1, 1, 1)) * F(sigma_data)
    p = (noise.astype(F) * e.astype(F)).astype(H)
    s = (p.astype(F) + m.astype(F)).astype(H)
    return np.repeat(np.repeat(s, 8, axis=-2), 8, axis=-1)


def exp_midpoint_distance(logvar):
    """the least relative distance of exp(fp16(0.5 v)) in float64 from a rounding midpoint of half"""
    return float(np.min(exp_midpoint_rel(logvar)))


def exp_midpoint_rel(logvar):
    """per element: the relative distance of exp(fp16(0.5 v)) in float64 from the nearest rounding midpoint of half"""
    hv = (logvar.astype(F) * F(0.5)).astype(H).astype(np.float64)
    x = np.exp(hv)
    h = x.astype(F).astype(H)
    lo, hi = np.nextafter(h, H(-np.inf)).astype(np.float64), np.nextafter(h, H(np.inf)).astype(np.float64)
    hd = h.astype(np.float64)
    return np.minimum(np.abs(x - (hd + lo) / 2), np.abs(x - (hd + hi) / 2)) / x


# ------------------------------------------------------------------------------------------------------------------------------ cond image
def blocks_of(v):
    """(..., V, V) -> (..., g, g, 1024): the 32 x 32 blocks, row-major inside a block"""
    g = v.shape[-1] // HALO
    lead = v.shape[:-2]
    return v.reshape(*lead, g, HALO, g, HALO).swapaxes(-3, -2).reshape(*lead, g, g, HALO * HALO)


def block_sums(b):
    """the kernels' float64 sum of (..., 1024): thread tid holds the values tid, tid + 256, ...; lanes by xor-shuffles; waves pairwise"""
    x = b.astype(np.float64).reshape(*b.shape[:-1], 4, 256)
    acc = np.zeros(x.shape[:-2] + (256,))
    with np.errstate(invalid="ignore"):
        for e in range(4):
            acc = acc + x[..., e, :]
        v = acc.reshape(*acc.shape[:-1], 4, 64)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lanes ^ o]
        wsum = v[..., 0]
        return (wsum[..., 0] + wsum[..., 1]) + (wsum[..., 2] + wsum[..., 3])


def block_means(v):
    with np.errstate(invalid="ignore"):
        return (block_sums(blocks_of(v)) / 1024.0).astype(F)


def block_p5(v, variant=None):
    b = blocks_of(v)
    bad = np.isnan(b).any(-1)
    s = np.sort(np.where(bad[..., None], F(0), b), axis=-1)
    lo, hi = s[..., RANK], s[..., RANK + 1]
    if variant == "f64_index":
        r = 0.05 * 1023
        q = (lo.astype(np.float64) + (hi.astype(np.float64) - lo.astype(np.float64)) * (r - np.floor(r))).astype(F)
    else:
        r = F(1023) * F(0.05)
        q = lo + (hi - lo) * F(r - F(RANK))
    return np.where(bad, F(np.nan), q).astype(F)


def zero_ties(v):
    """True when a +0 and a -0 meet at the ranks 51 / 52 of some block without NaN (where the key order and numpy's could pick different signs)"""
    b = blocks_of(v)
    ok = ~np.isnan(b).any(-1)
    s = np.sort(np.where(ok[..., None], b, F(1)), axis=-1)
    at_rank = (s[..., RANK] == 0) | (s[..., RANK + 1] == 0)
    both = ((b == 0) & np.signbit(b)).any(-1) & ((b == 0) & ~np.signbit(b)).any(-1)
    return bool((ok & at_rank & both).any())


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F))).astype(np.float64)


def cond_image(lowres, climate, li, lj, crop, t, *, u_drop=None, dropout_p=0.0, u_noise=None, max_noise=0.0, z_mean=None, z_p5=None,
               norm_mean=None, norm_std=None, raw=False, variant=None, e_mean=None):
    """td_batch_cond_image for one item: (7, g, g) fp32.  climate: the FULL climate array of the group (the channel list is applied here).
    With e_mean (5, g, g), the recorded |reference raw mean - float64 mean| of channels 0, 2 .. 5, also returns the bound of every element."""
    halo = 31 if variant == "halo31" else HALO
    V = crop + 2 * HALO
    chans = (0, 3, 11, 13) if variant == "climate13" else CLIMATE_CHANNELS
    lo = view(window(lowres, li - halo, lj - halo, V, V), t, variant)
    cl = view(window(climate[list(chans)], li - halo, lj - halo, V, V), t, variant)
    g = V // HALO
    mean, cmean, p5 = block_means(lo), block_means(cl), block_p5(lo, variant)
    d = np.zeros((7, g, g))
    if e_mean is not None:
        d[0] = np.where(np.isnan(mean), 0.0, e_mean[0] + ulp(mean))
        d[2:6] = np.where(np.isnan(cmean), 0.0, e_mean[1:] + ulp(cmean))
    mask = F(1) - np.isnan(mean).astype(F)
    if u_drop is not None:
        keep = (u_drop >= F(dropout_p)) if variant == "dropout_ge" else (u_drop > F(dropout_p))
        mask = mask * keep.astype(F)
        mean, p5 = np.where(mask == 0, F(np.nan), mean), np.where(mask == 0, F(np.nan), p5)
        d[0] = np.where(mask == 0, 0.0, d[0])
    if u_noise is not None:
        s = F(u_noise) * F(max_noise)
        mean, p5 = mean + z_mean * s, p5 + z_p5 * s
        d[0] = np.where(np.isnan(mean), 0.0, d[0] + ulp(mean))
    stack = np.concatenate([mean[None], p5[None], cmean, mask[None]]).astype(F)
    if not raw:
        nm, ns = np.asarray(norm_mean, F), np.asarray(norm_std, F)
        for ch in range(2):
            v = stack[ch]
            stack[ch] = np.where(np.isnan(v), nm[ch], np.where(np.isinf(v), np.copysign(np.finfo(F).max, v), v))
        diff = stack - nm[:, None, None]
        out = diff / ns[:, None, None]
        d = np.where(d > 0, (d + ulp(diff)) / np.abs(ns.astype(np.float64))[:, None, None] + ulp(out), 0.0)
        stack = out.astype(F)
    return (stack, d) if e_mean is not None else stack


# ------------------------------------------------------------------------------------------------------------------------------ cond vector
def mp_factors(sizes=(16, 16, 4, 16, 5, 1)):
    """mp_concat's scale of each part (mp_layers.py:77-86) as fp32 computes it: C / sqrt(N_i) * w_i, w = 1 / len, C = sqrt(sum N / sum w^2)"""
    n = len(sizes)
    w = np.full(n, F(1 / n), F)
    sq = w * w
    tot = F(0)
    for v in sq:
        tot = F(tot + v)
    C = np.sqrt(F(F(sum(sizes)) / tot)).astype(F)
    return [F(F(C / F(np.sqrt(s))) * w[i]) for i, s in enumerate(sizes)]


SQRT12 = F(np.sqrt(12))


def cond_vector(img, hist, noise_level, z_replace=None, d_img=None):
    """td_batch_cond_vector for one item: ((58,) fp32, (4,) NaN flags[, the bound per element])"""
    f = mp_factors()
    g = img.shape[-1]
    c0 = g // 2 - 2
    crop = lambda ch: img[ch, c0:c0 + 4, c0:c0 + 4].reshape(-1)
    r = c0 + 1
    with np.errstate(invalid="ignore"):
        s1 = img[2:6, r, r] + img[2:6, r, r + 1]
        s2 = s1 + img[2:6, r + 1, r]
        s3 = s2 + img[2:6, r + 1, r + 1]
        cm = (s3 / F(4)).astype(F)
    flags = np.isnan(cm)
    if z_replace is not None:
        cm = np.where(flags, np.asarray(z_replace, F), cm)
    nl = F(F(F(noise_level) - F(0.5)) * SQRT12)
    out = np.concatenate([crop(0) * f[0], crop(1) * f[1], cm * f[2], crop(6) * f[3], np.asarray(hist, F) * f[4], [nl * f[5]]]).astype(F)
    if d_img is None:
        return out, flags.astype(np.int32)
    dc = lambda ch: d_img[ch, c0:c0 + 4, c0:c0 + 4].reshape(-1)
    d1 = d_img[2:6, r, r] + d_img[2:6, r, r + 1] + ulp(s1)
    d2 = d1 + d_img[2:6, r + 1, r] + ulp(s2)
    d3 = (d2 + d_img[2:6, r + 1, r + 1] + ulp(s3)) / 4.0
    d3 = np.where(flags, 0.0, d3)
    d = np.concatenate([dc(0) * float(f[0]), dc(1) * float(f[1]), d3 * float(f[2]), dc(6) * float(f[3]), np.zeros(6)])
    return out, flags.astype(np.int32), np.where(d > 0, d + ulp(out), 0.0)


# ------------------------------------------------------------------------------------------------------------------------------ comparisons
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def equal_nan(a, b):
    """equal as values, NaN in the same places (NaN payloads are not compared)"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def within(a, b, d):
    """|a - b| <= d elementwise with NaN in the same places; d == 0 asks for equality"""
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return bool((err[~nan] <= d[~nan]).all())


# ------------------------------------------------------------------------------------------------------------------------------ whole items
def latents_item(args, path, i, j, t, draws, e_mean=None, variant=None, with_latent=True):
    """One H5LatentsDataset item from the definitions: args the constructor arguments, draws {'histogram_raw', 'noise', 'u_drop', 'u_noise',
    'z_mean', 'z_p5', 'z_replace' (one value per NaN centre, in slot order)} as recorded.  Returns a dict; with e_mean also the bounds."""
    g = TREE()[path]
    crop, S = args["crop_size"], g["lowfreq"].shape[0]
    li, lj = inverse_offsets(i, j, crop, crop, t, S)
    out = {"lowfreq": views(g["lowfreq"].array, li, lj, crop, crop, t, (LOWFREQ_MEAN, LOWFREQ_STD, args["sigma_data"]))}
    if with_latent:
        out["latent"] = latents(g["latent"].array, t, i, j, crop, crop, draws["noise"], 0, args["latents_mean"], args["latents_std"], args["sigma_data"])
    kw = {}
    if args.get("cond_input_dropout"):
        kw.update(u_drop=draws["u_drop"][0], dropout_p=args["cond_input_dropout"])
    noise_level = F(0)
    if args.get("cond_input_max_noise"):
        noise_level = F(draws["u_noise"][0])
        kw.update(u_noise=noise_level, max_noise=args["cond_input_max_noise"], z_mean=draws["z_mean"][0], z_p5=draws["z_p5"][0])
    res = cond_image(g["lowres_exact"].array, g["climate"].array, li, lj, crop, t, norm_mean=args["cond_input_mean"], norm_std=args["cond_input_std"],
                     variant=variant, e_mean=e_mean, **kw)
    img, d_img = res if e_mean is not None else (res, None)
    _, flags = cond_vector(img, draws["histogram_raw"], noise_level)
    z = np.zeros(4, F)
    if "z_replace" in draws:                                   # four values are by slot (get_batch), fewer are one per NaN centre in slot order
        zr, nan = np.asarray(draws["z_replace"], F), flags.astype(bool)
        if zr.size != 4 and zr.size != int(nan.sum()):         # only a wrong variant gets here: its flags are not the recorded item's
            zr = np.concatenate([zr, np.zeros(4, F)])[:int(nan.sum())]
        z[nan] = zr[nan] if zr.size == 4 else zr
    vec = cond_vector(img, draws["histogram_raw"], noise_level, z, d_img)
    out.update(cond_img=img, cond_vector=vec[0], flags=flags, noise_level=noise_level)
    if e_mean is not None:
        out.update(d_img=d_img, d_vector=vec[2])
    return out


def decoder_item(args, path, i, j, t, noise):
    g = TREE()[path]
    crop, h = args["crop_size"], args["crop_size"] // 8
    li, lj = inverse_offsets(i * 8, j * 8, crop, crop, t, g["residual"].shape[0])
    padded = views(g["lowfreq"].array, i - 1, j - 1, h + 2, h + 2, t)
    return {"image": views(g["residual"].array, li, lj, crop, crop, t, (args["residual_mean"], args["residual_std"], args["sigma_data"]))[None],
            "cond_img": latents(g["latent"].array, t, i, j, h, h, noise, 1), "lowfreq": padded[None, 1:-1, 1:-1], "lowfreq_padded": padded[None]}


def autoencoder_item(args, path, i, j, t):
    crop = args["crop_size"]
    return views(TREE()[path]["residual"].array, i, j, crop, crop, t, (args["residual_mean"], args["residual_std"], 1.0))[None]
