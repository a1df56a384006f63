"""Inputs and independent references for the training-batch kernels' element-wise tests (tests/test_train_data_ops_cpu.py,
tests/test_train_data_ops_gpu.py): small synthetic trees, built from seeds or by construction, that sit on the edges the committed tree
(tests/_train_data_twin.TREE) keeps away from -- rectangular views that overhang every side of groups of unlike sides, a residual whose side
is not 8 S, a missing plane, all 65536 half logvars, hand-placed half and fp32 arithmetic edges, 32 x 32 blocks designed against single parts
of the radix select and of the float64 sum, odd cond-image grids and the centre window of the cond vector.

The references here are written from include/td_batch.h alone and share no code with the twin's: a per-element loop for the views, float64
arithmetic rounded at each named step for the affine and the latent draw, numpy.quantile and math.fsum for the block statistics.  `variant`
arguments name deliberately WRONG restatements (VARIANTS); the CPU test shows that each changes at least one designed output.
NumPy only: no device code, no torch."""
import functools
import math

import numpy as np

import _train_data_twin as twin

F, H = np.float32, np.float16
NAN, INF = F(np.nan), F(np.inf)
Node, Dataset = twin.Node, twin.Dataset
KEPT = twin.CLIMATE_CHANNELS
POISON = F(1e30)                          # in the 11 climate channels nobody should read
RANK = 51
VARIANTS = ("ranks_50_51", "ranks_52_53", "k1_min_gt", "k1_prefix", "unsigned_keys", "nan_wave0_only", "nan_first_value_only", "fp32_sum",
            "halo31", "residual_side_as_side", "half_truncates", "no_swap", "c0_up")


def bits32(*patterns):
    return np.array(patterns, np.uint32).view(F)


def f32_of_f64(x):
    """float64 -> fp32, one rounding, quietly"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(F)


# ------------------------------------------------------------------------------------------------------------------------------ the trees
# placement groups (subchunk, S, R): unlike sides, and residuals whose sides are 8 S, not 8 S and smaller than S
PLACE = (("s0", 128, 1024), ("s1", 33, 40), ("s2", 256, 16))
PLACE_LC = 3
EDGE_S, EDGE_LC = 4, 2
EXP_S = 256
EXP_MULT = (1, 3, 5, 40503, 257, 65535, 12345, 31)      # odd: p -> (p * mult + add) mod 2^16 is a permutation of the half bit patterns
EXP_ADD = (0, 1, 77, 4242, 32768, 65535, 999, 2)
DESIGN_S = 128


def index_plane(S):
    """r * S + c, exact in fp32 for S <= 4096"""
    return np.arange(S * S, dtype=np.float64).reshape(S, S).astype(F)


def place_arrays(n):
    """lowfreq r S + c, lowres_exact r S + c + 0.5, residual -(r R + c) - 1, climate r S + c - 1000 ch in the kept channels and the sentinel in the
    others, a seeded latent of PLACE_LC channels"""
    _, S, R = PLACE[n]
    rng = np.random.default_rng(700 + n)
    idx = index_plane(S)
    climate = np.full((15, S, S), POISON, F)
    for ch in KEPT:
        climate[ch] = idx - F(1000 * ch)
    latent = np.concatenate([rng.standard_normal((8, PLACE_LC, S, S)), -2.0 + 1.5 * rng.standard_normal((8, PLACE_LC, S, S))], axis=1).astype(H)
    return {"latent": latent, "lowfreq": idx, "lowres_exact": idx + F(0.5), "climate": climate, "residual": -index_plane(R) - F(1)}


def exp_table():
    """(8, 256, 256) half: every one of the 65536 bit patterns once per slab, in a different permutation in each"""
    p = np.arange(65536, dtype=np.uint64)
    bits = np.stack([(p * EXP_MULT[t] + EXP_ADD[t]) & 0xffff for t in range(8)]).astype(np.uint16)
    assert all(np.unique(b).size == 65536 for b in bits)
    return bits.view(H).reshape(8, EXP_S, EXP_S)


def exp_arrays():
    return {"latent": np.concatenate([np.zeros((8, 1, EXP_S, EXP_S), H), exp_table()[:, None]], axis=1)}


# the affine operands: a 4 x 4 lowfreq plane of the edge group; 1.25 is also an `a`
AFFINE_X = np.array([0.0, 1.5, -np.inf, np.inf, np.nan, 1e-30, 3e38, -3e38, 1.25, 1e-40, -0.0, 7.0, 1e20, -1e-20, 65504.0, 2.0 ** -126], F)
# (a, b, c): x == a; a negative b (x == a then gives -0); a denormal quotient kept and halved; quotients and products that overflow; a
# difference that overflows; plain rounding; b = 0
AFFINE_ABC = ((1.25, 3.0, 1.0), (1.25, -3.0, 2.0), (0.0, 1e10, 1.0), (0.0, 1e10, 0.5), (0.0, 1e-10, 1e30), (-3e38, 1.0, 1.0), (1.0, 7.0, 1.0 / 3.0),
              (0.0, 0.0, 1.0), (twin.LOWFREQ_MEAN, twin.LOWFREQ_STD, 0.5))

# the latent edges: (mean m, logvar v, mode-0 noise, mode-1 noise) per position of the 4 x 4 edge latent, the same in both channels
_LN2 = math.log(2.0)
LATENT_EDGES = (
    (0.0, np.inf, 0.0, 0.0),                              # noise 0 against e = inf: NaN
    (0.0, 0.0, 1e-40, 2.0 ** -24),                        # denormal noise, fp32 and half
    (np.inf, 0.0, 1.0, 1.0),                              # m = +inf
    (-np.inf, 0.0, 1.0, -1.0),                            # m = -inf
    (2.0 ** -11, 0.0, 1.0, 1.0),                          # mode 1: 1 + 2^-11 is a half midpoint, ties to even: 1
    (2.0 ** -11, 0.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -10),  # mode 1: 1 + 2^-10 + 2^-11 ties to even: 1 + 2^-9
    (0.0, 12.0, 300.0, 300.0),                            # mode 1: 300 e overflows half
    (0.0, -20.0 * _LN2, 3.0, 2.0 ** -10),                 # mode 1: the product lands in half subnormals
    (-2.0 ** -12, 0.0, 1.0, 1.0),                         # mode 1: 1 - 2^-12 ties to even: 1
    (65504.0, 0.0, 16.0, 16.0),                           # mode 1: 65520 ties to even: inf
    (1.0, -40.0, np.inf, np.inf),                         # e = 0 against infinite noise: NaN
    (-0.0, -np.inf, -1.0, -1.0),                          # -0 + -0 keeps its sign
    (np.nan, 0.0, 1.0, 1.0),
    (1.0, np.nan, 1.0, 1.0),
    (1000.0, 2.0, -3.0, -3.0),                            # mode 0, channel 1: the quotient by the tiny std overflows
    (-2.5, -4.0, 0.33, 0.33),
)
EDGE_MEAN, EDGE_STD, EDGE_SIGMA = (0.0, 0.25), (1.0, 1e-38), 0.5


def edge_arrays():
    e = np.array(LATENT_EDGES, np.float64)
    with np.errstate(over="ignore"):
        m, v = e[:, 0].astype(H).reshape(EDGE_S, EDGE_S), e[:, 1].astype(H).reshape(EDGE_S, EDGE_S)
    slab = np.stack([m, m, v, v])
    return {"latent": np.stack([slab] * 8), "lowfreq": AFFINE_X.reshape(EDGE_S, EDGE_S).copy()}


def edge_noise(mode):
    e = np.array(LATENT_EDGES, np.float64)[:, 2 + mode].astype(H if mode else F).reshape(EDGE_S, EDGE_S)
    return np.stack([e, e])[None]


# ------------------------------------------------------------------------------------------------------------------------------ designed blocks
def _distinct(rng, n, lo, hi):
    """n distinct fp32 values in [lo, hi), shuffled"""
    v = (lo + (hi - lo) * (np.arange(n) + 0.5 * rng.random(n)) / n).astype(F)
    assert np.unique(v).size == n and v.min() >= F(lo) and v.max() < F(hi)
    return rng.permutation(v)


def _ranked(rng, below, at, above=(1.0, 900.0)):
    """a shuffled block: 51 distinct values in `below`, the values `at` on the ranks 51 and 52, distinct values in `above` after them"""
    at = np.asarray(at, F)
    return rng.permutation(np.concatenate([_distinct(rng, RANK, *below), at, _distinct(rng, 1024 - RANK - at.size, *above)]).astype(F))


def _copies(rng, k):
    return rng.permutation(np.concatenate([np.full(k, F(-3.5)), _distinct(rng, 1024 - k, 1.0, 900.0)]))


def _zeros(rng, first, second):
    """51 negatives, two zeros, positives: the zero `first` lies before `second` in memory"""
    b = _ranked(rng, (-900.0, -1.0), [7e-3, 7e-3])
    at = np.flatnonzero(b == F(7e-3))
    b[at[0]], b[at[1]] = F(first), F(second)
    return b


def _with_nan(rng, k):
    b = _distinct(rng, 1024, -50.0, 900.0)
    b[k] = NAN
    return b


def _multiset(rng):
    return np.sort((rng.standard_normal(1024) * 40.0).astype(F))


def _last_slot(rng):
    """the multiset permuted so that its rank-51 value is value 1023: the last value of thread 255"""
    s = _multiset(np.random.default_rng(4100))
    b = rng.permutation(s)
    a, z = int(np.flatnonzero(b == s[RANK])[0]), 1023
    b[a], b[z] = b[z], b[a]
    return b


def _cancel(rng):
    """integers near +-2^24 whose sum nearly cancels: every float64 partial sum is exact in any order, an fp32 one is not"""
    pos, neg = 2.0 ** 24 - rng.integers(0, 1000, 512), -(2.0 ** 24 - rng.integers(0, 1000, 512))
    return rng.permutation(np.concatenate([pos, neg])).astype(F)


# the top-byte design: 16 values 1.5 x 4^k that share their low 24 bits, the least of them 52 times so that the ranks 51 and 52 differ; two
# significant bits over a span of 2^30 keep every float64 partial sum exact
_TOP_COUNTS = [52] + [64] * 14 + [76]

DESIGNS = {
    "equal": lambda rng: np.full(1024, F(7.25)),
    "copies51": lambda rng: _copies(rng, 51),
    "copies52": lambda rng: _copies(rng, 52),                  # rank 52 must come from min_gt
    "copies53": lambda rng: _copies(rng, 53),                  # rank 52 must come from the prefix
    "copies54": lambda rng: _copies(rng, 54),
    "low_byte": lambda rng: rng.permutation(np.repeat((np.uint32(0x42c80000) | np.arange(256, dtype=np.uint32)).view(F), 4)),
    "top_byte": lambda rng: rng.permutation(np.repeat(((np.arange(0x38, 0x48, dtype=np.uint32) << 24) | np.uint32(0x00400000)).view(F), _TOP_COUNTS)),
    "sign_change": lambda rng: _ranked(rng, (-900.0, -1.0), [-0.5, 0.25]),
    "zeros_mp": lambda rng: _zeros(rng, -0.0, 0.0),
    "zeros_pm": lambda rng: _zeros(rng, 0.0, -0.0),
    "zeros_mm": lambda rng: _zeros(rng, -0.0, -0.0),
    "denormal_signs": lambda rng: _ranked(rng, (-900.0, -1.0), bits32(0x80000001, 0x00000001)),
    "denormal_gap": lambda rng: _ranked(rng, (-900.0, -1.0), bits32(0x00000003, 0x00000103)),
    "ninf53": lambda rng: rng.permutation(np.concatenate([np.full(53, -INF), _distinct(rng, 971, 1.0, 900.0)])),
    "ninf52": lambda rng: rng.permutation(np.concatenate([np.full(52, -INF), _distinct(rng, 972, 1.0, 900.0)])),
    "pinf_top": lambda rng: rng.permutation(np.concatenate([np.full(5, INF), _distinct(rng, 1019, -50.0, 900.0)])),
    "big_diff": lambda rng: _ranked(rng, (-3.3e38, -3.1e38), [-3e38, 3e38], (3.1e38, 3.39e38)),
    "nan0": lambda rng: _with_nan(rng, 0),
    "nan255": lambda rng: _with_nan(rng, 255),
    "nan256": lambda rng: _with_nan(rng, 256),
    "nan1023": lambda rng: _with_nan(rng, 1023),
    "ascending": lambda rng: _multiset(np.random.default_rng(4100)),
    "descending": lambda rng: _multiset(np.random.default_rng(4100))[::-1].copy(),
    "last_slot": _last_slot,
    "cancel": _cancel,
    "plain": lambda rng: _distinct(rng, 1024, -50.0, 900.0),
}
_ = "plain"
# three planes of 4 x 4 blocks; the NaN blocks lie apart so that each has whole neighbours
DESIGN_LAYOUT = (
    ("equal", "copies51", "copies52", "copies53", "copies54", "low_byte", "top_byte", "sign_change",
     "zeros_mp", "zeros_pm", "zeros_mm", "denormal_signs", "denormal_gap", "cancel", _, _),
    ("ninf53", "ninf52", "pinf_top", "big_diff", "ascending", "descending", "last_slot", _,
     "cancel", _, "copies52", "copies53", _, _, "equal", "sign_change"),
    ("nan0", _, "nan255", _, _, _, _, _,
     _, "nan256", _, _, _, _, _, "nan1023"),
)


@functools.lru_cache(maxsize=None)
def design_block(plane, slot):
    name = DESIGN_LAYOUT[plane][slot]
    b = np.asarray(DESIGNS[name](np.random.default_rng(4000 + 16 * plane + slot)), F)
    assert b.shape == (1024,)
    b.flags.writeable = False
    return b


def plane_of_blocks(blocks):
    """16 blocks of 1024, row-major inside a block -> the (128, 128) plane whose block (by, bx) is blocks[4 by + bx]"""
    return np.asarray(blocks, F).reshape(4, 4, 32, 32).swapaxes(1, 2).reshape(128, 128).copy()


def design_arrays(n):
    """lowres_exact of the designed blocks; every block of the four kept climate channels is a cancellation design (one of plane 2 holds a NaN)"""
    rng = np.random.default_rng(4500 + n)
    climate = np.full((15, DESIGN_S, DESIGN_S), POISON, F)
    for ch in KEPT:
        climate[ch] = plane_of_blocks([_cancel(rng) for _ in range(16)])
    if n == 2:
        climate[3, 40, 70] = NAN
    return {"lowres_exact": plane_of_blocks([design_block(n, s) for s in range(16)]), "climate": climate}


@functools.lru_cache(maxsize=None)
def TREE():
    """res 'place' / 'edge' / 'exp' / 'design', one chunk 'c0'; DeviceGroups(TREE(), keys, need) takes it unchanged"""
    root = Node()
    groups = {"place": {PLACE[n][0]: place_arrays(n) for n in range(len(PLACE))}, "edge": {"s0": edge_arrays()}, "exp": {"s0": exp_arrays()},
              "design": {f"s{n}": design_arrays(n) for n in range(len(DESIGN_LAYOUT))}}
    for res, subs in groups.items():
        chunk = Node()
        for sub, arrays in subs.items():
            g = Node({k: Dataset(v, pct_land=0.5, split="train") for k, v in arrays.items()})
            g.attrs["beauty_score"] = 3.0
            dict.__setitem__(chunk, sub, g)
        res_node = Node()
        dict.__setitem__(res_node, "c0", chunk)
        dict.__setitem__(root, res, res_node)
    return root


PLACE_KEYS = [("c0", "place", sub) for sub, _, _ in PLACE]
EDGE_KEYS = [("c0", "edge", "s0")]
EXP_KEYS = [("c0", "exp", "s0")]
DESIGN_KEYS = [("c0", "design", f"s{n}") for n in range(len(DESIGN_LAYOUT))]
ALL_PLANES = ("latent", "lowfreq", "lowres_exact", "climate", "residual")


def arrays(key):
    chunk, res, sub = key
    return {k: v.array for k, v in TREE()[f"{res}/{chunk}/{sub}"].items()}


# ------------------------------------------------------------------------------------------------------------------------------ 1. views
VIEW_SHAPES = ((1, 1), (1, 7), (7, 1), (5, 9), (33, 2))
VIEW_PLANES = ("lowfreq", "lowres_exact", "residual")
VIEW_OFFSETS = (-1, 2)                   # by origin: 0 reads (li, lj), 1 reads (i, j); the fields of the other origin point elsewhere


def view_items(h, w, plane, origin):
    """(N, 6) items over the three placement groups: every transform against every position of the window -- over the top, the bottom, the left
    and the right edge of THIS plane, wholly outside, wholly inside, over a corner.  59 items (295 for one pixel): N h w is above 256 and no
    multiple of it, and n % 8 with n % 7 meets every pair."""
    N = 59 * (5 if h * w == 1 else 1)
    assert N * h * w > 256 and (N * h * w) % 256
    rows = []
    for n in range(N):
        g, t, cat = n % 3, n % 8, n % 7
        side = PLACE[g][2] if plane == "residual" else PLACE[g][1]
        hh, ww = (w, h) if t % 2 else (h, w)
        inr, inc = max(0, min(1, side - hh)), max(0, min(2, side - ww))
        r0, c0 = ((-((hh + 1) // 2), inc), (side - hh // 2, inc), (inr, -((ww + 1) // 2)), (inr, side - ww // 2), (-hh - 3, side + 2), (inr, inc),
                  (-1, side - ww + 1))[cat]
        pos = (r0 - VIEW_OFFSETS[origin], c0 - VIEW_OFFSETS[origin])
        other = (pos[0] + 5, pos[1] - 3)
        rows.append([g, *pos, t, *other] if origin else [g, *other, t, *pos])
    return np.array(rows, np.int32)


def unview(t, h, w, r, c, swap=True):
    """the kernels' inverse map restated (only the wrong variant `no_swap` uses it): the window position shown at (r, c) of the (h, w) view"""
    k = t % 4
    hA, wA = (w, h) if (k % 2 and swap) else (h, w)
    br, bc = ((r, c), (c, wA - 1 - r), (hA - 1 - r, wA - 1 - c), (hA - 1 - c, r))[k]
    return br, (wA - 1 - bc if t // 4 else bc)


def view_loop(plane, r0, c0, h, w, t, variant=None, side=None):
    """The (h, w) view of the window of `plane` at (r0, c0) from the header's sentence alone -- flip the last axis if t / 4 == 1, then rot90 by
    t % 4 -- one element at a time; NaN outside the plane.  side: the side the plane is ADDRESSED with (the wrong variant that takes the
    residual's side for S reads the flat plane with the wrong stride and bound)."""
    S = plane.shape[-1] if side is None else side
    flat = plane.reshape(-1)

    def at(r, c):
        return flat[r * S + c] if 0 <= r < S and 0 <= c < S and r * S + c < flat.size else NAN
    k = t % 4
    if variant == "no_swap":
        return np.array([[at(*(np.add(unview(t, h, w, r, c, swap=False), (r0, c0)))) for c in range(w)] for r in range(h)], F)
    hA, wA = (w, h) if k % 2 else (h, w)
    A = [[at(r0 + r, c0 + c) for c in range(wA)] for r in range(hA)]
    if t // 4 == 1:
        A = [[row[wA - 1 - c] for c in range(wA)] for row in A]
    for _ in range(k):                   # one quarter turn counterclockwise: the last column becomes the first row
        rows, cols = len(A), len(A[0])
        A = [[A[c][cols - 1 - r] for c in range(rows)] for r in range(cols)]
    out = np.array(A, F)
    assert out.shape == (h, w)
    return out


def views_ref(plane_name, items, origin, h, w, keys=None, variant=None):
    """(N, h, w): view_loop for every item of view_items"""
    keys = PLACE_KEYS if keys is None else keys
    out = []
    for g, i, j, t, li, lj in items.tolist():
        a = arrays(keys[g])
        plane = a[plane_name]
        r0, c0 = ((i, j) if origin else (li, lj))
        side = a["lowfreq"].shape[-1] if (variant == "residual_side_as_side" and plane_name == "residual") else None
        out.append(view_loop(plane, r0 + VIEW_OFFSETS[origin], c0 + VIEW_OFFSETS[origin], h, w, t, variant, side))
    return np.stack(out)


def affine_ref(x, a, b, c):
    """((x - a) / b) * c: each operation in float64 on the promoted fp32 operands, rounded once to fp32"""
    x = np.asarray(x, F).astype(np.float64)
    with np.errstate(all="ignore"):
        d = f32_of_f64(x - np.float64(F(a)))
        q = f32_of_f64(d.astype(np.float64) / np.float64(F(b)))
        return f32_of_f64(q.astype(np.float64) * np.float64(F(c)))


# ------------------------------------------------------------------------------------------------------------------------------ 2. latents
def half_truncated(x):
    """fp32 -> half rounding toward zero (the wrong variant)"""
    x = np.asarray(x, F)
    with np.errstate(over="ignore"):
        h = x.astype(H)
    too_big = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))
    return np.where(too_big & ~np.isnan(h), np.nextafter(h, H(0)), h).astype(H)


def latent_draw_ref(m, v, noise, mode, mean=None, std=None, sigma_data=0.5, variant=None):
    """The header's arithmetic on halves m, v (c, h, w) and the noise: float64 operations on the promoted values, each rounded to fp32 and, in
    mode 1, from there to half at the steps the header names.  e is twin.half_std (the exhaustive test is what pins it)."""
    to_half = half_truncated if variant == "half_truncates" else (lambda x: np.asarray(x, F).astype(H))
    e = twin.half_std(v).astype(np.float64)
    n, m = np.asarray(noise).astype(np.float64), np.asarray(m).astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == 0:
            s = f32_of_f64(n * e)
            x = f32_of_f64(s.astype(np.float64) + m)
            d = f32_of_f64(x.astype(np.float64) - np.asarray(mean, F).astype(np.float64).reshape(-1, 1, 1))
            z = f32_of_f64(d.astype(np.float64) / np.asarray(std, F).astype(np.float64).reshape(-1, 1, 1))
            return f32_of_f64(z.astype(np.float64) * np.float64(F(sigma_data)))
        p = to_half(f32_of_f64(n * e))
        return to_half(f32_of_f64(p.astype(np.float64) + m))


def latents_window(latent, t, i, j, h, w, noise, mode, draw, **kw):
    """one item over a window that may leave the latent: `draw`(m, v, noise, mode, **kw) on the part inside, +0 elsewhere; mode 1 repeated 8 x 8"""
    lc, S = latent.shape[1] // 2, latent.shape[-1]
    out = np.zeros((lc, h, w), H if mode else F)
    a0, a1, b0, b1 = max(0, i), min(S, i + h), max(0, j), min(S, j + w)
    if a1 > a0 and b1 > b0:
        m, v = latent[t, :lc, a0:a1, b0:b1], latent[t, lc:, a0:a1, b0:b1]
        out[:, a0 - i:a1 - i, b0 - j:b1 - j] = draw(m, v, noise[:, a0 - i:a1 - i, b0 - j:b1 - j], mode, **kw)
    return np.repeat(np.repeat(out, 8, axis=-2), 8, axis=-1) if mode else out


def twin_draw(m, v, noise, mode, mean=None, std=None, sigma_data=0.5):
    """twin.latents on arrays already cut out"""
    lat = np.concatenate([m, v], axis=0)[None]
    out = twin.latents(lat, 0, 0, 0, m.shape[-2], m.shape[-1], noise, mode, mean, std, sigma_data)
    return out[:, ::8, ::8] if mode else out


RECT_SHAPES = ((3, 5), (1, 9))
RECT_MEAN, RECT_STD, RECT_SIGMA = (0.1, -0.2, 0.05), (1.1, 0.9, 1.3), 0.5


def rect_items(h, w):
    """items over the placement groups whose (h, w) latent windows start at negative i / j, run past S, lie outside and lie inside"""
    N = 7 if (h, w) == (3, 5) else 11
    assert (N * PLACE_LC * h * w) % 256 and N * PLACE_LC * h * w > 256
    rows = []
    for n in range(N):
        g, t = n % 3, (3 * n + 1) % 8
        S = PLACE[g][1]
        i, j = ((-1, 2), (S - 1, S - w + 1), (1, -2), (S - h + 1, 3), (-h, -w), (2, 2), (S, 0), (4, S - 2), (-2, -1), (0, 0), (S - h, S - w))[n]
        rows.append([g, i, j, t, 0, 0])
    return np.array(rows, np.int32)


def rect_noise(h, w, mode):
    rng = np.random.default_rng(910 + h + mode)
    return rng.standard_normal((len(rect_items(h, w)), PLACE_LC, h, w)).astype(H if mode else F)


def single_rounded_half(hv):
    """per unique finite half hv: the half that ONE rounding of the exact exp(hv) gives (mpmath, 200 bits), as a dict hv bits -> half bits"""
    import mpmath
    mpmath.mp.prec = 200
    out = {}
    for b in np.unique(np.asarray(hv, H).view(np.uint16)):
        x = np.array([b], np.uint16).view(H)[0]
        if not np.isfinite(x):
            continue
        y = mpmath.exp(mpmath.mpf(float(x)))
        ex = max(int(mpmath.floor(mpmath.log(y, 2))), -14)
        if ex >= 16:                                      # beyond every half: the rounding overflows
            out[int(b)] = 0x7c00
            continue
        q = mpmath.ldexp(y, 10 - ex)                      # in units of the half spacing at this exponent
        n = int(mpmath.floor(q))
        frac = q - n
        n += 1 if (frac > 0.5 or (frac == 0.5 and n % 2)) else 0
        val = math.ldexp(n, ex - 10)
        out[int(b)] = int(np.array([np.inf if val >= 65520.0 else val]).astype(H).view(np.uint16)[0])
    return out


def fp32_midpoint_distance(hv):
    """the least relative distance of the exact exp(hv) from a rounding midpoint of fp32, over the finite halves hv whose exponential is a
    normal fp32 number other than exp(0) = 1 (mpmath, 200 bits): a float64 exponential that much more accurate rounds to fp32 as the exact one"""
    import mpmath
    mpmath.mp.prec = 200
    least = mpmath.mpf(1)
    for b in np.unique(np.asarray(hv, H).view(np.uint16)):
        x = float(np.array([b], np.uint16).view(H)[0])
        if not math.isfinite(x) or x == 0.0 or not -87.0 < x < 88.0:
            continue
        y = mpmath.exp(mpmath.mpf(x))
        q = mpmath.ldexp(y, 23 - int(mpmath.floor(mpmath.log(y, 2))))
        least = min(least, abs(q - mpmath.floor(q) - mpmath.mpf(0.5)) / q)
    return float(least)


# ------------------------------------------------------------------------------------------------------------------------------ 3. cond image
def exact_mean(block):
    """math.fsum(block) / 1024 rounded once to fp32; NaN with a NaN; with an infinity the float64 sum (any order gives the same)"""
    b = np.asarray(block, F).astype(np.float64)
    if np.isnan(b).any():
        return NAN
    with np.errstate(all="ignore"):
        return F((math.fsum(b) if np.isfinite(b).all() else float(b.sum())) / 1024.0)


def numpy_p5(block):
    """numpy.quantile(block, 0.05) of the fp32 block, by NumPy itself"""
    with np.errstate(all="ignore"):
        q = np.quantile(np.asarray(block, F), 0.05)
    assert q.dtype == F
    return F(q)


def keys_of(v):
    u = np.asarray(v, F).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.uint32(k)
    return np.array([k & np.uint32(0x7fffffff) if k >> 31 else ~k], np.uint32).view(F)[0]


def select_p5(block, variant=None):
    """ba_select2 and the interpolation restated over a sort, for the wrong variants: the key of rank 51, the count of keys <= it, the least
    key above it, then a + (b - a) t in fp32"""
    block = np.asarray(block, F)
    nan = np.isnan(block)
    seen = nan.copy()
    if variant == "nan_wave0_only":
        seen &= (np.arange(1024) % 256) < 64
    if variant == "nan_first_value_only":
        seen &= np.arange(1024) < 256
    if seen.any():
        return NAN
    rank = {"ranks_50_51": 50, "ranks_52_53": 52}.get(variant, RANK)
    k = np.sort(keys_of(block) if variant != "unsigned_keys" else (block.view(np.uint32) | np.uint32(0x80000000)))
    k0 = k[rank]
    above = k[k > k0]
    min_gt = above.min() if above.size else np.uint32(0xffffffff)
    k1 = k0 if int((k <= k0).sum()) >= rank + 2 else min_gt
    if variant == "k1_min_gt":
        k1 = min_gt
    if variant == "k1_prefix":
        k1 = k0
    a, b = unkey(k0), unkey(k1)
    with np.errstate(all="ignore"):
        return F(a + F(F(b - a) * F(F(1023) * F(0.05) - F(RANK))))


def block_mean_fp32(block):
    """the wrong variant that runs the kernels' tree in fp32"""
    x = np.asarray(block, F).reshape(4, 256)
    with np.errstate(all="ignore"):
        acc = np.zeros(256, F)
        for e in range(4):
            acc = acc + x[e]
        v = acc.reshape(4, 64)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ o]
        return F(F(F(v[0, 0] + v[1, 0]) + F(v[2, 0] + v[3, 0])) / F(1024))


def block_grid(plane, stat):
    """(g, g): `stat` of every 32 x 32 block of a plane, row-major inside a block"""
    g = plane.shape[-1] // 32
    return np.array([[stat(plane[32 * by:32 * by + 32, 32 * bx:32 * bx + 32].reshape(-1)) for bx in range(g)] for by in range(g)], F)


@functools.lru_cache(maxsize=None)
def design_grids(n, variant=None):
    """the six 4 x 4 grids of statistics of the untransformed design plane n: mean, p5, four climate means"""
    a = arrays(DESIGN_KEYS[n])
    mean_of = block_mean_fp32 if variant == "fp32_sum" else exact_mean
    p5_of = numpy_p5 if variant is None else (lambda b: select_p5(b, variant))
    return [block_grid(a["lowres_exact"], mean_of), block_grid(a["lowres_exact"], p5_of)] + [block_grid(a["climate"][ch], mean_of) for ch in KEPT]


def design_raw_ref(n, t, variant=None):
    """The raw cond image (7, 4, 4) of design plane n under transform t, without the twin: a dihedral view of the plane carries whole blocks to
    whole blocks and keeps each block's multiset, so the statistics of the UNTRANSFORMED blocks are computed once (math.fsum, numpy.quantile) and
    their 4 x 4 grid is moved by the same view."""
    moved = [view_loop(g, 0, 0, 4, 4, t) for g in design_grids(n, variant)]
    return np.stack(moved + [F(1) - np.isnan(moved[0]).astype(F)]).astype(F)


NORM_MEAN = (13.36, 10.03, 16.17, 612.99, 869.73, 71.64, 0.674)
NORM_STD = (22.22, 22.13, 10.23, 453.81, 797.71, 34.23, 0.460)


def normalise_ref(raw, nm=NORM_MEAN, ns=NORM_STD):
    """raw = 0 of the header: nan_to_num of the channels 0 and 1, then (x - mean) / std, each in float64 rounded once to fp32"""
    nm, ns = np.asarray(nm, F), np.asarray(ns, F)
    x = np.array(raw, F)
    for ch in range(2):
        v = x[..., ch, :, :]
        x[..., ch, :, :] = np.where(np.isnan(v), nm[ch], np.where(np.isinf(v), np.copysign(np.finfo(F).max, v), v))
    with np.errstate(all="ignore"):
        d = f32_of_f64(x.astype(np.float64) - nm.astype(np.float64)[:, None, None])
        return f32_of_f64(d.astype(np.float64) / ns.astype(np.float64)[:, None, None])


def design_items(n_planes=len(DESIGN_LAYOUT)):
    """every design plane under every transform: S = 128, crop 64, li = lj = 32, so the haloed view is the whole plane"""
    return np.array([[g, 0, 0, t, 32, 32] for g in range(n_planes) for t in range(8)], np.int32)


# other crops: (crop, items over the placement groups); li / lj put one item partly off the plane, and S = 33 with one whole block
CROPS = {96: np.array([[2, 0, 0, 3, 40, 48], [0, 0, 0, 6, -10, 70], [1, 0, 0, 5, -32, -63]], np.int32),
         128: np.array([[2, 0, 0, 1, 32, 64], [2, 0, 0, 4, 150, -20], [0, 0, 0, 7, 0, -32]], np.int32)}
DROPOUT_P, MAX_NOISE = 0.2, 0.1


def crop_draws(crop):
    """u_drop, u_noise, z_mean, z_p5 for CROPS[crop] with the edges planted: a uniform EQUAL to fl(dropout_p) (drops: the comparison is a
    strict >), the fp32 number above it (keeps), a NaN uniform (drops), u_noise = 0 in the first item"""
    g, rng = (crop + 64) // 32, np.random.default_rng(crop)
    u_drop = rng.random((3, g, g)).astype(F)
    for n in range(3):
        u_drop[n, 1, 1], u_drop[n, 1, 2], u_drop[n, 2, 1] = F(DROPOUT_P), np.nextafter(F(DROPOUT_P), INF), NAN
    u_noise = np.array([0.0, 0.7, 1.0], F)
    return {"u_drop": u_drop, "u_noise": u_noise, "z_mean": rng.standard_normal((3, g, g)).astype(F), "z_p5": rng.standard_normal((3, g, g)).astype(F)}


def crop_twin(crop, *, draws=True, raw=False, norm_std=NORM_STD, variant=None):
    """(3, 7, g, g): the twin's cond image of CROPS[crop], with the planted draws or without"""
    d = crop_draws(crop)
    out = []
    for n, (g, _, _, t, li, lj) in enumerate(CROPS[crop].tolist()):
        a = arrays(PLACE_KEYS[g])
        kw = dict(u_drop=d["u_drop"][n], dropout_p=DROPOUT_P, u_noise=d["u_noise"][n], max_noise=MAX_NOISE, z_mean=d["z_mean"][n], z_p5=d["z_p5"][n]) if draws else {}
        with np.errstate(all="ignore"):
            out.append(twin.cond_image(a["lowres_exact"], a["climate"], li, lj, crop, t, norm_mean=NORM_MEAN, norm_std=norm_std, raw=raw, variant=variant, **kw))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def crop_raw_ref(crop):
    """(3, 7, g, g): the raw cond image of CROPS[crop] without the twin's statistics: the haloed view by view_loop, math.fsum and numpy.quantile"""
    V, out = crop + 64, []
    for g, _, _, t, li, lj in CROPS[crop].tolist():
        a = arrays(PLACE_KEYS[g])
        planes = [a["lowres_exact"]] + [a["climate"][ch] for ch in KEPT]
        v = [view_loop(p, li - 32, lj - 32, V, V, t) for p in planes]
        mean = block_grid(v[0], exact_mean)
        out.append(np.stack([mean, block_grid(v[0], numpy_p5)] + [block_grid(x, exact_mean) for x in v[1:]] + [F(1) - np.isnan(mean).astype(F)]))
    return np.stack(out).astype(F)


# ------------------------------------------------------------------------------------------------------------------------------ cond vector
VECTOR_N = 5
VECTOR_GS = (4, 5, 6, 7)
ORDER_CENTRE = (1e8, 1.0, -1e8, 1.0)      # only ((x00 + x01) + x10) + x11 gives 1 in fp32 (then 0.25); other orders give 2 or 0


def vector_inputs(g):
    """cond images (5, 7, g, g) of distinct elements 1000 ch + 10 r + c + n / 8: item 1 carries ORDER_CENTRE in the centre of every climate
    channel, item 2 one NaN in one centre cell (channel 3), item 3 a NaN in two (channels 2 and 5), item 4 a NaN INSIDE the 4 x 4 window of
    channel 2 but outside its centre (no flag); the histogram, the noise levels and the replacements"""
    ch, r, c = np.meshgrid(np.arange(7), np.arange(g), np.arange(g), indexing="ij")
    img = np.stack([(1000 * ch + 10 * r + c + n / 8.0).astype(F) for n in range(VECTOR_N)])
    m = g // 2
    img[1, 2:6, m - 1:m + 1, m - 1:m + 1] = np.array(ORDER_CENTRE, F).reshape(2, 2)
    img[2, 3, m, m - 1] = NAN
    img[3, 2, m, m] = img[3, 5, m - 1, m - 1] = NAN
    img[4, 2, m - 2, m - 2] = NAN
    rng = np.random.default_rng(60 + g)
    return {"img": img, "hist": rng.standard_normal((VECTOR_N, 5)).astype(F), "noise_level": rng.random(VECTOR_N).astype(F),
            "z_replace": rng.standard_normal((VECTOR_N, 4)).astype(F)}


def cond_vector_ref(img, hist, noise_level, z_replace=None, variant=None):
    """build_cond_inputs of one item from the header: ((58,) fp32, (4,) flags), one element at a time"""
    f = twin.mp_factors()
    g = img.shape[-1]
    c0 = g // 2 - 2
    if variant == "c0_up":
        c0 = -((4 - g) // 2)              # (g - 4) / 2 rounded up
    out, flags = np.empty(58, F), np.zeros(4, np.int32)
    with np.errstate(all="ignore"):
        for k in range(16):
            r, c = c0 + k // 4, c0 + k % 4
            out[k], out[16 + k], out[36 + k] = F(img[0, r, c] * f[0]), F(img[1, r, c] * f[1]), F(img[6, r, c] * f[3])
        for s in range(4):
            x = img[2 + s, c0 + 1:c0 + 3, c0 + 1:c0 + 3]
            m = F(F(F(F(x[0, 0] + x[0, 1]) + x[1, 0]) + x[1, 1]) / F(4))
            if np.isnan(m):
                flags[s] = 1
                if z_replace is not None:
                    m = F(z_replace[s])
            out[32 + s] = F(m * f[2])
        for k in range(5):
            out[52 + k] = F(F(hist[k]) * f[4])
        out[57] = F(F(F(F(noise_level) - F(0.5)) * twin.SQRT12) * f[5])
    return out, flags


# ------------------------------------------------------------------------------------------------------------------------------ comparisons
def same_values(a, b):
    """the same bits wherever neither is NaN, and NaN in the same places (NaN payloads are not compared)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(u)[~nan], b.view(u)[~nan]))


def first_difference(a, b):
    """a short description of where same_values fails, for assertion messages"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shapes / dtypes {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    bad = ~((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b)))
    at = np.argwhere(bad)
    return f"{len(at)} differ, first at {tuple(at[0])}: {a[tuple(at[0])]!r} vs {b[tuple(at[0])]!r}" if len(at) else "equal"
