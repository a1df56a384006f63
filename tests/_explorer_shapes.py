"""Inputs for the explorer kernels' element-wise tests (tests/test_explorer_ops_cpu.py, tests/test_explorer_ops_gpu.py): closed-form or seeded
fp32 arrays that sit on the edges the recorded route cases (tests/golden/explorer.npz) do not reach -- colour-table boundaries under explicit
ranges whose ends are no fp32 numbers, filter bounds met exactly, channel sums past the strided kernel's first 262144 pixels with zero,
negative, subnormal and NaN weights, every k / 255 quantisation step, raw tiles with odd pixel counts, and land planes at 1024, 1025 and 2080
blocks, at capacity 0, at a full index buffer and with window counts that meet the threshold exactly.  NumPy only: no device code, no torch."""
import functools

import numpy as np

F = np.float32
NAN, INF = F(np.nan), F(np.inf)


def neighbours(v):
    """v (fp32) followed by the fp32 number below and the one above each of its elements."""
    v = np.atleast_1d(np.asarray(v, F))
    return np.concatenate([v, np.nextafter(v, -INF), np.nextafter(v, INF)])


def _plant(base, planted, rng, free=None):
    """`base` (flat fp32, seeded) with `planted` written over distinct seeded positions (among `free`, when given)."""
    planted = np.asarray(planted, F)
    out = base.astype(F)
    free = np.arange(out.size) if free is None else np.asarray(free)
    assert planted.size < free.size, (planted.size, free.size)
    out[rng.permutation(free)[:planted.size]] = planted
    return out


# ------------------------------------------------------------------------------------------------------------------------------ 1. colour fields
RANGES = ((-100.3, 2500.7), (0.1, 0.7), (-1e-3, 1.0 / 3.0))      # no end is an fp32 number
COLOUR_SHAPE = (37, 67)                                          # 2479 pixels: 9 blocks of 256 and 175 more


def table_boundaries(vmin, vmax):
    """fp32(vmin + (vmax - vmin) k / 256) for k = 0 .. 256: where the table index steps; k = 0 is fp32(vmin), k = 256 is fp32(vmax)."""
    return (vmin + (vmax - vmin) * np.arange(257, dtype=np.float64) / 256.0).astype(F)


@functools.lru_cache(maxsize=None)
def colour_field(vmin, vmax, seed=0, infinities=True):
    """Seeded values from a quarter of the span below vmin to a quarter above vmax, with every table boundary and its two fp32 neighbours,
    NaN, +-0.0 and (infinities) +-inf planted."""
    rng = np.random.default_rng(100 + seed)
    n = COLOUR_SHAPE[0] * COLOUR_SHAPE[1]
    span = vmax - vmin
    base = rng.uniform(vmin - 0.25 * span, vmax + 0.25 * span, n)
    special = [NAN, F(0.0), F(-0.0)] + ([INF, -INF] if infinities else [])
    out = _plant(base, np.concatenate([neighbours(table_boundaries(vmin, vmax)), np.array(special, F)]), rng).reshape(COLOUR_SHAPE)
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def implicit_field():
    """A field for the implicit range: its own minimum and maximum are the fp32 numbers LO and HI below, the table boundaries between them
    (and their neighbours inside the range) are planted, with NaN and +-0.0.  No infinity: the range is the field's own."""
    lo, hi = float(F(-413.7)), float(F(1871.3))
    rng = np.random.default_rng(110)
    n = COLOUR_SHAPE[0] * COLOUR_SHAPE[1]
    planted = neighbours(table_boundaries(lo, hi))
    planted = planted[(planted >= F(lo)) & (planted <= F(hi))]
    out = _plant(rng.uniform(lo, hi, n), np.concatenate([planted, np.array([NAN, NAN, F(0.0), F(-0.0)], F)]), rng).reshape(COLOUR_SHAPE)
    assert np.nanmin(out) == F(lo) and np.nanmax(out) == F(hi)
    out.flags.writeable = False
    return out


def constant_field():
    """One value and a few NaN: vmax == vmin, so the colours use vmax = vmin + 1."""
    out = np.full(COLOUR_SHAPE, F(7.3))
    out[0, 0] = out[17, 40] = out[-1, -1] = NAN
    return out


def all_nan_field():
    return np.full(COLOUR_SHAPE, NAN)


@functools.lru_cache(maxsize=None)
def precip_field():
    """Seeded values over the precipitation range (a fifth of them negative: log1p(max(x, 0)) shows them as 0), two NaN, no planted boundary:
    the log1p view exempts pixels within 4 ulp of a boundary, and their share is capped."""
    rng = np.random.default_rng(120)
    out = rng.uniform(-700.0, 2800.0, COLOUR_SHAPE).astype(F)
    out[3, 5] = out[30, 66] = NAN
    out[9, 9], out[9, 10] = F(0.0), F(-0.0)
    out.flags.writeable = False
    return out


# ----------------------------------------------------------------------------------------------------------------------------- 2. filter planes
# (lo or None, hi or None): a bound that is no fp32 number and rounds up (0.1) or down (0.7) -- the host rounds it with (float) --, infinite
# bounds (only a NaN fails them), lo only, hi only and both
FILTER_BOUNDS = ((0.1, None), (None, 0.1), (0.7, None), (-2.5, 7.25), (None, float("inf")), (float("-inf"), None), (-100.3, 2500.7),
                 (float("-inf"), float("inf")))


@functools.lru_cache(maxsize=None)
def filter_planes():
    """Eight (plane, lo, hi) of the colour fields' shape: seeded values around the bounds, with NaN, +-inf, +-0.0, fp32(bound) and its two
    fp32 neighbours planted at positions of the plane's own."""
    out = []
    for k, (lo, hi) in enumerate(FILTER_BOUNDS):
        rng = np.random.default_rng(200 + k)
        ends = [b for b in (lo, hi) if b is not None and np.isfinite(b)]
        centre, scale = 0.0, 1.0                                  # about one value in six fails a finite bound
        if len(ends) == 2:
            centre, scale = np.mean(ends), np.ptp(ends) / 3.0
        elif ends:
            centre = ends[0] + (1.0 if lo is not None else -1.0)
        base = rng.normal(centre, scale, COLOUR_SHAPE[0] * COLOUR_SHAPE[1])
        planted = np.concatenate([neighbours(np.array(ends, F)) if ends else np.zeros(0, F), np.array([NAN, INF, -INF, F(0.0), F(-0.0)], F)])
        plane = _plant(base, np.tile(planted, 4), rng).reshape(COLOUR_SHAPE)
        plane.flags.writeable = False
        out.append((plane, lo, hi))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------------ 3. channel sums
WEIGHTS = np.array([0.0, -0.0, -1.5, 1e-8, -1e-8, 1e-40, -1e-40, np.nan, 1.0, 2.0 ** -126], F)
NUMERATORS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-20, -1e-20, 1e25, -3e38, 1.5, 3e-23], F)   # (1e-20 / 1)^2 is subnormal
CHANNEL_CASES = (("stride", (7, 520, 520), (0, 2, 6)), ("one", (2, 5, 13), (0, 1)), ("eight", (9, 3, 7), (0, 8)))
CHANNEL_EPS = (0.0, 1e-8)
CHANNELS_GRID_PIXELS = 1024 * 256      # what one sweep of the strided kernel covers


@functools.lru_cache(maxsize=None)
def channel_sums(name):
    """(C + 1, H, W) sums, the weight plane last.  Seeded values, and runs of edge pixels at flat index 0 and (where the plane is that large)
    past the strided kernel's first sweep: pixel p of a run has the weight WEIGHTS[p % 10] and, in channel c, the numerator
    NUMERATORS[(p // 10 + c) % 11], so every pairing occurs in some channel."""
    shape = dict((n, s) for n, s, _ in CHANNEL_CASES)[name]
    C, n = shape[0] - 1, shape[1] * shape[2]
    rng = np.random.default_rng(300 + C)
    w = rng.uniform(0.5, 1.5, n).astype(F)
    sums = np.concatenate([(rng.normal(0.0, 30.0, (C, n)) * w).astype(F), w[None]])
    run = min(n, WEIGHTS.size * NUMERATORS.size)
    for start in (0, CHANNELS_GRID_PIXELS + 17):
        if start + run <= n:
            p = np.arange(run)
            sums[C, start:start + run] = WEIGHTS[p % WEIGHTS.size]
            for c in range(C):
                sums[c, start:start + run] = NUMERATORS[(p // WEIGHTS.size + c) % NUMERATORS.size]
    sums = sums.reshape(shape)
    sums.flags.writeable = False
    return sums


# -------------------------------------------------------------------------------------------------------------------------- 4. RGB for quantize
RGB_SHAPE = (33, 31, 3)
RGB_SPECIAL = np.array([-0.5, -0.0, 0.0, 1.0, np.nextafter(F(1), F(2)), 7.0, np.nan, np.inf, -np.inf], F)


def quantize_steps():
    """Every fp32(k / 255) with its two neighbours, and the neighbours of fp32((k + 1) / 255 - 1e-6), just under the next step."""
    k = np.arange(256, dtype=np.float64)
    return np.concatenate([neighbours((k / 255.0).astype(F)), neighbours(((k + 1) / 255.0 - 1e-6).astype(F))])


@functools.lru_cache(maxsize=None)
def quantize_rgb():
    rng = np.random.default_rng(400)
    n = int(np.prod(RGB_SHAPE))
    lone = ((5, 5, 1), (20, 7, 0), (32, 30, 2))                     # pixels with a NaN in this one channel only
    taken = np.concatenate([np.arange(3) + 3 * (i * RGB_SHAPE[1] + j) for i, j, _ in lone])
    out = _plant(rng.uniform(-0.2, 1.2, n), np.concatenate([quantize_steps(), np.tile(RGB_SPECIAL, 3)]), rng,
                 free=np.setdiff1d(np.arange(n), taken)).reshape(RGB_SHAPE)
    for i, j, c in lone:
        out[i, j, c] = NAN
    out.flags.writeable = False
    return out


# --------------------------------------------------------------------------------------------------------------------------------- 5. raw tiles
RAW_SHAPES = ((1, 1), (3, 5), (17, 15), (255, 257))               # odd pixel counts: the fp32 words start at a byte offset of 2 mod 4
RAW_ELEV_EDGES = np.array([-0.25, 32768.7, -32768.7, np.nan, -1e-40, -0.0, np.inf, -np.inf, 32767.0, -32768.0, -1.0, 0.999, 32767.5, -32769.0,
                           -3.75, 40000.0, 1e-40], F)
RAW_TEMP_WORDS = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x3FC00000,
                           0x0000FFFF, 0xFFFF0000], np.uint32)   # quiet and signalling NaN payloads, -0.0, subnormals, +-inf, halves of all ones


def raw_tile(shape):
    """(elev, temp): the edge values cycled through the first pixels (as many as fit), seeded values after them -- elevations beyond the
    int16 range on both sides and in (-1, 0); temperatures as arbitrary words."""
    n = shape[0] * shape[1]
    rng = np.random.default_rng(500 + n)
    elev = np.where(rng.random(n) < 0.2, rng.uniform(-1.0, 0.0, n), rng.uniform(-40000.0, 40000.0, n)).astype(F)
    words = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k = min(n, 2 * RAW_ELEV_EDGES.size)
    elev[:k] = np.resize(RAW_ELEV_EDGES, k)
    k = min(n, 2 * RAW_TEMP_WORDS.size)
    words[:k] = np.resize(RAW_TEMP_WORDS, k)
    return elev.reshape(shape), words.view(F).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------------------- 6. land planes
def _seeded_land(H, W, seed, share=0.5):
    rng = np.random.default_rng(600 + seed)
    land = rng.random((H, W)) < share
    return np.where(land, rng.uniform(0.1, 900.0, (H, W)), -rng.uniform(0.0, 900.0, (H, W))).astype(F)


def _pattern(H, W, fn):
    i, j = np.mgrid[0:H, 0:W]
    return np.where(fn(i, j), F(25.0), F(-25.0)).astype(F)


def _six_by_six(i, j):
    """Period 6 both ways with 25 land residues of 36: every 6 x 6 window holds each residue once, so exactly 25 land cells."""
    return (i % 6) * 6 + (j % 6) < 25


def _subnormal_plane():
    rng = np.random.default_rng(650)
    land = rng.random((19, 23)) < 0.5
    sea = np.array([-0.0, 0.0, -1e-40, np.nan], F)[rng.integers(0, 4, (19, 23))]
    return np.where(land, F(1e-40), sea).astype(F)


UP = float(np.nextafter(1.0, 2.0))
# name -> (builder of the (H, W) elevation in metres, half, fractions).  256 pixels to a block of the flag and scatter kernels, 1024 blocks to
# a round of the scan.
LAND_CASES = {
    "blocks_1024": (lambda: _seeded_land(512, 512, 1), 2, (0.5,)),                 # 262144 pixels: exactly one round
    "blocks_1025": (lambda: _seeded_land(5, 52429, 2), 2, (0.5,)),                 # 262145 pixels: one block into the second round; one row
    "blocks_2080": (lambda: _seeded_land(1024, 520, 3), 2, (0.5,)),                # three rounds: the carry is carried twice
    "no_rows": (lambda: _seeded_land(40, 130, 4), 20, (0.0,)),                     # 2 half == H: capacity 0
    "no_columns": (lambda: _seeded_land(130, 40, 5), 20, (0.0,)),                  # 2 half == W
    "one_row": (lambda: _seeded_land(41, 130, 6), 20, (0.0, 0.5)),
    "all_land": (lambda: np.full((23, 37), F(3.0)), 3, (1.0, UP, 0.0)),            # 1.0: idx full to capacity; above 1: none
    "all_sea": (lambda: np.full((23, 37), F(-3.0)), 3, (0.5, 0.0)),
    "seven_in_ten": (lambda: _pattern(70, 90, lambda i, j: np.mod(7 * i + 3 * j, 10) < 7), 5, (0.7,)),       # 70 of 100 in every window
    "twentyfive_in_36": (lambda: _pattern(70, 90, _six_by_six), 3, (25.0 / 36.0,)),
    "half_64_at_050": (lambda: _pattern(200, 260, lambda i, j: (i + j) % 4 < 2), 64, (0.5, float(np.nextafter(F(0.5), F(1))))),
    "half_64_at_075": (lambda: _pattern(200, 260, lambda i, j: (i + 3 * j) % 4 < 3), 64, (0.75, float(np.nextafter(F(0.75), F(1))))),
    "subnormal": (_subnormal_plane, 2, (0.5, 0.25)),
}
LAND_SMALL = ("no_rows", "no_columns", "one_row", "all_land", "all_sea", "seven_in_ten", "twentyfive_in_36", "subnormal")   # the literal double loop
LAND_ON_THE_BOUNDARY = (("seven_in_ten", 0.7), ("twentyfive_in_36", 25.0 / 36.0))          # exact fraction and fp32 mean disagree


@functools.lru_cache(maxsize=None)
def land_plane(name):
    out = LAND_CASES[name][0]()
    out.flags.writeable = False
    return out


def land_capacity(shape, half):
    return 0 if half == 0 else (shape[0] - 2 * half) * (shape[1] - 2 * half)
