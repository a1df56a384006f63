"""NumPy-only restatement of the Minecraft terrain path (the reference's minecraft_api.py: _get_upsampled, _compute_climate_vars,
_classify_biome, _binary_response; api.py: _get_terrain) in the arithmetic order of mc_csrc/mc_kernels.hip, so that it reproduces the GPU bit
for bit (the growing season's asin to the rounding of a float64 asin):
  * noise: FastNoiseLite's Perlin FBm structure (hash primes, quintic fade, 1.4247691104677813 gain, fractal bounding, weighted strength 0,
    seed + 1 per octave) over a 128-entry gradient table rounded to fp32 from float64 angles -- this package's own values, not FastNoiseLite's;
  * upsample: torch's bilinear index and weight formula (align_corners=False, scale_factor = s), evaluated per output pixel, the source
    index as one fused multiply-add (as torch's CPU build has it) and the weighted sum in float64, rounded once;
  * Sobel: ((a02 - a00) + 2 (a12 - a10)) + (a22 - a20), times 1/8, the centre tap only propagating NaN;
  * pow(1.5) as fl32(x sqrt(x)) in float64, asin as fl32(asin(float64)), every other operation in fp32 in the reference's order.
margin() gives, per pixel, how close the classifier's decisions were: the smallest distance, in ulps, of a decision quantity to its threshold.
It gives expected values at sizes tests/golden/mc.npz cannot hold, and it is what tests/golden/make_mc_golden.py feeds the reference as noise."""
import numpy as np

F = np.float32
# the reference's seven generators (minecraft_api.py), in its order: (name, seed, frequency, octaves, gain); lacunarity 2 everywhere
GENERATORS = (
    ("_TEMP_NOISE", 12345, 1.0 / 500.0, 3, 0.5),
    ("_TEMP_NOISE_FINE", 54321, 1.0 / 128.0, 2, 0.5),
    ("_PRECIP_NOISE", 12345, 1.0 / 500.0, 5, 0.5),
    ("_SNOW_NOISE", 12345, 1.0 / 500.0, 3, 0.5),
    ("_SNOW_NOISE_FINE", 54321, 1.0 / 128.0, 2, 0.5),
    ("_ELEV_NOISE_COARSE", 99999, 1.0 / 24.0, 3, 0.5),
    ("_ELEV_NOISE_FINE", 88888, 1.0 / 6.0, 2, 0.6),
)
NAMES = tuple(g[0] for g in GENERATORS)
PLAINS = 1
BIOME_IDS = (1, 3, 5, 6, 8, 15, 16, 17, 19, 23, 31, 32, 33, 35, 41, 44, 46, 48, 108, 115, 116)

_ANG = np.arange(128, dtype=np.float64) * (2.0 * np.pi / 128.0) + np.pi / 128.0
GRAD_X = np.cos(_ANG).astype(F)
GRAD_Y = np.sin(_ANG).astype(F)
PRIME_X, PRIME_Y, HASH_MUL = 501125321, 1136930381, 0x27D4EB2D


# ---------------------------------------------------------------------------------------------------------------------------------- noise
def _grad(seed, xp, yp, xd, yd):
    h = (np.uint32(seed) ^ xp ^ yp) * np.uint32(HASH_MUL)
    k = (h ^ (h >> np.uint32(15))) & np.uint32(127)
    return xd * GRAD_X[k] + yd * GRAD_Y[k]


def perlin(seed, x, y):
    """One octave of 2-D Perlin noise at fp32 coordinates (already multiplied by the frequency)."""
    fx, fy = np.floor(x), np.floor(y)
    xd0, yd0 = x - fx, y - fy
    xd1, yd1 = xd0 - F(1), yd0 - F(1)
    xs = xd0 * xd0 * xd0 * (xd0 * (xd0 * F(6) - F(15)) + F(10))
    ys = yd0 * yd0 * yd0 * (yd0 * (yd0 * F(6) - F(15)) + F(10))
    x0 = fx.astype(np.int64).astype(np.uint32) * np.uint32(PRIME_X)
    y0 = fy.astype(np.int64).astype(np.uint32) * np.uint32(PRIME_Y)
    x1, y1 = x0 + np.uint32(PRIME_X), y0 + np.uint32(PRIME_Y)
    a, b = _grad(seed, x0, y0, xd0, yd0), _grad(seed, x1, y0, xd1, yd0)
    c, d = _grad(seed, x0, y1, xd0, yd1), _grad(seed, x1, y1, xd1, yd1)
    xf0 = a + xs * (b - a)
    xf1 = c + xs * (d - c)
    return (xf0 + ys * (xf1 - xf0)) * F(1.4247691104677813)


def bounding(octaves, gain):
    g = F(abs(gain))
    amp, total = g, F(1)
    for _ in range(1, octaves):
        total = total + amp
        amp = amp * g
    return F(1) / total


def fbm(seed, frequency, octaves, gain, coords, cache=None):
    """FBm of `octaves` octaves at coords (2, N) fp32 (x = column, y = row) -> (N,) fp32.  `cache` shares single octaves between generators
    with the same seed and frequency (their values are the same)."""
    c = np.asarray(coords, F)
    x, y = c[0] * F(frequency), c[1] * F(frequency)
    amp, g = bounding(octaves, gain), F(gain)
    total = np.zeros(x.shape, F)
    for o in range(octaves):
        key = (seed + o, F(frequency), o)
        if cache is None or key not in cache:
            v = perlin(seed + o, x, y)
            if cache is not None:
                cache[key] = v
        else:
            v = cache[key]
        total = total + v * amp
        x, y = x * F(2), y * F(2)
        amp = amp * g
    return total


def coords(i0, j0, H, W):
    """The reference's coordinate array: x = absolute column, y = absolute row, fp32, row-major (2, H W)."""
    xx, yy = np.meshgrid(np.arange(j0, j0 + W, dtype=F), np.arange(i0, i0 + H, dtype=F))
    return np.array([xx.ravel(), yy.ravel()], dtype=F)


def generate(name, c, cache=None):
    _, seed, freq, octs, gain = GENERATORS[NAMES.index(name)]
    return fbm(seed, freq, octs, gain, c, cache)


def noise_planes(i0, j0, H, W):
    """The seven built-in noise planes (7, H, W) for the box at absolute (i0, j0), in the reference's generator order."""
    c = coords(i0, j0, H, W)
    cache = {}
    return np.stack([generate(n, c, cache).reshape(H, W) for n in NAMES])


# ------------------------------------------------------------------------------------------------------------------------------ upsample
def _axis(n_in, s, start, n):
    u = np.arange(start, start + n, dtype=np.int64)
    if s == 1:
        return u, u, np.ones(n, F), np.zeros(n, F)
    # fma(fl32(1 / s), u + 0.5, -0.5), as torch's CPU build contracts it: the float64 product of two floats is exact, so is the subtraction
    real = (np.float64(F(1.0 / s)) * (u.astype(F) + F(0.5)).astype(np.float64) - 0.5).astype(F)
    real = np.where(real < F(0), F(0), real).astype(F)
    i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    l1 = np.minimum(np.maximum(real - i0.astype(F), F(0)), F(1)).astype(F)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, F(1) - l1, l1


def upsample(src, s, r0, c0, H, W):
    """Rows [r0, r0 + H) x columns [c0, c0 + W) of F.interpolate(src, scale_factor=s, mode='bilinear', align_corners=False) for src (Hn, Wn)
    or (C, Hn, Wn), fp32."""
    if s == 1:                                   # torch copies when the sizes agree
        return np.asarray(src, F)[..., r0:r0 + H, c0:c0 + W].copy()
    x = np.asarray(src, F).astype(np.float64)
    a, b, h0, h1 = _axis(x.shape[-2], s, r0, H)
    c, d, w0, w1 = _axis(x.shape[-1], s, c0, W)
    h0, h1 = h0[:, None].astype(np.float64), h1[:, None].astype(np.float64)
    w0, w1 = w0.astype(np.float64), w1.astype(np.float64)
    top = w0 * x[..., a[:, None], c[None, :]] + w1 * x[..., a[:, None], d[None, :]]
    bot = w0 * x[..., b[:, None], c[None, :]] + w1 * x[..., b[:, None], d[None, :]]
    return (h0 * top + h1 * bot).astype(F)


# ------------------------------------------------------------------------------------------------------------------------- Sobel, detail
def gradient(padded):
    """sqrt(dx^2 + dy^2) of the 3x3 Sobel / 8 of padded (H + 2, W + 2) -> (H, W) fp32; NaN wherever the 3x3 window holds one."""
    p = np.asarray(padded, F)
    a = lambda r, c: p[r:p.shape[0] - 2 + r, c:p.shape[1] - 2 + c]
    gx = ((a(0, 2) - a(0, 0)) + (a(1, 2) - a(1, 0)) * F(2)) + (a(2, 2) - a(2, 0))
    gy = ((a(2, 0) - a(0, 0)) + (a(2, 1) - a(0, 1)) * F(2)) + (a(2, 2) - a(0, 2))
    dx, dy = gx * F(0.125), gy * F(0.125)
    return np.sqrt(dx * dx + dy * dy) + F(0) * a(1, 1)


def _clamp01(x):
    return np.where(x < F(0), F(0), np.where(x > F(1), F(1), x)).astype(F)


def pow15(x):
    d = np.asarray(x, np.float64)
    return (d * np.sqrt(d)).astype(F)


def detail(elev_smooth, grad, n_coarse, n_fine, noise_scale, pixel_size_m, native_resolution):
    """_get_upsampled's noise step: elev = elev_smooth + (n_coarse amp_coarse + n_fine amp_fine) * (elev_smooth >= 0)."""
    sf = pow15(_clamp01(grad / F(40.0 * pixel_size_m / 90.0)))
    amp_c = sf * F(noise_scale * 100.0) * F(pixel_size_m) / F(native_resolution)
    amp_f = sf * F(noise_scale * 70.0) * F(pixel_size_m) / F(native_resolution)
    land = (elev_smooth >= F(0)).astype(F)
    return (elev_smooth + (n_coarse * amp_c + n_fine * amp_f) * land).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------- classifier
def climate_vars(temp, t_season, precip, p_cv):
    """_compute_climate_vars in fp32: (tree_moisture, growing_season, x, coldest_month, tropical, t_std)."""
    t_std = t_season / F(100.0)
    t_eff = temp + F(0.5) * t_std
    t_eff = np.where(t_eff < F(0), F(0), t_eff).astype(F)
    pet = F(250.0) + F(25.0) * t_eff + F(0.7) * (t_eff * t_eff)
    pet = np.where(pet < F(250.0), F(250.0), pet).astype(F)
    pet1 = np.where(pet < F(1), F(1), pet).astype(F)
    aridity = precip / pet1
    pc = p_cv / F(100.0)
    pc = np.where(pc > F(1), F(1), pc).astype(F)
    tree_moisture = aridity * (F(1) - F(0.35) * pc)
    amplitude = t_std * F(1.414)
    amplitude = np.where(amplitude < F(0.1), F(0.1), amplitude).astype(F)
    x = (F(5.0) - temp) / amplitude
    xc = np.where(x < F(-1), F(-1), np.where(x > F(1), F(1), x)).astype(F)
    asin = np.arcsin(xc.astype(np.float64)).astype(F)
    gs = F(365.0) * (F(0.5) - asin / F(3.14159))
    gs = np.where(x <= F(-1), F(365.0), np.where(x >= F(1), F(0), gs)).astype(F)
    coldest = temp - F(2.0) * t_std
    tropical = (temp >= F(18.0)) & (t_std < F(5.0))
    return tree_moisture.astype(F), gs, x.astype(F), coldest.astype(F), tropical, t_std.astype(F)


def _quantities(elev, climate, grad, pixel_size_m, planes):
    e = np.asarray(elev, F)
    temp = np.asarray(climate[0], F)
    t_season = np.asarray(climate[1], F)
    precip = np.asarray(climate[2], F)
    precip = np.where(precip < F(0), F(0), precip).astype(F)
    p_cv = np.asarray(climate[3], F)
    n = np.asarray(planes, F)
    temp = temp + (F(0.4) * n[0] + F(0.2) * n[1])
    precip = precip * (F(1.0) + F(0.2) * n[2])
    snow_noise = F(3.0) * n[3] + F(2.0) * n[4]
    tm, gs, x, _, tropical, t_std = climate_vars(temp, t_season, precip, p_cv)
    sr = grad / F(pixel_size_m)
    gsf = _clamp01((gs - F(60.0)) / F(90.0))
    eff = tm * gsf
    mf = _clamp01((tm - F(0.35)) / F(0.45))
    bt = F(0.7) + F(1.19 - 0.7) * mf
    return dict(e=e, temp=temp, precip=precip, snow_temp=temp + snow_noise, tm=tm, gs=gs, x=x, tropical=tropical, t_std=t_std, sr=sr, eff=eff,
                bt=bt)


def classify(elev, climate, grad, pixel_size_m, planes):
    """_classify_biome -> int16 (H, W).  grad: gradient() of elev_padded; planes: the seven noise planes (only 0..4 are read)."""
    e = np.asarray(elev, F)
    if climate is None or climate.shape[0] < 4:
        return np.full(e.shape, PLAINS, np.int16)
    q = _quantities(e, climate, grad, pixel_size_m, planes)
    temp, precip, tm, gs, eff, sr, bt = q["temp"], q["precip"], q["tm"], q["gs"], q["eff"], q["sr"], q["bt"]
    is_steep = sr > F(0.78)
    trees_none = eff < F(0.2)
    barren = (tm < F(0.05)) | (gs < F(60.0))
    sparse = ~trees_none & (eff < F(0.5))
    forest = ~trees_none & (eff >= F(0.5)) & (eff < F(0.8))
    dense = ~trees_none & (eff >= F(0.8)) & (eff < F(1.3))
    rain = ~trees_none & (eff >= F(1.3))
    medium = (sr >= F(0.62)) & (sr < bt)
    bare = sr >= bt
    had = forest | dense | rain
    sparse = sparse | (medium & had)
    forest, dense, rain = forest & ~medium, dense & ~medium, rain & ~medium
    trees_none = trees_none | bare
    sparse, forest, dense, rain = sparse & ~bare, forest & ~bare, dense & ~bare, rain & ~bare
    snow = (q["snow_temp"] < F(0)) & (precip > F(150.0)) & ~is_steep
    alt = np.where(e < F(0), F(0), e)
    ocean, mountains, lowland = e < F(0), alt > F(2500.0), alt < F(200.0)
    frozen = temp < F(-5.0)
    cold = (temp >= F(-5.0)) & (temp < F(5.0))
    cool = (temp >= F(5.0)) & (temp < F(12.0))
    temperate = (temp >= F(12.0)) & (temp < F(20.0))
    warm = (temp >= F(20.0)) & (temp < F(26.0))
    hot = temp >= F(26.0)
    steppe_dry = (tm < F(0.35)) | (precip < F(350))
    out = np.full(e.shape, PLAINS, np.int16)

    def put(m, v):
        out[m] = v
    of, oc, ow = ocean & frozen, ocean & cold & ~frozen, ocean & (warm | hot)
    put(of, 48); put(oc, 46); put(ow, 41); put(ocean & ~of & ~oc & ~ow, 44)
    mtn = mountains & ~ocean
    put(mtn & bare & snow, 33); put(mtn & bare & ~snow, 35)
    soil = mtn & ~bare
    put(soil & snow & trees_none, 32); put(soil & snow & (sparse | forest), 116); put(soil & snow & (dense | rain), 16)
    put(soil & ~snow & trees_none & barren, 19)
    mcs = soil & ~snow & trees_none & ~barren & steppe_dry
    put(mcs, 31); put(soil & ~snow & trees_none & ~barren & ~mcs, 1)
    put(soil & ~snow & (sparse | forest), 115); put(soil & ~snow & (dense | rain), 15)
    land = ~ocean & ~mtn
    sb = land & snow & trees_none
    put(sb, 3); land = land & ~sb
    sfs, sfd = land & snow & (sparse | forest), land & snow & (dense | rain)
    put(sfs, 116); put(sfd, 16); land = land & ~(sfs | sfd)
    db = land & ~snow & trees_none
    desert = db & (warm | hot)
    ws = db & (cold | cool | temperate) & ~lowland & barren
    cs = db & steppe_dry & ~barren
    put(desert, 5); put(ws, 31); put(cs, 31); put(db & ~desert & ~ws & ~cs, 1); land = land & ~db
    sfl = land & ~snow & (sparse | forest)
    put(sfl & hot, 23); put(sfl & warm & sparse & ~medium, 17); put(sfl & warm & forest, 108); put(sfl & temperate, 108)
    put(sfl & (cool | cold), 115); land = land & ~sfl
    dl = land & ~snow & dense
    jd, sw = dl & hot, dl & warm & lowland
    td = dl & (cool | cold) & ~jd & ~sw
    put(jd, 23); put(sw, 6); put(td, 15); put(dl & ~jd & ~sw & ~td, 8); land = land & ~dl
    rl = land & ~snow & rain
    jr = rl & (hot | (warm & q["tropical"]))
    sr_ = rl & ~jr & lowland
    tr = rl & (cool | cold) & ~jr & ~sr_
    put(jr, 23); put(sr_, 6); put(tr, 15); put(rl & ~jr & ~sr_ & ~tr, 8); land = land & ~rl
    put(land, 1)
    lb = bare & ~ocean & ~mountains
    put(lb & snow, 33); put(lb & ~snow, 35)
    return out


def _ord(x):
    b = np.asarray(x, F).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def ulp_distance(a, b):
    """|a - b| in units in the last place of fp32 (the number of floats between them); NaN gives a huge distance."""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    d = np.abs(_ord(a) - _ord(b))
    return np.where(np.isnan(a) | np.isnan(b), np.int64(1) << 40, d)


def margin(elev, climate, grad, pixel_size_m, planes):
    """Per pixel, the smallest distance in ulps of any decision quantity of classify() to its threshold (huge where climate is absent)."""
    e = np.asarray(elev, F)
    if climate is None or climate.shape[0] < 4:
        return np.full(e.shape, np.int64(1) << 40)
    q = _quantities(e, climate, grad, pixel_size_m, planes)
    checks = [("e", (0.0, 200.0, 2500.0)), ("temp", (-5.0, 5.0, 12.0, 18.0, 20.0, 26.0)), ("t_std", (5.0,)), ("precip", (150.0, 350.0)),
              ("tm", (0.05, 0.35)), ("eff", (0.2, 0.5, 0.8, 1.3)), ("gs", (60.0,)), ("x", (-1.0, 1.0)), ("sr", (0.62, 0.78)),
              ("snow_temp", (0.0,))]
    m = np.full(e.shape, np.int64(1) << 40)
    for k, ts in checks:
        for t in ts:
            m = np.minimum(m, ulp_distance(q[k], F(t)))
    return np.minimum(m, ulp_distance(q["sr"], q["bt"]))


# ------------------------------------------------------------------------------------------------------------------------------- payload
def payload(elev, biome=None):
    """_binary_response's body: clip(floor(elev), -32768, 32767) as int16-le (NaN written as 0), then the biome ids as int16-le."""
    e = np.asarray(elev, F)
    f = np.clip(np.floor(e), F(-32768), F(32767))
    body = np.where(np.isnan(f), F(0), f).astype("<i2").tobytes()
    if biome is not None:
        body += np.asarray(biome).astype("<i2").tobytes()
    return body


# ------------------------------------------------------------------------------------------------------------------------ request flows
def native_box(i1, j1, i2, j2, scale, pad):
    """The native window a scaled request reads: floor / ceil division as Python does it, padded by `pad` native pixels."""
    return i1 // scale - pad, j1 // scale - pad, -(-i2 // scale) + pad, -(-j2 // scale) + pad


def get_upsampled(elev_native, climate_native, i1, j1, i2, j2, scale, noise_scale, pixel_size_m, native_resolution, planes):
    """_get_upsampled over the native window world.get returned for native_box(..., pad=2)."""
    H, W = i2 - i1, j2 - j1
    r0 = 2 * scale + (i1 - (i1 // scale) * scale)
    c0 = 2 * scale + (j1 - (j1 // scale) * scale)
    padded = upsample(elev_native, scale, r0 - 1, c0 - 1, H + 2, W + 2)
    smooth = padded[1:-1, 1:-1]
    clim = None if climate_native is None else upsample(climate_native, scale, r0, c0, H, W)
    elev = smooth
    if noise_scale > 0:
        elev = detail(smooth, gradient(padded), planes[5], planes[6], noise_scale, pixel_size_m, native_resolution)
    return {"elev": elev, "elev_smooth": smooth, "climate": clim, "elev_padded": padded}


def get_terrain(elev_native, climate_native, i1, j1, i2, j2, scale):
    """api.py's _get_terrain (scale > 1) over the native window for native_box(..., pad=1)."""
    H, W = i2 - i1, j2 - j1
    r0 = scale + (i1 - (i1 // scale) * scale)
    c0 = scale + (j1 - (j1 // scale) * scale)
    return {"elev": upsample(elev_native, scale, r0, c0, H, W),
            "climate": None if climate_native is None else upsample(climate_native, scale, r0, c0, H, W)}


def minecraft_terrain(windows, i1, j1, i2, j2, scale, noise_scale, native_resolution, planes):
    """(elev, biome) of a /terrain request.  windows: what world.get returned, as (elev, climate) pairs -- at scale 1 the padded box without
    climate, then the box itself; otherwise the one padded native window."""
    if scale == 1:
        (padded, _), (elev, climate) = windows
        return np.asarray(elev, F), classify(elev, climate, gradient(padded), native_resolution, planes)
    en, cn = windows[0]
    pix = native_resolution / scale
    up = get_upsampled(en, cn, i1, j1, i2, j2, scale, noise_scale, pix, native_resolution, planes)
    return up["elev"], classify(up["elev_smooth"], up["climate"], gradient(up["elev_padded"]), pix, planes)


def upsample_scale(src, s, r0, c0, H, W):
    """Per output pixel of upsample(), the largest magnitude of the (up to) four native samples it interpolates: the scale of its rounding
    error (a lerp across 0 cancels, so the output itself is no measure)."""
    x = np.abs(np.asarray(src, F))
    a, b, _, _ = _axis(x.shape[-2], s, r0, H)
    c, d, _, _ = _axis(x.shape[-1], s, c0, W)
    m = np.maximum(x[..., a[:, None], c[None, :]], x[..., a[:, None], d[None, :]])
    return np.maximum(m, np.maximum(x[..., b[:, None], c[None, :]], x[..., b[:, None], d[None, :]]))


def crop_origin(i1, j1, scale, pad):
    """Row / column of the request's first pixel in the upsampled native window (pad native pixels of padding)."""
    return pad * scale + (i1 - (i1 // scale) * scale), pad * scale + (j1 - (j1 // scale) * scale)
