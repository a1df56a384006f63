"""NumPy-only restatement of the reference's hydrology (d8_flow, flow_accumulation, plot_flow_indicator, fill_depressions_priority_flood with
max_raise None) and the seeded canvases the hydrology tests use.  Written from the definitions, not from the reference's or the product's code:
  * d8: the eight fp32 slopes with edge padding, ocean handling and numpy's first-maximum argmax, vectorised;
  * fill: the fixed point d(c) = h(c) > m(c) ? h(c) : fl32(m(c) + fl32(eps)) relaxed from +inf by Jacobi sweeps (seeds keep h), which is
    the Priority-Flood+eps result for eps >= 0;
  * accumulation: a recurrence check, O(N) with np.bincount at any size -- A is exact when A[v] == 1 + the sum of A over v's donors on every
    valid cell and 0 elsewhere -- and, for small canvases, the counts themselves in descending-elevation order.
It gives expected values at sizes tests/golden/hydro.npz cannot hold."""
import numpy as np

from _relief_twin import land_and_sea  # noqa: F401  (the same seeded canvases as the relief tests)

DY = np.array([-1, 1, 0, 0, -1, -1, 1, 1])
DX = np.array([0, 0, -1, 1, -1, 1, -1, 1])
SQRT2_F32 = np.float32(np.sqrt(2.0))


def rugged(H, W, seed, sea=0.2):
    """land_and_sea with pits, a plateau, NaN holes and a valid region enclosed by NaN: the cases that exercise every branch."""
    e = land_and_sea(H, W, seed, sea=sea)
    rng = np.random.default_rng(seed + 1)
    land = np.argwhere(e > 50)
    for y, x in land[rng.choice(len(land), size=max(1, H * W // 400), replace=False)]:
        e[y, x] = np.float32(max(1.0, float(e[y, x]) - 300.0))          # single-cell pits
    py, px = H // 3, W // 2
    e[py:py + max(1, H // 8), px:px + max(1, W // 8)] = np.float32(e.max() * 0.6 + 1.0)   # plateau
    e[H // 5:H // 5 + 3, W // 7:W // 7 + 4] = np.nan                       # NaN hole
    y0, x0 = (2 * H) // 3, W // 5
    s = max(5, min(H, W) // 8)
    if y0 + s < H and x0 + s < W:                                          # NaN ring around a land block
        e[y0:y0 + s, x0:x0 + s] = np.nan
        e[y0 + 1:y0 + s - 1, x0 + 1:x0 + s - 1] = np.float32(400.0) + np.arange((s - 2) * (s - 2), dtype=np.float32).reshape(s - 2, s - 2) % 7
    return e


def neighbours(a, dy, dx, fill=None):
    """a[clamp(i + dy), clamp(j + dx)] (edge padding) or, with fill, `fill` outside the image."""
    H, W = a.shape
    if fill is None:
        yi = np.clip(np.arange(H) + dy, 0, H - 1)
        xi = np.clip(np.arange(W) + dx, 0, W - 1)
        return a[yi[:, None], xi[None, :]]
    p = np.pad(a, 1, mode="constant", constant_values=fill)
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def _argmax_first(stack):
    """numpy's argmax along axis 0 (first maximum; a NaN wins at once) and the value there."""
    best = stack[0].copy()
    k = np.zeros(best.shape, np.int64)
    for i in range(1, stack.shape[0]):
        take = ~np.isnan(best) & ~(stack[i] <= best)
        best = np.where(take, stack[i], best)
        k = np.where(take, i, k)
    return k, best


def d8(z, tol=1e-3):
    """(receiver flat int64, kmax int64, is_sink bool) of fp32 z."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    with np.errstate(invalid="ignore", over="ignore"):
        nb = np.stack([neighbours(z, DY[k], DX[k]) for k in range(8)])
        dist = np.array([1, 1, 1, 1] + [SQRT2_F32] * 4, np.float32)[:, None, None]
        s = (z[None] - nb) / dist
        s = np.where(s < np.float32(tol), np.float32(-np.inf), s)
        co = ~(z > 0)
        no = ~(nb > 0)
        prefer = np.where(co[None], -np.inf, np.where(no, np.inf, s)).astype(np.float32)
        ignore = np.where(co[None] | no, -np.inf, s).astype(np.float32)
    k, _ = _argmax_first(prefer)
    _, mi = _argmax_first(ignore)
    sink = co | (~no.any(axis=0) & ~np.isfinite(mi))
    rr = np.clip(np.arange(H)[:, None] + DY[k], 0, H - 1)
    cc = np.clip(np.arange(W)[None, :] + DX[k], 0, W - 1)
    return rr * W + cc, k, sink


def counted_edges(z, receiver, sink):
    """(source, receiver) flat indices of the edges the reference's accumulation adds along."""
    zf = np.asarray(z, np.float32).ravel()
    r = np.asarray(receiver).ravel()
    valid = zf > 0
    src = np.flatnonzero(valid & ~np.asarray(sink).ravel())
    ok = valid[r[src]]
    return src[ok], r[src[ok]]


def uphill_edges(z, receiver, sink):
    zf = np.asarray(z, np.float32).ravel()
    s, r = counted_edges(z, receiver, sink)
    return int(np.count_nonzero(~(zf[r] < zf[s])))


def accumulation_ok(z, receiver, sink, A):
    """The recurrence check: A == 1 + sum of A over the donors on valid cells, 0 on the others (exact, float64 sums of integers)."""
    zf = np.asarray(z, np.float32).ravel()
    a = np.asarray(A, np.float64).ravel()
    valid = zf > 0
    s, r = counted_edges(z, receiver, sink)
    inflow = np.bincount(r, weights=a[s], minlength=zf.size)
    return bool(np.all(a[~valid] == 0) and np.all(a[valid] == 1.0 + inflow[valid]))


def accumulate(z, receiver, sink):
    """Upstream counts in descending-elevation order (small canvases)."""
    zf = np.asarray(z, np.float32).ravel()
    A = (zf > 0).astype(np.float64)
    s, r = counted_edges(z, receiver, sink)
    nxt = np.full(zf.size, -1)
    nxt[s] = r
    for c in s[np.argsort(-zf[s], kind="stable")]:
        A[nxt[c]] += A[c]
    return A.astype(np.float32).reshape(np.shape(z))


def indicator(A, k=1):
    A = np.asarray(A, np.float32)
    if k > 1:
        Ho, Wo = A.shape[0] // k, A.shape[1] // k
        A = A[:Ho * k, :Wo * k].reshape(Ho, k, Wo, k).max(axis=(1, 3))
    return np.log1p(A)


def _invalid(h, nodata):
    inv = ~(h > 0)
    if nodata is not None:
        inv |= h == np.float32(nodata)
    return inv


def _seeds(inv, conn):
    H, W = inv.shape
    border = np.zeros_like(inv)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    ks = range(4) if conn == 4 else range(8)
    near = np.zeros_like(inv)
    for k in ks:
        near |= neighbours(inv, DY[k], DX[k], fill=False)
    return ~inv & (border | near)


def _g(d, h, eps, conn):
    ks = range(4) if conn == 4 else range(8)
    m = np.full(d.shape, np.inf, np.float32)
    for k in ks:
        m = np.minimum(m, neighbours(d, DY[k], DX[k], fill=np.float32(np.inf)))
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(h > m, h, m + np.float32(eps)).astype(np.float32)
    return np.where(np.isinf(m), np.float32(np.inf), g)


def fill(h, epsilon=1e-3, connectivity=8, nodata=None, max_iter=100000):
    """(filled fp32, Jacobi iterations) by relaxation from +inf."""
    h = np.asarray(h, np.float32)
    conn = 4 if connectivity == 4 else 8
    inv = _invalid(h, nodata)
    seed = _seeds(inv, conn)
    free = ~inv & ~seed
    d = np.where(seed, h, np.float32(np.inf)).astype(np.float32)
    for it in range(1, max_iter + 1):
        new = np.where(free, np.minimum(d, _g(d, h, epsilon, conn)), d)
        if np.array_equal(new, d):
            break
        d = new
    return np.where(inv, h, d).astype(np.float32), it


def fill_fixed_point_violations(h, d, epsilon=1e-3, connectivity=8, nodata=None):
    """Number of cells of d that break the fill's equations (seeds and invalid cells keep h, the others d = G(d)) or are left at +inf."""
    h = np.asarray(h, np.float32)
    d = np.asarray(d, np.float32)
    conn = 4 if connectivity == 4 else 8
    inv = _invalid(h, nodata)
    seed = _seeds(inv, conn)
    free = ~inv & ~seed
    dd = np.where(inv, np.float32(np.inf), d)
    bad = (inv & ~((d == h) | (np.isnan(d) & np.isnan(h)))) | (seed & (d != h)) | (free & (d != _g(dd, h, epsilon, conn)))
    bad |= ~inv & np.isinf(d) & ~np.isinf(h)
    return int(np.count_nonzero(bad))
