"""Closed-form fp32 terrains whose topology, not whose roughness, drives the hydrology kernels' iterative and order-dependent paths: one-cell
channels that wind through every tile (the fill's sweep cap, its batches of passes, tiles going idle and waking), one downhill chain of
thousands of cells and a trunk with many walkers (the accumulation walk), and integer surfaces on which most d8 slopes tie or meet tol exactly.
NumPy only, no randomness.  tests/golden/hydro_structured.npz records the reference's results on them."""
import numpy as np


def serpentine_path(H, W):
    """(rows, cols) of the channel from its outlet end (1, 1): odd rows 1, 3, ... < H - 1 over columns 1 .. W - 2, joined through one cell of
    the wall row between them, at column W - 2 and column 1 in turn."""
    rows, cols = [], []
    right = True                                   # the direction the current row is walked in
    for r in range(1, H - 1, 2):
        js = range(1, W - 1) if right else range(W - 2, 0, -1)
        rows += [r] * (W - 2)
        cols += list(js)
        if r + 2 < H - 1:
            rows.append(r + 1)
            cols.append(W - 2 if right else 1)
        right = not right
    return np.array(rows), np.array(cols)


def serpentine(H, W, outlet=10.0, floor=1.0, wall=1000.0):
    """A one-cell-wide depression at `floor` between walls, draining only through z[1, 0] = outlet along about H / 2 * W cells."""
    z = np.full((H, W), wall, np.float32)
    z[serpentine_path(H, W)] = np.float32(floor)
    z[1, 0] = np.float32(outlet)
    return z


def ramp_serpentine(H, W):
    """The same path as one downhill chain: 2 + 0.5 d at distance d from its start, walls of 5000, the sea (-1) at z[1, 0]."""
    z = np.full((H, W), 5000.0, np.float32)
    r, c = serpentine_path(H, W)
    z[r, c] = (2.0 + 0.5 * np.arange(len(r))).astype(np.float32)
    z[1, 0] = np.float32(-1.0)
    return z


def _ij(n):
    c = n // 2
    i, j = np.mgrid[0:n, 0:n]
    return i, j, np.abs(i - c), np.abs(j - c)


def pit_l1(n):
    _, _, a, b = _ij(n)
    return (1 + a + b).astype(np.float32)


def pit_linf(n):
    _, _, a, b = _ij(n)
    return (1 + np.maximum(a, b)).astype(np.float32)


def peak_linf_sea(n):
    _, _, a, b = _ij(n)
    z = (40 - np.maximum(a, b)).astype(np.float32)
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = np.float32(-1.0)
    return z


def saddle(n):
    _, _, a, b = _ij(n)
    return (50 + a * a - b * b).astype(np.float32)


def steps(n):
    """Used with tol = 0.5: a cardinal step down is a slope of exactly tol, a diagonal one 0.5 / sqrt 2 falls below it."""
    i, j, _, _ = _ij(n)
    return (1 + 0.5 * ((i + j) // 3)).astype(np.float32)


def checkerboard(n):
    i, j, _, _ = _ij(n)
    return (1 + (i + j) % 2).astype(np.float32)


def flat(n):
    return np.full((n, n), 7.0, np.float32)


def plane(n):
    i, j, _, _ = _ij(n)
    return (1 + i + 2 * j).astype(np.float32)


TIE_SURFACES = {"pit_l1": pit_l1, "pit_linf": pit_linf, "peak_linf_sea": peak_linf_sea, "saddle": saddle, "steps": steps,
                "checkerboard": checkerboard, "flat": flat, "plane": plane}


def comb(H=40, W=70):
    """Teeth (the even columns, between ridges 500 higher) that run down to one trunk row, which runs along the bottom into the sea."""
    i, j = np.mgrid[0:H, 0:W]
    z = (200 - 2 * i).astype(np.float32)
    z[:, 1::2] += np.float32(500.0)
    z[H - 2, :] = (100 - np.arange(W)).astype(np.float32)
    z[H - 1, :] = np.float32(900.0)
    z[:, W - 1] = np.float32(-5.0)
    return z


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Measures of what an input exercises, from the input and recorded results alone.

def tie_fraction(z, tol=1e-3):
    """Fraction of the land cells whose largest `prefer` slope (d8's: below tol -> -inf, into an ocean neighbour -> +inf) is attained at two
    or more of the eight neighbours."""
    import _hydro_twin as twin
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        nb = np.stack([twin.neighbours(z, twin.DY[k], twin.DX[k]) for k in range(8)])
        dist = np.array([1, 1, 1, 1] + [twin.SQRT2_F32] * 4, np.float32)[:, None, None]
        s = (z[None] - nb) / dist
        s = np.where(s < np.float32(tol), np.float32(-np.inf), s)
        prefer = np.where(~(nb > 0), np.float32(np.inf), s)
    land = z > 0
    tied = (prefer == prefer.max(axis=0)[None]).sum(axis=0) >= 2
    return float(np.count_nonzero(tied & land)) / max(1, int(np.count_nonzero(land)))


def longest_chain(z, receiver, sink):
    """Counted edges on the longest path of the receiver forest (the steps one walker can take), and the largest number of donors of a cell."""
    import _hydro_twin as twin
    zf = np.asarray(z, np.float32).ravel()
    s, r = twin.counted_edges(z, receiver, sink)
    nxt = np.full(zf.size, -1)
    nxt[s] = r
    depth = np.zeros(zf.size, np.int64)               # edges on the longest path that ends in the cell
    for c in s[np.argsort(-zf[s], kind="stable")]:     # donors before receivers
        depth[nxt[c]] = max(depth[nxt[c]], depth[c] + 1)
    fan_in = np.bincount(r, minlength=zf.size)
    return int(depth.max()), int(fan_in.max())
