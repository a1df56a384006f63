"""Training items on the GPU: the last link of the reference's data chain, DEM -> base dataset -> encoded dataset -> beauty scores -> items.

The reference builds one item at a time on the CPU in its three dataset classes (terrain_diffusion/training/datasets/): an HDF5 read, flips and
rotations, a 160 x 160 window reduced to 32 x 32 block means and a 5 % np.quantile, a latent reparameterisation, then a host-to-device copy.
Here the planes of every selected group are uploaded once (DeviceGroups) and stay resident; a batch of items is a fixed handful of launches of
libtd_batch.so (include/td_batch.h, batch_csrc/) on the engine's stream.  There is no CPU fallback.

  device forms   views, sample_latents, cond_image, cond_vector: tensors in and out over a DeviceGroups and an item table;
  host planners  the .plan_item() of each class: the torch.Generator draws of the reference's __getitem__ in its order, sizes and dtypes (the
                 decoder's randn is fp16), so that a seeded sequence picks the same groups, crops, transforms and noise;
  drop-ins       H5LatentsDataset, H5DecoderTerrainDataset, H5AutoencoderDataset: the reference's constructor arguments, dict keys, dtypes and
                 shapes, with the tensors on the device.  h5_file is any mapping shaped like the HDF5 file -- res / chunk / subchunk /
                 {latent, lowfreq, lowres_exact, climate, residual} with .attrs, an open h5py.File included; h5py is not required.

__getitem__ consumes the generator exactly as the reference does.  The last draw of a latents item has as many normals as the item has NaN
climate centres, which depends on the data: __getitem__ reads the four flags back first, one 16-byte read-back per item.  get_batch(n) builds
n items in one set of launches and always draws four replacement normals per item, so ITS STREAM OF DRAWS IS ITS OWN: a seeded get_batch does
not reproduce the items a seeded run of __getitem__ gives (after the first item's last draw).

Stated, not reproduced:
  * val_dset=True (its ground_truth needs the pre-padded laplacian_decode), signed_sqrt=False and the decoder class's residual_mean=None (a
    Welford pass over 10 000 items: dataset.calculate_stats_welford) raise NotImplementedError.
  * The reference's decoder class fails on clip_edges=False (it calls .float() on None); so does this one, with a NotImplementedError.
  * The reference's autoencoder class keeps its keys in set order, which changes from one interpreter to the next; here they are sorted.  With
    residual_mean=None its statistics pass stores values that nothing reads and its items stay unnormalised; here the pass is not run.
  * Groups are square (the reference assumes it); others raise ValueError, as does a latents crop that is no multiple of 32 or below 64.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import Library
from ._plumbing import call, engine_for as _engine_for
from .beauty import beauty_class

_P = C.c_void_p
_F = C.c_float
_SIGS = {
    "td_batch_last_error": (C.c_char_p, []),
    "td_batch_views": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, _F, _P, C.c_int]),
    "td_batch_latents": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _F, _P, C.c_int]),
    "td_batch_cond_image": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _F, _P, _F, _P, _P, _P, _P, _P, C.c_int, _P, C.c_int]),
    "td_batch_cond_vector": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _F, _F, _F, _F, _F, _F, _F, _P, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_batch.so", _SIGS, "td_batch_last_error", "td_batch")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

ITEM_FIELDS = 6             # include/td_batch.h TD_BATCH_ITEM_FIELDS: group, i, j, transform_idx, li, lj
MAX_ITEMS = 65536           # TD_BATCH_MAX_ITEMS
MAX_CROP = 4096             # TD_BATCH_MAX_CROP
HALO = 32                   # TD_BATCH_HALO
COND_CHANNELS = 7           # TD_BATCH_COND_CHANNELS
COND_LEN = 58               # TD_BATCH_COND_LEN
PLANES = {"lowfreq": 0, "lowres_exact": 1, "residual": 2}       # TD_BATCH_PLANE_*
CLIMATE_CHANNELS = (0, 3, 11, 14)                               # h5_latents_dataset.py:179
LOWFREQ_MEAN, LOWFREQ_STD = -31.4, 38.6                         # h5_latents_dataset.py:247-248
STATS_ITEMS = 1024                                              # compute_cond_input_stats


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def inverse_offsets(i, j, h, w, transform_idx, side):
    """(li, lj) of h5_latents_dataset.py:299-303: the origin, in the untransformed plane of side `side`, of the (h, w) crop at (i, j) of its view"""
    li, lj = i, j
    for _ in range(transform_idx % 4):
        li, lj = lj, side - li - h
    if transform_idx // 4 == 1:
        lj = side - lj - w
    return li, lj


def mp_concat_factors(sizes=(16, 16, 4, 16, 5, 1)):
    """mp_concat's scale of each part (mp_layers.py:77-86) as fp32 torch computes it, as Python floats of fp32 values"""
    w = torch.full((len(sizes),), 1 / len(sizes), dtype=torch.float32)
    sum_n = torch.tensor(sum(sizes), dtype=torch.float32)
    c = torch.sqrt(sum_n / torch.sum(torch.square(w)))
    return [float(c / np.sqrt(n) * w[k]) for k, n in enumerate(sizes)]


# ------------------------------------------------------------------------------------------------------------------------------ key lists
def _walk(tree, pct_land_ranges, subset_resolutions, split, dataset_name):
    """the reference's loop over res / chunk / subchunk (h5_latents_dataset.py:85-110): yields (subset, key, group)"""
    for n, (pct_land_range, res) in enumerate(zip(pct_land_ranges, subset_resolutions)):
        if pct_land_range is None:
            pct_land_range = [0, 1]
        if str(res) not in tree:
            continue
        res_group = tree[str(res)]
        for chunk_id in res_group:
            chunk_group = res_group[chunk_id]
            for subchunk_id in chunk_group:
                group = chunk_group[subchunk_id]
                if dataset_name not in group:
                    continue
                attrs = group[dataset_name].attrs
                if pct_land_range[0] <= attrs["pct_land"] <= pct_land_range[1] and (split is None or attrs["split"] == split):
                    yield n, (chunk_id, res, subchunk_id), group


def latents_keys(tree, pct_land_ranges, subset_resolutions, split, beauty_dist):
    """H5LatentsDataset.keys as the reference builds and sorts it: per subset five beauty buckets (a subset without beauty_dist fills bucket
    0), or per subset one list when no subset uses the beauty distribution"""
    n = len(pct_land_ranges)
    bucketed = beauty_dist != [False] * n
    keys = [[set() for _ in range(5)] for _ in range(n)] if bucketed else [set() for _ in range(n)]
    for s, key, group in _walk(tree, pct_land_ranges, subset_resolutions, split, "latent"):
        if beauty_dist[s]:
            keys[s][beauty_class(float(group.attrs["beauty_score"]))].add(key)
        else:
            keys[s][0].add(key)       # the reference's own line: with no bucket anywhere keys[s] is a set and this raises, as it does there
    return [[sorted(b) for b in k] for k in keys] if bucketed else [sorted(k) for k in keys]


def residual_keys(tree, pct_land_ranges, subset_resolutions, split):
    """the decoder and autoencoder classes' keys, sorted by (chunk, res, subchunk)"""
    keys = [set() for _ in pct_land_ranges]
    for s, key, _ in _walk(tree, pct_land_ranges, subset_resolutions, split, "residual"):
        keys[s].add(key)
    return [sorted(k, key=lambda x: (x[0], x[1], x[2])) for k in keys]


def _path(key):
    chunk_id, res, subchunk_id = key
    return f"{res}/{chunk_id}/{subchunk_id}"


def _group(tree, key):
    """the group of a key, walked level by level (a plain dict of dicts takes no 'a/b/c' path)"""
    chunk_id, res, subchunk_id = key
    return tree[str(res)][chunk_id][subchunk_id]


def _flat_keys(keys):
    out = []
    for k in keys:
        for b in (k if k and isinstance(k[0], list) else [k]):
            out.extend(tuple(x) for x in b)
    return sorted(set(out), key=lambda x: (str(x[1]), x[0], x[2]))


# ------------------------------------------------------------------------------------------------------------------------------ resident groups
class DeviceGroups:
    """The planes of the selected groups, resident on the device, and the group table libtd_batch.so reads them through.

    tree: a mapping shaped like the HDF5 file; keys: (chunk_id, res, subchunk_id) tuples; need: the datasets to upload, of latent (kept fp16),
    lowfreq, lowres_exact, climate (only the channels 0, 3, 11, 14 are kept) and residual.  Shapes are checked at construction, without a
    device; the upload happens once, on first use."""

    def __init__(self, tree, keys, need, *, device=None, engine=None):
        self.tree, self.keys, self.need = tree, [tuple(k) for k in keys], tuple(need)
        self.device, self.engine = device, engine
        self.index = {_path(k): n for n, k in enumerate(self.keys)}
        self.sides, self.residual_sides, self.latent_channels = [], [], None
        for k in self.keys:
            g = _group(tree, k)
            shapes = {name: tuple(int(d) for d in g[name].shape) for name in self.need}
            side = None
            for name, s in shapes.items():
                if s[-1] != s[-2]:
                    raise ValueError(f"{_path(k)}/{name} is {s}: groups must be square")
                if name != "residual":
                    if side not in (None, s[-1]):
                        raise ValueError(f"{_path(k)}: {name} has side {s[-1]}, another plane {side}")
                    side = s[-1]
            if "latent" in shapes:
                s = shapes["latent"]
                if len(s) != 4 or s[0] != 8 or s[1] % 2:
                    raise ValueError(f"{_path(k)}/latent is {s}: expected (8, 2 c, S, S)")
                if np.dtype(g["latent"].dtype) != np.float16:
                    raise ValueError(f"{_path(k)}/latent is {g['latent'].dtype}: the encoded dataset stores float16")
                if self.latent_channels not in (None, s[1] // 2):
                    raise ValueError(f"{_path(k)}/latent has {s[1] // 2} channels, another group {self.latent_channels}")
                self.latent_channels = s[1] // 2
            if "climate" in shapes and shapes["climate"][0] <= max(CLIMATE_CHANNELS):
                raise ValueError(f"{_path(k)}/climate is {shapes['climate']}: channels {CLIMATE_CHANNELS} are read")
            rs = shapes["residual"][-1] if "residual" in shapes else 0
            self.sides.append(side if side is not None else rs // 8)
            self.residual_sides.append(rs)
        self._planes, self._table = None, None

    def __len__(self):
        return len(self.keys)

    def resolve(self):
        """(engine, device), the engine made on first use"""
        self.engine, dev = _engine_for(torch.empty(0, device=self.device) if self.device is not None else None, self.engine)
        self.device = dev
        return self.engine, dev

    def table(self):
        """the device group table, int64 (G, 6): five plane addresses and side | residual_side << 32; uploads the planes on first use"""
        if self._table is None:
            _, dev = self.resolve()
            planes, rows = [], []
            for n, k in enumerate(self.keys):
                g = _group(self.tree, k)
                held = {}
                for name in self.need:
                    d = g[name]
                    if name == "climate":
                        a = torch.stack([torch.as_tensor(np.asarray(d[c]), dtype=torch.float32) for c in CLIMATE_CHANNELS]) if not torch.is_tensor(d) \
                            else d[list(CLIMATE_CHANNELS)].to(torch.float32)
                    else:
                        a = d if torch.is_tensor(d) else torch.as_tensor(np.asarray(d[:]))
                        a = a.to(torch.float16 if name == "latent" else torch.float32)
                    held[name] = a.to(dev).contiguous()
                planes.append(held)
                ptr = lambda name: held[name].data_ptr() if name in held else 0
                rows.append([ptr("latent"), ptr("lowfreq"), ptr("lowres_exact"), ptr("climate"), ptr("residual"),
                             self.sides[n] | (self.residual_sides[n] << 32)])
            self._planes = planes
            self._table = torch.tensor(rows, dtype=torch.int64).to(dev)
        return self._table

    def plane(self, path, name):
        """the resident tensor `name` of group `path` (climate: its four kept channels)"""
        self.table()
        return self._planes[self.index[path]][name]


def _items(groups, items):
    """the device item table, int32 (N, 6)"""
    _, dev = groups.resolve()
    t = torch.as_tensor(items, dtype=torch.int32)
    if t.dim() != 2 or t.shape[1] != ITEM_FIELDS or not 1 <= t.shape[0] <= MAX_ITEMS:
        raise ValueError(f"items must be (N, {ITEM_FIELDS}) with 1 <= N <= {MAX_ITEMS}, got {tuple(t.shape)}")
    return t.to(dev).contiguous()


def _dev32(x, dev, shape, what):
    t = torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


# ------------------------------------------------------------------------------------------------------------------------------ device forms
@torch.no_grad()
def views(groups, items, plane, size, *, origin="inverse", offset=0, affine=None, enqueue_only=False):
    """(N, size, size) fp32: the dihedral view of the size x size window of `plane` ('lowfreq', 'lowres_exact', 'residual') of every item, at its
    inverse offsets (li, lj) (origin='inverse') or at (i, j) itself (origin='own'), moved by `offset`; NaN outside the plane.
    affine=(a, b, c) applies ((x - a) / b) * c in fp32."""
    if plane not in PLANES:
        raise ValueError(f"plane must be one of {sorted(PLANES)}, got {plane!r}")
    if origin not in ("inverse", "own"):
        raise ValueError(f"origin must be 'inverse' or 'own', got {origin!r}")
    size = int(size)
    if not 1 <= size <= MAX_CROP:
        raise ValueError(f"size must be in 1 .. {MAX_CROP}, got {size}")
    engine, dev = groups.resolve()
    it = _items(groups, items)
    out = torch.empty((it.shape[0], size, size), dtype=torch.float32, device=dev)
    a, b, c = (float(v) for v in affine) if affine is not None else (0.0, 1.0, 1.0)
    call(_LIB, "td_batch_views", engine, dev, _dp(groups.table()), len(groups), _dp(it), it.shape[0], PLANES[plane], int(origin == "own"), int(offset),
         size, size, int(affine is not None), a, b, c, _dp(out), enqueue_only=enqueue_only, ordered=True)
    return out


@torch.no_grad()
def sample_latents(groups, items, noise, *, mode, mean=None, std=None, sigma_data=0.5, enqueue_only=False):
    """The reparameterisation from slab transform_idx of every item's latent at (i, j), noise (N, c, h, w).  mode 0 (the latents class): fp32
    noise -> fp32 (N, c, h, w), ((n e + m) - mean) / std * sigma_data; mode 1 (the decoder class): fp16 noise -> fp16 (N, c, 8 h, 8 w), the
    half-precision draw upsampled by nearest."""
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 or 1, got {mode!r}")
    engine, dev = groups.resolve()
    it = _items(groups, items)
    lc = groups.latent_channels
    if lc is None:
        raise ValueError("these groups hold no latent")
    nz = torch.as_tensor(noise)
    if nz.dim() != 4 or nz.shape[0] != it.shape[0] or nz.shape[1] != lc:
        raise ValueError(f"noise must be ({it.shape[0]}, {lc}, h, w), got {tuple(nz.shape)}")
    h, w = int(nz.shape[2]), int(nz.shape[3])
    nz = nz.to(device=dev, dtype=torch.float16 if mode else torch.float32).contiguous()
    if mode == 0:
        m, s = _dev32(mean, dev, (lc,), "mean"), _dev32(std, dev, (lc,), "std")
        out = torch.empty((it.shape[0], lc, h, w), dtype=torch.float32, device=dev)
    else:
        m = s = None
        out = torch.empty((it.shape[0], lc, 8 * h, 8 * w), dtype=torch.float16, device=dev)
    call(_LIB, "td_batch_latents", engine, dev, _dp(groups.table()), len(groups), _dp(it), it.shape[0], lc, h, w, mode, _dp(nz), _dp(m), _dp(s),
         float(sigma_data), _dp(out), enqueue_only=enqueue_only, ordered=True)
    return out


def _check_crop(crop):
    crop = int(crop)
    if crop % HALO or crop < 2 * HALO or crop > MAX_CROP:
        raise ValueError(f"the cond image needs a crop that is a multiple of {HALO} in {2 * HALO} .. {MAX_CROP}, got {crop}")
    return crop


@torch.no_grad()
def cond_image(groups, items, crop, *, u_drop=None, dropout=0.0, u_noise=None, max_noise=0.0, z_mean=None, z_p5=None, mean=None, std=None,
               enqueue_only=False):
    """_get_cond_image for every item: (N, 7, g, g) fp32, g = (crop + 64) / 32 -- block mean, 5 % quantile, four climate means, mask -- read
    straight from the resident planes.  u_drop (N, g, g) uniforms switch the dropout on, u_noise (N) with z_mean, z_p5 (N, g, g) the noise;
    mean / std (7) normalise, None leaves the stack raw (the reference's `cond_input_mean is None` branch)."""
    crop = _check_crop(crop)
    engine, dev = groups.resolve()
    it = _items(groups, items)
    N, g = it.shape[0], (crop + 2 * HALO) // HALO
    ud = _dev32(u_drop, dev, (N, g, g), "u_drop") if u_drop is not None else None
    un = zm = zp = None
    if u_noise is not None:
        un, zm, zp = _dev32(u_noise, dev, (N,), "u_noise"), _dev32(z_mean, dev, (N, g, g), "z_mean"), _dev32(z_p5, dev, (N, g, g), "z_p5")
    raw = mean is None
    m = s = None
    if not raw:
        m, s = _dev32(mean, dev, (COND_CHANNELS,), "mean"), _dev32(std, dev, (COND_CHANNELS,), "std")
    out = torch.empty((N, COND_CHANNELS, g, g), dtype=torch.float32, device=dev)
    call(_LIB, "td_batch_cond_image", engine, dev, _dp(groups.table()), len(groups), _dp(it), N, crop, float(dropout), _dp(ud), float(max_noise),
         _dp(un), _dp(zm), _dp(zp), _dp(m), _dp(s), int(raw), _dp(out), enqueue_only=enqueue_only, ordered=True)
    return out


_FACTORS = []


@torch.no_grad()
def cond_vector(cond_img, histogram_raw, noise_level, z_replace=None, *, engine=None, enqueue_only=False):
    """build_cond_inputs for every item: cond_img (N, 7, g, g) device tensor, histogram_raw (N, 5), noise_level (N) -> ((N, 58) fp32, (N, 4)
    int32 flags of the NaN climate centres).  z_replace (N, 4): the normal that replaces a NaN centre, by slot; None leaves the NaN."""
    if not (torch.is_tensor(cond_img) and cond_img.is_cuda):
        raise ValueError("cond_img must be a device tensor (the device forms take no host arrays)")
    if cond_img.dim() != 4 or cond_img.shape[1] != COND_CHANNELS or cond_img.shape[2] != cond_img.shape[3] or cond_img.shape[2] < 4:
        raise ValueError(f"cond_img must be (N, {COND_CHANNELS}, g, g) with g >= 4, got {tuple(cond_img.shape)}")
    engine, dev = _engine_for(cond_img, engine)
    img = cond_img.to(torch.float32).contiguous()
    N, g = int(img.shape[0]), int(img.shape[2])
    hist, nl = _dev32(histogram_raw, dev, (N, 5), "histogram_raw"), _dev32(noise_level, dev, (N,), "noise_level")
    zr = _dev32(z_replace, dev, (N, 4), "z_replace") if z_replace is not None else None
    if not _FACTORS:
        _FACTORS.extend(mp_concat_factors())
    out = torch.empty((N, COND_LEN), dtype=torch.float32, device=dev)
    flags = torch.empty((N, 4), dtype=torch.int32, device=dev)
    call(_LIB, "td_batch_cond_vector", engine, dev, _dp(img), N, g, _dp(hist), _dp(nl), _dp(zr), float(np.float32(np.sqrt(12))), *_FACTORS, _dp(out),
         _dp(flags), enqueue_only=enqueue_only, ordered=True)
    return out, flags


# ------------------------------------------------------------------------------------------------------------------------------ drop-ins
class _ItemDataset:
    """what the three classes share: the generator, the subset draw, the resident groups"""

    def _setup(self, h5_file, crop_size, pct_land_ranges, subset_resolutions, subset_weights, subset_class_labels, device, engine):
        self.h5_file, self.crop_size = h5_file, crop_size
        self.pct_land_ranges, self.subset_resolutions = pct_land_ranges, subset_resolutions
        self.subset_weights, self.subset_class_labels = subset_weights, subset_class_labels
        n = len(subset_weights)
        assert len(pct_land_ranges) == len(subset_resolutions) == n, \
            "Number of subsets must match between pct_land_ranges, dataset_resolutions, and subset_weights."
        assert subset_class_labels is None or len(subset_class_labels) == n, "Number of subset class labels must match number of subsets."
        self.rng = torch.Generator()
        self._device, self._engine = device, engine

    def set_seed(self, seed):
        self.rng = torch.Generator()
        self.rng.manual_seed(int(seed))

    def _draw_subset(self):
        return torch.multinomial(torch.tensor(self.subset_weights, dtype=torch.float32), 1, generator=self.rng).item()

    def _randint(self, *a):
        return torch.randint(*a, (1,), generator=self.rng).item()

    def _check_sides(self, least, what):
        for k, side in zip(self.groups.keys, self.groups.sides):
            if side < least:
                raise ValueError(f"{_path(k)}: side {side} is below {least} ({what})")

    def _labels(self, plans, dev):
        return torch.tensor([self.subset_class_labels[p["subset"]] for p in plans], device=dev)

    def _table(self, plans):
        return torch.tensor([[self.groups.index[p["path"]], p["i"], p["j"], p["t"], p["li"], p["lj"]] for p in plans], dtype=torch.int32)


class H5LatentsDataset(_ItemDataset):
    """Drop-in for h5_latents_dataset.py's H5LatentsDataset with the items built on the device (module docstring).  h5_file: the mapping."""

    def __init__(self, h5_file, crop_size, pct_land_ranges, subset_resolutions, subset_weights=None, subset_class_labels=None, eval_dataset=False,
                 latents_mean=None, latents_std=None, sigma_data=0.5, clip_edges=True, split=None, beauty_dist=True, residual_mean=None,
                 residual_std=None, cond_input_mean=None, cond_input_std=None, cond_input_dropout=0.0, cond_input_max_noise=0.0, val_dset=False,
                 *, device=None, engine=None):
        if val_dset:
            raise NotImplementedError("val_dset=True: its ground_truth needs the pre-padded laplacian_decode")
        _check_crop(crop_size)
        pct_land_ranges, subset_resolutions, subset_weights = pct_land_ranges or [[0, 1]], subset_resolutions or [480], subset_weights or [1.0]
        self._setup(h5_file, crop_size, pct_land_ranges, subset_resolutions, subset_weights, subset_class_labels, device, engine)
        as_col = lambda v: (torch.tensor(v) if isinstance(v, list) else torch.clone(v)).view(-1, 1, 1)
        self.latents_mean, self.latents_std = as_col(latents_mean), as_col(latents_std)
        self.sigma_data, self.split, self.eval_dataset, self.clip_edges, self.val_dset = sigma_data, split, eval_dataset, clip_edges, val_dset
        self.beauty_dist = beauty_dist or [True] * len(subset_weights)
        self.cond_input_dropout, self.cond_input_max_noise = cond_input_dropout, cond_input_max_noise
        self.keys = latents_keys(h5_file, pct_land_ranges, subset_resolutions, split, self.beauty_dist)
        self.groups = DeviceGroups(h5_file, _flat_keys(self.keys), ("latent", "lowfreq", "lowres_exact", "climate"), device=device, engine=engine)
        self._check_sides(crop_size + 2 if clip_edges else crop_size, "crop_size + 2 with clip_edges, else crop_size")
        self.residual_mean, self.residual_std = residual_mean, residual_std
        self.cond_input_mean, self.cond_input_std = cond_input_mean or None, cond_input_std or None
        if self.cond_input_mean is None:
            self.compute_cond_input_stats()

    def __len__(self):
        return 100000

    def compute_cond_input_stats(self):
        """the unnormalised cond image of 1024 items in one batch (get_batch's own stream of draws), then the reference's NumPy expressions"""
        values = self.get_batch(STATS_ITEMS)["cond_inputs_img"].cpu().numpy()
        self.cond_input_mean = [np.nanmean(values[:, c:c + 1]) for c in range(7)]
        values[:, :1] = np.nan_to_num(values[:, :1], self.cond_input_mean[0])
        values[:, 1:2] = np.nan_to_num(values[:, 1:2], self.cond_input_mean[1])
        self.cond_input_std = [np.std(values[:, :1]), np.std(values[:, 1:2])] + [np.nanstd(values[:, c:c + 1]) for c in range(2, 7)]
        print(f"Computed cond input mean: {self.cond_input_mean}, std: {self.cond_input_std}")

    # the host half: every draw of __getitem__ but the last, in the reference's order
    def plan_item(self):
        p = {"subset": self._draw_subset()}
        buckets = self.keys[p["subset"]]
        if self.beauty_dist[p["subset"]]:
            subset_lens = torch.tensor([len(buckets[b]) for b in range(5)]).float()
            baseline_probs = torch.log(subset_lens / subset_lens.sum())
            p["histogram_raw"] = torch.randn(5, generator=self.rng)
            histogram = torch.softmax(p["histogram_raw"] + baseline_probs, dim=0)
            bucket = torch.multinomial(histogram, 1, generator=self.rng).item()
        else:
            p["histogram_raw"] = torch.randn(5, generator=self.rng)
            bucket = 0
        p["index"] = self._randint(len(buckets[bucket]))
        key = tuple(buckets[bucket][p["index"]])
        p["path"] = _path(key)
        side = self.groups.sides[self.groups.index[p["path"]]]
        crop = self.crop_size
        if not self.eval_dataset:
            lo, hi = (1, side - crop) if self.clip_edges else (0, side - crop + 1)
            p["i"], p["j"] = self._randint(lo, hi), self._randint(lo, hi)
            p["t"] = self._randint(8)
        else:
            p["i"] = p["j"] = (side - crop) // 2
            p["t"] = 0
        p["li"], p["lj"] = inverse_offsets(p["i"], p["j"], crop, crop, p["t"], side)
        p["noise"] = torch.randn((self.groups.latent_channels, crop, crop), generator=self.rng)
        g = (crop + 2 * HALO) // HALO
        if self.cond_input_dropout:
            p["u_drop"] = torch.rand((1, g, g), generator=self.rng)
        if self.cond_input_max_noise:
            p["u_noise"] = torch.rand(1, generator=self.rng)
            p["z_mean"], p["z_p5"] = torch.randn((1, g, g), generator=self.rng), torch.randn((1, g, g), generator=self.rng)
        return p

    def draw_replacements(self, count):
        """the last draw of an item: one normal per NaN climate centre"""
        return torch.randn((int(count),), generator=self.rng)

    def _build(self, plans, z_replace):
        """the device half for planned items; z_replace (N, 4) or a callable flags -> (N, 4)"""
        G, crop = self.groups, self.crop_size
        _, dev = G.resolve()
        items = self._table(plans).to(dev)
        stack = lambda k: torch.stack([p[k] for p in plans])
        latent = sample_latents(G, items, stack("noise"), mode=0, mean=self.latents_mean.view(-1), std=self.latents_std.view(-1), sigma_data=self.sigma_data)
        lowfreq = views(G, items, "lowfreq", crop, affine=(LOWFREQ_MEAN, LOWFREQ_STD, self.sigma_data))
        kw = {}
        if self.cond_input_dropout:
            kw.update(u_drop=stack("u_drop")[:, 0], dropout=self.cond_input_dropout)
        if self.cond_input_max_noise:
            kw.update(u_noise=stack("u_noise")[:, 0], max_noise=self.cond_input_max_noise, z_mean=stack("z_mean")[:, 0], z_p5=stack("z_p5")[:, 0])
            noise_level = stack("u_noise")[:, 0]
        else:
            noise_level = torch.zeros(len(plans))
        img = cond_image(G, items, crop, mean=self.cond_input_mean, std=self.cond_input_std, **kw)
        hist = stack("histogram_raw")
        if callable(z_replace):
            _, flags = cond_vector(img, hist, noise_level, engine=G.engine)
            z_replace = z_replace(flags)
        vec, _ = cond_vector(img, hist, noise_level, z_replace, engine=G.engine)
        return {"image": torch.cat([latent, lowfreq[:, None]], dim=1), "cond_vector": vec, "cond_inputs_img": img, "histogram_raw": hist.to(dev),
                "noise_level": noise_level.to(dev)}

    def __getitem__(self, idx, _raw_cond_inputs=False):
        p = self.plan_item()

        def replacements(flags):
            f = flags.cpu()[0].bool()                      # the one read-back of the item: 16 bytes
            z = torch.zeros(1, 4)
            z[0, f] = self.draw_replacements(int(f.sum()))
            return z
        b = self._build([p], replacements)
        cond_inputs = [b["cond_vector"][0]]
        if self.subset_class_labels is not None:
            cond_inputs += [self._labels([p], b["image"].device)[0]]
        return {"image": b["image"][0], "cond_inputs": cond_inputs, "cond_inputs_img": b["cond_inputs_img"][0], "path": p["path"],
                "histogram_raw": b["histogram_raw"][0], "noise_level": b["noise_level"][0].reshape((1,) if self.cond_input_max_noise else ())}

    def get_batch(self, n):
        """n items in one set of launches: the keys of __getitem__ with a leading batch axis ('path' a list).  Every item draws FOUR replacement
        normals whatever its data holds, so the stream of draws is get_batch's own, not that of n successive __getitem__ calls."""
        plans = []
        for _ in range(int(n)):
            p = self.plan_item()
            p["z_replace"] = torch.randn(4, generator=self.rng)
            plans.append(p)
        b = self._build(plans, torch.stack([p["z_replace"] for p in plans]))
        cond_inputs = [b["cond_vector"]]
        if self.subset_class_labels is not None:
            cond_inputs += [self._labels(plans, b["image"].device)]
        return {"image": b["image"], "cond_inputs": cond_inputs, "cond_inputs_img": b["cond_inputs_img"], "path": [p["path"] for p in plans],
                "histogram_raw": b["histogram_raw"], "noise_level": b["noise_level"], "plan": plans}

    def denormalize_residual(self, residual):
        return residual * self.residual_std + self.residual_mean

    def denormalize_lowfreq(self, lowfreq):
        return lowfreq * LOWFREQ_STD + LOWFREQ_MEAN


class H5DecoderTerrainDataset(_ItemDataset):
    """Drop-in for h5_decoder_terrain_dataset.py's H5DecoderTerrainDataset with the items built on the device.  h5_file: the mapping."""

    def __init__(self, h5_file, crop_size, pct_land_ranges, subset_resolutions, subset_weights=None, subset_class_labels=None, eval_dataset=False,
                 clip_edges=True, split=None, residual_mean=None, residual_std=None, sigma_data=0.5, *, device=None, engine=None):
        if residual_mean is None or residual_std is None:
            raise NotImplementedError("residual_mean=None: the Welford pass over 10 000 items stays with the caller (dataset.calculate_stats_welford)")
        if not clip_edges:
            raise NotImplementedError("clip_edges=False: the reference's class fails on it (lowfreq_padded is None)")
        if crop_size % 8 or crop_size < 8:
            raise ValueError("Crop size must be divisible by 8")
        if subset_weights is None:
            subset_weights = [1] * len(pct_land_ranges)
        self._setup(h5_file, crop_size, pct_land_ranges, subset_resolutions, subset_weights, subset_class_labels, device, engine)
        self.eval_dataset, self.clip_edges, self.sigma_data = eval_dataset, clip_edges, sigma_data
        self.residual_mean, self.residual_std = residual_mean, residual_std
        self.keys = residual_keys(h5_file, pct_land_ranges, subset_resolutions, split)
        self.groups = DeviceGroups(h5_file, _flat_keys(self.keys), ("latent", "lowfreq", "residual"), device=device, engine=engine)
        for k, rs in zip(self.groups.keys, self.groups.residual_sides):
            if rs < crop_size + 2:
                raise ValueError(f"{_path(k)}: residual side {rs} is below crop_size + 2")
        self._check_sides(crop_size // 8 + 2, "crop_size / 8 + 2 with clip_edges")

    def __len__(self):
        return max(len(keys) for keys in self.keys)

    def plan_item(self):
        p = {"subset": self._draw_subset()}
        p["index"] = self._randint(len(self.keys[p["subset"]]))
        p["path"] = _path(self.keys[p["subset"]][p["index"]])
        n = self.groups.index[p["path"]]
        side, rside, h = self.groups.sides[n], self.groups.residual_sides[n], self.crop_size // 8
        if not self.eval_dataset:
            p["i"], p["j"] = self._randint(1, (side - h - 1) + 1), self._randint(1, (side - h - 1) + 1)
            p["t"] = self._randint(8)
        else:
            p["i"] = p["j"] = (side - h) // 2
            p["t"] = 0
        p["li"], p["lj"] = inverse_offsets(p["i"] * 8, p["j"] * 8, h * 8, h * 8, p["t"], rside)        # residual pixels
        p["noise"] = torch.randn((self.groups.latent_channels, h, h), generator=self.rng, dtype=torch.float16)
        return p

    def _build(self, plans):
        G, h = self.groups, self.crop_size // 8
        _, dev = G.resolve()
        items = self._table(plans).to(dev)
        padded = views(G, items, "lowfreq", h + 2, origin="own", offset=-1)
        image = views(G, items, "residual", self.crop_size, affine=(self.residual_mean, self.residual_std, self.sigma_data))
        cond = sample_latents(G, items, torch.stack([p["noise"] for p in plans]), mode=1)
        return {"image": image[:, None], "cond_img": cond, "lowfreq": padded[:, None, 1:-1, 1:-1].contiguous(), "lowfreq_padded": padded[:, None]}

    def __getitem__(self, index):
        p = self.plan_item()
        b = self._build([p])
        cond_inputs = [self._labels([p], b["image"].device)[0]] if self.subset_class_labels is not None else []
        return {"image": b["image"][0], "cond_img": b["cond_img"][0], "cond_inputs": cond_inputs, "path": p["path"], "lowfreq": b["lowfreq"][0],
                "lowfreq_padded": b["lowfreq_padded"][0]}

    def get_batch(self, n):
        """n items in one set of launches: the keys of __getitem__ with a leading batch axis ('path' a list); the same draws as n __getitem__ calls"""
        plans = [self.plan_item() for _ in range(int(n))]
        b = self._build(plans)
        b["cond_inputs"] = [self._labels(plans, b["image"].device)] if self.subset_class_labels is not None else []
        b["path"], b["plan"] = [p["path"] for p in plans], plans
        return b

    def denormalize_residual(self, residual):
        return (residual * self.residual_std) + self.residual_mean


class H5AutoencoderDataset(_ItemDataset):
    """Drop-in for h5_autoencoder_dataset.py's H5AutoencoderDataset with the items built on the device.  h5_file: the mapping."""

    def __init__(self, h5_file, crop_size, pct_land_ranges, subset_resolutions, subset_weights=None, subset_class_labels=None, split=None,
                 residual_mean=None, residual_std=None, signed_sqrt=True, *, device=None, engine=None):
        if not signed_sqrt:
            raise NotImplementedError("signed_sqrt=False: the decode / re-encode of every item stays with the caller")
        if residual_mean is not None and residual_std is None:
            raise ValueError("residual_mean without residual_std")
        if subset_weights is None:
            subset_weights = [1] * len(pct_land_ranges)
        self._setup(h5_file, crop_size, pct_land_ranges, subset_resolutions, subset_weights, subset_class_labels, device, engine)
        self.signed_sqrt, self.residual_mean, self.residual_std = signed_sqrt, residual_mean, residual_std
        self.keys = residual_keys(h5_file, pct_land_ranges, subset_resolutions, split)
        self.groups = DeviceGroups(h5_file, _flat_keys(self.keys), ("residual",), device=device, engine=engine)
        for k, rs in zip(self.groups.keys, self.groups.residual_sides):
            if rs < crop_size:
                raise ValueError(f"{_path(k)}: residual side {rs} is below crop_size")

    def __len__(self):
        return max(len(keys) for keys in self.keys)

    def plan_item(self):
        p = {"subset": self._draw_subset()}
        p["index"] = self._randint(len(self.keys[p["subset"]]))
        p["path"] = _path(self.keys[p["subset"]][p["index"]])
        rside = self.groups.residual_sides[self.groups.index[p["path"]]]
        most = (rside - self.crop_size) // 8
        p["i"], p["j"] = self._randint(0, most + 1) * 8, self._randint(0, most + 1) * 8
        p["t"] = self._randint(8)
        p["li"], p["lj"] = p["i"], p["j"]                    # the view applies to the window itself
        return p

    def _build(self, plans):
        _, dev = self.groups.resolve()
        affine = (self.residual_mean, self.residual_std, 1.0) if self.residual_mean is not None else None
        return views(self.groups, self._table(plans).to(dev), "residual", self.crop_size, origin="own", affine=affine)[:, None]

    def __getitem__(self, index):
        p = self.plan_item()
        image = self._build([p])[0]
        if self.subset_class_labels is not None:
            return {"image": image, "cond_inputs": [self._labels([p], image.device)[0]]}
        return {"image": image}

    def get_batch(self, n):
        """n items in one launch: 'image' (n, 1, crop, crop) and the labels; the same draws as n __getitem__ calls"""
        plans = [self.plan_item() for _ in range(int(n))]
        out = {"image": self._build(plans), "plan": plans}
        if self.subset_class_labels is not None:
            out["cond_inputs"] = [self._labels(plans, out["image"].device)]
        return out

    def denormalize_residual(self, residual):
        return (residual * self.residual_std) + self.residual_mean
