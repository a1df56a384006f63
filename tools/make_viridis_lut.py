"""Writes terrain_diffusion_amd/_viridis.py: matplotlib's "viridis" colormap as a 256 x 3 literal table, so that the package colours the
explorer's coarse view without importing matplotlib.  The source data (matplotlib/_cm_listed.py, _viridis_data; by Nathaniel Smith, Stefan van
der Walt and Eric Firing) is released under CC0.  Needs matplotlib; the written module does not.

    python tools/make_viridis_lut.py
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "terrain_diffusion_amd", "_viridis.py")


def main():
    import matplotlib
    from matplotlib import _cm_listed
    data = np.asarray(_cm_listed._viridis_data, dtype=np.float64)
    assert data.shape == (256, 3)
    lut = matplotlib.colormaps["viridis"](np.arange(256))[:, :3]
    assert np.array_equal(lut, data)   # a ListedColormap's lookup table is its colour list
    lines = ['"""matplotlib\'s "viridis" colormap: its 256 RGB rows (CC0 data of matplotlib/_cm_listed.py), written by tools/make_viridis_lut.py."""',
             "VIRIDIS = ("]
    lines += ["    (%r, %r, %r)," % tuple(float(v) for v in row) for row in data]
    lines += [")", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {OUT} (matplotlib {matplotlib.__version__})")


if __name__ == "__main__":
    main()
