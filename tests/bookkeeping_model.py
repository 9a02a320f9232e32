"""NumPy reference of the bookkeeping every step goes through: compaction, ID ranks, the sort key and the status flags.

Written from the documented contracts (include/odrift.h), not from the kernels; checked against plain Python
loops in tests/test_bookkeeping_model.py and used by tests/test_gpu_bookkeeping.py and tests/test_gpu_block_limits.py."""
import numpy as np


def compact_in_place(status):
    """odr_compact, the default: (src_of_slot, dead_src).  Slot j of the compacted set holds the element that sat at
    src_of_slot[j]; the deactivated store is extended by the elements at dead_src, in that order.

    kept = number of status == 0.  Holes are the removed indices below kept, ascending; fills are the kept indices at or above
    kept, DESCENDING; hole k takes fill k; every other slot below kept keeps its element.  The removed elements go to the
    store in ascending index order."""
    status = np.asarray(status)
    keep = status == 0
    kept = int(keep.sum())
    idx = np.arange(status.size, dtype=np.int64)
    holes = idx[:kept][~keep[:kept]]
    fills = idx[kept:][keep[kept:]][::-1]
    src = idx[:kept].copy()
    src[holes] = fills
    return src, idx[~keep]


def compact_ordered(status):
    """ODR_ORDERED_COMPACT: the survivors in index order, the same deactivated store."""
    keep = np.asarray(status) == 0
    idx = np.arange(keep.size, dtype=np.int64)
    return idx[keep], idx[~keep]


def ranks(ids, counted):
    """Position of every ID among the counted IDs in ascending order (IDs are distinct).  For an element that is not counted:
    the number of counted IDs below its own."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.searchsorted(np.sort(ids[np.asarray(counted, dtype=bool)]), ids, side='left')


def sort_bins(ny, nx):
    """Histogram bins of sort_by_cell: 8x8-cell tiles of 64 cells, plus one for elements outside the grid."""
    return ((nx + 7) // 8) * ((ny + 7) // 8) * 64 + 1


def cell_keys(x, y, lon, lat, lon_mode=2):
    """The sort key of sort_by_cell for a geographic grid with the coordinate arrays x, y: 8x8-cell tiles, row-major cells
    inside; outside the grid: the last bin.  lon_mode 1: longitudes wrapped to [-180, 180), 2: to [0, 360), 0: as they are."""
    ny, nx = len(y), len(x)
    lon = np.asarray(lon, dtype=np.float64)
    if lon_mode == 1:
        lon = np.mod(lon + 180.0, 360.0) - 180.0
    elif lon_mode == 2:
        lon = np.mod(lon, 360.0)
    xi = (lon - float(x[0])) / float(x[-1] - x[0]) * (nx - 1)
    yi = (lat - float(y[0])) / float(y[-1] - y[0]) * (ny - 1)
    inside = (xi >= 0) & (xi <= nx - 1) & (yi >= 0) & (yi <= ny - 1)
    ix, iy = np.where(inside, xi, 0).astype(np.int64), np.where(inside, yi, 0).astype(np.int64)
    ntx = (nx + 7) // 8
    key = ((iy >> 3) * ntx + (ix >> 3)) * 64 + (iy & 7) * 8 + (ix & 7)
    return np.where(inside, key, sort_bins(ny, nx) - 1)


def status_flags(status):
    """odr_scan_status: bit k is set when some element has the provisional status 100 + k, 0 <= k < 64."""
    s = np.unique(np.asarray(status, dtype=np.int64))
    flags = 0
    for v in s[(s >= 100) & (s < 164)]:
        flags |= 1 << int(v - 100)
    return flags
