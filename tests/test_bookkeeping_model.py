"""The NumPy reference of tests/bookkeeping_model.py against plain Python loops that follow the documented contracts one
element at a time: the reference of the GPU tests must not share a mistake with its own vectorisation."""
import numpy as np
import pytest

import bookkeeping_model as bm

RATES = (0.0, 0.01, 0.3, 0.5, 0.99, 1.0)


def _statuses(rng, n, rate):
    codes = np.array([1, 2, 99, 100, 131, 163, 164], dtype=np.int32)
    return np.where(rng.uniform(size=n) < rate, codes[rng.integers(0, codes.size, n)], 0).astype(np.int32)


def _compact_in_place_loop(status):
    """remove the deactivated elements one at a time: walk the holes upwards and the tail downwards"""
    n = len(status)
    kept = sum(1 for s in status if s == 0)
    slot = list(range(n))
    tail = n - 1
    for hole in range(kept):
        if status[hole] == 0:
            continue
        while status[tail] != 0:
            tail -= 1
        slot[hole] = tail
        tail -= 1
    dead = [i for i in range(n) if status[i] != 0]
    return slot[:kept], dead


@pytest.mark.parametrize('rate', RATES)
def test_compaction_models(rate):
    rng = np.random.default_rng(int(rate * 100) + 1)
    for n in list(range(1, 70)) + [255, 256, 257, 1000, 1025]:
        st = _statuses(rng, n, rate)
        src, dead = bm.compact_in_place(st)
        want_src, want_dead = _compact_in_place_loop(list(st))
        assert src.tolist() == want_src and dead.tolist() == want_dead, (n, rate)
        assert sorted(src.tolist() + dead.tolist()) == list(range(n))
        osrc, odead = bm.compact_ordered(st)
        assert osrc.tolist() == [i for i in range(n) if st[i] == 0] and odead.tolist() == want_dead, (n, rate)


def test_compaction_model_worked_example():
    #                 0  1  2  3  4  5  6  7
    st = np.array([0, 5, 0, 7, 0, 0, 9, 0])           # kept = 5: holes 1, 3; fills 7, 5 (from the end)
    src, dead = bm.compact_in_place(st)
    assert src.tolist() == [0, 7, 2, 5, 4] and dead.tolist() == [1, 3, 6]


def test_ranks():
    rng = np.random.default_rng(2)
    for n in (1, 2, 63, 64, 65, 700):
        for top in (n, 4 * n + 7, 2 ** 25):
            ids = rng.choice(top, size=n, replace=False)
            counted = rng.uniform(size=n) < 0.7
            got = bm.ranks(ids, counted)
            present = sorted(int(v) for v, c in zip(ids, counted) if c)
            want = [sum(1 for q in present if q < int(v)) for v in ids]
            assert got.tolist() == want, (n, top)
            assert sorted(got[counted].tolist()) == list(range(int(counted.sum())))


def _key_loop(x, y, lon, lat, lon_mode):
    ny, nx = len(y), len(x)
    if lon_mode == 1:
        lon = (lon + 180.0) % 360.0 - 180.0
    elif lon_mode == 2:
        lon = lon % 360.0
    xi = (lon - float(x[0])) / float(x[-1] - x[0]) * (nx - 1)
    yi = (lat - float(y[0])) / float(y[-1] - y[0]) * (ny - 1)
    if not (0 <= xi <= nx - 1 and 0 <= yi <= ny - 1):
        return bm.sort_bins(ny, nx) - 1
    ix, iy = int(xi), int(yi)
    tiles_per_row = (nx + 7) // 8
    tile = (iy // 8) * tiles_per_row + ix // 8
    return tile * 64 + (iy % 8) * 8 + ix % 8


@pytest.mark.parametrize('lon_mode', [0, 1, 2])
def test_cell_keys(lon_mode):
    rng = np.random.default_rng(3)
    for ny, nx in ((16, 24), (40, 40), (9, 17)):
        x, y = np.arange(nx, dtype=np.float64) + 3.0, 50.0 + 0.5 * np.arange(ny)
        lon = rng.uniform(x[0] - 2, x[-1] + 2, 500)
        lat = rng.uniform(y[0] - 1, y[-1] + 1, 500)
        lon[:4], lat[:4] = [x[0], x[-1], x[-1], x[0]], [y[0], y[-1], y[0], y[-1]]     # the corners are inside
        lon[4:8] += 360.0
        got = bm.cell_keys(x, y, lon, lat, lon_mode=lon_mode)
        want = [_key_loop(x, y, float(a), float(b), lon_mode) for a, b in zip(lon, lat)]
        assert got.tolist() == want
        assert got.max() == bm.sort_bins(ny, nx) - 1 and got.min() >= 0
        assert bm.sort_bins(ny, nx) == 64 * -(-nx // 8) * -(-ny // 8) + 1
    assert (bm.sort_bins(16, 24), bm.sort_bins(40, 40)) == (385, 1601)


def test_status_flags():
    rng = np.random.default_rng(4)
    assert bm.status_flags(np.zeros(5, np.int32)) == 0
    assert bm.status_flags(np.array([99, 164, 1, 2])) == 0
    assert bm.status_flags(np.array([100, 163])) == 1 | 1 << 63
    for _ in range(50):
        st = rng.integers(90, 170, size=rng.integers(1, 40))
        want = 0
        for s in st:
            if 100 <= s < 164:
                want |= 1 << (int(s) - 100)
        assert bm.status_flags(st) == want
