"""CPU: OpenDriftSimulation.get_density_array / get_residence_time around the device call: the edges (the reference's NumPy
expressions on the float32 result arrays, against tests/golden/c32_density.npz), what is handed to the device, and the refusals.
The device call itself is replaced by the host build of csrc/odr_density.hip.h (tests/density_host.py), which has the signature of
opendrift_amd.device.Context.density_map; tests/test_gpu_density.py runs the same cases on the device."""
import numpy as np
import pytest

import density_host as dh
from conftest import golden
from opendrift_amd.oceandrift import OceanDrift, density_edges

CATEGORIES = ['active', 'missing_data', 'stranded']


class HostContext:
    """Stands in for the model's device context: density_map by the host build, every call recorded."""

    def __init__(self):
        self.calls = []

    def density_map(self, lon, lat, z, status, lon_edges, lat_edges, weight=None, stranded_code=-1):
        self.calls.append(dict(weight=weight, stranded_code=stranded_code, lon_edges=lon_edges, lat_edges=lat_edges))
        return dh.density_map(lon, lat, z, status, lon_edges, lat_edges, weight, stranded_code)


@pytest.fixture(scope='module')
def g():
    return golden('c32_density.npz')


def model(g, categories=CATEGORIES, variables=('lon', 'lat', 'z', 'status', 'mass', 'mass_int')):
    o = OceanDrift(loglevel=50)
    o.result = dict(time=list(range(g['lon'].shape[1])), **{k: g[k] for k in variables})
    o.status_categories = list(categories)
    o._ctx = HostContext()
    return o


def test_edges_are_the_reference_expression(g):
    lon_array, lat_array = density_edges(g['lon'], g['lat'], float(g['pixelsize_m']))
    assert lat_array.dtype == g['lat_array'].dtype and np.array_equal(lat_array, g['lat_array'])      # no cosine in the latitude edges
    assert lon_array[0] == g['lon_array'][0]                                                          # nor in the lower longitude edge: deltaLAT
    mid = (np.nanmin(g['lat'].T) + np.nanmax(g['lat'].T)) / 2
    assert mid.dtype == np.float32 and mid == g['mid_latitude_f32']
    if np.cos(np.radians(g['mid_latitude_f32'])) != g['cos_mid_latitude_f32']:
        pytest.skip("np.cos of the float32 mid latitude differs on this host from the golden's (DESIGN.md section 7e): the longitude "
                    'edges, which divide by it, are not compared')
    assert lon_array.dtype == g['lon_array'].dtype and np.array_equal(lon_array, g['lon_array'])


def test_counts_with_golden_bins(g):
    o = model(g)
    bins = (g['lon_array'], g['lat_array'])
    H, Hsub, Hstr, lon_array, lat_array = o.get_density_array(float(g['pixelsize_m']), bins=bins)
    assert np.array_equal(H, g['counts_H']) and np.array_equal(Hsub, g['counts_H_submerged']) and np.array_equal(Hstr, g['counts_H_stranded'])
    assert np.array_equal(lon_array, bins[0]) and np.array_equal(lat_array, bins[1])
    assert o.ctx.calls[-1]['stranded_code'] == 2 and o.ctx.calls[-1]['weight'] is None


def test_no_stranded_category(g):
    o = model(g, categories=CATEGORIES[:2])
    H, Hsub, Hstr, _, _ = o.get_density_array(400.0, bins=(g['lon_array'], g['lat_array']))
    assert o.ctx.calls[-1]['stranded_code'] < 0
    assert not Hstr.any() and np.array_equal(H, g['nostranded_H']) and np.array_equal(Hsub, g['nostranded_H_submerged'])


def test_weight_is_taken_from_the_result(g):
    o = model(g)
    H, Hsub, Hstr, _, _ = o.get_density_array(400.0, weight='mass_int', bins=(g['lon_array'], g['lat_array']))
    assert o.ctx.calls[-1]['weight'] is o.result['mass_int']
    assert np.array_equal(H, g['wint_H']) and np.array_equal(Hsub, g['wint_H_submerged']) and np.array_equal(Hstr, g['wint_H_stranded'])


def test_without_bins_the_edges_are_derived(g):
    o = model(g)
    H, Hsub, Hstr, lon_array, lat_array = o.get_density_array(float(g['pixelsize_m']))
    want = density_edges(g['lon'], g['lat'], float(g['pixelsize_m']))
    assert np.array_equal(lon_array, want[0]) and np.array_equal(lat_array, want[1])
    assert o.ctx.calls[-1]['lon_edges'] is lon_array
    assert H.shape == (6, len(lon_array) - 1, len(lat_array) - 1)
    if np.array_equal(lon_array, g['lon_array']):
        assert np.array_equal(H, g['counts_H'])


def test_residence_time(g, monkeypatch):
    o = model(g)
    monkeypatch.setattr('opendrift_amd.oceandrift.density_edges', lambda lon, lat, pixelsize_m: (g['lon_array'], g['lat_array']))
    res, lon_array, lat_array = o.get_residence_time(float(g['pixelsize_m']))
    assert res.dtype == np.float64 and np.array_equal(res, g['residence'])
    assert np.array_equal(lon_array, g['lon_array']) and np.array_equal(lat_array, g['lat_array'])


def test_missing_variables_raise_keyerror_with_the_name(g):
    o = model(g, variables=('lon', 'lat', 'status', 'mass'))
    with pytest.raises(KeyError, match='z'):
        o.get_density_array(400.0)
    o = model(g, variables=('lon', 'lat', 'z', 'status'))
    with pytest.raises(KeyError, match='mass'):
        o.get_density_array(400.0, weight='mass')
    assert o.ctx.calls == []


def test_before_run_raises_runtimeerror():
    o = OceanDrift(loglevel=50)
    o._ctx = HostContext()
    with pytest.raises(RuntimeError):
        o.get_density_array(400.0)
    with pytest.raises(RuntimeError):
        o.get_residence_time(400.0)


def test_sharded_run_needs_bins(g):
    o = model(g)
    o._world, o._rank = 2, 1
    with pytest.raises(NotImplementedError, match='bins'):
        o.get_density_array(400.0)
    with pytest.raises(NotImplementedError, match='bins'):
        o.get_residence_time(400.0)
    H, _, _, _, _ = o.get_density_array(400.0, bins=(g['lon_array'], g['lat_array']))      # the rank's own rows
    assert np.array_equal(H, g['counts_H'])
