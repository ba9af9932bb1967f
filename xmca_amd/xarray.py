"""`xmca_amd.xarray.xMCA` - drop-in for `xmca.xarray.xMCA` (xmca/xarray.py:23-1488).

A thin facade over `xmca_amd.array.MCA`: the hot path (`solve`, `rotate`, `rule_n`) is inherited unchanged (the
reference's versions are pure pass-throughs, xarray.py:183-238, :1447-1488); every getter re-wraps the numpy result
as an `xarray.DataArray` with the reference's dims / coords / names (1-based `mode`, `time`, `lat`, `lon`, `run`) and
`attrs = str(self._analysis)` items.  xarray (and h5netcdf for IO, cartopy for maps) are imported lazily: they are
not part of the build image, so this module is only exercised where they exist (`pytest.importorskip('xarray')`).
"""
import os

import numpy as np

from . import gaps as _gaps
from . import lagged as _lagged
from . import prepare as _prepare
from . import spectral as _spectral
from .array import MCA, secure_str


def _xr():
    try:
        import xarray as xr
    except Exception as err:        # pragma: no cover - depends on the environment
        raise ImportError("xmca_amd.xarray needs the `xarray` package") from err
    return xr


class xMCA(MCA):
    """MCA / EOF analysis of one or two `xarray.DataArray` (time, lat, lon)."""

    def __init__(self, *fields, handle=None, preprocess=None):
        xr = _xr()
        if len(fields) > 2:
            raise ValueError("Too many fields. Pass 1 or 2 fields.")
        if not all(isinstance(f, xr.DataArray) for f in fields):
            raise TypeError('''One or more fields are not `xarray.DataArray`.
            Please provide `xarray.DataArray` only.''')
        self._field_dims = {}
        self._field_coords = {}
        for key, field in zip(['left', 'right'], fields):
            self._field_dims[key] = field.dims
            self._field_coords[key] = field.coords
        super().__init__(*[f.values for f in fields], handle=handle, preprocess=preprocess)

    # ------------------------------------------------------------------ scaling incl. coslat weights
    def _coslat_weights(self, k):
        coslat = np.sqrt(np.cos(np.deg2rad(self._field_coords[k]['lat']))).values
        weights = np.ones(self._fields_spatial_shape[k]) * coslat.reshape(coslat.size, 1)
        return weights.flatten()[self._no_nan_index[k]]

    def _scale_X(self, data_dict):
        k = None
        for k in data_dict:
            data_dict[k] -= self._field_means[k]
        # normalisation / coslat outside the loop: only the last field, as in the reference (xarray.py:97-108)
        if k is not None and self._analysis['is_normalized']:
            data_dict[k] /= self._field_stds[k]
        if k is not None and self._analysis['is_coslat_corrected']:
            data_dict[k] *= self._coslat_weights(k)
        return data_dict

    def _scale_X_inverse(self, data_dict):
        for k, field in data_dict.items():
            if self._analysis['is_coslat_corrected']:
                field /= self._coslat_weights(k)
            if self._analysis['is_normalized']:
                field *= self._field_stds[k]
            field += self._field_means[k]
        return data_dict

    def _device_column_weights(self, k):
        """The coslat weights of `_scale_X` / `_scale_X_inverse` for the device transforms (see `MCA._device_column_weights`).
        Weights given through `apply_weights` are, as in the reference, part of neither."""
        if not self._analysis['is_coslat_corrected']:
            return None
        w = self._coslat_weights(k)
        return w, w

    def _column_factor(self, k, weight):
        """The factor a time-independent `weight` puts on every kept grid point of field k: `(ones * weight)` over one time step of
        the field's dims / coords - xarray's own `*`, so the broadcasting is the library's - flattened, at the kept points.  None
        when the weight has the field's time dimension, when the product is not of the field's spatial shape (a foreign dimension,
        a mismatch) or for an unknown key: the host route then computes, or raises, as the reference does."""
        xr = _xr()
        if k not in self._field_dims or k not in self._fields_store:
            return None
        dims = self._field_dims[k]
        time_dim = dims[0]
        if time_dim in getattr(weight, 'dims', ()):
            return None
        coords = self._field_coords[k]
        one_step = {d: (np.asarray(getattr(coords[d], 'values', coords[d]))[:1] if d == time_dim else coords[d])
                    for d in dims if d in coords}
        shape = (1,) + tuple(self._fields_spatial_shape[k])
        ones = xr.DataArray(np.ones(shape, dtype=self._fields_store[k].dtype), dims=dims, coords=one_step)
        try:
            product = np.asarray((ones * weight).data)
        except Exception:
            return None
        if product.shape != shape:
            return None
        return product.reshape(-1)[self._no_nan_index[k]]

    def _apply_weights_on_device(self, weights):
        """Time-independent weights on a field that is still resident on the device: one multiply per element there, the host's own
        operation to the bit (`MCA._scale_on_device`, which refuses what it cannot do that way).  False: nothing was changed."""
        if not self._store_is_raw:
            return False
        factors = {k: 1 for k in self._keys}
        for k, weight in weights.items():
            factor = self._column_factor(k, weight)
            if factor is None or factor.dtype != self._fields_store[k].dtype:
                return False
            factors[k] = factor
        return self._scale_on_device(factors, divide=False)

    def apply_weights(self, **weights):
        """Weights as DataArrays broadcastable against the fields (keys `left` / `right`)."""
        if self._apply_weights_on_device(weights):
            return
        fields = self.fields()
        store = self._fields
        for k, weight in weights.items():
            try:
                new = (fields[k] * weight).data
            except KeyError as err:
                raise KeyError('Key `{:}` not found. Please use `left` or `right`'.format(k)) from err
            try:
                new = new.reshape(self._n_observations[k], self._n_variables[k])[:, self._no_nan_index[k]]
            except ValueError as err:
                msg = ('Error for {:} weights. Mismatch between dimensions of weights ({:}) and original field ({:}).')
                raise ValueError(msg.format(k, weight.shape, fields[k].shape)) from err
            store[k] = new
        self._fields = store              # (through the setter: the copy a device may still hold is stale now)

    def apply_coslat(self):
        """Weight by sqrt(cos(lat)) (area weighting on a regular grid)."""
        eps = 1e-6
        self.apply_weights(**{k: np.sqrt(np.cos(np.deg2rad(c['lat'])) + eps) for k, c in self._field_coords.items()})
        self._analysis['is_coslat_corrected'] = True

    # ------------------------------------------------------------------ wrapping helpers
    def _attrs(self):
        return {k: str(v) for k, v in self._analysis.items()}

    def _modes(self, n, length):
        sl = self._get_slice(n)
        return list(range(sl.start + 1, sl.stop + 1))[:length]

    def _mode_array(self, values, n, name):
        xr = _xr()
        return xr.DataArray(values, dims=['mode'], coords={'mode': self._modes(n, len(values))}, name=name,
                            attrs=self._attrs())

    def _time_array(self, key, values, n, what):
        xr = _xr()
        return xr.DataArray(values, dims=['time', 'mode'],
                            coords={'time': self._field_coords[key]['time'], 'mode': self._modes(n, values.shape[1])},
                            name=' '.join([self._field_names[key], what]), attrs=self._attrs())

    def _space_array(self, key, values, n, what):
        xr = _xr()
        c = self._field_coords[key]
        return xr.DataArray(values, dims=['lat', 'lon', 'mode'],
                            coords={'lon': c['lon'], 'lat': c['lat'], 'mode': self._modes(n, values.shape[-1])},
                            name=' '.join([self._field_names[key], what]), attrs=self._attrs())

    # ------------------------------------------------------------------ getters
    def fields(self, original_scale=False):
        xr = _xr()
        out = super().fields(original_scale)
        return {k: xr.DataArray(out[k], dims=self._field_dims[k], coords=self._field_coords[k], name=self._field_names[k])
                for k in self._keys}

    def singular_values(self, n=None):
        return self._mode_array(super().singular_values(n), n, 'singular values')

    def norm(self, n=None, sorted=True):
        return {k: self._mode_array(v, n, ' '.join([self._field_names[k], 'norm']))
                for k, v in super().norm(n=n, sorted=sorted).items()}

    def variance(self, n=None, sorted=True):
        return self._mode_array(super().variance(n, sorted), n, 'variance')

    def explained_variance(self, n=None):
        return self._mode_array(super().explained_variance(n), n, 'covariance fraction')

    def scf(self, n=None):
        return self._mode_array(super().scf(n), n, 'squared covariance fraction')

    def pcs(self, n=None, scaling='None', phase_shift=0, rotated=True):
        return {k: self._time_array(k, v, n, 'pcs') for k, v in super().pcs(n, scaling, phase_shift, rotated).items()}

    def eofs(self, n=None, scaling='None', phase_shift=0, rotated=True):
        return {k: self._space_array(k, v, n, 'eofs') for k, v in super().eofs(n, scaling, phase_shift, rotated).items()}

    def spatial_amplitude(self, n=None, scaling='None', rotated=True):
        return {k: self._space_array(k, v, n, 'spatial amplitude')
                for k, v in MCA.spatial_amplitude(self._plain(), n, scaling, rotated).items()}

    def spatial_phase(self, n=None, phase_shift=0, rotated=True):
        return {k: self._space_array(k, v, n, 'spatial phase')
                for k, v in MCA.spatial_phase(self._plain(), n, phase_shift, rotated).items()}

    def temporal_amplitude(self, n=None, scaling='None', rotated=True):
        return {k: self._time_array(k, v, n, 'temporal amplitude')
                for k, v in MCA.temporal_amplitude(self._plain(), n, scaling, rotated).items()}

    def temporal_phase(self, n=None, phase_shift=0, rotated=True):
        return {k: self._time_array(k, v, n, 'temporal phase')
                for k, v in MCA.temporal_phase(self._plain(), n, phase_shift, rotated).items()}

    def _plain(self):
        """View of this object whose getters return numpy arrays (the base-class implementations call
        self.eofs()/self.pcs(), which are overridden here)."""
        return _NumpyView(self)

    def homogeneous_patterns(self, n=None, phase_shift=0):
        r, p = super().homogeneous_patterns(n, phase_shift)
        return ({k: self._space_array(k, v, n, 'homogeneous patterns') for k, v in r.items()},
                {k: self._space_array(k, v, n, 'pvalues homogeneous patterns') for k, v in p.items()})

    def heterogeneous_patterns(self, n=None, phase_shift=0):
        r, p = super().heterogeneous_patterns(n, phase_shift)
        return ({k: self._space_array(k, v, n, 'heterogeneous patterns') for k, v in r.items()},
                {k: self._space_array(k, v, n, 'pvalues heterogeneous patterns') for k, v in p.items()})

    def reconstructed_fields(self, mode=None, original_scale=True):
        xr = _xr()
        out = super().reconstructed_fields(mode, original_scale)
        return {k: xr.DataArray(v, dims=self._field_dims[k], coords=self._field_coords[k],
                                name='reconstructed_{:}_field'.format(k)) for k, v in out.items()}

    def predict(self, left=None, right=None, n=None, scaling='None', phase_shift=0):
        xr = _xr()
        data = {k: d for k, d in zip(['left', 'right'], [left, right]) if d is not None}
        if not all(isinstance(d, xr.DataArray) for d in data.values()):
            raise TypeError('Data must be `xarray.DataArray`.')
        out = super().predict(left=None if left is None else left.values, right=None if right is None else right.values,
                              n=n, scaling=scaling, phase_shift=phase_shift)
        res = {}
        for k, v in out.items():
            res[k] = xr.DataArray(v, dims=['time', 'mode'],
                                  coords={'time': data[k].coords['time'], 'mode': list(range(1, v.shape[1] + 1))})
        return res

    # ------------------------------------------------------------------ significance
    def rule_north(self, n=None):
        return self._mode_array(super().rule_north(n), n, 'singular values')

    def _run_array(self, values):
        xr = _xr()
        return xr.DataArray(values, dims=['mode', 'run'],
                            coords={'mode': list(range(1, values.shape[0] + 1)), 'run': list(range(1, values.shape[1] + 1))},
                            name='singular values')

    def rule_n(self, n_runs, n_modes=None, **kwargs):
        return self._run_array(super().rule_n(n_runs, n_modes, **kwargs))

    def bootstrapping(self, n_runs, n_modes=20, axis=0, on_left=True, on_right=False, block_size=1, replace=True,
                      strategy='standard', disable_progress=False):
        # like the reference the facade always resamples along time (xarray.py:1418-1419)
        return self._run_array(_NumpyView(self).bootstrapping_base(n_runs, n_modes, 0, on_left, on_right, block_size,
                                                                    replace, strategy, disable_progress))

    def bootstrap_eofs(self, n_runs, n_modes=10, block_size=1, seed=None, indices=None):
        """`MCA.bootstrap_eofs` with 'mean' and 'std' as DataArrays over the dims and coordinates of `eofs(n_modes)`; 'congruence'
        and 'singular_values' (n_modes x n_runs) stay numpy arrays."""
        out = super().bootstrap_eofs(n_runs, n_modes, block_size=block_size, seed=seed, indices=indices)
        out['mean'] = {k: self._space_array(k, v, n_modes, 'bootstrap mean of eofs') for k, v in out['mean'].items()}
        out['std'] = {k: self._space_array(k, v, n_modes, 'bootstrap std of eofs') for k, v in out['std'].items()}
        return out

    def extended_eofs(self, embedding, tau=1, n_modes=10):
        """`MCA.extended_eofs` with 'eofs' as DataArrays with a leading `lag` dimension (coordinate arange(embedding) * tau) in front
        of the dims and coordinates of `eofs(n_modes)`, and 'pcs' as a DataArray over the first T' time coordinates and `mode`;
        'singular_values' and 'explained_variance' stay numpy arrays."""
        xr = _xr()
        out = super().extended_eofs(embedding, tau=tau, n_modes=n_modes)
        key = self._keys[0]
        k = out['pcs'].shape[1]
        lag = np.arange(int(embedding)) * int(tau)
        eofs = {}
        for name, values in out['eofs'].items():
            c = self._field_coords[name]
            eofs[name] = xr.DataArray(values, dims=['lag', 'lat', 'lon', 'mode'],
                                      coords={'lag': lag, 'lon': c['lon'], 'lat': c['lat'], 'mode': self._modes(n_modes, k)},
                                      name=' '.join([self._field_names[name], 'extended eofs']), attrs=self._attrs())
        out['eofs'] = eofs
        time = self._field_coords[key]['time'][:out['pcs'].shape[0]]
        out['pcs'] = xr.DataArray(out['pcs'], dims=['time', 'mode'], coords={'time': time, 'mode': self._modes(n_modes, k)},
                                  name=' '.join([self._field_names[key], 'extended pcs']), attrs=self._attrs())
        return out

    def extended_rule_n(self, embedding, tau=1, n_runs=100, n_modes=10, seed=None, phi=None):
        """`MCA.extended_rule_n`; the dict of numpy arrays is passed through as it is."""
        return super().extended_rule_n(embedding, tau=tau, n_runs=n_runs, n_modes=n_modes, seed=seed, phi=phi)

    def extended_reconstruct(self, embedding, tau=1, mode=None, original_scale=True):
        """`MCA.extended_reconstruct` as DataArrays over the field's own dims and coordinates, like `reconstructed_fields`; with
        `original_scale` the coslat weights are taken out on the device."""
        xr = _xr()
        out = super().extended_reconstruct(embedding, tau=tau, mode=mode, original_scale=original_scale)
        return {k: xr.DataArray(v, dims=self._field_dims[k], coords=self._field_coords[k],
                                name='extended_reconstructed_{:}_field'.format(k)) for k, v in out.items()}

    # ------------------------------------------------------------------ persistence (netCDF through xarray)
    def _save_data(self, data, path, engine='h5netcdf', *args, **kwargs):
        out = os.path.join(path, secure_str('.'.join([data.name, 'nc'])))
        data.to_netcdf(path=out, engine=engine, invalid_netcdf=(engine == 'h5netcdf'), *args, **kwargs)

    def plot(self, *args, **kwargs):
        """see `xmca_amd.array.MCA.plot`"""
        return MCA.plot(self, *args, **kwargs)

    def save_plot(self, *args, **kwargs):
        return MCA.plot(self, *args, **kwargs)

    def save_analysis(self, path=None, engine='h5netcdf'):
        """info.xmca + original-scale real fields, UNROTATED eofs and singular values (xarray.py:1253-1279)."""
        path = self._get_analysis_path(path)
        self._create_analysis_path(path)
        self._create_info_file(path)
        fields = self.fields(original_scale=True)
        eofs = self.eofs(rotated=False)
        self._save_data(self.singular_values(), path, engine)
        for key in self._keys:
            self._save_data(eofs[key], path, engine)
            self._save_data(fields[key].real, path, engine)

    def load_analysis(self, path, engine='h5netcdf'):
        xr = _xr()
        self._set_info_from_file(path)
        folder, _ = os.path.split(path)
        names = self._get_file_names(format='nc')
        singular_values = xr.open_dataarray(os.path.join(folder, names['singular']), engine=engine).data
        fields, eofs = {}, {}
        self._field_coords = {}
        for key in self._field_names.keys():
            eofs[key] = xr.open_dataarray(os.path.join(folder, names['eofs'][key]), engine=engine).data
            f = xr.open_dataarray(os.path.join(folder, names['fields'][key]), engine=engine)
            self._field_coords[key] = f.coords
            self._field_dims[key] = f.dims
            fields[key] = f.data
        MCA.load_analysis(self, path=path, fields=fields, eofs=eofs, singular_values=singular_values)
        if self._analysis['is_coslat_corrected']:
            self.apply_coslat()


def fill_gaps(da, n_modes, max_iter=300, tol=1e-5, cv_fraction=None, cv_idx=None, seed=None, handle=None, embedding=1, tau=1):
    """`xmca_amd.gaps.fill_gaps` of a DataArray whose first dimension is time: the same dict with 'field' as a DataArray over the
    dims, coordinates and attrs of `da`.  `cv_idx` holds flat indices into `da.values.reshape(T, -1)`."""
    xr = _xr()
    if not isinstance(da, xr.DataArray):
        raise TypeError("fill_gaps: the field is not an `xarray.DataArray`")
    out = _gaps.fill_gaps(da.values, n_modes, max_iter=max_iter, tol=tol, cv_fraction=cv_fraction, cv_idx=cv_idx, seed=seed, handle=handle,
                          embedding=embedding, tau=tau)
    out['field'] = xr.DataArray(out['field'], dims=da.dims, coords=da.coords, attrs=dict(da.attrs), name=da.name)
    return out


def anomalies(da, period=None, harmonics=None, trend=False, basis=None, handle=None):
    """`xmca_amd.prepare.anomalies` of a DataArray whose first dimension is time: the same dict as DataArrays - 'field' over the dims,
    coordinates and attrs of `da`, 'coefficients' over ('basis',) + the spatial dims, 'fitted' over the spatial dims, 'basis' over
    (time, 'basis') - each with those coordinates of `da` that lie along its own dims."""
    xr = _xr()
    if not isinstance(da, xr.DataArray):
        raise TypeError("anomalies: the field is not an `xarray.DataArray`")
    out = _prepare.anomalies(da.values, period=period, harmonics=harmonics, trend=trend, basis=basis, handle=handle)
    k = out['basis'].shape[1]

    def along(dims):
        """the coordinates of `da` that lie along `dims`, and the 'basis' index where it is one of them"""
        coords = {name: c for name, c in dict(da.coords).items() if getattr(c, 'dims', ()) and set(c.dims) <= set(dims)}
        if 'basis' in dims:
            coords['basis'] = np.arange(k)
        return coords
    time, spatial = tuple(da.dims[:1]), tuple(da.dims[1:])
    out['field'] = xr.DataArray(out['field'], dims=da.dims, coords=da.coords, attrs=dict(da.attrs), name=da.name)
    out['coefficients'] = xr.DataArray(out['coefficients'], dims=('basis',) + spatial, coords=along(('basis',) + spatial), name='coefficients')
    out['fitted'] = xr.DataArray(out['fitted'], dims=spatial, coords=along(spatial), name='fitted')
    out['basis'] = xr.DataArray(out['basis'], dims=time + ('basis',), coords=along(time + ('basis',)), name='basis')
    return out


def time_filter(da, weights, complement=False, missing='nan', min_weight=0.5, edges='nan', handle=None):
    """`xmca_amd.prepare.time_filter` of a DataArray whose first dimension is time: a DataArray over the dims, coordinates and attrs
    of `da`; with edges='trim' everything along time is sliced [h : T - h], h = (len(weights) - 1) // 2."""
    xr = _xr()
    if not isinstance(da, xr.DataArray):
        raise TypeError("time_filter: the field is not an `xarray.DataArray`")
    out = _prepare.time_filter(da.values, weights, complement=complement, missing=missing, min_weight=min_weight, edges=edges, handle=handle)
    coords = dict(da.coords)
    if edges == 'trim':
        time, h = da.dims[0], (len(weights) - 1) // 2
        for name, c in coords.items():
            dims = tuple(getattr(c, 'dims', ()))
            if time in dims:
                cut = tuple(slice(h, da.shape[0] - h) if d == time else slice(None) for d in dims)
                coords[name] = xr.DataArray(np.asarray(c.values)[cut], dims=dims, name=name, attrs=dict(getattr(c, 'attrs', {})))
    return xr.DataArray(out, dims=da.dims, coords=coords, attrs=dict(da.attrs), name=da.name)


def lead_lag_maps(da, index, lags, min_pairs=8, dof='n', handle=None):
    """`xmca_amd.lagged.lead_lag_maps` of a DataArray whose first dimension is time: the same dict as DataArrays - 'r', 'slope', 'p'
    and 'dof' over ('lag',) + the spatial dims + ('index',), 'pairs' over ('lag',) + the spatial dims, 'lag1' over the spatial dims,
    'lags' over ('lag',) - with `lags` as the 'lag' coordinate and those coordinates of `da` that lie along the spatial dims.
    `index` may be a DataArray over the time dim (and one more dim for several series)."""
    xr = _xr()
    if not isinstance(da, xr.DataArray):
        raise TypeError("lead_lag_maps: the field is not an `xarray.DataArray`")
    if isinstance(index, xr.DataArray):
        index = index.values
    out = _lagged.lead_lag_maps(da.values, index, lags, min_pairs=min_pairs, dof=dof, handle=handle)
    spatial = tuple(da.dims[1:])
    q = out['r'].shape[-1]

    def along(dims):
        coords = {name: c for name, c in dict(da.coords).items() if getattr(c, 'dims', ()) and set(c.dims) <= set(spatial)}
        if 'lag' in dims:
            coords['lag'] = out['lags'].copy()
        if 'index' in dims:
            coords['index'] = np.arange(q)
        return coords
    full = ('lag',) + spatial + ('index',)
    for key in ('r', 'slope', 'p', 'dof'):
        out[key] = xr.DataArray(out[key], dims=full, coords=along(full), name=key)
    out['pairs'] = xr.DataArray(out['pairs'], dims=('lag',) + spatial, coords=along(('lag',) + spatial), name='pairs')
    if 'lag1' in out:
        out['lag1'] = xr.DataArray(out['lag1'], dims=spatial, coords=along(spatial), name='lag1')
    out['lags'] = xr.DataArray(out['lags'], dims=('lag',), coords={'lag': out['lags'].copy()}, name='lags')
    return out


def spectral_maps(da, index=None, nperseg=256, step=None, window='hann', detrend='mean', bins=None, fs=1.0, min_segments=2, handle=None):
    """`xmca_amd.spectral.spectral_maps` of a DataArray whose first dimension is time: the same dict as DataArrays - 'power' over
    ('frequency',) + the spatial dims, 'index_power', 'cospectrum', 'quadrature', 'coherence', 'phase', 'gain' and 'p' over
    ('frequency',) + the spatial dims + ('index',), 'segments' over the spatial dims, 'freqs' and 'bins' over ('frequency',) - with
    'freqs' as the 'frequency' coordinate and those coordinates of `da` that lie along the spatial dims.  `index` may be a DataArray
    over the time dim (and one more dim for several series)."""
    xr = _xr()
    if not isinstance(da, xr.DataArray):
        raise TypeError("spectral_maps: the field is not an `xarray.DataArray`")
    if isinstance(index, xr.DataArray):
        index = index.values
    out = _spectral.spectral_maps(da.values, index, nperseg=nperseg, step=step, window=window, detrend=detrend, bins=bins, fs=fs,
                                  min_segments=min_segments, handle=handle)
    spatial = tuple(da.dims[1:])
    freqs = out['freqs']

    def along(dims):
        coords = {name: c for name, c in dict(da.coords).items() if getattr(c, 'dims', ()) and set(c.dims) <= set(spatial)}
        if 'frequency' in dims:
            coords['frequency'] = freqs.copy()
        if 'index' in dims:
            coords['index'] = np.arange(out['coherence'].shape[-1])
        return coords
    full = ('frequency',) + spatial + ('index',)
    for key in ('index_power', 'cospectrum', 'quadrature', 'coherence', 'phase', 'gain', 'p'):
        if key in out:
            out[key] = xr.DataArray(out[key], dims=full, coords=along(full), name=key)
    out['power'] = xr.DataArray(out['power'], dims=('frequency',) + spatial, coords=along(('frequency',) + spatial), name='power')
    out['segments'] = xr.DataArray(out['segments'], dims=spatial, coords=along(spatial), name='segments')
    for key in ('freqs', 'bins'):
        out[key] = xr.DataArray(out[key], dims=('frequency',), coords={'frequency': freqs.copy()}, name=key)
    return out


class _NumpyView:
    """Delegates attribute access to an xMCA but resolves the public getters to the numpy base-class versions."""

    _BASE = ('eofs', 'pcs', 'spatial_amplitude', 'spatial_phase', 'temporal_amplitude', 'temporal_phase', 'explained_variance',
             'singular_values', 'norm', 'variance', 'fields')

    def __init__(self, obj):
        object.__setattr__(self, '_obj', obj)

    def __getattr__(self, name):
        obj = object.__getattribute__(self, '_obj')
        if name in _NumpyView._BASE:
            return lambda *a, **k: getattr(MCA, name)(self, *a, **k)
        if name == 'bootstrapping_base':
            return lambda *a, **k: MCA.bootstrapping(self, *a, **k)
        return getattr(obj, name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, '_obj'), name, value)
