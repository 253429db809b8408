"""Joint modelling of the ROI cutouts: the arithmetic core of the reference's
lightcurver/processes/roi_modelling.py:198-335 (two-stage fit) and :450-474 (fluxes, uncertainties,
per-frame chi2), restated on the GPU STARRED mirror and taking arrays instead of the HDF5 / WCS /
config plumbing (which stays with the caller: SURVEY.md section 2 rows 6, 16, 17 are out of scope).

Stage 1 (roi_modelling.py:259-282): only the per-epoch translations and fluxes are free, L-BFGS-B,
flux-scatter regularisation.  Stage 2 (:284-335): background (optional), per-epoch constants, fluxes,
astrometry and translations, AdaBelief with the starlet-regularised background.
"""
import warnings
from copy import deepcopy

import numpy as np

from ..starred.deconvolution.deconvolution import setup_model
from ..starred.deconvolution.loss import Loss, Prior
from ..starred.deconvolution.parameters import ParametersDeconv
from ..starred.optim.optimization import Optimizer
from ..starred.utils.noise_utils import propagate_noise
from ..utilities.starred_utilities import _polished_fisher, get_flux_uncertainties, position_covariance_of

DEFAULT_REGULARIZATION = {  # code fall-backs of the reference (roi_modelling.py:273,308-312)
    'regularization_scatter_fluxes_pre_optim': 10.0,
    'regularization_strength_scales': 1.0,
    'regularization_strength_hf': 1.0,
    'regularization_strength_positivity': 100.0,
    'regularization_strength_pts_source': 0.01,
    'regularization_scatter_fluxes_main_optim': 10.0,
}


def _median_stack(data):
    """np.nanmedian(data, axis=0); the NaN-free case (the usual one) takes np.median, an order of magnitude faster than
    numpy's median along a strided axis for (epochs, n, n) stacks (a sort of contiguous rows)."""
    data = np.asarray(data)
    if np.isnan(data).any():
        return np.nanmedian(data, axis=0)
    E = data.shape[0]
    s = np.sort(np.ascontiguousarray(data.reshape(E, -1).T), axis=1)     # pixels x epochs, each row contiguous
    return (0.5 * (s[:, (E - 1) // 2] + s[:, E // 2])).reshape(data.shape[1:])


def initial_point_source_fluxes(data, xs, ys, radius, method='center', ctx=None):
    """Aperture sums on the median stack (roi_modelling.py:198-204 uses photutils' exact circular
    apertures).  ``method='center'``: the pixel-centre version on the host, good enough for a starting point;
    ``'exact'``: the reference's exact circle / pixel overlaps, median stack (``median_stack_batch``) and sums
    (``photutils.aperture_sums_batch``; DESIGN.md section 5 "Aperture sums") both on the device ``ctx``, in float32 data
    with float64 weights.  Bad pixels count as zero in both."""
    if method == 'exact':
        from ..photutils import aperture_sums_batch
        stack = median_stack_batch(np.asarray(data, dtype=np.float32)[None], ctx=ctx)
        xy = np.stack([np.atleast_1d(np.asarray(xs, np.float64)), np.atleast_1d(np.asarray(ys, np.float64))], axis=1)
        return [float(v) for v in aperture_sums_batch(stack, 0, xy, float(radius), ctx=ctx)['sum']]
    if method != 'center':
        raise ValueError(f"initial_point_source_fluxes: method must be 'center' or 'exact', not {method!r}")
    stack = _median_stack(data)
    n = stack.shape[0]
    yy, xx = np.mgrid[0:n, 0:n]
    return [float(np.nansum(stack[(xx - x) ** 2 + (yy - y) ** 2 <= radius ** 2])) for x, y in zip(xs, ys)]


def model_roi_cutouts(data, noisemap, psf, subsampling_factor, xs_pixels, ys_pixels, angles_to_north=None,
                      initial_a=None, aperture_radius=3.0, fix_point_source_astrometry=False,
                      starting_background=None, further_optimize_background=True, regularization=None,
                      roi_deconv_translations_iters=300, roi_deconv_all_iters=2000, rescale=True,
                      marginalize_positions=False, aperture_method='center', marginalize_shifts=False):
    """data, noisemap (E, n, n); psf (E, P, P), any side P (joint.place_psf); xs_pixels, ys_pixels: point-source positions in pixels of
    the first epoch (0-based, as astropy's world_to_pixel returns them).  ``aperture_method``: how the starting fluxes are
    summed where ``initial_a`` is not given (``initial_point_source_fluxes``: 'center', or 'exact' as the reference).

    Returns a dict: kwargs_final, kwargs_stage1, loss_history (stage 2), loss_history_stage1, scale, model,
    and the pieces needed downstream (model object, kwargs_up / kwargs_down).  ``marginalize_positions``: also
    ``astrometry_uncertainties`` = {'c_x_sigma', 'c_y_sigma' (M, data pixels), 'covariance' (2M, 2M; c_x, then c_y)} and
    ``fluxes_sigma`` (E * M, in the units of kwargs_final), from the Fisher information at the final point with the fluxes
    and the positions free (the astrometric prior of the fit included; conditional on dx, dy, alpha and h).
    ``marginalize_shifts``: ``fluxes_sigma`` marginal over the epochs' translations dx, dy, which both stages fit, and
    ``shift_uncertainties`` = {'dx_sigma', 'dy_sigma' (E, data pixels)}; combines with ``marginalize_positions``, which then
    needs the astrometric prior (a float ``fix_point_source_astrometry``: a common translation of the sources is a gauge of
    the shifts).
    """
    if marginalize_positions and isinstance(fix_point_source_astrometry, bool) and fix_point_source_astrometry:
        raise ValueError('marginalize_positions: the positions are fixed (fix_point_source_astrometry=True)')
    if marginalize_positions and marginalize_shifts and not isinstance(fix_point_source_astrometry, float):
        raise ValueError('marginalize_positions with marginalize_shifts needs the astrometric prior '
                         '(fix_point_source_astrometry as a float)')
    reg = dict(DEFAULT_REGULARIZATION)
    reg.update(regularization or {})
    data = np.array(data, dtype=np.float64)
    noisemap = np.array(noisemap, dtype=np.float64)
    scale = float(np.nanmax(data)) if rescale else 1.0
    data /= scale
    noisemap /= scale
    E, n, _ = data.shape
    xs = np.atleast_1d(np.asarray(xs_pixels, dtype=np.float64))
    ys = np.atleast_1d(np.asarray(ys_pixels, dtype=np.float64))
    M = xs.size
    if angles_to_north is None:
        angles = np.zeros(E)
    else:
        angles = np.asarray(angles_to_north, dtype=np.float64) - float(np.asarray(angles_to_north)[0])
    if initial_a is None:
        initial_a = initial_point_source_fluxes(data, xs, ys, aperture_radius, method=aperture_method)
    offset = (n - 1) / 2.0  # STARRED's origin is the stamp centre
    c_x0, c_y0 = xs - offset, ys - offset
    model, k_init, k_up, k_down, _ = setup_model(data, noisemap ** 2, psf, c_x0, c_y0, subsampling_factor,
                                                 E * list(initial_a))
    k_init['kwargs_analytic']['alpha'] = angles

    prior = None
    fix_astrometry = fix_point_source_astrometry
    if isinstance(fix_astrometry, float):
        prior = Prior(prior_analytic=[['c_x', c_x0, np.full(M, fix_astrometry)], ['c_y', c_y0, np.full(M, fix_astrometry)]])
    h_fixed_to_start = starting_background is not None
    if h_fixed_to_start:
        k_init['kwargs_background']['h'] = np.asarray(starting_background, dtype=np.float64).ravel() / scale

    # ---- stage 1: translations + fluxes --------------------------------------------------------------
    fixed = deepcopy(k_init)
    for name in ('dx', 'dy', 'a'):
        del fixed['kwargs_analytic'][name]
    pars = ParametersDeconv(kwargs_init=k_init, kwargs_fixed=fixed, kwargs_up=k_up, kwargs_down=k_down)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loss = Loss(data, model, pars, noisemap ** 2, prior=prior,
                    regularization_strength_flux_uniformity=reg['regularization_scatter_fluxes_pre_optim'])
    optim1 = Optimizer(loss, pars, method='l-bfgs-b')
    optim1.minimize(maxiter=int(roi_deconv_translations_iters))
    k_stage1 = deepcopy(pars.best_fit_values(as_kwargs=True))

    # ---- stage 2: everything (but the rotation) --------------------------------------------------------
    fixed = deepcopy(k_stage1)
    if further_optimize_background:
        del fixed['kwargs_background']['h']
    del fixed['kwargs_background']['mean']
    for name in ('a', 'c_x', 'c_y', 'dx', 'dy'):
        del fixed['kwargs_analytic'][name]
    if isinstance(fix_astrometry, bool) and fix_astrometry:
        fixed['kwargs_analytic']['c_x'] = c_x0
        fixed['kwargs_analytic']['c_y'] = c_y0
    W = propagate_noise(model, noisemap, k_init, wavelet_type_list=['starlet'], method='SLIT', num_samples=500, seed=1,
                        likelihood_type='chi2', verbose=False, upsampling_factor=subsampling_factor)[0]
    pars = ParametersDeconv(kwargs_init=k_stage1, kwargs_fixed=fixed, kwargs_up=k_up, kwargs_down=k_down)
    loss = Loss(data, model, pars, noisemap ** 2, regularization_terms='l1_starlet',
                regularization_strength_scales=reg['regularization_strength_scales'],
                regularization_strength_hf=reg['regularization_strength_hf'],
                regularization_strength_positivity=reg['regularization_strength_positivity'],
                regularization_strength_pts_source=reg['regularization_strength_pts_source'],
                regularization_strength_flux_uniformity=reg['regularization_scatter_fluxes_main_optim'],
                W=W, prior=prior)
    optim2 = Optimizer(loss, pars, method='adabelief')
    optim2.minimize(max_iterations=int(roi_deconv_all_iters), init_learning_rate=1e-4, schedule_learning_rate=False,
                    restart_from_init=False, stop_at_loss_increase=False, progress_bar=True, return_param_history=True)   # as the reference passes it (:331): recorded on the device, copied only if read
    k_final = deepcopy(pars.best_fit_values(as_kwargs=True))
    # position of the sources in the first epoch, back in pixels (roi_modelling.py:339-340)
    x_pix = np.array(k_final['kwargs_analytic']['c_x']) + np.array(k_final['kwargs_analytic']['dx'])[0] + offset
    y_pix = np.array(k_final['kwargs_analytic']['c_y']) + np.array(k_final['kwargs_analytic']['dy'])[0] + offset
    out = dict(kwargs_final=k_final, kwargs_stage1=k_stage1, loss_history=optim2.loss_history,
               loss_history_stage1=optim1.loss_history, scale=scale, model=model, kwargs_up=k_up, kwargs_down=k_down,
               data=data, noisemap=noisemap, x_pixels=x_pix, y_pixels=y_pix, W=W,
               initial_a=[float(v) for v in initial_a])
    if marginalize_positions or marginalize_shifts:
        fisher = _polished_fisher(k_final, k_up, k_down, data, noisemap, model, 0, False, free_positions=marginalize_positions,
                                  prior=prior if marginalize_positions else None, free_shifts=marginalize_shifts)
        sig = fisher.get_kwargs_sigma()['kwargs_analytic']
        if marginalize_positions:
            cov, sx, sy = position_covariance_of(fisher)
            out['astrometry_uncertainties'] = {'c_x_sigma': sx, 'c_y_sigma': sy, 'covariance': cov}
        if marginalize_shifts:
            out['shift_uncertainties'] = {'dx_sigma': np.array(sig['dx'], dtype=np.float64),
                                          'dy_sigma': np.array(sig['dy'], dtype=np.float64)}
        out['fluxes_sigma'] = np.array(sig['a'], dtype=np.float64)
    return out


def model_roi_cutouts_sharded(data, noisemap, psf, subsampling_factor, xs_pixels, ys_pixels, initial_a, scale,
                              group=None, use_peer=False, regularization=None, roi_deconv_translations_iters=300,
                              roi_deconv_all_iters=2000, further_optimize_background=True, ctx=None,
                              return_flux_covariance=False, marginalize_positions=False, marginalize_shifts=False):
    """The two-stage fit of ``model_roi_cutouts`` with the epochs spread over the ranks of a torch.distributed group (one
    process per GPU): every rank passes ITS epochs - data, noisemap (E_local, n, n), psf (E_local, P, P) - and the same
    ``initial_a`` (M fluxes) and ``scale`` (nanmax of the data of ALL epochs: ``global_scale``).  The reference has no
    counterpart (it keeps all epochs on one device, roi_modelling.py:154-160,213); this is what BASELINE configs[4] (1000
    epochs of 128 x 128 over eight GPUs) runs.

    Stage 1: fluxes and translations by L-BFGS-B (``distributed.sharded_lbfgs``: scipy on every rank, the evaluations sharded);
    noise propagation: every rank its epochs, the levels added in quadrature over the ranks; stage 2: AdaBelief on everything
    but the rotation (``ShardedJointOptimizer.run``: the loop in C++, one all-reduce of the shared block per iteration,
    ``use_peer``: by the one-shot peer-memory kernel).  Returns, on every rank, the parameters of ALL epochs (gathered), the
    loss histories and the Fisher 1-sigma of the fluxes at the final point.  ``return_flux_covariance``: also the (E, M, M)
    covariance blocks of the fluxes of all epochs (``fluxes_covariance``: every rank its epochs', gathered in the order of
    ``fluxes_sigma``).  ``marginalize_positions`` is not built here (NotImplementedError): the Schur complement of the
    positions sums over the epochs of all ranks; ``marginalize_shifts`` neither."""
    if marginalize_positions:
        raise NotImplementedError('marginalize_positions in the sharded ROI fit: the Schur sum crosses the ranks')
    if marginalize_shifts:
        raise NotImplementedError('marginalize_shifts is not built in the sharded ROI fit')
    import torch
    import torch.distributed as dist
    from ..distributed import PeerGroup, ShardedJointOptimizer, gather_epoch_blocks, host_group
    from ..joint import make_joint_fit
    from .. import _lib
    reg = dict(DEFAULT_REGULARIZATION)
    reg.update(regularization or {})
    data = np.array(data, dtype=np.float64) / scale
    noisemap = np.array(noisemap, dtype=np.float64) / scale
    E, n, _ = data.shape
    xs = np.atleast_1d(np.asarray(xs_pixels, dtype=np.float64))
    ys = np.atleast_1d(np.asarray(ys_pixels, dtype=np.float64))
    M, ss = xs.size, int(subsampling_factor)
    offset = (n - 1) / 2.0
    # (a stamp size without an epoch kernel of its own is fitted embedded in the next one, on every rank alike)
    fit = make_joint_fit(data, noisemap ** 2, psf, ss, M, ctx or _lib.default_context())
    peer = None
    try:
        fit.set_params(a=np.tile(np.asarray(initial_a, np.float64) / scale, E), c_x=xs - offset, c_y=ys - offset, dx=np.zeros(E),
                       dy=np.zeros(E), alpha=np.zeros(E), h=np.zeros((n * ss) ** 2), mean=np.zeros(E))
        peer = PeerGroup(fit, group) if use_peer else None
        opt = ShardedJointOptimizer(fit, group, peer=peer)
        # ---- stage 1: translations + fluxes (roi_modelling.py:259-282) ----------------------------------------------
        fit.set_loss(lam_flux_uniformity=reg['regularization_scatter_fluxes_pre_optim'])
        half = n / 2.0
        hist1, _ = opt.run_lbfgs(['a', 'dx', 'dy'], int(roi_deconv_translations_iters), lower={'a': 0.0, 'dx': -half, 'dy': -half},
                                 upper={'dx': half, 'dy': half})
        # ---- noise levels of the starlet coefficients: the epochs add in quadrature, over the ranks too -----------------
        W2 = torch.from_numpy(np.square(fit.propagate_noise().astype(np.float64)))
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            if dist.get_backend(group) == 'nccl':
                W2 = W2.to(torch.device('cuda', fit.ctx.stream()[1]))
            dist.all_reduce(W2, op=dist.ReduceOp.SUM, group=group)
            W2 = W2.cpu()
        W = np.sqrt(W2.numpy())
        # ---- stage 2: everything but the rotation (roi_modelling.py:284-335) -------------------------------------------
        fit.set_loss(W=W, lam_scales=reg['regularization_strength_scales'], lam_hf=reg['regularization_strength_hf'],
                     lam_positivity=reg['regularization_strength_positivity'],
                     lam_pts_source=reg['regularization_strength_pts_source'],
                     lam_flux_uniformity=reg['regularization_scatter_fluxes_main_optim'])
        fit.set_free(['a', 'c_x', 'c_y', 'dx', 'dy', 'mean'] + (['h'] if further_optimize_background else []))
        opt.run(int(roi_deconv_all_iters), init_learning_rate=1e-4, schedule_learning_rate=False)
        fit.ctx.synchronize()
        final = gather_epoch_blocks(fit.get_params(), M, group)
        sigma_loc = np.asarray(fit.fisher_flux_sigma(), np.float64)
        cov_loc = np.asarray(fit.fisher_flux_covariance()[1], np.float64) if return_flux_covariance else None
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            parts = [None] * dist.get_world_size(group)
            dist.all_gather_object(parts, (sigma_loc, cov_loc), group=host_group(group))
            sigma = np.concatenate([s for s, _ in parts])
            cov = np.concatenate([c for _, c in parts]) if return_flux_covariance else None
        else:
            sigma, cov = sigma_loc, cov_loc
        # (the entry lc_joint_get_loss_history appends for the final parameters is a local evaluation: dropped)
        out = dict(flat_final=final, loss_history=np.asarray(fit.loss_history(), np.float64)[:-1], loss_history_stage1=hist1,
                   fluxes_sigma=sigma, scale=scale, W=W)
        if return_flux_covariance:
            out['fluxes_covariance'] = cov
        return out
    finally:
        # (errors of the sharded stages are agreed over the ranks before they are raised - distributed.raise_together - so every
        #  rank arrives here, and the bounded host barrier inside peer.close() finds its partners)
        if peer is not None:
            peer.close()
        fit.close()


def global_scale(data, group=None):
    """nanmax of the data over the epochs of all ranks (what ``model_roi_cutouts`` divides by, roi_modelling.py:176)."""
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(np.nanmax(data))], dtype=torch.float64)
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        if dist.get_backend(group) == 'nccl':
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return float(t[0])


def fluxes_from_model(model, kwargs, kwargs_up, kwargs_down, data, noisemap, n_sources, model_scale,
                      normalization_errors, marginalize_positions=False, prior=None, marginalize_shifts=False):
    """Numeric part of get_fluxes_dataframe_from_model (roi_modelling.py:450-474): per-source light
    curves (a is epoch-major: curve i = a[i::M]), their uncertainties (Fisher 1-sigma compounded with the
    frame normalisation error), residuals and the per-frame reduced chi2.  ``marginalize_positions``: the photon error is
    the marginal one with the fluxes and the positions c_x, c_y free (``prior``: the fit's ``Prior`` on them), and the
    result gains ``astrometry_uncertainties`` = {'c_x_sigma', 'c_y_sigma', 'covariance'} (data pixels).
    ``marginalize_shifts``: the photon error is marginal over the epochs' translations dx, dy (too; the positions beside
    them need the ``prior``), and the result gains ``shift_uncertainties`` = {'dx_sigma', 'dy_sigma'} (data pixels)."""
    a = np.array(kwargs['kwargs_analytic']['a'])
    astrometry = shifts = None
    if marginalize_positions or marginalize_shifts:
        fisher = _polished_fisher(kwargs, kwargs_up, kwargs_down, data, noisemap, model, 10, False,
                                  free_positions=marginalize_positions, prior=prior if marginalize_positions else None,
                                  free_shifts=marginalize_shifts)
        sig = fisher.get_kwargs_sigma()['kwargs_analytic']
        sigma_a = np.array(sig['a'], dtype=np.float64)
        if marginalize_positions:
            cov, sx, sy = position_covariance_of(fisher)
            astrometry = {'c_x_sigma': sx, 'c_y_sigma': sy, 'covariance': cov}
        if marginalize_shifts:
            shifts = {'dx_sigma': np.array(sig['dx'], dtype=np.float64), 'dy_sigma': np.array(sig['dy'], dtype=np.float64)}
    else:
        sigma_a = np.array(get_flux_uncertainties(kwargs=kwargs, kwargs_up=kwargs_up, kwargs_down=kwargs_down,
                                                  data=data, noisemap=noisemap, model=model))
    norm_err = np.asarray(normalization_errors, dtype=np.float64)
    curves, d_curves = [], []
    for i in range(n_sources):
        curve = a[i::n_sources] * model_scale
        photon = sigma_a[i::n_sources] * model_scale
        curves.append(curve)
        d_curves.append(np.sqrt(photon ** 2 + (norm_err * curve) ** 2))
    residuals = data - model.model(kwargs)
    chi2_per_frame = np.nansum(residuals ** 2 / noisemap ** 2, axis=(1, 2)) / model.image_size ** 2
    out = dict(fluxes=np.array(curves), d_fluxes=np.array(d_curves), residuals=residuals,
               reduced_chi2=np.array(chi2_per_frame))
    if astrometry is not None:
        out['astrometry_uncertainties'] = astrometry
    if shifts is not None:
        out['shift_uncertainties'] = shifts
    return out


# ---- diagnostics of roi_modelling.py:34-125 ---------------------------------------------
def align_data_interpolation(array, starred_kwargs):
    """De-translate and de-rotate every epoch with the fitted dx, dy, alpha (spline interpolation, for
    diagnostics only; reference roi_modelling.py:34-57: shift by (-dy, -dx), then rotate by +alpha degrees)."""
    from scipy.ndimage import rotate, shift
    ka = starred_kwargs['kwargs_analytic']
    return np.array([rotate(shift(img, (-ddy, -ddx)), ang, reshape=False)
                     for img, ddx, ddy, ang in zip(array, ka['dx'], ka['dy'], ka['alpha'])])


def sigma_clipped_weighted_stack(data, noisemap, n_sigma=3.0):
    """Average stack with one pass of rejection around the per-pixel median (threshold n_sigma standard
    deviations) and weights 1 / noise: what the reference obtains from ccdproc's Combiner
    (roi_modelling.py:60-83), written out since ccdproc is not a dependency here."""
    data = np.asarray(data, dtype=np.float64)
    weights = 1.0 / np.asarray(noisemap, dtype=np.float64)
    med = _median_stack(data)
    dev = np.nanstd(data, axis=0)
    keep = np.abs(data - med) <= n_sigma * dev
    keep |= ~np.isfinite(dev)[None]
    w = np.where(keep & np.isfinite(data), weights, 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.nansum(w * np.nan_to_num(data), axis=0) / np.sum(w, axis=0)


def align_stack_batch(cubes, noisemap=None, shift_yx=None, angle_deg=None, n_sigma=3.0, clip=True, want=('stack',),
                      ctx=None):
    """One call of ``lc_align_stack`` (include/lcmi.h; the SPEC of DESIGN.md §5 "Align and stack") on C cubes (C, E, n, n),
    8 <= n <= 128, that share a noise map (E, n, n).  shift_yx (E, 2) and angle_deg (E,): scipy's ``shift`` and ``rotate``
    arguments per epoch; both None: no alignment.  want: which of 'aligned' (C, E, n, n), 'stack', 'median' (C, n, n) float32
    and 'n_rejected' (C, n, n) int32 to compute and return, next to 'kernel_ms'.  There is no CPU fallback."""
    import ctypes as C
    from .. import _lib
    ctx = ctx or _lib.default_context()
    lib = _lib.lib()
    v = _lib.f32(cubes)
    if v.ndim != 4 or v.shape[2] != v.shape[3]:
        raise ValueError(f'expected (C, E, n, n) cubes of square stamps, got {v.shape}')
    nc, E, n = v.shape[0], v.shape[1], v.shape[2]
    unknown = set(want) - {'aligned', 'stack', 'median', 'n_rejected'}
    if unknown:
        raise ValueError(f'unknown outputs {sorted(unknown)}')
    s = None
    if noisemap is not None:
        s = _lib.f32(noisemap)
        if s.shape != v.shape[1:]:
            raise ValueError(f'the noise map must be (E, n, n) = {v.shape[1:]}, got {s.shape}')
    sh = ang = None
    if shift_yx is not None or angle_deg is not None:
        sh = np.ascontiguousarray(shift_yx, dtype=np.float64)
        ang = np.ascontiguousarray(angle_deg, dtype=np.float64)
        if sh.shape != (E, 2) or ang.shape != (E,):
            raise ValueError(f'expected shifts (E, 2) and angles (E,), got {sh.shape} and {ang.shape}')
    out = {}
    if 'aligned' in want:
        out['aligned'] = np.empty(v.shape, np.float32)
    for name in ('stack', 'median'):
        if name in want:
            out[name] = np.empty((nc, n, n), np.float32)
    if 'n_rejected' in want:
        out['n_rejected'] = np.empty((nc, n, n), np.int32)
    cfg = _lib.StackCfg(float(n_sigma), int(bool(clip)))
    ms = C.c_float()
    dptr = lambda a: None if a is None else a.ctypes.data_as(_lib.dp)
    rej = out.get('n_rejected')
    ctx.check(lib.lc_align_stack(ctx.h, nc, E, n, _lib.ptr(v), _lib.ptr(s), dptr(sh), dptr(ang), C.byref(cfg),
                                 _lib.ptr(out.get('aligned')), _lib.ptr(out.get('stack')), _lib.ptr(out.get('median')),
                                 None if rej is None else rej.ctypes.data_as(_lib.ip), C.byref(ms)), 'lc_align_stack')
    out['kernel_ms'] = ms.value
    return out


def _alignment_of(starred_kwargs):
    """scipy's arguments of ``align_data_interpolation`` per epoch: shift (-dy, -dx), rotation +alpha degrees."""
    ka = starred_kwargs['kwargs_analytic']
    dx, dy = np.asarray(ka['dx'], dtype=np.float64), np.asarray(ka['dy'], dtype=np.float64)
    return np.stack([-dy, -dx], axis=1), np.asarray(ka['alpha'], dtype=np.float64)


def align_data_interpolation_batch(arrays, starred_kwargs, ctx=None):
    """``align_data_interpolation`` of every (E, n, n) cube of ``arrays`` (C, E, n, n) in one device call (float32)."""
    shift_yx, angle = _alignment_of(starred_kwargs)
    return align_stack_batch(arrays, None, shift_yx, angle, want=('aligned',), ctx=ctx)['aligned']


def median_stack_batch(cubes, ctx=None):
    """np.nanmedian over the epochs of every (E, n, n) cube of ``cubes`` (C, E, n, n) on the device (float32, exact order
    statistics; an infinite sample counts as missing, like a NaN): what ``_median_stack`` computes on the host."""
    return align_stack_batch(cubes, want=('median',), ctx=ctx)['median']


def stack_data_diagnostic(data, noisemap, starred_kwargs, starred_model, on_device=False, ctx=None):
    """Three aligned stacks: the data, the data minus the point sources, the data minus the background
    (reference roi_modelling.py:86-125).  Two extra forward models on the device; alignment and stacking on the host, or
    with ``on_device`` in one ``lc_align_stack`` call over the three cubes (float32 stacks, no CPU fallback)."""
    only_ps = deepcopy(starred_kwargs)
    only_ps['kwargs_background']['h'] = np.array(only_ps['kwargs_background']['h']) * 0.0
    no_ps = deepcopy(starred_kwargs)
    no_ps['kwargs_analytic']['a'] = np.array(no_ps['kwargs_analytic']['a']) * 0.0
    data = np.asarray(data, dtype=np.float64)
    if on_device:
        cubes = np.stack([data, data - starred_model.model(only_ps), data - starred_model.model(no_ps)])
        shift_yx, angle = _alignment_of(starred_kwargs)
        st = align_stack_batch(cubes, noisemap, shift_yx, angle, want=('stack',), ctx=ctx)['stack']
        return {'stack': st[0], 'stack_no_ps': st[1], 'stack_no_background': st[2]}
    minus_ps = align_data_interpolation(data - starred_model.model(only_ps), only_ps)
    minus_bg = align_data_interpolation(data - starred_model.model(no_ps), no_ps)
    aligned = align_data_interpolation(data, starred_kwargs)
    return {'stack': sigma_clipped_weighted_stack(aligned, noisemap),
            'stack_no_ps': sigma_clipped_weighted_stack(minus_ps, noisemap),
            'stack_no_background': sigma_clipped_weighted_stack(minus_bg, noisemap)}
