"""PSF photometry of one star over all its epochs = one joint forward-model fit, restated from the
reference's lightcurver/processes/star_photometry.py:23-151 on top of the GPU STARRED mirror.  Same
signature, same in-place rescaling of the inputs (callers plot the rescaled arrays, :47-49), same keys
in the returned dictionary (tests/test_starred_calls/test_starred_calls.py:21-64)."""
import numpy as np

from ..starred.deconvolution.deconvolution import setup_model
from ..starred.deconvolution.loss import Loss
from ..starred.deconvolution.parameters import ParametersDeconv
from ..starred.optim.optimization import Optimizer
from ..starred.utils.noise_utils import propagate_noise
from ..utilities.starred_utilities import get_flux_covariance, get_flux_uncertainties


def prepare_star_epochs(data, noisemap, cosmics_mask):
    """Clean-up of one star's epoch stack before the joint fit, as the reference does it at
    star_photometry.py:309-316: pixels where BOTH data and noise are NaN become (0, 1e7); then every EPOCH
    that contains at least one flagged pixel has its whole noise map multiplied by 1000 (the reference
    indexes epochs there, ``noisemap[np.where(~mask)[0]] *= 1000``, once per epoch: SURVEY.md 8(a) row a5).
    cosmics_mask: True where flagged.  Returns (data, noisemap) as new float64 arrays."""
    data = np.array(data, dtype=np.float64)
    noisemap = np.array(noisemap, dtype=np.float64)
    both_nan = np.isnan(data) & np.isnan(noisemap)
    data[both_nan] = 0.0
    noisemap[both_nan] = 1e7
    good = ~np.asarray(cosmics_mask, dtype=bool)
    flagged_epochs = np.unique(np.where(~good)[0])
    noisemap[flagged_epochs] *= 1000.0
    return data, noisemap


def _border_level(stack):
    """Sky estimate: mean over the four borders of the per-epoch median of the outermost row / column."""
    edges = [stack[:, :1, :], stack[:, :, :1], stack[:, -1:, :], stack[:, :, -1:]]
    with np.errstate(all='ignore'):
        level = np.nanmean([np.nanmedian(e, axis=(1, 2)) for e in edges])
    return float(np.nan_to_num(level, nan=0.0))


def do_one_star_forward_modelling(data, noisemap, psf, subsampling_factor, n_iter=2000,
                                  uniform_background_per_epoch=False, starlet_global_background=True,
                                  marginalize_shifts=False):
    """data, noisemap: (E, n, n) (rescaled IN PLACE by nanmax(data)); psf: (E, P, P) narrow PSFs, any side P
    (joint.place_psf).

    Returns dict: scale, kwargs_final, fluxes, fluxes_uncertainties, chi2, chi2_per_frame, loss_curve,
    residuals, deconvolved_image, starlet_background.  ``marginalize_shifts``: also ``fluxes_uncertainties_marginal`` (E,),
    the 1-sigma of the fluxes marginal over the epochs' translations dx, dy the fit frees (and over ``mean`` where the fit
    had it free); the star's position stays fixed there - it is the gauge of the shifts.
    """
    scale = np.nanmax(data)
    data /= scale
    noisemap /= scale
    variance = noisemap ** 2
    n_epochs = len(data)

    # rough aperture-like flux guess: stamp sum minus the border sky level
    flux_guess = np.nansum(data, axis=(1, 2)) - data[0].size * _border_level(data)
    model, k_init, k_up, k_down, _ = setup_model(data, variance, psf, np.array([0.]), np.array([0.]),
                                                 subsampling_factor, list(flux_guess))

    # what stays fixed: rotation always; background grid and per-epoch constant unless asked for
    fixed = {'kwargs_analytic': {'alpha': k_init['kwargs_analytic']['alpha']},
             'kwargs_background': {}, 'kwargs_sersic': {}}
    if not starlet_global_background:
        fixed['kwargs_background']['h'] = k_init['kwargs_background']['h']
    if not uniform_background_per_epoch:
        fixed['kwargs_background']['mean'] = np.zeros(n_epochs)
    pars = ParametersDeconv(kwargs_init=k_init, kwargs_fixed=fixed, kwargs_up=k_up, kwargs_down=k_down)

    loss_options = dict(data=data, deconv_class=model, param_class=pars, sigma_2=variance,
                        regularization_terms='l1_starlet', regularization_strength_scales=3.0,
                        regularization_strength_hf=3.0, regularization_strength_flux_uniformity=0.)
    if starlet_global_background:
        loss_options['W'] = propagate_noise(model, noisemap, k_init, wavelet_type_list=['starlet'], method='SLIT',
                                            num_samples=200, seed=1, likelihood_type='chi2', verbose=False,
                                            upsampling_factor=subsampling_factor)[0]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loss = Loss(**loss_options)
    optim = Optimizer(loss, pars, method='adabelief')
    optim.minimize(max_iterations=n_iter, min_iterations=None, init_learning_rate=1e-3, schedule_learning_rate=True,
                   restart_from_init=True, stop_at_loss_increase=False, progress_bar=True,
                   return_param_history=True)   # as the reference passes it (:119): recorded on the device, copied only if read
    k_final = pars.best_fit_values(as_kwargs=True)

    residuals = data - np.array(model.model(k_final))
    chi2_per_frame = np.nansum(residuals ** 2 / variance, axis=(1, 2)) / model.image_size ** 2
    sigma_a = get_flux_uncertainties(kwargs=k_final, kwargs_down=k_down, kwargs_up=k_up, data=data,
                                     noisemap=noisemap, model=model)
    scene, background = model.getDeconvolved(k_final, 0)
    extra = {}
    if marginalize_shifts:
        cov = get_flux_covariance(k_final, k_up, k_down, data, noisemap, model, free_shifts=True,
                                  free_mean=bool(uniform_background_per_epoch))
        extra['fluxes_uncertainties_marginal'] = scale * np.sqrt(cov[:, 0, 0])
    return {
        'scale': scale,
        'kwargs_final': k_final,
        'fluxes': scale * np.array(k_final['kwargs_analytic']['a']),
        'fluxes_uncertainties': scale * sigma_a,
        'chi2': float(np.nanmean(chi2_per_frame)),
        'chi2_per_frame': np.array(chi2_per_frame),
        'loss_curve': optim.loss_history,
        'residuals': scale * residuals,
        'deconvolved_image': scale * scene,
        'starlet_background': scale * background,
        **extra,
    }


def do_many_stars_forward_modelling(stacks, subsampling_factor, n_iter=2000, uniform_background_per_epoch=False,
                                    starlet_global_background=False, marginalize_shifts=False):
    """The reference's loop over its reference stars (star_photometry.py:257-326: ``do_one_star_forward_modelling`` once per
    star, each a 2000-iteration fit) as ONE batched device fit (``lightcurver_amd.joint.StarPhotometryBatch``,
    lc_joint_create_groups): every AdaBelief iteration advances all stars with one kernel pair instead of one pair per star.

    stacks: list of (data, noisemap, psf) per star - (E_g, n, n), (E_g, n, n), (E_g, N, N); the epoch counts may differ
    (each star keeps its own frame selection), the stamp size may not.  data and noisemap are rescaled IN PLACE by
    nanmax(data), as the one-star function does.  The two switches are the one-star function's (config.yaml:254-258
    ``star_photometry_uniform_background_per_epoch`` / ``star_photometry_starlet_global_background``; NOTE the defaults here are
    the pipeline's configuration, both off, whereas the one-star function's own default is ``starlet_global_background=True``):

    * both off (the pipeline's default): fluxes, the star's position and the per-epoch shifts free, no background - batched;
    * ``uniform_background_per_epoch=True``: the sky level of every epoch free as well - batched (one more per-epoch
      parameter of the same update);
    * ``starlet_global_background=True``: every star its own background grid with the starlet regulariser (W propagated from
      that star's noise maps, ``lam_scales = lam_hf = 3``) - batched as well (``StarPhotometryBatch(background=True)``,
      lc_joint_create_groups_background) where the stamp size's joint fit has a single-workgroup update: n = 16, 24 (the
      reference's default stamp_size_stars), 32 at subsampling 2 and n = 16 at 1, and the even sizes below 32 embedded in the
      next of these as ``EmbeddedJointFit`` does it (h padded on the way in, cropped on the way out).  Larger stamps (40 - 128
      at subsampling 2, everything above 16 at subsampling 1: multi-block, cluster and matrix-core forms of the one-star fit,
      or a size whose per-star form is not built) run one star after the other through ``do_one_star_forward_modelling`` -
      same numbers, no batching gain.

    Without a background the batch runs at every size the joint fit has: n = 16, 24, 32, 40, 48, 56, 64, 128 at subsampling 1
    and 2, and every other even size up to 128 embedded in the next of these.

    Returns one dictionary per star with ALL keys of ``do_one_star_forward_modelling`` (``deconvolved_image``: the scene of the
    star's first epoch, ``starlet_background``: zeros when no background is fitted - what the reference's caller reads at
    star_photometry.py:139-150); each star's numbers are bit for bit those of its own one-star fit.

    ``marginalize_shifts``: every star's dictionary also gets ``fluxes_uncertainties_marginal`` (E_g,), the 1-sigma of the
    fluxes marginal over the epochs' translations dx, dy the fit frees (and over ``mean`` where
    ``uniform_background_per_epoch`` frees it), the star's position fixed: ``scale * sqrt(C_local[e, 0, 0])`` of
    ``StarPhotometryBatch.fisher_shifts_per_star`` (lc_joint_groups_fisher_shifts, all stars in one call) at the batch's final
    parameters.  One difference from the one-star function: that one polishes the fluxes with 10 L-BFGS-B iterations
    before its Fisher call and the batch does not (lc_joint_run_lbfgs is not available on a batch); with the shifts free
    the information depends on ``a``, so the two agree closely after a converged fit, not bit for bit.  A star with a
    numerically singular epoch has NaN there, and no other star is touched.  Without the switch the dictionaries are
    unchanged and have no such key."""
    from ..joint import StarPhotometryBatch, EmbeddedJointFit, joint_fit_size, background_batch_supported
    from ..starred.deconvolution.deconvolution import nest_kwargs
    ss = int(subsampling_factor)
    if not stacks:
        return []
    shapes = {np.asarray(d).shape[1:] for d, _, _ in stacks}
    n_user = int(np.asarray(stacks[0][0]).shape[-1])
    if shapes != {(n_user, n_user)}:
        raise ValueError(f'every star of a batch needs square stamps of ONE size, got {sorted(shapes)}')
    for d, nm, p in stacks:
        if np.asarray(nm).shape != np.asarray(d).shape or np.asarray(p).shape != (len(d), n_user * ss, n_user * ss):
            raise ValueError('every star needs data, noisemap (E_g, n, n) and psf (E_g, n ss, n ss)')
    # a stamp size without a kernel of its own: the stamps in the centre of the next instantiated size, no weight on the ring
    # (what joint.EmbeddedJointFit does for the one-star fit: the model, and h where it is fitted, cut back to the caller's size)
    n_fit = joint_fit_size(n_user, ss)
    pad = (n_fit - n_user) // 2
    if starlet_global_background and not background_batch_supported(n_fit, ss):
        return [do_one_star_forward_modelling(d, nm, p, ss, n_iter=n_iter, uniform_background_per_epoch=uniform_background_per_epoch,
                                              starlet_global_background=True, marginalize_shifts=marginalize_shifts)
                for d, nm, p in stacks]

    def embed(a, fill, f=1):
        if pad == 0:
            return a
        a = np.asarray(a)
        out = np.full((a.shape[0], n_fit * f, n_fit * f), fill, dtype=a.dtype)
        out[:, pad * f:pad * f + n_user * f, pad * f:pad * f + n_user * f] = a
        return out

    scales, guesses, dev_stacks = [], [], []
    for data, noisemap, psf in stacks:
        scale = np.nanmax(data)
        data /= scale
        noisemap /= scale
        scales.append(scale)
        guesses.append(np.nansum(data, axis=(1, 2)) - data[0].size * _border_level(data))
        dev_stacks.append((embed(data, 0.0), embed(noisemap ** 2, EmbeddedJointFit.RING_VARIANCE), embed(psf, 0.0, ss)))
    bg = bool(starlet_global_background)
    batch = StarPhotometryBatch(dev_stacks, ss, M=1, background=bg)
    try:
        E, G, N = batch.E, batch.G, batch.N
        W = (batch.propagate_noise() if pad == 0 else _embedded_noise_levels(stacks, dev_stacks, ss, pad)) if bg else None
        batch.set_params(a=np.concatenate(guesses), c_x=np.zeros(G), c_y=np.zeros(G), dx=np.zeros(E), dy=np.zeros(E),
                         alpha=np.zeros(E), h=np.zeros(batch.sizes['h']), mean=np.zeros(E))
        # (the one-star function's Loss: starlet l1 at 3 / 3, positivity 0; without the background constants, h fixed at zero)
        batch.set_loss(W=W, lam_scales=3.0, lam_hf=3.0)
        batch.set_free(['a', 'c_x', 'c_y', 'dx', 'dy'] + (['h'] if bg else []) + (['mean'] if uniform_background_per_epoch else []))
        batch.run_adabelief(int(n_iter), init_learning_rate=1e-3, schedule_learning_rate=True)
        final = batch.get_params()
        hist = batch.loss_history()
        P, Nu = pad * ss, n_user * ss
        h_final = [hg.reshape(N, N)[P:P + Nu, P:P + Nu].ravel() for hg in batch.split(final['h'], 'h')] if bg else None
        if bg and pad:
            # the one-star function evaluates its model, uncertainties and scene from the caller-sized kwargs: h back on the
            # device with its ring at zero (EmbeddedJointFit pads what it is given)
            ring0 = np.zeros((G, N, N), np.float32)
            ring0[:, P:P + Nu, P:P + Nu] = np.stack(h_final).reshape(G, Nu, Nu)
            batch.set_params(h=ring0)
        model, _ = batch.model()
        model = model[:, pad:pad + n_user, pad:pad + n_user]
        sigma_a = batch.fisher_flux_sigma()
        # (the shifts free, and mean where the fit had it free, every star's position fixed: C_local [E][Lp][Lp], a_e first)
        marginal = batch.fisher_shifts_per_star(mean=bool(uniform_background_per_epoch))['C_local'] if marginalize_shifts else None
        decon = [batch.deconvolved(int(batch.starts[g])) for g in range(G)]
        scenes = [s[P:P + Nu, P:P + Nu] for s, _ in decon]
        backgrounds = [b[P:P + Nu, P:P + Nu] for _, b in decon]
    finally:
        batch.close()
    out = []
    for g, (data, noisemap, psf) in enumerate(stacks):
        e0, e1 = batch.starts[g], batch.starts[g + 1]
        h_g = np.ascontiguousarray(h_final[g]) if bg else np.zeros((n_user * ss) ** 2, np.float32)
        flat = dict(a=final['a'][e0:e1], c_x=final['c_x'][g:g + 1], c_y=final['c_y'][g:g + 1], dx=final['dx'][e0:e1],
                    dy=final['dy'][e0:e1], alpha=final['alpha'][e0:e1], h=h_g, mean=final['mean'][e0:e1])
        k_final = nest_kwargs(flat)
        residuals = data - model[e0:e1]
        chi2_per_frame = np.nansum(residuals ** 2 / noisemap ** 2, axis=(1, 2)) / data.shape[1] ** 2
        scale = scales[g]
        out.append({
            'scale': scale,
            'kwargs_final': k_final,
            'fluxes': scale * np.array(k_final['kwargs_analytic']['a']),
            'fluxes_uncertainties': scale * sigma_a[e0:e1],
            'chi2': float(np.nanmean(chi2_per_frame)),
            'chi2_per_frame': np.array(chi2_per_frame),
            'loss_curve': np.asarray(hist[g, 1:], dtype=np.float64).tolist(),
            'residuals': scale * residuals,
            'deconvolved_image': scale * np.ascontiguousarray(scenes[g]),
            'starlet_background': scale * (np.ascontiguousarray(backgrounds[g]) if bg else np.zeros((n_user * ss, n_user * ss), np.float32)),
        })
        if marginalize_shifts:
            out[-1]['fluxes_uncertainties_marginal'] = scale * np.sqrt(np.array(marginal[e0:e1, 0, 0], dtype=np.float64))
    return out


def _embedded_noise_levels(stacks, dev_stacks, ss, pad):
    """The starlet noise levels W of every star, (G, J + 1, N, N), of an embedded batch as EmbeddedJointFit.propagate_noise
    has them: from a twin with zero data whose ring sits at each epoch's median variance."""
    from ..joint import StarPhotometryBatch, ring_at_median_variance
    twin = [(np.zeros(np.shape(d), np.float32), ring_at_median_variance(var, np.asarray(noisemap ** 2, dtype=np.float32), pad), p)
            for (_, noisemap, _), (d, var, p) in zip(stacks, dev_stacks)]
    b = StarPhotometryBatch(twin, ss, M=1, background=True)
    try:
        return b.propagate_noise()
    finally:
        b.close()
