"""ctypes binding of liblcmi.so (C ABI: include/lcmi.h).

There is no CPU fallback: importing this module never fails, but ``lib()`` raises
``RuntimeError`` if the shared library has not been built (``python -c 'import
__graft_entry__ as g; g.build()'`` or ``make -C lightcurver_amd/csrc``), and ``Context()`` raises
if no HIP device is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'liblcmi.so')

P_A, P_CX, P_CY, P_DX, P_DY, P_ALPHA, P_H, P_MEAN, P_COUNT = range(9)
PARAM_INDEX = {'a': P_A, 'c_x': P_CX, 'c_y': P_CY, 'dx': P_DX, 'dy': P_DY, 'alpha': P_ALPHA,
               'h': P_H, 'mean': P_MEAN}

fp = C.POINTER(C.c_float)
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)
vp = C.c_void_p
LBFGS_EVAL = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, dp, dp)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
IPC_HANDLE_BYTES = 64
RCCL_ID_BYTES = 128


class AdabeliefCfg(C.Structure):
    _fields_ = [('init_learning_rate', C.c_float), ('schedule_learning_rate', C.c_int32),
                ('decay_rate', C.c_float), ('transition_steps', C.c_int32),
                ('b1', C.c_float), ('b2', C.c_float), ('eps', C.c_float), ('eps_root', C.c_float)]


class JointLossCfg(C.Structure):
    _fields_ = [('lam_scales', C.c_float), ('lam_hf', C.c_float), ('lam_positivity', C.c_float),
                ('lam_positivity_ps', C.c_float), ('lam_pts_source', C.c_float),
                ('lam_flux_uniformity', C.c_float), ('n_prior', C.c_int32),
                ('prior_cx_mean', fp), ('prior_cx_sigma', fp), ('prior_cy_mean', fp), ('prior_cy_sigma', fp)]


class CosmicsCfg(C.Structure):
    _fields_ = [('sigclip', C.c_float), ('sigfrac', C.c_float), ('objlim', C.c_float), ('gain', C.c_float),
                ('readnoise', C.c_float), ('satlevel', C.c_float), ('niter', C.c_int32), ('sepmed', C.c_int32),
                ('cleantype', C.c_int32), ('fsmode', C.c_int32)]


class CcdmaskCfg(C.Structure):
    _fields_ = [('ncmed', C.c_int32), ('nlmed', C.c_int32), ('lsigma', C.c_float), ('hsigma', C.c_float),
                ('ngood', C.c_int32), ('byblocks', C.c_int32), ('findbadcolumns', C.c_int32)]


class SegmentCfg(C.Structure):
    _fields_ = [('thresh', C.c_float), ('minarea', C.c_int32), ('deblend_nthresh', C.c_int32),
                ('deblend_cont', C.c_float), ('clean_param', C.c_float), ('clean', C.c_int32)]


class StackCfg(C.Structure):
    _fields_ = [('n_sigma', C.c_float), ('clip', C.c_int32)]


class CoaddCfg(C.Structure):
    _fields_ = [('order', C.c_int32), ('combine', C.c_int32), ('n_sigma', C.c_float), ('scratch_rows', C.c_int32)]


COADD_COMBINE = {'mean': 0, 'median': 1, 'sigma_clip': 2}   # LC_COADD_* of include/lcmi.h
COSMICS_APPLY = {None: 0, 'nan': 1, 'clean': 2}             # 0, LC_COSMICS_SET_NAN, LC_COSMICS_SET_CLEAN


class DiffimCfg(C.Structure):
    _fields_ = [('r', C.c_int32), ('bg_degree', C.c_int32), ('gy', C.c_int32), ('gx', C.c_int32),
                ('clip_iters', C.c_int32), ('n_sigma', C.c_float)]


# lc_diffim_out of include/lcmi.h: name -> element type, in the order of the struct
DIFFIM_OUT_FIELDS = (('diff', C.c_float), ('kernel', C.c_double), ('bg', C.c_double), ('scale', C.c_double),
                     ('n_used', C.c_int32), ('chi2', C.c_double), ('status', C.c_int32), ('gram', C.c_double),
                     ('rhs', C.c_double), ('split_ms', C.c_float))


class DiffimOut(C.Structure):
    _fields_ = [(name, C.POINTER(t)) for name, t in DIFFIM_OUT_FIELDS]


class BackgroundCfg(C.Structure):
    _fields_ = [('bw', C.c_int32), ('bh', C.c_int32), ('fw', C.c_int32), ('fh', C.c_int32), ('fthresh', C.c_float)]


class ExtractCfg(C.Structure):
    _fields_ = [('thresh', C.c_float), ('minarea', C.c_int32), ('filter', C.c_int32)]


class DeblendCfg(C.Structure):
    _fields_ = [('deblend_nthresh', C.c_int32), ('deblend_cont', C.c_float), ('clean', C.c_int32),
                ('clean_param', C.c_float)]


class RegisterCfg(C.Structure):
    _fields_ = [('max_matches', C.c_int32), ('pixel_tol', C.c_double), ('invariant_radius', C.c_double),
                ('min_matches_fraction', C.c_double)]


FISHER_POSITIONS, FISHER_MEAN, FISHER_PRIOR = 1, 2, 4   # LC_FISHER_* of include/lcmi.h
FISHER_POSITIONS_FIELDS = ('F_local', 'F_cross', 'F_shared', 'C_local', 'C_cross', 'C_shared', 'sigma_a', 'sigma_mean',
                           'sigma_c')


class FisherPositionsOut(C.Structure):
    _fields_ = [(name, fp) for name in FISHER_POSITIONS_FIELDS]


FISHER_SHIFTS_FIELDS = FISHER_POSITIONS_FIELDS + ('sigma_dx', 'sigma_dy')


class FisherShiftsOut(C.Structure):
    _fields_ = [(name, fp) for name in FISHER_SHIFTS_FIELDS]


class ExtractObject(C.Structure):
    _fields_ = [('first', C.c_int32), ('npix', C.c_int32), ('xmin', C.c_int32), ('xmax', C.c_int32), ('ymin', C.c_int32),
                ('ymax', C.c_int32), ('xpeak', C.c_int32), ('ypeak', C.c_int32), ('flag', C.c_int32), ('pad', C.c_int32),
                ('peak', C.c_float), ('cpeak', C.c_float), ('x', C.c_double), ('y', C.c_double), ('a', C.c_double),
                ('b', C.c_double), ('theta', C.c_double), ('flux', C.c_double)]


# lc_extract_object as a NumPy record: the same 96 bytes
EXTRACT_OBJECT_DTYPE = np.dtype([(n, {C.c_int32: '<i4', C.c_float: '<f4', C.c_double: '<f8'}[t])
                                 for n, t in ExtractObject._fields_])

SEGMENT_MAX_OBJECTS = 32   # LC_SEGMENT_MAX_OBJECTS of include/lcmi.h

# every symbol include/lcmi.h declares: name -> (restype, argtypes)
SIGNATURES = {
    'lc_version': (C.c_int, []),
    'lc_ctx_create': (C.c_int, [C.c_int, C.POINTER(vp)]),
    'lc_ctx_destroy': (None, [vp]),
    'lc_last_error': (C.c_char_p, [vp]),
    'lc_copy_bandwidth': (C.c_int, [vp, C.c_int64, C.c_int, C.POINTER(C.c_float)]),
    'lc_ctx_marker': (C.c_int, [vp, C.c_int]),
    'lc_prepare_stamps': (C.c_int, [vp, C.c_int, C.c_int, fp, fp, fp, fp, fp, C.POINTER(C.c_uint8), C.c_float, C.c_float,
                                    C.c_int, fp, fp, fp, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    'lc_cosmics_supported': (C.c_int, [C.c_int]),
    'lc_detect_cosmics': (C.c_int, [vp, C.c_int, C.c_int, fp, fp, C.POINTER(C.c_uint8), C.POINTER(CosmicsCfg),
                                    C.POINTER(C.c_uint8), fp, ip, C.POINTER(C.c_float)]),
    'lc_ccdmask_supported': (C.c_int, [C.c_int]),
    'lc_ccdmask_stamps': (C.c_int, [vp, C.c_int, C.c_int, fp, C.POINTER(CcdmaskCfg), C.POINTER(C.c_uint8),
                                    C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), fp,
                                    C.POINTER(C.c_float)]),
    'lc_mask_cutouts': (C.c_int, [vp, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.POINTER(CosmicsCfg),
                                  C.POINTER(CcdmaskCfg), C.POINTER(C.c_uint8), C.POINTER(C.c_float)]),
    'lc_segment_supported': (C.c_int, [C.c_int]),
    'lc_segment_stamps': (C.c_int, [vp, C.c_int, C.c_int, fp, fp, C.POINTER(SegmentCfg), C.POINTER(C.c_uint8), ip, ip, fp,
                                    ip, C.POINTER(C.c_float)]),
    'lc_align_stack_supported': (C.c_int, [C.c_int]),
    'lc_align_stack': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, dp, dp, C.POINTER(StackCfg), fp, fp, fp, ip,
                                 C.POINTER(C.c_float)]),
    'lc_background_supported': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'lc_background_frames': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, C.POINTER(C.c_uint8), C.POINTER(BackgroundCfg), fp,
                                       fp, fp, fp, fp, fp, ip, C.POINTER(C.c_float)]),
    'lc_background_map': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(C.c_float)]),
    'lc_extract_supported': (C.c_int, [C.c_int, C.c_int]),
    'lc_extract_frames': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(ExtractCfg), C.c_int, vp, ip, ip,
                                    C.POINTER(C.c_uint8), ip, C.POINTER(C.c_float)]),
    'lc_extract_frames_deblended': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(ExtractCfg),
                                              C.POINTER(DeblendCfg), C.c_int, vp, ip, ip, C.POINTER(C.c_uint8), ip,
                                              C.POINTER(C.c_float)]),
    'lc_import_frames_deblended': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(BackgroundCfg),
                                             C.POINTER(ExtractCfg), C.POINTER(DeblendCfg), C.c_int, C.POINTER(ExtractCfg),
                                             C.c_int, fp, fp, fp, fp, fp, ip, vp, ip, ip, ip, C.POINTER(C.c_float)]),
    'lc_frames_import_deblended': (C.c_int, [vp, fp, C.POINTER(BackgroundCfg), C.POINTER(ExtractCfg), C.POINTER(DeblendCfg),
                                             C.c_int, C.POINTER(ExtractCfg), C.c_int, fp, fp, fp, fp, fp, ip, vp, ip, ip, ip,
                                             C.POINTER(C.c_float)]),
    'lc_import_frames': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(BackgroundCfg), C.POINTER(ExtractCfg),
                                   C.c_int, C.POINTER(ExtractCfg), C.c_int, fp, fp, fp, fp, fp, ip, vp, ip, ip, ip,
                                   C.POINTER(C.c_float)]),
    'lc_frames_create': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, C.POINTER(vp)]),
    'lc_frames_destroy': (None, [vp]),
    'lc_frames_info': (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'lc_frames_get': (C.c_int, [vp, C.c_int, C.c_int, fp]),
    'lc_frames_import': (C.c_int, [vp, fp, C.POINTER(BackgroundCfg), C.POINTER(ExtractCfg), C.c_int, C.POINTER(ExtractCfg),
                                   C.c_int, fp, fp, fp, fp, fp, ip, vp, ip, ip, ip, C.POINTER(C.c_float)]),
    'lc_cutout_supported': (C.c_int, [C.c_int, C.c_int]),
    'lc_frames_cut_stamps': (C.c_int, [vp, C.c_int, C.c_int, ip, ip, ip, fp, fp, C.c_int, C.c_int, C.POINTER(CosmicsCfg),
                                       C.POINTER(CcdmaskCfg), fp, fp, C.POINTER(C.c_uint8), ip, C.POINTER(C.c_float)]),
    'lc_aperture_sums': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(C.c_uint8), C.c_int, ip, dp, dp, dp, dp,
                                   dp, dp, C.POINTER(C.c_float)]),
    'lc_frames_aperture_sums': (C.c_int, [vp, C.c_int, ip, dp, dp, fp, fp, C.c_int, dp, dp, dp, dp, C.POINTER(C.c_float)]),
    'lc_frames_coadd': (C.c_int, [vp, C.c_int, ip, dp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CoaddCfg), fp, fp,
                                  ip, ip, C.POINTER(C.c_float)]),
    'lc_diffim_supported': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'lc_diffim_frames': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(C.c_uint8), fp, C.POINTER(DiffimCfg),
                                   C.POINTER(DiffimOut), C.POINTER(C.c_float)]),
    'lc_frames_subtract_reference': (C.c_int, [vp, C.c_int, ip, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp,
                                               C.POINTER(C.c_uint8), C.POINTER(DiffimCfg), C.c_int, C.POINTER(DiffimOut),
                                               C.POINTER(C.c_float)]),
    'lc_cosmics_frames_supported': (C.c_int, [C.c_int, C.c_int]),
    'lc_detect_cosmics_frames': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(C.c_uint8), C.POINTER(CosmicsCfg),
                                           C.c_int, C.POINTER(C.c_uint8), fp, ip, ip, C.POINTER(C.c_float)]),
    'lc_frames_detect_cosmics': (C.c_int, [vp, C.c_int, ip, fp, fp, C.c_int, C.POINTER(C.c_uint8), C.POINTER(CosmicsCfg),
                                           C.c_int, C.c_int, C.POINTER(C.c_uint8), fp, ip, ip, C.POINTER(C.c_float)]),
    'lc_register_supported': (C.c_int, [C.c_int]),
    'lc_register_sources': (C.c_int, [vp, C.c_int, C.c_int, dp, ip, dp, ip, C.POINTER(RegisterCfg), dp, ip, ip, ip, ip,
                                      C.POINTER(C.c_float)]),
    'lc_ctx_stream': (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    'lc_ctx_synchronize': (C.c_int, [vp]),
    'lc_timer_start': (C.c_int, [vp]),
    'lc_timer_stop': (C.c_int, [vp, fp]),
    'lc_device_info': (C.c_int, [vp, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    'lc_adabelief_defaults': (None, [C.POINTER(AdabeliefCfg)]),
    'lc_psf_supported': (C.c_int, [C.c_int, C.c_int]),
    'lc_psf_batch_create': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(vp)]),
    'lc_psf_batch_destroy': (None, [vp]),
    'lc_psf_batch_set_moffat': (C.c_int, [vp, fp]),
    'lc_psf_batch_get_moffat': (C.c_int, [vp, fp]),
    'lc_psf_batch_set_stars': (C.c_int, [vp, fp]),
    'lc_psf_batch_get_stars': (C.c_int, [vp, fp]),
    'lc_psf_batch_set_grid': (C.c_int, [vp, fp]),
    'lc_psf_batch_get_grid': (C.c_int, [vp, fp]),
    'lc_psf_batch_set_regularization': (C.c_int, [vp, fp, C.c_float, C.c_float]),
    'lc_psf_batch_propagate_noise': (C.c_int, [vp]),
    'lc_psf_batch_get_weights': (C.c_int, [vp, fp]),
    'lc_psf_batch_eval': (C.c_int, [vp, fp, fp, fp, fp, fp, fp]),
    'lc_psf_batch_fit_moffat': (C.c_int, [vp, C.c_int, fp]),
    'lc_psf_batch_run_adabelief': (C.c_int, [vp, C.c_int, C.POINTER(AdabeliefCfg)]),
    'lc_psf_batch_iterations_done': (C.c_int, [vp]),
    'lc_psf_batch_split_fallbacks': (C.c_int, [vp, C.POINTER(C.c_int)]),
    'lc_psf_batch_get_loss_history': (C.c_int, [vp, fp, C.c_int]),
    'lc_psf_batch_get_results': (C.c_int, [vp, fp, fp, fp, fp]),
    'lc_psf_batch_set_moffat_q': (C.c_int, [vp, fp]),
    'lc_psf_batch_set_distortion': (C.c_int, [vp, C.c_int, fp, fp]),
    'lc_psf_distortion_forward': (C.c_int, [vp, vp]),
    'lc_psf_distortion_backward': (C.c_int, [vp, vp]),
    'lc_psf_batch_get_ext_grad': (C.c_int, [vp, fp]),
    'lc_psf_batch_step_adabelief': (C.c_int, [vp, C.POINTER(AdabeliefCfg), C.c_int, C.c_int]),
    'lc_psf_distortion_run': (C.c_int, [vp, vp, C.c_int, C.POINTER(AdabeliefCfg)]),
    'lc_batched_lbfgs': (C.c_int, [C.c_int, C.c_int, dp, dp, dp, C.c_int, LBFGS_EVAL, vp, dp, C.POINTER(C.c_int)]),
    'lc_apply_distortion': (C.c_int, [vp, C.c_int, C.c_int, fp, fp, fp, fp]),
    'lc_joint_supported': (C.c_int, [C.c_int, C.c_int]),
    'lc_joint_groups_background_supported': (C.c_int, [C.c_int, C.c_int]),
    'lc_joint_set_debug_global': (C.c_int, [C.c_int]),
    'lc_joint_create': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(vp)]),
    'lc_joint_create_psf': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(vp)]),
    'lc_joint_create_groups': (C.c_int, [vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(vp)]),
    'lc_joint_create_groups_background': (C.c_int, [vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(vp)]),
    'lc_joint_get_group_loss_history': (C.c_int, [vp, fp, C.c_int]),
    'lc_joint_destroy': (None, [vp]),
    'lc_joint_set_param': (C.c_int, [vp, C.c_int, fp, C.c_int]),
    'lc_joint_get_param': (C.c_int, [vp, C.c_int, fp, C.c_int]),
    'lc_joint_set_flux_reference': (C.c_int, [vp, fp, C.c_int]),
    'lc_joint_get_flux_reference': (C.c_int, [vp, fp, C.c_int]),
    'lc_joint_set_free': (C.c_int, [vp, ip]),
    'lc_joint_set_loss': (C.c_int, [vp, C.POINTER(JointLossCfg), fp]),
    'lc_joint_propagate_noise': (C.c_int, [vp, fp]),
    'lc_joint_loss_grad': (C.c_int, [vp, fp, C.POINTER(fp)]),
    'lc_joint_model': (C.c_int, [vp, fp, fp]),
    'lc_joint_deconvolved': (C.c_int, [vp, C.c_int, fp, fp]),
    'lc_joint_run_adabelief': (C.c_int, [vp, C.c_int, C.POINTER(AdabeliefCfg)]),
    'lc_joint_run_lbfgs': (C.c_int, [vp, C.c_int, C.POINTER(fp), C.POINTER(fp), fp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'lc_joint_get_loss_history': (C.c_int, [vp, fp, C.c_int]),
    'lc_joint_iterations_done': (C.c_int, [vp]),
    'lc_joint_cluster_info': (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'lc_joint_param_history_begin': (C.c_int, [vp, C.c_int, C.POINTER(C.c_int)]),
    'lc_joint_param_history_rows': (C.c_int, [vp]),
    'lc_joint_param_history_get': (C.c_int, [vp, C.c_int, C.c_int, fp]),
    'lc_joint_param_history_end': (C.c_int, [vp]),
    'lc_joint_fisher_flux_sigma': (C.c_int, [vp, fp]),
    'lc_joint_fisher_flux_cov': (C.c_int, [vp, fp, fp, fp]),
    'lc_joint_fisher_positions': (C.c_int, [vp, C.c_int, C.POINTER(FisherPositionsOut)]),
    'lc_joint_fisher_shifts': (C.c_int, [vp, C.c_int, C.POINTER(FisherShiftsOut)]),
    'lc_joint_groups_fisher_shifts': (C.c_int, [vp, C.c_int, C.POINTER(FisherShiftsOut), ip]),
    'lc_joint_step_local': (C.c_int, [vp]),
    'lc_joint_shared_buffer_dev': (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_int)]),
    'lc_joint_step_update': (C.c_int, [vp, C.POINTER(AdabeliefCfg)]),
    'lc_joint_step_grad': (C.c_int, [vp, fp, C.POINTER(fp)]),
    'lc_joint_shared_get': (C.c_int, [vp, fp, C.c_int]),
    'lc_joint_shared_set': (C.c_int, [vp, fp, C.c_int]),
    'lc_joint_run_sharded': (C.c_int, [vp, C.c_int, C.POINTER(AdabeliefCfg), C.c_void_p, vp]),
    'lc_peer_group_create': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    'lc_peer_group_export': (C.c_int, [vp, C.c_void_p, C.c_int]),
    'lc_peer_group_connect': (C.c_int, [vp, C.c_void_p, C.c_int]),
    'lc_peer_allreduce': (C.c_int, [vp, vp, C.c_int, vp]),
    'lc_peer_group_status': (C.c_int, [vp]),
    'lc_peer_group_destroy': (None, [vp]),
    'lc_rccl_available': (C.c_int, []),
    'lc_rccl_unique_id': (C.c_int, [C.c_void_p, C.c_int]),
    'lc_rccl_group_create': (C.c_int, [vp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    'lc_rccl_allreduce': (C.c_int, [vp, vp, C.c_int, vp]),
    'lc_rccl_group_info': (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    'lc_rccl_group_destroy': (None, [vp]),
}

_lib = None


def _share_hip_runtime_with_torch():
    """A process can drive the GPU through ONE HIP runtime.  The PyTorch-ROCm wheel bundles its own
    libamdhip64 / libhsa-runtime64; if liblcmi.so pulled in the system copies first, a later torch.cuda (RCCL
    collectives of the sharded joint fit) would find no device.  So when torch is installed its runtime is
    loaded first and liblcmi.so binds to it (same soname); without torch the system ROCm runtime is used."""
    import importlib.util
    import sys
    if 'torch' in sys.modules:
        return
    spec = importlib.util.find_spec('torch')
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load liblcmi.so and attach the prototypes; raises if the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: the HIP extension has not been built '
                '(run __graft_entry__.build() or make -C lightcurver_amd/csrc). There is no CPU fallback.')
        _share_hip_runtime_with_torch()
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def ptr(a):
    return None if a is None else a.ctypes.data_as(fp)


def adabelief_cfg(init_learning_rate=1e-3, schedule_learning_rate=True, decay_rate=0.99,
                  transition_steps=10, b1=0.9, b2=0.999, eps=1e-16, eps_root=1e-16):
    return AdabeliefCfg(float(init_learning_rate), int(bool(schedule_learning_rate)), float(decay_rate),
                        int(transition_steps), float(b1), float(b2), float(eps), float(eps_root))


class LcError(RuntimeError):
    pass


class Context:
    """One lc_ctx (device + stream).  Raises if no GPU is visible: the product path never falls
    back to the CPU."""

    def __init__(self, device=0):
        self._l = lib()
        h = vp()
        rc = self._l.lc_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise LcError(f'lc_ctx_create failed ({rc}): {self._l.lc_last_error(None).decode()}')
        self.h = h

    def check(self, rc, what=''):
        if rc != 0:
            raise LcError(f'{what} failed ({rc}): {self._l.lc_last_error(self.h).decode()}')

    def synchronize(self):
        self.check(self._l.lc_ctx_synchronize(self.h), 'lc_ctx_synchronize')

    def marker(self, tag):
        """A dispatch with grid size ``tag`` * 64 threads between two synchronisations: cuts a profiler trace into sections."""
        self.check(self._l.lc_ctx_marker(self.h, int(tag)), 'lc_ctx_marker')

    def stream(self):
        """(hipStream_t as int, device ordinal) of this context."""
        p = C.c_void_p()
        d = C.c_int()
        self.check(self._l.lc_ctx_stream(self.h, C.byref(p), C.byref(d)), 'lc_ctx_stream')
        return int(p.value or 0), d.value

    def timer_start(self):
        self.check(self._l.lc_timer_start(self.h), 'lc_timer_start')

    def timer_stop(self):
        ms = C.c_float()
        self.check(self._l.lc_timer_stop(self.h, C.byref(ms)), 'lc_timer_stop')
        return ms.value

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu = C.c_int()
        mem = C.c_int64()
        self.check(self._l.lc_device_info(self.h, name, 256, C.byref(ncu), C.byref(mem)), 'lc_device_info')
        return dict(name=name.value.decode(), n_cu=ncu.value, hbm_bytes=mem.value)

    def close(self):
        if getattr(self, 'h', None):
            self._l.lc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        # (not while the interpreter shuts down: objects are then torn down in no particular order, and destroying a device
        #  object whose context has already gone is a crash at exit; the process is about to return everything anyway)
        try:
            import sys
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
