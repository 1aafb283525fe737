"""ctypes binding of libuad_hip.so (C-ABI: include/uad_hip.h).  Fails loudly when the library is missing —
there is no CPU / eager fallback anywhere in the product path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('UAD_LIB') or os.path.join(_HERE, 'libuad_hip.so')   # UAD_LIB: A/B builds for kernel tuning

UAD_OK = 0
ARCH_AE, ARCH_VAE, ARCH_CEVAE, ARCH_GMVAE_SPATIAL, ARCH_AE_SPATIAL = 0, 1, 2, 3, 4
BUF_PARAMS, BUF_GRADS, BUF_ADAM_M, BUF_ADAM_V = 0, 1, 2, 3
SEG_DECODER, SEG_BOTTLENECK, SEG_ENCODER, SEG_ENCODER_HI, SEG_ENCODER_LO, SEG_ALL = 0, 1, 2, 3, 4, -1
MATH_F32, MATH_BF16X3, MATH_BF16X3_ALL, MATH_BF16X6 = 0, 1, 2, 3      # (BF16X3_ALL: uad_gan_* handles only; BF16X6: uad_create handles only)

c_float_p = C.c_void_p  # device pointers are passed as integers


class UadConfig(C.Structure):
    _fields_ = [('arch', C.c_int), ('height', C.c_int), ('width', C.c_int), ('channels', C.c_int),
                ('inter_res', C.c_int), ('zdim', C.c_int), ('max_batch', C.c_int),
                ('dim_c', C.c_int), ('dim_z', C.c_int), ('dim_w', C.c_int), ('c_lambda', C.c_float)]


class UadRngJob(C.Structure):
    _fields_ = [('out', C.c_void_p), ('per_sample', C.c_int), ('kind', C.c_int), ('rate', C.c_float), ('stream', C.c_int)]


RNG_NORMAL, RNG_KEEP_MASK = 0, 1


class UadIO(C.Structure):
    _fields_ = [('x', C.c_void_p), ('eps', C.c_void_p), ('mask_mu', C.c_void_p), ('mask_sigma', C.c_void_p),
                ('mask_dec', C.c_void_p), ('x_hat', C.c_void_p), ('l1_map', C.c_void_p), ('z_mu', C.c_void_p),
                ('z_log_sigma', C.c_void_p), ('z_sigma', C.c_void_p), ('scalars', C.c_void_p),
                ('rec_per_sample', C.c_void_p),
                # ceVAE only
                ('x_ce', C.c_void_p), ('mask_mu_ce', C.c_void_p), ('mask_dec_ce', C.c_void_p),
                ('x_hat_ce', C.c_void_p), ('l1_map_ce', C.c_void_p), ('anomaly', C.c_void_p),
                # spatial GMVAE only
                ('eps_w', C.c_void_p), ('eps_z', C.c_void_p), ('w_mu', C.c_void_p), ('w_log_sigma', C.c_void_p),
                ('pc', C.c_void_p)]


class UadGanConfig(C.Structure):
    _fields_ = [('height', C.c_int), ('width', C.c_int), ('channels', C.c_int), ('inter_res', C.c_int), ('zdim', C.c_int),
                ('max_batch', C.c_int), ('scale', C.c_float), ('kappa', C.c_float), ('variant', C.c_int), ('dim', C.c_int),
                ('kl_weight', C.c_float), ('aae_kind', C.c_int), ('rho', C.c_float), ('dim_w', C.c_int), ('c_lambda', C.c_float)]


class UadGanIO(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('x', 'z', 'alpha', 'mask_z', 'mask_g', 'generated', 'reconstruction', 'z_enc',
                                          'l1_map', 'scalars', 'eps', 'mask_sigma', 'eps_w', 'mask_w_mu', 'mask_w_ls', 'x_ce', 'l1_map_ce', 'anomaly')]


ZOOM_CONSTANT, ZOOM_NEAREST = 0, 1
ZOOM_F32, ZOOM_I32 = 0, 1
RESIZE_LINEAR, RESIZE_NEAREST = 0, 1
AFFINE_MAX_K = 16                                                  # include/uad_hip.h: UAD_AFFINE_MAX_K
SELECT_ALL, SELECT_NONNEG = 0, 1
SELECT_MAX_Q, SELECT_TILE, HISTOGRAM_MAX_BINS = 4, 8192, 1024      # include/uad_hip.h: UAD_SELECT_MAX_Q, UAD_SELECT_TILE, UAD_HISTOGRAM_MAX_BINS
HISTOGRAM_MAX_CLASSES, HISTOGRAM_SUM_CHAIN = 4, 1073                # include/uad_hip.h: UAD_HISTOGRAM_MAX_CLASSES, UAD_HISTOGRAM_SUM_CHAIN
SHIFTED_SUMS_CHAIN = 1072                                          # include/uad_hip.h: UAD_SHIFTED_SUMS_CHAIN
GAN_ENCODER, GAN_GENERATOR, GAN_DISCRIMINATOR = 0, 1, 2
GAN_UNIFIED, GAN_RESNET, GAN_ANOVAEGAN, GAN_AAE = 0, 1, 2, 3
GAN_GROUP_VAE = 3
BUF_ADAM_M2, BUF_ADAM_V2 = 4, 5
GAN_SCALARS = ('gen_loss', 'disc_fake', 'disc_real', 'penalty', 'disc_loss', 'loss_img', 'loss_fts', 'enc_loss',
               'reconstructionLoss', 'kl', 'gm_loss', 'gm_con', 'gm_w', 'gm_c')


class UadConvDesc(C.Structure):
    _fields_ = [(k, C.c_int) for k in ('N', 'HB', 'WB', 'CB', 'HS', 'WS', 'CS', 'KS', 'S', 'P')]


class UadXform(C.Structure):
    _fields_ = [('scale', C.c_void_p), ('shift', C.c_void_p), ('alpha', C.c_float)]


class UadGradFinish(C.Structure):
    _fields_ = [('slabs', C.c_void_p), ('S', C.c_int), ('L', C.c_int), ('dW', C.c_void_p),
                ('colpart', C.c_void_p), ('T', C.c_int), ('C', C.c_int), ('gamma', C.c_void_p), ('rstd', C.c_float),
                ('dgamma', C.c_void_p), ('dbeta', C.c_void_p), ('dbias', C.c_void_p),
                ('fin_partial', C.c_void_p), ('fin_T', C.c_int), ('fin_C', C.c_int), ('fin_gamma', C.c_void_p),
                ('dwf', C.c_void_p), ('dbf', C.c_void_p), ('fin_dgamma', C.c_void_p), ('fin_dbeta', C.c_void_p), ('fin_dbias', C.c_void_p),
                ('fin_red', C.c_void_p)]


class UadFinal(C.Structure):
    _fields_ = [('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('C', C.c_int),
                ('c_last', C.c_void_p), ('scale', C.c_void_p), ('shift', C.c_void_p), ('alpha', C.c_float), ('mult', C.c_float),
                ('wf', C.c_void_p), ('bf', C.c_void_p), ('x', C.c_void_p),
                ('x_hat', C.c_void_p), ('l1_map', C.c_void_p), ('rec_partial', C.c_void_p),
                ('d_c', C.c_void_p), ('red_partial', C.c_void_p), ('inv_batch', C.c_float), ('dxhat_in', C.c_void_p)]


class UadGanCritic(C.Structure):
    _fields_ = [('zd', C.c_int), ('h1', C.c_int), ('h2', C.c_int), ('mode', C.c_int), ('hat_mode', C.c_int),
                ('W1', C.c_void_p), ('b1', C.c_void_p), ('W2', C.c_void_p), ('b2', C.c_void_p), ('W3', C.c_void_p), ('b3', C.c_void_p),
                ('zf', C.c_void_p), ('zr', C.c_void_p), ('eps', C.c_void_p), ('inv_n', C.c_float), ('scale', C.c_float),
                ('d_fake', C.c_void_p), ('d_real', C.c_void_p), ('pen', C.c_void_p), ('slab', C.c_void_p), ('dz_fake', C.c_void_p)]


# every symbol include/uad_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'uad_last_error': (C.c_char_p, []),
    'uad_version': (C.c_char_p, []),
    'uad_create': (C.c_int, [C.POINTER(UadConfig), C.POINTER(C.c_void_p)]),
    'uad_destroy': (C.c_int, [C.c_void_p]),
    'uad_param_count': (C.c_longlong, [C.c_void_p]),
    'uad_num_tensors': (C.c_int, [C.c_void_p]),
    'uad_tensor_info': (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_longlong),
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'uad_buffer': (C.c_void_p, [C.c_void_p, C.c_int]),
    'uad_grad_segment': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    'uad_set_params': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong]),
    'uad_get_params': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong]),
    'uad_get_buffer': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]),
    'uad_set_buffer': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]),
    'uad_reset_optimizer': (C.c_int, [C.c_void_p]),
    'uad_get_step': (C.c_longlong, [C.c_void_p]),
    'uad_set_step': (C.c_int, [C.c_void_p, C.c_longlong]),
    'uad_forward': (C.c_int, [C.c_void_p, C.POINTER(UadIO), C.c_int, C.c_int, C.c_void_p]),
    'uad_backward': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'uad_backward_deferred': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    'uad_check_fault': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'uad_rccl_unique_id': (C.c_int, [C.c_void_p, C.c_int]),
    'uad_rccl_comm_create': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'uad_rccl_comm_destroy': (C.c_int, [C.c_void_p]),
    'uad_rccl_allreduce': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    'uad_allreduce_attach': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    'uad_backward_allreduce': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'uad_set_fault_deferred': (C.c_int, [C.c_void_p, C.c_int]),
    'uad_adam_step': (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    'uad_optimizer_step': (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    'uad_train_step': (C.c_int, [C.c_void_p, C.POINTER(UadIO), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_void_p]),
    'uad_restore_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                   C.c_void_p, C.c_void_p]),
    'uad_set_math_mode': (C.c_int, [C.c_void_p, C.c_int]),
    'uad_get_math_mode': (C.c_int, [C.c_void_p]),
    'uad_profile_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'uad_profile_report': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    'uad_residual': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    'uad_gather_slices': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    'uad_gather_mask': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_erode_cross': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_median3d': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_mc_stats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_cc_filter': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_scores_create': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.POINTER(C.c_void_p), C.c_void_p]),
    'uad_scores_auc': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'uad_scores_dice': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    'uad_scores_destroy': (C.c_int, [C.c_void_p]),
    'uad_scores_threshold_at_precision': (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_double)]),
    'uad_cc_label': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_detection_rate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_zoom_spline3_workspace': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'uad_zoom_spline3': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    'uad_affine_spline3_workspace': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'uad_affine_spline3': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'uad_curvature_flow_workspace': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'uad_curvature_flow': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    'uad_resize2d': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_mask_by_label': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'uad_cc_props_workspace': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'uad_cc_props': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_crop2d': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_brain_boxes': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_brain_boxes_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_assemble_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_ulonglong, C.c_ulonglong,
                                     C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_render_minmax_u8': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_render_heatmap': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_render_overlay': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_select_workspace': (C.c_size_t, [C.c_int]),
    'uad_select_quantiles': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.POINTER(C.c_double), C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    'uad_histogram_edges': (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_clamp_scale': (C.c_int, [C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'uad_select_quantiles_masked': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_double), C.c_int, C.c_uint,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'uad_histogram_by_class_workspace': (C.c_size_t, [C.c_longlong]),
    'uad_histogram_by_class': (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    'uad_confusion_by_segment': (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    'uad_shifted_sums_workspace': (C.c_size_t, [C.c_longlong]),
    'uad_shifted_sums': (C.c_int, [C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'uad_clamp_standardize': (C.c_int, [C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'uad_rng_fill': (C.c_int, [C.POINTER(UadRngJob), C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_longlong, C.c_void_p]),
    'uad_clock_probe': (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_void_p]),
    'uad_gan_create': (C.c_int, [C.POINTER(UadGanConfig), C.POINTER(C.c_void_p)]),
    'uad_gan_destroy': (C.c_int, [C.c_void_p]),
    'uad_gan_param_count': (C.c_longlong, [C.c_void_p]),
    'uad_gan_num_tensors': (C.c_int, [C.c_void_p]),
    'uad_gan_tensor_info': (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_longlong),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'uad_gan_buffer': (C.c_void_p, [C.c_void_p, C.c_int]),
    'uad_gan_group': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    'uad_gan_set_buffer': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]),
    'uad_gan_get_buffer': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]),
    'uad_gan_set_math_mode': (C.c_int, [C.c_void_p, C.c_int]),
    'uad_gan_get_step': (C.c_longlong, [C.c_void_p, C.c_int]),
    'uad_gan_set_step': (C.c_int, [C.c_void_p, C.c_int, C.c_longlong]),
    'uad_gan_phase': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(UadGanIO), C.c_int, C.c_int, C.c_void_p]),
    'uad_gan_adam': (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    'uad_gan_allreduce_attach': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    'uad_gan_reconstruct': (C.c_int, [C.c_void_p, C.POINTER(UadGanIO), C.c_int, C.c_void_p]),
    'uad_gan_restore_step': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(UadGanIO), C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'uad_debug_buffer': (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    'uad_debug_plan': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    'uad_k3_profile_enable': (C.c_int, [C.c_int]),
    'uad_k3_profile_read': (C.c_int, [C.c_char_p, C.c_int]),
    'uad_gan_debug_buffer': (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    'uad_op_conv_f': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.POINTER(UadXform), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_conv_d': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.POINTER(UadXform), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_conv_f_bwdact': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(UadXform), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_conv_d_bwdact': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(UadXform), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_conv_w': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.POINTER(UadXform), C.c_void_p,
                                C.POINTER(UadXform), C.c_void_p, C.c_void_p]),
    'uad_op_conv_plan': (C.c_int, [C.POINTER(UadConvDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    'uad_op_conv_d_final': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.POINTER(UadXform), C.c_void_p, C.c_void_p, C.POINTER(UadXform),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_conv_f_final_bwd': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(UadXform), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_conv_first_fwd': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    'uad_op_conv_first_wgrad': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_adam': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_float,
                              C.c_float, C.c_float, C.c_float, C.c_void_p]),
    'uad_op_grad_finish_scratch_floats': (C.c_longlong, []),
    'uad_op_grad_finish': (C.c_int, [C.POINTER(UadGradFinish), C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_final_blocks': (C.c_int, [C.c_int, C.c_int]),
    'uad_op_final': (C.c_int, [C.POINTER(UadFinal), C.c_void_p]),
    'uad_op_reparam_fwd': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 12),
    'uad_op_reparam_bwd': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_loss_finalize': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_conv_first_dgrad_form': (C.c_int, [C.POINTER(UadConvDesc), C.c_int]),
    'uad_op_conv_first_dgrad': (C.c_int, [C.POINTER(UadConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]),
    'uad_op_tv_dxhat': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'uad_op_optim': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_void_p, C.c_void_p]),
    'uad_op_spatial_z_fwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_spatial_z_bwd_blocks': (C.c_int, [C.c_int]),
    'uad_op_spatial_z_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    'uad_op_colsum_scratch_floats': (C.c_longlong, [C.c_int, C.c_int]),
    'uad_op_colsum': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_gan_rows_blocks': (C.c_int, [C.c_int, C.c_int]),
    'uad_op_gan_bn_act_fwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_gan_bn_act_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    'uad_op_gan_rowdot': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_gan_topgrad': (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    'uad_op_gan_coef_colsum': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_gan_gfinal_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    'uad_op_gan_interp': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_gan_flat': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_longlong, C.c_void_p, C.c_void_p]),
    'uad_op_gan_sum_blocks': (C.c_int, []),
    'uad_op_gan_sum': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_gan_pen_col_blocks': (C.c_int, [C.c_int, C.c_int]),
    'uad_op_gan_pen_col': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'uad_op_gan_pen_grad': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_gan_pool': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_gan_flip_taps': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'uad_op_gan_combine': (C.c_int, [C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    'uad_op_gan_critic': (C.c_int, [C.POINTER(UadGanCritic), C.c_int, C.c_void_p]),
}

_lib = None


def load():
    """Load libuad_hip.so and bind every declared symbol.  Raises RuntimeError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: the HIP extension has not been built '
            f'(run `python -m unsupervised_anomaly_detection_brain_mri_amd.build` or __graft_entry__.build()). '
            f'There is no CPU fallback.')
    # PyTorch-ROCm first: libuad_hip.so's HIP runtime dependency must resolve to the copy torch ships and initialises -- loaded on its own before torch, the
    # library binds the system runtime instead and the process then holds two, of which the library's reports "no ROCm-capable device" at the first hipMalloc
    # (seen with `python __graft_entry__.py smoke`, whose build() loads the library before smoke() imports torch)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != UAD_OK:
        msg = load().uad_last_error().decode('utf-8', 'replace')
        if rc in (1, 3):
            raise ValueError(f'uad_hip: {msg}')
        raise RuntimeError(f'uad_hip (code {rc}): {msg}')
