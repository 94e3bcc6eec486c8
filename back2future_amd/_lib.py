"""ctypes binding of libb2f.so (include/b2f.h).  There is no CPU fallback: if the HIP
library is missing or no GPU is present, calls fail loudly."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# B2F_LIB: profiling builds of the same library (tools/build_variant.py), never a different backend
SO_PATH = os.environ.get("B2F_LIB") or os.path.join(_HERE, "libb2f.so")
_lib = None

c_float_p = C.POINTER(C.c_float)


class LossGradOpts(C.Structure):
    """b2f_loss_grad_opts of include/b2f.h: the option weights of opts.lua:61-73, the level weights of test.lua:29-31, sizeAverage"""
    _fields_ = [("smooth_flow", C.c_double), ("const_vel", C.c_double), ("pme", C.c_double), ("smooth_occ", C.c_double),
                ("prior_occ", C.c_double), ("level_weights", C.c_double * 7), ("size_average", C.c_int)]


c_grad_opts_p = C.POINTER(LossGradOpts)


class LossGradFtOpts(C.Structure):
    """b2f_loss_grad_ft_opts of include/b2f.h: the fields of LossGradOpts, -smooth_second_order, -pme_criterion (0 OBCC, 1 OBGCC) and
    OBGCCriterion's alpha, beta, gamma"""
    _fields_ = LossGradOpts._fields_ + [("smooth_second_order", C.c_int), ("pme_criterion", C.c_int), ("pme_alpha", C.c_double),
                                        ("pme_beta", C.c_double), ("pme_gamma", C.c_double)]


c_grad_ft_opts_p = C.POINTER(LossGradFtOpts)


class LossGradSsimOpts(C.Structure):
    """b2f_loss_grad_ssim_opts of include/b2f.h: the fields of LossGradOpts, -smooth_second_order and the alpha of
    OSSIML1Criterion (1: OSSIM, 0.85: OSSIML1)"""
    _fields_ = LossGradOpts._fields_ + [("smooth_second_order", C.c_int), ("ssim_alpha", C.c_double)]


c_grad_ssim_opts_p = C.POINTER(LossGradSsimOpts)


class LossGradPlainOpts(C.Structure):
    """b2f_loss_grad_plain_opts of include/b2f.h: the fields of LossGradOpts, -smooth_second_order, the criterion (0 BCC, 1 SSIM), the
    penalty (0 L1, 1 quadratic; BCC only) and the alpha of MSSIML1Criterion (1: SSIM, 0.85: SSIML1)"""
    _fields_ = LossGradOpts._fields_ + [("smooth_second_order", C.c_int), ("criterion", C.c_int), ("penalty", C.c_int), ("ssim_alpha", C.c_double)]


c_grad_plain_opts_p = C.POINTER(LossGradPlainOpts)


class LossEpeOpts(C.Structure):
    """b2f_loss_epe_opts of include/b2f.h: -epe, the weight of the opt-in occlusion term (train.lua:316-332), -sizeAverage and the
    level weights of train.lua:56-58"""
    _fields_ = [("epe", C.c_double), ("occ", C.c_double), ("size_average", C.c_int), ("level_weights", C.c_double * 7)]


c_epe_opts_p = C.POINTER(LossEpeOpts)

# name -> (restype, argtypes); must list every symbol include/b2f.h declares
SIGNATURES = {
    "b2f_last_error": (C.c_char_p, []),
    "b2f_version": (C.c_int, []),
    "b2f_init": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "b2f_init_ex": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]),
    "b2f_destroy": (None, [C.c_void_p]),
    "b2f_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                           C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "b2f_param_count": (C.c_longlong, [C.c_int]),
    "b2f_random_weights": (C.c_int, [C.c_ulonglong, C.c_int, C.c_float, c_float_p, C.c_longlong]),
    "b2f_set_weights": (C.c_int, [C.c_void_p, c_float_p, C.c_longlong]),
    "b2f_get_weights": (C.c_int, [C.c_void_p, c_float_p, C.c_longlong]),
    "b2f_weights_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    "b2f_commit_weights": (C.c_int, [C.c_void_p]),
    "b2f_load_t7": (C.c_int, [C.c_char_p, c_float_p, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "b2f_load_t7_ex": (C.c_int, [C.c_char_p, C.c_char_p, c_float_p, C.c_longlong, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]),
    "b2f_compute_flow": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, C.c_int, C.c_int,
                                   C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, C.c_int, C.c_int,
                                         C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_batch_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                            C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(C.c_double),
                                            C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_forward_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_forward_sequence_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_compute_flow_sequence": (C.c_int, [C.c_void_p, C.c_int, c_float_p, C.c_int, C.c_int,
                                            C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_sequence_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                               C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence": (C.c_int, [C.c_void_p, C.c_int, c_float_p, C.c_int, C.c_int,
                                                  C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                                                     C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_batch_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_sequence_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_batch_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.c_int, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                      c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_compute_flow_sequence_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_flow_rgb_host": (C.c_int, [c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_ubyte),
                                    C.POINTER(C.c_double)]),
    "b2f_flow_rgb_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "b2f_op_flow_rgb": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_ubyte),
                                  C.POINTER(C.c_double)]),
    "b2f_compute_flow_batch_rgb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_double, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_double), c_float_p,
                                             C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_sequence_rgb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                C.c_double, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_double), c_float_p,
                                                C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_batch_rgb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                   C.c_double, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_double), c_float_p,
                                                   C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence_rgb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                      C.c_double, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_double), c_float_p,
                                                      C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_stream_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "b2f_stream_close": (None, [C.c_void_p]),
    "b2f_stream_reset": (C.c_int, [C.c_void_p]),
    "b2f_stream_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_longlong)]),
    "b2f_stream_push": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                  C.POINTER(C.c_int)]),
    "b2f_stream_push_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_double), c_float_p,
                                      C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(C.c_int)]),
    "b2f_stream_push_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int)]),
    "b2f_stream_open_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "b2f_stream_flags": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "b2f_stream_push_warp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p,
                                       C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), c_float_p, C.POINTER(C.c_int)]),
    "b2f_stream_push_warp_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "b2f_stream_push_past": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                       C.POINTER(C.c_int)]),
    "b2f_stream_push_past_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int)]),
    "b2f_flow_score_host": (C.c_int, [c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_float_p, C.POINTER(C.c_ubyte),
                                      C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)]),
    "b2f_flow_score_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_op_flow_score": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_float_p, C.POINTER(C.c_ubyte),
                                    C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)]),
    "b2f_compute_flow_batch_score": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_double, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong),
                                               c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_sequence_score": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_double, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong),
                                                  c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_batch_score": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                     C.c_double, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong),
                                                     c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence_score": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                        C.c_double, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong),
                                                        c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_flow_warp_host": (C.c_int, [c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "b2f_flow_warp_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_op_flow_warp": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "b2f_compute_flow_batch_warp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                              C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_sequence_warp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                                 C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_batch_warp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                                    C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p, C.POINTER(C.c_ubyte),
                                                    C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence_warp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                                       C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p, C.POINTER(C.c_ubyte),
                                                       C.POINTER(C.c_ubyte)]),
    "b2f_forward_device_past": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_forward_sequence_device_past": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_compute_flow_batch_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                              c_float_p, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_sequence_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                 c_float_p, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_batch_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_int, c_float_p, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                       c_float_p, c_float_p, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_device_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_compute_flow_sequence_device_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_flow_warp_past_host": (C.c_int, [c_float_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "b2f_flow_warp_past_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "b2f_op_flow_warp_past": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "b2f_compute_flow_batch_warp_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                   C.c_double, C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p, c_float_p,
                                                   C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_compute_flow_sequence_warp_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                                      C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p, c_float_p,
                                                      C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_batch_warp_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                         C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p,
                                                         c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_sequence_warp_past": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                                            C.c_void_p, C.POINTER(C.c_ulonglong), c_float_p, c_float_p, c_float_p,
                                                            C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_table_loss_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                      C.POINTER(C.c_ulonglong)]),
    "b2f_table_loss_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                        C.c_void_p, C.c_void_p]),
    "b2f_op_table_loss": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                    C.POINTER(C.c_ulonglong)]),
    "b2f_forward_loss": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong),
                                   C.POINTER(c_float_p), C.c_int]),
    "b2f_forward_loss_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
    "b2f_multi_forward_loss": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong)]),
    "b2f_table_loss_ft_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                      C.POINTER(C.c_ulonglong)]),
    "b2f_table_loss_ft_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                        C.c_void_p, C.c_void_p]),
    "b2f_op_table_loss_ft": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                    C.POINTER(C.c_ulonglong)]),
    "b2f_forward_loss_ft": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong),
                                   C.POINTER(c_float_p), C.c_int]),
    "b2f_forward_loss_ft_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
    "b2f_multi_forward_loss_ft": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong)]),
    "b2f_table_loss_ssim_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                           C.POINTER(C.c_ulonglong), C.c_int, c_float_p]),
    "b2f_table_loss_plain_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                           C.POINTER(C.c_ulonglong), C.c_int, c_float_p]),
    "b2f_table_loss_ssim_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                             C.c_void_p, C.c_void_p, C.c_int, c_float_p]),
    "b2f_table_loss_plain_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                             C.c_void_p, C.c_void_p, C.c_int, c_float_p]),
    "b2f_op_table_loss_ssim": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                         C.POINTER(C.c_ulonglong), C.c_int, c_float_p]),
    "b2f_op_table_loss_plain": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                         C.POINTER(C.c_ulonglong), C.c_int, c_float_p]),
    "b2f_forward_loss_ssim": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong),
                                        C.POINTER(c_float_p), C.c_int, C.c_int, c_float_p]),
    "b2f_forward_loss_plain": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong),
                                        C.POINTER(c_float_p), C.c_int, C.c_int, c_float_p]),
    "b2f_forward_loss_ssim_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                               C.c_int, c_float_p]),
    "b2f_forward_loss_plain_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                               C.c_int, c_float_p]),
    "b2f_multi_forward_loss_ssim": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong),
                                              C.c_int, c_float_p]),
    "b2f_multi_forward_loss_plain": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ulonglong),
                                              C.c_int, c_float_p]),
    "b2f_loss_ssim_weights": (C.c_int, [C.POINTER(C.c_double)]),
    "b2f_loss_grad_defaults": (C.c_int, [c_grad_opts_p]),
    "b2f_table_loss_grad_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double, c_grad_opts_p,
                                           C.POINTER(c_float_p)]),
    "b2f_table_loss_grad_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                             c_grad_opts_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "b2f_op_table_loss_grad": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double, c_grad_opts_p,
                                         C.POINTER(c_float_p)]),
    "b2f_forward_loss_grad": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_opts_p, C.POINTER(C.c_ulonglong),
                                        C.POINTER(c_float_p), C.c_int, C.POINTER(c_float_p)]),
    "b2f_forward_loss_grad_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_opts_p, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "b2f_multi_forward_loss_grad": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_opts_p, C.POINTER(C.c_ulonglong),
                                              C.POINTER(c_float_p), C.c_int]),
    "b2f_loss_grad_ft_defaults": (C.c_int, [c_grad_ft_opts_p]),
    "b2f_table_loss_grad_ft_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                              c_grad_ft_opts_p, C.POINTER(c_float_p)]),
    "b2f_table_loss_grad_ft_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                                c_grad_ft_opts_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "b2f_op_table_loss_grad_ft": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                            c_grad_ft_opts_p, C.POINTER(c_float_p)]),
    "b2f_forward_loss_grad_ft": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_ft_opts_p,
                                           C.POINTER(C.c_ulonglong), C.POINTER(c_float_p), C.c_int, C.POINTER(c_float_p)]),
    "b2f_forward_loss_grad_ft_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_ft_opts_p,
                                                  C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "b2f_multi_forward_loss_grad_ft": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_ft_opts_p,
                                                 C.POINTER(C.c_ulonglong), C.POINTER(c_float_p), C.c_int]),
    "b2f_loss_grad_ssim_defaults": (C.c_int, [c_grad_ssim_opts_p]),
    "b2f_loss_grad_plain_defaults": (C.c_int, [c_grad_plain_opts_p]),
    "b2f_table_loss_grad_ssim_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                                c_grad_ssim_opts_p, C.POINTER(c_float_p), C.c_int, c_float_p]),
    "b2f_table_loss_grad_plain_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                                c_grad_plain_opts_p, C.POINTER(c_float_p), C.c_int, c_float_p]),
    "b2f_table_loss_grad_ssim_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                                  c_grad_ssim_opts_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, c_float_p]),
    "b2f_table_loss_grad_plain_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                                  c_grad_plain_opts_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, c_float_p]),
    "b2f_op_table_loss_grad_ssim": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                              c_grad_ssim_opts_p, C.POINTER(c_float_p), C.c_int, c_float_p]),
    "b2f_op_table_loss_grad_plain": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_double,
                                              c_grad_plain_opts_p, C.POINTER(c_float_p), C.c_int, c_float_p]),
    "b2f_forward_loss_grad_ssim": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_ssim_opts_p,
                                             C.POINTER(C.c_ulonglong), C.POINTER(c_float_p), C.c_int, C.POINTER(c_float_p), C.c_int, c_float_p]),
    "b2f_forward_loss_grad_plain": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_plain_opts_p,
                                             C.POINTER(C.c_ulonglong), C.POINTER(c_float_p), C.c_int, C.POINTER(c_float_p), C.c_int, c_float_p]),
    "b2f_forward_loss_grad_ssim_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_ssim_opts_p,
                                                    C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, c_float_p]),
    "b2f_forward_loss_grad_plain_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_plain_opts_p,
                                                    C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, c_float_p]),
    "b2f_multi_forward_loss_grad_ssim": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_ssim_opts_p,
                                                   C.POINTER(C.c_ulonglong), C.POINTER(c_float_p), C.c_int, C.c_int, c_float_p]),
    "b2f_multi_forward_loss_grad_plain": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_double, c_grad_plain_opts_p,
                                                   C.POINTER(C.c_ulonglong), C.POINTER(c_float_p), C.c_int, C.c_int, c_float_p]),
    "b2f_loss_epe_defaults": (C.c_int, [c_epe_opts_p]),
    "b2f_table_loss_epe_host": (C.c_int, [C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.POINTER(C.c_ubyte),
                                          C.POINTER(C.c_ubyte), C.c_double, C.c_int, c_epe_opts_p, C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(C.c_ulonglong), C.POINTER(c_float_p)]),
    "b2f_table_loss_epe_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_double, c_epe_opts_p, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "b2f_op_table_loss_epe": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.POINTER(C.c_ubyte),
                                        C.POINTER(C.c_ubyte), C.c_double, c_epe_opts_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong),
                                        C.POINTER(c_float_p)]),
    "b2f_forward_loss_epe": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                       C.c_double, c_epe_opts_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong), C.POINTER(c_float_p),
                                       C.c_int, C.POINTER(c_float_p)]),
    "b2f_forward_loss_epe_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_double, c_epe_opts_p, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_void_p), C.c_int,
                                              C.c_void_p]),
    "b2f_multi_forward_loss_epe": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, c_float_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                             C.c_double, c_epe_opts_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong), C.POINTER(c_float_p),
                                             C.c_int]),
    "b2f_forward": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.POINTER(c_float_p), C.c_int]),
    "b2f_output_shapes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.c_int]),
    "b2f_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "b2f_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "b2f_profile_read": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong),
                                   C.c_int, C.POINTER(C.c_int)]),
    "b2f_profile_reset": (C.c_int, [C.c_void_p]),
    "b2f_synchronize": (C.c_int, [C.c_void_p]),
    "b2f_init_multi": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "b2f_destroy_multi": (None, [C.c_void_p]),
    "b2f_multi_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
    "b2f_multi_context": (C.c_void_p, [C.c_void_p, C.c_int]),
    "b2f_multi_rebroadcast": (C.c_int, [C.c_void_p]),
    "b2f_multi_weights_checksum": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    "b2f_shard_range": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "b2f_multi_compute_flow_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, C.c_int, C.c_int,
                                               C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_multi_compute_flow_batch_u8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                                  C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "b2f_op_costvol": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, c_float_p]),
    "b2f_op_warp_bhwd": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, c_float_p]),
    "b2f_op_warp_bhwd_backward": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, c_float_p, c_float_p]),
    "b2f_op_costvol_backward": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, c_float_p, c_float_p]),
    "b2f_op_warp_costvol": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, C.c_float, C.c_int,
                                      C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_conv3x3": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p,
                                 C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_conv3x3_backward": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, C.c_int, C.c_int,
                                          c_float_p, c_float_p, C.c_int, c_float_p, c_float_p, c_float_p]),
    "b2f_op_conv3x3_backward_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                               C.POINTER(C.c_longlong)]),
    "b2f_op_conv3x3s2_backward": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, C.c_int,
                                            c_float_p, c_float_p, C.c_int, c_float_p, c_float_p, c_float_p]),
    "b2f_op_conv3x3s2_backward_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                 C.POINTER(C.c_longlong)]),
    "b2f_op_layer": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p]),
    "b2f_op_cv_record": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, C.c_float, C.c_int, C.c_int, C.c_int,
                                   C.c_int, c_float_p]),
    "b2f_op_cv_variant": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "b2f_op_conv_first": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p]),
    "b2f_op_conv_head16": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]),
    "b2f_op_upsample_flow2x": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_image_scale": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, C.c_int]),
    "b2f_op_upsample_flow2x_ex": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_softmax_nearest4": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_avgpool2": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_pack_input": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_warp_image": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, c_float_p, C.c_float, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_conv_first_seq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p]),
    "b2f_op_layout": (C.c_int, [C.c_void_p, C.c_int, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_graph_put_channels": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, C.c_int]),
    "b2f_op_graph_costvol": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       c_float_p, C.c_int, c_float_p, C.c_int]),
    "b2f_op_graph_warp": (C.c_int, [C.c_void_p, c_float_p, C.c_int, c_float_p, C.c_float, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_graph_add_flow": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_longlong]),
    "b2f_op_graph_scale": (C.c_int, [C.c_void_p, c_float_p, C.c_longlong, C.c_float]),
    "b2f_op_graph_softmax_nearest": (C.c_int, [C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p]),
    "b2f_op_expf": (C.c_int, [C.c_void_p, c_float_p, C.c_longlong, c_float_p]),
    "b2f_arena_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "b2f_guard_selftest": (C.c_int, [C.c_void_p, C.c_int]),
    "b2f_arena_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong)]),
}


class B2FError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise B2FError("%s is missing: build it with `python -m back2future_amd.build` "
                           "(there is no CPU fallback for the computeFlow path)" % SO_PATH)
        L = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise B2FError(lib().b2f_last_error().decode("utf-8", "replace"))


def fptr(a):
    return a.ctypes.data_as(c_float_p)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)
