"""Host-side mirror of the reference's inference API (back2future.lua), over libb2f.so.

    back2future = require('back2future')                 from back2future_amd import back2future
    computeFlow = back2future.init('Ours-Soft-ft-KITTI') computeFlow = back2future.init('Ours-Soft-ft-KITTI')
    flow, fwd_occ, bwd_occ = computeFlow(im1, im2, im3)  flow, fwd_occ, bwd_occ = computeFlow(im1, im2, im3)

Same names, argument order, return order and error behaviour (a failing call raises, like
error() in Lua).  Images are 3 x H x W float arrays in [0,1] (what image.load returns);
flow is a 2 x H x W float64 array (raw network flow, NOT multiplied by 20, exactly like
back2future.lua:77-84), the masks are 1 x H x W uint8 arrays.  The Lua original keeps
`model` in a global (back2future.lua:113): one model per Lua state.  Here the model lives in
the returned closure, and `init` may be called several times.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib

meanstd = {"mean": [0.485, 0.456, 0.406], "std": [0.229, 0.224, 0.225]}   # back2future.lua:33-36
occ_threshold = 0.6666                                                     # back2future.lua:40

# in_kind of the device entry points (include/b2f.h); IN_U8 is taken by the sequence and float32 entries only
IN_NORMALIZED, IN_UNIT, IN_U8 = 0, 1, 2
# layout of the flow pictures (include/b2f.h): n x 3 x H x W, the reference's tensor order, or n x H x W x 3
RGB_PLANAR, RGB_PACKED = 0, 1
STREAM_WARP, STREAM_PAST = 1, 2   # B2F_STREAM_*: the flags of b2f_stream_open_ex
# words of a score record (include/b2f.h, B2F_SCORE_*): counted pixels, Q20 error sums and Fl outliers per bucket (0 occluded "bwd",
# 1 visible, 2 occluded "fwd", 3 unlabelled), the 3 x 3 occlusion matrix (ground-truth class major), NaN errors
SCORE_PIXELS, SCORE_EPE_Q20, SCORE_OUTLIERS, SCORE_OCC, SCORE_NONFINITE, SCORE_WORDS = 0, 4, 8, 12, 21, 22
# words of a photometric record (include/b2f.h, B2F_PHOTO_*), each base + direction (0 the past frame, 1 the future one): pixels whose
# target lies in / leaves the image, Q30 sums of the L1 penalty, of the squared difference, of the occlusion-weighted penalty and of
# the weights over the inside pixels, pixels with a NaN coordinate, error or weight
PHOTO_INSIDE, PHOTO_OUTSIDE, PHOTO_CHARB_Q30, PHOTO_SQ_Q30, PHOTO_OCHARB_Q30, PHOTO_WEIGHT_Q30, PHOTO_NONFINITE, PHOTO_WORDS = 0, 2, 4, 6, 8, 10, 12, 14
# words of a loss record (include/b2f.h, B2F_LOSS_*; test.lua:266-297), one record per image and table level: the level's pixels, Q30
# sums of the flow smoothness (future, past), the constant-velocity term, the occlusion smoothness and the occlusion prior, the photo
# words (each base + direction, 0 the past frame, 1 the future one) and the pixels with a NaN smoothness, velocity or prior term
LOSS_PIXELS, LOSS_SMOOTH_FLOW_Q30, LOSS_SMOOTH_PAST_Q30, LOSS_CONST_VEL_Q30, LOSS_SMOOTH_OCC_Q30, LOSS_PRIOR_OCC_Q30 = 0, 1, 2, 3, 4, 5
LOSS_PHOTO_INSIDE, LOSS_PHOTO_OUTSIDE, LOSS_PHOTO_OCHARB_Q30, LOSS_PHOTO_NONFINITE, LOSS_NONFINITE, LOSS_WORDS = 6, 8, 10, 12, 14, 16
LOSS_LEVEL_WEIGHTS = (0.005, 0.01, 0.02, 0.08, 0.32, 0.64, 1.28)                                               # test.lua:29-31
LOSS_WEIGHTS = {"smooth_flow": 1.0, "const_vel": 1.0, "pme": 1.0, "smooth_occ": 0.1, "prior_occ": 0.1}       # opts.lua:61-73
# further words of a fine-tuning record (include/b2f.h, B2F_LOSS_FT_*; objective="finetune"): Q30 sums of the second-order smoothness
# (future, past; criterions/SecondOrderSmoothnessCriterion.lua) and of the occlusion-weighted gradient-constancy errors in x and y
# (base + direction; criterions/OBGCCriterion.lua), pixels with a NaN second-order term, counted pixel-directions with a NaN gradient term
LOSS_FT_SMOOTH2_FLOW_Q30, LOSS_FT_SMOOTH2_PAST_Q30, LOSS_FT_PHOTO_OGX_Q30, LOSS_FT_PHOTO_OGY_Q30 = 16, 17, 18, 20
LOSS_FT_SMOOTH2_NONFINITE, LOSS_FT_GRAD_NONFINITE, LOSS_FT_WORDS = 22, 23, 24
# further words of an SSIM record (include/b2f.h, B2F_LOSS_SSIM_*; objective="ssim"; criterions/OSSIML1Criterion.lua), each base +
# direction or + (minimum, maximum): Q30 sums of the occlusion-weighted 1 - SSIM and of the L1 penalty of the range-normalised
# difference, counted pixel-directions with a NaN product or an unusable range, float bits of the range used and of the image's own
LOSS_SSIM_Q30, LOSS_SSIM_L1N_Q30, LOSS_SSIM_NONFINITE, LOSS_SSIM_RANGE_USED, LOSS_SSIM_RANGE_OWN, LOSS_SSIM_WORDS = 16, 18, 20, 22, 24, 32
SSIM_RANGE_BATCH, SSIM_RANGE_IMAGE, SSIM_RANGE_GIVEN = 0, 1, 2   # range_mode of the *_ssim entries (include/b2f.h, B2F_SSIM_RANGE_*)
SSIM_ALPHA = {"OSSIM": 1.0, "OSSIML1": 0.85}                      # model.lua:172-179
# further words of a record of the photometric terms without occlusion masking (include/b2f.h, B2F_LOSS_PLAIN_*; objective="plain";
# criterions/MBCCriterion.lua, criterions/MSSIML1Criterion.lua), each base + direction or + (minimum, maximum): Q30 sums over PHOTO_INSIDE
# of the L1 and of the quadratic penalty of the raw difference, of 1 - SSIM and of the L1 penalty of the range-normalised difference,
# counted pixel-directions with a NaN term or an unusable range, float bits of the range used and of the image's own (which covers the
# occlusions and, on Soft tables, the past flow: MSSIML1Criterion.lua:63-68)
LOSS_PLAIN_L1_Q30, LOSS_PLAIN_SQ_Q30, LOSS_PLAIN_SSIM_Q30, LOSS_PLAIN_L1N_Q30, LOSS_PLAIN_SSIM_NONFINITE = 16, 18, 20, 22, 24
LOSS_PLAIN_RANGE_USED, LOSS_PLAIN_RANGE_OWN, LOSS_PLAIN_WORDS = 26, 28, 40
PLAIN_ALPHA = {"SSIM": 1.0, "SSIML1": 0.85}                       # model.lua:149-159
PLAIN_BCC, PLAIN_SSIM, PLAIN_L1, PLAIN_QUADRATIC = 0, 1, 0, 1     # criterion / penalty of b2f_loss_grad_plain_opts (B2F_PLAIN_*)
# words of a record of the supervised objective (include/b2f.h, B2F_LOSS_EPE_*; objective="epe"; train.lua:296-334 with
# criterions/L2Criterion.lua): the level's pixels, the valid pixels with a finite end-point error, its Q20 sum in units of flow_scale
# pixels, the valid pixels with a non-finite one, and the same three of the occlusion term over the labelled pixels (0 unless occ > 0)
LOSS_EPE_PIXELS, LOSS_EPE_VALID, LOSS_EPE_Q20, LOSS_EPE_FLOW_NONFINITE = 0, 1, 2, 3
LOSS_EPE_LABELLED, LOSS_EPE_OCC_Q20, LOSS_EPE_OCC_NONFINITE, LOSS_EPE_WORDS = 4, 5, 6, 8
EPE_COUNT_BATCH, EPE_COUNT_IMAGE, EPE_COUNT_GIVEN = 0, 1, 2       # count_mode of the *_epe entries (include/b2f.h, B2F_EPE_COUNT_*)
# what each released model was trained on (the reference's README.md:85-102; anything not named keeps opts.lua:61-73), by the names
# of init.  pme_alpha is listed as given: OBGCCriterion.lua:97 never applies it.  (model.lua:171 assigns -pme_gamma to a field named
# `gamm`, so a reference run keeps gamma = 1 whatever the option says; pass pme_gamma=1.0 to loss_summary for what such a run printed.)
LOSS_OBJECTIVES = {
    "Ours-Hard": {"weights": {"pme": 1.0, "smooth_flow": 2.0}, "pme_criterion": "OBCC", "smooth_second_order": False,
                  "pme_alpha": 1.0, "pme_beta": 1.0, "pme_gamma": 1.0, "past_flow": False},
    "Ours-Soft-ft-KITTI": {"weights": {"pme": 2.0, "smooth_flow": 0.1, "const_vel": 0.0001}, "pme_criterion": "OBGCC",
                           "smooth_second_order": True, "pme_alpha": 0.0, "pme_beta": 1.0, "pme_gamma": 1.0, "past_flow": True},
    "Ours-Soft-ft-Sintel": {"weights": {"pme": 4.0, "smooth_flow": 0.1, "const_vel": 0.0001}, "pme_criterion": "OBGCC",
                            "smooth_second_order": True, "pme_alpha": 1.0, "pme_beta": 0.0, "pme_gamma": 0.0, "past_flow": True},
}


def loss_words(objective):
    """words per record of objective "pme" (16; test.lua:266-297), "finetune" (24; with the terms of README.md:89-102), "ssim" (32;
    with the SSIM + L1 sums of criterions/OSSIML1Criterion.lua), "plain" (40; with the photometric sums without occlusion masking of
    criterions/MBCCriterion.lua and MSSIML1Criterion.lua) or "epe" (8; the supervised objective of train.lua:296-334)"""
    if objective == "pme":
        return LOSS_WORDS
    if objective == "finetune":
        return LOSS_FT_WORDS
    if objective == "ssim":
        return LOSS_SSIM_WORDS
    if objective == "plain":
        return LOSS_PLAIN_WORDS
    if objective == "epe":
        return LOSS_EPE_WORDS
    raise ValueError("objective must be 'pme', 'finetune', 'ssim', 'plain' or 'epe', got %r" % (objective,))


def loss_entry(pattern, objective):
    """the library's entry for an unsupervised objective: `pattern` with %s replaced by "", "_ft", "_ssim" or "_plain" """
    if objective == "epe":
        raise ValueError("objective 'epe' needs ground truth: use ops.table_loss_epe, Model.tableLossDevice(objective='epe', gt_flow=...) or "
                         "Model.tableLossGradDevice(objective='epe', gt_flow=...)")
    return getattr(_lib.lib(), pattern % {LOSS_WORDS: "", LOSS_FT_WORDS: "_ft", LOSS_SSIM_WORDS: "_ssim", LOSS_PLAIN_WORDS: "_plain"}[loss_words(objective)])


def ssim_range_args(objective, ssim_range, L, who, batch_ok=True):
    """The trailing (range_mode, ranges) arguments of a b2f_*_ssim or b2f_*_plain entry as a tuple, () for the other objectives.  ssim_range: "batch"
    (the minimum and maximum over the call's images, OSSIML1Criterion.lua:62-67), "image" (each image's own) or L x 2 numbers
    (mn, mx per level)."""
    if loss_words(objective) not in (LOSS_SSIM_WORDS, LOSS_PLAIN_WORDS):
        return ()
    if isinstance(ssim_range, str):
        modes = {"batch": SSIM_RANGE_BATCH, "image": SSIM_RANGE_IMAGE}
        if ssim_range not in modes or (ssim_range == "batch" and not batch_ok):
            raise ValueError("%s: ssim_range must be %s'image' or an L x 2 array, got %r" % (who, "'batch', " if batch_ok else "", ssim_range))
        return (modes[ssim_range], None)
    r = np.ascontiguousarray(ssim_range, np.float32)
    if r.shape != (L, 2):
        raise ValueError("%s: an ssim_range array must have shape (%d, 2): mn, mx per level; got %r" % (who, L, r.shape))
    return (SSIM_RANGE_GIVEN, _lib.fptr(r))   # (the pointer keeps r alive)


def normalize(imgs):
    """M.normalize = TF.ColorNormalize(meanstd) (back2future.lua:42-45, transforms.lua:33-45)."""
    out = np.array(imgs, dtype=np.float32, copy=True)
    for c in range(out.shape[0]):
        out[c] = (out[c] + np.float32(-meanstd["mean"][c % 3])) / np.float32(meanstd["std"][c % 3])
    return out


def sequence_frames(frames):
    """frames -> (contiguous T x 3 x H x W array, as_bytes) for the sequence entry points: one T x 3 x H x W array or a list
    of 3 x H x W arrays, float (converted to float32) or uint8 (value = byte / 255, passed as bytes), never a mix of the two.
    Raises ValueError on anything else, before any library call."""
    if isinstance(frames, (list, tuple)):
        arrs = [np.asarray(f) for f in frames]
        if any(a.ndim != 3 or a.shape[0] != 3 for a in arrs):
            raise ValueError("computeFlowSequence: every frame must be 3 x H x W")
        if len({a.shape for a in arrs}) > 1:
            raise ValueError("computeFlowSequence: the frames must have the same size")
        kinds = {a.dtype == np.uint8 for a in arrs}
        if len(kinds) > 1:
            raise ValueError("computeFlowSequence: mixed dtypes (all frames uint8, or all float)")
        as_bytes = kinds == {True}
        v = np.stack(arrs) if arrs else np.empty((0, 3, 1, 1), np.float32)
    else:
        v = np.asarray(frames)
        if v.ndim != 4 or v.shape[1] != 3:
            raise ValueError("computeFlowSequence: expected T x 3 x H x W frames")
        as_bytes = v.dtype == np.uint8
    if v.shape[0] < 3:
        raise ValueError("computeFlowSequence: a sequence needs T >= 3 frames, got %d" % v.shape[0])
    v = np.ascontiguousarray(v) if as_bytes else _lib.f32(v)
    return v, as_bytes


def _f64_outputs(n, H0, W0, out):
    """(flow, fwd, bwd) for the float64 entries: out = (flow float64 n x 2 x H x W, fwd uint8 n x 1 x H x W, bwd), or new arrays."""
    if out is not None:
        flow, fwd, bwd = out
        assert flow.dtype == np.float64 and flow.shape == (n, 2, H0, W0) and flow.flags.c_contiguous
        for m in (fwd, bwd):
            assert m.dtype == np.uint8 and m.shape == (n, 1, H0, W0) and m.flags.c_contiguous
        return flow, fwd, bwd
    return np.empty((n, 2, H0, W0), np.float64), np.empty((n, 1, H0, W0), np.uint8), np.empty((n, 1, H0, W0), np.uint8)


def output_dtype(dtype, occ_prob, who):
    """The `dtype=` / `occ_prob=` keywords of the computeFlow* wrappers: float64 (the f64 entries, the default) or float32
    (the b2f_*_f32 entries); occ_prob=True needs float32.  Raises ValueError before any library call."""
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise ValueError("%s: dtype must be np.float64 or np.float32, got %r" % (who, dtype))
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("%s: dtype must be np.float64 or np.float32, got %s" % (who, dt))
    if occ_prob and dt != np.float32:
        raise ValueError("%s: occ_prob=True needs dtype=np.float32 (the float64 entries have no occlusion probabilities)" % who)
    return dt


def _f32_outputs(n, H0, W0, occ_prob, out, who):
    """(flow, fwd, bwd, occ_prob or None) for the f32 entries.  out = (flow float32 n x 2 x H x W, fwd uint8 n x 1 x H x W, bwd
    [, occ_prob float32 n x 2 x H x W]) with occ_prob=True; fwd / bwd may be None (the masks are then not computed)."""
    if out is None:
        return (np.empty((n, 2, H0, W0), np.float32), np.empty((n, 1, H0, W0), np.uint8), np.empty((n, 1, H0, W0), np.uint8),
                np.empty((n, 2, H0, W0), np.float32) if occ_prob else None)
    out = tuple(out)
    if len(out) != (4 if occ_prob else 3):
        raise ValueError("%s: out must be (flow, fwd_occ, bwd_occ%s)" % (who, ", occ_prob" if occ_prob else ""))
    spec = [(np.float32, (n, 2, H0, W0)), (np.uint8, (n, 1, H0, W0)), (np.uint8, (n, 1, H0, W0)), (np.float32, (n, 2, H0, W0))]
    for i, (a, (dt, shape)) in enumerate(zip(out, spec)):
        if a is None and i in (1, 2):
            continue
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shape or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError("%s: out[%d] must be a writeable C-contiguous %s array of shape %s" % (who, i, np.dtype(dt).name, shape))
    return out + ((None,) if not occ_prob else ())


def _call_f32(fn, h, count, in_kind, ins, H0, W0, outs, occ_prob):
    flow, fwd, bwd, occ = outs
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    _lib.check(getattr(_lib.lib(), fn)(h, count, in_kind, *[C.c_void_p(a.ctypes.data) for a in ins], H0, W0, _lib.fptr(flow),
                                       _lib.fptr(occ) if occ is not None else None, u8p(fwd), u8p(bwd)))
    return (flow, fwd, bwd) + ((occ,) if occ_prob else ())


def _call_f64(fn, h, count, as_bytes, ins, H0, W0, outs):
    """fn (float inputs) or fn + "_u8" (byte inputs) into the float64 outputs."""
    flow, fwd, bwd = outs
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    _lib.check(getattr(_lib.lib(), fn + ("_u8" if as_bytes else ""))(h, count, *[u8p(a) if as_bytes else _lib.fptr(a) for a in ins], H0, W0,
                                                                   flow.ctypes.data_as(C.POINTER(C.c_double)), u8p(fwd), u8p(bwd)))
    return flow, fwd, bwd


def _batch_inputs(im1, im2, im3):
    as_bytes = all(np.asarray(a).dtype == np.uint8 for a in (im1, im2, im3))
    if as_bytes:
        im1, im2, im3 = (np.ascontiguousarray(a) for a in (im1, im2, im3))
    else:
        im1, im2, im3 = _lib.f32(im1), _lib.f32(im2), _lib.f32(im3)
    assert im1.ndim == 4 and im1.shape == im2.shape == im3.shape and im1.shape[1] == 3, "expected three n x 3 x H x W arrays"
    return im1, im2, im3, as_bytes


def _compute_flow_batch(prefix, h, im1, im2, im3, out, dtype, occ_prob):
    """computeFlowBatch of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    f32 = output_dtype(dtype, occ_prob, "computeFlowBatch") == np.float32
    im1, im2, im3, as_bytes = _batch_inputs(im1, im2, im3)
    n, _, H0, W0 = im1.shape
    if f32:
        return _call_f32(prefix + "compute_flow_batch_f32", h, n, IN_U8 if as_bytes else IN_UNIT, (im1, im2, im3), H0, W0,
                         _f32_outputs(n, H0, W0, occ_prob, out, "computeFlowBatch"), occ_prob)
    return _call_f64(prefix + "compute_flow_batch", h, n, as_bytes, (im1, im2, im3), H0, W0, _f64_outputs(n, H0, W0, out))


def _compute_flow_sequence(prefix, h, frames, out, dtype, occ_prob):
    """computeFlowSequence of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    f32 = output_dtype(dtype, occ_prob, "computeFlowSequence") == np.float32
    v, as_bytes = sequence_frames(frames)
    T, _, H0, W0 = v.shape
    if f32:
        return _call_f32(prefix + "compute_flow_sequence_f32", h, T, IN_U8 if as_bytes else IN_UNIT, (v,), H0, W0,
                         _f32_outputs(T - 2, H0, W0, occ_prob, out, "computeFlowSequence"), occ_prob)
    return _call_f64(prefix + "compute_flow_sequence", h, T, as_bytes, (v,), H0, W0, _f64_outputs(T - 2, H0, W0, out))


def _past_outputs(n, H0, W0, occ_prob, out, who):
    """(flow, past_flow, fwd, bwd, occ_prob or None) for the _past entries.  out = (flow, past_flow float32 n x 2 x H x W, fwd uint8
    n x 1 x H x W, bwd[, occ_prob]); fwd / bwd may be None (the masks are then not computed)."""
    if out is None:
        flow, fwd, bwd, occ = _f32_outputs(n, H0, W0, occ_prob, None, who)
        return flow, np.empty((n, 2, H0, W0), np.float32), fwd, bwd, occ
    out = tuple(out)
    if len(out) != (5 if occ_prob else 4):
        raise ValueError("%s: out must be (flow, past_flow, fwd_occ, bwd_occ%s)" % (who, ", occ_prob" if occ_prob else ""))
    past = out[1]
    if not isinstance(past, np.ndarray) or past.dtype != np.float32 or past.shape != (n, 2, H0, W0) or not past.flags.c_contiguous or \
            not past.flags.writeable:
        raise ValueError("%s: out[1] must be a writeable C-contiguous float32 array of shape %s" % (who, (n, 2, H0, W0)))
    flow, fwd, bwd, occ = _f32_outputs(n, H0, W0, occ_prob, out[:1] + out[2:], who)
    return flow, past, fwd, bwd, occ


def _call_past(fn, h, count, in_kind, ins, H0, W0, outs, occ_prob):
    flow, past, fwd, bwd, occ = outs
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    _lib.check(getattr(_lib.lib(), fn)(h, count, in_kind, *[C.c_void_p(a.ctypes.data) for a in ins], H0, W0, _lib.fptr(flow), _lib.fptr(past),
                                       _lib.fptr(occ) if occ is not None else None, u8p(fwd), u8p(bwd)))
    return (flow, past, fwd, bwd) + ((occ,) if occ_prob else ())


def _compute_flow_batch_past(prefix, h, im1, im2, im3, out, occ_prob):
    """computeFlowBatchPast of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowBatchPast"
    arrs = [np.asarray(a) for a in (im1, im2, im3)]
    if any(a.ndim != 4 or a.shape[1] != 3 or a.shape[0] < 1 for a in arrs) or len({a.shape for a in arrs}) > 1:
        raise ValueError("%s: expected three n x 3 x H x W arrays of one shape" % who)
    im1, im2, im3, as_bytes = _batch_inputs(*arrs)
    n, _, H0, W0 = im1.shape
    return _call_past(prefix + "compute_flow_batch_past", h, n, IN_U8 if as_bytes else IN_UNIT, (im1, im2, im3), H0, W0,
                      _past_outputs(n, H0, W0, occ_prob, out, who), occ_prob)


def _compute_flow_sequence_past(prefix, h, frames, out, occ_prob):
    """computeFlowSequencePast of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowSequencePast"
    v, as_bytes = sequence_frames(frames)
    T, _, H0, W0 = v.shape
    return _call_past(prefix + "compute_flow_sequence_past", h, T, IN_U8 if as_bytes else IN_UNIT, (v,), H0, W0,
                      _past_outputs(T - 2, H0, W0, occ_prob, out, who), occ_prob)


def rgb_max_norm(max, who):
    """The `max=` keyword of the flow-picture wrappers as the library's max_norm: None (each picture's own maximum) -> 0, else a
    positive number (flowX.xy2rgb's third argument).  Raises ValueError before any library call."""
    if max is None:
        return 0.0
    try:
        m = float(max)
    except (TypeError, ValueError):
        raise ValueError("%s: max must be None or a positive number, got %r" % (who, max))
    if not m > 0.0:
        raise ValueError("%s: max must be None or a positive number, got %r" % (who, max))
    return m


def _rgb_outputs(n, H0, W0, packed, want_flow, want_masks, out, who):
    """(rgb, max_used, flow or None, fwd or None, bwd or None) for the rgb entries; out = (rgb, max_used[, flow][, fwd_occ, bwd_occ]),
    the buffers the call returns (page-locked ones are written by DMA), or new arrays."""
    spec = [(np.uint8, (n, H0, W0, 3) if packed else (n, 3, H0, W0)), (np.float64, (n,))]
    spec += [(np.float32, (n, 2, H0, W0))] if want_flow else []
    spec += [(np.uint8, (n, 1, H0, W0))] * 2 if want_masks else []
    if out is None:
        bufs = [np.empty(shape, dt) for dt, shape in spec]
    else:
        bufs = list(out)
        if len(bufs) != len(spec):
            raise ValueError("%s: out must be (rgb, max_used%s%s)" % (who, ", flow" if want_flow else "", ", fwd_occ, bwd_occ" if want_masks else ""))
        for i, (a, (dt, shape)) in enumerate(zip(bufs, spec)):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shape or not a.flags.c_contiguous or not a.flags.writeable:
                raise ValueError("%s: out[%d] must be a writeable C-contiguous %s array of shape %s" % (who, i, np.dtype(dt).name, shape))
    rest = bufs[2:]
    flow = rest.pop(0) if want_flow else None
    fwd, bwd = rest if want_masks else (None, None)
    return bufs[0], bufs[1], flow, fwd, bwd


def _call_rgb(fn, h, count, in_kind, ins, H0, W0, max_norm, packed, outs):
    rgb, mx, flow, fwd, bwd = outs
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    _lib.check(getattr(_lib.lib(), fn)(h, count, in_kind, *[C.c_void_p(a.ctypes.data) for a in ins], H0, W0, max_norm,
                                       RGB_PACKED if packed else RGB_PLANAR, u8p(rgb), mx.ctypes.data_as(C.POINTER(C.c_double)),
                                       _lib.fptr(flow) if flow is not None else None, u8p(fwd), u8p(bwd)))
    return tuple(a for a in outs if a is not None)


def _compute_flow_batch_rgb(prefix, h, im1, im2, im3, max, packed, want_flow, want_masks, out):
    """computeFlowBatchRGB of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowBatchRGB"
    max_norm = rgb_max_norm(max, who)
    arrs = [np.asarray(a) for a in (im1, im2, im3)]
    if any(a.ndim != 4 or a.shape[1] != 3 or a.shape[0] < 1 for a in arrs) or len({a.shape for a in arrs}) > 1:
        raise ValueError("%s: expected three n x 3 x H x W arrays of one shape" % who)
    im1, im2, im3, as_bytes = _batch_inputs(*arrs)
    n, _, H0, W0 = im1.shape
    outs = _rgb_outputs(n, H0, W0, packed, want_flow, want_masks, out, who)
    return _call_rgb(prefix + "compute_flow_batch_rgb", h, n, IN_U8 if as_bytes else IN_UNIT, (im1, im2, im3), H0, W0, max_norm, packed, outs)


def _compute_flow_sequence_rgb(prefix, h, frames, max, packed, want_flow, want_masks, out):
    """computeFlowSequenceRGB of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowSequenceRGB"
    max_norm = rgb_max_norm(max, who)
    v, as_bytes = sequence_frames(frames)
    T, _, H0, W0 = v.shape
    outs = _rgb_outputs(T - 2, H0, W0, packed, want_flow, want_masks, out, who)
    return _call_rgb(prefix + "compute_flow_sequence_rgb", h, T, IN_U8 if as_bytes else IN_UNIT, (v,), H0, W0, max_norm, packed, outs)


class FlowStream(object):
    """Frames that arrive one at a time (Model.openStream; b2f_stream_*): the features of the last frames stay on the GPU, every
    pushed frame is uploaded and run through the feature pyramid once.  Pushes 1 and 2 return None; push k >= 3 returns the outputs
    of the triplet of frames (k-2, k-1, k) with a leading `cams` axis -- with the model's default options output k-3 of
    computeFlowSequence(dtype=np.float32) on the same frames, bit for bit.  A context manager: `with model.openStream(H, W) as st:`."""

    def __init__(self, model, H0, W0, cams=1, dtype=np.uint8, flags=0):
        try:
            dt = np.dtype(dtype)
        except TypeError:
            raise ValueError("openStream: dtype must be np.uint8 or np.float32, got %r" % (dtype,))
        if dt not in (np.dtype(np.uint8), np.dtype(np.float32)):
            raise ValueError("openStream: dtype must be np.uint8 or np.float32, got %s" % dt)
        if int(cams) < 1 or int(H0) < 64 or int(W0) < 64:
            raise ValueError("openStream: cams >= 1 and H0, W0 >= 64, got cams=%r H0=%r W0=%r" % (cams, H0, W0))
        self._h = None
        self.cams, self.H0, self.W0, self.dtype = int(cams), int(H0), int(W0), dt
        self.in_kind = IN_U8 if dt == np.uint8 else IN_UNIT
        self.flags = int(flags)   # STREAM_*: what the stream was opened for (0: a plain stream, b2f_stream_open itself)
        h = C.c_void_p()
        if self.flags:
            _lib.check(_lib.lib().b2f_stream_open_ex(model._h, self.cams, self.in_kind, self.H0, self.W0, self.flags, C.byref(h)))
        else:
            _lib.check(_lib.lib().b2f_stream_open(model._h, self.cams, self.in_kind, self.H0, self.W0, C.byref(h)))
        self._h = h
        self._model = model
        model._streams.append(weakref.ref(self))   # Model.close closes the streams that are still open

    def close(self):
        if getattr(self, "_h", None):
            if _lib is not None:
                _lib.lib().b2f_stream_close(self._h)
            self._h = None
            self._model._streams[:] = [r for r in self._model._streams if r() not in (None, self)]

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _open(self, who):
        if not getattr(self, "_h", None):
            raise ValueError("%s: the stream is closed" % who)

    def _frames(self, frames, who):
        """The cams x 3 x H0 x W0 array of a push: 3 x H0 x W0 is accepted for one camera; the stream's dtype exactly."""
        self._open(who)
        v = np.asarray(frames)
        if v.dtype != self.dtype:
            raise ValueError("%s: this stream takes %s frames, got %s" % (who, self.dtype.name, v.dtype))
        if v.ndim == 3 and self.cams == 1:
            v = v[None]
        if v.shape != (self.cams, 3, self.H0, self.W0):
            raise ValueError("%s: expected %s frames, got %s" % (who, "%d x 3 x %d x %d" % (self.cams, self.H0, self.W0), "x".join(map(str, v.shape))))
        return np.ascontiguousarray(v)

    @property
    def frames_pushed(self):
        self._open("frames_pushed")
        n = C.c_longlong()
        _lib.check(_lib.lib().b2f_stream_info(self._h, None, None, None, None, C.byref(n)))
        return n.value

    def reset(self):
        """Forget the pushed frames (the next push is push 1) and clear the broken flag of a failed push."""
        self._open("reset")
        _lib.check(_lib.lib().b2f_stream_reset(self._h))

    def push(self, frames, out=None, occ_prob=False):
        """One new frame per camera (3 x H0 x W0 with one camera, else cams x 3 x H0 x W0).  Returns None for the first two pushes,
        then (flow, fwd_occ, bwd_occ[, occ_prob]) as computeFlowBatch(dtype=np.float32) with n = cams; out = those buffers."""
        v = self._frames(frames, "push")
        flow, fwd, bwd, occ = _f32_outputs(self.cams, self.H0, self.W0, occ_prob, out, "push")
        u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
        ready = C.c_int()
        _lib.check(_lib.lib().b2f_stream_push(self._h, C.c_void_p(v.ctypes.data), _lib.fptr(flow), _lib.fptr(occ) if occ is not None else None,
                                              u8p(fwd), u8p(bwd), C.byref(ready)))
        if not ready.value:
            return None
        return (flow, fwd, bwd) + ((occ,) if occ_prob else ())

    def pushRGB(self, frames, max=None, packed=False, want_flow=False, want_masks=False, out=None):
        """push with the flow pictures as the output (b2f_stream_push_rgb): None, or (rgb, max_used[, flow][, fwd_occ, bwd_occ]) as
        computeFlowBatchRGB with n = cams."""
        max_norm = rgb_max_norm(max, "pushRGB")
        v = self._frames(frames, "pushRGB")
        outs = _rgb_outputs(self.cams, self.H0, self.W0, packed, want_flow, want_masks, out, "pushRGB")
        rgb, mx, flow, fwd, bwd = outs
        u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
        ready = C.c_int()
        _lib.check(_lib.lib().b2f_stream_push_rgb(self._h, C.c_void_p(v.ctypes.data), max_norm, RGB_PACKED if packed else RGB_PLANAR, u8p(rgb),
                                                  mx.ctypes.data_as(C.POINTER(C.c_double)), _lib.fptr(flow) if flow is not None else None,
                                                  u8p(fwd), u8p(bwd), C.byref(ready)))
        return tuple(a for a in outs if a is not None) if ready.value else None

    def pushDevice(self, d_frames, d_flow, d_occ_prob=None, d_fwd_occ=None, d_bwd_occ=None, stream=None):
        """b2f_stream_push_device on device pointers (ints): d_frames cams x 3 x H0 x W0 of the stream's dtype; outputs as
        computeFlowDevice with n = cams, written only when the call returns True (from the third push on).  Asynchronous on `stream`."""
        self._open("pushDevice")
        if not d_frames or not d_flow:
            raise ValueError("pushDevice: d_frames and d_flow are required")
        p = lambda v: C.c_void_p(v) if v else None
        ready = C.c_int()
        _lib.check(_lib.lib().b2f_stream_push_device(self._h, p(d_frames), p(d_flow), p(d_occ_prob), p(d_fwd_occ), p(d_bwd_occ), p(stream),
                                                     C.byref(ready)))
        return bool(ready.value)


class MotionStream(FlowStream):
    """What Model.openStream(warp=True) / openStream(past=True) returns: a FlowStream opened with flags (b2f_stream_open_ex), which adds
    the pushes that need them -- motion compensation per pushed frame (warp=True: the stream keeps the caller's frames of its last
    three pushes) and the past flow of a Soft model (past=True).  Every push of FlowStream works on it as well, and may alternate with
    the new ones.  A push the stream was not opened for is refused by the library with a message that names the missing flag, and
    leaves the stream as it was.  A stream opened without either stays a plain FlowStream, which has none of these pushes."""

    def __init__(self, model, H0, W0, cams=1, dtype=np.uint8, warp=False, past=False):
        FlowStream.__init__(self, model, H0, W0, cams, dtype, (STREAM_WARP if warp else 0) | (STREAM_PAST if past else 0))

    def pushWarp(self, frames, flow_scale=20.0, want_warped=True, want_photo=True, want_flow=False, want_masks=False, want_prob=False,
                 own_past_flow=False, want_past=False, out=None):
        """push with motion compensation as the output (b2f_stream_push_warp; a stream opened with warp=True): None for the first two
        pushes, then what computeFlowSequenceWarp returns for one centre frame per camera, in its order and with its keywords --
        (warped, photo[, flow][, fwd_occ, bwd_occ][, occ_prob][, past_flow]) with n = cams, a single array alone -- where warped[:, 0]
        is the frame of two pushes ago and warped[:, 1] the frame of this push, both sampled onto the frame of the push before.
        own_past_flow / want_past need a stream opened with past=True as well.  photo_summary reads the records."""
        who = "pushWarp"
        own = _own_past(own_past_flow, want_past, who)
        v = self._frames(frames, who)
        outs = _warp_outputs(self.cams, self.H0, self.W0, self.in_kind == IN_U8, want_warped, want_photo, want_flow, want_masks, want_prob, out,
                             who, want_past)
        warped, photo, flow, fwd, bwd, prob, past = outs
        u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
        fp = lambda a: _lib.fptr(a) if a is not None else None
        ready = C.c_int()
        _lib.check(_lib.lib().b2f_stream_push_warp(self._h, C.c_void_p(v.ctypes.data), float(flow_scale), 1 if own else 0,
                                                   C.c_void_p(warped.ctypes.data) if warped is not None else None,
                                                   photo.ctypes.data_as(C.POINTER(C.c_ulonglong)) if photo is not None else None,
                                                   fp(flow), fp(prob), u8p(fwd), u8p(bwd), fp(past), C.byref(ready)))
        if not ready.value:
            return None
        res = tuple(a for a in outs if a is not None)
        return res[0] if len(res) == 1 else res

    def pushPast(self, frames, out=None, occ_prob=False):
        """push with the past flow of a Soft model (b2f_stream_push_past; a stream opened with past=True): None for the first two
        pushes, then (flow, past_flow, fwd_occ, bwd_occ[, occ_prob]) as computeFlowSequencePast for one centre frame per camera;
        out = those buffers (its masks may be None)."""
        v = self._frames(frames, "pushPast")
        flow, past, fwd, bwd, occ = _past_outputs(self.cams, self.H0, self.W0, occ_prob, out, "pushPast")
        u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
        ready = C.c_int()
        _lib.check(_lib.lib().b2f_stream_push_past(self._h, C.c_void_p(v.ctypes.data), _lib.fptr(flow), _lib.fptr(past),
                                                   _lib.fptr(occ) if occ is not None else None, u8p(fwd), u8p(bwd), C.byref(ready)))
        if not ready.value:
            return None
        return (flow, past, fwd, bwd) + ((occ,) if occ_prob else ())

    def pushDeviceWarp(self, d_frames, flow_scale=20.0, d_warped=None, d_photo=None, d_flow=None, d_occ_prob=None, d_fwd_occ=None,
                       d_bwd_occ=None, own_past_flow=False, d_past_flow=None, stream=None):
        """b2f_stream_push_warp_device on device pointers (ints): d_frames cams x 3 x H0 x W0 of the stream's dtype, d_warped
        cams x 2 x 3 x H0 x W0 of that dtype, d_photo cams x 14 uint64; at least one of the two, the rest optional.  Written only when
        the call returns True (from the third push on).  Asynchronous on `stream`."""
        self._open("pushDeviceWarp")
        if not d_frames or not (d_warped or d_photo):
            raise ValueError("pushDeviceWarp: d_frames and at least one of d_warped and d_photo are required")
        p = lambda v: C.c_void_p(v) if v else None
        ready = C.c_int()
        _lib.check(_lib.lib().b2f_stream_push_warp_device(self._h, p(d_frames), float(flow_scale), 1 if own_past_flow else 0, p(d_warped), p(d_photo),
                                                          p(d_flow), p(d_occ_prob), p(d_fwd_occ), p(d_bwd_occ), p(d_past_flow), p(stream),
                                                          C.byref(ready)))
        return bool(ready.value)

    def pushDevicePast(self, d_frames, d_flow, d_past_flow, d_occ_prob=None, d_fwd_occ=None, d_bwd_occ=None, stream=None):
        """b2f_stream_push_past_device on device pointers (ints): pushDevice with the past flow in d_past_flow (cams x 2 x H0 x W0)."""
        self._open("pushDevicePast")
        if not d_frames or not d_flow or not d_past_flow:
            raise ValueError("pushDevicePast: d_frames, d_flow and d_past_flow are required")
        p = lambda v: C.c_void_p(v) if v else None
        ready = C.c_int()
        _lib.check(_lib.lib().b2f_stream_push_past_device(self._h, p(d_frames), p(d_flow), p(d_past_flow), p(d_occ_prob), p(d_fwd_occ),
                                                          p(d_bwd_occ), p(stream), C.byref(ready)))
        return bool(ready.value)


def score_ground_truth(n, H, W, gt_flow, valid, gt_occ, who):
    """The ground truth of the score wrappers in the library's layouts: gt_flow float32 n x 2 x H x W (pixels, as a .flo file holds
    them), valid and gt_occ uint8 n x H x W or None (n x 1 x H x W and bool are taken too).  Arrays that already have the layout
    are passed as they are, so page-locked ones stay page-locked.  Raises ValueError before any library call."""
    gt = np.asarray(gt_flow)
    if gt.shape != (n, 2, H, W):
        raise ValueError("%s: gt_flow must have shape %r, got %r" % (who, (n, 2, H, W), gt.shape))
    planes = []
    for name, a in (("valid", valid), ("gt_occ", gt_occ)):
        if a is None:
            planes.append(None)
            continue
        a = np.asarray(a)
        if a.shape == (n, 1, H, W):
            a = a.reshape(n, H, W)
        if a.shape != (n, H, W) or a.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)):
            raise ValueError("%s: %s must be uint8 (or bool) of shape %r, got %s %r" % (who, name, (n, H, W), a.dtype, a.shape))
        planes.append(np.ascontiguousarray(a).view(np.uint8))
    return _lib.f32(gt), planes[0], planes[1]


def _score_outputs(n, H0, W0, want_flow, want_masks, out, who):
    """(scores, flow or None, fwd or None, bwd or None) for the score entries; out = (scores[, flow][, fwd_occ, bwd_occ]), the buffers
    the call returns (page-locked ones are written by DMA), or new arrays."""
    spec = [(np.uint64, (n, SCORE_WORDS))]
    spec += [(np.float32, (n, 2, H0, W0))] if want_flow else []
    spec += [(np.uint8, (n, 1, H0, W0))] * 2 if want_masks else []
    if out is None:
        bufs = [np.empty(shape, dt) for dt, shape in spec]
    else:
        bufs = [out] if isinstance(out, np.ndarray) else list(out)
        if len(bufs) != len(spec):
            raise ValueError("%s: out must be (scores%s%s)" % (who, ", flow" if want_flow else "", ", fwd_occ, bwd_occ" if want_masks else ""))
        for i, (a, (dt, shape)) in enumerate(zip(bufs, spec)):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shape or not a.flags.c_contiguous or not a.flags.writeable:
                raise ValueError("%s: out[%d] must be a writeable C-contiguous %s array of shape %s" % (who, i, np.dtype(dt).name, shape))
    rest = bufs[1:]
    flow = rest.pop(0) if want_flow else None
    fwd, bwd = rest if want_masks else (None, None)
    return bufs[0], flow, fwd, bwd


def _call_score(fn, h, count, in_kind, ins, H0, W0, flow_scale, truth, outs):
    gt, valid, gt_occ = truth
    scores, flow, fwd, bwd = outs
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    _lib.check(getattr(_lib.lib(), fn)(h, count, in_kind, *[C.c_void_p(a.ctypes.data) for a in ins], H0, W0, float(flow_scale), _lib.fptr(gt),
                                       u8p(valid), u8p(gt_occ), scores.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                       _lib.fptr(flow) if flow is not None else None, u8p(fwd), u8p(bwd)))
    res = tuple(a for a in outs if a is not None)
    return res[0] if len(res) == 1 else res


def _compute_flow_batch_score(prefix, h, im1, im2, im3, gt_flow, valid, gt_occ, flow_scale, want_flow, want_masks, out):
    """computeFlowBatchScore of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowBatchScore"
    arrs = [np.asarray(a) for a in (im1, im2, im3)]
    if any(a.ndim != 4 or a.shape[1] != 3 or a.shape[0] < 1 for a in arrs) or len({a.shape for a in arrs}) > 1:
        raise ValueError("%s: expected three n x 3 x H x W arrays of one shape" % who)
    im1, im2, im3, as_bytes = _batch_inputs(*arrs)
    n, _, H0, W0 = im1.shape
    truth = score_ground_truth(n, H0, W0, gt_flow, valid, gt_occ, who)
    outs = _score_outputs(n, H0, W0, want_flow, want_masks, out, who)
    return _call_score(prefix + "compute_flow_batch_score", h, n, IN_U8 if as_bytes else IN_UNIT, (im1, im2, im3), H0, W0, flow_scale, truth, outs)


def _compute_flow_sequence_score(prefix, h, frames, gt_flow, valid, gt_occ, flow_scale, want_flow, want_masks, out):
    """computeFlowSequenceScore of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowSequenceScore"
    v, as_bytes = sequence_frames(frames)
    T, _, H0, W0 = v.shape
    truth = score_ground_truth(T - 2, H0, W0, gt_flow, valid, gt_occ, who)
    outs = _score_outputs(T - 2, H0, W0, want_flow, want_masks, out, who)
    return _call_score(prefix + "compute_flow_sequence_score", h, T, IN_U8 if as_bytes else IN_UNIT, (v,), H0, W0, flow_scale, truth, outs)


def score_summary(scores):
    """The measures of test.lua:183-261 from score records (n x 22 or 22 uint64 words; ops.flow_score, computeFlow*Score), summed over
    the images given: a dict of
      epe       mean end-point error in pixels over the counted pixels (criterions/L2Criterion.lua:36-38 times flownet_factor)
      epe_noc   the same over the pixels labelled visible (bucket 1), epe_occ over the occluded ones (buckets 0 and 2)
      fl        share of the counted pixels whose error exceeds 3 px and 5 % of the ground truth (KITTI's Fl)
      oacc      share of the labelled pixels whose occlusion class is right (test.lua:241-242); occ_acc_bwd / occ_acc_vis /
                occ_acc_fwd: the same within ground-truth class 0 / 0.5 / 1 (test.lua:244-259)
      pixels    counted pixels, nonfinite: valid pixels whose error was NaN (counted nowhere else)
    A ratio whose denominator is 0 is nan.  The sums are exact integers; the errors carry the records' Q20 rounding (2^-21 px)."""
    s = np.asarray(scores)
    if s.dtype != np.uint64 or s.shape[-1:] != (SCORE_WORDS,) or s.ndim not in (1, 2):
        raise ValueError("score_summary: expected uint64 records of %d words, got %s %r" % (SCORE_WORDS, s.dtype, s.shape))
    t = [sum(int(v) for v in col) for col in s.reshape(-1, SCORE_WORDS).T]   # Python integers: no overflow over many images
    pix, epe, out = t[SCORE_PIXELS:SCORE_PIXELS + 4], t[SCORE_EPE_Q20:SCORE_EPE_Q20 + 4], t[SCORE_OUTLIERS:SCORE_OUTLIERS + 4]
    occ = [t[SCORE_OCC + 3 * g:SCORE_OCC + 3 * g + 3] for g in range(3)]
    ratio = lambda a, b: a / b if b else float("nan")
    px = lambda q, k: ratio(q / float(1 << 20), k)
    return {"epe": px(sum(epe), sum(pix)), "epe_noc": px(epe[1], pix[1]), "epe_occ": px(epe[0] + epe[2], pix[0] + pix[2]),
            "fl": ratio(sum(out), sum(pix)),
            "oacc": ratio(sum(occ[g][g] for g in range(3)), sum(map(sum, occ))),
            "occ_acc_bwd": ratio(occ[0][0], sum(occ[0])), "occ_acc_vis": ratio(occ[1][1], sum(occ[1])),
            "occ_acc_fwd": ratio(occ[2][2], sum(occ[2])),
            "pixels": sum(pix), "nonfinite": t[SCORE_NONFINITE]}


def _warp_outputs(n, H0, W0, as_bytes, want_warped, want_photo, want_flow, want_masks, want_prob, out, who, want_past=False):
    """[warped, photo, flow, fwd, bwd, occ_prob, past_flow] (None: not asked for) for the warp entries; out = the buffers the call
    returns, in the order (warped, photo[, flow][, fwd_occ, bwd_occ][, occ_prob][, past_flow]) without what is not asked for, or new
    arrays."""
    if not want_warped and not want_photo:
        raise ValueError("%s: at least one of want_warped and want_photo" % who)
    spec = [(np.uint8 if as_bytes else np.float32, (n, 2, 3, H0, W0)) if want_warped else None,
            (np.uint64, (n, PHOTO_WORDS)) if want_photo else None,
            (np.float32, (n, 2, H0, W0)) if want_flow else None,
            (np.uint8, (n, 1, H0, W0)) if want_masks else None, (np.uint8, (n, 1, H0, W0)) if want_masks else None,
            (np.float32, (n, 2, H0, W0)) if want_prob else None,
            (np.float32, (n, 2, H0, W0)) if want_past else None]
    asked = [s for s in spec if s is not None]
    if out is None:
        bufs = [np.empty(shape, dt) for dt, shape in asked]
    else:
        bufs = [out] if isinstance(out, np.ndarray) else list(out)
        if len(bufs) != len(asked):
            raise ValueError("%s: out must hold the %d arrays the call returns" % (who, len(asked)))
        for i, (a, (dt, shape)) in enumerate(zip(bufs, asked)):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shape or not a.flags.c_contiguous or not a.flags.writeable:
                raise ValueError("%s: out[%d] must be a writeable C-contiguous %s array of shape %s" % (who, i, np.dtype(dt).name, shape))
    it = iter(bufs)
    return [next(it) if s is not None else None for s in spec]


def _own_past(own_past_flow, want_past, who):
    """the own_past_flow / want_past keywords of the warp wrappers: the past flow is an output of the own-past-flow entries only"""
    if want_past and not own_past_flow:
        raise ValueError("%s: want_past needs own_past_flow=True" % who)
    return bool(own_past_flow)


def _call_warp(fn, h, count, in_kind, ins, H0, W0, flow_scale, outs, own_past=False):
    """fn, or with own_past fn + "_past" (the past frame follows the model's own past flow; its argument list has past_flow after flow)"""
    warped, photo, flow, fwd, bwd, prob, past = outs
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    fp = lambda a: _lib.fptr(a) if a is not None else None
    _lib.check(getattr(_lib.lib(), fn + ("_past" if own_past else ""))(
        h, count, in_kind, *[C.c_void_p(a.ctypes.data) for a in ins], H0, W0, float(flow_scale),
        C.c_void_p(warped.ctypes.data) if warped is not None else None,
        photo.ctypes.data_as(C.POINTER(C.c_ulonglong)) if photo is not None else None,
        *((fp(flow), fp(past), fp(prob)) if own_past else (fp(flow), fp(prob))), u8p(fwd), u8p(bwd)))
    res = tuple(a for a in outs if a is not None)
    return res[0] if len(res) == 1 else res


def _compute_flow_batch_warp(prefix, h, im1, im2, im3, flow_scale, want_warped, want_photo, want_flow, want_masks, out, want_prob,
                             own_past_flow=False, want_past=False):
    """computeFlowBatchWarp of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowBatchWarp"
    own = _own_past(own_past_flow, want_past, who)
    arrs = [np.asarray(a) for a in (im1, im2, im3)]
    if any(a.ndim != 4 or a.shape[1] != 3 or a.shape[0] < 1 for a in arrs) or len({a.shape for a in arrs}) > 1:
        raise ValueError("%s: expected three n x 3 x H x W arrays of one shape" % who)
    im1, im2, im3, as_bytes = _batch_inputs(*arrs)
    n, _, H0, W0 = im1.shape
    outs = _warp_outputs(n, H0, W0, as_bytes, want_warped, want_photo, want_flow, want_masks, want_prob, out, who, want_past)
    return _call_warp(prefix + "compute_flow_batch_warp", h, n, IN_U8 if as_bytes else IN_UNIT, (im1, im2, im3), H0, W0, flow_scale, outs, own)


def _compute_flow_sequence_warp(prefix, h, frames, flow_scale, want_warped, want_photo, want_flow, want_masks, out, want_prob,
                                own_past_flow=False, want_past=False):
    """computeFlowSequenceWarp of Model (prefix "b2f_") and MultiModel ("b2f_multi_")."""
    who = "computeFlowSequenceWarp"
    own = _own_past(own_past_flow, want_past, who)
    v, as_bytes = sequence_frames(frames)
    T, _, H0, W0 = v.shape
    outs = _warp_outputs(T - 2, H0, W0, as_bytes, want_warped, want_photo, want_flow, want_masks, want_prob, out, who, want_past)
    return _call_warp(prefix + "compute_flow_sequence_warp", h, T, IN_U8 if as_bytes else IN_UNIT, (v,), H0, W0, flow_scale, outs, own)


def photo_summary(photo):
    """The photometric measures of test.lua:285 from photometric records (n x 14 or 14 uint64 words; ops.flow_warp,
    computeFlow*Warp), summed over the images given: a dict of
      pme            criterions/OBCCriterion.lua:updateOutput with the L1 penalty, penalty_out = 1 and sizeAverage, both directions:
                     sum_d (OCHARB_d / 2^30 + 1.0 * OUTSIDE_d) / (3 * 2 * pixels); pixels = the images' pixels (a pixel that is
                     non-finite in one direction counts half).  The weights are the occlusion probabilities the records were made with:
                     est[2] of a Hard model, est[3] of a Soft one (what the f32 entries return as occ_prob); without them pme is 0 + the
                     outside share
      bc             sum CHARB / (3 * sum INSIDE): the unmasked L1 error per sample of the pixels that stay in the image
      psnr_past, psnr_future   10 log10(3 * INSIDE_d * 2^30 / SQ_d) of the warped neighbour against the reference frame (inf: equal)
      inside_past, inside_future   share of the pixels whose target lies in the image
      pme_weighted   sum OCHARB / (3 * sum WEIGHT)
      nonfinite      pixels (per direction) with a NaN coordinate, error or weight; they are counted nowhere else
    A ratio whose denominator is 0 is nan.  The sums are exact integers; each pixel term carries the records' Q30 rounding (2^-31)."""
    s = np.asarray(photo)
    if s.dtype != np.uint64 or s.shape[-1:] != (PHOTO_WORDS,) or s.ndim not in (1, 2):
        raise ValueError("photo_summary: expected uint64 records of %d words, got %s %r" % (PHOTO_WORDS, s.dtype, s.shape))
    t = [sum(int(v) for v in col) for col in s.reshape(-1, PHOTO_WORDS).T]   # Python integers: no overflow over many images
    pair = lambda base: t[base:base + 2]
    ins, outs, charb, sq, ocharb, wsum, nonf = (pair(b) for b in (PHOTO_INSIDE, PHOTO_OUTSIDE, PHOTO_CHARB_Q30, PHOTO_SQ_Q30, PHOTO_OCHARB_Q30,
                                                                  PHOTO_WEIGHT_Q30, PHOTO_NONFINITE))
    one = float(1 << 30)
    ratio = lambda a, b: a / b if b else float("nan")
    seen = [ins[d] + outs[d] + nonf[d] for d in range(2)]   # every pixel of every image, per direction
    pixels = (seen[0] + seen[1] - sum(nonf)) / 2.0
    psnr = lambda d: float("nan") if not ins[d] else float("inf") if not sq[d] else 10.0 * np.log10(3.0 * ins[d] * one / sq[d])
    return {"pme": ratio(sum(ocharb) / one + 1.0 * sum(outs), 3.0 * 2.0 * pixels),
            "bc": ratio(sum(charb) / one, 3.0 * sum(ins)),
            "psnr_past": float(psnr(0)), "psnr_future": float(psnr(1)),
            "inside_past": ratio(ins[0], seen[0]), "inside_future": ratio(ins[1], seen[1]),
            "pme_weighted": ratio(sum(ocharb) / one, 3.0 * (sum(wsum) / one)),
            "nonfinite": sum(nonf)}


def loss_summary(records, like="test", size_average=False, weights=None, smooth_second_order=False, pme_criterion="OBCC", pme_beta=1.0,
                 pme_gamma=1.0, objective=None, ssim_alpha=None, flow_scale=20.0, count="batch", pme_penalty="L1", no_occ=False):
    """objective="epe": the supervised objective from the 8-word records of ops.table_loss_epe; see _loss_summary_epe, which takes
    size_average, weights ("epe", "occ", "level_weights"), flow_scale and count.  Otherwise:
    The unsupervised validation loss of test.lua:266-297 from loss records (uint64 n x L x 16 or L x 16; ops.table_loss,
    Model.forwardLoss; or n x L x 24 / L x 24 of objective="finetune").  Per level j
        level_weights[j] * (smooth_flow * S + const_vel * cv + pme * ((OCHARB0 + OCHARB1) / 2^30 + OUTSIDE0 + OUTSIDE1) / (3 * 2)
                            + smooth_occ * so + prior_occ * pr)
    with the level weights of test.lua:29-31 and the weights of opts.lua:61-73 (1, 1, 1, 0.1, 0.1; `weights` replaces any of them).
    like="test": S = n_flow * fs, test.lua:275-277 takes the future flow n_flow times (2 for a Soft table, 1 for a Hard one);
    like="train": S = fs + fp (train.lua:428-432).  A table is Soft when its records carry past-flow or constant-velocity sums.
    size_average=True applies the criteria's own norm factors per triplet: 1 / (2 h w) for the smoothness and velocity terms,
    1 / (h w) for the photometric term and the prior.
    With 24-word records: smooth_second_order=True takes fs and fp from the second-order sums (-smooth_second_order,
    SecondOrderSmoothnessCriterion.lua; like and size_average keep their meaning), and pme_criterion="OBGCC" makes the photometric term
        sum over d of ((OCHARB_d + pme_beta * OGX_d + pme_gamma * OGY_d) / 2^30 + OUTSIDE_d) / (3 * 2)
    (OBGCCriterion.lua:96-105,135-143: the brightness part is never multiplied by -pme_alpha, a quirk of updateOutput that is kept).
    With 32-word records (objective="ssim"): pme_criterion="OSSIM" | "OSSIML1" makes the photometric term
        sum over d of ((alpha * SSIM_d + (1 - alpha) * L1N_d) / 2^30 + OUTSIDE_d) / (3 * 2)
    (OSSIML1Criterion.lua:119,149-157) with alpha = 1 for OSSIM and 0.85 for OSSIML1 (model.lua:172-179; ssim_alpha replaces it);
    "OBCC" reads their first 16 words as before.  Records of another width raise ValueError for these two criteria.
    With 40-word records (objective="plain"): pme_criterion="BCC" | "SSIM" | "SSIML1" makes the photometric term that of
    criterions/MBCCriterion.lua resp. MSSIML1Criterion.lua, which do not mask occlusions and have no penalty_out:
        BCC:            sum over d of PLAIN_L1_d / 2^30 / (3 * 2)     (pme_penalty="Quadratic": PLAIN_SQ_d; model.lua:189-190)
        SSIM | SSIML1:  sum over d of (alpha * PLAIN_SSIM_d + (1 - alpha) * PLAIN_L1N_d) / 2^30 / (3 * 2), alpha = 1 | 0.85
    no_occ=True (opts.lua:85, train.lua:456, test.lua:289) drops the occlusions' smoothness and prior from "level", "loss" and "mean",
    whatever the records' width; the two terms are still returned.  "OBCC" reads the first 16 words of 40-word records as before.
    objective=NAME applies LOSS_OBJECTIVES[NAME], the options the named model was trained with, in place of these three arguments and
    under `weights`.  With 16-word records any of them set away from its default raises ValueError.
    Returns a dict: every term per triplet and level (n x L float64 arrays "smooth_flow", "smooth_past", "const_vel", "pme",
    "smooth_occ", "prior_occ", weighted by neither), "level" (n x L, the weighted sum above), "loss" (n, the sum over the levels),
    "mean" (the mean of "loss") and "nonfinite" (pixels left out of a sum that was used because a term was NaN).  The sums are exact
    integers; each pixel term carries the Q30 rounding (2^-31)."""
    s = np.asarray(records)
    if objective == "epe":
        if like != "test" or smooth_second_order or pme_criterion != "OBCC" or pme_beta != 1.0 or pme_gamma != 1.0 or ssim_alpha is not None:
            raise ValueError("loss_summary: objective='epe' takes size_average, weights, flow_scale and count only (train.lua is its definition; "
                             "there is no like='test' of it)")
        return _loss_summary_epe(s, size_average, weights, flow_scale, count)
    if s.dtype != np.uint64 or s.shape[-1:] not in ((LOSS_WORDS,), (LOSS_FT_WORDS,), (LOSS_SSIM_WORDS,), (LOSS_PLAIN_WORDS,)) or s.ndim not in (2, 3):
        raise ValueError("loss_summary: expected uint64 records of shape (n, L, w) or (L, w) with w = %d, %d, %d or %d, got %s %r"
                         % (LOSS_WORDS, LOSS_FT_WORDS, LOSS_SSIM_WORDS, LOSS_PLAIN_WORDS, s.dtype, s.shape))
    if like not in ("test", "train"):
        raise ValueError("loss_summary: like must be 'test' or 'train'")
    wt = dict(LOSS_WEIGHTS)
    if objective is not None:
        if objective not in LOSS_OBJECTIVES:
            raise ValueError("loss_summary: unknown objective %r (one of %s)" % (objective, ", ".join(sorted(LOSS_OBJECTIVES))))
        if smooth_second_order or pme_criterion != "OBCC" or pme_beta != 1.0 or pme_gamma != 1.0:
            raise ValueError("loss_summary: objective=%r sets smooth_second_order, pme_criterion, pme_beta and pme_gamma itself" % (objective,))
        o = LOSS_OBJECTIVES[objective]
        smooth_second_order, pme_criterion, pme_beta, pme_gamma = o["smooth_second_order"], o["pme_criterion"], o["pme_beta"], o["pme_gamma"]
        wt.update(o["weights"])
    if pme_criterion not in ("OBCC", "OBGCC", "OSSIM", "OSSIML1", "BCC", "SSIM", "SSIML1"):
        raise ValueError("loss_summary: pme_criterion must be 'OBCC', 'OBGCC', 'OSSIM', 'OSSIML1', 'BCC', 'SSIM' or 'SSIML1'")
    plain = pme_criterion in ("BCC", "SSIM", "SSIML1")
    if plain and s.shape[-1] != LOSS_PLAIN_WORDS:
        raise ValueError("loss_summary: pme_criterion=%r needs the %d-word records of objective='plain', got records of %d words"
                         % (pme_criterion, LOSS_PLAIN_WORDS, s.shape[-1]))
    if pme_penalty not in ("L1", "Quadratic"):
        raise ValueError("loss_summary: pme_penalty must be 'L1' or 'Quadratic' (the Lorentzian penalty is not provided)")
    if pme_penalty == "Quadratic" and pme_criterion != "BCC":
        raise ValueError("loss_summary: pme_penalty='Quadratic' goes with pme_criterion='BCC' only (model.lua:189-190 replaces the penalty of every "
                         "other criterion by the L1 one or leaves it without effect)")
    gradients = pme_criterion == "OBGCC"
    ssim = pme_criterion in SSIM_ALPHA
    if ssim and s.shape[-1] != LOSS_SSIM_WORDS:
        raise ValueError("loss_summary: pme_criterion=%r needs the %d-word records of objective='ssim', got records of %d words"
                         % (pme_criterion, LOSS_SSIM_WORDS, s.shape[-1]))
    if ssim_alpha is not None and not ssim and pme_criterion not in PLAIN_ALPHA:
        raise ValueError("loss_summary: ssim_alpha goes with pme_criterion 'OSSIM', 'OSSIML1', 'SSIM' or 'SSIML1'")
    if ssim_alpha is not None and not (0.0 <= float(ssim_alpha) <= 1.0):
        raise ValueError("loss_summary: ssim_alpha must lie in [0, 1], got %r" % (ssim_alpha,))
    ft = s.shape[-1] == LOSS_FT_WORDS
    if not ft and (smooth_second_order or gradients or pme_beta != 1.0 or pme_gamma != 1.0):
        raise ValueError("loss_summary: only 24-word records carry second-order and gradient sums; compute them with objective='finetune'")
    s = s.reshape((-1,) + s.shape[-2:])
    n, L, _ = s.shape
    if L > len(LOSS_LEVEL_WEIGHTS):
        raise ValueError("loss_summary: at most %d levels" % len(LOSS_LEVEL_WEIGHTS))
    wt.update(weights or {})
    one = float(1 << 30)
    f = s.astype(np.float64)                    # a sum beyond 2^53 rounds by 2^-53 of itself here
    px = f[:, :, LOSS_PIXELS]
    w_fs, w_fp = (LOSS_FT_SMOOTH2_FLOW_Q30, LOSS_FT_SMOOTH2_PAST_Q30) if smooth_second_order else (LOSS_SMOOTH_FLOW_Q30, LOSS_SMOOTH_PAST_Q30)
    fs, fp, cv = f[:, :, w_fs] / one, f[:, :, w_fp] / one, f[:, :, LOSS_CONST_VEL_Q30] / one
    so, pr = f[:, :, LOSS_SMOOTH_OCC_Q30] / one, f[:, :, LOSS_PRIOR_OCC_Q30] / one
    photo = f[:, :, LOSS_PHOTO_OCHARB_Q30] + f[:, :, LOSS_PHOTO_OCHARB_Q30 + 1]
    if gradients:
        photo = photo + float(pme_beta) * (f[:, :, LOSS_FT_PHOTO_OGX_Q30] + f[:, :, LOSS_FT_PHOTO_OGX_Q30 + 1]) \
                      + float(pme_gamma) * (f[:, :, LOSS_FT_PHOTO_OGY_Q30] + f[:, :, LOSS_FT_PHOTO_OGY_Q30 + 1])
    if ssim:
        alpha = SSIM_ALPHA[pme_criterion] if ssim_alpha is None else float(ssim_alpha)
        photo = alpha * (f[:, :, LOSS_SSIM_Q30] + f[:, :, LOSS_SSIM_Q30 + 1]) + (1.0 - alpha) * (f[:, :, LOSS_SSIM_L1N_Q30] + f[:, :, LOSS_SSIM_L1N_Q30 + 1])
    pme = (photo / one + f[:, :, LOSS_PHOTO_OUTSIDE] + f[:, :, LOSS_PHOTO_OUTSIDE + 1]) / (3.0 * 2.0)
    if plain:   # no occlusion weight and no penalty_out (MBCCriterion.lua:89-99, MSSIML1Criterion.lua:140-150)
        if pme_criterion == "BCC":
            w_b = LOSS_PLAIN_L1_Q30 if pme_penalty == "L1" else LOSS_PLAIN_SQ_Q30
            photo = f[:, :, w_b] + f[:, :, w_b + 1]
        else:
            alpha = PLAIN_ALPHA[pme_criterion] if ssim_alpha is None else float(ssim_alpha)
            photo = alpha * (f[:, :, LOSS_PLAIN_SSIM_Q30] + f[:, :, LOSS_PLAIN_SSIM_Q30 + 1]) \
                    + (1.0 - alpha) * (f[:, :, LOSS_PLAIN_L1N_Q30] + f[:, :, LOSS_PLAIN_L1N_Q30 + 1])
        pme = photo / one / (3.0 * 2.0)
    if size_average:
        fs, fp, cv, so = fs / (2.0 * px), fp / (2.0 * px), cv / (2.0 * px), so / (2.0 * px)
        pme, pr = pme / px, pr / px
    soft = bool((s[:, :, LOSS_SMOOTH_PAST_Q30].any() or s[:, :, LOSS_CONST_VEL_Q30].any()))
    n_flow = float(wt.pop("n_flow", 2.0 if soft else 1.0))   # (weights={"n_flow": ...} overrides what the records suggest)
    S = n_flow * fs if like == "test" else fs + fp
    lw = np.asarray(LOSS_LEVEL_WEIGHTS[:L], np.float64)[None, :]
    level = wt["smooth_flow"] * S + wt["const_vel"] * cv + wt["pme"] * pme
    if not no_occ:   # train.lua:456, test.lua:289
        level = level + wt["smooth_occ"] * so + wt["prior_occ"] * pr
    level = lw * level
    loss = level.sum(axis=1)
    counted = [LOSS_NONFINITE, LOSS_PHOTO_NONFINITE, LOSS_PHOTO_NONFINITE + 1]
    counted += [LOSS_FT_SMOOTH2_NONFINITE] if smooth_second_order else []
    counted += [LOSS_FT_GRAD_NONFINITE] if gradients else []
    counted += [LOSS_SSIM_NONFINITE, LOSS_SSIM_NONFINITE + 1] if ssim else []
    counted += [LOSS_PLAIN_SSIM_NONFINITE, LOSS_PLAIN_SSIM_NONFINITE + 1] if pme_criterion in PLAIN_ALPHA else []
    nonf = int(sum(int(v) for v in s[:, :, counted].ravel()))
    return {"smooth_flow": fs, "smooth_past": fp, "const_vel": cv, "pme": pme, "smooth_occ": so, "prior_occ": pr, "level": level,
            "loss": loss, "mean": float(loss.mean()), "nonfinite": nonf}


def _epe_weights(who, weights):
    """(epe, occ, level weights) from a `weights` dict over the defaults of b2f_loss_epe_defaults; negative and non-finite ones raise"""
    wt = {"epe": 1.0, "occ": 0.0, "level_weights": LOSS_LEVEL_WEIGHTS}
    for k, v in (weights or {}).items():
        if k not in wt:
            raise ValueError(who + ": unknown weight %r (one of 'epe', 'occ', 'level_weights')" % (k,))
        wt[k] = v
    lw = [float(t) for t in wt["level_weights"]]
    if len(lw) > len(LOSS_LEVEL_WEIGHTS):
        raise ValueError(who + ": at most %d level weights" % len(LOSS_LEVEL_WEIGHTS))
    lw = lw + list(LOSS_LEVEL_WEIGHTS[len(lw):])
    for k, t in [("epe", float(wt["epe"])), ("occ", float(wt["occ"]))] + [("level_weights", t) for t in lw]:
        if not (t >= 0.0 and np.isfinite(t)):
            raise ValueError(who + ": %s must be finite and >= 0, got %r" % (k, t))
    return float(wt["epe"]), float(wt["occ"]), lw


def loss_epe_options(weights=None, size_average=False):
    """The options of the supervised objective, -optimize epe (a _lib.LossEpeOpts, b2f_loss_epe_opts of include/b2f.h), from
    b2f_loss_epe_defaults: epe 1 (-epe), occ 0, the level weights of train.lua:56-58, sizeAverage off.  `weights` replaces "epe", "occ"
    and, as "level_weights", the first level weights (at most 7).  occ > 0 switches on the occlusion term that train.lua:316-332
    intends (the Lua as written cannot run); it needs gt_occ.  size_average=True: every level weight counts as 1 (train.lua:60-64)
    and a level is divided by its valid resp. labelled pixels (L2Criterion.lua:40-42,66-68)."""
    o = _lib.LossEpeOpts()
    _lib.check(_lib.lib().b2f_loss_epe_defaults(C.byref(o)))
    o.epe, o.occ, lw = _epe_weights("loss_epe_options", weights)
    for j, t in enumerate(lw):
        o.level_weights[j] = t
    o.size_average = 1 if size_average else 0
    return o


def epe_count_args(count, L, who, batch_ok=True):
    """(count_mode, counts) of a b2f_*_epe entry.  count: "batch" (N_j over the call's images, mask:sum() of L2Criterion.lua:34,56),
    "image" (each image's own) or L x 2 numbers (valid, labelled pixels per level)."""
    if isinstance(count, str):
        modes = {"batch": EPE_COUNT_BATCH, "image": EPE_COUNT_IMAGE}
        if count not in modes or (count == "batch" and not batch_ok):
            raise ValueError("%s: count must be %s'image' or an L x 2 array, got %r" % (who, "'batch', " if batch_ok else "", count))
        return (modes[count], None)
    r = np.ascontiguousarray(count, np.float64)
    if r.shape != (L, 2):
        raise ValueError("%s: a count array must have shape (%d, 2): valid, labelled pixels per level; got %r" % (who, L, r.shape))
    return (EPE_COUNT_GIVEN, r.ctypes.data_as(C.POINTER(C.c_double)))   # (the pointer keeps r alive)


def _epe_opts_ptr(options):
    if options is None:
        return None
    if not isinstance(options, _lib.LossEpeOpts):
        raise ValueError("objective 'epe': expected the result of back2future.loss_epe_options (or None for the defaults)")
    return C.byref(options)


def _loss_summary_epe(records, size_average=False, weights=None, flow_scale=20.0, count="batch"):
    """The supervised objective of train.lua:296-334 from its records (uint64 n x L x 8 or L x 8; ops.table_loss_epe).  Per level j
        flow_j = epe * lw_j * sum EPE_Q20 / 2^20,    occ_j = occ * lw_j * sum OCC_Q20 / 2^20
    summed over the records' images as criterion:forward sums over its batch (train.lua:312-313,328-329; lw: train.lua:56-58);
    size_average=True: lw_j = 1 and each sum is divided by N_j = VALID + FLOW_NONFINITE resp. N'_j = LABELLED + OCC_NONFINITE
    (mask:sum(), L2Criterion.lua:34,40-42), taken over all records (count="batch"), per image, the per-image values then added
    ("image"), or from an L x 2 array; a level without a counted pixel adds 0.  weights: "epe", "occ", "level_weights" as for
    loss_epe_options (the occlusion sums are 0 unless the records were made with occ > 0).  Returns a dict: "flow" and "occ" (L
    float64 each, weighted), "err" (their sum over the levels, what train.lua accumulates), "epe" (flow_scale * sum EPE_Q20[level 0] /
    2^20 / sum VALID[level 0], train.lua:340-344; nan without a valid pixel) and "nonfinite".  The sums are exact integers; each pixel
    term carries the Q20 rounding (2^-21)."""
    s = np.asarray(records)
    if s.dtype != np.uint64 or s.shape[-1:] != (LOSS_EPE_WORDS,) or s.ndim not in (2, 3):
        raise ValueError("loss_summary: objective='epe' expects uint64 records of shape (n, L, %d) or (L, %d), got %s %r"
                         % (LOSS_EPE_WORDS, LOSS_EPE_WORDS, s.dtype, s.shape))
    s = s.reshape((-1,) + s.shape[-2:])
    n, L, _ = s.shape
    if L > len(LOSS_LEVEL_WEIGHTS):
        raise ValueError("loss_summary: at most %d levels" % len(LOSS_LEVEL_WEIGHTS))
    w_epe, w_occ, lw = _epe_weights("loss_summary", weights)
    one = float(1 << 20)
    parts = []
    for w_sum, w_cnt, w_nonf in ((LOSS_EPE_Q20, LOSS_EPE_VALID, LOSS_EPE_FLOW_NONFINITE), (LOSS_EPE_OCC_Q20, LOSS_EPE_LABELLED, LOSS_EPE_OCC_NONFINITE)):
        t = len(parts)
        level = np.zeros(L, np.float64)
        for j in range(L):
            q = [int(v) for v in s[:, j, w_sum]]
            if not size_average:
                level[j] = sum(q) / one
                continue
            if isinstance(count, str) and count in ("batch", "image"):
                N = [int(a) + int(b) for a, b in zip(s[:, j, w_cnt], s[:, j, w_nonf])]
                N = [sum(N)] * n if count == "batch" else N
            elif isinstance(count, str):
                raise ValueError("loss_summary: count must be 'batch', 'image' or an L x 2 array, got %r" % (count,))
            else:
                c = np.asarray(count, np.float64)
                if c.shape != (L, 2):
                    raise ValueError("loss_summary: a count array must have shape (%d, 2), got %r" % (L, c.shape))
                N = [float(c[j, t])] * n
            level[j] = sum((qi / one) / Ni for qi, Ni in zip(q, N) if Ni > 0)
        parts.append(level)
    lwj = np.ones(L) if size_average else np.asarray(lw[:L], np.float64)
    flow, occ = w_epe * lwj * parts[0], w_occ * lwj * parts[1]
    valid0 = int(s[:, 0, LOSS_EPE_VALID].sum())
    epe = float(flow_scale) * (sum(int(v) for v in s[:, 0, LOSS_EPE_Q20]) / one) / valid0 if valid0 else float("nan")
    nonf = int(s[:, :, LOSS_EPE_FLOW_NONFINITE].sum()) + int(s[:, :, LOSS_EPE_OCC_NONFINITE].sum())
    return {"flow": flow, "occ": occ, "err": float(flow.sum() + occ.sum()), "epe": epe, "nonfinite": nonf}


def _apply_grad_weights(who, o, wt):
    """the weights of loss_grad_options / loss_grad_ft_options into the options struct"""
    for k, v in wt.items():
        if k == "level_weights":
            v = [float(t) for t in v]
            if len(v) > len(LOSS_LEVEL_WEIGHTS):
                raise ValueError(who + ": at most %d level weights" % len(LOSS_LEVEL_WEIGHTS))
            bad = [t for t in v if not (t >= 0.0 and np.isfinite(t))]
            for j, t in enumerate(v):
                o.level_weights[j] = t
        elif k in LOSS_WEIGHTS:
            bad = [] if (float(v) >= 0.0 and np.isfinite(float(v))) else [v]
            setattr(o, k, float(v))
        else:
            raise ValueError(who + ": unknown weight %r" % (k,))
        if bad:
            raise ValueError(who + ": %s must be finite and >= 0, got %r" % (k, bad[0]))


def loss_grad_options(weights=None, size_average=False, objective=None):
    """The options of the gradient table of train.lua:428-468 (a _lib.LossGradOpts, b2f_loss_grad_opts of include/b2f.h), from
    b2f_loss_grad_defaults: the weights of opts.lua:61-73, the level weights of test.lua:29-31, sizeAverage off.  objective=NAME
    applies the weights of LOSS_OBJECTIVES[NAME] first; only "Ours-Hard" is accepted: the two Soft models were fine-tuned with
    SecondOrderSmoothnessCriterion and OBGCCriterion, whose gradients are not provided.  `weights` then replaces any of
    "smooth_flow", "const_vel", "pme", "smooth_occ", "prior_occ" and, as "level_weights", the first level weights (at most 7).  A
    weight of exactly 0 switches its term off (it is not evaluated); negative and non-finite weights are refused."""
    o = _lib.LossGradOpts()
    _lib.check(_lib.lib().b2f_loss_grad_defaults(C.byref(o)))
    wt = {}
    if objective is not None:
        if objective not in LOSS_OBJECTIVES:
            raise ValueError("loss_grad_options: unknown objective %r (one of %s)" % (objective, ", ".join(sorted(LOSS_OBJECTIVES))))
        ob = LOSS_OBJECTIVES[objective]
        if ob["smooth_second_order"] or ob["pme_criterion"] != "OBCC":
            raise ValueError("loss_grad_options: the gradient of objective %r is not provided: it uses SecondOrderSmoothnessCriterion and "
                             "OBGCCriterion, and only the gradients of the first-order pme objective (\"Ours-Hard\") are" % (objective,))
        wt.update(ob["weights"])
    wt.update(weights or {})
    _apply_grad_weights("loss_grad_options", o, wt)
    o.size_average = 1 if size_average else 0
    return o


def loss_grad_ft_options(weights=None, size_average=False, objective=None, smooth_second_order=None, pme_criterion=None, pme_alpha=None,
                         pme_beta=None, pme_gamma=None):
    """The options of the gradient table for objectives with SecondOrderSmoothnessCriterion and / or OBGCCriterion (a
    _lib.LossGradFtOpts, b2f_loss_grad_ft_opts of include/b2f.h), from b2f_loss_grad_ft_defaults: those of loss_grad_options,
    -smooth_second_order on, -pme_criterion OBGCC, alpha = beta = gamma = 1.  objective=NAME (any of LOSS_OBJECTIVES) applies the
    weights, the two flags and alpha, beta, gamma the named model was trained with first (gamma as given: LOSS_OBJECTIVES);
    `weights` and the five keywords then replace what they name.  pme_criterion: "OBCC" or "OBGCC".  A weight of exactly 0, alpha, beta
    and gamma included, switches its term off; negative and non-finite ones are refused.  Every entry point that takes the options of
    loss_grad_options takes these too."""
    o = _lib.LossGradFtOpts()
    _lib.check(_lib.lib().b2f_loss_grad_ft_defaults(C.byref(o)))
    wt = {}
    if objective is not None:
        if objective not in LOSS_OBJECTIVES:
            raise ValueError("loss_grad_ft_options: unknown objective %r (one of %s)" % (objective, ", ".join(sorted(LOSS_OBJECTIVES))))
        ob = LOSS_OBJECTIVES[objective]
        wt.update(ob["weights"])
        o.smooth_second_order = 1 if ob["smooth_second_order"] else 0
        o.pme_criterion = 1 if ob["pme_criterion"] == "OBGCC" else 0
        o.pme_alpha, o.pme_beta, o.pme_gamma = ob["pme_alpha"], ob["pme_beta"], ob["pme_gamma"]
    wt.update(weights or {})
    _apply_grad_weights("loss_grad_ft_options", o, wt)
    if smooth_second_order is not None:
        o.smooth_second_order = 1 if smooth_second_order else 0
    if pme_criterion is not None:
        if pme_criterion not in ("OBCC", "OBGCC"):
            raise ValueError("loss_grad_ft_options: pme_criterion must be 'OBCC' or 'OBGCC'")
        o.pme_criterion = 1 if pme_criterion == "OBGCC" else 0
    for k, v in (("pme_alpha", pme_alpha), ("pme_beta", pme_beta), ("pme_gamma", pme_gamma)):
        if v is not None:
            if not (float(v) >= 0.0 and np.isfinite(float(v))):
                raise ValueError("loss_grad_ft_options: %s must be finite and >= 0, got %r" % (k, v))
            setattr(o, k, float(v))
    o.size_average = 1 if size_average else 0
    return o


def loss_grad_ssim_options(weights=None, size_average=False, smooth_second_order=False, pme_criterion="OSSIML1", ssim_alpha=None):
    """The options of the gradient table with the occlusion-aware SSIM + L1 photometric term (a _lib.LossGradSsimOpts,
    b2f_loss_grad_ssim_opts of include/b2f.h; criterions/OSSIML1Criterion.lua:165-302), from b2f_loss_grad_ssim_defaults: those of
    loss_grad_options, -smooth_second_order off, alpha 0.85.  pme_criterion: "OSSIML1" or "OSSIM" (SSIM_ALPHA); an explicit
    ssim_alpha, finite and in [0, 1], overrides its value.  Every entry point that takes the options of loss_grad_options takes these
    too, with a keyword ssim_range as for the objective "ssim"."""
    o = _lib.LossGradSsimOpts()
    _lib.check(_lib.lib().b2f_loss_grad_ssim_defaults(C.byref(o)))
    _apply_grad_weights("loss_grad_ssim_options", o, dict(weights or {}))
    if pme_criterion not in SSIM_ALPHA:
        raise ValueError("loss_grad_ssim_options: pme_criterion must be 'OSSIML1' or 'OSSIM'")
    o.ssim_alpha = SSIM_ALPHA[pme_criterion]
    if ssim_alpha is not None:
        if not (0.0 <= float(ssim_alpha) <= 1.0):
            raise ValueError("loss_grad_ssim_options: ssim_alpha must be in [0, 1], got %r" % (ssim_alpha,))
        o.ssim_alpha = float(ssim_alpha)
    o.smooth_second_order = 1 if smooth_second_order else 0
    o.size_average = 1 if size_average else 0
    return o


def loss_grad_plain_options(weights=None, size_average=False, smooth_second_order=False, pme_criterion="BCC", pme_penalty="L1", ssim_alpha=None,
                            no_occ=False):
    """The options of the gradient table with the photometric terms that do not mask occlusions (a _lib.LossGradPlainOpts,
    b2f_loss_grad_plain_opts of include/b2f.h; criterions/MBCCriterion.lua:104-186, MSSIML1Criterion.lua:155-261), from
    b2f_loss_grad_plain_defaults: those of loss_grad_options, -smooth_second_order off, BCC with the L1 penalty.  pme_criterion: "BCC",
    "SSIM" or "SSIML1" (PLAIN_ALPHA; an explicit ssim_alpha, finite and in [0, 1], overrides its value); pme_penalty: "L1" or, with
    "BCC" only, "Quadratic" (model.lua:189-190).  no_occ=True (opts.lua:85, train.lua:456) sets the weights of the occlusions'
    smoothness and prior to 0, after `weights`: the occlusion planes of the gradient are then +0.0.  Every entry point that takes the
    options of loss_grad_options takes these too, with a keyword ssim_range as for the objective "plain"."""
    o = _lib.LossGradPlainOpts()
    _lib.check(_lib.lib().b2f_loss_grad_plain_defaults(C.byref(o)))
    _apply_grad_weights("loss_grad_plain_options", o, dict(weights or {}))
    if pme_criterion not in ("BCC", "SSIM", "SSIML1"):
        raise ValueError("loss_grad_plain_options: pme_criterion must be 'BCC', 'SSIM' or 'SSIML1'")
    if pme_penalty not in ("L1", "Quadratic"):
        raise ValueError("loss_grad_plain_options: pme_penalty must be 'L1' or 'Quadratic' (the Lorentzian penalty is not provided)")
    if pme_penalty == "Quadratic" and pme_criterion != "BCC":
        raise ValueError("loss_grad_plain_options: pme_penalty='Quadratic' goes with pme_criterion='BCC' only")
    if ssim_alpha is not None and pme_criterion == "BCC":
        raise ValueError("loss_grad_plain_options: ssim_alpha goes with pme_criterion 'SSIM' or 'SSIML1'")
    o.criterion = PLAIN_BCC if pme_criterion == "BCC" else PLAIN_SSIM
    o.penalty = PLAIN_QUADRATIC if pme_penalty == "Quadratic" else PLAIN_L1
    o.ssim_alpha = PLAIN_ALPHA.get(pme_criterion, 0.85)
    if ssim_alpha is not None:
        if not (0.0 <= float(ssim_alpha) <= 1.0):
            raise ValueError("loss_grad_plain_options: ssim_alpha must be in [0, 1], got %r" % (ssim_alpha,))
        o.ssim_alpha = float(ssim_alpha)
    o.smooth_second_order = 1 if smooth_second_order else 0
    o.size_average = 1 if size_average else 0
    if no_occ:
        o.smooth_occ = o.prior_occ = 0.0
    return o


def _grad_opts_ptr(options):
    if options is None:
        return None
    if not isinstance(options, (_lib.LossGradOpts, _lib.LossGradFtOpts, _lib.LossGradSsimOpts, _lib.LossGradPlainOpts)):
        raise ValueError("expected the result of back2future.loss_grad_options or loss_grad_ft_options, of loss_grad_ssim_options or of "
                         "loss_grad_plain_options (or None for the defaults)")
    return C.byref(options)


def _grad_entry(name, options):
    """the entry `name` of the library for these options: b2f_*_grad* or, for loss_grad_ft_options / loss_grad_ssim_options, its
    b2f_*_grad_ft* / b2f_*_grad_ssim* twin"""
    if isinstance(options, _lib.LossGradFtOpts):
        name = name.replace("_grad", "_grad_ft", 1)
    elif isinstance(options, _lib.LossGradSsimOpts):
        name = name.replace("_grad", "_grad_ssim", 1)
    elif isinstance(options, _lib.LossGradPlainOpts):
        name = name.replace("_grad", "_grad_plain", 1)
    return getattr(_lib.lib(), name)


def _grad_words(options):
    """words per record beside a gradient table: the fine-tuning options give the 24-word records of objective "finetune", the SSIM +
    L1 options the 32-word records of objective "ssim", the options of loss_grad_plain_options the 40-word records of objective "plain"""
    if isinstance(options, _lib.LossGradPlainOpts):
        return LOSS_PLAIN_WORDS
    return LOSS_FT_WORDS if isinstance(options, _lib.LossGradFtOpts) else LOSS_SSIM_WORDS if isinstance(options, _lib.LossGradSsimOpts) else LOSS_WORDS


def _grad_range_args(options, ssim_range, L, who, batch_ok=True):
    """the trailing (range_mode, ranges) of a b2f_*_grad_ssim or b2f_*_grad_plain entry (ssim_range_args), () for the other options"""
    return ssim_range_args("ssim", ssim_range, L, who, batch_ok) if isinstance(options, (_lib.LossGradSsimOpts, _lib.LossGradPlainOpts)) else ()


def _forward_loss_grad(fn, h, x, flow_scale, options, shapes, L, want_loss, want_table, tail=()):
    """x n x 9 x H x W normalized -> (gradient table, records or None, table or None): b2f_forward_loss_grad / b2f_multi_forward_loss_grad;
    tail: _grad_range_args"""
    x = _lib.f32(x)
    if x.ndim != 4 or x.shape[1] != 9:
        raise ValueError("forwardLossGrad: expected an n x 9 x H x W normalized input, got shape %r" % (x.shape,))
    n, _, H, W = x.shape
    sh = shapes(H, W)
    grad = [np.empty((n, c, hh, ww), np.float32) for (c, hh, ww) in sh]
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])
    loss = np.empty((n, L, _grad_words(options)), np.uint64) if want_loss else None
    lp = loss.ctypes.data_as(C.POINTER(C.c_ulonglong)) if want_loss else None
    outs = [np.empty((n, c, hh, ww), np.float32) for (c, hh, ww) in sh] if want_table else None
    op = (_lib.c_float_p * len(outs))(*[_lib.fptr(t) for t in outs]) if want_table else None
    _lib.check(fn(h, _lib.fptr(x), n, H, W, float(flow_scale), _grad_opts_ptr(options), lp, gp, len(grad), op, *tail))
    return grad, loss, outs


def _forward_loss_epe(fn, h, who, x, gt_flow, valid, gt_occ, flow_scale, options, count, shapes, L, want_loss, want_grad, want_table, multi=False):
    """x n x 9 x H x W normalized and its ground truth -> (records or None, gradient table or None, table or None):
    b2f_forward_loss_epe / b2f_multi_forward_loss_epe (train.lua:296-334 behind model:forward)"""
    x = _lib.f32(x)
    if x.ndim != 4 or x.shape[1] != 9:
        raise ValueError("%s: expected an n x 9 x H x W normalized input, got shape %r" % (who, x.shape))
    if gt_flow is None:
        raise ValueError("%s: objective='epe' needs gt_flow (n x 2 x H x W, pixels)" % who)
    n, _, H, W = x.shape
    gt, va, lb = score_ground_truth(n, H, W, gt_flow, valid, gt_occ, who)
    sh = shapes(H, W)
    mode, counts = epe_count_args(count, L, who, batch_ok=not multi)
    loss = np.empty((n, L, LOSS_EPE_WORDS), np.uint64) if want_loss else None
    lp = loss.ctypes.data_as(C.POINTER(C.c_ulonglong)) if want_loss else None
    grad = [np.empty((n, c, hh, ww), np.float32) for (c, hh, ww) in sh] if want_grad else None
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad]) if want_grad else None
    outs = [np.empty((n, c, hh, ww), np.float32) for (c, hh, ww) in sh] if want_table else None
    op = (_lib.c_float_p * len(outs))(*[_lib.fptr(t) for t in outs]) if want_table else None
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    args = (h, _lib.fptr(x), n, H, W, _lib.fptr(gt), u8p(va), u8p(lb), float(flow_scale), _epe_opts_ptr(options), mode, counts, lp, gp, len(sh))
    _lib.check(fn(*(args if multi else args + (op,))))
    return loss, grad, outs


def _forward_loss(fn, h, x, flow_scale, L, shapes, words=LOSS_WORDS):
    """x n x 9 x H x W normalized -> (records uint64 n x L x words, table or None): b2f_forward_loss* / b2f_multi_forward_loss*"""
    x = _lib.f32(x)
    if x.ndim != 4 or x.shape[1] != 9:
        raise ValueError("forwardLoss: expected an n x 9 x H x W normalized input, got shape %r" % (x.shape,))
    n, _, H, W = x.shape
    loss = np.empty((n, L, words), np.uint64)
    lp = loss.ctypes.data_as(C.POINTER(C.c_ulonglong))
    if shapes is None:
        _lib.check(fn(h, _lib.fptr(x), n, H, W, float(flow_scale), lp))
        return loss, None
    outs = [np.empty((n, c, hh, ww), np.float32) for (c, hh, ww) in shapes(H, W)]
    ptrs = (_lib.c_float_p * len(outs))(*[_lib.fptr(o) for o in outs])
    _lib.check(fn(h, _lib.fptr(x), n, H, W, float(flow_scale), lp, ptrs, len(outs)))
    return loss, outs


class Model(object):
    """Owns a b2f_ctx (the `model` global of back2future.lua:113)."""

    def __init__(self, name="Ours-Soft-ft-KITTI", device=0, graph=None):
        """graph: createModelMulti options other than the shipped ones, e.g. "win=5,levels=4" (b2f_init_ex)."""
        L = _lib.lib()
        h = C.c_void_p()
        _lib.check(L.b2f_init_ex(name.encode() if name is not None else None, int(device),
                                 graph.encode() if graph else None, C.byref(h)))
        self._h = h
        self._streams = []
        self.name = name
        self.device = int(device)
        lv, win, pf, no, npar = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        _lib.check(L.b2f_info(h, C.byref(lv), C.byref(win), C.byref(pf), C.byref(no), C.byref(npar)))
        self.levels, self.win, self.past_flow = lv.value, win.value, bool(pf.value)
        self.n_outputs, self.n_params = no.value, npar.value

    def close(self):
        if getattr(self, "_h", None):
            for ref in list(getattr(self, "_streams", [])):   # the context owns its streams: b2f_destroy would free them under their wrappers
                if ref() is not None:
                    ref().close()
            if _lib is not None:            # None while the interpreter tears the module down
                _lib.lib().b2f_destroy(self._h)
            self._h = None

    __del__ = close

    # -- weights --
    def set_weights(self, flat):
        flat = _lib.f32(flat).ravel()
        _lib.check(_lib.lib().b2f_set_weights(self._h, _lib.fptr(flat), flat.size))
        self.past_flow = flat.size == _lib.lib().b2f_param_count(1)
        self.n_params = flat.size

    def get_weights(self):
        out = np.empty(self.n_params, np.float32)
        _lib.check(_lib.lib().b2f_get_weights(self._h, _lib.fptr(out), out.size))
        return out

    def weights_device_ptr(self):
        p, n = C.c_void_p(), C.c_longlong()
        _lib.check(_lib.lib().b2f_weights_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def commit_weights(self):
        _lib.check(_lib.lib().b2f_commit_weights(self._h))

    def set_option(self, key, value):
        _lib.check(_lib.lib().b2f_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int()
        _lib.check(_lib.lib().b2f_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def options(self, **kv):
        """Context manager: set options for the duration of a `with` block, then restore the previous values."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            old = {k: self.get_option(k) for k in kv}
            try:
                for k, v in kv.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return _cm()

    def synchronize(self):
        _lib.check(_lib.lib().b2f_synchronize(self._h))

    def arena_check(self, detail=False):
        """b2f_arena_check (tests; options arena_guard / arena_fill): the number of guard words of the workspace that a kernel has
        overwritten since the workspace was filled.  detail: (count, buffer index, offset, message) with the first such word."""
        i, off = C.c_int(), C.c_longlong()
        n = _lib.lib().b2f_arena_check(self._h, C.byref(i), C.byref(off))
        if n < 0:
            _lib.check(1)
        if not detail:
            return n
        return n, i.value, off.value, (_lib.lib().b2f_last_error().decode("utf-8", "replace") if n else "")

    def guard_selftest(self, which):
        """b2f_guard_selftest: overwrite one guard word from the host (0 / 1: the workspace's, 2 / 3: a guarded op-level buffer's, 4 / 5: one of an op-level staging scope's three)."""
        _lib.check(_lib.lib().b2f_guard_selftest(self._h, int(which)))

    def profile_reset(self):
        _lib.check(_lib.lib().b2f_profile_reset(self._h))

    def profile_read(self):
        cap = 256
        while True:     # the library returns at most cap rows and keeps every row name a context has ever used: a full buffer may be cut
            names = C.create_string_buffer(32 * cap)
            ms = (C.c_double * cap)()
            cnt = (C.c_longlong * cap)()
            n = C.c_int()
            _lib.check(_lib.lib().b2f_profile_read(self._h, names, ms, cnt, cap, C.byref(n)))
            if n.value < cap:
                break
            cap *= 4
        out = {}
        for i in range(n.value):
            nm = names.raw[32 * i:32 * i + 32].split(b"\0", 1)[0].decode()
            out[nm] = (ms[i], cnt[i])
        return out

    # -- the hot path --
    def computeFlow(self, im1, im2, im3):
        """computeFlow(im1, im2, im3) of back2future.lua:47-95."""
        im1, im2, im3 = _lib.f32(im1), _lib.f32(im2), _lib.f32(im3)
        assert im1.ndim == 3 and im1.shape[0] == 3 and im1.shape == im2.shape == im3.shape, \
            "expected three 3 x H x W images"
        _, H0, W0 = im1.shape
        flow = np.empty((2, H0, W0), np.float64)
        fwd = np.empty((1, H0, W0), np.uint8)
        bwd = np.empty((1, H0, W0), np.uint8)
        _lib.check(_lib.lib().b2f_compute_flow(
            self._h, _lib.fptr(im1), _lib.fptr(im2), _lib.fptr(im3), H0, W0,
            flow.ctypes.data_as(C.POINTER(C.c_double)), fwd.ctypes.data_as(C.POINTER(C.c_ubyte)),
            bwd.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return flow, fwd, bwd

    def computeFlowBatch(self, im1, im2, im3, out=None, dtype=np.float64, occ_prob=False):
        """n independent triplets at once: inputs n x 3 x H x W.  The library pipelines sub-batches through
        pinned staging buffers; inputs / `out` = (flow f64 n x 2 x H x W, fwd u8 n x 1 x H x W, bwd) that already
        live in page-locked memory (e.g. views of torch pin_memory() tensors) are DMA'd in place instead.
        uint8 inputs (frames as decoded from 8-bit files, value = byte / 255) are uploaded as bytes.
        dtype=np.float32 (b2f_compute_flow_batch_f32): the flow is the float64 one rounded to float32, bit for bit, and
        never widened on the host; occ_prob=True (float32 only) appends the n x 2 x H x W occlusion probabilities to the
        returned tuple.  `out` then holds float32 flow / occ_prob buffers, and its masks may be None (not computed)."""
        return _compute_flow_batch("b2f_", self._h, im1, im2, im3, out, dtype, occ_prob)

    def computeFlowSequence(self, frames, out=None, dtype=np.float64, occ_prob=False):
        """Flow for every centre frame of a video: frames is a T x 3 x H x W float32 or uint8 array (or a list of 3 x H x W
        arrays); output i is computeFlow(frames[i], frames[i+1], frames[i+2]), i = 0 .. T-3, with the shapes and dtypes of
        computeFlowBatch.  Every frame is uploaded and run through the feature pyramid once (b2f_compute_flow_sequence).
        dtype / occ_prob / out as for computeFlowBatch (dtype=np.float32: b2f_compute_flow_sequence_f32)."""
        return _compute_flow_sequence("b2f_", self._h, frames, out, dtype, occ_prob)

    def computeFlowDevice(self, d_im1, d_im2, d_im3, n, H0, W0, d_flow, d_occ_prob=None, d_fwd_occ=None, d_bwd_occ=None,
                          in_kind=IN_UNIT, stream=None):
        """b2f_compute_flow_device on device pointers (ints): computeFlowBatch(dtype=np.float32) on frames that are already
        in GPU memory, any H0 x W0.  d_im1..3: n x 3 x H0 x W0 float32 in [0,1] (in_kind=IN_UNIT) or uint8 (IN_U8);
        d_flow / d_occ_prob: n x 2 x H0 x W0 float32, the masks n x H0 x W0 uint8 (all but d_flow may be None).
        Asynchronous on `stream`."""
        p = lambda v: C.c_void_p(v) if v else None
        _lib.check(_lib.lib().b2f_compute_flow_device(self._h, int(n), int(in_kind), p(d_im1), p(d_im2), p(d_im3), int(H0), int(W0),
                                                       p(d_flow), p(d_occ_prob), p(d_fwd_occ), p(d_bwd_occ), p(stream)))

    def computeFlowSequenceDevice(self, d_frames, T, H0, W0, d_flow, d_occ_prob=None, d_fwd_occ=None, d_bwd_occ=None,
                                  in_kind=IN_UNIT, stream=None):
        """b2f_compute_flow_sequence_device on device pointers (ints): computeFlowSequence(dtype=np.float32) on T x 3 x H0 x W0
        device frames (float32 in [0,1] with in_kind=IN_UNIT, uint8 with IN_U8); outputs as computeFlowDevice with n = T - 2.
        Asynchronous on `stream`."""
        if T < 3:
            raise ValueError("computeFlowSequenceDevice: a sequence needs T >= 3 frames, got %d" % T)
        p = lambda v: C.c_void_p(v) if v else None
        _lib.check(_lib.lib().b2f_compute_flow_sequence_device(self._h, int(T), int(in_kind), p(d_frames), int(H0), int(W0), p(d_flow),
                                                                p(d_occ_prob), p(d_fwd_occ), p(d_bwd_occ), p(stream)))

    def computeFlowBatchPast(self, im1, im2, im3, out=None, occ_prob=False):
        """computeFlowBatch(dtype=np.float32) of a Soft model with its past flow (b2f_compute_flow_batch_past): returns (flow,
        past_flow, fwd_occ, bwd_occ[, occ_prob]).  past_flow is the network's skip_ubfs[3] (models/pwc.lua:328-385), float32
        n x 2 x H x W, a raw flow rescaled like flow: the past frame is sampled at x - past_flow * 20, and under constant velocity
        past_flow == flow.  The other outputs are computeFlowBatch(dtype=np.float32)'s, bit for bit.  out = those buffers (its masks
        may be None).  A Hard model has no past flow and is refused."""
        return _compute_flow_batch_past("b2f_", self._h, im1, im2, im3, out, occ_prob)

    def computeFlowSequencePast(self, frames, out=None, occ_prob=False):
        """computeFlowSequence(dtype=np.float32) of a Soft model with its past flow (b2f_compute_flow_sequence_past): (flow, past_flow,
        fwd_occ, bwd_occ[, occ_prob]) with n = T - 2; output i belongs to centre frame i + 1, whose past frame is frame i."""
        return _compute_flow_sequence_past("b2f_", self._h, frames, out, occ_prob)

    def computeFlowDevicePast(self, d_im1, d_im2, d_im3, n, H0, W0, d_flow, d_past_flow, d_occ_prob=None, d_fwd_occ=None, d_bwd_occ=None,
                              in_kind=IN_UNIT, stream=None):
        """b2f_compute_flow_device_past on device pointers (ints): computeFlowDevice with the past flow of a Soft model in d_past_flow
        (n x 2 x H0 x W0 float32).  Asynchronous on `stream`."""
        p = lambda v: C.c_void_p(v) if v else None
        _lib.check(_lib.lib().b2f_compute_flow_device_past(self._h, int(n), int(in_kind), p(d_im1), p(d_im2), p(d_im3), int(H0), int(W0),
                                                            p(d_flow), p(d_past_flow), p(d_occ_prob), p(d_fwd_occ), p(d_bwd_occ), p(stream)))

    def computeFlowSequenceDevicePast(self, d_frames, T, H0, W0, d_flow, d_past_flow, d_occ_prob=None, d_fwd_occ=None, d_bwd_occ=None,
                                      in_kind=IN_UNIT, stream=None):
        """b2f_compute_flow_sequence_device_past on device pointers (ints): computeFlowSequenceDevice with the past flow of a Soft
        model in d_past_flow ((T - 2) x 2 x H0 x W0 float32).  Asynchronous on `stream`."""
        if T < 3:
            raise ValueError("computeFlowSequenceDevicePast: a sequence needs T >= 3 frames, got %d" % T)
        p = lambda v: C.c_void_p(v) if v else None
        _lib.check(_lib.lib().b2f_compute_flow_sequence_device_past(self._h, int(T), int(in_kind), p(d_frames), int(H0), int(W0), p(d_flow),
                                                                     p(d_past_flow), p(d_occ_prob), p(d_fwd_occ), p(d_bwd_occ), p(stream)))

    def openStream(self, H0, W0, cams=1, dtype=np.uint8, warp=False, past=False):
        """A FlowStream of `cams` cameras delivering H0 x W0 frames of `dtype` (np.uint8 or np.float32 in [0,1]) one at a time.
        warp=True: the stream keeps the caller's frames of its last three pushes, for pushWarp / pushDeviceWarp; past=True (Soft
        models): it may return the past flow, for pushPast and the own_past_flow / want_past keywords of pushWarp.  With either the
        stream is a MotionStream, the FlowStream that has those pushes."""
        if not getattr(self, "_h", None):
            raise ValueError("openStream: the model is closed")
        return MotionStream(self, H0, W0, cams, dtype, warp, past) if (warp or past) else FlowStream(self, H0, W0, cams, dtype)

    def computeFlowBatchRGB(self, im1, im2, im3, max=None, packed=False, want_flow=False, want_masks=False, out=None):
        """computeFlowBatch with the flow pictures as the output (b2f_compute_flow_batch_rgb): returns (rgb, max_used[, flow]
        [, fwd_occ, bwd_occ]).  rgb is flowX.xy2rgb(flow[1], flow[2], max) of every triplet as bytes, n x 3 x H x W or, with
        packed=True, n x H x W x 3 (what PNG and video encoders take); max=None scales every picture by its own largest flow,
        and max_used (float64, n) is the maximum of each.  want_flow / want_masks append the float32 flow and the masks of
        computeFlowBatch(dtype=np.float32); what is not asked for is not downloaded.  Inputs as for computeFlowBatch;
        out = the returned tuple's buffers (page-locked ones are written by DMA)."""
        return _compute_flow_batch_rgb("b2f_", self._h, im1, im2, im3, max, packed, want_flow, want_masks, out)

    def computeFlowSequenceRGB(self, frames, max=None, packed=False, want_flow=False, want_masks=False, out=None):
        """computeFlowSequence with the flow pictures as the output (b2f_compute_flow_sequence_rgb): one picture per centre
        frame; keywords and results as for computeFlowBatchRGB with n = T - 2."""
        return _compute_flow_sequence_rgb("b2f_", self._h, frames, max, packed, want_flow, want_masks, out)

    def flowRGBDevice(self, d_flow, n, H, W, d_rgb, max=None, packed=False, d_max_used=None, stream=None):
        """b2f_flow_rgb_device on device pointers (ints): the pictures of an n x 2 x H x W float32 flow into d_rgb (n x 3 x H x W
        bytes, or n x H x W x 3 with packed), d_max_used (n float64) optional.  Asynchronous on `stream`: after
        computeFlowDevice on the same stream it needs no synchronisation in between."""
        max_norm = rgb_max_norm(max, "flowRGBDevice")
        if n < 1 or H < 1 or W < 1:
            raise ValueError("flowRGBDevice: bad shape %r" % ((n, H, W),))
        p = lambda v: C.c_void_p(v) if v else None
        _lib.check(_lib.lib().b2f_flow_rgb_device(self._h, p(d_flow), int(n), int(H), int(W), max_norm, RGB_PACKED if packed else RGB_PLANAR,
                                                   p(d_rgb), p(d_max_used), p(stream)))

    def computeFlowBatchScore(self, im1, im2, im3, gt_flow, valid=None, gt_occ=None, flow_scale=20.0, want_flow=False, want_masks=False,
                              out=None):
        """computeFlowBatch scored against ground truth on the GPU (b2f_compute_flow_batch_score; test.lua:183-261): returns the
        records, uint64 n x 22 (score_summary turns them into EPE, Fl and the occlusion accuracies) -- alone, or as
        (scores[, flow][, fwd_occ, bwd_occ]) with want_flow / want_masks, which append the float32 flow and the masks of
        computeFlowBatch(dtype=np.float32); what is not asked for is not downloaded.  gt_flow: float32 n x 2 x H x W in pixels
        (.flo); valid: uint8 n x H x W, nonzero = counted (None: every pixel); gt_occ: uint8 n x H x W, 0 / 1 / 2 = occluded
        "bwd" / visible / occluded "fwd", other bytes unlabelled (None: no split, no occlusion accuracies); flow_scale: pixels per
        unit of raw flow (20 for the shipped models).  The words are ops.flow_score of the float32 flow and occ_prob."""
        return _compute_flow_batch_score("b2f_", self._h, im1, im2, im3, gt_flow, valid, gt_occ, flow_scale, want_flow, want_masks, out)

    def computeFlowSequenceScore(self, frames, gt_flow, valid=None, gt_occ=None, flow_scale=20.0, want_flow=False, want_masks=False, out=None):
        """computeFlowSequence scored against ground truth (b2f_compute_flow_sequence_score): ground truth i belongs to output i,
        the flow of centre frame i + 1; keywords and results as for computeFlowBatchScore with n = T - 2."""
        return _compute_flow_sequence_score("b2f_", self._h, frames, gt_flow, valid, gt_occ, flow_scale, want_flow, want_masks, out)

    def flowScoreDevice(self, d_flow, n, H, W, d_gt_flow, d_scores, d_occ_prob=None, d_valid=None, d_gt_occ=None, flow_scale=20.0, stream=None):
        """b2f_flow_score_device on device pointers (ints): the records (n x 22 uint64 in d_scores) of an n x 2 x H x W float32 flow
        against d_gt_flow (n x 2 x H x W float32), d_valid / d_gt_occ (n x H x W bytes) and d_occ_prob (n x 2 x H x W float32), all
        optional but the first.  Asynchronous on `stream`: after computeFlowDevice on the same stream it needs no synchronisation
        in between."""
        if n < 1 or H < 1 or W < 1:
            raise ValueError("flowScoreDevice: bad shape %r" % ((n, H, W),))
        p = lambda v: C.c_void_p(v) if v else None
        _lib.check(_lib.lib().b2f_flow_score_device(self._h, p(d_flow), p(d_occ_prob), int(n), int(H), int(W), float(flow_scale), p(d_gt_flow),
                                                     p(d_valid), p(d_gt_occ), p(d_scores), p(stream)))

    def computeFlowBatchWarp(self, im1, im2, im3, flow_scale=20.0, want_warped=True, want_photo=True, want_flow=False, want_masks=False,
                             out=None, want_prob=False, own_past_flow=False, want_past=False):
        """computeFlowBatch with motion compensation on the GPU (b2f_compute_flow_batch_warp; models/pwc.lua:67-73,
        criterions/OBCCriterion.lua:79-100): returns (warped, photo[, flow][, fwd_occ, bwd_occ][, occ_prob]) without what is not asked
        for (a single array alone); what is not asked for is not downloaded.  warped: n x 2 x 3 x H x W in the frames' dtype, [:, 0]
        im1 (the past frame) and [:, 1] im3 (the future frame) sampled where the flow says the reference pixels came from / go to --
        not normalized, bytes rounded as image.save does; photo: uint64 n x 14 photometric records (photo_summary turns them into pme,
        PSNR and the inside shares); flow_scale: pixels per unit of raw flow (20 for the shipped models).  The outputs are
        ops.flow_warp of the float32 flow and occ_prob of computeFlowBatch(dtype=np.float32, occ_prob=True).
        own_past_flow=True (Soft models; b2f_compute_flow_batch_warp_past): the past frame is sampled with the model's own past flow
        instead of minus the future flow -- the reference's warped_img_1 and the past half of its pme (pwc.lua:425-432,
        OBCCriterion.lua:80-81) --, i.e. ops.flow_warp(..., past_flow=) of computeFlowBatchPast's outputs; want_past=True then appends
        that past flow to the returned tuple."""
        return _compute_flow_batch_warp("b2f_", self._h, im1, im2, im3, flow_scale, want_warped, want_photo, want_flow, want_masks, out, want_prob,
                                        own_past_flow, want_past)

    def computeFlowSequenceWarp(self, frames, flow_scale=20.0, want_warped=True, want_photo=True, want_flow=False, want_masks=False, out=None,
                                want_prob=False, own_past_flow=False, want_past=False):
        """computeFlowSequence with motion compensation (b2f_compute_flow_sequence_warp): output i belongs to centre frame i + 1, whose
        neighbours are frames i and i + 2; keywords and results as for computeFlowBatchWarp with n = T - 2."""
        return _compute_flow_sequence_warp("b2f_", self._h, frames, flow_scale, want_warped, want_photo, want_flow, want_masks, out, want_prob,
                                           own_past_flow, want_past)

    def flowWarpDevice(self, d_flow, n, H, W, d_im1, d_im2, d_im3, d_warped=None, d_photo=None, d_occ_prob=None, flow_scale=20.0, as_bytes=False,
                       stream=None, own_past_flow=False, d_past_flow=None):
        """b2f_flow_warp_device on device pointers (ints): the warped neighbours (n x 2 x 3 x H x W in d_warped, bytes with as_bytes,
        float32 otherwise, like the frames d_im1 / d_im2 / d_im3, n x 3 x H x W each) and / or the photometric records (n x 14 uint64
        in d_photo) of an n x 2 x H x W float32 flow and, optionally, d_occ_prob.  Asynchronous on `stream`: after computeFlowDevice
        on the same stream it needs no synchronisation in between.  own_past_flow=True (b2f_flow_warp_past_device): the past frame
        follows d_past_flow (n x 2 x H x W float32, e.g. computeFlowDevicePast's) instead of d_flow."""
        if n < 1 or H < 1 or W < 1:
            raise ValueError("flowWarpDevice: bad shape %r" % ((n, H, W),))
        if bool(own_past_flow) != bool(d_past_flow):
            raise ValueError("flowWarpDevice: own_past_flow=True and d_past_flow go together")
        p = lambda v: C.c_void_p(v) if v else None
        if own_past_flow:
            _lib.check(_lib.lib().b2f_flow_warp_past_device(self._h, p(d_flow), p(d_past_flow), p(d_occ_prob), int(n), int(H), int(W),
                                                             float(flow_scale), IN_U8 if as_bytes else IN_UNIT, p(d_im1), p(d_im2), p(d_im3),
                                                             p(d_warped), p(d_photo), p(stream)))
            return
        _lib.check(_lib.lib().b2f_flow_warp_device(self._h, p(d_flow), p(d_occ_prob), int(n), int(H), int(W), float(flow_scale),
                                                    IN_U8 if as_bytes else IN_UNIT, p(d_im1), p(d_im2), p(d_im3), p(d_warped), p(d_photo), p(stream)))

    def output_shapes(self, H, W):
        cap = 32
        ch, oh, ow = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
        _lib.check(_lib.lib().b2f_output_shapes(self._h, H, W, ch, oh, ow, cap))
        return [(ch[i], oh[i], ow[i]) for i in range(self.n_outputs)]

    def forward(self, x):
        """model:forward(imgs) (back2future.lua:74): x is B x 9 x H x W, already normalized;
        returns the whole output table of pwc.lua:459-489 as a list of B x C x h x w arrays."""
        x = _lib.f32(x)
        B, nine, H, W = x.shape
        assert nine == 9
        outs = [np.empty((B, c, h, w), np.float32) for (c, h, w) in self.output_shapes(H, W)]
        ptrs = (_lib.c_float_p * len(outs))(*[_lib.fptr(o) for o in outs])
        _lib.check(_lib.lib().b2f_forward(self._h, _lib.fptr(x), B, H, W, ptrs, len(outs)))
        return outs

    def forwardLoss(self, x, flow_scale=20.0, want_table=False, objective="pme", ssim_range="batch", gt_flow=None, valid=None, gt_occ=None,
                    options=None):
        """model:forward followed by the unsupervised validation loss of test.lua:266-297 (b2f_forward_loss): x n x 9 x H x W,
        already normalized -> uint64 records (n, L, 16), those of ops.table_loss(self.forward(x), x[:, 3:6]); the table stays on the
        GPU.  want_table=True returns (records, table) with the table of Model.forward, bit for bit.  loss_summary reads the
        records.  objective="finetune" (b2f_forward_loss_ft): records (n, L, 24), those of ops.table_loss(..., objective="finetune").
        objective="ssim" (b2f_forward_loss_ssim): records (n, L, 32) with the SSIM + L1 sums of OSSIML1Criterion.lua; ssim_range as for
        ops.table_loss: "batch" is refused when the request is cut into sub-batches, "image" and an L x 2 array do not depend on the cut.
        objective="plain" (b2f_forward_loss_plain): records (n, L, 40) with the sums of the photometric terms that do not mask occlusions
        (MBCCriterion.lua, MSSIML1Criterion.lua); ssim_range likewise.  The other loss and gradient methods of Model and MultiModel take
        objective="plain", resp. the options of loss_grad_plain_options, in the same way as "ssim" and loss_grad_ssim_options.
        objective="epe" (b2f_forward_loss_epe; train.lua:296-334): records (n, L, 8), those of ops.table_loss_epe(self.forward(x), gt_flow,
        valid, gt_occ, options=options); the ground truth of a sub-batch is uploaded with its frames."""
        words = loss_words(objective)
        L = self.n_outputs // (5 if self.past_flow else 4)
        if objective == "epe":
            loss, _, outs = _forward_loss_epe(_lib.lib().b2f_forward_loss_epe, self._h, "forwardLoss", x, gt_flow, valid, gt_occ, flow_scale, options,
                                              "batch", self.output_shapes, L, True, False, want_table)
            return (loss, outs) if want_table else loss
        base, tail = loss_entry("b2f_forward_loss%s", objective), ssim_range_args(objective, ssim_range, L, "forwardLoss")
        entry = lambda *a: base(*(a + tail))
        if want_table:
            return _forward_loss(entry, self._h, x, flow_scale, L, self.output_shapes, words)
        fn = lambda h, xp, n, H, W, fsc, lp: entry(h, xp, n, H, W, fsc, lp, None, 0)
        return _forward_loss(fn, self._h, x, flow_scale, L, None, words)[0]

    def _forward_loss_epe_device(self, who, d_in, n, H, W, d_loss, d_grad, flow_scale, stream, gt_flow, valid, gt_occ, count, options):
        """b2f_forward_loss_epe_device: gt_flow (n x 2 x H x W float32), valid and gt_occ (n x H x W uint8, or None) are device pointers"""
        if not gt_flow:
            raise ValueError(who + ": objective='epe' needs gt_flow, a device pointer to n x 2 x H x W float32")
        gptrs = (C.c_void_p * len(d_grad))(*[C.c_void_p(int(p)) for p in d_grad]) if d_grad is not None else None
        mode, counts = epe_count_args(count, self.n_outputs // (5 if self.past_flow else 4), who)
        p = lambda v: C.c_void_p(int(v)) if v else None
        _lib.check(_lib.lib().b2f_forward_loss_epe_device(self._h, p(d_in), IN_NORMALIZED, int(n), int(H), int(W), p(gt_flow), p(valid), p(gt_occ),
                                                          float(flow_scale), _epe_opts_ptr(options), mode, counts, p(d_loss), gptrs,
                                                          len(d_grad) if d_grad is not None else 0, p(stream)))

    def forwardLossDevice(self, d_in, n, H, W, d_loss, flow_scale=20.0, stream=None, objective="pme", ssim_range="batch", gt_flow=None, valid=None,
                          gt_occ=None, options=None):
        """b2f_forward_loss_device on device pointers (ints): d_in n x 9 x H x W normalized float32, d_loss n x L x 16 uint64 (test.lua:266-297);
        asynchronous on `stream`.  objective="finetune" (b2f_forward_loss_ft_device): d_loss n x L x 24; objective="ssim"
        (b2f_forward_loss_ssim_device): d_loss n x L x 32, ssim_range as for forwardLoss.  objective="epe" (b2f_forward_loss_epe_device): d_loss
        n x L x 8, gt_flow / valid / gt_occ device pointers, options of loss_epe_options."""
        if objective == "epe":
            return self._forward_loss_epe_device("forwardLossDevice", d_in, n, H, W, d_loss, None, flow_scale, stream, gt_flow, valid, gt_occ, "batch", options)
        entry = loss_entry("b2f_forward_loss%s_device", objective)
        tail = ssim_range_args(objective, ssim_range, self.n_outputs // (5 if self.past_flow else 4), "forwardLossDevice")
        _lib.check(entry(self._h, C.c_void_p(d_in), IN_NORMALIZED, int(n), int(H), int(W), float(flow_scale), C.c_void_p(d_loss),
                         C.c_void_p(stream) if stream else None, *tail))

    def _table_loss_epe_device(self, who, d_table, n, H, W, d_loss, d_grad, flow_scale, stream, gt_flow, valid, gt_occ, count, options):
        """b2f_table_loss_epe_device: gt_flow (n x 2 x H x W float32), valid and gt_occ (n x H x W uint8, or None) are device pointers"""
        if not gt_flow:
            raise ValueError(who + ": objective='epe' needs gt_flow, a device pointer to n x 2 x H x W float32")
        if d_grad is not None and len(d_grad) != len(d_table):
            raise ValueError(who + ": the gradient table must have the table's %d tensors" % len(d_table))
        ptrs = (C.c_void_p * len(d_table))(*[C.c_void_p(int(p)) for p in d_table])
        gptrs = (C.c_void_p * len(d_grad))(*[C.c_void_p(int(p)) for p in d_grad]) if d_grad is not None else None
        mode, counts = epe_count_args(count, len(d_table) // (5 if self.past_flow else 4), who)
        p = lambda v: C.c_void_p(int(v)) if v else None
        _lib.check(_lib.lib().b2f_table_loss_epe_device(self._h, ptrs, len(d_table), int(n), int(H), int(W), p(gt_flow), p(valid), p(gt_occ),
                                                        float(flow_scale), _epe_opts_ptr(options), mode, counts, p(d_loss), gptrs, p(stream)))

    def tableLossDevice(self, d_table, n, H, W, d_ref, d_loss, flow_scale=20.0, stream=None, objective="pme", ssim_range="batch", gt_flow=None,
                        valid=None, gt_occ=None, count="batch", options=None):
        """b2f_table_loss_device on device pointers (ints): d_table the L x 4 | 5 tensors of an output table in table order, d_ref
        n x 3 x H x W, d_loss n x L x 16 uint64 (test.lua:266-297); asynchronous on `stream`.  objective="finetune"
        (b2f_table_loss_ft_device): d_loss n x L x 24; objective="ssim" (b2f_table_loss_ssim_device): d_loss n x L x 32, ssim_range
        "batch" (over the call's n images), "image" or an L x 2 array.  objective="epe" (b2f_table_loss_epe_device; train.lua:296-334):
        d_loss n x L x 8, d_ref is not read (None), gt_flow / valid / gt_occ device pointers as for flowScoreDevice, options of
        loss_epe_options; count is read by the gradient only."""
        if objective == "epe":
            return self._table_loss_epe_device("tableLossDevice", d_table, n, H, W, d_loss, None, flow_scale, stream, gt_flow, valid, gt_occ, count, options)
        ptrs = (C.c_void_p * len(d_table))(*[C.c_void_p(int(p)) for p in d_table])
        entry = loss_entry("b2f_table_loss%s_device", objective)
        tail = ssim_range_args(objective, ssim_range, len(d_table) // (5 if self.past_flow else 4), "tableLossDevice")
        _lib.check(entry(self._h, ptrs, len(d_table), int(n), int(H), int(W), C.c_void_p(d_ref), float(flow_scale), C.c_void_p(d_loss),
                         C.c_void_p(stream) if stream else None, *tail))

    def forwardLossGrad(self, x, flow_scale=20.0, options=None, want_loss=True, want_table=False, ssim_range="batch", objective=None, gt_flow=None,
                        valid=None, gt_occ=None, count="batch"):
        """model:forward followed by `gradOutputs` of train.lua:428-468 (b2f_forward_loss_grad): x n x 9 x H x W, already normalized ->
        the gradient of the pme objective with respect to every tensor of the output table, a list with the shapes of
        Model.forward's, that of ops.table_loss_grad(self.forward(x), x[:, 3:6]); the table stays on the GPU.  options: of
        loss_grad_options (None: the defaults) or of loss_grad_ft_options (b2f_forward_loss_grad_ft: the fine-tuning objectives of the
        Soft models).  want_loss=True returns (gradient, records) with the records of forwardLoss (of forwardLoss(objective="finetune")
        with loss_grad_ft_options), from the same pass; want_table=True appends the table of Model.forward, bit for bit.  With the options
        of loss_grad_ssim_options: b2f_forward_loss_grad_ssim, the records of forwardLoss(objective="ssim"), ssim_range as there.
        objective="epe" (b2f_forward_loss_epe; train.lua:296-334): options of loss_epe_options, gt_flow / valid / gt_occ as for
        ops.table_loss_epe, whose gradient and records of self.forward(x) these are; count "batch" takes the counts of sizeAverage over the
        whole request before its first sub-batch, so a cut changes nothing."""
        L = self.n_outputs // (5 if self.past_flow else 4)
        if objective == "epe":
            loss, grad, outs = _forward_loss_epe(_lib.lib().b2f_forward_loss_epe, self._h, "forwardLossGrad", x, gt_flow, valid, gt_occ, flow_scale,
                                                 options, count, self.output_shapes, L, want_loss, True, want_table)
            if not want_loss and not want_table:
                return grad
            return (grad,) + ((loss,) if want_loss else ()) + ((outs,) if want_table else ())
        if objective is not None:
            raise ValueError("forwardLossGrad: objective is 'epe' or None (the options name every other objective)")
        grad, loss, outs = _forward_loss_grad(_grad_entry("b2f_forward_loss_grad", options), self._h, x, flow_scale, options, self.output_shapes, L,
                                              want_loss, want_table, _grad_range_args(options, ssim_range, L, "forwardLossGrad"))
        if not want_loss and not want_table:
            return grad
        return (grad,) + ((loss,) if want_loss else ()) + ((outs,) if want_table else ())

    def forwardLossGradDevice(self, d_in, n, H, W, d_grad, d_loss=None, flow_scale=20.0, options=None, stream=None, ssim_range="batch", objective=None,
                              gt_flow=None, valid=None, gt_occ=None, count="batch"):
        """b2f_forward_loss_grad_device on device pointers (ints): d_in n x 9 x H x W normalized float32, d_grad the n_outputs tensors
        of the gradient table (train.lua:428-468), d_loss n x L x 16 uint64 or None; asynchronous on `stream`.  With the options of
        loss_grad_ft_options: b2f_forward_loss_grad_ft_device, d_loss n x L x 24; of loss_grad_ssim_options:
        b2f_forward_loss_grad_ssim_device, d_loss n x L x 32, ssim_range as for forwardLoss.  objective="epe"
        (b2f_forward_loss_epe_device): options of loss_epe_options, gt_flow / valid / gt_occ device pointers, d_loss n x L x 8; with
        size_average, count "batch" is refused when the request would be cut into sub-batches."""
        if objective == "epe":
            return self._forward_loss_epe_device("forwardLossGradDevice", d_in, n, H, W, d_loss, d_grad, flow_scale, stream, gt_flow, valid, gt_occ, count,
                                                 options)
        if objective is not None:
            raise ValueError("forwardLossGradDevice: objective is 'epe' or None (the options name every other objective)")
        ptrs = (C.c_void_p * len(d_grad))(*[C.c_void_p(int(p)) for p in d_grad])
        tail = _grad_range_args(options, ssim_range, self.n_outputs // (5 if self.past_flow else 4), "forwardLossGradDevice")
        _lib.check(_grad_entry("b2f_forward_loss_grad_device", options)(self._h, C.c_void_p(d_in), IN_NORMALIZED, int(n), int(H), int(W), float(flow_scale),
                                                            _grad_opts_ptr(options), C.c_void_p(d_loss) if d_loss else None, ptrs, len(d_grad),
                                                            C.c_void_p(stream) if stream else None, *tail))

    def tableLossGradDevice(self, d_table, n, H, W, d_ref, d_grad, flow_scale=20.0, options=None, stream=None, ssim_range="batch", objective=None,
                            gt_flow=None, valid=None, gt_occ=None, count="batch", d_loss=None):
        """b2f_table_loss_grad_device on device pointers (ints): d_table the L x 4 | 5 tensors of an output table in table order, d_ref
        n x 3 x H x W, d_grad as many tensors of the same shapes (train.lua:428-468); asynchronous on `stream`.  With the options of
        loss_grad_ft_options: b2f_table_loss_grad_ft_device; of loss_grad_ssim_options: b2f_table_loss_grad_ssim_device, ssim_range as for
        tableLossDevice.  objective="epe" (b2f_table_loss_epe_device; train.lua:296-334): options of loss_epe_options, d_ref is not read
        (None), gt_flow / valid / gt_occ device pointers, count "batch" (N_j over the call's images), "image" or an L x 2 array, d_loss
        (n x L x 8 uint64) or None for the records of the same launches."""
        if objective == "epe":
            return self._table_loss_epe_device("tableLossGradDevice", d_table, n, H, W, d_loss, d_grad, flow_scale, stream, gt_flow, valid, gt_occ, count, options)
        if objective is not None:
            raise ValueError("tableLossGradDevice: objective is 'epe' or None (the options name every other objective)")
        ptrs = (C.c_void_p * len(d_table))(*[C.c_void_p(int(p)) for p in d_table])
        gptrs = (C.c_void_p * len(d_grad))(*[C.c_void_p(int(p)) for p in d_grad])
        if len(d_grad) != len(d_table):
            raise ValueError("tableLossGradDevice: the gradient table must have the table's %d tensors" % len(d_table))
        tail = _grad_range_args(options, ssim_range, len(d_table) // (5 if self.past_flow else 4), "tableLossGradDevice")
        _lib.check(_grad_entry("b2f_table_loss_grad_device", options)(self._h, ptrs, len(d_table), int(n), int(H), int(W), C.c_void_p(d_ref), float(flow_scale),
                                                          _grad_opts_ptr(options), gptrs, C.c_void_p(stream) if stream else None, *tail))

    def forward_device(self, d_in, B, H, W, d_flow=None, d_occ=None, d_est3=None, unit_input=False, stream=None, d_past_flow=None):
        """model:forward on device pointers (ints); asynchronous on `stream`.  d_past_flow (B x 2 x H x W float32, Soft models;
        b2f_forward_device_past): the network's past flow skip_ubfs[3]; the pruned pass then runs the past-flow decoders too."""
        if d_past_flow:
            _lib.check(_lib.lib().b2f_forward_device_past(
                self._h, C.c_void_p(d_in), 1 if unit_input else 0, B, H, W,
                C.c_void_p(d_flow) if d_flow else None, C.c_void_p(d_past_flow), C.c_void_p(d_occ) if d_occ else None,
                C.c_void_p(d_est3) if d_est3 else None, C.c_void_p(stream) if stream else None))
            return
        _lib.check(_lib.lib().b2f_forward_device(
            self._h, C.c_void_p(d_in), 1 if unit_input else 0, B, H, W,
            C.c_void_p(d_flow) if d_flow else None, C.c_void_p(d_occ) if d_occ else None,
            C.c_void_p(d_est3) if d_est3 else None, C.c_void_p(stream) if stream else None))

    def forward_sequence_device(self, d_frames, T, H, W, d_flow=None, d_occ=None, d_est3=None, in_kind=IN_NORMALIZED, stream=None,
                                d_past_flow=None):
        """b2f_forward_sequence_device on device pointers (ints): d_frames is T x 3 x H x W (float32, or uint8 with
        in_kind=IN_U8); outputs (T-2) x 2|2|C3 x H x W, output i that of the triplet (i, i+1, i+2).  Asynchronous on `stream`."""
        if T < 3:
            raise ValueError("forward_sequence_device: a sequence needs T >= 3 frames, got %d" % T)
        if d_past_flow:   # b2f_forward_sequence_device_past: (T-2) x 2 x H x W, the past flow of every triplet (Soft models)
            _lib.check(_lib.lib().b2f_forward_sequence_device_past(
                self._h, C.c_void_p(d_frames), int(in_kind), T, H, W,
                C.c_void_p(d_flow) if d_flow else None, C.c_void_p(d_past_flow), C.c_void_p(d_occ) if d_occ else None,
                C.c_void_p(d_est3) if d_est3 else None, C.c_void_p(stream) if stream else None))
            return
        _lib.check(_lib.lib().b2f_forward_sequence_device(
            self._h, C.c_void_p(d_frames), int(in_kind), T, H, W,
            C.c_void_p(d_flow) if d_flow else None, C.c_void_p(d_occ) if d_occ else None,
            C.c_void_p(d_est3) if d_est3 else None, C.c_void_p(stream) if stream else None))


class MultiModel(object):
    """One process, several GPUs (b2f_init_multi): replaces nn.DataParallelTable of util.lua:27-48 for inference.  The
    weights are loaded once and broadcast to every GPU's replica (RCCL / peer copy) inside the library; computeFlowBatch
    splits the triplets contiguously over the GPUs."""

    TRANSPORT = {0: "single GPU", 1: "RCCL broadcast", 2: "hipMemcpyPeer"}

    def __init__(self, name="Ours-Soft-ft-KITTI", n_gpus=0, devices=None):
        L = _lib.lib()
        h = C.c_void_p()
        dv = (C.c_int * len(devices))(*devices) if devices is not None else None
        _lib.check(L.b2f_init_multi(name.encode() if name is not None else None, int(n_gpus), dv, C.byref(h)))
        self._h = h
        n, tr = C.c_int(), C.c_int()
        devs = (C.c_int * 64)()
        _lib.check(L.b2f_multi_info(h, C.byref(n), devs, 64, C.byref(tr)))
        self.n_gpus, self.devices, self.transport = n.value, [devs[i] for i in range(n.value)], self.TRANSPORT[tr.value]

    def close(self):
        if getattr(self, "_h", None):
            if _lib is not None:
                _lib.lib().b2f_destroy_multi(self._h)
            self._h = None

    __del__ = close

    def weights_checksums(self):
        sums = (C.c_ulonglong * self.n_gpus)()
        _lib.check(_lib.lib().b2f_multi_weights_checksum(self._h, sums, self.n_gpus))
        return [int(v) for v in sums]

    def set_option(self, key, value):
        for i in range(self.n_gpus):
            _lib.check(_lib.lib().b2f_set_option(C.c_void_p(_lib.lib().b2f_multi_context(self._h, i)), key.encode(), int(value)))

    def computeFlowBatch(self, im1, im2, im3, out=None, dtype=np.float64, occ_prob=False):
        """Model.computeFlowBatch over the GPUs, with the same keywords."""
        return _compute_flow_batch("b2f_multi_", self._h, im1, im2, im3, out, dtype, occ_prob)

    def computeFlowSequence(self, frames, out=None, dtype=np.float64, occ_prob=False):
        """Model.computeFlowSequence over the GPUs: the T-2 triplets are split with shard_range, every replica reads the
        frames its triplets need (T_i = its triplets + 2).  dtype / occ_prob / out as for Model.computeFlowSequence."""
        return _compute_flow_sequence("b2f_multi_", self._h, frames, out, dtype, occ_prob)

    def computeFlowBatchPast(self, im1, im2, im3, out=None, occ_prob=False):
        """Model.computeFlowBatchPast over the GPUs, with the same keywords and the same bits."""
        return _compute_flow_batch_past("b2f_multi_", self._h, im1, im2, im3, out, occ_prob)

    def computeFlowSequencePast(self, frames, out=None, occ_prob=False):
        """Model.computeFlowSequencePast over the GPUs, with the same keywords and the same bits."""
        return _compute_flow_sequence_past("b2f_multi_", self._h, frames, out, occ_prob)

    def computeFlowBatchRGB(self, im1, im2, im3, max=None, packed=False, want_flow=False, want_masks=False, out=None):
        """Model.computeFlowBatchRGB over the GPUs, with the same keywords and the same bytes."""
        return _compute_flow_batch_rgb("b2f_multi_", self._h, im1, im2, im3, max, packed, want_flow, want_masks, out)

    def computeFlowSequenceRGB(self, frames, max=None, packed=False, want_flow=False, want_masks=False, out=None):
        """Model.computeFlowSequenceRGB over the GPUs, with the same keywords and the same bytes."""
        return _compute_flow_sequence_rgb("b2f_multi_", self._h, frames, max, packed, want_flow, want_masks, out)


    def computeFlowBatchScore(self, im1, im2, im3, gt_flow, valid=None, gt_occ=None, flow_scale=20.0, want_flow=False, want_masks=False,
                              out=None):
        """Model.computeFlowBatchScore over the GPUs, with the same keywords and the same words."""
        return _compute_flow_batch_score("b2f_multi_", self._h, im1, im2, im3, gt_flow, valid, gt_occ, flow_scale, want_flow, want_masks, out)

    def computeFlowSequenceScore(self, frames, gt_flow, valid=None, gt_occ=None, flow_scale=20.0, want_flow=False, want_masks=False, out=None):
        """Model.computeFlowSequenceScore over the GPUs, with the same keywords and the same words."""
        return _compute_flow_sequence_score("b2f_multi_", self._h, frames, gt_flow, valid, gt_occ, flow_scale, want_flow, want_masks, out)


    def computeFlowBatchWarp(self, im1, im2, im3, flow_scale=20.0, want_warped=True, want_photo=True, want_flow=False, want_masks=False,
                             out=None, want_prob=False, own_past_flow=False, want_past=False):
        """Model.computeFlowBatchWarp over the GPUs, with the same keywords, the same bytes and the same words."""
        return _compute_flow_batch_warp("b2f_multi_", self._h, im1, im2, im3, flow_scale, want_warped, want_photo, want_flow, want_masks, out,
                                        want_prob, own_past_flow, want_past)

    def computeFlowSequenceWarp(self, frames, flow_scale=20.0, want_warped=True, want_photo=True, want_flow=False, want_masks=False, out=None,
                                want_prob=False, own_past_flow=False, want_past=False):
        """Model.computeFlowSequenceWarp over the GPUs, with the same keywords, the same bytes and the same words."""
        return _compute_flow_sequence_warp("b2f_multi_", self._h, frames, flow_scale, want_warped, want_photo, want_flow, want_masks, out,
                                           want_prob, own_past_flow, want_past)

    def _shapes_and_levels(self):
        """(output_shapes(H, W), L) of the replicas' model"""
        c0 = C.c_void_p(_lib.lib().b2f_multi_context(self._h, 0))
        lv, win, pf, no, npar = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        _lib.check(_lib.lib().b2f_info(c0, C.byref(lv), C.byref(win), C.byref(pf), C.byref(no), C.byref(npar)))

        def shapes(H, W):
            ch, oh, ow = (C.c_int * 64)(), (C.c_int * 64)(), (C.c_int * 64)()
            _lib.check(_lib.lib().b2f_output_shapes(c0, H, W, ch, oh, ow, 64))
            return [(ch[i], oh[i], ow[i]) for i in range(no.value)]

        return shapes, no.value // (5 if pf.value else 4)

    def forwardLoss(self, x, flow_scale=20.0, objective="pme", ssim_range="image", gt_flow=None, valid=None, gt_occ=None, options=None):
        """Model.forwardLoss over the GPUs (b2f_multi_forward_loss / b2f_multi_forward_loss_ft / b2f_multi_forward_loss_ssim;
        test.lua:266-297): the same words.  objective="ssim" takes ssim_range="image" or an L x 2 array: the batch's range would depend
        on how the images are split over the GPUs.  objective="epe" (b2f_multi_forward_loss_epe): gt_flow / valid / gt_occ / options as
        for Model.forwardLoss; the ground truth is split with the triplets."""
        words = loss_words(objective)
        if objective == "epe":
            shapes, L = self._shapes_and_levels()
            return _forward_loss_epe(_lib.lib().b2f_multi_forward_loss_epe, self._h, "MultiModel.forwardLoss", x, gt_flow, valid, gt_occ, flow_scale,
                                     options, "image", shapes, L, True, False, False, multi=True)[0]
        c0 = C.c_void_p(_lib.lib().b2f_multi_context(self._h, 0))
        lv, win, pf, no, npar = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        _lib.check(_lib.lib().b2f_info(c0, C.byref(lv), C.byref(win), C.byref(pf), C.byref(no), C.byref(npar)))
        L = no.value // (5 if pf.value else 4)
        base = loss_entry("b2f_multi_forward_loss%s", objective)
        tail = ssim_range_args(objective, ssim_range, L, "MultiModel.forwardLoss", batch_ok=False)
        return _forward_loss(lambda *a: base(*(a + tail)), self._h, x, flow_scale, L, None, words)[0]

    def forwardLossGrad(self, x, flow_scale=20.0, options=None, want_loss=True, ssim_range="image", objective=None, gt_flow=None, valid=None,
                        gt_occ=None, count="image"):
        """Model.forwardLossGrad over the GPUs (b2f_multi_forward_loss_grad, b2f_multi_forward_loss_grad_ft,
        b2f_multi_forward_loss_grad_ssim; train.lua:428-468): the same bits.  With loss_grad_ssim_options ssim_range is "image" or an
        L x 2 array, as for MultiModel.forwardLoss.  objective="epe" (b2f_multi_forward_loss_epe): as Model.forwardLossGrad, with count
        "image" (the default here) or an L x 2 array: the batch's counts would depend on how the images are split over the GPUs."""
        if objective == "epe":
            shapes, L = self._shapes_and_levels()
            loss, grad, _ = _forward_loss_epe(_lib.lib().b2f_multi_forward_loss_epe, self._h, "MultiModel.forwardLossGrad", x, gt_flow, valid, gt_occ,
                                              flow_scale, options, count, shapes, L, want_loss, True, False, multi=True)
            return (grad, loss) if want_loss else grad
        if objective is not None:
            raise ValueError("MultiModel.forwardLossGrad: objective is 'epe' or None (the options name every other objective)")
        c0 = C.c_void_p(_lib.lib().b2f_multi_context(self._h, 0))
        lv, win, pf, no, npar = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        _lib.check(_lib.lib().b2f_info(c0, C.byref(lv), C.byref(win), C.byref(pf), C.byref(no), C.byref(npar)))

        def shapes(H, W):
            ch, oh, ow = (C.c_int * 64)(), (C.c_int * 64)(), (C.c_int * 64)()
            _lib.check(_lib.lib().b2f_output_shapes(c0, H, W, ch, oh, ow, 64))
            return [(ch[i], oh[i], ow[i]) for i in range(no.value)]

        entry = _grad_entry("b2f_multi_forward_loss_grad", options)
        fn = lambda h, xp, n, H, W, fsc, op, lp, gp, ng, outs, *tail: entry(h, xp, n, H, W, fsc, op, lp, gp, ng, *tail)
        L = no.value // (5 if pf.value else 4)
        grad, loss, _ = _forward_loss_grad(fn, self._h, x, flow_scale, options, shapes, L, want_loss, False,
                                           _grad_range_args(options, ssim_range, L, "MultiModel.forwardLossGrad", batch_ok=False))
        return (grad, loss) if want_loss else grad


ARENA_BUFFERS = (["img", "tmp"] + ["cs[%d]" % l for l in range(2, 8)] + ["U[%d]" % l for l in range(3, 7)] + ["UB[%d]" % l for l in range(3, 7)]
                 + ["cv"] + ["d[%d]" % i for i in range(1, 6)] + ["fs", "bfs", "logits", "u2", "flow_planar"] + ["ds[%d]" % k for k in range(2, 6)])


def arena_plan(B, H, W, full=False, past_flow=False, seq=False, stream=False, want_past=False, arena_guard=0):
    """b2f_arena_plan (host only): ({buffer name: float offset}, total floats) of the workspace of such a pass."""
    off, total = (C.c_longlong * 40)(), C.c_longlong()
    flags = (1 if full else 0) | (2 if past_flow else 0) | (4 if seq else 0) | (8 if stream else 0) | (16 if want_past else 0)
    n = _lib.lib().b2f_arena_plan(int(arena_guard), int(B), int(H), int(W), flags, off, 40, C.byref(total))
    if n < 0:
        _lib.check(1)
    assert n == len(ARENA_BUFFERS)
    return dict(zip(ARENA_BUFFERS, list(off)[:n])), total.value


def shard_range(n, rank, world):
    """b2f_shard_range: [lo, hi) of `rank` when n triplets are split over `world` GPUs (util.lua:32)."""
    lo, hi = C.c_int(), C.c_int()
    _lib.check(_lib.lib().b2f_shard_range(int(n), int(rank), int(world), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def init(opt=None, device=0):
    """back2future.init(opt) (back2future.lua:97-129): returns the computeFlow closure.
    The closure carries the model as `.model`."""
    opt = opt or "Ours-Soft-ft-KITTI"
    model = Model(opt, device)

    def computeFlow(im1, im2, im3):
        return model.computeFlow(im1, im2, im3)

    computeFlow.model = model
    return computeFlow
