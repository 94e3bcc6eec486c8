"""Op-level calls through the C ABI, in the layouts of the reference modules
(nn.CostVolMulti, nn.BilinearSamplerBHWD, nn.SpatialConvolution, ...).  Used by the parity
tests; every call runs the HIP kernels of libb2f.so."""
import ctypes as C

import numpy as np

from . import _lib, weights


def _h(model):
    return model._h


def costvol(model, ref, frm, win=9, fwd=True):
    ref, frm = _lib.f32(ref), _lib.f32(frm)
    B, Cc, h, w = ref.shape
    out = np.empty((B, win * win, h, w), np.float32)
    _lib.check(_lib.lib().b2f_op_costvol(_h(model), _lib.fptr(ref), _lib.fptr(frm), B, Cc, h, w, win, int(bool(fwd)),
                                         _lib.fptr(out)))
    return out


def warp_bhwd(model, img, grid):
    img, grid = _lib.f32(img), _lib.f32(grid)
    B, ih, iw, Cc = img.shape
    _, gh, gw, _two = grid.shape
    out = np.empty((B, gh, gw, Cc), np.float32)
    _lib.check(_lib.lib().b2f_op_warp_bhwd(_h(model), _lib.fptr(img), _lib.fptr(grid), B, ih, iw, Cc, gh, gw,
                                           _lib.fptr(out)))
    return out


def warp_costvol(model, ref, nbr_future, nbr_past, flow, k):
    ref, nf, npast = _lib.f32(ref), _lib.f32(nbr_future), _lib.f32(nbr_past)
    B, Cc, h, w = ref.shape
    fl = _lib.f32(flow) if flow is not None else None
    out = np.empty((B, 162, h, w), np.float32)
    _lib.check(_lib.lib().b2f_op_warp_costvol(_h(model), _lib.fptr(ref), _lib.fptr(nf), _lib.fptr(npast),
                                              _lib.fptr(fl) if fl is not None else None, float(k), B, Cc, h, w,
                                              _lib.fptr(out)))
    return out


def conv3x3(model, x, w, b, stride=1, leaky=False):
    x, w, b = _lib.f32(x), _lib.f32(w), _lib.f32(b)
    B, ci, H, W = x.shape
    co = w.shape[0]
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    y = np.empty((B, co, Ho, Wo), np.float32)
    _lib.check(_lib.lib().b2f_op_conv3x3(_h(model), _lib.fptr(x), B, ci, H, W, _lib.fptr(w), _lib.fptr(b), co, stride,
                                         int(bool(leaky)), _lib.fptr(y)))
    return y


def conv3x3_backward(model, x, w, grad_y, y=None, leaky=False, layout=0, want=("x", "w", "b"), stride=1):
    """nn.SpatialConvolution(Ci, Co, 3, 3, 1, 1, 1, 1) [+ LeakyReLU(0.2)] :backward.  x: B x Ci x H x W, w: Co x Ci x 3 x 3, grad_y and
    y (the layer's output, needed with leaky): B x Co x H x W.  layout 0: NHWC strides on the device, 1: the forward's chunk-planar ones.
    Returns {"x": grad_x, "w": grad_w, "b": grad_b} with the keys of `want`; only those are computed.  stride 2 is refused."""
    x, w, grad_y = _lib.f32(x), _lib.f32(w), _lib.f32(grad_y)
    y = _lib.f32(y) if y is not None else None
    B, ci, H, W = x.shape
    co = w.shape[0]
    if w.shape != (co, ci, 3, 3) or grad_y.shape != (B, co, H, W) or (y is not None and y.shape != grad_y.shape):
        raise ValueError("ops.conv3x3_backward: shapes %s, %s, %s do not belong to one stride-1 layer" % (x.shape, w.shape, grad_y.shape))
    out = {}
    if "x" in want:
        out["x"] = np.empty_like(x)
    if "w" in want:
        out["w"] = np.empty_like(w)
    if "b" in want:
        out["b"] = np.empty(co, np.float32)
    ptr = lambda k: _lib.fptr(out[k]) if k in out else None
    _lib.check(_lib.lib().b2f_op_conv3x3_backward(_h(model), _lib.fptr(x), B, ci, H, W, _lib.fptr(w), co, int(stride), int(bool(leaky)),
                                                  _lib.fptr(y) if y is not None else None, _lib.fptr(grad_y), int(layout), ptr("x"), ptr("w"),
                                                  ptr("b")))
    return out


def conv3x3_backward_plan(model, B, ci, H, W, co):
    """(partials, longest chain) of conv3x3_backward's gradWeight / gradBias at these sizes under the model's options: how many partial
    sums the pixels are cut into, and the most pixels one of them adds up.  Launches nothing."""
    partials, chain = C.c_int(0), C.c_longlong(0)
    _lib.check(_lib.lib().b2f_op_conv3x3_backward_plan(_h(model), int(B), int(ci), int(H), int(W), int(co), C.byref(partials), C.byref(chain)))
    return partials.value, chain.value


def conv3x3s2_backward(model, x, w, grad_y, y=None, leaky=False, layout=0, want=("x", "w", "b")):
    """nn.SpatialConvolution(Ci, Co, 3, 3, 2, 2, 1, 1) [+ LeakyReLU(0.2)] :backward.  x: B x Ci x H x W, w: Co x Ci x 3 x 3, grad_y and
    y (the layer's output, needed with leaky): B x Co x Ho x Wo with Ho = (H - 1) // 2 + 1, Wo = (W - 1) // 2 + 1.  layout and the returned
    dict as conv3x3_backward."""
    x, w, grad_y = _lib.f32(x), _lib.f32(w), _lib.f32(grad_y)
    y = _lib.f32(y) if y is not None else None
    B, ci, H, W = x.shape
    co = w.shape[0]
    if w.shape != (co, ci, 3, 3) or grad_y.shape != (B, co, (H - 1) // 2 + 1, (W - 1) // 2 + 1) or (y is not None and y.shape != grad_y.shape):
        raise ValueError("ops.conv3x3s2_backward: shapes %s, %s, %s do not belong to one stride-2 layer" % (x.shape, w.shape, grad_y.shape))
    out = {}
    if "x" in want:
        out["x"] = np.empty_like(x)
    if "w" in want:
        out["w"] = np.empty_like(w)
    if "b" in want:
        out["b"] = np.empty(co, np.float32)
    ptr = lambda k: _lib.fptr(out[k]) if k in out else None
    _lib.check(_lib.lib().b2f_op_conv3x3s2_backward(_h(model), _lib.fptr(x), B, ci, H, W, _lib.fptr(w), co, int(bool(leaky)),
                                                    _lib.fptr(y) if y is not None else None, _lib.fptr(grad_y), int(layout), ptr("x"),
                                                    ptr("w"), ptr("b")))
    return out


def conv3x3s2_backward_plan(model, B, ci, H, W, co):
    """conv3x3_backward_plan for conv3x3s2_backward; H, W are the input map's, the chain counts output pixels.  Launches nothing."""
    partials, chain = C.c_int(0), C.c_longlong(0)
    _lib.check(_lib.lib().b2f_op_conv3x3s2_backward_plan(_h(model), int(B), int(ci), int(H), int(W), int(co), C.byref(partials),
                                                         C.byref(chain)))
    return partials.value, chain.value


KINDS = {"feat": 0, "occ": 1, "flow": 2, "past": 3}


def layer(model, kind, level, idx, x):
    """Conv (kind, level, idx) of the model's own packed weights on the launch path of the forward pass (chunk-planar buffers, the kernel the
    model's options choose for a batch of len(x)); kind 'feat' / 'occ' / 'flow' / 'past'.  x: n x Ci x H x W in the layer's Torch input
    order (a first decoder layer: {cv 162, cs[ref] C_l, flow 2}); returns n x Co x Ho x Wo."""
    x = _lib.f32(x)
    n, ci, H, W = x.shape
    name = ("feat%d.conv%d" % (level, idx)) if kind == "feat" else "l%d.%s.conv%d" % (level, kind, idx)
    co, ci_w = dict((nm, shape) for nm, shape, _ in weights.layout(model.past_flow)[0])[name + ".w"][:2]
    if ci != ci_w:
        raise ValueError("ops.layer: %s takes %d input channels, got %d" % (name, ci_w, ci))
    stride = 2 if (kind == "feat" and idx == 1) else 1
    y = np.empty((n, co, (H - 1) // stride + 1, (W - 1) // stride + 1), np.float32)
    _lib.check(_lib.lib().b2f_op_layer(_h(model), KINDS[kind], level, idx, n, H, W, _lib.fptr(x), _lib.fptr(y)))
    return y


def cv_record(model, ref, nbr_future, nbr_past, flow, flow_b, k):
    """The warp + cost-volume kernel on the forward's strides: the whole record, B x 168 x h x w in slot order; flow / flow_b may be None."""
    ref, nf, npast = _lib.f32(ref), _lib.f32(nbr_future), _lib.f32(nbr_past)
    B, Cc, h, w = ref.shape
    fl = [_lib.f32(f) if f is not None else None for f in (flow, flow_b)]
    assert all(f is None or f.shape == (B, 2, h, w) for f in fl)
    rec = np.empty((B, 168, h, w), np.float32)
    _lib.check(_lib.lib().b2f_op_cv_record(_h(model), _lib.fptr(ref), _lib.fptr(nf), _lib.fptr(npast), *[_lib.fptr(f) if f is not None else None for f in fl],
                                           float(k), B, Cc, h, w, _lib.fptr(rec)))
    return rec


def cv_variant(model, B, Cc, h, w, layout=0):
    """The variant of the warp + cost-volume kernel that the launcher runs for a B x Cc x h x w call under the model's options, on the
    strides of warp_costvol (layout 0) or of cv_record (layout 1).  Launches nothing."""
    v = _lib.lib().b2f_op_cv_variant(_h(model), int(B), int(Cc), int(h), int(w), int(layout))
    if v < 0:
        _lib.check(1)
    return v


def conv_head16(model, x, w1, b1, w2, b2):
    """conv(16,16,s1) + LeakyReLU(0.2) + conv(16,32,s2) + LeakyReLU(0.2) in the fused streaming kernel (pwc.lua:60-62)."""
    x, w1, b1, w2, b2 = _lib.f32(x), _lib.f32(w1), _lib.f32(b1), _lib.f32(w2), _lib.f32(b2)
    B, ci, H, W = x.shape
    assert ci == 16 and w1.shape == (16, 16, 3, 3) and w2.shape == (32, 16, 3, 3)
    y = np.empty((B, 32, (H - 1) // 2 + 1, (W - 1) // 2 + 1), np.float32)
    _lib.check(_lib.lib().b2f_op_conv_head16(_h(model), _lib.fptr(x), B, H, W, _lib.fptr(w1), _lib.fptr(b1), _lib.fptr(w2),
                                             _lib.fptr(b2), _lib.fptr(y)))
    return y


def conv_first(model, x, w, b, normalize=False):
    """The first pyramid conv as the forward launches it: conv(3, 16, s2) + LeakyReLU(0.2) on each of the three frames of x (B x 9 x H x W,
    H and W even), after ColorNormalize when normalize; returns 3 B x 16 x H/2 x W/2, image f * B + b (pwc.lua:59)."""
    x, w, b = _lib.f32(x), _lib.f32(w), _lib.f32(b)
    B, nine, H, W = x.shape
    assert nine == 9 and w.shape == (16, 3, 3, 3) and b.shape == (16,)
    y = np.empty((3 * B, 16, H // 2, W // 2), np.float32)
    _lib.check(_lib.lib().b2f_op_conv_first(_h(model), _lib.fptr(x), B, H, W, int(bool(normalize)), _lib.fptr(w), _lib.fptr(b), _lib.fptr(y)))
    return y


def upsample_flow2x(model, x):
    x = _lib.f32(x)
    B, two, h, w = x.shape
    assert two == 2
    y = np.empty((B, 2, 2 * h, 2 * w), np.float32)
    _lib.check(_lib.lib().b2f_op_upsample_flow2x(_h(model), _lib.fptr(x), B, h, w, _lib.fptr(y)))
    return y


def image_scale(model, src, Hd, Wd, normalize=False):
    """image.scale(src, Wd, Hd) 'bilinear' (back2future.lua:71) on C x Hs x Ws, optionally after ColorNormalize."""
    src = _lib.f32(src)
    Cc, Hs, Ws = src.shape
    dst = np.empty((Cc, Hd, Wd), np.float32)
    _lib.check(_lib.lib().b2f_op_image_scale(_h(model), _lib.fptr(src), Cc, Hs, Ws, int(normalize), _lib.fptr(dst), Hd, Wd))
    return dst


def warp_bhwd_backward(model, img, grid, grad_out, only_grid=False):
    """BilinearSamplerBHWD:updateGradInput: returns (grad_img or None, grad_grid)."""
    img, grid, grad_out = _lib.f32(img), _lib.f32(grid), _lib.f32(grad_out)
    B, ih, iw, Cc = img.shape
    _, gh, gw, _two = grid.shape
    gi = None if only_grid else np.empty_like(img)
    gg = np.empty_like(grid)
    _lib.check(_lib.lib().b2f_op_warp_bhwd_backward(_h(model), _lib.fptr(img), _lib.fptr(grid), _lib.fptr(grad_out), B, ih, iw, Cc,
                                                     gh, gw, _lib.fptr(gi) if gi is not None else None, _lib.fptr(gg)))
    return gi, gg


def costvol_backward(model, ref, frm, grad_out, win=9, fwd=True):
    """CostVolMulti:updateGradInput for {ref, frm}: returns (grad_ref, grad_frm)."""
    ref, frm, grad_out = _lib.f32(ref), _lib.f32(frm), _lib.f32(grad_out)
    B, Cc, h, w = ref.shape
    gr, gf = np.empty_like(ref), np.empty_like(frm)
    _lib.check(_lib.lib().b2f_op_costvol_backward(_h(model), _lib.fptr(ref), _lib.fptr(frm), _lib.fptr(grad_out), B, Cc, h, w, win,
                                                   int(bool(fwd)), _lib.fptr(gr), _lib.fptr(gf)))
    return gr, gf


def flow_rgb(flow, max=None, packed=False, model=None):
    """flowX.xy2rgb(flow[1], flow[2], max) (flowExtensions.lua:123-148) as bytes: flow 2 x H x W or n x 2 x H x W float32 ->
    (rgb uint8, max_used float64[n]); rgb is [n x] 3 x H x W or, with packed, [n x] H x W x 3.  max=None scales every image by
    its own largest norm.  model=None computes on the CPU (b2f_flow_rgb_host, no GPU), a Model on its GPU (b2f_op_flow_rgb)."""
    from .back2future import RGB_PACKED, RGB_PLANAR, rgb_max_norm
    max_norm = rgb_max_norm(max, "flow_rgb")
    f = np.asarray(flow)
    single = f.ndim == 3
    if single:
        f = f[None]
    if f.ndim != 4 or f.shape[1] != 2 or min(f.shape) < 1:
        raise ValueError("flow_rgb: expected a 2 x H x W or n x 2 x H x W flow, got shape %r" % (np.shape(flow),))
    f = _lib.f32(f)
    n, _, H, W = f.shape
    rgb = np.empty((n, H, W, 3) if packed else (n, 3, H, W), np.uint8)
    mx = np.empty(n, np.float64)
    args = (_lib.fptr(f), n, H, W, max_norm, RGB_PACKED if packed else RGB_PLANAR, rgb.ctypes.data_as(C.POINTER(C.c_ubyte)),
            mx.ctypes.data_as(C.POINTER(C.c_double)))
    if model is None:
        _lib.check(_lib.lib().b2f_flow_rgb_host(*args))
    else:
        _lib.check(_lib.lib().b2f_op_flow_rgb(_h(model), *args))
    return (rgb[0] if single else rgb), mx


def flow_score(flow, gt_flow, occ_prob=None, valid=None, gt_occ=None, flow_scale=20.0, model=None):
    """The score records of test.lua:183-261 (masked end-point error of criterions/L2Criterion.lua:36-38 split by the occlusion label,
    KITTI's Fl, the occlusion confusion matrix): flow n x 2 x H x W float32 raw network flow, gt_flow the same shape in pixels,
    occ_prob n x 2 x H x W float32, valid / gt_occ uint8 n x H x W (see Model.computeFlowBatchScore) -> uint64 (n, 22);
    back2future.score_summary turns them into EPE, Fl and the accuracies.  model=None computes on the CPU (b2f_flow_score_host, no
    GPU), a Model on its GPU (b2f_op_flow_score): the words are the same."""
    from .back2future import SCORE_WORDS, score_ground_truth
    f = np.asarray(flow)
    if f.ndim != 4 or f.shape[1] != 2 or min(f.shape) < 1:
        raise ValueError("flow_score: expected an n x 2 x H x W flow, got shape %r" % (np.shape(flow),))
    f = _lib.f32(f)
    n, _, H, W = f.shape
    gt, va, lb = score_ground_truth(n, H, W, gt_flow, valid, gt_occ, "flow_score")
    prob = None
    if occ_prob is not None:
        prob = np.asarray(occ_prob)
        if prob.shape != f.shape:
            raise ValueError("flow_score: occ_prob must have the flow's shape %r, got %r" % (f.shape, prob.shape))
        prob = _lib.f32(prob)
    scores = np.empty((n, SCORE_WORDS), np.uint64)
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    args = (_lib.fptr(f), _lib.fptr(prob) if prob is not None else None, n, H, W, float(flow_scale), _lib.fptr(gt), u8p(va), u8p(lb),
            scores.ctypes.data_as(C.POINTER(C.c_ulonglong)))
    if model is None:
        _lib.check(_lib.lib().b2f_flow_score_host(*args))
    else:
        _lib.check(_lib.lib().b2f_op_flow_score(_h(model), *args))
    return scores


def flow_warp(flow, im1, im2, im3, occ_prob=None, flow_scale=20.0, want_warped=True, want_photo=True, model=None, own_past_flow=False,
              past_flow=None):
    """Motion compensation (the warpingUnit of models/pwc.lua:67-73, nn.BilinearSamplerBHWD with CUDA semantics) and its photometric
    error (criterions/OBCCriterion.lua:79-100 with the L1 penalty): flow n x 2 x H x W float32 raw network flow; im1 / im2 / im3 the
    past, reference and future frames, n x 3 x H x W each, all uint8 (value byte / 255) or all float, not normalized; occ_prob
    n x 2 x H x W float32 or None -> (warped, photo): warped n x 2 x 3 x H x W in the frames' dtype ([:, 0] im1 warped with
    -flow_scale, [:, 1] im3 with +flow_scale), photo uint64 (n, 14) (back2future.photo_summary reads it); None for what is not
    wanted.  model=None computes on the CPU (b2f_flow_warp_host, no GPU), a Model on its GPU (b2f_op_flow_warp): the bytes and the
    words are the same.  own_past_flow=True with past_flow (n x 2 x H x W float32, a Soft model's own past flow, e.g.
    computeFlowBatchPast's): im1 is sampled at x - past_flow * flow_scale instead of x - flow * flow_scale (pwc.lua:425-432,
    OBCCriterion.lua:80-81; b2f_flow_warp_past_host / b2f_op_flow_warp_past); everything else is unchanged."""
    from .back2future import IN_U8, IN_UNIT, PHOTO_WORDS
    f = np.asarray(flow)
    if f.ndim != 4 or f.shape[1] != 2 or min(f.shape) < 1:
        raise ValueError("flow_warp: expected an n x 2 x H x W flow, got shape %r" % (np.shape(flow),))
    f = _lib.f32(f)
    n, _, H, W = f.shape
    ims = [np.asarray(a) for a in (im1, im2, im3)]
    if any(a.shape != (n, 3, H, W) for a in ims):
        raise ValueError("flow_warp: im1, im2 and im3 must have shape %r, got %r" % ((n, 3, H, W), [a.shape for a in ims]))
    kinds = {a.dtype == np.uint8 for a in ims}
    if len(kinds) > 1:
        raise ValueError("flow_warp: mixed dtypes (all frames uint8, or all float)")
    as_bytes = kinds == {True}
    ims = [np.ascontiguousarray(a) if as_bytes else _lib.f32(a) for a in ims]
    prob = None
    if occ_prob is not None:
        prob = np.asarray(occ_prob)
        if prob.shape != f.shape:
            raise ValueError("flow_warp: occ_prob must have the flow's shape %r, got %r" % (f.shape, prob.shape))
        prob = _lib.f32(prob)
    if bool(own_past_flow) != (past_flow is not None):
        raise ValueError("flow_warp: own_past_flow=True and past_flow go together")
    past = None
    if own_past_flow:
        past = np.asarray(past_flow)
        if past.shape != f.shape:
            raise ValueError("flow_warp: past_flow must have the flow's shape %r, got %r" % (f.shape, past.shape))
        past = _lib.f32(past)
    warped = np.empty((n, 2, 3, H, W), np.uint8 if as_bytes else np.float32) if want_warped else None
    photo = np.empty((n, PHOTO_WORDS), np.uint64) if want_photo else None
    args = (_lib.fptr(f), *((_lib.fptr(past),) if own_past_flow else ()), _lib.fptr(prob) if prob is not None else None, n, H, W, float(flow_scale), IN_U8 if as_bytes else IN_UNIT,
            *[C.c_void_p(a.ctypes.data) for a in ims], C.c_void_p(warped.ctypes.data) if warped is not None else None,
            photo.ctypes.data_as(C.POINTER(C.c_ulonglong)) if photo is not None else None)
    L = _lib.lib()
    if model is None:
        _lib.check((L.b2f_flow_warp_past_host if own_past_flow else L.b2f_flow_warp_host)(*args))
    else:
        _lib.check((L.b2f_op_flow_warp_past if own_past_flow else L.b2f_op_flow_warp)(_h(model), *args))
    return warped, photo


def table_loss(table, ref, flow_scale=20.0, model=None, objective="pme", ssim_range="batch"):
    """The records of the unsupervised validation loss (the -optimize pme branch of test.lua:266-297) of an output table of
    model:forward: table a list of L x 4 (Hard: per level future flow, occlusions, warped image 1, warped image 3) or L x 5 (Soft:
    the past flow second) float32 arrays n x C x (H >> j) x (W >> j), what Model.forward returns; ref n x 3 x H x W float32, the
    normalized centre frame (x[:, 3:6] of the network's input) -> uint64 (n, L, 16) (back2future.LOSS_*; back2future.loss_summary
    reads it).  model=None computes on the CPU (b2f_table_loss_host, no GPU), a Model on its GPU (b2f_op_table_loss; a table whose
    length fits both kinds, 20 tensors, is read as the model's kind): the words are the same.  objective="finetune" returns
    (n, L, 24) (b2f_table_loss_ft_host / b2f_op_table_loss_ft): the same 16 words, then the second-order smoothness and the
    gradient-constancy sums the Soft models were fine-tuned on (back2future.LOSS_FT_*).  objective="ssim" returns (n, L, 32)
    (b2f_table_loss_ssim_host / b2f_op_table_loss_ssim): the same 16 words, then the SSIM + L1 sums of -pme_criterion OSSIM | OSSIML1
    (criterions/OSSIML1Criterion.lua; back2future.LOSS_SSIM_*) on values normalised by ssim_range: "batch", the minimum and maximum
    over the n images of the call as in the reference; "image", each image's own; or an L x 2 array of (mn, mx) per level.
    objective="plain" returns (n, L, 40) (b2f_table_loss_plain_host / b2f_op_table_loss_plain): the same 16 words, then the sums of the
    photometric terms that do not mask occlusions, -pme_criterion BCC | SSIM | SSIML1 (criterions/MBCCriterion.lua,
    criterions/MSSIML1Criterion.lua; back2future.LOSS_PLAIN_*), with ssim_range as above; the range reaches over the occlusions and, on a
    Soft table, the past flow, as the Lua's does."""
    from .back2future import loss_words, loss_entry, ssim_range_args
    words = loss_words(objective)
    r = np.asarray(ref)
    if r.ndim != 4 or r.shape[1] != 3 or min(r.shape) < 1:
        raise ValueError("table_loss: expected an n x 3 x H x W reference image, got shape %r" % (np.shape(ref),))
    r = _lib.f32(r)
    n, _, H, W = r.shape
    tab = [_lib.f32(t) for t in table]
    if not tab or any(t.ndim != 4 or t.shape[0] != n for t in tab):
        raise ValueError("table_loss: the table must be a non-empty list of n x C x h x w arrays with the reference's n")
    per = 5 if (len(tab) >= 5 and tab[1].shape[1] == 2 and tab[2].shape[1] == 2) else 4
    if len(tab) % per:
        raise ValueError("table_loss: %d tensors are no whole number of levels of %d" % (len(tab), per))
    L = len(tab) // per
    for i, t in enumerate(tab):
        want = (n, 3 if i % per >= per - 2 else 2, H >> (i // per), W >> (i // per))
        if t.shape != want:
            raise ValueError("table_loss: tensor %d of the table must have shape %r, got %r" % (i, want, t.shape))
    ptrs = (_lib.c_float_p * len(tab))(*[_lib.fptr(t) for t in tab])
    loss = np.empty((n, L, words), np.uint64)
    lp = loss.ctypes.data_as(C.POINTER(C.c_ulonglong))
    tail = ssim_range_args(objective, ssim_range, L, "table_loss")
    if model is None:
        _lib.check(loss_entry("b2f_table_loss%s_host", objective)(ptrs, len(tab), n, H, W, int(per == 5), _lib.fptr(r), float(flow_scale), lp, *tail))
    else:
        if per != (5 if model.past_flow else 4) and len(tab) % (5 if model.past_flow else 4) == 0:
            raise ValueError("table_loss: a %s table of %d tensors on a %s model would be read as the model's kind; use a model of the "
                             "table's kind or model=None" % ("Soft" if per == 5 else "Hard", len(tab), "Soft" if model.past_flow else "Hard"))
        _lib.check(loss_entry("b2f_op_table_loss%s", objective)(_h(model), ptrs, len(tab), n, H, W, _lib.fptr(r), float(flow_scale), lp, *tail))
    return loss


def table_loss_grad(table, ref, flow_scale=20.0, options=None, model=None, ssim_range="batch"):
    """`gradOutputs` of train.lua:428-468 for an output table of model:forward: the gradient of the -optimize pme objective
    (first-order smoothness with L1, constant velocity, OBCC with L1, occlusion smoothness, occlusion prior; include/b2f.h gives every
    element) with respect to each tensor of the table.  table, ref, model as for table_loss; options: of
    back2future.loss_grad_options (None: the defaults of opts.lua:61-73), or of back2future.loss_grad_ft_options for the objectives
    with second-order smoothness and / or OBGCC (b2f_table_loss_grad_ft_host, b2f_op_table_loss_grad_ft) -> a list of float32 arrays
    with the table's shapes.  With the options of back2future.loss_grad_ssim_options the photometric term is the occlusion-aware SSIM +
    L1 of criterions/OSSIML1Criterion.lua:165-302 (b2f_table_loss_grad_ssim_host, b2f_op_table_loss_grad_ssim) on values normalised by
    ssim_range, as for table_loss; ssim_range is not read otherwise.  With the options of back2future.loss_grad_plain_options it is that of
    criterions/MBCCriterion.lua:104-186 or MSSIML1Criterion.lua:155-261, which do not mask occlusions (b2f_table_loss_grad_plain_host,
    b2f_op_table_loss_grad_plain), with ssim_range likewise.
    model=None computes on the CPU (b2f_table_loss_grad_host), a Model on its GPU (b2f_op_table_loss_grad): the bits are the same."""
    from .back2future import _grad_opts_ptr, _grad_entry, _grad_range_args
    r = np.asarray(ref)
    if r.ndim != 4 or r.shape[1] != 3 or min(r.shape) < 1:
        raise ValueError("table_loss_grad: expected an n x 3 x H x W reference image, got shape %r" % (np.shape(ref),))
    r = _lib.f32(r)
    n, _, H, W = r.shape
    tab = [_lib.f32(t) for t in table]
    if not tab or any(t.ndim != 4 or t.shape[0] != n for t in tab):
        raise ValueError("table_loss_grad: the table must be a non-empty list of n x C x h x w arrays with the reference's n")
    per = 5 if (len(tab) >= 5 and tab[1].shape[1] == 2 and tab[2].shape[1] == 2) else 4
    if len(tab) % per:
        raise ValueError("table_loss_grad: %d tensors are no whole number of levels of %d" % (len(tab), per))
    for i, t in enumerate(tab):
        want = (n, 3 if i % per >= per - 2 else 2, H >> (i // per), W >> (i // per))
        if t.shape != want:
            raise ValueError("table_loss_grad: tensor %d of the table must have shape %r, got %r" % (i, want, t.shape))
    ptrs = (_lib.c_float_p * len(tab))(*[_lib.fptr(t) for t in tab])
    grad = [np.empty(t.shape, np.float32) for t in tab]
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad])
    tail = _grad_range_args(options, ssim_range, len(tab) // per, "table_loss_grad")
    if model is None:
        _lib.check(_grad_entry("b2f_table_loss_grad_host", options)(ptrs, len(tab), n, H, W, int(per == 5), _lib.fptr(r), float(flow_scale), _grad_opts_ptr(options), gp, *tail))
    else:
        if per != (5 if model.past_flow else 4) and len(tab) % (5 if model.past_flow else 4) == 0:
            raise ValueError("table_loss_grad: a %s table of %d tensors on a %s model would be read as the model's kind; use a model of the "
                             "table's kind or model=None" % ("Soft" if per == 5 else "Hard", len(tab), "Soft" if model.past_flow else "Hard"))
        _lib.check(_grad_entry("b2f_op_table_loss_grad", options)(_h(model), ptrs, len(tab), n, H, W, _lib.fptr(r), float(flow_scale), _grad_opts_ptr(options), gp, *tail))
    return grad


def table_loss_epe(table, gt_flow, valid=None, gt_occ=None, flow_scale=20.0, options=None, count="batch", want_loss=True, want_grad=False,
                   model=None, rescale=False):
    """The supervised objective, -optimize epe (train.lua:296-334 with criterions/L2Criterion.lua:27-71; include/b2f.h gives every
    word and element), of an output table of model:forward against ground truth: table as for table_loss; gt_flow n x 2 x H x W
    float32, the true flow in pixels at the size of level 0; valid and gt_occ uint8 n x H x W or None (the conventions of flow_score:
    gt_occ bytes 0 / 1 / 2 are the labels 0 / 0.5 / 1, anything else is unlabelled); level j reads them at (y << j, x << j).
    options: of back2future.loss_epe_options (None: the defaults: epe 1, no occlusion term, no sizeAverage).  -> the records, uint64
    (n, L, 8) (back2future.LOSS_EPE_*; back2future.loss_summary(objective="epe") reads them), with want_grad the gradient table, a
    list of float32 arrays with the table's shapes (the future flow and, with occ > 0, the occlusions; every other tensor is +0.0);
    both as a tuple when both are wanted.  count: where sizeAverage takes its pixel counts from: "batch" (the n images of the call, as
    the reference), "image" or an L x 2 array (valid, labelled pixels per level); read by the gradient only.  model=None computes on
    the CPU (b2f_table_loss_epe_host, no GPU; rescale: the rescale_flow of the model that made the table, train.lua:300-302), a Model
    on its GPU (b2f_op_table_loss_epe, the model's own rescale_flow): the words and the bits are the same."""
    from .back2future import LOSS_EPE_WORDS, _epe_opts_ptr, epe_count_args, score_ground_truth
    if not want_loss and not want_grad:
        raise ValueError("table_loss_epe: want_loss and want_grad are both False")
    tab = [_lib.f32(t) for t in table]
    if not tab or any(t.ndim != 4 or t.shape[0] != tab[0].shape[0] or min(t.shape) < 1 for t in tab):
        raise ValueError("table_loss_epe: the table must be a non-empty list of n x C x h x w arrays of one n")
    n, _, H, W = tab[0].shape
    gt, va, lb = score_ground_truth(n, H, W, gt_flow, valid, gt_occ, "table_loss_epe")
    per = 5 if (len(tab) >= 5 and tab[1].shape[1] == 2 and tab[2].shape[1] == 2) else 4
    if len(tab) % per:
        raise ValueError("table_loss_epe: %d tensors are no whole number of levels of %d" % (len(tab), per))
    L = len(tab) // per
    for i, t in enumerate(tab):
        want = (n, 3 if i % per >= per - 2 else 2, H >> (i // per), W >> (i // per))
        if t.shape != want:
            raise ValueError("table_loss_epe: tensor %d of the table must have shape %r, got %r" % (i, want, t.shape))
    ptrs = (_lib.c_float_p * len(tab))(*[_lib.fptr(t) for t in tab])
    loss = np.empty((n, L, LOSS_EPE_WORDS), np.uint64) if want_loss else None
    lp = loss.ctypes.data_as(C.POINTER(C.c_ulonglong)) if want_loss else None
    grad = [np.empty(t.shape, np.float32) for t in tab] if want_grad else None
    gp = (_lib.c_float_p * len(grad))(*[_lib.fptr(g) for g in grad]) if want_grad else None
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None
    mode, counts = epe_count_args(count, L, "table_loss_epe")
    if model is None:
        _lib.check(_lib.lib().b2f_table_loss_epe_host(ptrs, len(tab), n, H, W, int(per == 5), _lib.fptr(gt), u8p(va), u8p(lb), float(flow_scale),
                                                      int(bool(rescale)), _epe_opts_ptr(options), mode, counts, lp, gp))
    else:
        if per != (5 if model.past_flow else 4) and len(tab) % (5 if model.past_flow else 4) == 0:
            raise ValueError("table_loss_epe: a %s table of %d tensors on a %s model would be read as the model's kind; use a model of the "
                             "table's kind or model=None" % ("Soft" if per == 5 else "Hard", len(tab), "Soft" if model.past_flow else "Hard"))
        _lib.check(_lib.lib().b2f_op_table_loss_epe(_h(model), ptrs, len(tab), n, H, W, _lib.fptr(gt), u8p(va), u8p(lb), float(flow_scale),
                                                    _epe_opts_ptr(options), mode, counts, lp, gp))
    if want_loss and want_grad:
        return loss, grad
    return loss if want_loss else grad


# ---- the small kernels of a forward pass, one launcher each, on the caller's own strides (tests/glue_float64.py) ----------------------

def _u8_or_f32(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a) if a.dtype == np.uint8 else _lib.f32(a)


def _in_kind(a, normalized):
    from .back2future import IN_NORMALIZED, IN_U8, IN_UNIT
    return IN_U8 if a.dtype == np.uint8 else (IN_NORMALIZED if normalized else IN_UNIT)


def upsample_flow2x_records(model, x, planar=False):
    """nn.SpatialUpSamplingBilinear(2) of slots 0..1 of the records x: B x h x w x ps -> B x 2h x 2w x 2, or planar B x 2 x 2h x 2w."""
    x = _lib.f32(x)
    B, h, w, ps = x.shape
    y = np.empty((B, 2, 2 * h, 2 * w) if planar else (B, 2 * h, 2 * w, 2), np.float32)
    _lib.check(_lib.lib().b2f_op_upsample_flow2x_ex(_h(model), _lib.fptr(x), ps, B, h, w, int(bool(planar)), _lib.fptr(y)))
    return y


def softmax_nearest4(model, logits):
    """softmax over slots 0..1 of the records logits: B x h x w x ps, repeated 4 x 4 -> B x 2 x 4h x 4w"""
    x = _lib.f32(logits)
    B, h, w, ps = x.shape
    y = np.empty((B, 2, 4 * h, 4 * w), np.float32)
    _lib.check(_lib.lib().b2f_op_softmax_nearest4(_h(model), _lib.fptr(x), ps, B, h, w, _lib.fptr(y)))
    return y


def avgpool2(model, x):
    """nn.SpatialAveragePooling(2,2,2,2) on n x H x W x C -> n x H/2 x W/2 x C"""
    x = _lib.f32(x)
    n, H, W, Cc = x.shape
    y = np.empty((n, H // 2, W // 2, Cc), np.float32)
    _lib.check(_lib.lib().b2f_op_avgpool2(_h(model), _lib.fptr(x), n, H, W, Cc, _lib.fptr(y)))
    return y


def pack_input(model, x, normalize=False):
    """B x 9 x H x W -> the packed frames 3 x B x H x W x 8"""
    x = _lib.f32(x)
    B, nine, H, W = x.shape
    assert nine == 9
    y = np.empty((3, B, H, W, 8), np.float32)
    _lib.check(_lib.lib().b2f_op_pack_input(_h(model), _lib.fptr(x), int(bool(normalize)), B, H, W, _lib.fptr(y)))
    return y


def warp_image(model, which, x, flow, k, normalized=True, frame=0):
    """which 'image': x B x H x W x 8 packed (launch_warp_image_planar); 'input': x B x 9 x H x W, its frame `frame`, normalized on the
    fly unless `normalized` (launch_warp_input_planar); 'seq': x B x 3 x H x W float32 or uint8 (launch_warp_input_seq).
    flow B x 2 x H x W -> B x 3 x H x W."""
    w_i = {"image": 0, "input": 1, "seq": 2}[which]
    x, flow = _u8_or_f32(x), _lib.f32(flow)
    B, _two, H, W = flow.shape
    assert x.shape == {0: (B, H, W, 8), 1: (B, 9, H, W), 2: (B, 3, H, W)}[w_i] and (w_i == 2 or x.dtype == np.float32)
    out = np.empty((B, 3, H, W), np.float32)
    _lib.check(_lib.lib().b2f_op_warp_image(_h(model), w_i, C.c_void_p(x.ctypes.data), _in_kind(x, normalized), int(frame), _lib.fptr(flow),
                                            float(k), B, H, W, _lib.fptr(out)))
    return out


def conv_first_seq(model, x, w, b, normalized=True):
    """ops.conv_first on the frames of a sequence: x T x 3 x H x W float32 (normalized or unit) or uint8 -> T x 16 x H/2 x W/2"""
    x, w, b = _u8_or_f32(x), _lib.f32(w), _lib.f32(b)
    T, three, H, W = x.shape
    assert three == 3 and w.shape == (16, 3, 3, 3) and b.shape == (16,)
    y = np.empty((T, 16, H // 2, W // 2), np.float32)
    _lib.check(_lib.lib().b2f_op_conv_first_seq(_h(model), C.c_void_p(x.ctypes.data), _in_kind(x, normalized), T, H, W, _lib.fptr(w), _lib.fptr(b),
                                                _lib.fptr(y)))
    return y


def layout(model, which, x, Cc, pix_stride=0):
    """'nhwc_to_planar': B x h x w x pix_stride -> B x Cc x h x w; 'cp8_to_planar': B x ceil(Cc/8) x h x w x 8 -> B x Cc x h x w;
    'planar_to_nhwc': B x Cc x h x w -> B x h x w x pix_stride"""
    w_i = {"nhwc_to_planar": 0, "cp8_to_planar": 1, "planar_to_nhwc": 2}[which]
    x = _lib.f32(x)
    if w_i == 0:
        B, h, w, pix_stride = x.shape
    elif w_i == 1:
        B, _chunks, h, w, _eight = x.shape
        assert _chunks == (Cc + 7) // 8 and _eight == 8
    else:
        B, _c, h, w = x.shape
        assert _c == Cc
    out = np.empty((B, h, w, pix_stride) if w_i == 2 else (B, Cc, h, w), np.float32)
    _lib.check(_lib.lib().b2f_op_layout(_h(model), w_i, _lib.fptr(x), Cc, pix_stride, B, h, w, _lib.fptr(out)))
    return out


def graph_put_channels(model, src, kind, Cc, dst, c_off):
    """put_channels of the generic executor: Cc channels of src (kind 0: B x chunks x hw x 8, 1: B x hw x Cc, 2: B x Cc x hw) into
    channels c_off .. of a copy of dst (B x chunks x hw x 8), which is returned"""
    src, dst = _lib.f32(src), _lib.f32(dst).copy()
    B, dch, hw, _e = dst.shape
    _lib.check(_lib.lib().b2f_op_graph_put_channels(_h(model), _lib.fptr(src), kind, src.shape[1] if kind == 0 else 0, Cc, B, hw, _lib.fptr(dst),
                                                    dch, c_off))
    return dst


def graph_costvol(model, ref, frmF, frmB, Cc, win, chunksJ, chunksS=0):
    """costvol_cp8 of the generic executor on chunk-planar maps B x chunks x h x w x 8: (dstJ B x chunksJ x h x w x 8, dstS or None)"""
    ref, frmF = _lib.f32(ref), _lib.f32(frmF)
    frmB = _lib.f32(frmB) if frmB is not None else None
    B, ch, h, w, _e = ref.shape
    J = np.empty((B, chunksJ, h, w, 8), np.float32)
    S = np.empty((B, chunksS, h, w, 8), np.float32) if chunksS else None
    _lib.check(_lib.lib().b2f_op_graph_costvol(_h(model), _lib.fptr(ref), _lib.fptr(frmF), _lib.fptr(frmB) if frmB is not None else None, ch, Cc, B,
                                               h, w, win, _lib.fptr(J), chunksJ, _lib.fptr(S) if S is not None else None, chunksS))
    return J, S


def graph_warp(model, img, flow, k):
    """warp_cp8 of the generic executor: img B x chunks x h x w x 8, flow B x h x w x 2"""
    img, flow = _lib.f32(img), _lib.f32(flow)
    B, ch, h, w, _e = img.shape
    assert flow.shape == (B, h, w, 2)
    out = np.empty_like(img)
    _lib.check(_lib.lib().b2f_op_graph_warp(_h(model), _lib.fptr(img), ch, _lib.fptr(flow), float(k), B, h, w, _lib.fptr(out)))
    return out


def graph_add_flow(model, fs, u):
    """fs: npix x 8 records, u: npix x 2 -> fs with u added to slots 0..1"""
    fs, u = _lib.f32(fs).copy(), _lib.f32(u)
    assert fs.ndim == 2 and fs.shape[1] == 8 and u.shape == (fs.shape[0], 2)
    _lib.check(_lib.lib().b2f_op_graph_add_flow(_h(model), _lib.fptr(fs), _lib.fptr(u), fs.shape[0]))
    return fs


def graph_scale(model, p, k):
    p = _lib.f32(p).copy()
    _lib.check(_lib.lib().b2f_op_graph_scale(_h(model), _lib.fptr(p), p.size, float(k)))
    return p


def graph_softmax_nearest(model, logits, f):
    """softmax_nearest of the generic executor: logits B x h x w x 8 -> B x 2 x f h x f w"""
    x = _lib.f32(logits)
    B, h, w, _e = x.shape
    assert _e == 8
    out = np.empty((B, 2, f * h, f * w), np.float32)
    _lib.check(_lib.lib().b2f_op_graph_softmax_nearest(_h(model), _lib.fptr(x), B, h, w, int(f), _lib.fptr(out)))
    return out


def expf(model, x):
    """expf of the device library, elementwise, as the softmax kernels call it"""
    x = _lib.f32(x)
    y = np.empty_like(x)
    _lib.check(_lib.lib().b2f_op_expf(_h(model), _lib.fptr(x), x.size, _lib.fptr(y)))
    return y
