#!/usr/bin/env python3
"""The unsupervised validation loss of a clip on the GPU: for every centre frame (a frame with a neighbour on both sides) the
objective the reference validates a model trained without labels with -- the -optimize pme branch of test.lua:266-297: flow
smoothness, constant velocity, the occlusion-aware photometric error of the model's own warped images, occlusion smoothness and
the occlusion prior, on every level of the output table.  No ground truth is needed.  The table stays on the GPU
(Model.forwardLoss); 128 bytes per level and centre frame come back.  --objective NAME prints instead the objective the named model
was trained on (back2future.LOSS_OBJECTIVES, the commands of the reference's README.md:85-102): for the two Soft models the
second-order smoothness and the brightness and gradient constancy of OBGCC, from records of 192 bytes (objective="finetune").
--pme-criterion OSSIM | OSSIML1 replaces the photometric term by the occlusion-aware SSIM (+ L1) term of
criterions/OSSIML1Criterion.lua, from records of 256 bytes (objective="ssim"); --ssim-range image (the default) normalises every
triplet by its own minimum and maximum, which does not depend on how the clip is cut into calls; --ssim-range batch takes them over
the triplets of a call as the reference does over a batch.
--grad also computes `gradOutputs` of train.lua:428-468, the gradient of the pme objective with respect to every tensor of the output
table (Model.forwardLossGrad, in the same pass as the records), under the chosen options (--size-average; --objective Ours-Hard --
--grad refuses the two Soft objectives), and prints per level and tensor its L2 norm and largest magnitude over the clip.  --grad-ft
does the same with the gradients of SecondOrderSmoothnessCriterion and OBGCCriterion (back2future.loss_grad_ft_options): any
--objective NAME, or without one both criteria with alpha = beta = gamma = 1; its loss lines come from the 192-byte records.
--grad-ssim does the same with the gradient of the SSIM (+ L1) term (back2future.loss_grad_ssim_options; OSSIML1Criterion.lua:165-302):
--pme-criterion OSSIM | OSSIML1 (the default) and --ssim-range as above; its loss lines come from the 256-byte records of the same pass.
--plain-criterion BCC | SSIM | SSIML1 takes the photometric terms that do not mask occlusions instead (the reference's -pme_criterion
BCC | SSIM | SSIML1: criterions/MBCCriterion.lua, criterions/MSSIML1Criterion.lua, the paper's baseline), from records of 320 bytes
(objective="plain"); --pme-penalty Quadratic leaves MBCCriterion's own penalty in place (BCC only); --no-occ drops the occlusions'
smoothness and prior from the sum (opts.lua:85); --grad-plain also computes the gradient under these options
(back2future.loss_grad_plain_options) in the same pass.  (--pme-criterion keeps the two occlusion-aware names it had.)
--objective epe --gt GT_DIR prints the supervised objective instead (-optimize epe, train.lua:296-334: the masked end-point error of
the future flow of every level against ground truth; Model.forwardLoss(objective="epe"), 64 bytes per level and centre frame come
back).  GT_DIR holds, per centre frame NAME, what examples/evaluate.py reads: NAME.flo, and optionally NAME_valid.png and NAME_occ.png
(cropped like the frames).  --occ-weight W > 0 adds the occlusion term that train.lua:316-332 intends (it needs every NAME_occ.png);
--size-average divides every level by its valid (labelled) pixels, per triplet; --grad also computes its `gradOutputs`
(Model.forwardLossGrad(objective="epe")).  It prints `err`, `flow LEVEL value` and `occ LEVEL value` per level, `epe` in pixels
(train.lua:340-344) and `nonfinite`, the values of back2future.loss_summary(objective="epe"), then the grad lines.

Usage: python examples/validate.py FRAMES_DIR MODEL [--scale S] [--like test|train] [--size-average] [--objective NAME]
       [--pme-criterion OSSIM|OSSIML1 [--ssim-range image|batch]] [--grad | --grad-ft | --grad-ssim]
       python examples/validate.py FRAMES_DIR MODEL --plain-criterion BCC|SSIM|SSIML1 [--pme-penalty Quadratic] [--no-occ] [--grad-plain]
       [--scale S] [--like test|train] [--size-average] [--ssim-range image|batch]
       python examples/validate.py FRAMES_DIR MODEL --objective epe --gt GT_DIR [--scale S] [--occ-weight W] [--size-average] [--grad]
FRAMES_DIR: 8-bit frames, sorted by name; they are cropped (top left) to multiples of 64 and normalized with
back2future.normalize.  MODEL as for examples/run_sequence.py.  --scale: pixels per unit of raw network flow (default 20).
Prints one `name loss` line per centre frame, then `mean loss` and `nonfinite count`; with --grad, --grad-ft or --grad-ssim then one line
`grad LEVEL TENSOR l2 max` per level and tensor (f, p for Soft models, o, iw1, iw3).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from back2future_amd import back2future   # noqa: E402

EXTS = (".png", ".jpg", ".jpeg", ".ppm", ".bmp")
BATCH = 8   # triplets per forwardLoss call


def load_unit(path, H, W):
    from PIL import Image
    a = np.asarray(Image.open(path).convert("RGB"), np.uint8)[:H, :W]
    return np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


def load_grey(path, H, W):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.uint8)[:H, :W]


def main_epe(src, model, gt_dir, scale, occ_weight, size_average, grad):
    """--objective epe: the supervised objective of train.lua:296-334 over the clip"""
    from back2future_amd import flow_io
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(EXTS))
    if len(names) < 3:
        sys.exit("%s: need at least 3 frames, found %d" % (src, len(names)))
    from PIL import Image
    W0, H0 = Image.open(os.path.join(src, names[0])).size
    H, W = H0 // 64 * 64, W0 // 64 * 64
    if H < 64 or W < 64:
        sys.exit("%s: frames of %d x %d are smaller than 64 x 64" % (src, H0, W0))
    stems = [os.path.join(gt_dir, os.path.splitext(f)[0]) for f in names[1:-1]]
    for s in stems:
        if not os.path.exists(s + ".flo"):
            sys.exit("%s.flo: no ground truth for this centre frame" % s)
    gt = np.stack([flow_io.loadFLO(s + ".flo") for s in stems])
    if gt.shape[2:] != (H0, W0):
        sys.exit("the ground truth is %d x %d, the frames are %d x %d" % (gt.shape[2:] + (H0, W0)))
    gt = np.ascontiguousarray(gt[:, :, :H, :W], np.float32)
    valid = occ = None
    if all(os.path.exists(s + "_valid.png") for s in stems):
        valid = np.stack([(load_grey(s + "_valid.png", H, W) != 0).astype(np.uint8) for s in stems])
    if all(os.path.exists(s + "_occ.png") for s in stems):
        lut = np.full(256, 255, np.uint8)     # the labels of examples/evaluate.py: 0 occluded "bwd", 127 / 128 visible, 255 occluded "fwd"
        lut[0], lut[127], lut[128], lut[255] = 0, 1, 1, 2
        occ = np.stack([lut[load_grey(s + "_occ.png", H, W)] for s in stems])
    if occ_weight > 0 and occ is None:
        sys.exit("--occ-weight: needs NAME_occ.png for every centre frame")
    weights = {"occ": occ_weight}
    options = back2future.loss_epe_options(weights=weights, size_average=size_average)
    frames = [back2future.normalize(load_unit(os.path.join(src, f), H, W)) for f in names]
    m = back2future.Model(model)
    records, sumsq, largest = [], None, None
    for b0 in range(0, len(frames) - 2, BATCH):
        b1 = min(b0 + BATCH, len(frames) - 2)
        x = np.stack([np.concatenate(frames[i:i + 3], axis=0) for i in range(b0, b1)])
        kw = dict(flow_scale=scale, objective="epe", gt_flow=gt[b0:b1], valid=None if valid is None else valid[b0:b1],
                  gt_occ=None if occ is None else occ[b0:b1], options=options)
        if grad:
            g, rec = m.forwardLossGrad(x, count="image", **kw)
            sq = [float((t.astype(np.float64) ** 2).sum()) for t in g]
            mx = [float(np.abs(t).max()) for t in g]
            sumsq = sq if sumsq is None else [a + b for a, b in zip(sumsq, sq)]
            largest = mx if largest is None else [max(a, b) if a == a and b == b else float("nan") for a, b in zip(largest, mx)]
        else:
            rec = m.forwardLoss(x, **kw)
        records.append(rec)
    tensors = ("f", "p", "o", "iw1", "iw3") if m.past_flow else ("f", "o", "iw1", "iw3")
    m.close()
    s = back2future.loss_summary(np.concatenate(records), objective="epe", size_average=size_average, weights=weights, flow_scale=scale, count="image")
    print("err %r" % s["err"])
    for j, v in enumerate(s["flow"]):
        print("flow %d %r" % (j, float(v)))
    for j, v in enumerate(s["occ"]):
        print("occ %d %r" % (j, float(v)))
    print("epe %r" % s["epe"])
    print("nonfinite %d" % s["nonfinite"])
    if grad:
        for i, (sq, mx) in enumerate(zip(sumsq, largest)):
            print("grad %d %s %r %r" % (i // len(tensors), tensors[i % len(tensors)], float(np.sqrt(sq)), mx))


def main():
    args = list(sys.argv[1:])
    scale, like, objective, criterion, ssim_range = 20.0, "test", None, None, "image"
    gt_dir, occ_weight, penalty = None, 0.0, "L1"
    size_average, grad_ft, grad_ssim = "--size-average" in args, "--grad-ft" in args, "--grad-ssim" in args
    grad_plain, no_occ = "--grad-plain" in args, "--no-occ" in args
    grad = "--grad" in args or grad_ft or grad_ssim or grad_plain
    if ("--grad" in args) + grad_ft + grad_ssim + grad_plain > 1:
        sys.exit("--grad, --grad-ft, --grad-ssim and --grad-plain exclude one another")
    args = [a for a in args if a not in ("--size-average", "--grad", "--grad-ft", "--grad-ssim", "--grad-plain", "--no-occ")]
    plain_criterion = None
    for flag in ("--scale", "--like", "--objective", "--pme-criterion", "--plain-criterion", "--pme-penalty", "--ssim-range", "--gt", "--occ-weight"):
        if flag in args:
            i = args.index(flag)
            try:
                if flag == "--scale":
                    scale = float(args[i + 1])
                elif flag == "--like":
                    like = args[i + 1]
                elif flag == "--pme-criterion":
                    criterion = args[i + 1]
                elif flag == "--plain-criterion":
                    plain_criterion = args[i + 1]
                elif flag == "--pme-penalty":
                    penalty = args[i + 1]
                elif flag == "--ssim-range":
                    ssim_range = args[i + 1]
                elif flag == "--gt":
                    gt_dir = args[i + 1]
                elif flag == "--occ-weight":
                    occ_weight = float(args[i + 1])
                else:
                    objective = args[i + 1]
            except (IndexError, ValueError):
                sys.exit(flag + ": bad value")
            del args[i:i + 2]
    if len(args) != 2 or like not in ("test", "train"):
        sys.exit(__doc__)
    if objective == "epe":
        if gt_dir is None or criterion is not None or plain_criterion is not None or grad_ft or grad_ssim or grad_plain or no_occ or like != "test" or not (occ_weight >= 0.0 and np.isfinite(occ_weight)):
            sys.exit("--objective epe: needs --gt GT_DIR, takes --scale, --occ-weight W >= 0, --size-average and --grad")
        return main_epe(args[0], args[1], gt_dir, scale, occ_weight, size_average, grad)
    if gt_dir is not None or occ_weight != 0.0:
        sys.exit("--gt and --occ-weight go with --objective epe")
    if objective is not None and objective not in back2future.LOSS_OBJECTIVES:
        sys.exit("--objective: epe, or one of " + ", ".join(sorted(back2future.LOSS_OBJECTIVES)))
    unmasked = ("BCC", "SSIM", "SSIML1")
    if criterion is not None and criterion not in back2future.SSIM_ALPHA:
        sys.exit("--pme-criterion: one of " + ", ".join(sorted(back2future.SSIM_ALPHA)) + " (the criteria that do not mask occlusions: --plain-criterion)")
    if plain_criterion is not None and plain_criterion not in unmasked:
        sys.exit("--plain-criterion: one of " + ", ".join(unmasked))
    if plain_criterion is not None and criterion is not None:
        sys.exit("--pme-criterion and --plain-criterion exclude one another")
    if ssim_range not in ("image", "batch"):
        sys.exit("--ssim-range: image or batch")
    if grad_ssim and criterion is None and plain_criterion is None:
        criterion = "OSSIML1"
    if grad_plain and plain_criterion is None and criterion is None:
        plain_criterion = "BCC"
    plain = plain_criterion is not None
    if plain:
        criterion = plain_criterion
    if penalty not in ("L1", "Quadratic") or (penalty == "Quadratic" and plain_criterion != "BCC"):
        sys.exit("--pme-penalty: L1, or Quadratic with --plain-criterion BCC")
    if (grad_plain or no_occ) and not plain:
        sys.exit("--grad-plain and --no-occ go with --plain-criterion BCC, SSIM or SSIML1")
    if criterion is not None and (objective is not None or (grad and not (grad_plain if plain else grad_ssim))):
        sys.exit("--pme-criterion and --plain-criterion go without --objective, --grad and --grad-ft (the gradient of a --pme-criterion is that of "
                 "--grad-ssim, of a --plain-criterion that of --grad-plain)")
    options = None
    if grad_plain:
        options = back2future.loss_grad_plain_options(size_average=size_average, pme_criterion=criterion, pme_penalty=penalty, no_occ=no_occ)
    elif grad_ssim:
        options = back2future.loss_grad_ssim_options(size_average=size_average, pme_criterion=criterion)
    elif grad:
        try:
            make = back2future.loss_grad_ft_options if grad_ft else back2future.loss_grad_options
            options = make(size_average=size_average, objective=objective)
        except ValueError as e:
            sys.exit("%s: %s" % ("--grad-ft" if grad_ft else "--grad", e))
    src, model = args
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(EXTS))
    if len(names) < 3:
        sys.exit("%s: need at least 3 frames, found %d" % (src, len(names)))
    from PIL import Image
    W0, H0 = Image.open(os.path.join(src, names[0])).size
    H, W = H0 // 64 * 64, W0 // 64 * 64
    if H < 64 or W < 64:
        sys.exit("%s: frames of %d x %d are smaller than 64 x 64" % (src, H0, W0))
    frames = [back2future.normalize(load_unit(os.path.join(src, f), H, W)) for f in names]
    m = back2future.Model(model)
    records, sumsq, largest = [], None, None
    for b0 in range(0, len(frames) - 2, BATCH):
        x = np.stack([np.concatenate(frames[i:i + 3], axis=0) for i in range(b0, min(b0 + BATCH, len(frames) - 2))])
        if grad:
            g, rec = m.forwardLossGrad(x, flow_scale=scale, options=options, ssim_range=ssim_range)
            records.append(rec)
            sq = [float((t.astype(np.float64) ** 2).sum()) for t in g]
            mx = [float(np.abs(t).max()) for t in g]
            sumsq = sq if sumsq is None else [a + b for a, b in zip(sumsq, sq)]
            largest = mx if largest is None else [max(a, b) if a == a and b == b else float("nan") for a, b in zip(largest, mx)]
        elif criterion is not None:
            records.append(m.forwardLoss(x, flow_scale=scale, objective="plain" if plain else "ssim", ssim_range=ssim_range))
        else:
            records.append(m.forwardLoss(x, flow_scale=scale, objective="pme" if objective is None else "finetune"))
    tensors = ("f", "p", "o", "iw1", "iw3") if m.past_flow else ("f", "o", "iw1", "iw3")
    m.close()
    if plain:
        s = back2future.loss_summary(np.concatenate(records), like=like, size_average=size_average, pme_criterion=criterion, pme_penalty=penalty, no_occ=no_occ)
    elif criterion is not None:
        s = back2future.loss_summary(np.concatenate(records), like=like, size_average=size_average, pme_criterion=criterion)
    elif grad_ft and objective is None:     # the defaults of loss_grad_ft_options
        s = back2future.loss_summary(np.concatenate(records), like=like, size_average=size_average, smooth_second_order=True, pme_criterion="OBGCC")
    else:
        s = back2future.loss_summary(np.concatenate(records), like=like, size_average=size_average, objective=objective)
    for f, v in zip(names[1:-1], s["loss"]):
        print("%s %r" % (os.path.splitext(f)[0], float(v)))
    print("mean %r" % s["mean"])
    print("nonfinite %d" % s["nonfinite"])
    if grad:
        for i, (sq, mx) in enumerate(zip(sumsq, largest)):
            print("grad %d %s %r %r" % (i // len(tensors), tensors[i % len(tensors)], float(np.sqrt(sq)), mx))


if __name__ == "__main__":
    main()
