#!/usr/bin/env python3
"""Score the flow of a clip against ground truth on the GPU: the evaluation of the reference's test.lua:183-261 (end-point error,
its split into visible and occluded pixels, the occlusion accuracies) plus KITTI's outlier rate Fl.  The frames are uploaded once
with their ground truth (Model.computeFlowSequenceScore); 176 bytes per centre frame come back.

Usage: python examples/evaluate.py FRAMES_DIR GT_DIR [model] [--scale S]
FRAMES_DIR: the frames, sorted by name.  GT_DIR holds, for every centre frame NAME (a frame with a neighbour on both sides):
  NAME.flo         the ground-truth flow in pixels (required)
  NAME_valid.png   optional: nonzero = the pixel counts (absent: every pixel; Sintel's unknown pixels must be masked here)
  NAME_occ.png     optional: 0 = occluded "bwd", 127 / 128 = visible, 255 = occluded "fwd" (the labels 0 / 0.5 / 1 of test.lua as
                   image.save writes them); any other grey level = unlabelled
A plane that is absent for one frame is left out for the whole clip.  model as for examples/run_sequence.py (default
'Ours-Soft-ft-KITTI'); --scale: pixels per unit of raw network flow (default 20, opts.lua flownet_factor).
Prints one `name value` line per measure of back2future.score_summary.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from back2future_amd import back2future, flow_io   # noqa: E402

EXTS = (".png", ".jpg", ".jpeg", ".ppm", ".bmp")


def load_grey(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.uint8)


def occ_labels(grey):
    """grey levels of an occlusion picture -> the library's labels 0 / 1 / 2, 255 = unlabelled"""
    lut = np.full(256, 255, np.uint8)
    lut[0], lut[127], lut[128], lut[255] = 0, 1, 1, 2
    return lut[grey]


def main():
    args = list(sys.argv[1:])
    scale = 20.0
    if "--scale" in args:
        i = args.index("--scale")
        try:
            scale = float(args[i + 1])
        except (IndexError, ValueError):
            sys.exit("--scale S: S must be a number")
        del args[i:i + 2]
    if len(args) < 2:
        sys.exit(__doc__)
    src, gt_dir = args[0], args[1]
    model = args[2] if len(args) > 2 else "Ours-Soft-ft-KITTI"
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(EXTS))
    if len(names) < 3:
        sys.exit("%s: need at least 3 frames, found %d" % (src, len(names)))
    frames = np.stack([flow_io.load_image(os.path.join(src, f)) for f in names])
    stems = [os.path.join(gt_dir, os.path.splitext(f)[0]) for f in names[1:-1]]
    for s in stems:
        if not os.path.exists(s + ".flo"):
            sys.exit("%s.flo: no ground truth for this centre frame" % s)
    gt = np.stack([flow_io.loadFLO(s + ".flo") for s in stems])
    if gt.shape[2:] != frames.shape[2:]:
        sys.exit("the ground truth is %d x %d, the frames are %d x %d" % (gt.shape[2:] + frames.shape[2:]))
    valid = occ = None
    if all(os.path.exists(s + "_valid.png") for s in stems):
        valid = np.stack([(load_grey(s + "_valid.png") != 0).astype(np.uint8) for s in stems])
    if all(os.path.exists(s + "_occ.png") for s in stems):
        occ = np.stack([occ_labels(load_grey(s + "_occ.png")) for s in stems])
    m = back2future.Model(model)
    scores = m.computeFlowSequenceScore(frames, gt, valid=valid, gt_occ=occ, flow_scale=scale)
    m.close()
    for k, v in back2future.score_summary(scores).items():
        print("%s %r" % (k, v))


if __name__ == "__main__":
    main()
