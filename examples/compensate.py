#!/usr/bin/env python3
"""Motion compensation of a clip on the GPU: for every centre frame (a frame with a neighbour on both sides) the past and the
future frame warped onto it by the flow -- what the reference returns as warped_img_1 .. warped_img_N (models/pwc.lua:67-73) --
and the photometric error of those warps, the measure test.lua:285 reports through criterions/OBCCriterion.lua with the L1
penalty.  No ground truth is needed.  The frames are uploaded once as bytes (Model.computeFlowSequenceWarp); the warped frames and
112 bytes per centre frame come back, or with --no-images the 112 bytes alone.

Usage: python examples/compensate.py FRAMES_DIR OUT_DIR [model] [--scale S] [--no-images] [--own-past-flow] [--stream]
FRAMES_DIR: 8-bit frames, sorted by name.  OUT_DIR receives NAME_past.png and NAME_future.png for every centre frame NAME.
model as for examples/run_sequence.py (default 'Ours-Soft-ft-KITTI'); --scale: pixels per unit of raw network flow (default 20).
--own-past-flow (Soft models): the past frame is warped with the model's own past flow instead of minus the future flow, which is
the reference's warped_img_1 and the past half of its photometric error (pwc.lua:425-432, OBCCriterion.lua:80-81).
--stream: push the frames one at a time (Model.openStream(warp=True) / MotionStream.pushWarp, the calling pattern of a camera:
every frame is uploaded once and the compensated neighbours of a centre frame come back with the push of its future frame) instead
of handing over the clip; the files and the printed lines are the same, byte for byte.
Prints one `name value` line per measure of back2future.photo_summary.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from back2future_amd import back2future, flow_io   # noqa: E402

EXTS = (".png", ".jpg", ".jpeg", ".ppm", ".bmp")


def load_bytes(path):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), np.uint8).transpose(2, 0, 1))


def main():
    args = list(sys.argv[1:])
    scale = 20.0
    images = "--no-images" not in args
    own = "--own-past-flow" in args
    stream = "--stream" in args
    args = [a for a in args if a not in ("--no-images", "--own-past-flow", "--stream")]
    if "--scale" in args:
        i = args.index("--scale")
        try:
            scale = float(args[i + 1])
        except (IndexError, ValueError):
            sys.exit("--scale S: S must be a number")
        del args[i:i + 2]
    if len(args) < 2:
        sys.exit(__doc__)
    src, dst = args[0], args[1]
    model = args[2] if len(args) > 2 else "Ours-Soft-ft-KITTI"
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(EXTS))
    if len(names) < 3:
        sys.exit("%s: need at least 3 frames, found %d" % (src, len(names)))
    frames = np.stack([load_bytes(os.path.join(src, f)) for f in names])
    m = back2future.Model(model)
    if stream:
        # output i is what the push of frame i + 2 returns; own_past_flow needs a stream that runs the past-flow decoders
        with m.openStream(frames.shape[2], frames.shape[3], dtype=frames.dtype, warp=True, past=own) as st:
            outs = [st.pushWarp(f, flow_scale=scale, want_warped=images, own_past_flow=own) for f in frames][2:]
        if images:
            warped, photo = (np.concatenate(parts) for parts in zip(*outs))
        else:
            photo = np.concatenate(outs)
    elif images:
        warped, photo = m.computeFlowSequenceWarp(frames, flow_scale=scale, own_past_flow=own)
    else:
        photo = m.computeFlowSequenceWarp(frames, flow_scale=scale, want_warped=False, own_past_flow=own)
    m.close()
    if images:
        os.makedirs(dst, exist_ok=True)
        for i, f in enumerate(names[1:-1]):
            stem = os.path.join(dst, os.path.splitext(f)[0])
            flow_io.save_image(stem + "_past.png", warped[i, 0] / 255.0)
            flow_io.save_image(stem + "_future.png", warped[i, 1] / 255.0)
    for k, v in back2future.photo_summary(photo).items():
        print("%s %r" % (k, v))


if __name__ == "__main__":
    main()
