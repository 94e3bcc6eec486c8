#!/usr/bin/env python3
"""Flow for every centre frame of a video: a directory of frames (sorted by name) -> one .flo and two occlusion masks per
frame that has a neighbour on both sides.  Every frame is uploaded and run through the feature pyramid once
(Model.computeFlowSequence); output t is computeFlow(frame[t-1], frame[t], frame[t+1]) bit for bit.

Usage: python examples/run_sequence.py DIR OUT/ [model]
model: 'Ours-Hard' | 'Ours-Soft-ft-KITTI' | 'Ours-Soft-ft-Sintel' (needs models/RoamingImages_*.t7 in the current
directory, as in the reference) or 'random:soft' / a .t7 / .b2fw path (default 'Ours-Soft-ft-KITTI').
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from back2future_amd import back2future, flow_io   # noqa: E402

EXTS = (".png", ".jpg", ".jpeg", ".ppm", ".bmp")


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    src, out = sys.argv[1], sys.argv[2]
    model = sys.argv[3] if len(sys.argv) > 3 else "Ours-Soft-ft-KITTI"
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(EXTS))
    if len(names) < 3:
        sys.exit("%s: need at least 3 frames, found %d" % (src, len(names)))
    frames = np.stack([flow_io.load_image(os.path.join(src, f)) for f in names])
    os.makedirs(out, exist_ok=True)
    m = back2future.Model(model)
    flow, fwd_occ, bwd_occ = m.computeFlowSequence(frames)
    for i in range(len(names) - 2):
        stem = os.path.join(out, os.path.splitext(names[i + 1])[0])   # named after the centre frame
        flow_io.writeFLO(stem + ".flo", flow[i].astype("float32"))
        flow_io.save_mask(stem + "_fwd_occ.png", fwd_occ[i])
        flow_io.save_mask(stem + "_bwd_occ.png", bwd_occ[i])
    print("%d frames -> %d flows in %s" % (len(names), len(names) - 2, out))
    m.close()


if __name__ == "__main__":
    main()
