#!/usr/bin/env python3
"""Flow for every centre frame of a video: a directory of frames (sorted by name) -> one .flo and two occlusion masks per
frame that has a neighbour on both sides.  Every frame is uploaded and run through the feature pyramid once
(Model.computeFlowSequence); output t is computeFlow(frame[t-1], frame[t], frame[t+1]) bit for bit.  The flow comes from the
float32 entry (dtype=np.float32: the float64 flow rounded to float32, which is what a .flo file stores).

Usage: python examples/run_sequence.py DIR OUT/ [model] [--occ-prob]
model: 'Ours-Hard' | 'Ours-Soft-ft-KITTI' | 'Ours-Soft-ft-Sintel' (needs models/RoamingImages_*.t7 in the current
directory, as in the reference) or 'random:soft' / a .t7 / .b2fw path (default 'Ours-Soft-ft-KITTI').
--occ-prob: also write the occlusion probabilities of every centre frame as a 2 x H x W float32 .npy file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from back2future_amd import back2future, flow_io   # noqa: E402

EXTS = (".png", ".jpg", ".jpeg", ".ppm", ".bmp")


def main():
    args = [a for a in sys.argv[1:] if a != "--occ-prob"]
    want_occ = len(args) < len(sys.argv) - 1
    if len(args) < 2:
        sys.exit(__doc__)
    src, out = args[0], args[1]
    model = args[2] if len(args) > 2 else "Ours-Soft-ft-KITTI"
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(EXTS))
    if len(names) < 3:
        sys.exit("%s: need at least 3 frames, found %d" % (src, len(names)))
    frames = np.stack([flow_io.load_image(os.path.join(src, f)) for f in names])
    os.makedirs(out, exist_ok=True)
    m = back2future.Model(model)
    res = m.computeFlowSequence(frames, dtype=np.float32, occ_prob=want_occ)
    flow, fwd_occ, bwd_occ = res[:3]
    for i in range(len(names) - 2):
        stem = os.path.join(out, os.path.splitext(names[i + 1])[0])   # named after the centre frame
        flow_io.writeFLO(stem + ".flo", flow[i])
        flow_io.save_mask(stem + "_fwd_occ.png", fwd_occ[i])
        flow_io.save_mask(stem + "_bwd_occ.png", bwd_occ[i])
        if want_occ:
            np.save(stem + "_occ_prob.npy", res[3][i])
    print("%d frames -> %d flows in %s" % (len(names), len(names) - 2, out))
    m.close()


if __name__ == "__main__":
    main()
