#!/usr/bin/env python3
"""Flow for every centre frame of a video: a directory of frames (sorted by name) -> one .flo and two occlusion masks per
frame that has a neighbour on both sides.  Every frame is uploaded and run through the feature pyramid once
(Model.computeFlowSequence); output t is computeFlow(frame[t-1], frame[t], frame[t+1]) bit for bit.  The flow comes from the
float32 entry (dtype=np.float32: the float64 flow rounded to float32, which is what a .flo file stores).

Usage: python examples/run_sequence.py DIR OUT/ [model] [--occ-prob] [--past-flow] [--rgb [MAX]] [--flo] [--stream]
model: 'Ours-Hard' | 'Ours-Soft-ft-KITTI' | 'Ours-Soft-ft-Sintel' (needs models/RoamingImages_*.t7 in the current
directory, as in the reference) or 'random:soft' / a .t7 / .b2fw path (default 'Ours-Soft-ft-KITTI').
--occ-prob: also write the occlusion probabilities of every centre frame as a 2 x H x W float32 .npy file.
--past-flow: also write the past flow of every centre frame as NAME_past.flo (Soft models only: Model.computeFlowSequencePast; the
past frame lies at x - past_flow, as the future frame lies at x + flow).
--rgb [MAX]: write the flow picture of every centre frame (flowX.xy2rgb, coloured on the GPU: Model.computeFlowSequenceRGB) as
a PNG instead; MAX is xy2rgb's `max` (default: every picture's own largest flow).  Only the pictures are downloaded; --flo
writes the .flo files and masks as well.
--stream: push the frames one at a time (Model.openStream / FlowStream.push, the calling pattern of a camera) instead of handing
over the clip; the files are the same, byte for byte.  With --past-flow the stream is opened for the past flow
(Model.openStream(past=True) / MotionStream.pushPast).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from back2future_amd import back2future, flow_io   # noqa: E402

EXTS = (".png", ".jpg", ".jpeg", ".ppm", ".bmp")


def main():
    args = list(sys.argv[1:])
    want_occ, want_flo, want_rgb, rgb_max = "--occ-prob" in args, "--flo" in args, "--rgb" in args, None
    stream = "--stream" in args
    want_past = "--past-flow" in args
    if want_past and want_rgb:
        sys.exit("--past-flow cannot be combined with --rgb")
    if want_rgb:
        i = args.index("--rgb")
        try:
            rgb_max = float(args[i + 1])
            del args[i + 1]
        except (IndexError, ValueError):
            pass
        if rgb_max is not None and not rgb_max > 0:
            sys.exit("--rgb MAX: MAX must be positive")
        if want_occ:
            sys.exit("--rgb and --occ-prob cannot be combined")
    args = [a for a in args if a not in ("--occ-prob", "--flo", "--rgb", "--stream", "--past-flow")]
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

    def pushed(push):
        """The sequence call's results from a stream: output i is what the push of frame i + 2 returns."""
        with m.openStream(frames.shape[2], frames.shape[3], dtype=frames.dtype, past=want_past) as st:
            outs = [push(st, f) for f in frames][2:]
        return tuple(np.concatenate(parts) for parts in zip(*outs))

    if want_rgb:
        from PIL import Image
        if stream:
            res = pushed(lambda st, f: st.pushRGB(f, max=rgb_max, packed=True, want_flow=want_flo, want_masks=want_flo))
        else:
            res = m.computeFlowSequenceRGB(frames, max=rgb_max, packed=True, want_flow=want_flo, want_masks=want_flo)
        for i in range(len(names) - 2):
            stem = os.path.join(out, os.path.splitext(names[i + 1])[0])
            Image.fromarray(res[0][i]).save(stem + "_flow.png")
            if want_flo:
                flow_io.writeFLO(stem + ".flo", res[2][i])
                flow_io.save_mask(stem + "_fwd_occ.png", res[3][i])
                flow_io.save_mask(stem + "_bwd_occ.png", res[4][i])
        print("%d frames -> %d flow pictures in %s" % (len(names), len(names) - 2, out))
        m.close()
        return
    past = None
    if want_past:
        if stream:
            res = pushed(lambda st, f: st.pushPast(f, occ_prob=want_occ))
        else:
            res = m.computeFlowSequencePast(frames, occ_prob=want_occ)
        past, res = res[1], res[:1] + res[2:]
    elif stream:
        res = pushed(lambda st, f: st.push(f, occ_prob=want_occ))
    else:
        res = m.computeFlowSequence(frames, dtype=np.float32, occ_prob=want_occ)
    flow, fwd_occ, bwd_occ = res[:3]
    for i in range(len(names) - 2):
        stem = os.path.join(out, os.path.splitext(names[i + 1])[0])   # named after the centre frame
        flow_io.writeFLO(stem + ".flo", flow[i])
        if past is not None:
            flow_io.writeFLO(stem + "_past.flo", past[i])
        flow_io.save_mask(stem + "_fwd_occ.png", fwd_occ[i])
        flow_io.save_mask(stem + "_bwd_occ.png", bwd_occ[i])
        if want_occ:
            np.save(stem + "_occ_prob.npy", res[3][i])
    print("%d frames -> %d flows in %s" % (len(names), len(names) - 2, out))
    m.close()


if __name__ == "__main__":
    main()
