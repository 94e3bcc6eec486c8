"""Latency of one new frame: a stream push against today's per-frame calls (GPU box only).

    python tools/stream_rate.py [--height 1024] [--width 1920] [--pushes 20] [--out profiles/r09_stream_rate.json]
                                [--parent-root DIR]

One run at 1024 x 1920, random Hard weights, byte frames, library defaults (use_graph = 1 for the device rows, as in
tools/sequence_rate.py).  Every row is the median of `--pushes` steady-state calls with the min and max, in ms per new frame:
  a  computeFlowDevice with n = 1 per new frame (three device frames per call): today's way
  b  pushDevice, default (map-size) kernel rule
  c  pushDevice with adaptive_kernels = 1 (per-launch rule)
  d  host computeFlowBatch(dtype=np.float32) with n = 1 from bytes
  e  host push, pageable buffers
  f  host push, page-locked buffers
  g  pushRGB(packed=True), pageable
  h  cams = 4, pushDevice, per camera-frame
  i  host push(occ_prob=True), pageable: what (j) is held against
  j  pushWarp(want_warped=False) on a stream opened with warp=True, pageable: 112 bytes down instead of 10 B/px, one kernel more
  k  pushWarp with warped frames and photo, pageable
  l  host computeFlowBatchWarp with n = 1 per new frame (three uploads, three pyramids): today's way to (k)'s outputs
plus the profile_layers = 1 split of one push into the pyramid and the rest, the flow_warp profile row of a push and of a
three-frame sequence (one image each) against 31 B/px at the copy rate of DESIGN.md section 7.6, and the conditions of DESIGN.md
sections 7.4 and 7.15.
--parent-root DIR: a built checkout of the parent commit; rows (a), (b) and (e) are measured there too, by this tool in a process
of its own (--only-plain --root DIR), to show that the triplet path and the plain pushes did not move.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

# --root DIR: import the package from another checkout (the parent commit's, for row (a))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from back2future_amd import back2future
from tools.sequence_rate import clip


def row(ms, per=1):
    ms = [v / per for v in ms]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def timed(m, call, n, warm=6, device=True):
    """ms of each of n calls after `warm` (ring phases x eager / capture / replay)."""
    for i in range(warm):
        call(i)
    m.synchronize()
    out = []
    for i in range(n):
        t0 = time.perf_counter()
        call(warm + i)
        if device:
            m.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--only-a", action="store_true", help="row (a) alone: the call a parent commit can run")
    ap.add_argument("--only-plain", action="store_true", help="rows (a), (b) and (e): the triplet call and the plain pushes of a parent commit")
    a = ap.parse_args()
    H, W, N = a.height, a.width, a.pushes
    T = 12
    m = back2future.Model("random:hard:2:1.0")
    V = clip(T, H, W, seed=2)
    Vn = V.numpy()
    d = V.cuda()
    flow = torch.empty(4, 2, H, W, device="cuda")
    fo = torch.empty(4, 1, H, W, dtype=torch.uint8, device="cuda")
    bo = torch.empty_like(fo)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    res = {"metric": "ms per new frame", "H": H, "W": W, "model": "random:hard:2:1.0", "frames": "uint8", "pushes": N, "rows": {}}
    R = res["rows"]
    with m.options(use_graph=1):
        R["a"] = row(timed(m, lambda i: m.computeFlowDevice(p(d[i % 10]), p(d[i % 10 + 1]), p(d[i % 10 + 2]), 1, H, W, p(flow), None, p(fo), p(bo),
                                                            in_kind=back2future.IN_U8), N))
        R["a"]["path"] = "computeFlowDevice n=1, three u8 device frames, use_graph=1"
    if a.only_a:
        print(json.dumps(res))
        m.close()
        return
    out1 = (np.empty((1, 2, H, W), np.float32), np.empty((1, 1, H, W), np.uint8), np.empty((1, 1, H, W), np.uint8))
    if a.only_plain:
        with m.options(use_graph=1), m.openStream(H, W) as st:
            R["b"] = row(timed(m, lambda i: st.pushDevice(p(d[i % T]), p(flow), None, p(fo), p(bo)), N, warm=9))
        with m.openStream(H, W) as st:
            R["e"] = row(timed(m, lambda i: st.push(Vn[i % T], out=out1), N, warm=9, device=False))
        print(json.dumps(res))
        m.close()
        return
    with m.options(use_graph=1):
        for key, opts in (("b", {}), ("c", {"adaptive_kernels": 1})):
            with m.options(**opts), m.openStream(H, W) as st:
                R[key] = row(timed(m, lambda i: st.pushDevice(p(d[i % T]), p(flow), None, p(fo), p(bo)), N, warm=9))
        R["b"]["path"] = "pushDevice, default rule, use_graph=1"
        R["c"]["path"] = "pushDevice, adaptive_kernels=1, use_graph=1"
        d4 = torch.stack([d, d.flip(0), d.roll(3, 0), d.roll(5, 0)], dim=1).contiguous()   # T x 4 x 3 x H x W
        with m.openStream(H, W, cams=4) as st:
            R["h"] = row(timed(m, lambda i: st.pushDevice(p(d4[i % T]), p(flow), None, p(fo), p(bo)), N, warm=9), per=4)
        R["h"]["path"] = "pushDevice cams=4, per camera-frame, use_graph=1"
    R["d"] = row(timed(m, lambda i: m.computeFlowBatch(Vn[i % 10:i % 10 + 1], Vn[i % 10 + 1:i % 10 + 2], Vn[i % 10 + 2:i % 10 + 3], out=out1,
                                                       dtype=np.float32), N, device=False))
    R["d"]["path"] = "computeFlowBatch(dtype=float32) n=1, u8 host frames, pageable"
    with m.openStream(H, W) as st:
        R["e"] = row(timed(m, lambda i: st.push(Vn[i % T], out=out1), N, warm=9, device=False))
    R["e"]["path"] = "push, pageable host buffers"
    pin_in = V.pin_memory()
    pin_out = (torch.empty((1, 2, H, W)).pin_memory(), torch.empty((1, 1, H, W), dtype=torch.uint8).pin_memory(),
               torch.empty((1, 1, H, W), dtype=torch.uint8).pin_memory())
    pin_np = tuple(t.numpy() for t in pin_out)
    with m.openStream(H, W) as st:
        R["f"] = row(timed(m, lambda i: st.push(pin_in[i % T].numpy(), out=pin_np), N, warm=9, device=False))
    R["f"]["path"] = "push, page-locked host buffers"
    rgb_out = (np.empty((1, H, W, 3), np.uint8), np.empty((1,), np.float64))
    with m.openStream(H, W) as st:
        R["g"] = row(timed(m, lambda i: st.pushRGB(Vn[i % T], packed=True, out=rgb_out), N, warm=9, device=False))
    R["g"]["path"] = "pushRGB(packed=True), pageable"
    # ---- motion compensation per pushed frame
    out_prob = out1 + (np.empty((1, 2, H, W), np.float32),)
    with m.openStream(H, W) as st:
        R["i"] = row(timed(m, lambda i: st.push(Vn[i % T], out=out_prob, occ_prob=True), N, warm=9, device=False))
    R["i"]["path"] = "push(occ_prob=True), pageable"
    photo1, warped1 = np.empty((1, back2future.PHOTO_WORDS), np.uint64), np.empty((1, 2, 3, H, W), np.uint8)
    with m.openStream(H, W, warp=True) as st:
        R["j"] = row(timed(m, lambda i: st.pushWarp(Vn[i % T], want_warped=False, out=photo1), N, warm=9, device=False))
    R["j"]["path"] = "pushWarp(want_warped=False), pageable"
    with m.openStream(H, W, warp=True) as st:
        R["k"] = row(timed(m, lambda i: st.pushWarp(Vn[i % T], out=(warped1, photo1)), N, warm=9, device=False))
    R["k"]["path"] = "pushWarp, warped frames + photo, pageable"
    R["l"] = row(timed(m, lambda i: m.computeFlowBatchWarp(Vn[i % 10:i % 10 + 1], Vn[i % 10 + 1:i % 10 + 2], Vn[i % 10 + 2:i % 10 + 3],
                                                           out=(warped1, photo1)), N, device=False))
    R["l"]["path"] = "computeFlowBatchWarp n=1, warped frames + photo, u8 host frames, pageable"
    # the stage alone: the flow_warp profile row of one push and of a three-frame sequence (one image each), against 31 B/px
    with m.options(profile=1):
        with m.openStream(H, W, warp=True) as st:
            for k in range(3):
                st.pushWarp(Vn[k], out=(warped1, photo1))
            m.profile_reset()
            for k in range(3, 8):
                st.pushWarp(Vn[k], out=(warped1, photo1))
            push_ms, push_n = m.profile_read()["flow_warp"]
        m.computeFlowSequenceWarp(Vn[:3], out=(warped1, photo1))
        m.profile_reset()
        for k in range(5):
            m.computeFlowSequenceWarp(Vn[k:k + 3], out=(warped1, photo1))
        seq_ms, seq_n = m.profile_read()["flow_warp"]
        m.profile_reset()
    copy_tb_s, bpp = 6.29, 31   # tools/warp_rate.py: the copy rate and the compulsory bytes per pixel of DESIGN.md section 7.6
    stage = lambda ms, n: {"ms": round(ms / n, 4), "launches": n, "TB_per_s": round(H * W * bpp / (ms / n * 1e-3) / 1e12, 3),
                           "share_of_hbm_copy_rate": round(H * W * bpp / (ms / n * 1e-3) / 1e12 / copy_tb_s, 3)}
    res["flow_warp_stage"] = {"push": stage(push_ms, push_n), "sequence_of_3_frames": stage(seq_ms, seq_n), "bytes_per_px": bpp,
                              "hbm_copy_TB_per_s": copy_tb_s}
    # one push split into pyramid and rest
    with m.options(profile=1, profile_layers=1), m.openStream(H, W) as st:
        for k in range(3):
            st.pushDevice(p(d[k]), p(flow), None, p(fo), p(bo))
        m.synchronize()
        m.profile_reset()
        st.pushDevice(p(d[3]), p(flow), None, p(fo), p(bo))
        m.synchronize()
        rows = {k: v[0] for k, v in m.profile_read().items()}
        m.profile_reset()
        # the first push after a reset runs the pyramid alone
        st.reset()
        st.pushDevice(p(d[4]), p(flow), None, p(fo), p(bo))
        m.synchronize()
        pyr_rows = {k: v[0] for k, v in m.profile_read().items()}
        m.profile_reset()
    pyr = sum(pyr_rows.values())
    res["push_split_ms"] = {"pyramid": round(pyr, 4), "rest": round(sum(rows.values()) - pyr, 4),
                            "pyramid_rows": {k: round(v, 4) for k, v in sorted(pyr_rows.items(), key=lambda kv: -kv[1])},
                            "rows": {k: round(v, 4) for k, v in sorted(rows.items(), key=lambda kv: -kv[1])}}
    best = min(R["b"]["median_ms"], R["c"]["median_ms"])
    res["conditions"] = {
        "best_of_b_c_no_slower_than_a": {"best_ms": best, "a_ms": R["a"]["median_ms"], "margin_ms": round(R["a"]["max_ms"] - R["a"]["min_ms"], 4),
                                         "holds": best <= R["a"]["median_ms"] + (R["a"]["max_ms"] - R["a"]["min_ms"])},
        "e_no_slower_than_d": {"e_ms": R["e"]["median_ms"], "d_ms": R["d"]["median_ms"], "margin_ms": round(R["d"]["max_ms"] - R["d"]["min_ms"], 4),
                               "holds": R["e"]["median_ms"] <= R["d"]["median_ms"] + (R["d"]["max_ms"] - R["d"]["min_ms"])},
        "b_vs_a": round(R["a"]["median_ms"] / R["b"]["median_ms"], 4),
        "j_no_slower_than_i": {"j_ms": R["j"]["median_ms"], "i_ms": R["i"]["median_ms"], "margin_ms": round(R["i"]["max_ms"] - R["i"]["min_ms"], 4),
                               "holds": R["j"]["median_ms"] <= R["i"]["median_ms"] + (R["i"]["max_ms"] - R["i"]["min_ms"])},
        "l_vs_k": round(R["l"]["median_ms"] / R["k"]["median_ms"], 4),
    }
    m.close()
    if a.parent_root:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-plain", "--root", a.parent_root, "--height", str(H), "--width", str(W),
                            "--pushes", str(N)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit("rows (a), (b), (e) on the parent checkout failed:\n" + r.stdout + r.stderr)
        parent = json.loads(r.stdout.strip().splitlines()[-1])["rows"]
        res["a_on_parent_commit"] = parent["a"]
        res["plain_on_parent_commit"] = {k: parent[k] for k in ("b", "e")}
        # a plain push does not move: this commit's median within the parent row's own min-max spread of the parent's median
        res["conditions"]["plain_push_did_not_move"] = {
            k: {"ms": R[k]["median_ms"], "parent_ms": parent[k]["median_ms"], "margin_ms": round(parent[k]["max_ms"] - parent[k]["min_ms"], 4),
                "holds": R[k]["median_ms"] <= parent[k]["median_ms"] + (parent[k]["max_ms"] - parent[k]["min_ms"])} for k in ("b", "e")}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
