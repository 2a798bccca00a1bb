"""Scan detection: what savsr_video_field_stats_u8 / _u16 reach beside the kernels of the same shape, and what upscale_video(scan="detect")
costs over the call with the explicit argument.

  kernels   7 frames of 720 x 1280 I420 at 8 and at 10 bits (the Y plane): savsr_video_field_stats_* beside savsr_video_field_scores_* (the
            yardstick: the same lane layout with four 16-byte loads per lane where the new kernel has five) and savsr_video_pair_sad_yuvp
            of the same build on the same frames.  One process, interleaved rounds: field_scores, field_stats, pair_sad, field_scores,
            each a HIP-event pair around --launches back-to-back calls (every call includes its hipMemsetAsync), --rounds times after one
            warm-up call each.  The yardstick is read twice per round; the margin is the largest spread of its two readings.
            `lane_bytes_ratio` is what the loads alone predict: field_stats has a lane for every row and five loads per lane,
            field_scores a lane for every second row and four loads: (rows x 5) / ((rows - 2) / 2 x 4).
  end2end   an interlaced (tff) video of 12 frames of 120 x 180, x4, uint8 in and out: scan="detect" against fields="tff" on the same
            frames, interleaved, in wall time per call; and detect_scan's own time (the kernel, the copy of 8 N integers, the decision).

    python3 tools/bench_scan.py [--rounds 5 --launches 50 --scale 4 --out profiles/bench_scan.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_FRAMES = 7
SIZE = (720, 1280)


def timed(fn, launches):
    """Microseconds per call of `launches` back-to-back calls on the current stream (HIP events)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def time_kernels(dev, rounds, launches):
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import CHROMAS, i420_bytes
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, (h, w), out = N_FRAMES, SIZE, []
    stats = torch.empty(n, 8, dtype=torch.int64, device=dev)
    scores = torch.empty(n, 2, dtype=torch.int64, device=dev)
    sad = torch.empty(n - 1, dtype=torch.int64, device=dev)
    y8 = torch.randint(0, 256, (n, i420_bytes(h, w)), dtype=torch.uint8, device=dev)
    y10 = torch.randint(0, 1024, (n, i420_bytes(h, w)), dtype=torch.int16, device=dev).view(torch.uint8).reshape(n, -1)
    fb8, fb10, c420 = i420_bytes(h, w), i420_bytes(h, w, 10), CHROMAS.index("420")
    cases = (
        ("I420 8-bit", 8, h * w,
         "savsr_video_field_stats_u8", lambda: lib.savsr_video_field_stats_u8(y8.data_ptr(), n, fb8, 0, h, w, 0, n, stats.data_ptr(), st),
         "savsr_video_field_scores_u8", lambda: lib.savsr_video_field_scores_u8(y8.data_ptr(), n, fb8, 0, h, w, 0, 0, n, scores.data_ptr(), st),
         lambda: lib.savsr_video_pair_sad_yuvp(y8.data_ptr(), n, h, w, 8, c420, sad.data_ptr(), st)),
        ("I420 10-bit", 10, 2 * h * w,
         "savsr_video_field_stats_u16", lambda: lib.savsr_video_field_stats_u16(y10.data_ptr(), n, fb10, 0, h, w, 10, 0, n, stats.data_ptr(), st),
         "savsr_video_field_scores_u16", lambda: lib.savsr_video_field_scores_u16(y10.data_ptr(), n, fb10, 0, h, w, 10, 0, 0, n, scores.data_ptr(), st),
         lambda: lib.savsr_video_pair_sad_yuvp(y10.data_ptr(), n, h, w, 10, c420, sad.data_ptr(), st)),
    )
    for kind, depth, mat_b, stats_name, stats_fn, scores_name, scores_fn, sad_fn in cases:
        for name, fn in ((stats_name, stats_fn), (scores_name, scores_fn), ("savsr_video_pair_sad_yuvp", sad_fn)):          # warm-up, and the return codes once
            _lib.check(fn(), name)
        torch.cuda.synchronize()
        t_stats, t_scores, t_sad, margins = [], [], [], []
        for _ in range(rounds):
            a = timed(scores_fn, launches)
            t_stats.append(timed(stats_fn, launches))
            t_sad.append(timed(sad_fn, launches))
            b = timed(scores_fn, launches)
            t_scores += [a, b]
            margins.append(abs(a - b) / ((a + b) / 2))
        us_stats, us_scores, us_sad = (statistics.median(t) for t in (t_stats, t_scores, t_sad))
        row = {"frames": kind, "size": [h, w], "n": n, "matrix_bytes": mat_b, "kernel": stats_name, "us_per_call": round(us_stats, 2),
               "us_per_call_rounds": [round(v, 2) for v in t_stats], "matrix_gb_s": round(n * mat_b / us_stats / 1e3, 1),
               "yardstick": scores_name, "yardstick_us_per_call": round(us_scores, 2), "yardstick_us_readings": [round(v, 2) for v in t_scores],
               "margin": round(max(margins), 4), "vs_yardstick_time": round(us_stats / us_scores, 4),
               "lane_bytes_ratio": round((h * 5) / ((h - 2) / 2 * 4), 4),
               "pair_sad": "savsr_video_pair_sad_yuvp", "pair_sad_us_per_call": round(us_sad, 2), "vs_pair_sad_time": round(us_stats / us_sad, 4)}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def interlaced(n, h, w, seed=0):
    """[n, h, w, 3] uint8: a smooth picture moving (2, 1) samples per field, consecutive field pictures woven top field first."""
    import numpy as np
    t, y, x = np.mgrid[0:2 * n, 0:h, 0:w * 3].astype(np.float64)
    v = np.full(t.shape, 128.0)
    for amp, fx, fy, ph in ((50.0, 0.013, 0.031, 0.3), (34.0, -0.009, 0.058, 1.1), (22.0, 0.027, -0.017, 2.0)):
        v += amp * np.sin(2 * np.pi * (fx * (x - 6 * t) + fy * (y - t)) + ph)
    v = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    frames = v[0::2].copy()
    frames[:, 1::2] = v[1::2][:, 1::2]
    return frames.reshape(n, h, w, 3)


def time_end2end(dev, scale, rounds):
    import torch
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    n, h, w = 12, 120, 180
    u8 = torch.from_numpy(interlaced(n, h, w)).to(dev)
    verdict = savsr_amd.detect_scan(u8)
    calls = {"detect": lambda: net.upscale_video(u8, scale=scale, out="uint8", scan="detect"),
             "explicit": lambda: net.upscale_video(u8, scale=scale, out="uint8", fields="tff"),
             "detect_scan": lambda: savsr_amd.detect_scan(u8)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        del r
        return time.perf_counter() - t0
    same = bool(torch.equal(calls["detect"](), calls["explicit"]()))          # warm-up, and the property
    wall(calls["detect_scan"])
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"interlaced tff video: {n} frames {h}x{w} x{scale:g}, uint8 in and out ({2 * n} network frames)",
           "verdict": [verdict.scan, verdict.order], "detect_equals_explicit": same,
           "ms_per_call": {k: round(1e3 * med[k], 3) for k in calls}, "ms_per_call_rounds": {k: [round(1e3 * v, 3) for v in t[k]] for k in calls},
           "detect_vs_explicit_time": round(med["detect"] / med["explicit"], 4),
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in calls},
           "detect_scan_share_of_call": round(med["detect_scan"] / med["detect"], 5)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--only", default="kernels,end2end")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds, "launches": a.launches, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if "kernels" in a.only:
            res["kernels"] = time_kernels(dev, a.rounds, a.launches)
        if "end2end" in a.only:
            res["end2end"] = time_end2end(dev, a.scale, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
