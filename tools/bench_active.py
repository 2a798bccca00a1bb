"""The active-picture path: what the line-sum kernels reach beside the scene detector's, and what cropping the bars saves end to end.

  kernels   savsr_video_line_sums_u8 (packed RGB and the Y plane of 8-bit I420) and savsr_video_line_sums_u16 (10-bit I420) beside the
            existing savsr_video_pair_sad_u8 / _i420 / _i420_16 on the same 7 frames, at 720 x 1280 and at 180 x 320.  One process,
            interleaved rounds: yardstick, new kernel, yardstick, each a HIP-event pair around --launches back-to-back calls, --rounds
            times.  GB/s of bytes read: a line-sum call reads every frame's matrix once, a SAD call every inner frame twice
            ((2 n - 2) matrices).  The yardstick is read twice per round; the spread of its two readings is the margin.
  end2end   upscale_video on --frames uint8 frames of 180 x 320 whose picture is rows 22 .. 157 (136 rows, 2.39:1 in 16:9), uint8 out:
            crop=None against crop="auto", bars="keep", in frames per second, interleaved; detect_active_area's own time (with its
            device -> host copy) as a share of the cropped call.  The pixel ratio predicts 180 / 136 = 1.32.

    python3 tools/bench_active.py [--rounds 5 --launches 50 --frames 16 --scale 4 --out profiles/bench_active.json]
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
PICTURE = (22, 0, 136, 320)


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
    from savsr_amd.yuv import i420_bytes
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    for h, w in ((720, 1280), (180, 320)):
        sad = torch.empty(n - 1, dtype=torch.int64, device=dev)
        cells = torch.empty(n * (h + w * 3), dtype=torch.int32, device=dev)          # rows then columns, as savsr_amd.line_sums lays them out
        u8 = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
        y8 = torch.randint(0, 256, (n, i420_bytes(h, w)), dtype=torch.uint8, device=dev)
        y10 = torch.randint(0, 256, (n, i420_bytes(h, w, 10)), dtype=torch.uint8, device=dev)
        p = (cells.data_ptr(), cells.data_ptr() + 4 * n * h, st)
        cases = (
            ("uint8 RGB", h * w * 3, "savsr_video_line_sums_u8", lambda: lib.savsr_video_line_sums_u8(u8.data_ptr(), n, h * w * 3, h, w * 3, *p),
             "savsr_video_pair_sad_u8", lambda: lib.savsr_video_pair_sad_u8(u8.data_ptr(), n, 3, h, w, sad.data_ptr(), st)),
            ("I420 8-bit", h * w, "savsr_video_line_sums_u8", lambda: lib.savsr_video_line_sums_u8(y8.data_ptr(), n, i420_bytes(h, w), h, w, *p),
             "savsr_video_pair_sad_i420", lambda: lib.savsr_video_pair_sad_i420(y8.data_ptr(), n, h, w, sad.data_ptr(), st)),
            ("I420 10-bit", 2 * h * w, "savsr_video_line_sums_u16",
             lambda: lib.savsr_video_line_sums_u16(y10.data_ptr(), n, i420_bytes(h, w, 10), h, w, 10, *p),
             "savsr_video_pair_sad_i420_16", lambda: lib.savsr_video_pair_sad_i420_16(y10.data_ptr(), n, h, w, 10, sad.data_ptr(), st)),
        )
        for kind, mat_bytes, new_name, new_fn, old_name, old_fn in cases:
            new_b, old_b = n * mat_bytes, (2 * n - 2) * mat_bytes
            for name, fn in ((new_name, new_fn), (old_name, old_fn)):          # warm-up, and the return codes once
                _lib.check(fn(), name)
            torch.cuda.synchronize()
            new_gbs, old_gbs, margins = [], [], []
            for _ in range(rounds):
                a = old_b / timed(old_fn, launches) / 1e3
                x = new_b / timed(new_fn, launches) / 1e3
                b = old_b / timed(old_fn, launches) / 1e3
                new_gbs.append(x)
                old_gbs += [a, b]
                margins.append(abs(a - b) / ((a + b) / 2))
            row = {"frames": kind, "size": [h, w], "n": n, "kernel": new_name, "bytes_read": new_b, "gb_s": round(statistics.median(new_gbs), 1),
                   "gb_s_rounds": [round(v, 1) for v in new_gbs], "us_per_call": round(new_b / statistics.median(new_gbs) / 1e3, 2),
                   "yardstick": old_name, "yardstick_bytes_read": old_b, "yardstick_gb_s": round(statistics.median(old_gbs), 1),
                   "yardstick_gb_s_readings": [round(v, 1) for v in old_gbs], "margin": round(max(margins), 4)}
            row["vs_yardstick"] = round(row["gb_s"] / row["yardstick_gb_s"], 4)
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def letterboxed(n, seed=0):
    """[n, 180, 320, 3] uint8: a smooth drifting texture in rows 22 .. 157, bars of 16 +- 2 around it."""
    import numpy as np
    rng = np.random.RandomState(seed)
    y0, _, ah, w = PICTURE
    v = rng.randint(14, 19, size=(n, 180, 320, 3)).astype(np.uint8)
    g = rng.uniform(40, 255, (ah // 16 + 2, (w + n) // 16 + 2, 3))
    ys, xs = np.arange(ah) / 16, np.arange(w + n) / 16
    iy, ix = ys.astype(int), xs.astype(int)
    fy, fx = (ys - iy)[:, None, None], (xs - ix)[None, :, None]
    tex = (g[iy][:, ix] * (1 - fx) + g[iy][:, ix + 1] * fx) * (1 - fy) + (g[iy + 1][:, ix] * (1 - fx) + g[iy + 1][:, ix + 1] * fx) * fy
    for i in range(n):
        v[i, y0:y0 + ah] = np.rint(tex[:, i:i + w]).astype(np.uint8)
    return v


def time_end2end(dev, frames, scale, rounds):
    import torch
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    u8 = torch.from_numpy(letterboxed(frames)).to(dev)
    rect = savsr_amd.detect_active_area(u8)
    calls = {"none": lambda: net.upscale_video(u8, scale=scale, out="uint8"),
             "auto_keep": lambda: net.upscale_video(u8, scale=scale, out="uint8", crop="auto", bars="keep"),
             "detect": lambda: savsr_amd.detect_active_area(u8)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        del r
        return time.perf_counter() - t0
    for fn in calls.values():          # warm-up: every (unit size, stream) graph captured
        wall(fn)
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"{frames} frames 180x320 x{scale:g}, uint8 in and out, picture rows 22 .. 157", "rect_found": list(rect),
           "fps_none": round(frames / med["none"], 3), "fps_auto_keep": round(frames / med["auto_keep"], 3),
           "fps_none_rounds": [round(frames / v, 3) for v in t["none"]], "fps_auto_keep_rounds": [round(frames / v, 3) for v in t["auto_keep"]],
           "speedup": round(med["none"] / med["auto_keep"], 4), "pixel_ratio": round(180 / PICTURE[2], 4),
           "detect_ms": round(1e3 * med["detect"], 3), "detect_share_of_call": round(med["detect"] / med["auto_keep"], 5)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--only", default="kernels,end2end")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds, "launches": a.launches}
    with torch.no_grad():
        if "kernels" in a.only:
            res["kernels"] = time_kernels(dev, a.rounds, a.launches)
        if "end2end" in a.only:
            res["end2end"] = time_end2end(dev, a.frames, a.scale, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
