"""Pulldown removal: what savsr_video_field_scores_u8 / _u16 and savsr_video_weave reach beside the scene detector's kernels, and what
upscale_video(pulldown=...) gains on telecined film.

  kernels   7 source frames at 180 x 320 and at 480 x 720 (NTSC), as uint8 RGB, 8-bit I420 and 10-bit I420: the score call (one launch:
            every byte of packed frames, the Y plane of planar ones) and the weave (one launch per plane), beside savsr_video_pair_sad_u8 /
            _i420 / _i420_16 of the same build on the same frames.  One process, interleaved rounds: yardstick, scores, weave, yardstick,
            each a HIP-event pair around --launches back-to-back calls, --rounds times.  GB/s count the bytes HBM must move: a score
            call reads every frame's matrix once plus the second-field rows (half the matrix) of its predecessor; a weave reads the
            source once and writes the output once; a SAD call reads every inner frame twice ((2 n - 2) matrices).  The yardstick is
            read twice per round; the margin is the largest spread of its two readings.
  end2end   telecine of a 24-frame film: 30 video frames of 180 x 320, x4, uint8 in and out.  pulldown="tff" against pulldown=None on
            the same 30 frames and against fields="tff", interleaved, in input frames per second; the network frames each runs; and
            remove_pulldown's own time as a share of the call.

    python3 tools/bench_pulldown.py [--rounds 5 --launches 50 --scale 4 --out profiles/bench_pulldown.json]
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
FILM_FRAMES = 24


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
    from savsr_amd.frames import detector_side, plane_table
    from savsr_amd.yuv import i420_bytes
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    delta = torch.tensor([0, 0, -1, -1, 0, 0, 0], dtype=torch.int32, device=dev)
    for h, w in ((180, 320), (480, 720)):
        sad = torch.empty(n - 1, dtype=torch.int64, device=dev)
        scores = torch.empty(n, 2, dtype=torch.int64, device=dev)
        u8 = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
        y8 = torch.randint(0, 256, (n, i420_bytes(h, w)), dtype=torch.uint8, device=dev)
        y10 = (torch.randint(0, 1024, (n, i420_bytes(h, w)), dtype=torch.int16, device=dev)).view(torch.uint8).reshape(n, -1)
        o8, oy8, oy10 = (torch.empty_like(t) for t in (u8, y8, y10))

        def planar_weave(src, dst, depth):
            fb, _, planes = plane_table(*detector_side("i420", (h, w), depth))

            def call():
                rc = 0
                for p in planes:
                    rc |= lib.savsr_video_weave(src.data_ptr(), n, fb, p.offset, p.rows, p.row_bytes, 0, 0, n, delta.data_ptr(), dst.data_ptr(), fb, p.offset, st)
                return rc
            return call

        fb8, fb10 = i420_bytes(h, w), i420_bytes(h, w, 10)
        cases = (
            ("uint8 RGB", h * w * 3, h * w * 3,
             lambda: lib.savsr_video_field_scores_u8(u8.data_ptr(), n, h * w * 3, 0, h, w * 3, 0, 0, n, scores.data_ptr(), st),
             "savsr_video_weave", lambda: lib.savsr_video_weave(u8.data_ptr(), n, h * w * 3, 0, h, w * 3, 0, 0, n, delta.data_ptr(), o8.data_ptr(), h * w * 3, 0, st),
             "savsr_video_field_scores_u8", "savsr_video_pair_sad_u8", lambda: lib.savsr_video_pair_sad_u8(u8.data_ptr(), n, 3, h, w, sad.data_ptr(), st)),
            ("I420 8-bit", fb8, h * w,
             lambda: lib.savsr_video_field_scores_u8(y8.data_ptr(), n, fb8, 0, h, w, 0, 0, n, scores.data_ptr(), st),
             "savsr_video_weave x3", planar_weave(y8, oy8, 8),
             "savsr_video_field_scores_u8", "savsr_video_pair_sad_i420", lambda: lib.savsr_video_pair_sad_i420(y8.data_ptr(), n, h, w, sad.data_ptr(), st)),
            ("I420 10-bit", fb10, 2 * h * w,
             lambda: lib.savsr_video_field_scores_u16(y10.data_ptr(), n, fb10, 0, h, w, 10, 0, 0, n, scores.data_ptr(), st),
             "savsr_video_weave x3", planar_weave(y10, oy10, 10),
             "savsr_video_field_scores_u16", "savsr_video_pair_sad_i420_16",
             lambda: lib.savsr_video_pair_sad_i420_16(y10.data_ptr(), n, h, w, 10, sad.data_ptr(), st)),
        )
        for kind, frame_b, mat_b, score_fn, weave_name, weave_fn, score_name, old_name, old_fn in cases:
            score_b = n * mat_b + (n - 1) * mat_b // 2          # every matrix once plus the predecessor's second-field rows (frame 0 is its own)
            weave_b, old_b = 2 * n * frame_b, (2 * n - 2) * mat_b
            for name, fn in ((score_name, score_fn), (weave_name, weave_fn), (old_name, old_fn)):          # warm-up, and the return codes once
                _lib.check(fn(), name)
            torch.cuda.synchronize()
            s_gbs, w_gbs, old_gbs, margins = [], [], [], []
            for _ in range(rounds):
                a = old_b / timed(old_fn, launches) / 1e3
                s_gbs.append(score_b / timed(score_fn, launches) / 1e3)
                w_gbs.append(weave_b / timed(weave_fn, launches) / 1e3)
                b = old_b / timed(old_fn, launches) / 1e3
                old_gbs += [a, b]
                margins.append(abs(a - b) / ((a + b) / 2))
            yard = statistics.median(old_gbs)
            for name, moved, gbs in ((score_name, score_b, s_gbs), (weave_name, weave_b, w_gbs)):
                row = {"frames": kind, "size": [h, w], "n": n, "kernel": name, "bytes_moved": moved, "gb_s": round(statistics.median(gbs), 1),
                       "gb_s_rounds": [round(v, 1) for v in gbs], "us_per_call": round(moved / statistics.median(gbs) / 1e3, 2),
                       "yardstick": old_name, "yardstick_bytes_read": old_b, "yardstick_gb_s": round(yard, 1),
                       "yardstick_us_per_call": round(old_b / yard / 1e3, 2), "yardstick_gb_s_readings": [round(v, 1) for v in old_gbs],
                       "margin": round(max(margins), 4)}
                row["vs_yardstick"] = round(row["gb_s"] / row["yardstick_gb_s"], 4)
                out.append(row)
                print(json.dumps(row), flush=True)
    return out


def film(m, h=180, w=320, seed=0):
    """[m, h, w, 3] uint8 film frames: a smooth texture drifting two pixels per frame."""
    import numpy as np
    rng = np.random.RandomState(seed)
    g = rng.uniform(20, 235, (h // 16 + 2, (w + 2 * m) // 16 + 2, 3))
    ys, xs = np.arange(h) / 16, np.arange(w + 2 * m) / 16
    iy, ix = ys.astype(int), xs.astype(int)
    fy, fx = (ys - iy)[:, None, None], (xs - ix)[None, :, None]
    tex = (g[iy][:, ix] * (1 - fx) + g[iy][:, ix + 1] * fx) * (1 - fy) + (g[iy + 1][:, ix] * (1 - fx) + g[iy + 1][:, ix + 1] * fx) * fy
    tex = np.rint(tex).astype(np.uint8)
    return np.stack([tex[:, 2 * k:2 * k + w] for k in range(m)])


def time_end2end(dev, scale, rounds):
    import numpy as np
    import torch
    import savsr_amd
    from savsr_amd import pulldown as pd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    frames = film(FILM_FRAMES)
    video = pd.telecine(frames, "tff")
    n = video.shape[0]
    u8 = torch.from_numpy(video).to(dev)
    recovered, info = savsr_amd.remove_pulldown(u8, "tff", return_info=True)
    exact = bool(np.array_equal(recovered.cpu().numpy(), frames))          # (a smooth texture: the matcher recovers the film itself)
    calls = {"pulldown": lambda: net.upscale_video(u8, scale=scale, out="uint8", pulldown="tff"),
             "plain": lambda: net.upscale_video(u8, scale=scale, out="uint8"),
             "fields": lambda: net.upscale_video(u8, scale=scale, out="uint8", fields="tff"),
             "remove_pulldown": lambda: savsr_amd.remove_pulldown(u8, "tff")}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        del r
        return time.perf_counter() - t0
    assert torch.equal(calls["pulldown"](), net.upscale_video(recovered, scale=scale, out="uint8"))          # warm-up, and the property
    for k in ("plain", "fields", "remove_pulldown"):          # warm-up: every (unit size, stream) graph captured
        wall(calls[k])
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    net_frames = {"pulldown": n - n // 5, "plain": n, "fields": 2 * n}
    res = {"workload": f"telecine of a {FILM_FRAMES}-frame film: {n} video frames 180x320 x{scale:g}, uint8 in and out",
           "film_recovered_exactly": exact, "matched_from_predecessor": info["matches"].count(-1), "network_frames": net_frames,
           "input_fps": {k: round(n / med[k], 3) for k in net_frames},
           "input_fps_rounds": {k: [round(n / v, 3) for v in t[k]] for k in net_frames},
           "pulldown_vs_plain": round(med["plain"] / med["pulldown"], 4), "pulldown_vs_fields": round(med["fields"] / med["pulldown"], 4),
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in net_frames},
           "remove_pulldown_ms": round(1e3 * med["remove_pulldown"], 3), "remove_pulldown_share_of_call": round(med["remove_pulldown"] / med["pulldown"], 5)}
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
    res = {"rounds": a.rounds, "launches": a.launches}
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
