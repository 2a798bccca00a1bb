"""Scene cuts in the sequence path: what the detector costs and that windows stopping at cuts cost nothing.

  kernels      savsr_video_pair_sad_u8 / _i420 / _f32 alone on one stream: HIP events around 50 back-to-back calls over 8 pairs, us per
               pair and the fraction of 8 TB/s of HBM on the 2 * S sample bytes (8 * S for fp32) a pair reads; at the LR size and at
               720 x 1280
  none         upscale_video(uint8 in, uint8 out, cuts=None): frames/s
  auto         the same video (one scene: smooth texture, drifting) with cuts="auto": detector + one D2H of N - 1 integers + planning
  every10      cuts=[10, 20, ...]: the same number of windows, more of them padded
  stream_none / stream_auto    VideoUpscaler in chunks of 16, without cuts / cuts="auto" (one detector call and D2H per push)

Every variant runs in a fresh process (its own warm-up pass, then --reps timed passes, the median reported); the parent runs the list
--rounds times in the same order (A B C .., A B C ..), so the spread between a variant's rounds is the A/A spread of the session.
--tree DIR (repeatable): run `none` from another checkout as well (e.g. the parent commit, built), as `none@DIR`.

    python3 tools/bench_scenes.py [--frames 64 --h 180 --w 320 --scale 4 --reps 3 --rounds 2 --out profiles/bench_scenes.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12
VARIANTS = ("none", "auto", "every10", "stream_none", "stream_auto")


def one_scene(n, h, w, seed=0):
    """n frames [n, h, w, 3] uint8 of one scene: a smooth random texture drifting a pixel per frame (no cut for any sane threshold)."""
    import numpy as np
    rng = np.random.RandomState(seed)
    cell = 16
    g = rng.uniform(0, 255, (h // cell + 2, (w + n) // cell + 2, 3))
    ys, xs = np.arange(h) / cell, np.arange(w + n) / cell
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    tex = (g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx) * (1 - fy) + (g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx) * fy
    return np.stack([np.rint(tex[:, i:i + w]).astype(np.uint8) for i in range(n)], 0)


def time_kernels(h, w, dev, iters=50, n=9):
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import i420_bytes
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = []

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / iters
    for (hh, ww) in ((h, w), (720, 1280)):
        sad = torch.empty(n - 1, dtype=torch.int64, device=dev)
        u8 = torch.randint(0, 256, (n, hh, ww, 3), dtype=torch.uint8, device=dev)
        yv = torch.randint(0, 256, (n, i420_bytes(hh, ww)), dtype=torch.uint8, device=dev)
        fl = torch.rand(n, 3, hh, ww, device=dev)
        calls = (("savsr_video_pair_sad_u8", lambda: lib.savsr_video_pair_sad_u8(u8.data_ptr(), n, 3, hh, ww, sad.data_ptr(), st), 2 * 3 * hh * ww),
                 ("savsr_video_pair_sad_i420", lambda: lib.savsr_video_pair_sad_i420(yv.data_ptr(), n, hh, ww, sad.data_ptr(), st), 2 * hh * ww),
                 ("savsr_video_pair_sad_f32", lambda: lib.savsr_video_pair_sad_f32(fl.data_ptr(), n, 3, hh, ww, sad.data_ptr(), st), 8 * 3 * hh * ww))
        for name, fn, pair_bytes in calls:
            us = timed(lambda: _lib.check(fn(), name))
            rows.append({"kernel": name, "frame": [hh, ww], "pairs": n - 1, "us_per_call": round(us, 2), "us_per_pair": round(us / (n - 1), 3),
                         "pair_mb": round(pair_bytes / 1e6, 3), "hbm_frac": round(pair_bytes * (n - 1) / (us * 1e-6) / HBM_BYTES_PER_S, 3)})
    return rows


def run_variant(a):
    """One variant in this process: a JSON line."""
    sys.path.insert(0, a.root)
    import torch
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    dev = torch.device("cuda:0")
    if a.variant == "kernels":
        print(json.dumps({"variant": "kernels", "kernels": time_kernels(a.h, a.w, dev)}), flush=True)
        return
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    n, sc = a.frames, (a.scale, a.scale)
    u8 = torch.from_numpy(one_scene(n, a.h, a.w)).to(dev)
    found = None

    def stream(**kw):
        from savsr_amd import VideoUpscaler
        up = VideoUpscaler(net, sc, "reflection", out="uint8", **kw)
        parts = [up.push(u8[c0:c0 + 16]) for c0 in range(0, n, 16)] + [up.finish()]
        return parts

    if a.variant == "auto":
        from savsr_amd import detect_cuts
        found = detect_cuts(u8)
    fn = {"none": lambda: net.upscale_video(u8, scale=sc, out="uint8"),
          "auto": lambda: net.upscale_video(u8, scale=sc, out="uint8", cuts="auto"),
          "every10": lambda: net.upscale_video(u8, scale=sc, out="uint8", cuts=list(range(10, n, 10))),
          "stream_none": lambda: stream(),
          "stream_auto": lambda: stream(cuts="auto")}[a.variant]
    ts = []
    with torch.no_grad():
        fn()                                   # warm-up: every (unit size, stream) graph captured
        torch.cuda.synchronize()
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            del r
    res = {"variant": a.variant, "fps": round(n / statistics.median(ts), 2), "fps_all": [round(n / t, 2) for t in ts]}
    if found is not None:
        res["cuts_found"] = found
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--h", type=int, default=180)
    ap.add_argument("--w", type=int, default=320)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tree", action="append", default=[], help="another built checkout to run `none` from (e.g. the parent commit)")
    ap.add_argument("--lease", default="", help="a name for the session the figures were taken in")
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.variant:
        run_variant(a)
        return
    jobs = [("kernels", ROOT)]
    for _ in range(a.rounds):
        for tree in a.tree:
            jobs.append(("none", os.path.abspath(tree)))
        jobs += [(v, ROOT) for v in VARIANTS]
    res = {"workload": f"{a.frames} frames {a.h}x{a.w} x{a.scale:g}, uint8 in and out, one scene", "reps": a.reps, "rounds": a.rounds,
           "lease": a.lease, "runs": {}}
    for variant, root in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--variant", variant, "--root", root, "--frames", str(a.frames), "--h", str(a.h),
               "--w", str(a.w), "--scale", str(a.scale), "--reps", str(a.reps)]
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=420)
        if r.returncode != 0:                  # nothing more is started after a failure
            raise SystemExit(f"{variant} in {root} failed ({r.returncode}): {r.stderr[-2000:]}")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        if variant == "kernels":
            res["kernels"] = line["kernels"]
            continue
        key = variant if root == ROOT else f"none@{os.path.basename(root)}"
        res["runs"].setdefault(key, []).append(line["fps"])
        if "cuts_found" in line:
            res["auto_cuts_found"] = line["cuts_found"]
        print(key, line, flush=True)
    base = statistics.mean(res["runs"]["none"])
    res["aa_spread_none"] = round((max(res["runs"]["none"]) - min(res["runs"]["none"])) / base, 5)
    res["vs_none"] = {k: round(statistics.mean(v) / base, 5) for k, v in res["runs"].items()}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
