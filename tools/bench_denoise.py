"""denoise=: what savsr_video_denoise_u8 costs beside the kernels it stands next to, and what upscale_video(denoise="ata") adds.

  kernels   16 frames of 576 x 720 and of 720 x 1280 I420 (walks of tests/denoise_cases.py's kind: most samples keep their taps, some
            jump), every plane one call: the denoiser at radius 1 / 4 / 16 with strength (4, 9), beside savsr_video_deinterlace_u8_m at
            the same rate (bwdif) and savsr_video_pair_sad_yuvp on the same frames.  One process, interleaved rounds, each reading a
            HIP-event pair around --launches back-to-back passes over the planes, --rounds times; medians and the rounds.  GB/s count
            the bytes HBM must move: the denoiser and the deinterlacer read every frame once and write it once (their other reads
            are re-reads of lines other output frames load as well); the pair SAD reads the Y plane once.
  end2end   24 noisy frames of 180 x 320, x4, uint8 in and out: upscale_video with and without denoise="ata", interleaved A / B / A / B in
            one process, in frames per second, and denoise_video's own time.

Numbers are recorded, not gated.

    python3 tools/bench_denoise.py [--rounds 5 --launches 50 --scale 4 --lease "..." --out profiles/bench_denoise.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_FRAMES = 16
E2E_FRAMES = 24
RADII = (1, 4, 16)


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


def noisy(n, rows, cols, seed):
    """[n, rows, cols] uint8: a random walk per sample (steps of up to +-3 with probability 0.6, a jump of up to +-20 with 0.08)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    m = np.empty((n, rows, cols), dtype=np.int16)
    m[0] = rng.integers(0, 256, (rows, cols))
    for t in range(1, n):
        step = rng.integers(-3, 4, (rows, cols), dtype=np.int16) * (rng.random((rows, cols), dtype=np.float32) < 0.6)
        jump = rng.integers(-20, 21, (rows, cols), dtype=np.int16) * (rng.random((rows, cols), dtype=np.float32) < 0.08)
        m[t] = np.clip(m[t - 1] + step + jump, 0, 255)
    return m.astype(np.uint8)


def time_kernels(dev, rounds, launches):
    import numpy as np
    import torch
    from savsr_amd import _lib
    from savsr_amd.denoise import denoise_matrix
    from savsr_amd.frames import detector_side, plane_table
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    for h, w in ((576, 720), (720, 1280)):
        side, size = detector_side("i420", (h, w), 8)
        tab = plane_table(side, size)
        fb = tab.stride
        host = np.concatenate([noisy(n, p.rows, p.row_bytes, 7 + i).reshape(n, -1) for i, p in enumerate(tab.planes)], 1)
        src = torch.from_numpy(host).to(dev)
        dst = torch.empty_like(src)
        sad = torch.empty(n - 1, dtype=torch.int64, device=dev)
        p, d = src.data_ptr(), dst.data_ptr()

        def denoise(r):
            for q in tab.planes:
                _lib.check(lib.savsr_video_denoise_u8(p, n, fb, q.offset, q.rows, q.row_bytes, r, 4, 9, 0, n, d, fb, q.offset, st), "denoise")

        def deint():
            for q in tab.planes:
                _lib.check(lib.savsr_video_deinterlace_u8_m(p, n, fb, q.offset, q.rows, q.row_bytes, 1, 0, 0, n, d, fb, q.offset, 1, 1, st), "deinterlace")

        calls = {f"denoise r={r}": (lambda r=r: denoise(r)) for r in RADII}
        calls["deinterlace_m same bwdif"] = deint
        calls["pair_sad_yuvp"] = lambda: _lib.check(lib.savsr_video_pair_sad_yuvp(p, n, h, w, 8, 0, sad.data_ptr(), st), "pair_sad")
        moved = {name: 2 * n * fb for name in calls}
        moved["pair_sad_yuvp"] = n * h * w
        taps = {}
        for r in RADII:          # warm-up, the result against the specification on the Y plane's first rows, and the mean tap count
            denoise(r)
            y = tab.planes[0]
            want, counts = denoise_matrix(host[:, :8 * y.row_bytes].reshape(n, 8, y.row_bytes), r, 4, 9, return_counts=True)
            assert np.array_equal(dst[:, :8 * y.row_bytes].cpu().numpy().reshape(n, 8, -1), want)
            taps[r] = float((counts["k"] * np.arange(counts["k"].size)).sum() / counts["k"].sum())
        deint()
        calls["pair_sad_yuvp"]()
        torch.cuda.synchronize()
        us = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                us[name].append(timed(fn, launches))
        med = {name: statistics.median(v) for name, v in us.items()}
        for name in calls:
            row = {"size": [h, w], "format": "i420", "n": n, "call": name, "us_per_call": round(med[name], 2),
                   "us_rounds": [round(v, 2) for v in us[name]], "spread": round((max(us[name]) - min(us[name])) / med[name], 4),
                   "bytes_moved": moved[name], "gb_s": round(moved[name] / med[name] / 1e3, 1)}
            if name.startswith("denoise"):
                r = int(name.split("=")[1])
                row.update(radius=r, mean_frames_averaged=round(taps[r], 2), time_vs_deinterlace=round(med[name] / med["deinterlace_m same bwdif"], 4))
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def time_end2end(dev, scale, rounds):
    import torch
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    n = E2E_FRAMES
    u8 = torch.from_numpy(noisy(n, 180, 320 * 3, 3).reshape(n, 180, 320, 3)).to(dev)
    calls = {"plain": lambda: net.upscale_video(u8, scale=scale, out="uint8"),
             "denoise": lambda: net.upscale_video(u8, scale=scale, out="uint8", denoise="ata"),
             "denoise_video": lambda: savsr_amd.denoise_video(u8)}

    def wall(fn, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        del r
        return (time.perf_counter() - t0) / reps
    assert torch.equal(calls["denoise"](), net.upscale_video(calls["denoise_video"](), scale=scale, out="uint8"))          # warm-up, and the property
    wall(calls["plain"])
    t = {k: [] for k in calls}
    for _ in range(rounds):          # A / B / A / B
        for k, fn in calls.items():
            t[k].append(wall(fn, 20 if k == "denoise_video" else 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"{n} noisy frames 180x320 x{scale:g}, uint8 in and out, radius 4, strength (4, 9)",
           "fps": {k: round(n / med[k], 3) for k in ("plain", "denoise")},
           "fps_rounds": {k: [round(n / v, 3) for v in t[k]] for k in ("plain", "denoise")},
           "denoise_vs_plain_time": round(med["denoise"] / med["plain"], 4),
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in calls},
           "denoise_video_ms": round(1e3 * med["denoise_video"], 3)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--only", default="kernels,end2end")
    ap.add_argument("--board", default="MI355X", help="the board's name for the record (the driver reports a generic one)")
    ap.add_argument("--lease", default="lease 1 (one MI355X, one process, nothing else of ours on the board)", help="which machine session the numbers are from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    board = f"{props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, {props.total_memory >> 30} GiB)"
    res = {"board": f"{a.board}: {board}", "lease": a.lease, "rounds": a.rounds, "launches": a.launches}
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
