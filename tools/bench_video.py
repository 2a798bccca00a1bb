"""The sequence path (SAVSR.upscale_video) against today's way of getting SR frames of a video, on a seeded uint8 video:

  upscale_video      uint8 frames on the GPU -> uint8 SR frames on the GPU (window gather, network, quantisation: savsr_video_*)
  upscale_video_f32  the same with out="float" (fp32 SR frames)
  forward_many_pre   forward_many on the windows gathered beforehand (fp32 in and out; gathering not timed): the yardstick of the
                     >= 0.98x target for upscale_video_f32
  by_hand            today's way: fp32 conversion (the FrameStore table), the windows gathered by hand with torch indexing, forward_many,
                     tensor2img(rgb2bgr=False) on the host per frame
  cli                python -m savsr_amd.upscale on a folder of PNGs written from the same noise: decode + network + encode, its own
                     printed frames/s (a fresh process: includes its hipGraph captures; may be bound by PNG encoding on the host)

The GPU variants run alternately (A B C D, A B C D, ...) after one warm-up pass each; frames/s per variant is the median over --reps.
`kernels` in the line: savsr_video_gather_u8 (nb = 1 .. 4 windows of 7 frames) and savsr_video_quantize_u8 (1 and 3 frames) launched
alone on one stream, HIP events around 50 back-to-back calls, (distinct bytes read + bytes written) / time against 8 TB/s of HBM.
--kernels-only: that part alone (for a `rocprofv3 --kernel-trace --stats` run).

    python3 tools/bench_video.py [--frames 100 --h 180 --w 320 --scale 4 --reps 3 --out profiles/bench_video.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from savsr_amd import io as sio  # noqa: E402
from savsr_amd.archs.savsr_arch import SAVSR  # noqa: E402
from savsr_amd.harness import window_indices  # noqa: E402
from savsr_amd.metrics import tensor2img  # noqa: E402
from savsr_amd.utils import synth  # noqa: E402


HBM_BYTES_PER_S = 8e12


def time_kernels(h, w, scale, dev, iters=50):
    """The two kernels alone: us per call and the fraction of the HBM bound (distinct bytes read + bytes written, / 8 TB/s)."""
    import ctypes as C
    from savsr_amd import _lib
    from savsr_amd.packing import get_hw
    lib = _lib.load()
    st = torch.cuda.current_stream()
    H, W = get_hw(h, w, (scale, scale))
    frames = torch.randint(0, 256, (16, h, w, 3), dtype=torch.uint8, device=dev)
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
    for nb in (1, 2, 3, 4):
        idx = [b + j for b in range(nb) for j in range(7)]          # the windows of nb consecutive frames: 7 + nb - 1 distinct frames
        out = torch.empty(7 * nb, 3, h, w, device=dev)
        arr = (C.c_int32 * len(idx))(*idx)
        us = timed(lambda: _lib.check(lib.savsr_video_gather_u8(frames.data_ptr(), 16, 3, h, w, arr, len(idx), out.data_ptr(), st.cuda_stream), "gather"))
        nbytes = len(set(idx)) * h * w * 3 + out.numel() * 4
        rows.append({"kernel": "savsr_video_gather_u8", "nb": nb, "lr": [h, w], "us": round(us, 2), "mb": round(nbytes / 1e6, 2),
                     "hbm_frac": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3)})
    for n in (1, 3):
        x = torch.rand(n, 3, H, W, device=dev)
        q = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        us = timed(lambda: _lib.check(lib.savsr_video_quantize_u8(x.data_ptr(), n, 3, H, W, q.data_ptr(), st.cuda_stream), "quantize"))
        nbytes = x.numel() * 4 + q.numel()
        rows.append({"kernel": "savsr_video_quantize_u8", "frames": n, "hr": [H, W], "us": round(us, 2), "mb": round(nbytes / 1e6, 2),
                     "hbm_frac": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--h", type=int, default=180)
    ap.add_argument("--w", type=int, default=320)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.kernels_only:
        print(json.dumps({"kernels": time_kernels(a.h, a.w, a.scale, dev), "device": torch.cuda.get_device_name(dev)}), flush=True)
        return
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    n, sc = a.frames, (a.scale, a.scale)
    u8_host = np.random.RandomState(0).randint(0, 256, size=(n, a.h, a.w, 3), dtype=np.uint8)
    u8 = torch.from_numpy(u8_host).to(dev)
    lut = torch.from_numpy(np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0).to(dev)
    f32 = torch.index_select(lut, 0, u8.permute(0, 3, 1, 2).reshape(-1).to(torch.int64)).view(n, 3, a.h, a.w)
    wins = [window_indices(i, n, net.num_frame, "reflection") for i in range(n)]
    pre = [f32[w] for w in wins]

    def upscale_u8():
        return net.upscale_video(u8, scale=sc, out="uint8")

    def upscale_f32():
        return net.upscale_video(u8, scale=sc)

    def forward_many_pre():
        return net.forward_many(pre, [sc] * n)

    def by_hand():
        f = torch.index_select(lut, 0, u8.permute(0, 3, 1, 2).reshape(-1).to(torch.int64)).view(n, 3, a.h, a.w)
        outs = net.forward_many([f[w] for w in wins], [sc] * n)
        return [tensor2img(o, rgb2bgr=False) for o in outs]

    variants = {"upscale_video": upscale_u8, "upscale_video_f32": upscale_f32, "forward_many_pre": forward_many_pre, "by_hand": by_hand}
    times = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():          # warm-up: every (unit size, stream) graph captured
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
                del r
    res = {"workload": f"{n} frames {a.h}x{a.w} x{a.scale:g}, uint8 in", "device": torch.cuda.get_device_name(dev),
           "reps": a.reps, "padding": "reflection"}
    for k, ts in times.items():
        res[f"{k}_fps"] = round(n / statistics.median(ts), 2)
        res[f"{k}_fps_all"] = [round(n / t, 2) for t in ts]
    res["upscale_video_f32_vs_forward_many_pre"] = round(res["upscale_video_f32_fps"] / res["forward_many_pre_fps"], 4)
    res["upscale_video_vs_by_hand"] = round(res["upscale_video_fps"] / res["by_hand_fps"], 3)
    res["kernels"] = time_kernels(a.h, a.w, a.scale, dev)
    if not a.no_cli:
        from PIL import Image
        with tempfile.TemporaryDirectory() as td:
            src, dst = os.path.join(td, "lr"), os.path.join(td, "sr")
            os.makedirs(src)
            for i in range(n):
                Image.fromarray(u8_host[i]).save(os.path.join(src, f"{i:08d}.png"))
            ckpt = os.path.join(td, "net.pth")
            sio.save_network(net, ckpt)
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "savsr_amd.upscale", "-i", src, "-o", dst, "--scale", str(a.scale), "--checkpoint", ckpt],
                               cwd=ROOT, capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise SystemExit(f"CLI failed ({r.returncode}): {r.stderr[-2000:]}")
            line = r.stdout.strip().splitlines()[-1]
            res["cli_line"] = line
            res["cli_fps"] = float(line.split(":")[-1].split()[0])
            res["cli_process_wall_s"] = round(wall, 2)
            res["cli_writers"] = "min(16, usable CPUs)"
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
