"""deblock=: what savsr_video_deblock_u8 costs beside the memory-bound kernels it stands next to, and what upscale_video(deblock="strong")
adds.

  kernels   16 frames of 576 x 720 and of 720 x 1280 I420 (a smooth picture with an offset per 8 x 8 block), every plane one call:
            deblocking at block 8, weak and strong, progressive and field-wise, beside the temporal denoiser at radius 1
            (savsr_video_denoise_u8) and savsr_video_deinterlace_u8_m at the same rate (bwdif) on the same frames.  One process,
            interleaved rounds, each reading a HIP-event pair around --launches back-to-back passes over the planes, --rounds times;
            medians and the rounds.  GB/s on one read plus one write of the frames.
  end2end   24 blocky frames of 180 x 320, x4, uint8 in and out: upscale_video with and without deblock="strong" at the defaults,
            interleaved A / B / A / B in one process, in frames per second, deblock_video's own time, and the stage's share of the call
            (its own time over the call's time with the stage).

Numbers are recorded, not gated: there is no number to beat, the yardsticks are the two memory-bound kernels and the network's own time.

    python3 tools/bench_deblock.py [--rounds 5 --launches 20 --scale 4 --lease "..." --out profiles/bench_deblock.json]
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
BLOCK = 8
STRENGTH = (25, 13)
FORMS = (("weak", 0), ("strong", 0), ("weak", 1), ("strong", 1))          # (mode, field-wise)


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


def blocky(n, rows, cols, seed):
    """[n, rows, cols] uint8: 128 + 60 sin(x / 11) cos(y / 13), moving one sample per frame, plus an offset in -4 .. 4 per 8 x 8 block and
    frame and sigma = 1 noise."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    out = np.empty((n, rows, cols), np.uint8)
    for t in range(n):
        offs = rng.integers(-4, 5, (rows // 8 + 1, cols // 8 + 1))
        clean = 128 + 60 * np.sin((x + t) / 11.0) * np.cos(y / 13.0) + offs[y // 8, x // 8]
        out[t] = np.clip(np.rint(clean + rng.normal(0, 1, (rows, cols))), 0, 255)
    return out


def time_kernels(dev, rounds, launches):
    import numpy as np
    import torch
    from savsr_amd import _lib
    from savsr_amd.deblock import deblock_plane
    from savsr_amd.frames import detector_side, plane_table
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    for h, w in ((576, 720), (720, 1280)):
        side, size = detector_side("i420", (h, w), 8)
        tab = plane_table(side, size)
        fb = tab.stride
        host = np.concatenate([blocky(n, p.rows, p.row_bytes, 7 + i).reshape(n, -1) for i, p in enumerate(tab.planes)], 1)
        src = torch.from_numpy(host).to(dev)
        dst = torch.empty_like(src)
        p, d = src.data_ptr(), dst.data_ptr()

        def deblock(mode, fieldwise):
            for q in tab.planes:
                _lib.check(lib.savsr_video_deblock_u8(p, n, fb, q.offset, q.rows, q.row_bytes, 1, BLOCK, int(mode == "strong"), fieldwise, *STRENGTH, d, fb,
                                                      q.offset, st), "deblock")

        def denoise():
            for q in tab.planes:
                _lib.check(lib.savsr_video_denoise_u8(p, n, fb, q.offset, q.rows, q.row_bytes, 1, 4, 9, 0, n, d, fb, q.offset, st), "denoise")

        def deint():
            for q in tab.planes:
                _lib.check(lib.savsr_video_deinterlace_u8_m(p, n, fb, q.offset, q.rows, q.row_bytes, 1, 0, 0, n, d, fb, q.offset, 1, 1, st), "deinterlace")

        name_of = lambda mode, fw: f"deblock {mode} {'fields' if fw else 'progressive'}"          # noqa: E731
        calls = {name_of(mode, fw): (lambda mode=mode, fw=fw: deblock(mode, fw)) for mode, fw in FORMS}
        calls["denoise r=1"] = denoise
        calls["deinterlace_m same bwdif"] = deint
        for mode, fw in FORMS:          # warm-up, and the last frame's planes against the specification
            deblock(mode, fw)
            for q in tab.planes:
                got = dst[n - 1, q.offset:q.offset + q.rows * q.row_bytes].cpu().numpy().reshape(q.rows, q.row_bytes)
                want = deblock_plane(host[n - 1, q.offset:q.offset + q.rows * q.row_bytes].reshape(q.rows, q.row_bytes), 8, BLOCK, mode, STRENGTH, bool(fw))
                assert np.array_equal(got, want), (mode, fw, q)
        denoise()
        deint()
        torch.cuda.synchronize()
        us = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                us[name].append(timed(fn, launches))
        med = {name: statistics.median(v) for name, v in us.items()}
        for name in calls:
            row = {"size": [h, w], "format": "i420", "n": n, "call": name, "us_per_call": round(med[name], 2),
                   "us_rounds": [round(v, 2) for v in us[name]], "spread": round((max(us[name]) - min(us[name])) / med[name], 4),
                   "bytes_moved": 2 * n * fb, "gb_s": round(2 * n * fb / med[name] / 1e3, 1)}
            if name.startswith("deblock"):
                row.update(block=BLOCK, strength=list(STRENGTH), us_per_frame=round(med[name] / n, 2),
                           time_vs_denoise=round(med[name] / med["denoise r=1"], 2),
                           time_vs_deinterlace=round(med[name] / med["deinterlace_m same bwdif"], 2))
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
    u8 = torch.from_numpy(blocky(n, 180, 320 * 3, 3).reshape(n, 180, 320, 3)).to(dev)
    calls = {"plain": lambda: net.upscale_video(u8, scale=scale, out="uint8"),
             "deblock": lambda: net.upscale_video(u8, scale=scale, out="uint8", deblock="strong"),
             "deblock_video": lambda: savsr_amd.deblock_video(u8, mode="strong")}

    def wall(fn, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        del r
        return (time.perf_counter() - t0) / reps
    assert torch.equal(calls["deblock"](), net.upscale_video(calls["deblock_video"](), scale=scale, out="uint8"))          # warm-up, and the property
    wall(calls["plain"])
    t = {k: [] for k in calls}
    for _ in range(rounds):          # A / B / A / B
        for k, fn in calls.items():
            t[k].append(wall(fn, 20 if k == "deblock_video" else 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"{n} blocky frames 180x320 x{scale:g}, uint8 in and out, strong, block {BLOCK}, strength {STRENGTH[0]},{STRENGTH[1]}",
           "fps": {k: round(n / med[k], 3) for k in ("plain", "deblock")},
           "fps_rounds": {k: [round(n / v, 3) for v in t[k]] for k in ("plain", "deblock")},
           "deblock_vs_plain_time": round(med["deblock"] / med["plain"], 4),
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in calls},
           "deblock_video_ms": round(1e3 * med["deblock_video"], 3),
           "stage_share_of_call": round(med["deblock_video"] / med["deblock"], 4)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
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
