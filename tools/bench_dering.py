"""dering=: what savsr_video_dering_u8 costs beside the kernels it stands next to, and what upscale_video(dering="cdef") adds.

  kernels   16 frames of 576 x 720 and of 720 x 1280 I420 (oblique edges coded by a coarse 8 x 8 DCT: a ringing picture), every plane
            one call: deringing at the default strength (4, 2) and damping 5, progressive and field-wise, beside
            savsr_video_deblock_u8 (block 8, strong, (25, 13)) and savsr_video_nlmeans_u8 at (patch, search) = (1, 3) on the same frames.
            One process, interleaved rounds, each reading a HIP-event pair around --launches back-to-back passes over the planes,
            --rounds times; medians and the rounds.  GB/s on one read plus one write of the frames.  With --parent (a checkout of the
            parent commit with its library built, or the library's path) savsr_video_deblock_u8 of that library runs in the same rounds:
            what the library's unchanged kernels cost before this stage was added to it.
  end2end   24 coded frames of 180 x 320, x4, uint8 in and out: upscale_video with and without dering="cdef" at the defaults, interleaved
            A / B / A / B in one process, in frames per second, dering_video's own time, and the stage's share of the call (its own time
            over the call's time with the stage).  dering=None is the call without the argument: the lines that ran before.

Numbers are recorded, not gated: there is no number to beat, the yardsticks are the deblocker, the small non-local means and the
network's own time.

    python3 tools/bench_dering.py [--parent ../parent_checkout --rounds 5 --launches 20 --scale 4 --lease "..." --out profiles/bench_dering.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_FRAMES = 16
E2E_FRAMES = 24
STRENGTH = (4, 2)
DAMPING = 5
DEBLOCK = (8, 1, 25, 13)          # block, strong, thresholds
NLM = (1, 3, 3.0)                 # patch, search, strength


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


def ringing(n, rows, cols, seed, q=40.0):
    """[n, rows, cols] uint8: oblique edges and smooth shading, moving one sample per frame, coded by an orthonormal 8 x 8 DCT whose AC
    coefficients are quantised with the step q (the DC with q / 4); rows and columns beyond the last whole block repeat the last ones."""
    import numpy as np
    k, m = np.mgrid[0:8, 0:8].astype(np.float64)
    d = np.cos((2 * m + 1) * k * np.pi / 16) * 0.5
    d[0] /= np.sqrt(2.0)
    step = np.full((8, 8), q)
    step[0, 0] = q / 4
    R, Cc = -(-rows // 8) * 8, -(-cols // 8) * 8
    y, x = np.mgrid[0:R, 0:Cc].astype(np.float64)
    rng = np.random.default_rng(seed)
    out = np.empty((n, rows, cols), np.uint8)
    for t in range(n):
        clean = 90 + 0.1 * x + 0.1 * y + 80 * ((x + t + 1.7 * y) % 61 < 24) - 50 * ((2.3 * x - y + t) % 83 < 30) + rng.normal(0, 1, (R, Cc))
        blocks = np.clip(clean, 0, 255).reshape(R // 8, 8, Cc // 8, 8).transpose(0, 2, 1, 3) - 128
        coded = d.T @ (np.rint((d @ blocks @ d.T) / step) * step) @ d + 128
        out[t] = np.clip(np.rint(coded.transpose(0, 2, 1, 3).reshape(R, Cc)), 0, 255)[:rows, :cols]
    return out


def parent_deblock(path):
    """savsr_video_deblock_u8 of the parent checkout's library (its own copy in this process), or None without --parent."""
    if not path:
        return None
    so = path if path.endswith(".so") else os.path.join(path, "savsr_amd", "csrc", "libsavsr_hip.so")
    lib = C.CDLL(so)
    from savsr_amd import _lib
    fn = lib.savsr_video_deblock_u8
    fn.restype, fn.argtypes = _lib.SIGNATURES["savsr_video_deblock_u8"]
    lib.savsr_abi_version.restype = C.c_int
    return fn, int(lib.savsr_abi_version())


def time_kernels(dev, rounds, launches, parent):
    import numpy as np
    import torch
    from savsr_amd import _lib
    from savsr_amd.dering import dering_plane
    from savsr_amd.frames import detector_side, plane_table
    from savsr_amd.nlmeans import divisor
    lib = _lib.load()
    old = parent_deblock(parent)
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    for h, w in ((576, 720), (720, 1280)):
        side, size = detector_side("i420", (h, w), 8)
        tab = plane_table(side, size)
        fb = tab.stride
        host = np.concatenate([ringing(n, p.rows, p.row_bytes, 7 + i).reshape(n, -1) for i, p in enumerate(tab.planes)], 1)
        src = torch.from_numpy(host).to(dev)
        dst = torch.empty_like(src)
        p, d = src.data_ptr(), dst.data_ptr()

        def dering(fieldwise):
            for q in tab.planes:
                _lib.check(lib.savsr_video_dering_u8(p, n, fb, q.offset, q.rows, q.row_bytes, 1, fieldwise, *STRENGTH, DAMPING, d, fb, q.offset, st), "dering")

        def deblock(fn=lib.savsr_video_deblock_u8):
            for q in tab.planes:
                rc = fn(p, n, fb, q.offset, q.rows, q.row_bytes, 1, DEBLOCK[0], DEBLOCK[1], 0, DEBLOCK[2], DEBLOCK[3], d, fb, q.offset, st)
                assert rc == 0, rc

        def nlmeans():
            for q in tab.planes:
                _lib.check(lib.savsr_video_nlmeans_u8(p, n, fb, q.offset, q.rows, q.row_bytes, 1, NLM[0], NLM[1], divisor(NLM[0], NLM[2]), d, fb, q.offset, st),
                           "nlmeans")

        calls = {"dering progressive": lambda: dering(0), "dering fields": lambda: dering(1), "deblock strong": deblock, "nlmeans (1, 3)": nlmeans}
        if old is not None:
            calls[f"deblock strong, parent library (ABI {old[1]})"] = lambda: deblock(old[0])
        for fw in (0, 1):          # warm-up, and the last frame's planes against the specification
            dering(fw)
            for q in tab.planes:
                got = dst[n - 1, q.offset:q.offset + q.rows * q.row_bytes].cpu().numpy().reshape(q.rows, q.row_bytes)
                want = dering_plane(host[n - 1, q.offset:q.offset + q.rows * q.row_bytes].reshape(q.rows, q.row_bytes), 8, STRENGTH, DAMPING, bool(fw))
                assert np.array_equal(got, want), (fw, q)
        for fn in calls.values():
            fn()
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
            if name.startswith("dering"):
                row.update(strength=list(STRENGTH), damping=DAMPING, us_per_frame=round(med[name] / n, 2),
                           time_vs_deblock=round(med[name] / med["deblock strong"], 2), time_vs_nlmeans=round(med[name] / med["nlmeans (1, 3)"], 2))
            if name == "deblock strong" and old is not None:
                row["time_vs_parent"] = round(med[name] / med[f"deblock strong, parent library (ABI {old[1]})"], 4)
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
    u8 = torch.from_numpy(ringing(n, 180, 320 * 3, 3).reshape(n, 180, 320, 3)).to(dev)
    calls = {"plain": lambda: net.upscale_video(u8, scale=scale, out="uint8"),
             "dering": lambda: net.upscale_video(u8, scale=scale, out="uint8", dering="cdef"),
             "dering_video": lambda: savsr_amd.dering_video(u8)}

    def wall(fn, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        del r
        return (time.perf_counter() - t0) / reps
    assert torch.equal(calls["dering"](), net.upscale_video(calls["dering_video"](), scale=scale, out="uint8"))          # warm-up, and the property
    wall(calls["plain"])
    t = {k: [] for k in calls}
    for _ in range(rounds):          # A / B / A / B
        for k, fn in calls.items():
            t[k].append(wall(fn, 20 if k == "dering_video" else 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"{n} coded frames 180x320 x{scale:g}, uint8 in and out, cdef, strength {STRENGTH[0]},{STRENGTH[1]}, damping {DAMPING}",
           "fps": {k: round(n / med[k], 3) for k in ("plain", "dering")},
           "fps_rounds": {k: [round(n / v, 3) for v in t[k]] for k in ("plain", "dering")},
           "dering_vs_plain_time": round(med["dering"] / med["plain"], 4),
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in calls},
           "dering_video_ms": round(1e3 * med["dering_video"], 3),
           "stage_share_of_call": round(med["dering_video"] / med["dering"], 4)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--only", default="kernels,end2end")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (or the library's path)")
    ap.add_argument("--board", default="MI355X", help="the board's name for the record (the driver reports a generic one)")
    ap.add_argument("--lease", default="lease 1 (one MI355X, one process, nothing else of ours on the board)", help="which machine session the numbers are from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    board = f"{props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, {props.total_memory >> 30} GiB)"
    res = {"board": f"{a.board}: {board}", "lease": a.lease, "rounds": a.rounds, "launches": a.launches, "parent": bool(a.parent)}
    with torch.no_grad():
        if "kernels" in a.only:
            res["kernels"] = time_kernels(dev, a.rounds, a.launches, a.parent)
        if "end2end" in a.only:
            res["end2end"] = time_end2end(dev, a.scale, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
