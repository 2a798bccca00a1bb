"""Video surfaces ("Video surfaces"), measured.  Every leg is a process of its own under its own time limit; a leg
that fails, times out or dies ends the run (nothing more is started on the GPU) and what the earlier legs gave is kept.

  kernels   savsr_video_unpack_surface / _pack_surface for NV12, P010 and UYVY on 7 frames of 180x320 and of 720x1280, tight and with a
            256-byte pitch, beside savsr_video_gather_i420 / _quantize_i420 of the same build on the same 7 frames, in one process,
            interleaved rounds: us and GB/s = (bytes read + bytes written) / time.  HIP events around `iters` back-to-back launches, as
            tools/bench_y4m.py times its kernels (launch rate included).
  e2e       upscale_video on 100 resident frames of 180x320 at x4, I420 out: (A) I420 in and out on the PARENT commit's tree (--parent DIR,
            a checkout of it with its library built), (B) NV12 in and NV12 out on this tree, (C) I420 in and out on this tree (the
            no-regression leg).  Fresh processes, interleaved A/B/C/A/B/C..., `--rounds` of them.  The bound is the parent's own
            run-to-run spread: the medians of legs B and C must lie within the range of A's repeats widened by that range once more.  All
            raw values, the spread and the verdict are recorded.

    python3 tools/bench_surface.py --parent /path/to/parent/checkout --out profiles/bench_surface.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG_TIMEOUT_S = {"kernels": 240, "e2e": 180}


def _root(a):
    root = os.path.abspath(a.root or ROOT)
    sys.path.insert(0, root)
    return root


def leg_kernels(a):
    _root(a)
    import ctypes as C
    import numpy as np
    import torch
    from savsr_amd import _lib
    from savsr_amd import surface as S
    from savsr_amd.yuv import frame_bytes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    n = 7
    rows = []
    for h, w in ((180, 320), (720, 1280)):
        fns, moved = {}, {}
        keep = []
        for kind, depth in (("nv12", 8), ("p010", 10), ("uyvy", 8)):
            layout = "422" if kind == "uyvy" else "420"
            for pitch in ("tight", "pitch256"):
                surf = getattr(S.Surface, kind)() if pitch == "tight" else getattr(S.Surface, kind)(pitch_align=256)
                tab = surf.resolve(h, w, depth, layout)
                fb = frame_bytes(h, w, depth, layout)
                s_buf = torch.randint(0, 256, (n, tab.bytes), dtype=torch.uint8, device=dev)
                p_buf = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device=dev)
                desc = S.descriptor(tab)
                dp = desc.ctypes.data_as(C.POINTER(C.c_int64))
                keep.append((desc, s_buf, p_buf))
                head = (h, w, depth, S.LAYOUTS.index(layout), int(tab.msb), dp, len(tab.planes))
                covered = sum(p.rows * tab.row_bytes(p) for p in tab.planes)
                fns[f"savsr_video_unpack_surface {kind} {pitch}"] = (
                    lambda s=s_buf, p=p_buf, t=tab, f=fb, hd=head: lib.savsr_video_unpack_surface(s.data_ptr(), n, t.bytes, *hd, p.data_ptr(), f, st))
                fns[f"savsr_video_pack_surface {kind} {pitch}"] = (
                    lambda s=s_buf, p=p_buf, t=tab, f=fb, hd=head: lib.savsr_video_pack_surface(p.data_ptr(), n, f, *hd, s.data_ptr(), t.bytes, t.bytes, st))
                moved[f"savsr_video_unpack_surface {kind} {pitch}"] = n * (covered + fb)
                moved[f"savsr_video_pack_surface {kind} {pitch}"] = n * (fb + covered + (0 if tab.tight else tab.bytes))          # (+ the memset)
        arr = (C.c_int32 * n)(*range(n))
        i420 = torch.randint(0, 256, (n, frame_bytes(h, w)), dtype=torch.uint8, device=dev)
        slots = torch.empty(n, 3, h, w, device=dev)
        x = torch.rand(n, 3, h, w, device=dev)
        q420 = torch.empty(n, frame_bytes(h, w), dtype=torch.uint8, device=dev)
        fns["savsr_video_gather_i420"] = lambda: lib.savsr_video_gather_i420(i420.data_ptr(), n, h, w, arr, n, slots.data_ptr(), st)
        fns["savsr_video_quantize_i420"] = lambda: lib.savsr_video_quantize_i420(x.data_ptr(), n, h, w, q420.data_ptr(), st)
        moved["savsr_video_gather_i420"] = moved["savsr_video_quantize_i420"] = int(n * (4 * 3 + 1.5) * h * w)
        us = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn() == 0, (k, lib.savsr_last_error())
        torch.cuda.synchronize()
        for _ in range(a.kernel_rounds):                # interleaved rounds: every kernel sees the same clocks
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1) / a.iters)
        for k in fns:
            med = statistics.median(us[k])
            rows.append({"kernel": k, "size": [h, w], "frames": n, "us": round(med, 2), "mb": round(moved[k] / 1e6, 3),
                         "gbs": round(moved[k] / (med * 1e-6) / 1e9, 1), "us_rounds": [round(v, 2) for v in us[k]]})
        del keep
    return {"kernels": rows, "rounds": a.kernel_rounds, "iters": a.iters,
            "timing": "HIP events around `iters` back-to-back launches (launch rate included); GB/s = (bytes read + bytes written) / time"}


def leg_e2e(a):
    root = _root(a)
    import numpy as np
    import torch
    from savsr_amd import yuv
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    dev = torch.device("cuda:0")
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    h, w, n = a.h, a.w, a.frames
    clip = synth.synth_clip(n, 3, h, w, seed=3)[0].numpy().astype(np.float32)
    frames = yuv.rgb_to_i420(clip)
    kw = dict(scale=a.scale, pixel_format="i420", size=(h, w), out="i420")
    if a.surface == "nv12":
        from savsr_amd import surface as S
        s_in = S.Surface.nv12(pitch_align=256, lines_align=16)          # what a hardware decoder hands out
        frames = S.pack_frames(frames, s_in, h, w)
        kw.update(surface=s_in, out_surface=S.Surface.nv12(pitch_align=256, lines_align=16))
    frames = torch.from_numpy(frames).to(dev)
    net.upscale_video(frames[:16], **kw)                 # warm-up: the library, the plans, the allocator
    torch.cuda.synchronize()
    fps = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = net.upscale_video(frames, **kw)
        torch.cuda.synchronize()
        fps.append(n / (time.perf_counter() - t0))
        del out
    return {"tree": "this" if os.path.samefile(root, ROOT) else "parent", "surface": a.surface, "frames": n, "size": [h, w], "scale": a.scale,
            "fps": [round(v, 3) for v in fps], "fps_median": round(statistics.median(fps), 3)}


LEGS = {"kernels": leg_kernels, "e2e": leg_e2e}


def _child(a, leg, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(a.frames), "--h", str(a.h), "--w", str(a.w), "--scale", str(a.scale),
           "--reps", str(a.reps), "--kernel-rounds", str(a.kernel_rounds), "--iters", str(a.iters), *extra]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=LEG_TIMEOUT_S[leg])
    except subprocess.TimeoutExpired:
        return None, f"{leg}: no result within {LEG_TIMEOUT_S[leg]} s"
    if r.returncode != 0:
        return None, f"{leg}: exit status {r.returncode}: {r.stderr[-600:]}"
    return json.loads(r.stdout.strip().splitlines()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--h", type=int, default=180)
    ap.add_argument("--w", type=int, default=320)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="fresh processes per end-to-end leg")
    ap.add_argument("--kernel-rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (the A leg); without it the e2e leg is skipped")
    ap.add_argument("--legs", default="kernels,e2e")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)          # (a child process: run one leg, print its JSON)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)         # (a child process: the tree to import savsr_amd from)
    ap.add_argument("--surface", default="none", help=argparse.SUPPRESS)
    ap.add_argument("--note", default=None, help="recorded as \"machine\": what ran where, and what ran beside it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(LEGS[a.leg](a)), flush=True)
        return
    res = {"tool": "tools/bench_surface.py", "legs": {}}
    legs = a.legs.split(",")
    err = None
    if "kernels" in legs:
        res["legs"]["kernels"], err = _child(a, "kernels")
        print("kernels", json.dumps(res["legs"]["kernels"]), flush=True)
    if "e2e" in legs and err is None and a.parent:
        plan = (("parent_i420", a.parent, "none"), ("nv12", ROOT, "nv12"), ("i420", ROOT, "none"))
        runs = {name: [] for name, _, _ in plan}
        for _ in range(a.rounds):
            for name, root, surf in plan:
                if err is None:
                    r, err = _child(a, "e2e", "--root", root, "--surface", surf)
                    if r is not None:
                        runs[name].append(r)
                        print(name, r["fps"], flush=True)
        e2e = {"runs": runs, "order": "fresh processes, interleaved parent_i420 / nv12 / i420, round after round"}
        if err is None:
            med = {k: [r["fps_median"] for r in v] for k, v in runs.items()}
            lo, hi = min(med["parent_i420"]), max(med["parent_i420"])
            spread = hi - lo
            e2e.update(fps_medians=med, parent_range=[lo, hi], parent_spread=round(spread, 3), bound=[round(lo - spread, 3), round(hi + spread, 3)],
                       rule="a leg's median over its processes must lie within the range of the parent's processes widened by that range once more")
            for k in ("nv12", "i420"):
                m = statistics.median(med[k])
                e2e[f"{k}_median"] = round(m, 3)
                e2e[f"{k}_vs_parent"] = round(m / statistics.median(med["parent_i420"]), 4)
                e2e[f"{k}_within_bound"] = bool(lo - spread <= m <= hi + spread)
                e2e[f"{k}_processes_within_bound"] = sum(lo - spread <= v <= hi + spread for v in med[k])
        res["legs"]["e2e"] = e2e
    if err is not None:
        res["stopped"] = err
        print("STOPPED:", err, flush=True)
    if a.note:
        res["machine"] = a.note
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if err is not None:
        sys.exit(1)


if __name__ == "__main__":
    main()
