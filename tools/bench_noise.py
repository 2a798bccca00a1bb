"""The noise estimator: what savsr_video_noise_stats_u8 costs beside the one-read reductions it stands next to, and what
upscale_video(denoise_strength="auto") / (spatial_strength="auto") add to a call.

  stats     16 noisy frames (sigma 2) of 576 x 720 and of 720 x 1280 I420: noise_stats on the Y plane and on all three planes (what
            estimate_noise launches), progressive and field-wise, beside savsr_video_grid_stats_u8 and savsr_video_line_sums_u8 on the
            same planes in the same rounds -- the yardsticks for one read of the frames.  GB/s of one read.  The last frame's table is
            compared with the specification first.
  end2end   24 noisy frames of 180 x 320, x4, uint8 in and out: upscale_video with denoise="ata" and with spatial_denoise="nlm", each
            at the strength the estimator finds given explicitly and with "auto" (one more launch and one more host synchronisation),
            interleaved, in frames per second.
  parent    with --parent (a checkout of the parent commit with its library built): the explicit-strength calls from this tree and
            from the parent's, each in fresh child processes of this tool (--only explicit --root TREE), alternating -- two trees
            cannot share a process, so this comparison carries the processes' start-up state in its spread.

One process, interleaved rounds, each reading a HIP-event pair around --launches back-to-back passes, --rounds times; medians and the
rounds with their spread.  Numbers are recorded, not gated.

    python3 tools/bench_noise.py [--parent ../parent_checkout --rounds 5 --launches 20 --lease "..." --out profiles/bench_noise.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES = 16
E2E_FRAMES = 24
SIGMA = 2.0


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


def noisy(n, rows, cols, seed, sigma=SIGMA):
    """[n, rows, cols] uint8: 128 + 60 sin(x / 11) cos(y / 13), moving one sample per frame, plus sigma noise."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    out = np.empty((n, rows, cols), np.uint8)
    for t in range(n):
        out[t] = np.clip(np.rint(128 + 60 * np.sin((x + t) / 11.0) * np.cos(y / 13.0) + rng.normal(0, sigma, (rows, cols))), 0, 255)
    return out


def row_of(name, us, nbytes, **more):
    med = statistics.median(us)
    row = {"call": name, "us_per_call": round(med, 2), "us_rounds": [round(v, 2) for v in us], "spread": round((max(us) - min(us)) / med, 4),
           "bytes": nbytes, "gb_s": round(nbytes / med / 1e3, 1)}
    row.update(more)
    return row


def time_kernels(dev, rounds, launches):
    import numpy as np
    import torch
    from savsr_amd import _lib
    from savsr_amd.frames import detector_side, plane_table
    from savsr_amd.noise import noise_stats_matrix
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, rows = N_FRAMES, []
    for h, w in ((576, 720), (720, 1280)):
        side, size = detector_side("i420", (h, w), 8)
        tab = plane_table(side, size)
        fb = tab.stride
        host = np.concatenate([noisy(n, p.rows, p.row_bytes, 7 + i).reshape(n, -1) for i, p in enumerate(tab.planes)], 1)
        src = torch.from_numpy(host).to(dev)
        p = src.data_ptr()
        table = torch.zeros(n, 256, 2, dtype=torch.int64, device=dev)
        cells = torch.zeros(n, 2, 16, dtype=torch.int64, device=dev)
        sums = torch.zeros(n * (h + w), dtype=torch.int32, device=dev)

        def noise(planes, fw):
            for q in planes:
                _lib.check(lib.savsr_video_noise_stats_u8(p, n, fb, q.offset, q.rows, q.row_bytes, 1, fw, table.data_ptr(), st), "noise_stats")

        def grid(planes, fw):
            for q in planes:
                _lib.check(lib.savsr_video_grid_stats_u8(p, n, fb, q.offset, q.rows, q.row_bytes, 1, fw, 32, cells.data_ptr(), st), "grid_stats")

        def line_sums():
            _lib.check(lib.savsr_video_line_sums_u8(p, n, fb, h, w, sums.data_ptr(), sums.data_ptr() + 4 * n * h, st), "line_sums")

        for fw in (0, 1):          # warm-up, and the last frame's table against the specification
            table.zero_()
            noise(tab.planes[:1], fw)
            assert np.array_equal(table[n - 1].cpu().numpy(), noise_stats_matrix(host[n - 1, :h * w].reshape(h, w), 8, bool(fw))), fw
        grid(tab.planes[:1], 0)
        line_sums()
        calls = {"noise_stats Y progressive": lambda: noise(tab.planes[:1], 0), "noise_stats Y fields": lambda: noise(tab.planes[:1], 1),
                 "grid_stats Y progressive": lambda: grid(tab.planes[:1], 0), "grid_stats Y fields": lambda: grid(tab.planes[:1], 1),
                 "line_sums Y": line_sums,
                 "noise_stats Y+Cb+Cr progressive": lambda: noise(tab.planes, 0), "noise_stats Y+Cb+Cr fields": lambda: noise(tab.planes, 1),
                 "grid_stats Y+Cb+Cr progressive": lambda: grid(tab.planes, 0), "grid_stats Y+Cb+Cr fields": lambda: grid(tab.planes, 1)}
        torch.cuda.synchronize()
        us = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                us[name].append(timed(fn, launches))
        for name in calls:
            nbytes = n * (fb if "Cb" in name else h * w)
            more = {}
            if name.startswith("noise_stats"):
                more["time_vs_grid_stats"] = round(statistics.median(us[name]) / statistics.median(us[name.replace("noise_stats", "grid_stats")]), 2)
            rows.append(row_of(name, us[name], nbytes, size=[h, w], format="i420", n=n, **more))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def e2e_setup(dev):
    import numpy as np
    import torch
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    n = E2E_FRAMES
    u8 = torch.from_numpy(np.stack([noisy(n, 180, 320, 20 + c) for c in range(3)], -1)).to(dev)
    return net, u8


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    del r
    return time.perf_counter() - t0


def summary(t, n, base=None):
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"fps": {k: round(n / med[k], 3) for k in t}, "fps_rounds": {k: [round(n / v, 3) for v in t[k]] for k in t},
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in t}}
    if base:
        res["time_vs_explicit"] = {k: round(med[k] / med[base[k]], 4) for k in t if k in base}
    return res


def time_end2end(dev, scale, rounds):
    import torch
    import savsr_amd
    net, u8 = e2e_setup(dev)
    first = savsr_amd.estimate_noise(u8)
    kw_t, kw_s = first.denoise_kwargs(), first.spatial_kwargs()
    assert kw_t and kw_s, first
    kw = dict(scale=scale, out="uint8")
    calls = {"denoise explicit": lambda: net.upscale_video(u8, denoise="ata", **kw_t, **kw),
             "denoise auto": lambda: net.upscale_video(u8, denoise="ata", denoise_strength="auto", **kw),
             "spatial explicit": lambda: net.upscale_video(u8, spatial_denoise="nlm", **kw_s, **kw),
             "spatial auto": lambda: net.upscale_video(u8, spatial_denoise="nlm", spatial_strength="auto", **kw)}
    for a in ("denoise", "spatial"):          # warm-up, and the property
        assert torch.equal(calls[f"{a} auto"](), calls[f"{a} explicit"]()), a
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn))
    res = {"workload": f"{E2E_FRAMES} noisy frames (sigma {SIGMA:g}) 180x320 x{scale:g}, uint8 in and out",
           "verdict": {"sigma": float(first.sigma), "denoise_strength": list(kw_t["denoise_strength"]), "spatial_strength": kw_s["spatial_strength"]}}
    res.update(summary(t, E2E_FRAMES, {"denoise auto": "denoise explicit", "spatial auto": "spatial explicit"}))
    print(json.dumps(res), flush=True)
    return res


def time_explicit(dev, scale, rounds):
    """The explicit-strength calls alone, at fixed strengths (this mode also runs from the parent's tree, which has no estimator)."""
    net, u8 = e2e_setup(dev)
    kw = dict(scale=scale, out="uint8")
    calls = {"denoise explicit": lambda: net.upscale_video(u8, denoise="ata", denoise_strength=(7, 15), **kw),
             "spatial explicit": lambda: net.upscale_video(u8, spatial_denoise="nlm", spatial_strength=3.0625, **kw)}
    for fn in calls.values():
        wall(fn)
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn))
    return {k: [round(v, 6) for v in t[k]] for k in calls}


def time_parent(parent, scale, rounds, visits=2):
    """The explicit calls from this tree and from the parent's, in fresh child processes, alternating."""
    t = {"this": {}, "parent": {}}
    for _ in range(visits):
        for name, root in (("this", HERE), ("parent", os.path.abspath(parent))):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "explicit", "--root", root, "--rounds", str(rounds), "--scale", str(scale)],
                                 capture_output=True, text=True, timeout=600)
            if out.returncode:
                raise SystemExit(f"the child for {root} failed:\n{out.stdout[-1000:]}{out.stderr[-3000:]}")
            for k, v in json.loads(out.stdout.strip().splitlines()[-1]).items():
                t[name].setdefault(k, []).extend(v)
    res = {"processes_per_tree": visits}
    for name in t:
        res[name] = summary(t[name], E2E_FRAMES)
    res["time_vs_parent"] = {k: round(statistics.median(t["this"][k]) / statistics.median(t["parent"][k]), 4) for k in t["this"]}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--root", default=HERE, help="the tree savsr_amd is imported from (the child processes of --parent)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--only", default="kernels,end2end,parent")
    ap.add_argument("--board", default="MI355X", help="the board's name for the record (the driver reports a generic one)")
    ap.add_argument("--lease", default="lease 1 (one MI355X, one process at a time, nothing else of ours on the board)", help="which machine session the numbers are from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    dev = torch.device("cuda:0")
    with torch.no_grad():
        if a.only == "explicit":
            print(json.dumps(time_explicit(dev, a.scale, a.rounds)), flush=True)
            return
        props = torch.cuda.get_device_properties(0)
        board = f"{props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, {props.total_memory >> 30} GiB)"
        res = {"board": f"{a.board}: {board}", "lease": a.lease, "rounds": a.rounds, "launches": a.launches, "parent": bool(a.parent)}
        if "kernels" in a.only:
            res["noise_stats"] = time_kernels(dev, a.rounds, a.launches)
        if "end2end" in a.only:
            res["end2end"] = time_end2end(dev, a.scale, a.rounds)
    if "parent" in a.only and a.parent:
        res["explicit_vs_parent"] = time_parent(a.parent, a.scale, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
