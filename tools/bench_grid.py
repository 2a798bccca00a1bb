"""The grid origin and the grid detector: what savsr_video_grid_stats_u8 costs beside the one-read reductions it stands next to, what the
origin path costs the deblocker, and what upscale_video(deblock_grid="auto") adds.

  stats     16 frames of 576 x 720 and of 720 x 1280 I420 (a smooth picture with an offset per 8 x 8 block): grid_stats on the Y plane,
            progressive and field-wise, beside savsr_video_line_sums_u8 and savsr_video_field_stats_u8 on the same plane -- the two
            yardsticks for a one-read reduction -- and on all three planes (what detect_grid launches).  GB/s of one read.
  deblock   the same frames, every plane one call, strong, block 8: origin (0, 0) through the entry without an origin, from this tree's
            library and from the parent commit's (--parent: a checkout of it with its library built), alternating in one process; and
            origin (3, 5) through the `_o` entry (up to one more tile column and row, and rows that start off a dword).
  end2end   24 blocky frames of 180 x 320, x4, uint8 in and out: upscale_video with deblock="strong" alone, with an explicit origin, and
            with deblock_grid="auto" (one more launch and one more host synchronisation), interleaved, in frames per second.

One process, interleaved rounds, each reading a HIP-event pair around --launches back-to-back passes, --rounds times; medians and the
rounds with their spread.  Numbers are recorded, not gated.

    python3 tools/bench_grid.py [--parent ../parent_checkout --rounds 5 --launches 20 --lease "..." --out profiles/bench_grid.json]
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
from tools.bench_deblock import blocky, timed  # noqa: E402

N_FRAMES = 16
E2E_FRAMES = 24
STRENGTH = (25, 13)
ORIGIN = (3, 5)


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


def row_of(name, us, nbytes, **more):
    med = statistics.median(us)
    row = {"call": name, "us_per_call": round(med, 2), "us_rounds": [round(v, 2) for v in us], "spread": round((max(us) - min(us)) / med, 4),
           "bytes": nbytes, "gb_s": round(nbytes / med / 1e3, 1)}
    row.update(more)
    return row


def time_kernels(dev, rounds, launches, parent):
    import numpy as np
    import torch
    from savsr_amd import _lib
    from savsr_amd.deblock import deblock_plane
    from savsr_amd.frames import detector_side, plane_table
    from savsr_amd.grid import grid_stats_matrix
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, stats, deblock = N_FRAMES, [], []
    old = parent_deblock(parent)
    for h, w in ((576, 720), (720, 1280)):
        side, size = detector_side("i420", (h, w), 8)
        tab = plane_table(side, size)
        fb, y = tab.stride, tab.planes[0]
        host = np.concatenate([blocky(n, p.rows, p.row_bytes, 7 + i).reshape(n, -1) for i, p in enumerate(tab.planes)], 1)
        src = torch.from_numpy(host).to(dev)
        dst = torch.empty_like(src)
        p, d = src.data_ptr(), dst.data_ptr()
        cells = torch.zeros(n, 2, 16, dtype=torch.int64, device=dev)
        sums = torch.zeros(n * (h + w), dtype=torch.int32, device=dev)
        scan = torch.zeros(n, 8, dtype=torch.int64, device=dev)

        def grid(planes, fw):
            for q in planes:
                _lib.check(lib.savsr_video_grid_stats_u8(p, n, fb, q.offset, q.rows, q.row_bytes, 1, fw, 32, cells.data_ptr(), st), "grid_stats")

        def line_sums():
            _lib.check(lib.savsr_video_line_sums_u8(p, n, fb, h, w, sums.data_ptr(), sums.data_ptr() + 4 * n * h, st), "line_sums")

        def field_stats():
            _lib.check(lib.savsr_video_field_stats_u8(p, n, fb, 0, h, w, 0, n, scan.data_ptr(), st), "field_stats")

        for fw in (0, 1):          # warm-up, and the last frame's cells against the specification
            cells.zero_()
            grid(tab.planes[:1], fw)
            assert np.array_equal(cells[n - 1].cpu().numpy(), grid_stats_matrix(host[n - 1, :h * w].reshape(h, w), 8, bool(fw))), fw
        line_sums()
        field_stats()
        calls = {"grid_stats Y progressive": lambda: grid(tab.planes[:1], 0), "grid_stats Y fields": lambda: grid(tab.planes[:1], 1),
                 "line_sums Y": line_sums, "field_stats Y": field_stats,
                 "grid_stats Y+Cb+Cr progressive": lambda: grid(tab.planes, 0), "grid_stats Y+Cb+Cr fields": lambda: grid(tab.planes, 1)}
        torch.cuda.synchronize()
        us = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                us[name].append(timed(fn, launches))
        slower = max(statistics.median(us["line_sums Y"]), statistics.median(us["field_stats Y"]))
        for name in calls:
            nbytes = n * (fb if "Cb" in name else h * w) * (3 if name.startswith("field_stats") else 1)
            more = {"time_vs_slower_yardstick": round(statistics.median(us[name]) / slower, 2)} if name.startswith("grid_stats Y ") else {}
            if name.startswith("field_stats"):
                more["note"] = "reads three frames a sample (previous, current, next): gb_s counts all three, one read of the plane is a third"
            stats.append(row_of(name, us[name], nbytes, size=[h, w], format="i420", n=n, **more))
            print(json.dumps(stats[-1]), flush=True)

        def run(fn, origin):
            for q in tab.planes:
                head = (p, n, fb, q.offset, q.rows, q.row_bytes, 1, 8, 1, 0, *STRENGTH, d, fb, q.offset)
                rc = fn(*head, st) if origin is None else fn(*head, *origin, st)
                assert rc == 0, lib.savsr_last_error()

        calls = {"deblock (0,0), entry without origin": lambda: run(lib.savsr_video_deblock_u8, None)}
        if old is not None:
            calls[f"deblock (0,0), parent library (ABI {old[1]})"] = lambda: run(old[0], None)
        calls["deblock (0,0), _o entry"] = lambda: run(lib.savsr_video_deblock_u8_o, (0, 0))
        calls[f"deblock ({ORIGIN[0]},{ORIGIN[1]}), _o entry"] = lambda: run(lib.savsr_video_deblock_u8_o, ORIGIN)
        want = {}
        for name, fn in calls.items():          # warm-up; the default path writes the parent's bytes, the origin path the specification's
            dst.zero_()
            fn()
            want[name] = dst.clone()
        base = want["deblock (0,0), entry without origin"]
        for name, got in want.items():
            if "(0,0)" in name:
                assert torch.equal(got, base), name
        got = want[f"deblock ({ORIGIN[0]},{ORIGIN[1]}), _o entry"][n - 1, :h * w].cpu().numpy().reshape(h, w)
        assert np.array_equal(got, deblock_plane(host[n - 1, :h * w].reshape(h, w), 8, 8, "strong", STRENGTH, False, ORIGIN))
        us = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                us[name].append(timed(fn, launches))
        ref = statistics.median(us[[k for k in calls if "parent" in k][0]]) if old is not None else None
        for name in calls:
            more = {} if ref is None else {"time_vs_parent": round(statistics.median(us[name]) / ref, 4)}
            deblock.append(row_of(name, us[name], 2 * n * fb, size=[h, w], format="i420", n=n, mode="strong", block=8, **more))
            print(json.dumps(deblock[-1]), flush=True)
    return stats, deblock


def time_end2end(dev, scale, rounds):
    import numpy as np
    import torch
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    n = E2E_FRAMES
    from tests.grid_cases import blocky as picture, case_seed          # every channel of every frame: block 8 cropped so that the grid sits at ORIGIN
    u8 = torch.from_numpy(np.stack([np.stack([picture(case_seed(t, c), 180, 320, 8, 4, 1.0, ORIGIN) for c in range(3)], -1) for t in range(n)])).to(dev)
    kw = dict(scale=scale, out="uint8", deblock="strong")
    verdict = savsr_amd.detect_grid(u8)
    assert (verdict.block, verdict.origin) == (8, ORIGIN), verdict
    calls = {"deblock": lambda: net.upscale_video(u8, **kw),
             "deblock + origin": lambda: net.upscale_video(u8, deblock_origin=ORIGIN, **kw),
             "deblock + grid auto": lambda: net.upscale_video(u8, deblock_grid="auto", **kw)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        del r
        return time.perf_counter() - t0
    assert torch.equal(calls["deblock + grid auto"](), net.upscale_video(u8, **kw, **verdict.kwargs()))          # warm-up, and the property
    wall(calls["deblock"])
    wall(calls["deblock + origin"])
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"{n} blocky frames 180x320 x{scale:g}, uint8 in and out, strong, the grid at ({ORIGIN[0]}, {ORIGIN[1]})",
           "verdict": {"block": verdict.block, "origin": verdict.origin},
           "fps": {k: round(n / med[k], 3) for k in calls}, "fps_rounds": {k: [round(n / v, 3) for v in t[k]] for k in calls},
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in calls},
           "time_vs_deblock": {k: round(med[k] / med["deblock"], 4) for k in calls}}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (or the library's path)")
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
    res = {"board": f"{a.board}: {board}", "lease": a.lease, "rounds": a.rounds, "launches": a.launches, "parent": bool(a.parent)}
    with torch.no_grad():
        if "kernels" in a.only:
            res["grid_stats"], res["deblock"] = time_kernels(dev, a.rounds, a.launches, a.parent)
        if "end2end" in a.only:
            res["end2end"] = time_end2end(dev, a.scale, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
