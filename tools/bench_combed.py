"""combed=: what savsr_video_comb_windows_u8 / _u16 and savsr_video_deinterlace_masked_u8 / _u16 cost beside the kernels they stand next
to, and what upscale_video(pulldown=..., combed=...) adds on clean telecined film, where nothing is flagged (the pure overhead).

  kernels   16 frames of one plane at 480 x 720 and at 1080 x 1920, 8 and 10 bits: the comb call beside savsr_video_field_scores_* (the
            match's measure on the same frames), and the masked deinterlacer with no flag, every flag and every second flag set, for
            both methods, beside savsr_video_deinterlace_*_m at rate 1 (every frame deinterlaced).  One process, interleaved rounds, each
            reading a HIP-event pair around --launches back-to-back calls, --rounds times; medians and the rounds.  GB/s count the bytes
            HBM must move: the comb call reads every plane once; a score call every plane once plus the second-field rows (half a
            plane) of its predecessor; a copied frame is read once and written once; a deinterlaced frame reads three frames and
            writes one.
  end2end   telecine of a 24-frame film: 30 video frames of 180 x 320, x4, uint8 in and out.  pulldown="tff" with and without
            combed="bwdif", interleaved, in input frames per second, and remove_pulldown's own time with and without it.

Numbers are recorded, not gated.

    python3 tools/bench_combed.py [--rounds 5 --launches 50 --scale 4 --out profiles/bench_combed.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N_FRAMES = 16
FILM_FRAMES = 24
SLOWER_NOTE = ("the comb call reads fewer bytes than the score call but does more per byte: the score is a sum, so a dword of four samples is "
               "three v_sad_u8; the comb rule compares every sample's own measure with the threshold, so each of a chunk's 16 samples is "
               "unpacked and compared on its own (three bit-field extracts, three absolute differences, a compare), followed by two popcounts "
               "and up to two LDS adds per row piece, a second pass over the LDS cells for the window sums, and the halo (one cell row in nine "
               "and one cell column per tile are counted twice)")


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
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    flag_sets = {"none": [0] * n, "half": [k % 2 for k in range(n)], "all": [1] * n}
    for h, w in ((480, 720), (1080, 1920)):
        for depth in (8, 10):
            s = 1 if depth == 8 else 2
            fb = h * w * s
            if depth == 8:
                src = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device=dev)
            else:
                src = torch.randint(0, 1024, (n, h * w), dtype=torch.int16, device=dev).view(torch.uint8).reshape(n, fb)
            dst = torch.empty_like(src)
            cells = torch.empty(n, 2, dtype=torch.int64, device=dev)
            flags = {k: torch.tensor(v, dtype=torch.int32, device=dev) for k, v in flag_sets.items()}
            p, d, c = src.data_ptr(), dst.data_ptr(), cells.data_ptr()
            if depth == 8:
                calls = {"field_scores": lambda: lib.savsr_video_field_scores_u8(p, n, fb, 0, h, w, 0, 0, n, c, st),
                         "comb_windows": lambda: lib.savsr_video_comb_windows_u8(p, n, fb, 0, h, w, 1, 0, 0, n, 9, c, st)}
                for mid, method in enumerate(("yadif", "bwdif")):
                    calls[f"deinterlace_m same {method}"] = lambda mid=mid: lib.savsr_video_deinterlace_u8_m(p, n, fb, 0, h, w, 1, 0, 0, n, d, fb, 0, mid, 1, st)
                    for k, t in flags.items():
                        calls[f"deinterlace_masked {method} flags {k}"] = (
                            lambda mid=mid, t=t: lib.savsr_video_deinterlace_masked_u8(p, n, fb, 0, h, w, 1, 0, 0, n, d, fb, 0, mid, t.data_ptr(), st))
            else:
                calls = {"field_scores": lambda: lib.savsr_video_field_scores_u16(p, n, fb, 0, h, w, depth, 0, 0, n, c, st),
                         "comb_windows": lambda: lib.savsr_video_comb_windows_u16(p, n, fb, 0, h, w, depth, 0, 0, n, 9, c, st)}
                for mid, method in enumerate(("yadif", "bwdif")):
                    calls[f"deinterlace_m same {method}"] = (
                        lambda mid=mid: lib.savsr_video_deinterlace_u16_m(p, n, fb, 0, h, w, depth, 0, 0, n, d, fb, 0, mid, 1, st))
                    for k, t in flags.items():
                        calls[f"deinterlace_masked {method} flags {k}"] = (
                            lambda mid=mid, t=t: lib.savsr_video_deinterlace_masked_u16(p, n, fb, 0, h, w, depth, 0, 0, n, d, fb, 0, mid, t.data_ptr(), st))
            moved = {"field_scores": n * fb + (n - 1) * fb // 2, "comb_windows": n * fb}
            for name in calls:
                if name.startswith("deinterlace"):
                    k = sum(flag_sets[name.split()[-1]]) if "masked" in name else n
                    moved[name] = k * 4 * fb + (n - k) * 2 * fb          # (three frames read, one written; a copy reads one and writes one)
            for name, fn in calls.items():          # warm-up, and the return codes once
                _lib.check(fn(), name)
            torch.cuda.synchronize()
            us = {name: [] for name in calls}
            for _ in range(rounds):
                for name, fn in calls.items():
                    us[name].append(timed(fn, launches))
            med = {name: statistics.median(v) for name, v in us.items()}
            for name in calls:
                beside = "field_scores" if name == "comb_windows" else ("deinterlace_m same " + name.split()[1] if "masked" in name else None)
                row = {"size": [h, w], "depth": depth, "n": n, "call": name, "us_per_call": round(med[name], 2),
                       "us_rounds": [round(v, 2) for v in us[name]], "spread": round((max(us[name]) - min(us[name])) / med[name], 4),
                       "bytes_moved": moved[name], "gb_s": round(moved[name] / med[name] / 1e3, 1)}
                if beside is not None:
                    row["beside"], row["time_vs_beside"] = beside, round(med[name] / med[beside], 4)
                out.append(row)
                print(json.dumps(row), flush=True)
    return out


def time_end2end(dev, scale, rounds):
    import numpy as np
    import torch
    import savsr_amd
    from bench_pulldown import film
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
    recovered, info = savsr_amd.remove_pulldown(u8, "tff", return_info=True, combed="bwdif")
    exact = bool(np.array_equal(recovered.cpu().numpy(), frames))
    calls = {"pulldown": lambda: net.upscale_video(u8, scale=scale, out="uint8", pulldown="tff"),
             "pulldown combed": lambda: net.upscale_video(u8, scale=scale, out="uint8", pulldown="tff", combed="bwdif"),
             "remove_pulldown": lambda: savsr_amd.remove_pulldown(u8, "tff"),
             "remove_pulldown combed": lambda: savsr_amd.remove_pulldown(u8, "tff", combed="bwdif")}

    def wall(fn, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        del r
        return (time.perf_counter() - t0) / reps
    assert torch.equal(calls["pulldown combed"](), calls["pulldown"]())          # warm-up; nothing is flagged, so the bytes are the same
    for k in ("remove_pulldown", "remove_pulldown combed"):
        wall(calls[k])
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn, 20 if k.startswith("remove") else 1))          # (a call of half a millisecond: 20 per reading)
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"telecine of a {FILM_FRAMES}-frame film: {n} video frames 180x320 x{scale:g}, uint8 in and out; clean film: nothing is flagged",
           "film_recovered_exactly": exact, "flagged": len(info["combed"]), "largest_window": int(info["comb"][:, 0].max()),
           "input_fps": {k: round(n / med[k], 3) for k in ("pulldown", "pulldown combed")},
           "input_fps_rounds": {k: [round(n / v, 3) for v in t[k]] for k in ("pulldown", "pulldown combed")},
           "combed_vs_plain_time": round(med["pulldown combed"] / med["pulldown"], 4),
           "spread": {k: round((max(t[k]) - min(t[k])) / med[k], 4) for k in calls},
           "remove_pulldown_ms": {k: round(1e3 * med[k], 3) for k in ("remove_pulldown", "remove_pulldown combed")},
           "combed_overhead_ms": round(1e3 * (med["remove_pulldown combed"] - med["remove_pulldown"]), 3)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--only", default="kernels,end2end")
    ap.add_argument("--board", default="MI355X", help="the board's name for the record (the driver reports a generic one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    board = f"{props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, {props.total_memory >> 30} GiB)"
    res = {"board": f"{a.board}: {board}", "rounds": a.rounds, "launches": a.launches}
    with torch.no_grad():
        if "kernels" in a.only:
            res["kernels"] = time_kernels(dev, a.rounds, a.launches)
            ratios = [r["time_vs_beside"] for r in res["kernels"] if r["call"] == "comb_windows"]
            res["note"] = (f"comb_windows takes {min(ratios):g} .. {max(ratios):g} of field_scores' time on the same frames"
                           + (": " + SLOWER_NOTE if max(ratios) > 1 else ""))
        if "end2end" in a.only:
            res["end2end"] = time_end2end(dev, a.scale, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
