"""num_in_ch != 3 checkpoints (the width-generic SATU writing 9 num_in_ch planes, savsr_satu_nf_hr_planes + savsr_tail_gather_nch) against
the default 3-channel one (the tuned SATU) on the headline shape: one-clip and throughput-flow HR Mpixel/s, the SATU stage time from the
engine's `satu_events`, and the SATU LR / HR / tail launches timed alone.

    python3 tools/bench_channels.py [--configs 3:64 1:64 --h 180 --w 320 --scale 4 4 --steps 20 --warmup 5 --clips 3 --out profiles/bench_channels.json]

One JSON line per num_in_ch:num_feat configuration on stdout (and in --out).  Synthetic key-seeded weights: speed does not depend on the values.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from savsr_amd.archs.savsr_arch import SAVSR  # noqa: E402
from savsr_amd.packing import get_hw  # noqa: E402
from savsr_amd.utils import synth  # noqa: E402


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps          # ms per call


def bench(nch, nf, a, dev):
    net = SAVSR(num_in_ch=nch, num_feat=nf)
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    sc = tuple(a.scale)
    net.set_scale(sc)
    H, W = get_hw(a.h, a.w, sc)
    one = synth.synth_clip(7, nch, a.h, a.w, seed=1).to(dev)
    many = torch.cat([synth.synth_clip(7, nch, a.h, a.w, seed=s) for s in range(a.clips)], 0).to(dev)
    with torch.no_grad():
        ms1 = _timed(lambda: net(one), a.steps, a.warmup)
        msb = _timed(lambda: net(many), a.steps, a.warmup)
        eng = net.engine()
        eng.satu_events = []
        for _ in range(a.steps):
            net(one)
        torch.cuda.synchronize()
        satu_us = 1e3 * sum(e0.elapsed_time(e1) for e0, e1, _ in eng.satu_events) / sum(n for _, _, n in eng.satu_events)
        eng.satu_events = None

        def timer(fn):
            return 1e3 * _timed(fn, 20, 3)
        parts = eng.time_satu_parts(one[0], sc, timer)
    return {"num_in_ch": nch, "num_feat": nf,
            "satu_kernels": "tuned (satu.hip)" if (nch, nf) == (3, 64) else f"savsr_satu_nf_* (width-generic, {9 * nch} planes)",
            "lr": [a.h, a.w], "hr": [H, W], "scale": list(sc),
            "one_clip_ms": round(ms1, 3), "one_clip_hr_mpix_s": round(H * W / (1e3 * ms1), 2),
            "throughput_clips": a.clips, "throughput_ms": round(msb, 3), "throughput_hr_mpix_s": round(a.clips * H * W / (1e3 * msb), 2),
            "satu_stage_us_per_clip": round(satu_us, 1), **{k: round(v, 1) for k, v in parts.items()},
            "device": torch.cuda.get_device_name(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=180)
    ap.add_argument("--w", type=int, default=320)
    ap.add_argument("--scale", type=float, nargs=2, default=[4, 4])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clips", type=int, default=3)
    ap.add_argument("--configs", nargs="+", default=["3:64", "1:64"], help="num_in_ch:num_feat pairs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for c in a.configs:
        nch, nf = (int(v) for v in c.split(":"))
        r = bench(nch, nf, a, dev)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
