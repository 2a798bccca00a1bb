"""A/B of the precision modes on BASELINE config 2 (7x3x180x320 -> 720x1280, synthetic weights seed 0): one-clip latency and throughput at
16 clips per step (forward_many, as the bench line), in interleaved fp32 / fp16 rounds in one process, plus the fp16 drift and dPSNR-Y of
the output against the fp32 output on a synthetic GT (tests/precision_cases.py).  Writes profiles/bench_precision.json.

    python tools/bench_precision.py [--rounds 4] [--lease NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.archs.savsr_arch import SAVSR  # noqa: E402
from savsr_amd.utils import synth  # noqa: E402
from tests.precision_cases import psnr_y, synth_gt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--lease", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_precision.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = SAVSR().eval()
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net = net.to(dev)
    net.set_scale((4, 4))
    lq = synth.synth_clip(7, 3, 180, 320, seed=0).to(dev)
    clips = [synth.synth_clip(7, 3, 180, 320, seed=i)[0].to(dev) for i in range(16)]
    outs = {}
    for mode in ("fp32", "fp16"):                       # warm-up: images, captures
        net.set_precision(mode)
        outs[mode] = net(lq)[0].cpu().numpy()
        net.forward_many(clips, [(4, 4)] * 16)
    torch.cuda.synchronize()

    def lat(n=10):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            net(lq)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3

    def thr(n=3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            net.forward_many(clips, [(4, 4)] * 16)
        torch.cuda.synchronize()
        return 16 * n * 720 * 1280 / (time.perf_counter() - t) / 1e6

    res = {m: {"latency_ms": [], "hr_mpix_s": []} for m in ("fp32", "fp16")}
    for r in range(a.rounds):
        for mode in (("fp32", "fp16") if r % 2 == 0 else ("fp16", "fp32")):
            net.set_precision(mode)
            res[mode]["latency_ms"].append(lat())
            res[mode]["hr_mpix_s"].append(thr())
    d = np.abs(outs["fp16"].astype(np.float64) - outs["fp32"])
    gt = synth_gt(outs["fp32"])
    summary = {
        "lease": a.lease, "config": "2: 7x3x180x320 -> 720x1280, synthetic weights seed 0", "rounds": res,
        "speedup_latency": float(np.median(res["fp32"]["latency_ms"]) / np.median(res["fp16"]["latency_ms"])),
        "speedup_throughput": float(np.median(res["fp16"]["hr_mpix_s"]) / np.median(res["fp32"]["hr_mpix_s"])),
        "fp16_vs_fp32_max_abs": float(d.max()), "fp16_vs_fp32_mean_abs": float(d.mean()),
        "dpsnr_y_db": psnr_y(outs["fp16"], gt) - psnr_y(outs["fp32"], gt),
    }
    print(json.dumps(summary))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f)


if __name__ == "__main__":
    main()
