"""The self-ensemble (SAVSR.set_self_ensemble) on BASELINE config 2 (7x3x180x320 -> 720x1280 at x4, key-seeded weights seed 0), in one
process, plain single pass against x8:

  latency_ms         one clip, net(lq)                                         (median over --rounds, plain and x8 alternating)
  hr_mpix_s          16 clips, net.forward_many(clips): HR output pixels / s   (x8: the ensemble's output pixels, not the 8 variants')
  orientation_ms     device time per clip of the throughput flow for 16 clips of the plain (180x320) and of the transposed (320x180)
                     orientation alone (HIP events around forward_many): what the 4 transposed variants of the ensemble cost against
                     the 4 plain ones
  kernels            savsr_ensemble_gather_u8 / _f32 (one 7-frame window, plain and transposed variant) and savsr_ensemble_merge
                     (fp32 and uint8 out): us per call over 50 back-to-back calls, merge bytes (8 reads + 1 write) / time against 8 TB/s
  hr_plans           whether savsr_amd/hr_plans.json holds an entry for each scale of the YAML lists and for its swapped pair

    python3 tools/bench_ensemble.py [--rounds 3] [--lease <name>] [--out <file.json>]
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
import torch  # noqa: E402

from savsr_amd import _lib  # noqa: E402
from savsr_amd.archs.savsr_arch import SAVSR  # noqa: E402
from savsr_amd.packing import get_hw  # noqa: E402
from savsr_amd.utils import synth  # noqa: E402

HBM_BYTES_PER_S = 8e12
H_LR, W_LR, SC, NCLIP = 180, 320, (4.0, 4.0), 16


def timed_us(fn, iters=50):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def kernel_rows(dev):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    u8 = torch.randint(0, 256, (7, H_LR, W_LR, 3), dtype=torch.uint8, device=dev)
    f32 = torch.rand(7, 3, H_LR, W_LR, device=dev)
    idx = (C.c_int32 * 7)(*range(7))
    out = torch.empty(7, 3, H_LR, W_LR, device=dev)
    for name, src, fn in (("gather_u8", u8, lib.savsr_ensemble_gather_u8), ("gather_f32", f32, lib.savsr_ensemble_gather_f32)):
        for k in (0, 3, 4, 7):
            us = timed_us(lambda: _lib.check(fn(src.data_ptr(), 7, 3, H_LR, W_LR, idx, 7, k, out.data_ptr(), st), name))
            nbytes = src.numel() * src.element_size() + out.numel() * 4
            rows.append({"kernel": "savsr_ensemble_" + name, "k": k, "us": round(us, 2), "hbm_frac": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3)})
    H, W = get_hw(H_LR, W_LR, SC)
    outs = [torch.rand(3, W, H, device=dev) if k >> 2 else torch.rand(3, H, W, device=dev) for k in range(8)]
    ptrs = [o.data_ptr() for o in outs]
    base = min(ptrs)
    offs = (C.c_int64 * 8)(*[(p - base) // 4 for p in ptrs])
    for u8_out in (0, 1):
        o = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if u8_out else torch.empty(3, H, W, device=dev)
        us = timed_us(lambda: _lib.check(lib.savsr_ensemble_merge(base, offs, 3, H, W, u8_out, o.data_ptr(), st), "merge"))
        nbytes = 8 * 3 * H * W * 4 + o.numel() * o.element_size()
        rows.append({"kernel": "savsr_ensemble_merge", "out": "uint8" if u8_out else "fp32", "hr": [H, W], "us": round(us, 2),
                     "mb": round(nbytes / 1e6, 2), "hbm_frac": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3)})
    return rows


def plan_coverage(net):
    from tests.golden_cases import YAML_SCALES
    table = net.engine()._hr_table
    asym = sorted({tuple(map(float, s)) for s in YAML_SCALES if s[0] != s[1]})
    sym = sorted({tuple(map(float, s)) for s in YAML_SCALES if s[0] == s[1]})
    return {"table_entries": len(table),
            "symmetric_with_plan": sum(s in table for s in sym), "symmetric": len(sym),
            "asymmetric": [{"scale": list(s), "plan": s in table, "swapped_plan": (s[1], s[0]) in table} for s in asym]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lease", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = SAVSR().eval()
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net = net.to(dev)
    net.set_scale(SC)
    H, W = get_hw(H_LR, W_LR, SC)
    lq = synth.synth_clip(7, 3, H_LR, W_LR, seed=0).to(dev)
    clips = [synth.synth_clip(7, 3, H_LR, W_LR, seed=i)[0].to(dev) for i in range(NCLIP)]
    clips_t = [c.transpose(-1, -2).contiguous() for c in clips]
    for on in (False, True):                            # warm-up: every capture of both flows and both orientations
        net.set_self_ensemble(on)
        net(lq)
        net.forward_many(clips, [SC] * NCLIP)
    net.set_self_ensemble(False)
    net.forward_many(clips_t, [SC] * NCLIP)
    torch.cuda.synchronize()

    def lat(n=5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            net(lq)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3

    def thr(n=2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            net.forward_many(clips, [SC] * NCLIP)
        torch.cuda.synchronize()
        return NCLIP * n * H * W / (time.perf_counter() - t) / 1e6

    def dev_ms(cl, n=2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            net.forward_many(cl, [SC] * NCLIP)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (n * NCLIP)

    res = {m: {"latency_ms": [], "hr_mpix_s": []} for m in ("plain", "x8")}
    orient = {"plain_180x320": [], "transposed_320x180": []}
    for r in range(a.rounds):
        for mode in (("plain", "x8") if r % 2 == 0 else ("x8", "plain")):
            net.set_self_ensemble(mode == "x8")
            res[mode]["latency_ms"].append(round(lat(), 3))
            res[mode]["hr_mpix_s"].append(round(thr(), 2))
        net.set_self_ensemble(False)
        orient["plain_180x320"].append(round(dev_ms(clips), 3))
        orient["transposed_320x180"].append(round(dev_ms(clips_t), 3))
    med = lambda v: statistics.median(v)      # noqa: E731
    summary = {
        "lease": a.lease, "config": "2: 7x3x180x320 -> 720x1280 x4, synthetic weights seed 0", "rounds": res,
        "latency_ms": {m: med(res[m]["latency_ms"]) for m in res}, "hr_mpix_s": {m: med(res[m]["hr_mpix_s"]) for m in res},
        "x8_cost_latency": med(res["x8"]["latency_ms"]) / med(res["plain"]["latency_ms"]),
        "x8_cost_throughput": med(res["plain"]["hr_mpix_s"]) / med(res["x8"]["hr_mpix_s"]),
        "orientation_ms_per_clip": {k: med(v) for k, v in orient.items()}, "orientation_rounds": orient,
        "kernels": kernel_rows(dev), "hr_plans": plan_coverage(net),
    }
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
