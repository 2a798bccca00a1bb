#!/usr/bin/env python3
"""SAVSR hot-path benchmark on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 5                  # BASELINE config 2 (the judged line)
    python bench.py --config 3 | 4 | 5 ...                          # the arbitrary-scale configs (same JSON contract)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Config 2 (default): a "step" is one pass of the hot path (SAVSR.forward) over one batch of `--clips-per-step` synthetic
7x3x180x320 clips already resident in HBM, scale x4 -> 720x1280 (16 clips: two HIP streams x four clips per launch sequence x two units), followed by
the GPU PSNR-Y / SSIM-Y of every output frame against a synthetic ground truth.  Clips are independent, so for N > 1
every rank runs its own K steps (weak scaling, no data-path collective); the only collective is ONE RCCL all_gather of the
per-frame [PSNR-Y, SSIM-Y] rows, as the reference reduces its metric tensor once per dataset
(video_base_model.py:108-113).  Rank 0 prints ONE JSON line.  `--steps K` is the number of timed steps: they run in up to `--regions`
back-to-back timed regions and `value` is the median region's rate.  `--dump-outputs DIR` writes what the last timed step returned
(rank 0's; `dump_outputs`).

`--config run_test`: the YAML workflow (savsr_amd.test.run_test = lbasicsr/test.py:11-48) on a synthetic Vid4-shaped PNG tree
(4 folders x `--frames-per-folder` frames, 6 datasets = 6 scales over ONE dataroot_gt, checkpoint through torch.save): frames/s of
the whole job incl. PNG decode, upload, LR synthesis, network, metrics; GPU-busy fraction; the same frames through the network
alone for comparison.

`--gpus N` without a torch.distributed environment: this process starts the N ranks itself (fresh children through
`python -m torch.distributed.run`, before anything here touches a GPU), relays rank 0's line and exits with the launcher's code.

Config 3: the 30 symmetric Vid4 scales x1.1 ... x4.0 at LR 180x320 (batch 1, as the reference's test flow); config 4: the
UDM10 asymmetric shapes (LR 480x318 x(1.5, 4), LR 204x636 x(3.5, 2)); config 5: a seeded stream of Vimeo90K training
(shape, scale) pairs.  Their lines carry per-scale / per-shape figures (`per_case`) next to the aggregate `value`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

from savsr_amd.utils.host import cpu_model, effective_cpus  # noqa: E402

LR_H, LR_W, SCALE = 180, 320, (4, 4)
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_BF16_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: dense bf16 matrix peak (sustained under load: ~1870, tools/micro/mfma_rate.hip)
MAC_PER_LR_PX = 22.99e6          # algorithmic MACs of the network, reference formulation
MAC_PER_HR_PX = 19.9e3
DTYPE = "f32 (bf16x3 split products, fp32 accumulate)"
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "satu_traffic.json")     # PMC-measured HBM bytes of the SATU launches (tools/pmc_summary.py)


def cpu_baseline(sd, threads):
    """Oracle (CPU restatement of the reference path, kind='port') on a bounded sample of the same
    workload: whole 7x3x180x320 -> 720x1280 frames until ~12 s of CPU time are spent (>= 1 frame),
    after one untimed quarter-area warm-up that pages the weights in."""
    from oracle import savsr_oracle as O
    from savsr_amd.utils import synth
    torch.set_num_threads(threads)
    lq = synth.synth_clip(7, 3, LR_H, LR_W, seed=0)
    with torch.no_grad():
        O.forward(sd, lq[..., :90, :160].contiguous(), SCALE)
        n, t0 = 0, time.perf_counter()
        while True:
            out = O.forward(sd, lq, SCALE)
            n += 1
            dt = time.perf_counter() - t0
            if dt > 12.0 or n >= 8:
                break
    hr_px = n * out.shape[-1] * out.shape[-2]
    return {"value": round(hr_px / dt / 1e6, 5), "unit": "HR Mpixel/s", "cores": threads, "cpu_model": cpu_model(), "kind": "port",
            "sample": f"{n} frame(s) of the workload clip (7x3x180x320, x4 -> 720x1280) through oracle/savsr_oracle.py, {dt:.2f} s"}, out, lq


def sysfs_device_dir(dev=None):
    """sysfs directory of the GPU this process runs on (by PCI address: a node has eight cards and card0 is rarely ours); None if unknown."""
    import glob
    try:
        pr = torch.cuda.get_device_properties(dev if dev is not None else torch.cuda.current_device())
        d = "/sys/bus/pci/devices/%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        if os.path.isdir(d):
            return d
    except (AttributeError, RuntimeError, AssertionError):
        pass
    cards = sorted(glob.glob("/sys/class/drm/card*/device"))
    return cards[0] if len(cards) == 1 else None


def sysfs_sclk_mhz(dev=None):
    """Current shader-clock level the driver reports (pp_dpm_sclk, the line marked '*'); None where sysfs is not readable.  Not the
    clock a loaded kernel holds (MI355X_MICROARCH.md, DVFS give-back item 6): reported beside the in-kernel probe."""
    d = sysfs_device_dir(dev)
    try:
        for ln in open(os.path.join(d, "pp_dpm_sclk")):
            if "*" in ln:
                return int(ln.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
    except (OSError, ValueError, IndexError, TypeError):
        pass
    return None


def sysfs_power_w(dev=None):
    """(socket power now, power cap) in W from the card's hwmon (power1_input / power1_average, power1_cap: microwatts); None where unreadable."""
    import glob
    d = sysfs_device_dir(dev)
    if not d:
        return None, None
    out = []
    for name in (("power1_input", "power1_average"), ("power1_cap",)):
        v = None
        for n in name:
            for f in glob.glob(os.path.join(d, "hwmon", "hwmon*", n)):
                try:
                    v = int(open(f).read().strip()) / 1e6
                except (OSError, ValueError):
                    continue
            if v is not None:
                break
        out.append(v)
    return out[0], out[1]


class PowerSampler:
    """Socket power sampled every 50 ms by a host thread while some load runs (the hwmon figure is the driver's own running average)."""

    def __init__(self, dev):
        import threading
        self.dev, self.samples, self.stop_flag = dev, [], threading.Event()
        self.thread = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self.stop_flag.is_set():
            w, _ = sysfs_power_w(self.dev)
            if w is not None:
                self.samples.append(w)
            self.stop_flag.wait(0.05)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop_flag.set()
        self.thread.join()


class ClockProbe:
    """savsr_clock_probe on a side stream: one wave reads s_memtime / s_memrealtime around `ms` of wall time; launched just before
    some load is enqueued on the main stream it reports the shader clock the chip holds under that load."""

    def __init__(self, eng, dev):
        self.lib, self.dev = eng.lib, dev
        self.stream = torch.cuda.Stream(device=dev, priority=-1)      # (its own hardware queue: a default-priority side stream can share one with a compute stream and then runs BEFORE the load, not beside it)
        self.windows = 8
        self.buf = torch.zeros(2 * self.windows, dtype=torch.int64, device=dev)

    def start(self, ms):
        self.buf.zero_()
        torch.cuda.synchronize()
        rc = self.lib.savsr_clock_probe(self.buf.data_ptr(), max(1, int(ms * 1e5 / self.windows)), self.windows, self.stream.cuda_stream)
        assert rc == 0, rc

    def mhz(self):
        """Median and range over the probe's windows (the first window may start before the load does)."""
        self.stream.synchronize()
        v = self.buf.cpu().view(self.windows, 2).tolist()
        mhz = sorted(100.0 * c / r for c, r in v if r > 0)
        if not mhz:
            return None
        self.last_range = [round(mhz[0], 1), round(mhz[-1], 1)]
        return round(mhz[len(mhz) // 2], 1)


def conv_roofline(eng, dev, iters=20, probe=None):
    """The kernel that dominates GPU time (conv_bf16x3_kernel, ~85 % of a frame) on its most frequent launch
    geometry: one savsr_conv2d_batch of six 128->64 3x3 convs at 180x320 with bias, LeakyReLU and a residual
    (the ResidualBlock conv2 launches, savsr_arch.py:412-414; 20 of them per frame).  HIP events on the launch
    stream.  The frame's launches replay inside a hipGraph, which cannot hold timing events, so this times the
    same launch right after the timed region; the rocprofv3 summary of the bench command holds the in-graph
    average of this kernel (profiles/)."""
    from savsr_amd import engine as E
    from savsr_amd._lib import ACT_LRELU
    g = torch.Generator().manual_seed(1)
    n, cin, cout = 6, 128, 64
    keep, descs = [], []
    wy = bool(getattr(eng, "conv_wy", False))
    for k in range(n):
        wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
        weights = (E.pack_conv_weight(wt).to(dev), torch.randn(cout, generator=g).to(dev), cout, cin, 3)
        if wy:                                              # the engine's own path: both images registered, conv_launch picks the form per launch
            eng.pw[f"bench.{k}"] = weights
            eng.pw_wy[f"bench.{k}"] = E.pack_conv_weight_wy(wt).to(dev)
        xs = [torch.randn(LR_H, LR_W, 64, generator=g).to(dev) for _ in range(2)]
        res, out = torch.randn(LR_H, LR_W, cout, generator=g).to(dev), torch.empty(LR_H, LR_W, cout, device=dev)
        keep.append((weights, xs, res, out))
        descs.append(eng.conv_desc(f"bench.{k}", [eng.full(x) for x in xs], eng.full(out), LR_H, LR_W, ACT_LRELU, 0.2,
                                   res1=eng.full(res), weights=None if wy else weights))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        eng.conv_launch(descs)
    ev0.record()
    for _ in range(iters):
        eng.conv_launch(descs)
    ev1.record()
    torch.cuda.synchronize()
    sec = ev0.elapsed_time(ev1) / 1e3 / iters
    clock = None
    if probe is not None:                                   # the clock the chip holds under this launch, looped (~40 ms)
        nloop = max(iters, int(0.04 / sec))
        probe.start(0.6 * nloop * sec * 1e3)
        for _ in range(nloop):
            eng.conv_launch(descs)
        torch.cuda.synchronize()
        clock = probe.mhz()
    alg = 2.0 * n * cin * cout * 9 * LR_H * LR_W            # fp32-equivalent flops (2 x MACs)
    direct_eq = 3.0 * alg                                   # split-bf16 direct form: three bf16 MFMA products per fp32 product
    form = int(descs[0].algo)
    is_wy = form == 3
    # MFMAs the launch really issues (v_mfma_f32_32x32x16_bf16 = 32768 flop): per 32-px column block, ROW PAIR (waves below the image run an
    # MFMA-free body), 16-channel phase and 64 output channels 108 in the direct form (9 taps x 2 rows x 2 channel blocks x 3 products), 72 in
    # the Winograd-y form (12 taps for the two rows).  6 x 128->64 at 180x320: 3.1104 M = the PMC count (profiles/r04_conv_wy_pmc_summary.csv: 3.110 M)
    n_mfma = n * ((LR_W + 31) // 32) * ((LR_H + 1) // 2) * (cin // 16) * (cout // 64) * (72 if is_wy else 108)
    issued = n_mfma * 32768.0
    r = {"kernel": ("conv_wy_kernel (Winograd F(2,3) along y" if is_wy else "conv_bf16x3_kernel<3,2,2> (direct") +
                   "; 6 x conv3x3 128->64 + bias + LeakyReLU + residual, 180x320)", "bound": "mfma",
         "achieved": round(issued / sec / 1e12, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(issued / sec / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4),
         "traffic": None, "issued_mfma": n_mfma, "issued_flops": issued,
         "direct_equivalent_tflops": round(direct_eq / sec / 1e12, 1), "direct_equivalent_frac": round(direct_eq / sec / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4),
         "algorithmic_flops": alg, "fp32_equivalent_tflops": round(alg / sec / 1e12, 1), "algorithmic_frac": round(alg / sec / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4),
         "avg_ms": round(1e3 * sec, 4), "clock_mhz_under_launch": clock,
         "note": "achieved / frac = bf16 MFMA flops the launch ISSUES (issued_mfma x 32768; the instruction count is the PMC's) / time"
                 + ("; direct_equivalent_* = what the same conv work costs in the direct split-bf16 form (3 products per MAC), the figure rounds 1-4 reported as "
                    "frac; the Winograd form issues 2/3 of it" if is_wy else "") + "; algorithmic_* = 2 x MACs (fp32-equivalent); launch timed solo after the timed region"}
    return r


def time_events(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters       # us


def satu_alg_bytes(h, w, H, W):
    return 4 * 64 * (2 * h * w + H * W)             # read x, st once + write out once


def satu_roofline(eng, clip, h, w, scale, in_flight_ms=None):
    """SATU stage (LR + HR launches of the product path) vs the HBM roofline, SURVEY 8(d)'s contract figure:
    achieved = 4 C (2 h w + H W) bytes / launch time.  `frac` is the figure of the launches ALONE on the GPU (HIP events on
    the launch stream, each kernel looped); `in_flight_*` the event-bracketed time inside the timed region, where the other
    in-flight clips' kernels share the GPU."""
    from savsr_amd.engine import get_hw
    H, W = get_hw(h, w, scale)
    parts = eng.time_satu_parts(clip, scale, time_events)
    t = (parts["satu_lr_us"] + parts["satu_hr_us"]) * 1e-6
    alg = satu_alg_bytes(h, w, H, W)
    achieved = alg / t / 1e9
    traffic, src, traffic_note = None, None, None
    lib_hash = eng.lib.savsr_source_hash_satu().decode()
    try:
        tr = json.load(open(TRAFFIC_FILE))
        if tr.get("lib_source_hash") == lib_hash:
            traffic, src = tr.get("bytes_per_stage"), tr.get("source")
        else:           # PMC bytes of ANOTHER build say nothing about the library that ran: drop them
            traffic_note = f"profiles/satu_traffic.json was measured on library sources {tr.get('lib_source_hash')}, this run is {lib_hash}: traffic dropped"
    except (OSError, ValueError):
        pass
    r = {"kernel": "SATU = satu_lr_stream_kernel<NB=1> + satu_hr_kernel<NB=1" + (", row-summed" if eng.satu_q else "") + "> (tail-projected form: the 3x3 tail conv's channel "
                   "contraction is folded in" + ("; the HR stage also adds the tail's three horizontal taps and writes 9 planes + seams instead of 27 planes" if eng.satu_q else "")
                   + "; the phase table is evaluated once per size / scale / weights)",
         "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
         "traffic": traffic if (h, w, tuple(scale)) == (LR_H, LR_W, SCALE) else None, "traffic_source": src,
         "algorithmic_bytes": alg, "avg_ms": round(1e3 * t, 4), "lr_us": round(parts["satu_lr_us"], 1), "hr_us": round(parts["satu_hr_us"], 1),
         "tail_gather_us": round(parts["tail_us"], 1),
         "satu_plus_tail_us": round(parts["satu_lr_us"] + parts["satu_hr_us"] + parts["tail_us"], 1),
         "frac_definition": "frac = frac_algorithmic = SURVEY 8(d)'s CONTRACT bytes (x + st read once, the [64,H,W] output written once) / time / peak: a "
                            "figure of merit per HR pixel, NOT achieved bandwidth -- the tail-projected kernels write 27 planes instead of 64 and move "
                            "fewer bytes; moved_frac = PMC-measured HBM bytes of these launches (`traffic`) / time / peak is the bandwidth actually "
                            "achieved (DESIGN.md section 4b)",
         "note": "launches alone on the GPU, each looped on the tensors of a real frame (inputs of 22-29 MB may be served by the 256 MB Infinity "
                 "Cache, as they are in the frame itself, where the previous kernels have just written them)"}
    r["frac_algorithmic"] = r["frac"]
    r["lib_source_hash"] = lib_hash
    if traffic_note:
        r["traffic_note"] = traffic_note
    # SATU + tail against the bytes of the REFERENCE formulation of savsr_arch.py:315-376 + :738-739: SATU's contract bytes + the tail conv
    # reading the [64,H,W] map again and writing [3,H,W] + the centre LR frame of the bilinear residual.  Work moved between the HR launch
    # and the tail launch (the row-summed form) does not change this figure; it does change `frac` (LR + HR only).
    alg_tail = alg + 4 * (64 + 3) * H * W + 12 * h * w
    t_all = t + parts["tail_us"] * 1e-6
    r["satu_tail"] = {"algorithmic_bytes": alg_tail, "us": round(1e6 * t_all, 1), "achieved": round(alg_tail / t_all / 1e9, 1), "unit": "GB/s",
                      "frac": round(alg_tail / t_all / 1e9 / HBM_PEAK_GBS, 4),
                      "definition": "(265.42 MB-form SATU bytes + 4 (64 + 3) H W + 12 h w) / (LR + HR + tail launches alone) / 8 TB/s"}
    if r["frac"] < 0.40:
        # the row-summed form moves the tail's three horizontal taps into the HR launch (+1.8 us there, -10 us in the tail launch).
        r["below_target_note"] = ("frac (LR + HR launches on the contract bytes) reads under 0.40 on this board: the shipped row-summed form does ~1.8 us of the "
                                  "tail's work inside the HR launch (27-plane form: HR 34.7 -> 36.5 us on one lease, tail gather 22.6 -> 12.7 us); satu_tail.frac "
                                  "is the figure that does not depend on where that work runs")
    if r["traffic"]:
        r["moved_gbs"] = round(r["traffic"] / t / 1e9, 1)
        r["moved_frac"] = round(r["traffic"] / t / 1e9 / HBM_PEAK_GBS, 4)
    if in_flight_ms:
        avg = sum(in_flight_ms) / len(in_flight_ms) / 1e3
        r["in_flight_avg_ms"] = round(1e3 * avg, 4)
        r["in_flight_frac"] = round(alg / avg / 1e9 / HBM_PEAK_GBS, 4)
    return r


DUMP_SAMPLE = 1 << 22            # --dump-outputs: elements of the step's output drawn for sr_sample.npy (16 MiB of fp32)
DUMP_LIMIT = 64 << 20


def dump_outputs(dirname, out, rows):
    """--dump-outputs DIR: what the timed path handed back in its last step, for comparing two builds output for output.
      sr_clip0.npy    [3, H, W] fp32: the step's first output frame, whole
      sr_sample.npy   [DUMP_SAMPLE] fp32: out.reshape(-1)[idx] of the whole step output [clips, 3, H, W] (every clip, every unit and stream),
                      idx = np.sort(np.random.RandomState(0).randint(0, out.numel(), DUMP_SAMPLE)) -- the same elements in every run
      psnr_ssim_y.npy [clips, 2] fp64: the GPU PSNR-Y / SSIM-Y rows of the step's frames against the synthetic GT
    The inputs (key-seeded weights, seeded clips and GT) depend on the arguments only."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    torch.cuda.synchronize()
    idx = np.sort(np.random.RandomState(0).randint(0, out.numel(), DUMP_SAMPLE))
    arrays = {"sr_clip0": out[0].float().cpu().numpy(),
              "sr_sample": out.reshape(-1)[torch.from_numpy(idx).to(out.device)].float().cpu().numpy(),
              "psnr_ssim_y": rows.double().cpu().numpy()}
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_LIMIT
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def build_net(dev):
    import savsr_amd
    from savsr_amd.utils import synth
    sd = synth.synth_state_dict(seed=0)                   # random-init weights of the full architecture
    net = savsr_amd.build_network(dict(type="SAVSR", num_in_ch=3, num_feat=64, num_frame=7, slid_win=3, fusion_win=5,
                                       interval=0, w1_num_block=4, w2_num_block=2, n_resgroups=4, n_resblocks=8,
                                       center_frame_idx=None)).eval()
    net.load_state_dict(sd, strict=True)
    net.to(dev)
    return net, sd


def timed(dist, dev, fn):
    """barrier + synchronize | fn() | barrier + synchronize; MAX over ranks."""
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([elapsed], device=dev if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    return elapsed


def base_line(args, world, value, elapsed, workload, extra_cfg):
    cfg = {"workload": workload, "parallelism": f"clip-sharded dp{world}"}
    cfg.update(extra_cfg)
    return {"metric": "HR Mpixels/sec (7-frame window)", "value": round(value, 3), "unit": "HR Mpixel/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": DTYPE, "data": "synthetic", "config": cfg}


# --------------------------------------------------------------------------------------------- config 2
def run_config2(args, rank, world, dev, dist):
    from savsr_amd.metrics_gpu import psnr_ssim_y
    from savsr_amd.utils import synth
    net, sd = build_net(dev)
    net.set_scale(SCALE)
    eng = net.engine()
    eng.census = {}               # matrix work of every conv launch by the form it takes (engine._count_conv), filled while the frames are captured
    H, W = LR_H * SCALE[0], LR_W * SCALE[1]
    cps = max(1, args.clips_per_step)
    n_batches = 2
    # distinct clips per rank, resident in HBM before the timed region
    clips = [torch.cat([synth.synth_clip(7, 3, LR_H, LR_W, seed=1000 * rank + cps * i + j) for j in range(cps)], 0).to(dev)
             for i in range(n_batches)]
    gt = synth.synth_gt(3, H, W, seed=0).to(dev)
    rows = torch.zeros(args.steps * cps, 2, device=dev, dtype=torch.float64)
    gathered = torch.empty(world * args.steps * cps, 2, device=dev, dtype=torch.float64)

    last = {}

    def step(i, record):
        out = net(clips[i % n_batches])
        if record:
            for j in range(cps):              # GPU PSNR-Y / SSIM-Y of every output frame (row f3), rows stay in HBM
                psnr_ssim_y(out[j], gt, 0, out=rows[i * cps + j])
            last["i"], last["out"] = i, out   # (a reference only: --dump-outputs reads it after the timed steps)
        return out

    for i in range(args.warmup):
        step(i, False)
    eng.satu_events = []          # HIP events on the launch stream around the SATU launches (in-flight figure)

    def region(i0, n):
        for i in range(i0, i0 + n):
            step(i, True)
        if dist is not None and i0 + n == args.steps:      # the one collective of the "dataset" (RCCL all_gather over xGMI)
            if dist.get_backend() == "nccl":
                dist.all_gather_into_tensor(gathered, rows)
            else:                 # SAVSR_DIST_BACKEND=gloo (ranks sharing one GPU in a test): the rows take the host path
                lst = [torch.empty(rows.shape, dtype=rows.dtype) for _ in range(world)]
                dist.all_gather(lst, rows.cpu())
                gathered.copy_(torch.cat(lst, 0))
    # Exactly K timed steps, split into up to `--regions` back-to-back regions (K = 20: 7 + 7 + 6 steps), each bracketed by barrier +
    # synchronize with the MAX over ranks; `value` is the MEDIAN region's per-step rate (a lease's shader clock drifts by a few % over
    # seconds; one region cannot tell that from a code change)
    nreg = min(max(1, args.regions), args.steps)
    sizes = [args.steps // nreg + (1 if r < args.steps % nreg else 0) for r in range(nreg)]
    starts = [sum(sizes[:r]) for r in range(nreg)]
    sclk0 = sysfs_sclk_mhz(dev)
    regions = [timed(dist, dev, lambda i0=i0, n=n: region(i0, n)) for i0, n in zip(starts, sizes)]
    sclk1 = sysfs_sclk_mhz(dev)
    per_step = sorted(e / n for e, n in zip(regions, sizes))
    step_s = per_step[len(per_step) // 2]
    elapsed = step_s * args.steps             # the median region's rate over all K steps (ms_per_step = 1e3 x step_s)
    in_flight = [a.elapsed_time(b) / n for a, b, n in eng.satu_events]       # per clip: a batched launch sequence holds several clips' SATU stages
    eng.satu_events = None
    assert last["i"] == args.steps - 1
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, last["out"], rows[last["i"] * cps:(last["i"] + 1) * cps])
    last.clear()
    if rank != 0:
        return
    hr_mpx = H * W / 1e6
    value = world * cps * hr_mpx / step_s
    line = base_line(args, world, value, elapsed, "BASELINE config 2: synthetic 7x3x180x320 clips, scale x4 -> 720x1280, key-seeded random-init weights",
                     {"frames_per_step": cps, "streams_per_gpu": min(cps, eng.streams_for(LR_H * LR_W)), "clips_per_launch_sequence": eng.clip_batch})
    line["config"]["knobs"] = eng.knobs.knobs()          # non-default SAVSR_* switches of the engine (savsr_amd/config.py); empty = product configuration
    line["metric"] = "HR Mpixels/sec (Vid4-shape x4, 7-frame window)"
    line["timed_region_s"] = round(elapsed, 3)           # K steps at the median region's rate
    line["timed_s"] = round(sum(regions), 3)             # all K timed steps
    line["timed_steps_per_region"] = sizes
    vals = sorted(world * cps * hr_mpx / s for s in per_step)
    line["value_min"], line["value_median"], line["value_max"] = round(vals[0], 3), round(vals[len(vals) // 2], 3), round(vals[-1], 3)
    line["region_values"] = [round(world * n * cps * hr_mpx / e, 3) for e, n in zip(regions, sizes)]
    line["regions_note"] = f"{args.steps} timed steps in {nreg} back-to-back regions of {sizes} steps; value = ms_per_step = the median region's"
    probe = ClockProbe(eng, dev)
    probe.start(2.0)
    clock = {"idle_probe": probe.mhz(), "sysfs_sclk_before": sclk0, "sysfs_sclk_after": sclk1}
    probe.start(0.5 * 1e3 * step_s)          # under the frame load: half a step, beside one untimed step
    step(0, False)
    torch.cuda.synchronize()
    clock["under_frame_load"] = probe.mhz()
    # board power under the same load: ~1 s of untimed steps with the hwmon figure sampled every 50 ms (the frame sits at the power cap)
    idle_w, cap_w = sysfs_power_w(dev)
    with PowerSampler(dev) as ps:
        for i in range(max(2, int(round(1.0 / step_s)))):
            step(i, False)
        torch.cuda.synchronize()
    if ps.samples:
        tail = sorted(ps.samples[len(ps.samples) // 2:])          # second half: the running average has caught up with the load
        line["power_w"] = {"under_frame_load": round(tail[len(tail) // 2], 1), "max_sample": round(max(ps.samples), 1), "before": idle_w, "cap": cap_w,
                           "samples": len(ps.samples), "note": "hwmon power1 of this GPU, sampled every 50 ms over ~1 s of untimed steps (median of the second half)"}
    allrows = (gathered if dist is not None else rows).cpu()
    line["psnr_y_vs_synthetic_gt"] = round(float(allrows[:, 0].mean()), 4)
    line["ssim_y_vs_synthetic_gt"] = round(float(allrows[:, 1].mean()), 6)
    # batch-1 flow of the reference (one clip in flight, video_base_model.py:51-53), timed right after the region
    one = clips[0][:1]
    for _ in range(3):
        net(one)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb1 = 30
    for _ in range(nb1):
        net(one)
    torch.cuda.synchronize()
    b1 = (time.perf_counter() - t0) / nb1
    line["batch1_value"] = round(hr_mpx / b1, 3)
    line["batch1_ms_per_frame"] = round(1e3 * b1, 3)
    frame_s = elapsed / (args.steps * cps)
    macs = MAC_PER_LR_PX * LR_H * LR_W + MAC_PER_HR_PX * H * W
    # Matrix-unit utilisation of the whole frame = flops of the bf16 MFMAs the frame ISSUES / frame time / dense bf16 peak.  Issued: the conv
    # launches from the engine's census of the captured frame (3 split products per MAC in the direct form, 2 in the Winograd-y form, on the
    # padded tile grid) + the SATU LR stage's (kernel_conv 64 -> 1600 and the three projections, 3 products per MAC).  Rounds 1-4 reported
    # `whole_frame_direct_equivalent_frac` under this name: 3 products for EVERY MAC of the SURVEY census, executed or not.
    cen = eng.census
    mode = "tp" if cen.get("frames_tp") else "b1"
    nfr = max(1, cen.get("frames_" + mode, 1))
    satu_lr_issued = 3 * 2 * LR_H * LR_W * (1600 * 64 + 96 * 64)
    issued = cen.get("issued_" + mode, 0.0) / nfr + satu_lr_issued
    line["whole_frame_mfma_frac"] = round(issued / frame_s / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4)
    line["whole_frame_direct_equivalent_frac"] = round(3 * 2 * macs / frame_s / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4)
    line["whole_frame_algorithmic_frac"] = round(2 * macs / frame_s / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4)
    line["whole_frame_winograd_share"] = round(cen.get("wy_alg_" + mode, 0.0) / max(cen.get("alg_" + mode, 1.0), 1.0), 4)
    line["whole_frame_note"] = ("whole_frame_mfma_frac = ISSUED bf16 MFMA flops per frame (conv census of the captured frame: 3 products per MAC direct, 2 in the "
                                "Winograd-y form, padded tiles; + SATU LR) / frame time / 2.5 PF; _direct_equivalent_ = 3 x 2 x 1.34 TMAC (SURVEY 8(d)) / time / peak "
                                "(rounds 1-4's figure: counts products the Winograd launches do not execute); _algorithmic_ = 2 x 1.34 TMAC / time / peak; "
                                "winograd_share = share of the conv MACs that ran in the Winograd-y form")
    line["roofline"] = satu_roofline(eng, clips[0][0], LR_H, LR_W, SCALE, in_flight)
    line["roofline_conv"] = conv_roofline(eng, dev, probe=probe)
    clock["under_conv_launch"] = line["roofline_conv"]["clock_mhz_under_launch"]
    clock["note"] = ("in-kernel shader clock = s_memtime / s_memrealtime x 100 MHz read by one wave on a side stream (savsr_clock_probe) while the named load runs; "
                     "sysfs_sclk_* = pp_dpm_sclk before / after the timed regions")
    line["clock_mhz"] = clock
    if world == 1 and not args.no_cpu_baseline:
        threads = effective_cpus()
        cb, ref, lq_c = cpu_baseline(sd, threads)
        # The oracle on the path the headline TIMES: clips[0][0] is the oracle sample's clip (seed 0), so the output of one more step of the timed
        # configuration (b = cps clips: n_streams streams x clip_batch clips per launch sequence, throughput tiling, ~99 % Winograd-y) is compared
        # with it directly; the one-clip latency flow's figure (another tiling, other per-launch form choices) stays beside it under its own name.
        assert torch.equal(clips[0][0].cpu(), lq_c[0]), "clips[0][0] of the timed step is the oracle sample's clip"
        got_t = step(0, False)[0].cpu()
        got_1 = net(lq_c.to(dev))[0].cpu()
        from savsr_amd.metrics import calculate_psnr, calculate_ssim, tensor2img
        gti = tensor2img(gt.cpu())
        m = {k: (calculate_psnr(tensor2img(v), gti, 0, test_y_channel=True), calculate_ssim(tensor2img(v), gti, 0, test_y_channel=True))
             for k, v in (("gpu", got_t), ("oracle", ref[0]))}
        cb["gpu_vs_oracle_max_abs_timed_path"] = float((got_t - ref[0]).abs().max())
        cb["gpu_vs_oracle_max_abs_on_sample"] = cb["gpu_vs_oracle_max_abs_timed_path"]
        cb["gpu_vs_oracle_max_abs_one_clip_flow"] = float((got_1 - ref[0]).abs().max())
        cb["d_psnr_y_timed_path_vs_oracle"] = abs(m["gpu"][0] - m["oracle"][0])
        cb["d_ssim_y_timed_path_vs_oracle"] = abs(m["gpu"][1] - m["oracle"][1])
        cb["timed_path_note"] = (f"clip 0 of a step of the timed configuration ({cps} clips per step, {min(cps, eng.streams_for(LR_H * LR_W))} streams x {eng.clip_batch} clips per launch "
                                 "sequence) against the oracle's output for the same clip; PSNR-Y / SSIM-Y of both against the synthetic GT (host metrics)")
        line["gpu_vs_oracle_max_abs_timed_path"] = cb["gpu_vs_oracle_max_abs_timed_path"]
        line["cpu_baseline"] = cb
    print(json.dumps(line), flush=True)


# --------------------------------------------------------------------------------------------- configs 3 / 4 / 5
def run_cases(args, rank, world, dev, dist, cases, workload, config_id):
    """cases: [(h, w, (sh, sw))]; every rank runs `steps` frames of every case (weak scaling), batch 1 like the reference's
    test flow; per-case HR Mpixel/s + SATU figures, aggregate value = all HR pixels / total time."""
    from savsr_amd.engine import get_hw
    from savsr_amd.utils import synth
    net, sd = build_net(dev)
    eng = net.engine()
    per_case, total_px, total_t = [], 0.0, 0.0
    for (h, w, sc) in cases:
        lq = synth.synth_clip(7, 3, h, w, seed=7 + rank).to(dev)
        net.set_scale(sc)
        H, W = get_hw(h, w, sc)
        for _ in range(max(1, args.warmup)):
            out = net(lq)
        assert tuple(out.shape) == (1, 3, H, W)

        def region():
            for _ in range(args.steps):
                net(lq)
        el = timed(dist, dev, region)
        total_px += world * args.steps * H * W
        total_t += el
        if rank == 0:
            ax = eng.satu_axes(h, w, sc)
            r = satu_roofline(eng, lq[0], h, w, sc)
            per_case.append({"lr": [h, w], "scale": list(sc), "hr": [H, W], "ms_per_frame": round(1e3 * el / args.steps, 3),
                             "hr_mpix_per_s": round(world * args.steps * H * W / el / 1e6, 2), "table_entries": ax["n_uh"] * ax["n_uw"],
                             "satu_lr_us": r["lr_us"], "satu_hr_us": r["hr_us"], "tail_gather_us": r["tail_gather_us"], "satu_frac": r["frac"],
                             "hr_ns_per_hr_px": round(1e3 * r["hr_us"] / (H * W), 4)})
    if rank != 0:
        return
    line = base_line(args, world, total_px / total_t / 1e6, total_t, workload, {"frames_per_case": args.steps, "cases": len(cases), "batch": 1})
    line["config"]["knobs"] = eng.knobs.knobs()          # non-default SAVSR_* switches of the engine (savsr_amd/config.py); empty = product configuration
    line["ms_per_step"] = round(1e3 * total_t / (args.steps * len(cases)), 3)
    line["bench_config"] = config_id
    line["per_case"] = per_case
    x4 = [c for c in per_case if c["scale"] == [4.0, 4.0] or c["scale"] == [4, 4]]
    if x4:
        line["roofline"] = {"bound": "hbm", "achieved": round(x4[0]["satu_frac"] * HBM_PEAK_GBS, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": x4[0]["satu_frac"], "traffic": None, "note": "SATU stage of the x4 case; per-case figures in per_case"}
    print(json.dumps(line), flush=True)


def run_config5(args, rank, world, dev, dist):
    """Vimeo90K-shape mixed-scale throughput: `clips-per-step` x (steps + warmup) (shape, scale) pairs drawn from the 60-entry training list
    (random.Random(seed = rank)) run as a stream of independent clips over the engine's HIP streams.  The stream is BUCKETED, as a loader for
    mixed-shape data would deliver it (batching clips of equal (shape, scale) is allowed): the draws are ordered so that equal pairs
    are adjacent, and the engine runs up to SAVSR_CLIP_BATCH of them per launch sequence (`--no-bucket`: the draw order)."""
    from savsr_amd.engine import get_hw
    from savsr_amd.utils import synth, workloads
    net, sd = build_net(dev)
    eng = net.engine()                                    # product defaults: the byte budget (SAVSR_CACHE_GB) decides what stays resident
    cps = max(1, args.clips_per_step)
    draws = workloads.config5_cases(cps * args.steps, seed=rank)
    if not args.no_bucket:
        draws = sorted(draws, key=lambda k: (k[0] * k[1], k[2]))
    uniq = sorted(set(draws))
    clips = {k: synth.synth_clip(7, 3, k[0], k[1], seed=11, batch=1).to(dev) for k in uniq}

    def run_step(i):
        ks = draws[i * cps:(i + 1) * cps]
        outs = net.forward_many([clips[k][0] for k in ks], [k[2] for k in ks])       # launch units dealt over the HIP streams
        return sum(o.shape[-1] * o.shape[-2] for o in outs)
    # The steady state of a long stream (64 612 clips over 60 pairs: ~1000 visits each): every context the timed pass uses -- (shape, scale,
    # clips per launch sequence) on the stream that runs it -- exists.  The untimed passes run the SAME step sequence (the draws are
    # deterministic), `--warmup` + 1 times.
    for _ in range(max(1, args.warmup) + eng.capture_after):
        for i in range(args.steps):
            run_step(i)
    px = [0]

    def region():
        for i in range(args.steps):
            px[0] += run_step(i)
    hs0 = dict(eng.host_stats)
    ev0 = eng.cache_stats()["evictions"]
    el = timed(dist, dev, region)
    if rank != 0:
        return
    line = base_line(args, world, world * px[0] / el / 1e6, el,
                     "BASELINE config 5: synthetic Vimeo90K-shape clips (GT 256x448), (sh, sw) drawn from the 60-entry training list, random-init weights",
                     {"frames_per_step": cps, "distinct_shape_scale_pairs": len(uniq), "streams_per_gpu": eng.n_streams,
                      "clips_per_launch_sequence": eng.clip_batch, "bucketed_by_shape_and_scale": not args.no_bucket})
    line["config"]["knobs"] = eng.knobs.knobs()          # non-default SAVSR_* switches of the engine (savsr_amd/config.py); empty = product configuration
    line["bench_config"] = 5
    line["clips_per_s"] = round(world * cps * args.steps / el, 2)
    st = eng.cache_stats()
    line["captures_in_timed_region"] = eng.host_stats["captures"] - hs0["captures"]
    line["eager_frames_in_timed_region"] = eng.host_stats["eager_frames"] - hs0["eager_frames"]
    line["evictions_in_timed_region"] = st["evictions"] - ev0
    line["cache"] = {"budget_gb": round(st["budget_limit"] / 2 ** 30, 1), "used_gb": round(st["budget_used"] / 2 ** 30, 2),
                     "resident_contexts_all_streams": sum(e.cache_stats()["scales"] for e in [eng] + eng._siblings),
                     "note": "product defaults: SAVSR_CACHE_GB unset = half of the free HBM at engine build, shared by the stream engines"}
    line["roofline"] = None
    if world == 1 and not args.no_cpu_baseline:
        # the oracle on the timed path: the two most frequent (shape, scale) groups of the stream, each clip 0 of its group as a step of the timed
        # region delivers it (bucketed, batched into launch sequences), against the oracle's output for the same clip
        from collections import Counter
        from oracle import savsr_oracle as O
        torch.set_num_threads(effective_cpus())
        checks = []
        for k, cnt in Counter(draws).most_common(2):
            i = next(i for i in range(args.steps) if k in draws[i * cps:(i + 1) * cps])
            ks = draws[i * cps:(i + 1) * cps]
            outs = net.forward_many([clips[q][0] for q in ks], [q[2] for q in ks])
            torch.cuda.synchronize()
            with torch.no_grad():
                ref = O.forward(sd, clips[k].cpu(), k[2])
            checks.append({"lr": [k[0], k[1]], "scale": list(k[2]), "clips_of_this_pair_in_the_step": ks.count(k), "draws_of_this_pair": cnt,
                           "max_abs": float((outs[ks.index(k)].cpu() - ref[0]).abs().max())})
        line["gpu_vs_oracle_timed_path"] = checks
        line["gpu_vs_oracle_max_abs_timed_path"] = max(c["max_abs"] for c in checks)
    print(json.dumps(line), flush=True)


# --------------------------------------------------------------------------------------------- the YAML workflow
VID4_SHAPES = [("calendar", 576, 720), ("city", 576, 704), ("foliage", 480, 720), ("walk", 480, 720)]     # GT sizes of Vid4
RUN_TEST_SCALES = [(4, 4), (3.5, 3.5), (3, 3), (2.5, 2.5), (2, 2), (1.5, 4)]


VID4_FRAMES = [41, 34, 49, 47]                   # frames of the four Vid4 folders (calendar, city, foliage, walk)


def job_dims(args):
    """(scales, frames per folder) of the synthetic job: --yaml-dims = the shipped Vid4 YAML's own dimensions (42 datasets = 30 symmetric + 12
    asymmetric scales over folders of 41 / 34 / 49 / 47 frames, options/test/SAVSR/test_SAVSR_Vid4_asBI.yml:24-826), else 6 scales x 4 folders of
    --frames-per-folder frames."""
    if args.yaml_dims:
        from savsr_amd.utils import workloads
        return list(workloads.YAML_SCALES), list(VID4_FRAMES)
    return list(RUN_TEST_SCALES), [args.frames_per_folder] * len(VID4_SHAPES)


def make_png_tree(root, frames):
    """Synthetic Vid4-shaped ground truth: per folder one smooth base image, each frame a shifted crop of it (a panning
    camera), written as PNG through the product's own writer.  frames: per-folder frame counts."""
    import numpy as np
    from savsr_amd import io as sio
    from savsr_amd.utils import synth
    for k, (name, H, W) in enumerate(VID4_SHAPES):
        frames_per_folder = frames[k]
        base = (synth.synth_gt(3, H + 2 * frames_per_folder, W + 2 * frames_per_folder, seed=40 + k).numpy() * 255.0).round().astype(np.uint8)
        for i in range(frames_per_folder):
            img = base[:, 2 * i: 2 * i + H, i: i + W].transpose(1, 2, 0)[:, :, ::-1]          # HWC BGR, as cv2 / tensor2img hand it over
            sio.imwrite(np.ascontiguousarray(img), os.path.join(root, "GT", name, f"{i:08d}.png"))


def run_test_opt(root, ckpt, save_img, scales=None):
    ds = {}
    for i, sc in enumerate(scales if scales is not None else RUN_TEST_SCALES):
        ds[f"test_{i + 1:02d}"] = dict(name=f"Vid4_x{sc[0]}_{sc[1]}", type="ASVideoTestDataset", dataroot_gt=os.path.join(root, "GT"),
                                       dataroot_lq=os.path.join(root, "unused"), io_backend=dict(type="disk"), cache_data=False, num_frame=7,
                                       padding="reflection", use_arbitrary_scale_downsampling=True, downsampling_scale=tuple(sc),
                                       downsampling_mode="torch", phase="test")
    return dict(name="bench_run_test", model_type="ASVSRModel", num_gpu=1, manual_seed=0, is_train=False, datasets=ds,
                network_g=dict(type="SAVSR", num_in_ch=3, num_feat=64, num_frame=7, slid_win=3, fusion_win=5, interval=0, w1_num_block=4,
                               w2_num_block=2, n_resgroups=4, n_resblocks=8, center_frame_idx=None),
                path=dict(pretrain_network_g=ckpt, strict_load_g=True, resume_state=None, visualization=os.path.join(root, "results")),
                val=dict(save_img=bool(save_img), suffix=None,
                         metrics=dict(psnr_y=dict(type="calculate_psnr", crop_border=0, test_y_channel=True),
                                      ssim_y=dict(type="calculate_ssim", crop_border=0, test_y_channel=True))),
                profile_gpu_time=True)


def run_run_test(args, rank, world, dev, dist):
    """One pass = run_test(opt) over the 6 datasets (every rank its per-folder blocks; ONE all_gather per dataset).  Pass 1 is the
    cold process (PNG decode + upload once, hipGraph capture per LR shape); pass 2 the steady state of a long YAML (the shipped
    Vid4 YAML runs 42 datasets over the same files: decoded frames and captured graphs are reused).  `value` = HR Mpixel/s of
    the steady-state pass; both passes' frames/s and GPU-busy fractions are in the line."""
    import shutil
    import tempfile
    from savsr_amd import io as sio
    from savsr_amd import models as M
    from savsr_amd import test as T
    from savsr_amd.utils import synth
    emu = args.emulate_world > 0                # a lone process running rank --emulate-rank's share of a world-size --emulate-world run
    own_tree = not args.tree
    root = args.tree or (tempfile.mkdtemp(prefix="savsr_bench_") if rank == 0 else None)
    if dist is not None:
        box = [root]
        dist.broadcast_object_list(box, src=0)
        root = box[0]
    try:
        scales, frames = job_dims(args)
        if rank == 0 and own_tree:
            make_png_tree(root, frames)
            sd = synth.synth_state_dict(seed=0)
            torch.save({"params": sd}, os.path.join(root, "net.pth"))
        if dist is not None:
            dist.barrier()
        opt = run_test_opt(root, os.path.join(root, "net.pth"), args.save_img, scales)
        opt["rank"], opt["world_size"], opt["dist"] = rank, world, dist is not None
        if emu:
            opt["rank"], opt["world_size"], opt["dist"], opt["emulate_world"] = args.emulate_rank, args.emulate_world, False, True    # (no process group)
            rank_e, world_e = args.emulate_rank, args.emulate_world
        torch.cuda.set_device(dev)
        model = M.build_model(opt)            # one model (= one engine, its graphs) across the passes, as in one long YAML
        model_box = {"m": model}
        passes = []
        n_frames = sum(frames) * len(scales)
        hr_px = sum(round_hw(H, W, sc) * nf for (_, H, W), nf in zip(VID4_SHAPES, frames) for sc in scales)
        results = None
        p = -1
        while True:
            p += 1
            # passes: 0 = cold, 1 = steady; an emulated rank whose steady pass reads SLOWER than its cold pass (the steady work is a subset of the
            # cold pass's: a clock dip of the lease, 12.4 s against 10.3 s on one rank of profiles/r06_emulate_world8.json) repeats it once and keeps the faster
            if p >= 2 and not (emu and p == 2 and passes[1]["wall_s"] > passes[0]["wall_s"]):
                break
            if "m" in model_box:
                model_box["m"].gpu_ms = 0.0
            st0 = dict(sio.frame_store().stats)
            box = {}

            def region():
                if p == 0 and os.environ.get("SAVSR_BENCH_PROFILE"):      # where the cold pass's host time goes (cProfile, top of the cumulative list -> stderr)
                    import cProfile
                    import pstats
                    pr = cProfile.Profile()
                    pr.enable()
                    box["res"] = T.run_test(dict(opt), model=model)
                    pr.disable()
                    pstats.Stats(pr, stream=sys.stderr).sort_stats("cumulative").print_stats(45)
                    return
                box["res"] = T.run_test(dict(opt), model=model)
            el = timed(dist, dev, region)
            results = box["res"]
            st1 = sio.frame_store().stats
            hs = dict(model.net_g.engine().host_stats)
            passes.append({"wall_s": round(el, 3), "frames_per_s": round(n_frames / el, 2), "gpu_busy_frac": round(model_box["m"].gpu_ms / 1e3 / el, 4),
                           "png_decoded_rank0": st1["decoded"] - st0["decoded"], "uploaded_rank0": st1["uploaded"] - st0["uploaded"],
                           "host_stats_cumulative": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in hs.items()}})
        if len(passes) == 3:
            first = passes.pop(1) if passes[2]["wall_s"] < passes[1]["wall_s"] else passes.pop(2)
            passes[1]["repeated_because_slower_than_cold"] = True
            passes[1]["discarded_wall_s"] = first["wall_s"]
        if emu:                                # the child of --emulate-world: its passes are the result
            plan = model.last_plan             # (harness.plan_job: the (dataset, folder) segments of this rank)
            segs = plan["segments"][rank_e]
            mine = sum(hi - lo for _, _, lo, hi in segs)
            for ps in passes:
                ps["frames_per_s"] = round(mine / ps["wall_s"], 2)
            print(json.dumps({"emulated_world": world_e, "emulated_rank": rank_e, "frames": mine, "segments": len(segs),
                              "folders": sorted({f for _, f, _, _ in segs}), "planned_cost_share": round(plan["cost"][rank_e] / max(sum(plan["cost"]), 1e-9), 4),
                              "cold_pass": passes[0], "steady_pass": passes[1]}), flush=True)
            return
        # the same frames through the network alone (inputs resident in HBM, groups of n_streams clips in flight, no metrics):
        # what the workflow would run at if everything around the path were free
        m = model_box["m"]
        net = m.net_g
        eng = net.engine()
        t_net, t_one = 0.0, 0.0
        for dsname, dso in sorted(opt["datasets"].items()):
            from savsr_amd.datasets import build_dataset
            ds = build_dataset(dict(dso))
            mine = ds.shard_frames(model.last_plan["owners"][sorted(opt["datasets"]).index(dsname)][rank])
            items = [ds[i]["lq"] for i in mine]
            net.set_scale(dso["downsampling_scale"])
            g = eng.n_streams * eng.clip_batch              # what a validation call hands forward_many: every stream a unit of clip_batch clips

            def region2():
                for k0 in range(0, len(items), g):
                    net.forward_many(items[k0:k0 + g], [dso["downsampling_scale"]] * len(items[k0:k0 + g]))
            t_net += timed(dist, dev, region2)

            def region1():                    # ... and one clip in flight: the reference's own flow (video_base_model.py:51-53)
                for it in items:
                    net(it.unsqueeze(0))
            t_one += timed(dist, dev, region1)
        if rank != 0:
            return
        warm = passes[1]
        line = base_line(args, world, hr_px / warm["wall_s"] / 1e6, warm["wall_s"],
                         f"YAML workflow run_test(opt): synthetic Vid4-shaped PNG tree (4 folders of {frames} frames), {len(scales)} datasets = scales "
                         + ", ".join(f"x{a}/{b}" for a, b in scales) + " over one dataroot_gt, ASVideoTestDataset + ASVSRModel, PSNR-Y / SSIM-Y",
                         {"frames_per_folder": frames, "frames": n_frames, "save_img": bool(args.save_img),
                          "decode_threads": sio.frame_store().workers, "streams_per_gpu": eng.n_streams})
        line["config"]["knobs"] = eng.knobs.knobs()          # non-default SAVSR_* switches of the engine (savsr_amd/config.py); empty = product configuration
        line["metric"] = "HR Mpixels/sec (YAML workflow, steady-state pass)"
        line["steps"], line["warmup"], line["ms_per_step"] = 1, 1, round(1e3 * warm["wall_s"], 1)
        line["bench_config"] = "run_test"
        line["cold_pass"], line["steady_pass"] = passes[0], passes[1]
        line["network_only_frames_per_s"] = round(n_frames / t_net, 2)
        line["network_only_one_in_flight_frames_per_s"] = round(n_frames / t_one, 2)
        line["steady_vs_one_in_flight"] = round(warm["frames_per_s"] / (n_frames / t_one), 4)
        line["cold_vs_one_in_flight"] = round(passes[0]["frames_per_s"] / (n_frames / t_one), 4)
        line["steady_vs_network_only"] = round(warm["frames_per_s"] / (n_frames / t_net), 4)
        line["cold_vs_network_only"] = round(passes[0]["frames_per_s"] / (n_frames / t_net), 4)
        line["metrics_x4"] = {k: round(v, 4) for k, v in results[0]["metrics"].items()}
        line["roofline"] = None
        print(json.dumps(line), flush=True)
    finally:
        if dist is not None:
            dist.barrier()
        if rank == 0 and root and own_tree:
            shutil.rmtree(root, ignore_errors=True)


def run_emulate_world(args, argv):
    """`--config run_test --emulate-world N` without --emulate-rank: the part of the 1 -> N strong-scaling curve of the YAML flow that one GPU
    can know in advance.  Fresh child processes (what a rank is: its own decode cache, engine, captures, HR plan choices), one at a time on
    the one GPU, over ONE PNG tree: the whole job (world 1) and the ranks of a world-size-N run, each its share of the job plan alone
    (harness.plan_job: (dataset, folder) units, folder-major, cost-balanced; the collective -- ONE all_gather of the metric rows per job -- is
    left out).  `--emulate-ranks all` (default with --yaml-dims) times every rank, `ends` ranks 0 and N - 1.  predicted efficiency =
    T(1) / (N x max_r T_r), for the cold pass (what `python -m savsr_amd.test -opt <yaml>` is) and for the steady one."""
    import shutil
    import subprocess
    import tempfile
    from savsr_amd.utils import synth
    n = args.emulate_world
    scales, frames = job_dims(args)
    root = tempfile.mkdtemp(prefix="savsr_bench_emu_")
    try:
        make_png_tree(root, frames)
        torch.save({"params": synth.synth_state_dict(seed=0)}, os.path.join(root, "net.pth"))
        runs = {}
        which = args.emulate_ranks or ("all" if args.yaml_dims else "ends")
        ranks_run = list(range(n)) if which == "all" else sorted({0, n - 1})
        for w, r in [(1, 0)] + [(n, r) for r in ranks_run]:
            cmd = [sys.executable, os.path.abspath(__file__), "--config", "run_test", "--emulate-world", str(w), "--emulate-rank", str(r),
                   "--tree", root, "--frames-per-folder", str(args.frames_per_folder)] + (["--save-img"] if args.save_img else []) + (["--yaml-dims"] if args.yaml_dims else [])
            p = subprocess.run(cmd, capture_output=True, text=True)
            if os.environ.get("SAVSR_BENCH_PROFILE"):
                print(f"==== world {w} rank {r}\n" + p.stderr[-9000:], file=sys.stderr, flush=True)
            if p.returncode != 0:
                print(p.stdout[-2000:] + p.stderr[-4000:], file=sys.stderr, flush=True)
                sys.exit(p.returncode)
            runs[(w, r)] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        one = runs[(1, 0)]
        ranks = [runs[(n, r)] for r in ranks_run]
        line = {"metric": f"predicted strong-scaling efficiency of the YAML flow at world size {n} (one GPU, ranks emulated one at a time)",
                "unit": "fraction of linear", "n_gpus": 1, "higher_is_better": True, "bench_config": "run_test --emulate-world",
                "emulated_world": n, "data": "synthetic", "frames_per_folder": frames, "datasets": len(scales), "ranks_timed": ranks_run,
                "partition": "harness.plan_job: (dataset, folder) units folder-major on one line, cut into N pieces of equal modelled cost",
                "world1": one, "ranks": ranks}
        for name in ("cold_pass", "steady_pass"):
            t1 = one[name]["wall_s"]
            tr = max(x[name]["wall_s"] for x in ranks)
            line["predicted_strong_scaling_eff_" + name.split("_")[0]] = round(t1 / (n * tr), 4)
            line["rank_wall_s_" + name.split("_")[0]] = [x[name]["wall_s"] for x in ranks]
        slow = max(ranks, key=lambda x: x["cold_pass"]["wall_s"])
        hs = slow["cold_pass"]["host_stats_cumulative"]
        ideal = one["cold_pass"]["wall_s"] / n
        line["value"] = line["predicted_strong_scaling_eff_cold"]
        line["loss_breakdown_cold_slowest_rank"] = {
            "rank": slow["emulated_rank"], "rank_wall_s": slow["cold_pass"]["wall_s"], "ideal_s (T1 / N)": round(ideal, 3), "graph_capture_s": hs["capture_s"], "hr_plan_timing_s": hs["plan_s"],
            "captures": hs["captures"], "eager_frames": hs["eager_frames"], "png_decoded": slow["cold_pass"]["png_decoded_rank0"],
            "gpu_busy_frac": slow["cold_pass"]["gpu_busy_frac"], "frames": slow["frames"], "segments": slow["segments"], "folders": slow["folders"],
            "note": "what a rank pays per (folder, scale) context it owns whatever its share of the frames: PNG decode of its folders, the first frame's "
                    "buffer plan and table upload, graph captures and HR plan timing (scales missing from savsr_amd/hr_plans.json); "
                    "the collective (one all_gather of the job's metric rows) is not in the emulation"}
        print(json.dumps(line), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def round_hw(H, W, sc):
    """HR pixels of one output frame of a (GT size, scale) dataset: the mod-cropped GT size."""
    from savsr_amd.resize_gpu import as_mod_crop_hw
    h, w = as_mod_crop_hw(H, W, (float(sc[0]), float(sc[1])))
    return h * w


def self_launch(args, argv):
    """`--gpus N` outside a torch.distributed environment: start the N ranks as FRESH child processes -- nothing in this
    process has touched a GPU (torch.cuda.device_count() does not initialise one) -- relay their output (rank 0 prints the one
    JSON line) and exit with the launcher's return code."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if os.environ.get("SAVSR_BENCH_SHARE_GPU") == "1" and have >= 1:
        have = args.gpus              # TEST mode: all ranks on GPU 0 over a gloo group (exercises the N > 1 code path on a 1-GPU box)
    if have < args.gpus:
        print(f"bench.py: --gpus {args.gpus} requested but this node shows {have} GPU(s); refusing to run a smaller job under that label",
              file=sys.stderr, flush=True)
        sys.exit(2)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    rc = subprocess.call(cmd)
    sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=str, default="2", choices=["2", "3", "4", "5", "run_test"],
                    help="BASELINE.json config (2 = the judged line); run_test = the YAML workflow on a synthetic PNG tree")
    ap.add_argument("--frames-per-folder", type=int, default=32, help="run_test: frames per synthetic folder (4 folders)")
    ap.add_argument("--save-img", action="store_true", help="run_test: also write every output frame as PNG (val.save_img)")
    ap.add_argument("--emulate-world", type=int, default=0, help="run_test on ONE GPU: time the whole job and ranks 0 / N-1 of a world-size-N run in fresh "
                                                                 "processes, report the predicted strong-scaling efficiency")
    ap.add_argument("--yaml-dims", action="store_true", help="run_test: the shipped Vid4 YAML's dimensions (42 scales; folders of 41 / 34 / 49 / 47 frames) "
                                                            "instead of 6 scales x --frames-per-folder")
    ap.add_argument("--emulate-ranks", type=str, default="", choices=["", "all", "ends"], help="--emulate-world: time every rank or ranks 0 and N - 1")
    ap.add_argument("--emulate-rank", type=int, default=-1, help="(internal: the child of --emulate-world that runs one rank's share)")
    ap.add_argument("--tree", type=str, default="", help="(internal: an existing synthetic PNG tree + net.pth)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--regions", type=int, default=3, help="config 2: back-to-back regions the K timed steps are split into (value = the median region)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="config 2: after the timed steps, write what the last timed step computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--clips-per-step", type=int, default=16,
                    help="independent clips per step (two HIP streams x four clips per launch sequence x two units; 16 keeps 20 timed steps at ~2.3 s)")
    ap.add_argument("--scales", type=str, default="", help="config 3: comma-separated subset, e.g. 1.1,2.5,4")
    ap.add_argument("--no-bucket", action="store_true", help="config 5: keep the draw order instead of grouping equal (shape, scale) clips")
    args = ap.parse_args()
    if args.config != "run_test":
        args.config = int(args.config)
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.dump_outputs and args.config != 2:
        ap.error("--dump-outputs goes with config 2")
    if args.emulate_world:
        if args.config != "run_test" or args.gpus != 1:
            ap.error("--emulate-world goes with --config run_test on one GPU")
        if args.emulate_rank < 0:
            run_emulate_world(args, sys.argv[1:])       # children first: this process never touches the GPU
            return
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            self_launch(args, sys.argv[1:])            # never returns
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}: launch one rank per GPU "
              f"(--nproc-per-node {args.gpus}) or drop the launcher", file=sys.stderr, flush=True)
        sys.exit(2)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("SAVSR_BENCH_SHARE_GPU") == "1"      # test mode (see self_launch): not a performance configuration
    if share:
        local_rank = 0
        os.environ.setdefault("SAVSR_DIST_BACKEND", "gloo")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or os.environ.get("SAVSR_BENCH_FORCE_DIST"):     # (the env switch exercises the RCCL path with one rank)
        import torch.distributed as dist
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29533"), RANK="0", WORLD_SIZE="1")
        if os.environ.get("SAVSR_DIST_BACKEND", "nccl") == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)    # RCCL over xGMI
        else:
            dist.init_process_group(backend=os.environ["SAVSR_DIST_BACKEND"])
    try:
        if args.config == "run_test":
            run_run_test(args, rank, world, dev, dist)
        elif args.config == 2:
            run_config2(args, rank, world, dev, dist)
        elif args.config == 3:
            from savsr_amd.utils import workloads
            scales = workloads.CONFIG3_SCALES
            if args.scales:
                scales = [(float(s), float(s)) for s in args.scales.split(",")]
            run_cases(args, rank, world, dev, dist, [(LR_H, LR_W, s) for s in scales],
                      "BASELINE config 3: Vid4 sweep, synthetic 7x3x180x320 clips, symmetric scales x1.1 ... x4.0", 3)
        elif args.config == 4:
            from savsr_amd.utils import workloads
            cases = [workloads.lr_shape(g, s) + (s,) for g, s in workloads.CONFIG4_CASES]
            run_cases(args, rank, world, dev, dist, cases,
                      "BASELINE config 4: UDM10 asymmetric scales, GT 720x1272: LR 480x318 x(1.5, 4) and LR 204x636 x(3.5, 2)", 4)
        else:
            run_config5(args, rank, world, dev, dist)
    finally:
        if dist is not None:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
