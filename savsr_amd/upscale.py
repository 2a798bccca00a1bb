"""Command-line upscaler: a folder of LR frames (PNG) in, a folder of SR frames (PNG, same file names) out.

    python -m savsr_amd.upscale -i <lr_frames/> -o <sr_frames/> --scale 4 --checkpoint <net.pth>
    python -m savsr_amd.upscale -i <lr_frames/> -o <sr_frames/> --scale 3.5 2.5 --padding reflection --opt <test.yml>
    python -m savsr_amd.upscale -i <lr_frames/> -o <sr_frames/> --scale 4 --checkpoint <net.pth> --self-ensemble

Frames are taken in the order read_img_seq reads a folder (sorted scandir, lbasicsr/data/data_util.py:29-60), decoded on the
FrameStore pool (savsr_amd.io), pushed through VideoUpscaler in chunks (uint8 in, uint8 out: the windows, the network and the
quantisation run on the GPU) and encoded on a writer pool of this tool's own (at most 16 threads).  It ends with one line: frames,
seconds, frames/s.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

MAX_WRITERS = 16


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m savsr_amd.upscale", description="Upscale a folder of LR video frames (PNG) with SAVSR.")
    p.add_argument("-i", "--input", required=True, help="folder of LR frames (PNG), taken in sorted order")
    p.add_argument("-o", "--output", required=True, help="output folder (created); SR frames keep the input file names")
    p.add_argument("--scale", type=float, nargs="+", required=True, metavar="S", help="s, or sh sw")
    p.add_argument("--padding", default="reflection", choices=["replicate", "reflection", "reflection_circle", "circle"],
                   help="window padding at the ends of the video (generate_frame_indices); default reflection")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--opt", help="test YAML: network_g and path.pretrain_network_g / param_key_g / strict_load_g")
    src.add_argument("--checkpoint", help="checkpoint (.pth, 'params' key) for SAVSR with default constructor arguments")
    p.add_argument("--chunk", type=int, default=16, help="frames per push (default 16)")
    p.add_argument("--writers", type=int, default=0, help=f"PNG encoder threads (default: the usable CPUs, at most {MAX_WRITERS})")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16"],
                   help="conv operand precision (default fp32; fp16: faster, ~1e-3 drift, see DESIGN.md section 3)")
    p.add_argument("--self-ensemble", action="store_true",
                   help="average the 8 flip / transpose variants of every window (8x the work; DESIGN.md section 11)")
    return p


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = build_parser()
    a = p.parse_args(argv)
    if len(a.scale) not in (1, 2):
        p.error("--scale takes one value (s) or two (sh sw)")
    if any(s <= 0 for s in a.scale):
        p.error("--scale must be positive")
    a.scale = (a.scale[0], a.scale[0]) if len(a.scale) == 1 else tuple(a.scale)
    if a.chunk < 1:
        p.error("--chunk must be >= 1")
    if a.writers < 0 or a.writers > MAX_WRITERS:
        p.error(f"--writers must be in 0 .. {MAX_WRITERS}")
    return a


def list_frames(folder: str) -> List[str]:
    from .io import scandir
    if not os.path.isdir(folder):
        raise SystemExit(f"input folder {folder!r} does not exist")
    paths = sorted(scandir(folder, suffix=".png", full_path=True))
    if not paths:
        raise SystemExit(f"no .png frames in {folder!r}")
    return paths


def load_net(a: argparse.Namespace):
    """The network as models.py builds it from a YAML (network_g, path.*), or SAVSR() from a bare checkpoint."""
    from . import io as sio
    from .archs import build_network
    from .archs.savsr_arch import SAVSR
    if a.opt is not None:
        from .options import yaml_load
        opt = yaml_load(a.opt)
        net = build_network(opt["network_g"])
        path = opt.get("path") or {}
        if path.get("pretrain_network_g") is not None:
            sio.load_network(net, path["pretrain_network_g"], path.get("strict_load_g", True), path.get("param_key_g", "params"))
    else:
        net = SAVSR()
        sio.load_network(net, a.checkpoint, True, "params")
    if net.cfg["num_in_ch"] != 3:
        raise SystemExit(f"num_in_ch = {net.cfg['num_in_ch']}: the CLI decodes RGB frames; run such a checkpoint through SAVSR.upscale_video")
    return net.eval()


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    paths = list_frames(a.input)
    import numpy as np
    import torch
    from PIL import Image

    from .io import FrameStore
    from .utils.host import effective_cpus
    from .video import VideoUpscaler, check_length

    net = load_net(a)
    net.set_precision(a.precision)
    net.set_self_ensemble(a.self_ensemble)
    check_length(len(paths), net.num_frame, a.padding)        # (before the GPU is touched)
    dev = torch.device(a.device)
    net = net.to(dev)
    os.makedirs(a.output, exist_ok=True)
    names = [os.path.basename(p) for p in paths]
    store = FrameStore()
    writers = ThreadPoolExecutor(max_workers=a.writers or max(1, min(MAX_WRITERS, effective_cpus())), thread_name_prefix="savsr-upscale-png")
    pending = []

    def save(img: np.ndarray, path: str) -> None:
        Image.fromarray(img).save(path)

    def emit(sr: torch.Tensor, first: int) -> int:
        host = sr.cpu().numpy()
        for j in range(host.shape[0]):
            pending.append(writers.submit(save, host[j], os.path.join(a.output, names[first + j])))
        while len(pending) > 4 * MAX_WRITERS:          # bound the queue of encoded-but-unwritten frames
            pending.pop(0).result()
        return first + host.shape[0]

    t0 = time.perf_counter()
    up = VideoUpscaler(net, a.scale, a.padding, out="uint8")
    store.request(paths)
    done = 0
    for c0 in range(0, len(paths), a.chunk):
        chunk = np.stack([store.host(p) for p in paths[c0:c0 + a.chunk]], 0)
        done = emit(up.push(torch.from_numpy(chunk)), done)
    done = emit(up.finish(), done)
    for f in pending:
        f.result()
    writers.shutdown()
    dt = time.perf_counter() - t0
    print(f"upscaled {done} frames in {dt:.2f} s: {done / dt:.2f} frames/s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
