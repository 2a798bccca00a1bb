"""Golden fixtures of the sequence path (SAVSR.upscale_video / VideoUpscaler): the REFERENCE's generate_frame_indices lists and the
REFERENCE's SAVSR run on every frame's window of short seeded videos, case table in tests/video_cases.py.

Build-container only (needs the reference checkout, see tools/ref_import.py).  The reference's data_util.py imports cv2 and
torchvision, which are absent, so generate_frame_indices alone is taken out of the file's syntax tree and compiled here at generation
time (nothing of it is stored in the repository).  Writes tests/golden/video_outputs.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_video.py
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402
from video_cases import INDEX_MAX_N, INDEX_NUM_FRAMES, PADDINGS, VIDEO_CASES, VIDEO_SEED, WEIGHT_SEED  # noqa: E402
from savsr_amd.utils import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def reference_generate_frame_indices():
    path = os.path.join(ref_import.REF_ROOT, "lbasicsr", "data", "data_util.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "generate_frame_indices"]
    assert len(fn) == 1
    ns = {}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["generate_frame_indices"]


def main():
    torch.set_num_threads(8)
    gfi = reference_generate_frame_indices()
    out = {}
    for p in PADDINGS:
        for nf in INDEX_NUM_FRAMES:
            for n in range(1, INDEX_MAX_N + 1):
                out[f"idx/{p}/{nf}/{n}"] = np.array([gfi(i, n, nf, padding=p) for i in range(n)], dtype=np.int32)
    ref = ref_import.load_reference_arch()
    with torch.no_grad():
        for name, cfg, n, h, w, sc, pad in VIDEO_CASES:
            net = ref.SAVSR(**cfg).eval()
            net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
            net.set_scale(sc)
            video = synth.synth_clip(n, cfg.get("num_in_ch", 3), h, w, seed=VIDEO_SEED)[0]
            nf = cfg.get("num_frame", 7)
            srs = []
            for i in range(n):
                win = gfi(i, n, nf, padding=pad)
                assert min(win) >= 0 and max(win) < n, (name, i, win)
                srs.append(net(video[win][None])[0])
            sr = torch.stack(srs, 0)
            out[f"{name}/sr"] = sr.numpy()
            print(name, cfg, pad, tuple(sr.shape), float(sr.abs().max()))
    np.savez_compressed(os.path.join(GOLD, "video_outputs.npz"), **out)
    print("wrote", os.path.getsize(os.path.join(GOLD, "video_outputs.npz")) / 1e3, "KB")


if __name__ == "__main__":
    main()
