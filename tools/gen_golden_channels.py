"""Golden fixtures for num_in_ch / slid_win checkpoints beside the shipped 3 / 3 (savsr_pack_windows_nch, savsr_satu_nf_hr_planes,
savsr_tail_gather_nch): outputs of the REFERENCE's `SAVSR(**cfg)` on key-seeded weights and a hash of its state_dict manifest (names +
shapes), case table in tests/channel_cases.py.

Build-container only (needs the reference checkout, see tools/ref_import.py).  Writes tests/golden/channels_outputs.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_channels.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402
from golden_cases import manifest_hash  # noqa: E402
from channel_cases import CHANNEL_CASES  # noqa: E402
from savsr_amd.utils import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    torch.set_num_threads(8)
    ref = ref_import.load_reference_arch()
    out = {}
    with torch.no_grad():
        for name, cfg, h, w, sc in CHANNEL_CASES:
            net = ref.SAVSR(**cfg).eval()
            manifest = synth.manifest_of(net.state_dict())
            out[f"{name}/manifest_sha"] = np.frombuffer(bytes.fromhex(manifest_hash(manifest)), dtype=np.uint8)
            out[f"{name}/n_keys"] = np.array([len(manifest)], dtype=np.int32)
            net.load_state_dict(synth.synth_state_dict(manifest, seed=3), strict=True)
            lq = synth.synth_clip(cfg.get("num_frame", 7), cfg.get("num_in_ch", 3), h, w, seed=5)
            net.set_scale(sc)
            sr = net(lq)
            out[f"{name}/sr"] = sr.numpy()
            print(name, cfg, tuple(sr.shape), float(sr.abs().max()))
    np.savez_compressed(os.path.join(GOLD, "channels_outputs.npz"), **out)
    print("wrote", os.path.getsize(os.path.join(GOLD, "channels_outputs.npz")) / 1e3, "KB")


if __name__ == "__main__":
    main()
