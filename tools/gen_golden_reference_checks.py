"""Fixtures that let tests/test_oracle_vs_reference.py run without the reference tree (build container only).

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_reference_checks.py

Writes, under tests/golden/:
  reference_manifest.json    [key, shape, dtype] of the reference SAVSR's state_dict
  oracle_vs_reference.npz    the reference SAVSR's outputs on key-seeded weights (seed 3) for FORWARD_CASES
                             (clip synth_clip(7, 3, h, w, seed=4))
Only data (a manifest, outputs) is stored; no reference source text enters the repository.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402
from savsr_amd.utils import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FORWARD_CASES = [(10, 12, (4, 4)), (11, 9, (2.5, 2.5)), (9, 11, (1.7, 3.75))]


def case_key(h, w, sc):
    return f"sr/{h}x{w}/{sc[0]}_{sc[1]}"


def main():
    torch.set_num_threads(8)
    ref = ref_import.load_reference_arch()
    net = ref.SAVSR().eval()
    manifest = synth.manifest_of(net.state_dict())
    with open(os.path.join(GOLD, "reference_manifest.json"), "w") as f:
        json.dump(manifest, f)
    net.load_state_dict(synth.synth_state_dict(manifest, seed=3), strict=True)
    out = {}
    with torch.no_grad():
        for h, w, sc in FORWARD_CASES:
            net.set_scale(sc)
            out[case_key(h, w, sc)] = net(synth.synth_clip(7, 3, h, w, seed=4)).numpy()
    np.savez_compressed(os.path.join(GOLD, "oracle_vs_reference.npz"), **out)
    print("wrote", GOLD, sorted(out))


if __name__ == "__main__":
    main()
