"""Oracle <-> reference arch on the reference's own state_dict manifest and outputs (tests/golden/reference_manifest.json,
tests/golden/oracle_vs_reference.npz, written by tools/gen_golden_reference_checks.py from the reference tree; data only)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import savsr_oracle as O
from savsr_amd.utils import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref_manifest():
    with open(os.path.join(GOLD, "reference_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref_out():
    return np.load(os.path.join(GOLD, "oracle_vs_reference.npz"))


def test_manifest_matches_reference(ref_manifest):
    assert ref_manifest == synth.load_manifest()


@pytest.mark.parametrize("h,w,sc", [(10, 12, (4, 4)), (11, 9, (2.5, 2.5)), (9, 11, (1.7, 3.75))])
def test_forward_identical(ref_manifest, ref_out, h, w, sc):
    sd = synth.synth_state_dict(ref_manifest, seed=3)
    lq = synth.synth_clip(7, 3, h, w, seed=4)
    a = torch.from_numpy(ref_out[f"sr/{h}x{w}/{sc[0]}_{sc[1]}"])
    with torch.no_grad():
        b = O.forward(sd, lq, sc)
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-6
