"""What the video boundary refuses, and in which words: a fixed subsample of the refusal census (tests/video_refusal_cases.py; the whole
grid: tools/video_refusals.py) against tests/golden/video_refusals.json.  The subsample holds every distinct outcome of the whole grid
at least once, for SAVSR.upscale_video and for VideoUpscaler, so a changed message, a changed exception type and a changed winner
among two simultaneous errors each fail here.  CPU networks: no GPU is needed."""
import json
import os

from tests import video_refusal_cases as vc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_refusals.json")


def test_refusals_match_the_recorded_census():
    with open(FIXTURE) as f:
        want = json.load(f)
    cases, outcomes, index = want["cases"], want["outcomes"], want["index"]
    assert 2000 <= len(cases) <= 10000 and len(index) == 2 * len(cases) and max(cases) == vc.CASES - 1
    assert set(index) == set(range(len(outcomes)))          # every recorded outcome is exercised
    wrong = []
    for j, k in enumerate(cases):
        got = vc.record(k)
        exp = [outcomes[index[2 * j]], outcomes[index[2 * j + 1]]]
        if got != exp:
            wrong.append((k, vc.grid_case(k) if k < vc.GRID_CASES else vc.TENSOR_CASES[k - vc.GRID_CASES][:2], got, exp))
    assert not wrong, f"{len(wrong)} of {len(cases)} cases answer otherwise; the first: {wrong[0]}"
