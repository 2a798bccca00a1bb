"""Refusal census of the video boundary: what SAVSR.upscale_video and VideoUpscaler answer, on CPU networks, to every case of the grid
in tests/video_refusal_cases.py -- (exception type, message) per entry point, or "constructed".  No GPU is needed.

    python tools/video_refusals.py --census out.json      the whole grid -> {"cases", "outcomes", "index"}; prints counts and a sha256
    python tools/video_refusals.py --fixture              the whole grid, then tests/golden/video_refusals.json: the subsample
                                                          tests/test_video_refusals.py runs

Two commits refuse alike when their --census files are equal (compare the printed sha256).  The subsample is every STRIDE-th case,
the tensor cases, and the first case of every distinct (upscale_video outcome, VideoUpscaler outcome) pair of the whole grid, so it
holds every distinct message at least once; generate the fixture on the commit whose behaviour is to be kept.
"""
import argparse
import hashlib
import json
import os
import sys
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_refusal_cases as vc  # noqa: E402

STRIDE = 709          # (a prime that divides no axis length: the strided cases walk through every value of every axis)
CHUNK = 20000
FIXTURE = os.path.join(ROOT, "tests", "golden", "video_refusals.json")


def _chunk(a: int):
    """Cases [a, a + CHUNK): (the distinct outcomes in order of appearance, two positions in that list per case)."""
    import torch
    torch.set_num_threads(1)
    seen, outcomes, index = {}, [], []
    for k in range(a, min(a + CHUNK, vc.CASES)):
        for o in vc.record(k):
            key = tuple(o)
            if key not in seen:
                seen[key] = len(outcomes)
                outcomes.append(list(o))
            index.append(seen[key])
    return outcomes, index


def census(jobs: int) -> dict:
    """The whole grid, in case order: the distinct outcomes in order of appearance and two positions in that list per case."""
    seen, index = {}, []
    with Pool(jobs) as pool:
        for part, idx in pool.imap(_chunk, range(0, vc.CASES, CHUNK)):
            remap = [seen.setdefault(tuple(o), len(seen)) for o in part]
            index += [remap[i] for i in idx]
    return {"cases": vc.CASES, "outcomes": [list(o) for o in seen], "index": index}


def subsample(full: dict) -> dict:
    """The fixture: the chosen case numbers, their outcomes once, and two positions in that list per chosen case."""
    index = full["index"]
    cases, pairs = set(range(0, vc.GRID_CASES, STRIDE)) | set(range(vc.GRID_CASES, vc.CASES)), set()
    for k in range(vc.CASES):
        pair = (index[2 * k], index[2 * k + 1])
        if pair not in pairs:
            pairs.add(pair)
            cases.add(k)
    cases = sorted(cases)
    used = sorted({index[2 * k + j] for k in cases for j in (0, 1)})
    assert len(used) == len(full["outcomes"])          # every distinct outcome of the whole grid is in the subsample
    return {"cases": cases, "outcomes": full["outcomes"], "index": [index[2 * k + j] for k in cases for j in (0, 1)]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--census", metavar="FILE", help="write the whole grid's outcomes there")
    ap.add_argument("--fixture", action="store_true", help=f"write {os.path.relpath(FIXTURE, ROOT)}")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    full = census(args.jobs)
    text = json.dumps(full, separators=(",", ":"))
    print(f"cases {full['cases']} (2 calls each)  distinct outcomes {len(full['outcomes'])}  "
          f"distinct messages {len({o[1] for o in full['outcomes']})}  sha256 {hashlib.sha256(text.encode()).hexdigest()}")
    if args.census:
        with open(args.census, "w") as f:
            f.write(text)
    if args.fixture:
        sub = subsample(full)
        with open(FIXTURE, "w") as f:
            json.dump(sub, f, separators=(",", ":"))
            f.write("\n")
        print(f"{os.path.relpath(FIXTURE, ROOT)}: {len(sub['cases'])} cases, {os.path.getsize(FIXTURE)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
