"""The cases the surface tests share (tests/test_surface.py on the CPU, tests/test_gpu_surface.py on the GPU, and
tools/check_surface_host.py under the sanitizers): every named constructor of savsr_amd.surface.Surface at every depth and layout it
admits, at four frame sizes and three pitches, with N = 3 frames whose stride exceeds the surface's bytes.

Sizes: (2, 2), (5, 7), (6, 34), (9, 66) -- odd sizes for the chroma ceilings, widths on either side of one and two 32-byte vector items,
and a tail.  Pitches: tight; tight + 3 bytes (+ 2 with 16-bit samples), which keeps every row off the 16-byte grid, so the one-sample
form runs; a multiple of 128 with lines = h + 3, so that padded lines run.  The frame stride is 5 bytes (6 with 16-bit samples) beyond the
surface's bytes, which takes frames 1 and 2 off the 16-byte grid; a fourth pitch, "vector", is the third with a stride 16 bytes beyond, so
that the vector form runs on every frame (from an aligned base pointer).  Content: random samples over the full range of
the depth; the low bits of msb words, the row padding, the padded lines, the pad Y of odd-width packed rows and the bytes between frames
are random as well.
"""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from savsr_amd import surface as S
from savsr_amd.yuv import frame_bytes

SIZES = ((2, 2), (5, 7), (6, 34), (9, 66))
PITCHES = ("tight", "odd", "aligned", "vector")
N_FRAMES = 3
FORMAT_OF = {"420": "i420", "422": "i422", "444": "i444", "400": "y400"}


class Case(NamedTuple):
    id: str
    kind: str
    layout: str
    depth: int
    h: int
    w: int
    pitch: str
    surface: S.Surface
    table: S.SurfaceTable

    @property
    def stride(self) -> int:
        return self.table.bytes + (16 if self.pitch == "vector" else 5 if self.depth == 8 else 6)

    @property
    def pixel_format(self) -> str:
        return FORMAT_OF[self.layout]


def make_surface(kind: str, pitch: str, h: int, w: int, depth: int, layout: str) -> S.Surface:
    make = getattr(S.Surface, kind)
    if pitch == "tight":
        return make()
    if pitch == "odd":
        return make(pitch=make().resolve(h, w, depth, layout).planes[0].pitch + (3 if depth == 8 else 2), lines=h)
    return make(lines=h + 3, pitch_align=128)


def _cases():
    out = []
    for kind in S.KINDS:
        layouts, depths = S._KINDS[kind][:2]
        for layout in layouts:
            for depth in depths:
                for h, w in SIZES:
                    for pitch in PITCHES:
                        surf = make_surface(kind, pitch, h, w, depth, layout)
                        out.append(Case(f"{kind}-{layout}-{depth}-{h}x{w}-{pitch}", kind, layout, depth, h, w, pitch, surf,
                                        surf.resolve(h, w, depth, layout)))
    return out


CASES = _cases()
BY_KIND = {kind: [c for c in CASES if c.kind == kind] for kind in S.KINDS}


def _seed(case: Case) -> int:
    return CASES.index(case) + 1


@lru_cache(maxsize=None)
def planar_frames(case: Case) -> np.ndarray:
    """[N, frame_bytes] uint8: random in-range samples (read-only)."""
    rng = np.random.default_rng(_seed(case))
    fb = frame_bytes(case.h, case.w, case.depth, case.layout)
    v = rng.integers(0, 1 << case.depth, (N_FRAMES, fb // case.table.sample))
    v[:, ::7] = (1 << case.depth) - 1          # the largest sample is among them
    out = v.astype("<u2").view(np.uint8).reshape(N_FRAMES, -1) if case.depth > 8 else v.astype(np.uint8)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def sample_mask(case: Case) -> np.ndarray:
    """[surface bytes] uint8: the bits of a surface frame that carry a sample (pack_frames of all-ones samples)."""
    ones = np.full((1, frame_bytes(case.h, case.w, case.depth, case.layout)), 255, dtype=np.uint8)
    mask = S.pack_frames(ones, case.surface, case.h, case.w, case.depth, case.layout)[0]
    mask.setflags(write=False)
    return mask


@lru_cache(maxsize=None)
def surface_frames(case: Case, poison: int = 0) -> np.ndarray:
    """[N, stride] uint8: planar_frames(case) in the case's surface, every bit that carries no sample random (another `poison`: other
    random bits, the same samples).  Read-only."""
    rng = np.random.default_rng(1000 * (poison + 1) + _seed(case))
    tab = case.table
    out = rng.integers(0, 256, (N_FRAMES, case.stride), dtype=np.uint8)
    packed = S.pack_frames(planar_frames(case), case.surface, case.h, case.w, case.depth, case.layout)
    mask = sample_mask(case)
    out[:, :tab.bytes] = (packed & mask) | (out[:, :tab.bytes] & ~mask)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def packed_frames(case: Case) -> np.ndarray:
    """[N, surface bytes] uint8: the specification's pack of planar_frames(case) (read-only)."""
    out = S.pack_frames(planar_frames(case), case.surface, case.h, case.w, case.depth, case.layout)
    out.setflags(write=False)
    return out
