"""The synthetic edited video of the scene tests: independent smooth textures, each drifting by a pixel per frame under a little noise."""
import numpy as np

SCENE_SEEDS = (1, 2, 3)
SCENE_LENGTHS = (9, 4, 8)
SCENE_CUTS = [9, 13]
SCENE_HW = (24, 32)
CELL = 16


def texture(seed, h, w, cell=CELL):
    """A smooth random picture [h, w, 3] (float levels 0 .. 255): a coarse grid of values, one per `cell` pixels and stretched so that
    many sit at black or white, interpolated linearly."""
    rng = np.random.RandomState(seed)
    gh, gw = h // cell + 2, w // cell + 2
    g = np.clip(rng.uniform(-255, 510, (gh, gw, 3)), 0, 255)
    ys, xs = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx
    bot = g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx
    return top * (1 - fy) + bot * fy


def scene(seed, n, h, w):
    """n frames [n, h, w, 3] uint8: a window drifting one pixel per frame over the texture, with noise of +-2 levels."""
    tex = texture(seed, h, w + n)
    rng = np.random.RandomState(seed + 1000)
    return np.stack([np.clip(np.rint(tex[:, i:i + w] + rng.randint(-2, 3, (h, w, 3))), 0, 255).astype(np.uint8) for i in range(n)], 0)


def edited_video(seeds=SCENE_SEEDS, lengths=SCENE_LENGTHS, hw=SCENE_HW):
    """The scenes one after the other: [sum(lengths), h, w, 3] uint8; the cuts are the running sums of the lengths."""
    return np.concatenate([scene(s, n, *hw) for s, n in zip(seeds, lengths)], 0)


def scores(sad, samples):
    """scdet's damped score of every pair in per cent of the largest change (exact fractions would do; floats suffice for a margin)."""
    out, prev = [], 0
    for s in (int(v) for v in sad):
        out.append(min(s, abs(s - prev)) * 100.0 / (255 * samples))
        prev = s
    return out
