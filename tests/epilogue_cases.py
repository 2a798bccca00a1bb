"""The conv kernels' epilogue observed alone: float64 reference, derived per-element bound, float32 emulation, inputs and mutants.

Everything a conv launch does after its accumulator (conv_mfma.hip, conv_wy.hip; include/savsr_hip.h, savsr_conv_desc), per output element:

    t0  = a + bias                      bias [cout], absent: t0 = a
    t1  = act(t0)                       NONE, RELU, LRELU(slope), SIGMOID
    t2  = t1 * mul                      mul [h][w], one factor per pixel, absent: t2 = t1
    t3  = t2 + res1                     absent: t3 = t2
    out = t3 + res2_scale * res2        absent: out = t3

`a` is what a BARE run of the same conv stored (no bias, ACT_NONE, no mask, no residual): same inputs, weight image, algo and geometry, so
the accumulation is bit-identical and the split-bf16 (fp16) product error cancels.  `reference(a, E)` evaluates the chain in float64 on
that stored `a`; what separates a correct kernel from it are the epilogue's own roundings, and `bound(a, E)` sums them.

The bound (u = 2^-24, fp32's unit roundoff; nothing measured enters).  Every fp32 operation rounds its exact result x to fl(x) with
|fl(x) - x| <= u |x|.  Let e_k bound |kernel's t_k - reference's t_k|.  The kernel's operation k works on inputs that are off by e_(k-1):
its exact result is off by at most L_k e_(k-1) (L_k the step's Lipschitz factor) and has magnitude <= |t_k| + L_k e_(k-1), so

    e_k = L_k e_(k-1) + u (|t_k| + L_k e_(k-1))          for a step that rounds,         e_k = L_k e_(k-1)   for an exact one.

  bias     present: one addition of exact inputs, e0 = u |t0|.  Absent: a + 0 is exact (the interior paths add a quad of zeros), e0 = 0.
  NONE     nothing is computed.  e1 = e0.
  RELU     v_max_f32(v, v * 0) or a select: exact, L = 1.  e1 = e0.
  LRELU    x > 0 ? x : slope x is piecewise linear and continuous: L = max(1, |slope|).  The product slope * v rounds once, and only where
           the kernel's v can be <= 0, i.e. where t0 - e0 <= 0: there e1 = L e0 + u |slope| (|t0| + e0), elsewhere e1 = L e0.  The max form
           v_max_f32(v, fl(slope v)) for 0 <= slope <= 1 returns the same value as the select (fl is monotone: v > 0 gives fl(slope v) <= v,
           v <= 0 gives fl(slope v) >= v), so one rule covers both.
  SIGMOID  L = 1/4; sigmoidf_ (1 / (1 + expf(-x))) itself is within 3 u of the exact sigmoid of its fp32 argument -- the term
           tests/osconv_cases.py uses for the same function (the result is <= 1: expf's relative error enters times s (1 - s) <= 1/4, the
           addition and the division round once each).  e1 = e0 / 4 + 3 u.
  mul      L = |mul| (exact fp32 input), one rounding: e2 = |mul| e1 + u (|t2| + |mul| e1).
  res1     L = 1, one rounding: e3 = e2 + u (|t3| + e2).  Absent: exact (zeros are added), e3 = e2.
  res2     p = res2_scale * res2 and the addition: the compiler may contract them into one FMA (one rounding of t3 + p) or not (p rounds,
           then the sum).  The bound takes the larger, uncontracted count: e' = e3 + u |p|, e4 = e' + u (|out| + e'); the FMA's error
           e3 + u (|out| + e3) is below it.
The same holds one step earlier: `v *= mul; v += res1` may become fma(v, mul, res1), which rounds once: its error |mul| e1 + u (|t3| +
|mul| e1) is below e3, because e2 >= |mul| e1.  No other pair of steps can fuse (the bias addition feeds a product, not a sum; the
activation stands between the bias and the mask).  `emulate32` has both contractions as switches and the CPU test runs all four forms.
Underflow plays no part: every operand of the cases below is O(1e-3) or larger or an exact zero.  `slope` and `res2_scale` are the fp32
values the descriptor holds (fp32(0.2), fp32(0.9)), converted exactly to float64.

Non-finite accumulators (fp16 mode only) follow include/savsr_hip.h: NONE, RELU and LRELU pass a NaN on and keep an infinity an infinity
-- RELU(-inf) = -inf, not 0, on every path (v_max_f32(v, v * 0) returns v when v * 0 is NaN); LRELU gives slope * (-inf); SIGMOID gives
exactly 0 / 1 / NaN.  `reference` computes that; `bound` is meaningless there and the GPU test compares classes.

Arrays are numpy, planar [c][h][w]; operands float32.  No GPU import.
"""
import itertools

import numpy as np

F32 = np.float32
U = 2.0 ** -24

NONE, RELU, LRELU, SIGMOID = 0, 1, 2, 3          # savsr_hip.h SAVSR_ACT_*, _lib.ACT_*
ACT_NAMES = {NONE: "none", RELU: "relu", LRELU: "lrelu", SIGMOID: "sigmoid"}
# the activations of the matrix: the max form (none, relu, lrelu 0.2), the select branch (slope outside [0, 1]), the sigmoid
ACTS = ((NONE, 0.0), (RELU, 0.0), (LRELU, 0.2), (LRELU, 1.5), (LRELU, -0.25), (SIGMOID, 0.0))
OPERANDS = ("bias", "mul", "res1", "res2")
SUBSETS = tuple(tuple(o for o, on in zip(OPERANDS, bits) if on) for bits in itertools.product((False, True), repeat=4))
RES2_SCALE = 0.9
REGIMES = ("unit", "large", "mirror")            # accumulator ~ operands; accumulator 1e3 x the operands; operands 1e3 x the accumulator
ACC_SCALE = dict(unit=1.0, large=1e3, mirror=1.0)
OP_SCALE = dict(unit=1.0, large=1.0, mirror=1e3)
SIGMOID_MAGS = (0.1, 5.0, 30.0, 100.0)           # the sigmoid input set: +-0.1, +-5, +-30, +-100 (expf overflows: exactly 0 or 1)


class Epilogue:
    """One epilogue: activation, slope and the operands that are present (float32 arrays, None = absent)."""

    def __init__(self, act=NONE, slope=0.0, bias=None, mul=None, res1=None, res2=None, res2_scale=RES2_SCALE):
        self.act, self.slope, self.res2_scale = act, float(F32(slope)), float(F32(res2_scale))      # as the descriptor holds them
        self.bias, self.mul, self.res1, self.res2 = bias, mul, res1, res2

    def with_(self, **kw):
        d = dict(act=self.act, slope=self.slope, bias=self.bias, mul=self.mul, res1=self.res1, res2=self.res2, res2_scale=self.res2_scale)
        d.update(kw)
        return Epilogue(**d)

    def subset(self):
        return tuple(o for o in OPERANDS if getattr(self, o) is not None)

    def name(self):
        a = ACT_NAMES[self.act] + (f" {self.slope:g}" if self.act == LRELU else "")
        return f"{a:11s} {subset_name(self.subset())}"


def subset_name(sub) -> str:
    return "".join(ch if o in sub else "-" for o, ch in zip(OPERANDS, "bm12"))


def act_name(act, slope) -> str:
    return ACT_NAMES[act] + (f" {slope:g}" if act == LRELU else "")


def matrix():
    """The 96 (act, slope, operand subset) combinations, activations fastest: neighbours in a launch differ in the activation, and every
    launch of 24 holds four operand subsets."""
    return [(act, slope, sub) for sub in SUBSETS for act, slope in ACTS]


def epilogue(act, slope, sub, ops) -> Epilogue:
    return Epilogue(act, slope, **{o: ops[o] for o in sub})


def _d(v):
    return np.asarray(v, dtype=np.float64)


def sigmoid64(x):
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))                   # (+-inf: exactly 1 / 0; a NaN stays a NaN through e)


def _act64(t, act, slope):
    if act == RELU:
        return np.where(t > 0, t, np.where(np.isfinite(t), 0.0, t))               # a non-finite value keeps its class (module docstring)
    if act == LRELU:
        with np.errstate(invalid="ignore"):
            return np.where(t > 0, t, slope * t)
    if act == SIGMOID:
        return sigmoid64(t)
    return t


def _chain(a, E: Epilogue):
    """(reference, bound): the float64 chain and the error recursion of the module docstring, step by step."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = _d(a)
        e = np.zeros_like(t)
        if E.bias is not None:
            t = t + _d(E.bias)[:, None, None]
            e = U * np.abs(t)
        if E.act == LRELU:
            lip = max(1.0, abs(E.slope))
            e = lip * e + np.where(t - e <= 0, U * abs(E.slope) * (np.abs(t) + e), 0.0)
        elif E.act == SIGMOID:
            e = e / 4 + 3 * U
        t = _act64(t, E.act, E.slope)
        if E.mul is not None:
            m = _d(E.mul)[None]
            t = t * m
            e = np.abs(m) * e
            e = e + U * (np.abs(t) + e)
        if E.res1 is not None:
            t = t + _d(E.res1)
            e = e + U * (np.abs(t) + e)
        if E.res2 is not None:
            p = E.res2_scale * _d(E.res2)
            t = t + p
            e = e + U * np.abs(p)
            e = e + U * (np.abs(t) + e)
    return t, e


def reference(a, E: Epilogue) -> np.ndarray:
    """E applied in float64 to the stored accumulators a [c][h][w]."""
    return _chain(a, E)[0]


def bound(a, E: Epilogue) -> np.ndarray:
    """Per element: the sum of the epilogue's own roundings, each propagated through the later steps (module docstring)."""
    return _chain(a, E)[1]


def sigmoid32(x):
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x.astype(F32)).astype(F32))).astype(F32)


def emulate32(a, E: Epilogue, fma: bool = False, fma_mask: bool = False) -> np.ndarray:
    """The chain in float32, in the kernels' operation order.  fma: res2_scale * res2 + t3 with ONE rounding (the contracted form; computed
    in float64, whose 53 bits hold the 48-bit product exactly) instead of two; fma_mask: the same for t1 * mul + res1 where both are there."""
    v = np.asarray(a, dtype=F32)
    if E.bias is not None:
        v = v + E.bias.astype(F32)[:, None, None]
    if E.act == RELU:
        v = np.maximum(v, v * F32(0))
    elif E.act == LRELU:
        sv = v * F32(E.slope)
        v = np.maximum(v, sv) if 0 <= E.slope <= 1 else np.where(v > 0, v, sv)
    elif E.act == SIGMOID:
        v = sigmoid32(v)
    if fma_mask and E.mul is not None and E.res1 is not None:
        v = (_d(v) * _d(E.mul)[None] + _d(E.res1)).astype(F32)
    else:
        if E.mul is not None:
            v = v * E.mul.astype(F32)[None]
        if E.res1 is not None:
            v = v + E.res1.astype(F32)
    if E.res2 is not None:
        if fma:
            v = (_d(F32(E.res2_scale)) * _d(E.res2) + _d(v)).astype(F32)
        else:
            v = v + F32(E.res2_scale) * E.res2.astype(F32)
    assert v.dtype == F32
    return v


# ----------------------------------------------------------------------------- inputs
def _rng(seed, *more):
    return np.random.RandomState([int(seed)] + [int(m) for m in more])


def _away(v, floor):
    """v with every magnitude brought into [floor, 2 floor] (signs kept): seen by a mutant that reads it, and a one-channel bias that
    large still leaves accumulators of both signs behind it."""
    return np.where(v < 0, -1.0, 1.0) * np.clip(np.abs(v), floor, 2 * floor)


def operands(c: int, h: int, w: int, seed: int, regime: str = "unit") -> dict:
    """bias [c] and res1 / res2 [c][h][w]: Gaussian, both signs, O(OP_SCALE[regime]); mul [h][w] uniform in (0.05, 0.95), never 0 or 1.
    The first channel quad of bias and of res1's first pixel is kept away from zero (the `absent_*` mutants read it)."""
    g, s = _rng(seed, REGIMES.index(regime)), OP_SCALE[regime]
    bias, res1, res2 = g.standard_normal(c), g.standard_normal((c, h, w)), g.standard_normal((c, h, w))
    bias[:4] = _away(bias[:4], 0.5)
    bias[0] = -abs(bias[0])          # (a one-channel conv keeps negative t0 = a + bias in the mirror regime too, where the bias decides the sign)
    res1[:4, 0, 0] = _away(res1[:4, 0, 0], 0.5)
    return dict(bias=(bias * s).astype(F32), mul=g.uniform(0.05, 0.95, (h, w)).astype(F32), res1=(res1 * s).astype(F32), res2=(res2 * s).astype(F32))


def accumulator(c: int, h: int, w: int, seed: int, regime: str = "unit") -> np.ndarray:
    """A stand-in for the stored accumulators in the CPU tests: Gaussian, both signs, O(ACC_SCALE[regime])."""
    return (_rng(seed, 7).standard_normal((c, h, w)) * ACC_SCALE[regime]).astype(F32)


def sigmoid_values(c: int, h: int, w: int, seed: int) -> np.ndarray:
    """The sigmoid input set: magnitudes 0.1, 5, 30, 100 (each +-5 %) in turn along the flat index, random signs."""
    g = _rng(seed, 11)
    n = c * h * w
    mag = np.asarray(SIGMOID_MAGS)[np.arange(n) % 4] * (1 + 0.05 * g.uniform(-1, 1, n))
    return (mag * np.where(g.uniform(size=n) < 0.5, -1.0, 1.0)).reshape(c, h, w).astype(F32)


def conv_inputs(cin: int, cout: int, ks: int, h: int, w: int, seed: int, regime: str = "unit"):
    """(x [cin][h][w], weight [cout][cin][ks][ks]) whose conv gives accumulators of both signs and of magnitude ~ACC_SCALE[regime] in every
    tile: Gaussian activations, Gaussian weights / sqrt(fan-in)."""
    g = _rng(seed, 13)
    x = g.standard_normal((cin, h, w))
    wt = g.standard_normal((cout, cin, ks, ks)) / np.sqrt(cin * ks * ks) * ACC_SCALE[regime]
    return x.astype(F32), wt.astype(F32)


def sigmoid_conv_inputs(cin: int, cout: int, ks: int, h: int, w: int, seed: int):
    """(x, weight) whose conv reproduces the sigmoid input set: x = sigmoid_values, the weight selects input channel co % cin at the centre
    tap (weight 1: exact in bf16 and fp16), so accumulator [co] ~ x[co % cin]."""
    wt = np.zeros((cout, cin, ks, ks), F32)
    wt[np.arange(cout), np.arange(cout) % cin, ks // 2, ks // 2] = 1
    return sigmoid_values(cin, h, w, seed), wt


def covers_sigmoid_set(t0) -> bool:
    """Whether t0 holds both signs of every magnitude class of the sigmoid input set (around 0.1, 5, 30 and 100)."""
    t0 = _d(t0)
    return all(bool(((s * t0 > lo) & (s * t0 < hi)).any()) for lo, hi in ((0, 2), (3, 8), (25, 35), (90, 110)) for s in (-1, 1))


# ----------------------------------------------------------------------------- mutants
def bf16(v: float) -> float:
    """v rounded to bfloat16 (RNE), as a Python float."""
    b = np.asarray([v], F32).view(np.uint32)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return float(b.view(F32)[0])


def _quad(t, c):
    """What an unconditional 16-byte load at offset 0 hands the lanes: the tensor's first four values, channel ch getting value ch % 4."""
    return np.resize(np.asarray(t, F32).reshape(-1)[:4] if t.ndim == 1 else np.asarray(t[:4, 0, 0], F32), c)


def _all_true(a):
    return np.ones(np.shape(a), bool)


def _neg_t0(a, E):
    return (_d(a) + (_d(E.bias)[:, None, None] if E.bias is not None else 0.0)) < 0


def _m_bias_after_act(a, E, ops):
    b = _d(E.bias)[:, None, None]
    out = reference(_d(_act64(_d(a), E.act, E.slope)) + b, E.with_(act=NONE, bias=None))
    return out, ~((_d(a) > 0) & (_d(a) + b > 0))             # (a > 0 and a + b > 0: both orders give a + b)


def _m_mask_before_act(a, E, ops):
    t = (_d(a) + (_d(E.bias)[:, None, None] if E.bias is not None else 0.0)) * _d(E.mul)[None]
    return reference(t, E.with_(bias=None, mul=None)), _all_true(a)


def _m_res1_before_mask(a, E, ops):
    t = _act64(_d(a) + _d(E.bias)[:, None, None], E.act, E.slope)
    t = (t + _d(E.res1)) * _d(E.mul)[None]
    return t + E.res2_scale * _d(E.res2), _all_true(a)


# name -> (act, slope, operands of the epilogue the mutant is judged on, fn(a, E, ops) -> (the mutant's output, elements it can change))
MUTANTS = {
    "slope_bf16":          (LRELU, 0.2, OPERANDS, lambda a, E, ops: (reference(a, E.with_(slope=bf16(0.2))), _neg_t0(a, E))),
    "res2_scale_bf16":     (LRELU, 0.2, OPERANDS, lambda a, E, ops: (reference(a, E.with_(res2_scale=bf16(RES2_SCALE))), _all_true(a))),
    # (sigmoid: ReLU and LeakyReLU commute with a positive factor; no bias: behind a bias 1e3 times the accumulator the sigmoid is 0 or 1 with
    # or without the mask in front of it)
    "mask_before_act":     (SIGMOID, 0.0, ("mul", "res1", "res2"), _m_mask_before_act),
    "res1_before_mask":    (LRELU, 0.2, OPERANDS, _m_res1_before_mask),
    "bias_after_act":      (LRELU, 0.2, OPERANDS, _m_bias_after_act),
    "res2_unscaled":       (LRELU, 0.2, OPERANDS, lambda a, E, ops: (reference(a, E.with_(res2_scale=1.0)), _all_true(a))),
    "mask_of_next_pixel":  (LRELU, 0.2, OPERANDS, lambda a, E, ops: (reference(a, E.with_(mul=np.roll(E.mul.reshape(-1), -1).reshape(E.mul.shape))),
                                                                    _all_true(a))),
    "res1_of_channel_c4":  (LRELU, 0.2, OPERANDS, lambda a, E, ops: (reference(a, E.with_(res1=np.roll(E.res1, -4, axis=0))), _all_true(a))),
    "relu_for_lrelu":      (LRELU, 0.2, OPERANDS, lambda a, E, ops: (reference(a, E.with_(act=RELU)), _neg_t0(a, E))),
    # an absent operand treated as present with the first quad of the tensor: what the interior paths' unconditional loads would add if the
    # select that sends them to the block of zeros were lost
    "absent_res1_as_quad": (RELU, 0.0, ("bias", "mul", "res2"),
                            lambda a, E, ops: (reference(a, E.with_(res1=np.broadcast_to(_quad(ops["res1"], a.shape[0])[:, None, None], a.shape))), _all_true(a))),
    "absent_bias_as_quad": (RELU, 0.0, ("mul", "res1", "res2"),
                            lambda a, E, ops: (reference(a, E.with_(bias=_quad(ops["bias"], a.shape[0]))), _all_true(a))),
}


def mutant_applies(name: str, c: int) -> bool:
    """`res1_of_channel_c4` needs a channel c + 4 that is another channel."""
    return name != "res1_of_channel_c4" or c > 4


def mutant_epilogue(name: str, ops: dict) -> Epilogue:
    act, slope, sub, _ = MUTANTS[name]
    return epilogue(act, slope, sub, ops)


def mutant_share(name: str, a, E: Epilogue, ops: dict, got) -> tuple:
    """(elements the mutant can change, share of them at which `got` leaves the bound around the MUTANT's output)."""
    out, can = MUTANTS[name][3](a, E, ops)
    seen = np.abs(_d(got) - out) > bound(a, E)
    return int(can.sum()), float((seen & can).sum()) / max(1, int(can.sum()))


def worst_ratio(got, a, E: Epilogue) -> float:
    """max |got - reference| / bound over the elements (0 / 0 counts as 0)."""
    ref, b = _chain(a, E)
    err = np.abs(_d(got) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(r.max())
