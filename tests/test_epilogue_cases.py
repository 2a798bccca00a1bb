"""tests/epilogue_cases.py on the CPU: the float32 emulation of the epilogue stays inside the derived bound on every element, for every
activation, operand subset and scale regime (each of `t1 * mul + res1` and `t3 + res2_scale * res2` contracted into an FMA or not); every mutant leaves it -- on at least one
element of every shape and regime, and at 12 x 33 in the unit regime on at least half of the elements the mutation can change.  The
mutant conditions are conditions on the INPUTS (operands away from zero where a mutant reads them, the mask away from 0 and 1): they are met
here by the reference alone, before any kernel runs."""
import numpy as np
import pytest

from tests import epilogue_cases as EC

# (c, h, w): the output shapes of tests/test_gpu_conv_epilogue.py's forms that differ in channel count or in how tiles end
SHAPES = [(64, 12, 33), (64, 7, 50), (16, 10, 12), (8, 5, 6), (1, 10, 12), (1, 5, 6), (64, 17, 34)]


@pytest.mark.parametrize("regime", EC.REGIMES)
@pytest.mark.parametrize("c,h,w", SHAPES)
def test_emulation_inside_bound(c, h, w, regime):
    a = EC.accumulator(c, h, w, 1, regime)
    a_sig = EC.sigmoid_values(c, h, w, 1)
    worst = {}
    for k, (act, slope, sub) in enumerate(EC.matrix()):
        E = EC.epilogue(act, slope, sub, EC.operands(c, h, w, 100 + k, regime))
        acc = a_sig if act == EC.SIGMOID and regime == "unit" else a
        ref, b = EC.reference(acc, E), EC.bound(acc, E)
        assert ref.dtype == np.float64 and bool(np.isfinite(ref).all()) and bool((b >= 0).all())
        for fma, fma_mask in ((False, False), (True, False), (False, True), (True, True)):
            got = EC.emulate32(acc, E, fma, fma_mask)
            err = np.abs(got.astype(np.float64) - ref)
            assert bool((err <= b).all()), (E.name(), fma, fma_mask, EC.worst_ratio(got, acc, E))
            key = EC.act_name(act, slope)
            worst[key] = max(worst.get(key, 0.0), EC.worst_ratio(got, acc, E))
        if not sub and act in (EC.NONE, EC.RELU):
            assert bool((b == 0).all()) and bool((EC.emulate32(acc, E) == ref).all())          # nothing rounds: the bare result, exactly
    print(f"{c} x {h} x {w} {regime}: worst |emulate32 - reference| / bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) > 0.1                                                           # the bound is not slack by orders of magnitude


def test_sigmoid_input_set():
    """+-0.1, +-5, +-30, +-100 are all there (the operand subsets without a bias see them unshifted); at +-100 the float32 sigmoid is exactly
    0 or 1."""
    for c, h, w in SHAPES:
        if c * h * w < 64:
            continue
        a = EC.sigmoid_values(c, h, w, 1)
        assert EC.covers_sigmoid_set(a)
        got = EC.emulate32(a, EC.Epilogue(EC.SIGMOID))
        big = np.abs(a) > 90
        assert bool(big.any()) and bool((got[big & (a < 0)] == 0).all()) and bool((got[big & (a > 0)] == 1).all())
        assert bool(((got > 0) & (got < 1)).any())
    x, wt = EC.sigmoid_conv_inputs(16, 1, 3, 10, 12, 5)
    assert wt.sum() == 1 and wt[0, 0, 1, 1] == 1 and EC.covers_sigmoid_set(x[0])


def test_operand_conditions():
    for regime in EC.REGIMES:
        ops = EC.operands(64, 12, 33, 9, regime)
        assert 0.05 <= float(ops["mul"].min()) and float(ops["mul"].max()) <= 0.95
        s = EC.OP_SCALE[regime]
        assert float(np.abs(ops["bias"][:4]).min()) >= 0.5 * s * (1 - 1e-6) and float(np.abs(ops["res1"][:4, 0, 0]).min()) >= 0.5 * s * (1 - 1e-6)
        for k in ("bias", "res1", "res2"):
            assert bool((ops[k] > 0).any()) and bool((ops[k] < 0).any()) and ops[k].dtype == np.float32
    assert EC.bf16(0.2) == 0.2001953125 and EC.bf16(0.9) == 0.8984375
    assert len(EC.matrix()) == 96 and len(set(EC.matrix())) == 96


@pytest.mark.parametrize("name", list(EC.MUTANTS))
def test_mutants_leave_the_bound(name):
    """Against the float32 emulation of the CORRECT epilogue (both res2 forms), every mutant used as the reference fails the bound."""
    for c, h, w in SHAPES:
        if not EC.mutant_applies(name, c):
            continue
        for regime in EC.REGIMES:
            ops = EC.operands(c, h, w, 21, regime)
            a = EC.accumulator(c, h, w, 2, regime)
            E = EC.mutant_epilogue(name, ops)
            for fma in (False, True):
                got = EC.emulate32(a, E, fma)
                assert EC.worst_ratio(got, a, E) <= 1.0
                n, share = EC.mutant_share(name, a, E, ops, got)
                if (c, h, w) == (64, 12, 33):
                    print(f"{name:20s} {regime:6s} fma={int(fma)}: leaves the bound on {100 * share:5.1f} % of the {n} elements it can change")
                assert n >= 1 and share * n >= 1, (name, (c, h, w), regime)
                if (c, h, w) == (64, 12, 33) and regime == "unit":
                    assert n >= c * h * w // 4 and share >= 0.5, (name, share)
