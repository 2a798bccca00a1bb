"""The self-ensemble on the host: the variant plan (shapes and swapped scales), the transforms against the order the reference's
SRModel.test_selfensemble builds its list in, the module switch, the taps refusal, the CLI flags and the argument checks of the
ABI 33 entry points (all refused before the device is touched)."""
import ctypes as C

import numpy as np
import pytest
import torch

from savsr_amd import _lib
from savsr_amd.engine import HipEngine
from savsr_amd.packing import get_hw
from tests.ensemble_cases import bits, fwd_np, inv_np, variant_scale
from tests.golden_cases import GRID_SIZES, YAML_SCALES


def _sizes_and_scales():
    rng = np.random.RandomState(13)
    cases = [(h, w, sh, sw) for h, w in GRID_SIZES for sh, sw in YAML_SCALES]
    for _ in range(3000):
        cases.append((int(rng.randint(2, 700)), int(rng.randint(2, 1300)), float(rng.randint(10, 41)) / 10, float(rng.randint(10, 41)) / 10))
    for _ in range(500):
        cases.append((int(rng.randint(2, 400)), int(rng.randint(2, 400)), float(rng.uniform(1, 4)), float(rng.uniform(1, 4))))
    return cases


def test_variant_plan_shapes_and_scales():
    for h, w, sh, sw in _sizes_and_scales():
        plan = HipEngine.ensemble_plan(h, w, (sh, sw))
        assert len(plan) == 8
        H, W = get_hw(h, w, (sh, sw))
        for k, ((hk, wk), sk) in enumerate(plan):
            assert sk == variant_scale(k, (sh, sw))
            if k >> 2:
                assert (hk, wk) == (w, h) and sk == (sw, sh)
                assert get_hw(hk, wk, sk) == (W, H), (h, w, sh, sw)       # a transposed variant's output is the exact transpose
            else:
                assert (hk, wk) == (h, w) and sk == (sh, sw)
                assert get_hw(hk, wk, sk) == (H, W)


def _reference_order(x: np.ndarray):
    """The list test_selfensemble builds: start from [x]; for 'v' (flip width), 'h' (flip height), 't' (transpose the last two dims) in
    turn, append that transform of every entry so far."""
    ops = {"v": lambda a: a[..., ::-1], "h": lambda a: a[..., ::-1, :], "t": lambda a: np.swapaxes(a, -1, -2)}
    lst = [x]
    for op in ("v", "h", "t"):
        lst.extend([np.ascontiguousarray(ops[op](a)) for a in lst])
    return lst


def _reference_inverse(y: np.ndarray, i: int) -> np.ndarray:
    """The undo step of test_selfensemble: 't' for i > 3, then 'h' for i % 4 > 1, then 'v' for odd i % 4."""
    if i > 3:
        y = np.swapaxes(y, -1, -2)
    if i % 4 > 1:
        y = y[..., ::-1, :]
    if (i % 4) % 2 == 1:
        y = y[..., ::-1]
    return np.ascontiguousarray(y)


def test_transforms_follow_the_reference_order():
    x = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)
    ref = _reference_order(x)
    assert len(ref) == 8
    for k in range(8):
        fw, fh, t = bits(k)
        assert (fw, fh, t) == (k & 1, (k >> 1) & 1, k >> 2)
        y = fwd_np(x, k)
        assert np.array_equal(y, ref[k]), k
        assert y.shape == ((2, 3, 7, 5) if t else (2, 3, 5, 7))
        assert np.array_equal(inv_np(y, k), x), k
        assert np.array_equal(inv_np(y, k), _reference_inverse(y, k)), k
    assert len({fwd_np(x, k).tobytes() for k in range(8)}) == 8          # eight different variants


def _net():
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(num_feat=32, n_resgroups=1, n_resblocks=1).eval()


def test_switch_is_module_state():
    net = _net()
    assert net.self_ensemble is False
    keys = set(net.state_dict())
    net.set_self_ensemble(True)
    assert net.self_ensemble is True
    assert set(net.state_dict()) == keys                       # not in state_dict()
    net = net.to(torch.float32).to("cpu")
    assert net.self_ensemble is True
    net.load_state_dict(_net().state_dict(), strict=True)
    assert net.self_ensemble is True
    net.set_precision("fp16")
    assert net.self_ensemble is True and net.precision == "fp16"
    net.set_self_ensemble(False)
    assert net.self_ensemble is False


def test_taps_refused_with_the_ensemble():
    net = _net()
    net.set_self_ensemble(True)
    with pytest.raises(ValueError, match="taps"):
        net(torch.zeros(1, 7, 3, 8, 8), taps={})


def test_cli_flags():
    from savsr_amd import test as T
    from savsr_amd import upscale as U
    base = ["-i", "in", "-o", "out", "--scale", "3.5", "2", "--checkpoint", "x.pth"]
    assert U.parse_args(base).self_ensemble is False
    assert U.parse_args(base + ["--self-ensemble"]).self_ensemble is True
    assert T.parse_args(["-opt", "x.yml"]).self_ensemble is False
    a = T.parse_args(["-opt", "x.yml", "--self-ensemble", "--precision", "fp16"])
    assert a.self_ensemble is True and a.precision == "fp16"
    assert T.parse_args(["-opt", "x.yml", "--check-readme"]).check_readme is True


def test_check_readme_refused_with_the_ensemble(capsys):
    from savsr_amd import test as T
    with pytest.raises(SystemExit) as e:
        T.parse_args(["-opt", "x.yml", "--self-ensemble", "--check-readme"])
    assert e.value.code == 2
    assert "single-pass" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.main(["-opt", "x.yml", "--check-readme", "--self-ensemble"])


def test_abi_entries_refuse_bad_arguments():
    """Refused before anything is enqueued: the pointers below are never dereferenced."""
    lib = _lib.load()
    idx = (C.c_int32 * 3)(0, 1, 2)
    fake = 1 << 20
    for gather, tag in ((lib.savsr_ensemble_gather_u8, b"ensemble_gather_u8"), (lib.savsr_ensemble_gather_f32, b"ensemble_gather_f32")):
        assert gather(None, 3, 3, 4, 4, idx, 3, 0, fake, None) == -1          # null frames
        assert tag in lib.savsr_last_error()
        assert gather(fake, 3, 3, 4, 4, idx, 3, 0, None, None) == -1          # null out
        assert gather(fake, 3, 3, 4, 4, idx, 3, 8, fake, None) == -1          # k = 8
        assert b"variant 8" in lib.savsr_last_error()
        assert gather(fake, 3, 3, 4, 4, idx, 3, -1, fake, None) == -1
        assert gather(fake, 3, 4, 4, 4, idx, 3, 0, fake, None) == -1          # c = 4
        assert gather(fake, 3, 0, 4, 4, idx, 3, 0, fake, None) == -1          # c = 0
        assert gather(fake, 2, 3, 4, 4, idx, 3, 0, fake, None) == -1          # frame 2 of 2
        assert gather(fake, 3, 3, 4, 4, None, 3, 0, fake, None) == -1         # null index list
        assert gather(fake, 3, 3, 4, 4, (C.c_int32 * 65)(), 65, 0, fake, None) == -1     # > SAVSR_VIDEO_MAX_SLOTS
        assert gather(fake, 3, 3, 0, 4, idx, 3, 0, fake, None) == -1          # h = 0
    offs = (C.c_int64 * 8)(*range(8))
    assert lib.savsr_ensemble_merge(None, offs, 3, 8, 8, 0, fake, None) == -1
    assert b"ensemble_merge" in lib.savsr_last_error()
    assert lib.savsr_ensemble_merge(fake, None, 3, 8, 8, 0, fake, None) == -1
    assert lib.savsr_ensemble_merge(fake, offs, 3, 8, 8, 0, None, None) == -1
    assert lib.savsr_ensemble_merge(fake, offs, 4, 8, 8, 0, fake, None) == -1     # c = 4
    assert lib.savsr_ensemble_merge(fake, offs, 0, 8, 8, 1, fake, None) == -1
    assert lib.savsr_ensemble_merge(fake, offs, 3, 0, 8, 0, fake, None) == -1
    assert lib.savsr_ensemble_merge(fake, offs, 3, 8, 8, 2, fake, None) == -1     # out_u8 not 0 / 1
