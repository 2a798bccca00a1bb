"""conv_wy.hip after its instruction diet (the (hi, lo) split from ONE packed conversion per pair of values; waves whose row pair lies below
the image stage nothing while the staged phase is theirs too): the outputs AND the fused pool partials are those of the parent commit's
library, bit for bit, and a wave that skipped its staging leaks nothing of the stale LDS it left in place.

The comparisons against the parent need a library built from the parent commit (its libsavsr_hip.so under another name), named by the
environment variable SAVSR_PARENT_LIB; without it those tests SKIP and say so, and only test_dead_waves_ignore_stale_lds runs.  Every
height class (0, 1, 2, 3, 4 row pairs left over by the 16-row tiles, and the strips-only image) and both widths that are no multiple of
32 are test cases of their own; profiles/conv_wy_diet_tests_vs_parent.log is the run with the parent library, in which none skipped.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARENT_ENV = "SAVSR_PARENT_LIB"
COUT = 64


@pytest.fixture(scope="module")
def eng(synth_sd):
    from savsr_amd.engine import HipEngine
    from savsr_amd.archs.savsr_arch import SAVSR
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return HipEngine(synth_sd, SAVSR().cfg, torch.device("cuda:0"))


@pytest.fixture(scope="module")
def parent():
    from savsr_amd import _lib
    path = os.environ.get(PARENT_ENV)
    if not path:
        pytest.skip(f"{PARENT_ENV} is not set: no parent-built library to compare with (build the parent commit's library and name it there)")
    assert os.path.isfile(path), f"{PARENT_ENV}={path}: no such file"
    lib = C.CDLL(os.path.abspath(path))
    res, args = _lib.SIGNATURES["savsr_conv2d_batch"]
    lib.savsr_conv2d_batch.restype, lib.savsr_conv2d_batch.argtypes = res, args
    lib.savsr_prepare_device.restype = C.c_int
    lib.savsr_last_error.restype = C.c_char_p
    assert lib.savsr_prepare_device() == 0, lib.savsr_last_error()
    return lib


class Batch:
    """n distinct 3x3 convs cin -> 64 at h x w (bias, LeakyReLU, residual, pool partials) as one descriptor array per Winograd-y flavour."""

    def __init__(self, eng, n, cin, h, w, seed):
        from savsr_amd import _lib
        from savsr_amd import engine as E
        from savsr_amd._lib import ACT_LRELU
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(seed)
        nsrc = max(1, cin // 64)
        self.n, self.h, self.w = n, h, w
        self.keep, self.outs, self.parts = [], [], []
        descs = {_lib.CONV_WINOGRAD_Y: [], _lib.CONV_WINOGRAD_Y_THROUGHPUT: []}
        rows = eng.pool_rows(h, w)
        for _ in range(n):
            wt = torch.randn(COUT, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
            img, bias = E.pack_conv_weight_wy(wt).to(dev), torch.randn(COUT, generator=g).to(dev)
            xs = [torch.randn(h, w, cin // nsrc, generator=g).to(dev) for _ in range(nsrc)]
            res = torch.randn(h, w, COUT, generator=g).to(dev)
            out, part = torch.empty(h, w, COUT, device=dev), torch.empty(rows, COUT, device=dev)
            self.keep.append((img, bias, xs, res))
            self.outs.append(out)
            self.parts.append(part)
            for algo, dl in descs.items():
                dl.append(eng.conv_desc("t", [eng.full(x) for x in xs], eng.full(out), h, w, ACT_LRELU, 0.2, res1=eng.full(res),
                                        weights=(img, bias, COUT, cin, 3, algo), pool=(part, 0, COUT)))
        self.arrs = {algo: (E.ConvDesc * n)(*dl) for algo, dl in descs.items()}

    def run(self, lib, algo):
        for t in self.outs + self.parts:
            t.fill_(float("nan"))
        rc = lib.savsr_conv2d_batch(self.arrs[algo], self.n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, lib.savsr_last_error())
        torch.cuda.synchronize()
        return [o.clone() for o in self.outs], [p.clone() for p in self.parts]


def _same_as_parent(eng, parent, n, cin, h, w, seed):
    from savsr_amd import _lib
    b = Batch(eng, n, cin, h, w, seed)
    for algo in (_lib.CONV_WINOGRAD_Y, _lib.CONV_WINOGRAD_Y_THROUGHPUT):
        want_o, want_p = b.run(parent, algo)
        got_o, got_p = b.run(eng.lib, algo)
        for k in range(n):
            assert bool(torch.isfinite(want_o[k]).all()) and bool(torch.isfinite(want_p[k]).all())
            assert torch.equal(got_o[k], want_o[k]), ("output differs from the parent's", n, cin, h, w, algo, k)
            assert torch.equal(got_p[k], want_p[k]), ("pool partials differ from the parent's", n, cin, h, w, algo, k)


@pytest.mark.parametrize("n,cin", [(6, 128), (6, 64), (2, 192)])
def test_headline_convs_equal_parent(eng, parent, n, cin):
    _same_as_parent(eng, parent, n, cin, 180, 320, seed=11)


# rows left over by the 16-row tiles: 176 -> 0 row pairs, 178 -> 1, 180 -> 2, 182 -> 3, 184 -> 4; 8 -> an image of strips only
@pytest.mark.parametrize("h", [176, 178, 180, 182, 184, 8])
def test_every_height_class_equals_parent(eng, parent, h):
    _same_as_parent(eng, parent, 6, 128, h, 320, seed=12)


@pytest.mark.parametrize("h,w", [(180, 180), (180, 176), (182, 180), (90, 176)])
def test_ragged_widths_equal_parent(eng, parent, h, w):
    _same_as_parent(eng, parent, 6, 128, h, w, seed=13)


def _poison_lds(eng):
    """Every CU's LDS full of NaN patterns: a Winograd-y launch over NaN inputs (678 tiles: every workgroup of the persistent grid stages split
    NaNs into all eight V regions, then NaNs through the epilogue slices)."""
    from savsr_amd import _lib
    b = _poison_lds.batch
    if b is None:
        b = _poison_lds.batch = Batch(eng, 6, 64, 180, 320, seed=3)
        for (_, _, xs, _) in b.keep:
            for x in xs:
                x.fill_(float("nan"))
    out, _ = b.run(eng.lib, _lib.CONV_WINOGRAD_Y_THROUGHPUT)
    assert bool(torch.isnan(out[0]).all())


_poison_lds.batch = None


@pytest.mark.parametrize("h,w", [(182, 320), (90, 320), (90, 180), (22, 1280)])
def test_dead_waves_ignore_stale_lds(eng, h, w):
    """Images whose last tile row has waves below the image (182: one of a 4-pair strip; 90: three of a full tile; 22: five) -- those waves keep
    stale LDS in their V regions instead of staging zeros.  With every CU's LDS preconditioned to NaN patterns the outputs and pool partials stay
    finite, equal an undisturbed run's bit for bit, and the two flavours agree.  With a parent library they also equal the parent's."""
    from savsr_amd import _lib
    b = Batch(eng, 6, 128, h, w, seed=14)
    ref_o, ref_p = b.run(eng.lib, _lib.CONV_WINOGRAD_Y)
    for algo in (_lib.CONV_WINOGRAD_Y, _lib.CONV_WINOGRAD_Y_THROUGHPUT):
        _poison_lds(eng)
        got_o, got_p = b.run(eng.lib, algo)
        for k in range(b.n):
            assert bool(torch.isfinite(got_o[k]).all()) and bool(torch.isfinite(got_p[k]).all()), ("NaN leaked from stale LDS", h, w, algo, k)
            assert torch.equal(got_o[k], ref_o[k]) and torch.equal(got_p[k], ref_p[k]), (h, w, algo, k)


@pytest.mark.parametrize("h,w", [(182, 320), (90, 180)])
def test_dead_waves_after_poison_equal_parent(eng, parent, h, w):
    from savsr_amd import _lib
    b = Batch(eng, 6, 128, h, w, seed=15)
    for algo in (_lib.CONV_WINOGRAD_Y, _lib.CONV_WINOGRAD_Y_THROUGHPUT):
        _poison_lds(eng)
        want_o, want_p = b.run(parent, algo)
        _poison_lds(eng)
        got_o, got_p = b.run(eng.lib, algo)
        for k in range(b.n):
            assert bool(torch.isfinite(got_o[k]).all()) and bool(torch.isfinite(got_p[k]).all())
            assert torch.equal(got_o[k], want_o[k]) and torch.equal(got_p[k], want_p[k]), (h, w, algo, k)
