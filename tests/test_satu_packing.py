"""The SATU weight packers on the host (packing.fold_satu_nf, lanes_*, pack_satu_*): every lane layout against a plain loop that
transcribes include/savsr_hip.h's formula, the forms against each other bit for bit, and the float64 fold of the tuned row orders
against the oracle's STAUpsample + tail conv."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import savsr_oracle as O
from savsr_amd import packing as P
from savsr_amd.utils import synth
from tests.golden_cases import rnd
from tests.test_num_feat import p32_float64

ROW_P27 = lambda ky, kx, o: 3 * (3 * ky + kx) + o      # noqa: E731  (savsr_satu_*_tail, savsr_satu_nf_*)
TAPS = [(ky, kx, o) for ky in range(3) for kx in range(3) for o in range(3)]


def _mat(rows, cols, seed):
    return np.random.default_rng(seed).standard_normal((rows, cols))


# ----------------------------------------------------------------------------- the lane layouts, one loop per formula of the header
@pytest.mark.parametrize("rows,k,r0", [(32, 32, 0), (64, 64, 32), (96, 32, 64)])
def test_lanes_a_is_the_a_operand_order(rows, k, r0):
    m = _mat(rows, k, 1)
    ref = np.zeros((k // 16, 64, 8))
    for ks in range(k // 16):
        for lane in range(64):
            for j in range(8):
                ref[ks, lane, j] = m[r0 + (lane & 31)][16 * ks + 8 * (lane >> 5) + j]
    assert np.array_equal(P.lanes_a(m, r0), ref)


@pytest.mark.parametrize("rows,k,r0", [(32, 32, 0), (64, 64, 32)])
def test_lanes_acc_is_the_accumulator_order(rows, k, r0):
    m = _mat(rows, k, 2)
    ref = np.zeros((k // 16, 64, 8))
    for g in range(k // 16):
        for lane in range(64):
            for j in range(8):
                ref[g, lane, j] = m[r0 + (lane & 31)][32 * (g // 2) + 16 * (g % 2) + 8 * (j // 4) + 4 * (lane >> 5) + j % 4]
    got = P.lanes_acc(m, r0)
    assert np.array_equal(got, ref)
    # the k of register j of lane half `half` in k step g is the accumulator row the LR stage holds there
    for g in range(k // 16):
        for half in range(2):
            for j in range(8):
                assert got[g, 32 * half + 5, j] == m[r0 + 5][32 * (g // 2) + P.acc_row(8 * (g % 2) + j, half)]


@pytest.mark.parametrize("c", [32, 64])
def test_lanes_kconv_groups(c):
    wk = _mat(25 * c, c, 3)
    ref = np.zeros((25, c // 32, c // 16, 64, 8))
    for tap in range(25):
        for cg in range(c // 32):
            for ks in range(c // 16):
                for lane in range(64):
                    for j in range(8):
                        ref[tap, cg, ks, lane, j] = wk[25 * (32 * cg + (lane & 31)) + tap][16 * ks + 8 * (lane >> 5) + j]
    assert np.array_equal(P.lanes_kconv(wk, c), ref)


@pytest.mark.parametrize("rows,r0", [(32, 0), (64, 32)])
def test_lanes_wbe_tile_order(rows, r0):
    wbe = np.random.default_rng(4).standard_normal((4, rows, 8))
    ref = np.zeros((2, 64, 8))
    for ks in range(2):
        for lane in range(64):
            for j in range(8):
                k = 16 * ks + 8 * (lane >> 5) + j                       # = 8 n + j
                ref[ks, lane, j] = wbe[k // 8][r0 + (lane & 31)][k % 8]
    assert np.array_equal(P.lanes_wbe(wbe, r0), ref)


@pytest.mark.parametrize("tiles", [1, 2])
def test_bias_acc_order(tiles):
    b = np.random.default_rng(5).standard_normal(32 * tiles)
    ref = np.zeros((2, 16 * tiles))
    for half in range(2):
        for t in range(tiles):
            for r in range(16):
                ref[half, 16 * t + r] = b[32 * t + 8 * (r // 4) + 4 * half + r % 4]
    assert np.array_equal(P.bias_acc_order(b), ref)


def test_row_q_is_a_permutation_of_27_rows():
    rows = [P.row_q(*t) for t in TAPS]
    assert len(set(rows)) == 27 and all(0 <= r < 32 for r in rows)
    for ky in range(3):
        for o in range(3):
            g = 3 * ky + o
            gi, half = (g, 0) if g < 5 else (g - 5, 1)
            assert [P.row_q(ky, kx, o) for kx in range(3)] == [P.acc_row(3 * gi + kx, half) for kx in range(3)]


# ----------------------------------------------------------------------------- the forms against each other
def _parts(img):
    """split-bf16 image (int16 [n][2][512]) -> (hi, lo) as flat int16 arrays in element order."""
    a = img.numpy().reshape(-1, 2, 512)
    return a[:, 0].reshape(-1), a[:, 1].reshape(-1)


def _unlay(layout, shape, values):
    """Inverse of a lane layout: the matrix `shape` whose image under `layout` is `values` (every element of the matrix is read once)."""
    idx = layout(np.arange(int(np.prod(shape))).reshape(shape)).reshape(-1)
    assert np.array_equal(np.sort(idx), np.arange(int(np.prod(shape))))
    out = np.zeros(int(np.prod(shape)), dtype=values.dtype)
    out[idx] = values
    return out.reshape(shape)


@pytest.mark.parametrize("seed", [0, 3])
def test_generic_packer_at_64_equals_the_tuned_27_plane_form(seed):
    sd = synth.synth_state_dict(seed=seed)
    nf, plain, p27 = P.pack_satu_nf(sd, 64), P.pack_satu_tuned(sd, "plain"), P.pack_satu_tuned(sd, "p27")
    assert nf["kconv_w"].dtype == torch.int16 and nf["kconv_w"].numel() == 2 * 25 * 64 * 64
    assert torch.equal(nf["kconv_w"], plain["kconv_w"])
    assert torch.equal(nf["kconv_b"], plain["kconv_b"])
    assert nf["proj_w"].numel() == 2 * 3 * 32 * 64
    assert torch.equal(nf["proj_w"], p27["proj_w"])
    assert set(p27) == {"proj_w", "wbe_w", "fusion_b"}
    # the generic form's fp32 wbe [n][j][p] and fb are the tuned form's images, un-laid
    wbe_hi, wbe_lo = (_unlay(P.lanes_wbe, (4, 32, 8), v) for v in _parts(p27["wbe_w"]))
    hi, lo = _parts(P.split_bf16_image(nf["wbe"].permute(0, 2, 1).contiguous().reshape(-1)))
    assert np.array_equal(wbe_hi.reshape(-1), hi) and np.array_equal(wbe_lo.reshape(-1), lo)
    assert np.array_equal(_unlay(P.bias_acc_order, (32,), p27["fusion_b"].numpy().reshape(-1)), nf["fusion_b"].numpy())


@pytest.mark.parametrize("seed", [0, 3])
def test_row_summed_images_are_the_27_plane_rows_permuted(seed):
    sd = synth.synth_state_dict(seed=seed)
    p27, q = P.pack_satu_tuned(sd, "p27"), P.pack_satu_tuned(sd, "q")

    def matrices(t):
        """Every image decoded to matrices with the tail row p first: (hi, lo) of Wt Wa, Wt Wb, the C-stack, (Wt Wb E_n) [p][n][j]; Wt b."""
        out = []
        for part in _parts(t["proj_w"]):
            a, b, cs = part[:2048], part[2048:4096], part[4096:]
            out += [_unlay(P.lanes_acc, (32, 64), a), _unlay(P.lanes_a, (32, 64), b), _unlay(P.lanes_a, (32, 64), cs)]
        out += [_unlay(P.lanes_wbe, (4, 32, 8), part).transpose(1, 0, 2) for part in _parts(t["wbe_w"])]
        return out + [_unlay(P.bias_acc_order, (32,), t["fusion_b"].numpy().reshape(-1))]

    live_q = sorted(P.row_q(*t) for t in TAPS)
    dead_q = [r for r in range(32) if r not in live_q]
    for i, (m27, mq) in enumerate(zip(matrices(p27), matrices(q))):
        if i in (2, 5):                                     # the C-stack does not meet Wt
            assert np.array_equal(m27, mq)
            continue
        assert m27[:27].any()
        for t in TAPS:
            assert np.array_equal(mq[P.row_q(*t)], m27[ROW_P27(*t)]), (i, t)
        assert not m27[27:].any() and not mq[dead_q].any()


def test_plain_form_is_the_unprojected_fusion():
    """The plain form (savsr_satu_lr_stage / savsr_satu_hr_upsample): the fp32 fusion weight itself in the lane orders, two 32-row tiles."""
    sd = synth.synth_state_dict(seed=3)
    plain = P.pack_satu_tuned(sd, "plain")
    fus = sd["upsample.fusion.weight"].reshape(64, 128).numpy()
    comp = sd["upsample.weight_compress"].reshape(32, 64).numpy()
    ref = np.concatenate([P.lanes_acc(fus[:, :64], r).reshape(-1) for r in (0, 32)] + [P.lanes_a(fus[:, 64:], r).reshape(-1) for r in (0, 32)]
                         + [P.lanes_a(comp).reshape(-1)])
    assert torch.equal(plain["proj_w"], P.split_bf16_image(torch.from_numpy(ref)))
    assert torch.equal(plain["fusion_b"], torch.from_numpy(P.bias_acc_order(sd["upsample.fusion.bias"].numpy())))
    assert plain["fusion_b"].shape == (2, 32) and plain["wbe_w"].numel() == 2 * 2 * 2 * 512


def test_heads_are_the_coordinate_mlp(synth_sd):
    h = P.pack_satu_heads(synth_sd)
    assert torch.equal(h["body2_w"], synth_sd["upsample.body.2.weight"].reshape(64, 64).t())
    assert torch.equal(h["head_w"][4:6], synth_sd["upsample.offset.weight"].reshape(2, 64))
    assert torch.equal(h["head_b"][6:], synth_sd["upsample.st_offset.bias"])
    assert {k: tuple(v.shape) for k, v in h.items()} == dict(body0_w=(64, 4), body0_b=(64,), body2_w=(64, 64), body2_b=(64,), head_w=(8, 64),
                                                             head_b=(8,))


def test_struct_of_renames_and_later_dicts_win():
    from savsr_amd._lib import SatuNfWeights, SatuWeights
    a, b, c = torch.zeros(4), torch.zeros(4), torch.zeros(4)
    w = P.struct_of(SatuWeights, dict(proj_w=a, fusion_b=a), dict(proj_w=b, wbe=c), rename={"wbe": "wbe_w"})
    assert (w.proj_w, w.fusion_b, w.wbe_w) == (b.data_ptr(), a.data_ptr(), c.data_ptr()) and not w.kconv_w
    assert P.struct_of(SatuNfWeights, dict(wbe=c), C=32).C == 32


# ----------------------------------------------------------------------------- the fold of the tuned row orders against the oracle
@pytest.mark.parametrize("row_of", [ROW_P27, P.row_q], ids=["p27", "q"])
@pytest.mark.parametrize("h,w,sc", [(5, 7, (3.5, 2)), (7, 6, (4, 4))])
def test_tuned_folds_reproduce_satu_and_tail_conv(row_of, h, w, sc):
    """fold_satu_nf at 64 with the row order of a tuned tail form, evaluated the way the kernels evaluate it (LR record, two bilinear
    gathers, expert mixing, the nine shifted taps read at row_of), equals the oracle's STAUpsample followed by the 3x3 tail conv."""
    sd = synth.synth_state_dict(seed=4)
    x = rnd((1, 64, h, w), 71, 1.0)
    st = rnd((1, 64, h, w), 72, 0.6)
    with torch.no_grad():
        ref = F.conv2d(O.sta_upsample(sd, "upsample", x, sc, st), sd["tail.weight"], sd["tail.bias"], padding=1)[0].double()
    H, W = O.get_hw(h, w, sc)
    p = p32_float64(sd, 64, x, st, sc, row_of=row_of)
    live = [row_of(*t) for t in TAPS]
    assert float(p[[r for r in range(32) if r not in live]].abs().max()) == 0.0
    pp = F.pad(p, (1, 1, 1, 1))
    out = sd["tail.bias"].double()[:, None, None].repeat(1, H, W)
    for ky, kx, o in TAPS:
        out[o] += pp[row_of(ky, kx, o), ky:ky + H, kx:kx + W]
    err = float((out - ref).abs().max())
    print(row_of.__name__, sc, "folded float64 vs oracle", err, "magnitude", float(ref.abs().max()))
    assert err <= 1e-5
