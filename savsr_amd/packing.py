"""Weight images and SATU matrices for the HIP kernels, built once per engine (device-side scatter / split; float64 folds).

Host helpers (integer grids, index maps of the weight-image layouts, split-bf16 packing) and `WeightPacking`, the part of
`HipEngine` that turns a reference state_dict (791 keys, savsr_arch.py:576-636) into what the kernels read: BatchNorm folded into
the convs (:191-204), every conv as a split-bf16 image in MFMA lane order (direct and, for static 3x3 convs, Winograd-y), the OSConv
kernel banks + routing / attention matrices (:139-172), the SATU matrices with the tail conv's channel contraction folded in
(:315-376, :738).  Pure data movement + RNE conversions; include/savsr_hip.h documents every layout.

SATU, every form: ONE float64 fold (`fold_satu_nf`; the forms differ in the row order of Wt, `tail_rows27`), ONE set of lane layouts
(`lanes_*`, `bias_acc_order`), pure host packers sd -> {name: host tensor} (`pack_satu_heads`, `pack_satu_nf`, `pack_satu_tuned`; testable
without a GPU, tests/test_satu_packing.py); `WeightPacking._pack_satu` only uploads them and fills the structs (`struct_of`).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SatuNfWeights, SatuWeights

BN_EPS = 1e-5


# ----------------------------------------------------------------------------- host helpers (integer / grid logic)
def get_hw(h: int, w: int, scale: Sequence[float]) -> Tuple[int, int]:
    """Output size, savsr_arch.py:745-751 (Python round = half-to-even on the double product)."""
    return round(h * scale[0]), round(w * scale[1])


def satu_axis_tables(n_out: int, n_in: int, s: float):
    """Per-axis SATU tables, evaluated in fp32 exactly like the reference's torch CPU ops.

    Returns (coor, floor_idx, grid_norm):
      coor      = (i+.5)/s - floor((i+.5)/s + 1e-3) - .5          savsr_arch.py:331-333
      floor_idx = floor((i+.5)/s + 1e-3)  (the integer LR index grid, bit-exact contract)
      grid_norm = ((i+.5)/s - .5) * 2 / (n_in-1) - 1              savsr_arch.py:270-280
    """
    f32 = np.float32
    i = np.arange(n_out, dtype=np.float32)
    q = (i + f32(0.5)) / f32(s)
    fl = np.floor(q + f32(1e-3))
    coor = (q - fl) - f32(0.5)
    g = (i + f32(0.5)) / f32(s) - f32(0.5)
    g = (g * f32(2)) / f32(n_in - 1) - f32(1)
    return coor.astype(np.float32), fl.astype(np.int32), g.astype(np.float32)


_PACK_IDX_CACHE: Dict[Tuple[int, int, int], Tuple[np.ndarray, int]] = {}

CONV_TH, CONV_TW = 8, 32      # pixel tile of one conv workgroup (mirrors common.hpp)


def conv_pack_geometry(cout: int, cin: int, ks: int):
    kc = 16 if ks == 3 else 32
    cot = 64 if cout > 32 else 32
    if cin % kc:
        raise ValueError(f"conv cin={cin} must be a multiple of {kc} (pad the weight with zero channels)")
    return kc, cot, cin // kc, (cout + cot - 1) // cot


def conv_pack_index(cout: int, cin: int, ks: int):
    """Index map [cout, cin, ks*ks] -> position inside one part of the weight image
    (mirror of savsr_conv_pack_index)."""
    key = (cout, cin, ks)
    if key not in _PACK_IDX_CACHE:
        kc, cot, nchunk, ncob = conv_pack_geometry(cout, cin, ks)
        taps, nt, ksteps = ks * ks, cot // 32, kc // 16
        co = np.arange(cout, dtype=np.int64)[:, None, None]
        ci = np.arange(cin, dtype=np.int64)[None, :, None]
        tap = np.arange(taps, dtype=np.int64)[None, None, :]
        cob, col = co // cot, co % cot
        t, row = col // 32, col % 32
        chunk, cl = ci // kc, ci % kc
        kstep, kh, j = cl // 16, (cl % 16) // 8, cl % 8
        group = (((cob * nchunk + chunk) * taps + tap) * ksteps + kstep) * nt + t
        idx = group * 512 + (kh * 32 + row) * 8 + j
        total = ncob * nchunk * taps * kc * cot
        _PACK_IDX_CACHE[key] = (np.array(np.broadcast_to(idx, (cout, cin, taps))).reshape(-1), total)      # (a writable copy: torch.from_numpy warns on read-only views)
    return _PACK_IDX_CACHE[key]


_IDX_DEV_CACHE: Dict[tuple, torch.Tensor] = {}


def _index_on(kind: str, key: tuple, idx: np.ndarray, device: torch.device) -> torch.Tensor:
    """The (cached) index map of a weight-image layout as a tensor on `device`."""
    k = (kind, key, str(device))
    t = _IDX_DEV_CACHE.get(k)
    if t is None:
        t = torch.from_numpy(idx).to(device)
        _IDX_DEV_CACHE[k] = t
    return t


def _scatter_image(idx: np.ndarray, total: int, values: torch.Tensor, kind: str, key: tuple, device: Optional[torch.device]) -> torch.Tensor:
    """zeros[total] with values scattered to idx: numpy on the host, one index_put on a GPU (round 5: the engine packs its ~190 conv
    images and 12 OSConv banks ON THE DEVICE -- 1.7 s of host scatter / split work per process became a few ms; a rank of an 8-GPU run of
    a YAML spends 2-7 s on the GPU in all).  Pure data movement + RNE conversions: bit-identical either way
    (tests/test_gpu_kernels.py::test_weight_images_packed_on_device_equal_host_packing)."""
    if device is None or device.type == "cpu":
        out = np.zeros(total, dtype=np.float32)
        out[idx] = values.detach().to("cpu", torch.float32).contiguous().numpy().reshape(-1)
        return torch.from_numpy(out)
    out = torch.zeros(total, dtype=torch.float32, device=device)
    out[_index_on(kind, key, idx, device)] = values.detach().to(device, torch.float32).reshape(-1)
    return out


def pack_conv_part(w: torch.Tensor, device: Optional[torch.device] = None) -> torch.Tensor:
    """[cout, cin, k, k] -> fp32 tensor of one image part (zero padded), lane order; on `device` (default: host)."""
    cout, cin, ks, _ = w.shape
    idx, total = conv_pack_index(cout, cin, ks)
    return _scatter_image(idx, total, w, "direct", (cout, cin, ks), device)


def split_bf16_image(part: torch.Tensor) -> torch.Tensor:
    """fp32 part [n*512] -> int16 image [n][2][512]: hi = bf16(v), lo = bf16(v - hi) (RNE both)."""
    hi = part.to(torch.bfloat16)
    lo = (part - hi.to(torch.float32)).to(torch.bfloat16)
    img = torch.stack([hi.view(-1, 512), lo.view(-1, 512)], dim=1).contiguous()
    return img.view(torch.int16).reshape(-1)


def pack_conv_weight(w: torch.Tensor, device: Optional[torch.device] = None) -> torch.Tensor:
    """[cout, cin, k, k] -> split-bf16 weight image (int16 tensor) for savsr_conv2d."""
    return split_bf16_image(pack_conv_part(w, device))


_WY_IDX_CACHE: Dict[tuple, tuple] = {}


def conv_wy_pack_index(cout: int, cin: int):
    """Index map [4 pos, cout, cin, 3 kx] -> position inside one part of the Winograd-y weight image (mirror of
    savsr_conv_wy_pack_index): [cob][chunk][hf][s = vr * 3 + kx][t] groups of 512 = (kh * 32 + row) * 8 + j."""
    key = (cout, cin)
    if key not in _WY_IDX_CACHE:
        if cout % 64 or cin % 16:
            raise ValueError("Winograd-y conv image: cout must be a multiple of 64 and cin of 16")
        nchunk = cin // 16
        pos = np.arange(4, dtype=np.int64)[:, None, None, None]
        co = np.arange(cout, dtype=np.int64)[None, :, None, None]
        ci = np.arange(cin, dtype=np.int64)[None, None, :, None]
        kx = np.arange(3, dtype=np.int64)[None, None, None, :]
        cob, col = co // 64, co % 64
        t, row = col // 32, col % 32
        chunk, cl = ci // 16, ci % 16
        kh, j = cl // 8, cl % 8
        hf, vr = pos // 2, pos % 2
        group = (((cob * nchunk + chunk) * 2 + hf) * 6 + (vr * 3 + kx)) * 2 + t
        idx = group * 512 + (kh * 32 + row) * 8 + j
        total = (cout // 64) * nchunk * 12 * 16 * 64
        _WY_IDX_CACHE[key] = (np.array(np.broadcast_to(idx, (4, cout, cin, 3))).reshape(-1), total)
    return _WY_IDX_CACHE[key]


def _wy_transform(g: torch.Tensor) -> torch.Tensor:
    """The F(2,3) weight transform over the tap ROWS g_ky of a float64 [cout][cin][3 ky][3 kx] weight: U0 = g0, U1 = (g0 + g1 + g2) / 2,
    U2 = (g0 - g1 + g2) / 2, U3 = g2, per kx -> [4 pos][cout][cin][3 kx]."""
    g0, g1, g2 = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    return torch.stack([g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2], 0)


def pack_conv_part_wy(w: torch.Tensor, device: Optional[torch.device] = None) -> torch.Tensor:
    """[cout, cin, 3, 3] -> fp32 tensor of one part of the Winograd-y image (zero padded), lane order: _wy_transform in float64 (on
    `device`), rounded once to fp32."""
    cout, cin, ks, _ = w.shape
    assert ks == 3
    dev = device if device is not None and device.type != "cpu" else torch.device("cpu")
    u = _wy_transform(w.detach().to(dev, torch.float64)).to(torch.float32)
    idx, total = conv_wy_pack_index(cout, cin)
    return _scatter_image(idx, total, u, "wy", (cout, cin), device)


def pack_conv_weight_wy(w: torch.Tensor, device: Optional[torch.device] = None) -> torch.Tensor:
    """[cout, cin, 3, 3] -> split-bf16 Winograd-y weight image (SAVSR_CONV_WINOGRAD_Y): pack_conv_part_wy, then (hi, lo)."""
    return split_bf16_image(pack_conv_part_wy(w, device))


# ----------------------------------------------------------------------------- the RCAB's SE gate folded into conv.2 (savsr_rcab_gate_weights_batch)
def tap_sums_border(r1: torch.Tensor) -> torch.Tensor:
    """S [c][3 ky][3 kx] of a [c][h][w] map: its sum over the pixels tap (ky, kx) of a zero-padded 3x3 conv sees, in the border form the
    kernel evaluates -- the channel's total, less the bottom (ky = 0) / top (ky = 2) row and the right (kx = 0) / left (kx = 2) column,
    plus the corner both took away.  In r1's dtype (the tests run it in float64)."""
    tot = r1.sum((1, 2))
    rows = {0: r1[:, -1].sum(1), 2: r1[:, 0].sum(1)}                 # the row tap ky never sees
    cols = {0: r1[:, :, -1].sum(1), 2: r1[:, :, 0].sum(1)}
    crn = {(0, 0): r1[:, -1, -1], (0, 2): r1[:, -1, 0], (2, 0): r1[:, 0, -1], (2, 2): r1[:, 0, 0]}
    s = tot[:, None, None].repeat(1, 3, 3)
    for ky in range(3):
        for kx in range(3):
            if ky in rows:
                s[:, ky, kx] -= rows[ky]
            if kx in cols:
                s[:, ky, kx] -= cols[kx]
            if (ky, kx) in crn:
                s[:, ky, kx] += crn[(ky, kx)]
    return s


def rcab_fold_tables(w: torch.Tensor, b: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The SE gate's first layer composed with conv.2 (w [c, c, 3, 3], b [c]; w1 [cmid, c], b1 [cmid]), in the `A` form: with S the
    tap sums of conv.2's INPUT (tap_sums_border) and n = h w,  w1 mean(conv.2) + b1 = A S / n + cz,  A = w1 W.reshape(c, c 9) as
    [cmid][c * 9] (column ci * 9 + 3 ky + kx), cz = w1 b + b1.  float64 products, rounded once to fp32."""
    c = w.shape[0]
    w1d = w1.detach().to("cpu", torch.float64).reshape(-1, c)
    a = w1d @ w.detach().to("cpu", torch.float64).reshape(c, -1)
    cz = w1d @ b.detach().to("cpu", torch.float64) + b1.detach().to("cpu", torch.float64)
    return a.to(torch.float32).contiguous(), cz.to(torch.float32).contiguous()


FP16_MAX = 65504.0      # largest finite fp16: the operand range of the precision mode "fp16"


def _f16_image(idx: np.ndarray, total: int, values: np.ndarray) -> torch.Tensor:
    """int16 view of an fp16 image: zeros[total] with float16(values) (RNE, straight from float64 by numpy) scattered to idx."""
    out = np.zeros(total, dtype=np.float16)
    out[idx] = np.asarray(values, dtype=np.float64).reshape(-1).astype(np.float16)
    return torch.from_numpy(out.view(np.int16))


def pack_conv_weight_f16(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, k, k] -> fp16 weight image (int16 tensor on the host) for savsr_conv2d_batch_f16: ONE part, fp16(W) at position p of
    savsr_conv_pack_index, no hi/lo interleave."""
    cout, cin, ks, _ = w.shape
    idx, total = conv_pack_index(cout, cin, ks)
    return _f16_image(idx, total, w.detach().to("cpu", torch.float64).numpy())


def wy_transform_f64(w: torch.Tensor) -> np.ndarray:
    """[cout, cin, 3, 3] -> the F(2,3)-along-y weight transform U [4 pos][cout][cin][3 kx] in float64 (pack_conv_weight_wy's arithmetic)."""
    return _wy_transform(w.detach().to("cpu", torch.float64)).numpy()


def pack_conv_weight_wy_f16(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, 3, 3] -> fp16 Winograd-y weight image (int16 tensor on the host): U in float64, rounded ONCE to fp16, at position p of
    savsr_conv_wy_pack_index."""
    cout, cin, ks, _ = w.shape
    assert ks == 3
    idx, total = conv_wy_pack_index(cout, cin)
    return _f16_image(idx, total, wy_transform_f64(w))


def check_f16_range(name: str, a: np.ndarray) -> None:
    """Refuse an operand outside the fp16 range (it would become an infinity in the precision mode "fp16"), naming it.  Nothing is refused
    at the low side: below 2^-14 a weight is an fp16 subnormal, which the kernels keep and multiply as such."""
    m = float(np.abs(a).max()) if a.size else 0.0
    if not m <= FP16_MAX:
        raise ValueError(f"precision 'fp16': {name} has a weight of magnitude {m:.6g}, beyond the fp16 range (+-{FP16_MAX:g}); "
                         f"run this checkpoint with precision 'fp32'")


def acc_row(r: int, half: int) -> int:
    """Row of register r of a 32x32 MFMA accumulator for lane half `half`."""
    return (r & 3) + 8 * (r >> 2) + 4 * half


def tail_rows27(sd, c: int, row_of=None) -> np.ndarray:
    """Wt27 [32][c] (float64): the 3x3 tail conv's weights (savsr_arch.py:738, c -> nch = num_in_ch outputs) regrouped by output row
    p = row_of(ky, kx, o), by default nch (3 ky + kx) + o; rows 9 nch .. 31 zero (27 .. 31 for the shipped nch = 3)."""
    tw = sd["tail.weight"].to("cpu", torch.float64).numpy()                          # [nch o][c][3 ky][3 kx]
    nch = tw.shape[0]
    if nch > 3:
        raise ValueError(f"num_in_ch = {nch}: the 9 num_in_ch tail rows must fit the 32-row MFMA tile of the LRcat record (num_in_ch <= 3)")
    if row_of is None:
        row_of = lambda ky, kx, o: nch * (3 * ky + kx) + o      # noqa: E731
    wt27 = np.zeros((32, c), dtype=np.float64)
    for ky in range(3):
        for kx in range(3):
            for o in range(nch):
                wt27[row_of(ky, kx, o)] = tw[o, :, ky, kx]
    return wt27


def window_record(nch: int, sw: int) -> int:
    """Floats per pixel of a packed input window (savsr_pack_windows_nch): nch * sw live channels rounded up to 16 or 32."""
    return 16 if nch * sw <= 16 else 32


def row_q(ky: int, kx: int, o: int) -> int:
    """Row order of the row-summed tail form (savsr_satu_hr_tail_q, 3 channels): the three kx of group g = 3 ky + o at MFMA rows
    acc_row(3 gi + kx, half), groups 0 .. 4 in lane half 0 (gi = g), 5 .. 8 in half 1 (gi = g - 5)."""
    g = 3 * ky + o
    return acc_row(3 * g + kx, 0) if g < 5 else acc_row(3 * (g - 5) + kx, 1)


def fold_satu_nf(sd, c: int, row_of=None, tail: bool = True) -> Dict[str, np.ndarray]:
    """The matrices of every SATU form in float64 (savsr_arch.py:315-376, :738); Wt = tail_rows27(sd, c, row_of) [32][c] for the
    tail-projected forms (savsr_satu_nf_*, savsr_satu_*_tail with row_of = None, savsr_satu_hr_tail_q with row_q), the identity [c][c]
    (nothing multiplied) for the plain form, tail = False:
      kconv [25 c][c], kconv_b [25 c]   kernel_conv (row n = 25 ch + tap, :227), unchanged
      ta [rows][c] = Wt Wa              applies to sta (fusion's first half, :374)
      tb [rows][c] = Wt Wb              applies to x
      cstack [c/2][c]                   C_m rows at (c/8) m + j (weight_compress, :232-235)
      wbe [4][c/8][rows] = (Wt Wb E_n)[p][j] as [n][j][p]   (weight_expand, :238-241)
      fb [rows] = Wt b                  (fusion bias)"""
    p = "upsample."
    g = lambda k: sd[p + k].to("cpu", torch.float64).numpy()
    wt27 = tail_rows27(sd, c, row_of) if tail else None
    wt = lambda a: wt27 @ a if tail else a
    fus = g("fusion.weight").reshape(c, 2 * c)
    wa, wb = fus[:, :c], fus[:, c:]                                                   # cat((sta, fea)), :374
    expd = g("weight_expand").reshape(4, c, c // 8)                                   # E_n[c][j]
    tb = wt(wb)
    return dict(kconv=g("kernel_conv.0.weight").reshape(25 * c, c), kconv_b=g("kernel_conv.0.bias"),
                ta=wt(wa), tb=tb, cstack=g("weight_compress").reshape(c // 2, c),
                wbe=np.einsum("pc,ncj->njp", tb, expd), fb=wt(g("fusion.bias")))


# ----------------------------------------------------------------------------- MFMA lane layouts of the SATU images (include/savsr_hip.h,
# savsr_satu_weights / savsr_satu_nf_weights): pure index maps, every one [..][64 lanes][8 j] with the lane's row at (lane & 31)
_LANE, _J = np.arange(64)[:, None], np.arange(8)[None, :]
_LI, _LH = _LANE & 31, _LANE >> 5


def lanes_a(m: np.ndarray, r0: int = 0) -> np.ndarray:
    """A-operand k steps of the 32-row tile at r0: [K/16 ks][lane][j] = m[r0 + (lane & 31)][16 ks + 8 (lane >> 5) + j]."""
    ks = np.arange(m.shape[1] // 16)[:, None, None]
    return m[r0 + _LI, 16 * ks + 8 * _LH + _J]


def lanes_acc(m: np.ndarray, r0: int = 0) -> np.ndarray:
    """k steps in accumulator order (the B operand is an accumulator: k step g consumes registers 8 (g % 2) .. + 7 of channel group g / 2):
    [K/16 g][lane][j] = m[r0 + (lane & 31)][32 (g / 2) + 16 (g % 2) + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)]."""
    g = np.arange(m.shape[1] // 16)[:, None, None]
    return m[r0 + _LI, 32 * (g // 2) + 16 * (g % 2) + 8 * (_J >> 2) + 4 * _LH + (_J & 3)]


def lanes_kconv(wk: np.ndarray, c: int) -> np.ndarray:
    """kernel_conv groups of width c: [25 tap][c/32 cg][c/16 ks][lane][j] = wk[25 (32 cg + (lane & 31)) + tap][16 ks + 8 (lane >> 5) + j]."""
    tap, cg, ks = np.arange(25)[:, None, None, None, None], np.arange(c // 32)[:, None, None, None], np.arange(c // 16)[:, None, None]
    return wk[25 * (32 * cg + _LI) + tap, 16 * ks + 8 * _LH + _J]


def lanes_wbe(wbe: np.ndarray, r0: int = 0) -> np.ndarray:
    """The tuned (W E_n) tile at row r0 of wbe [4 n][rows][8 j]: [2 ks][lane][j] = wbe[2 ks + (lane >> 5)][r0 + (lane & 31)][j]
    (k = 16 ks + 8 (lane >> 5) + j = 8 n + j)."""
    ks = np.arange(2)[:, None, None]
    return wbe[2 * ks + _LH, r0 + _LI, _J]


def group_kconv(tap: int, cg: int, ks: int, c: int) -> int:
    """Index of the 512-element (hi | lo) group of lanes_kconv's (tap, cg, ks) in the kconv_w image."""
    return (tap * (c // 32) + cg) * (c // 16) + ks


def group_proj_tuned(part: int, tile: int, ks: int, ntiles: int) -> int:
    """Group of k step ks of a tile of pack_satu_tuned's proj_w image: part 0 = Wa (lanes_acc), 1 = Wb, 2 = the C-stack (lanes_a; tile 0);
    ntiles 32-row tiles per projection (2: "plain", 1: "p27" / "q")."""
    return ((part * ntiles + tile) if part < 2 else 2 * ntiles) * 4 + ks


def group_wbe(tile: int, ks: int) -> int:
    """Group of k step ks (k = 8 n + j) of lanes_wbe's tile in the wbe_w image."""
    return 2 * tile + ks


def bias_acc_order(b: np.ndarray) -> np.ndarray:
    """A bias of 32 T rows in accumulator-register order: [2 half][16 t + r] = b[32 t + acc_row(r, half)], r < 16."""
    half, t, r = np.arange(2)[:, None, None], np.arange(len(b) // 32)[:, None], np.arange(16)
    return b[32 * t + acc_row(r, half)].reshape(2, -1)


# ----------------------------------------------------------------------------- SATU host packers: state_dict -> {name: host tensor}
def _f32(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _img(*parts: np.ndarray) -> torch.Tensor:
    """The split-bf16 image of the parts, each rounded to fp32, one after the other."""
    return split_bf16_image(torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in parts])))


def pack_satu_heads(sd) -> Dict[str, torch.Tensor]:
    """The coordinate MLP (body, routing / offset / st_offset heads, savsr_arch.py:242-257): 64 hidden units at every num_feat."""
    p = "upsample."
    head_w = torch.cat([sd[p + "routing.0.weight"], sd[p + "offset.weight"], sd[p + "st_offset.weight"]], 0)
    head_b = torch.cat([sd[p + "routing.0.bias"], sd[p + "offset.bias"], sd[p + "st_offset.bias"]], 0)
    return dict(body0_w=sd[p + "body.0.weight"].reshape(64, 4), body0_b=sd[p + "body.0.bias"],
                body2_w=sd[p + "body.2.weight"].reshape(64, 64).t(), body2_b=sd[p + "body.2.bias"],
                head_w=head_w.reshape(8, 64), head_b=head_b)


def _pack_kconv(m: Dict[str, np.ndarray], c: int) -> Dict[str, torch.Tensor]:
    return dict(kconv_w=_img(lanes_kconv(m["kconv"], c)), kconv_b=_f32(m["kconv_b"].reshape(c, 25).T))      # bias [tap][ch]


def pack_satu_nf(sd, c: int) -> Dict[str, torch.Tensor]:
    """savsr_satu_nf_weights (num_feat = c): fold_satu_nf's products rounded to fp32, the LR-side matrices then split to (hi, lo) bf16
    pairs in lane order; wbe and fb stay fp32.  proj_w = Wt27 Wa in accumulator order, then the x side as A-operand tiles: tile 0 =
    Wt27 Wb, tiles 1 .. = the C-stack, zero-padded to whole 32-row tiles."""
    m = fold_satu_nf(sd, c)
    xm = np.zeros((32 + (c // 2 + 31) // 32 * 32, c), dtype=np.float64)
    xm[:32], xm[32:32 + c // 2] = m["tb"], m["cstack"]
    return dict(**_pack_kconv(m, c), proj_w=_img(lanes_acc(m["ta"]), *(lanes_a(xm, r) for r in range(0, len(xm), 32))),
                wbe=_f32(m["wbe"]), fusion_b=_f32(m["fb"]))


def pack_satu_tuned(sd, form: str) -> Dict[str, torch.Tensor]:
    """savsr_satu_weights of a tuned 64-wide form (3 channels): "plain" (savsr_satu_lr_stage / _hr_upsample: Wa | Wb | C-stack, Wb E_n and
    b un-projected, two 32-row tiles each, plus the kernel_conv images every form shares), "p27" (savsr_satu_*_tail) or "q"
    (savsr_satu_hr_tail_q, rows by row_q): proj_w = (Wt Wa | Wt Wb | C-stack), wbe_w = (Wt Wb E_n) as MFMA tiles, fusion_b = Wt b."""
    m = fold_satu_nf(sd, 64, row_q if form == "q" else None, tail=form != "plain")
    tiles = range(0, len(m["fb"]), 32)
    wbe = m["wbe"].transpose(0, 2, 1)                                                 # [n][p][j]
    t = dict(proj_w=_img(*(lanes_acc(m["ta"], r) for r in tiles), *(lanes_a(m["tb"], r) for r in tiles), lanes_a(m["cstack"])),
             wbe_w=_img(*(lanes_wbe(wbe, r) for r in tiles)), fusion_b=_f32(bias_acc_order(m["fb"])))
    return dict(**_pack_kconv(m, 64), **t) if form == "plain" else t


def struct_of(cls, *tensors: Dict[str, torch.Tensor], rename: Optional[Dict[str, str]] = None, **fields):
    """A ctypes struct of device pointers: field rename.get(k, k) = the address of tensors[..][k]; later dicts win.  The struct holds raw
    addresses: the caller keeps the tensors referenced."""
    w = cls(**fields)
    for d in tensors:
        for k, v in d.items():
            setattr(w, (rename or {}).get(k, k), v.data_ptr())
    return w


def fuse_window_conv(sd, d: str, nch: int, sw: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv_c (nch -> nf) and conv_sup (nch (sw - 1) -> nf) of one direction fused into one RW -> 2 nf conv over the packed window
    tensor (channels: frame t | the support frames in sup_index order | zeros; RW = window_record), savsr_arch.py:429-431,456-457.
    (nch = 3, sw = 3: the 16 -> 128 conv over frame t | t-1 | t+1 | zeros.)"""
    wc, bc = sd[d + ".conv_c.weight"].cpu().float(), sd[d + ".conv_c.bias"].cpu().float()
    ws, bs = sd[d + ".conv_sup.weight"].cpu().float(), sd[d + ".conv_sup.bias"].cpu().float()
    nf = wc.shape[0]
    w = torch.zeros(2 * nf, window_record(nch, sw), 3, 3)
    w[:nf, 0:nch] = wc
    w[nf:, nch:nch * sw] = ws
    return w, torch.cat([bc, bs])


class WeightPacking:
    """Mixin of HipEngine: state_dict -> device-resident kernel operands (`pw`, `pw_wy`, `osc`, `se`, `satu_*`, `tail_*`)."""

    def _dev(self, t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        d = t.to(self.dev, dtype).contiguous()
        self._keep.append(d)
        return d

    def _fold(self, sd, key: str, bn: Optional[str]):
        w = sd[key + ".weight"].to("cpu", torch.float32)
        b = sd.get(key + ".bias")
        b = None if b is None else b.to("cpu", torch.float32)
        if bn is not None:      # eval BatchNorm folded into the conv (savsr_arch.py:191,196,199,204)
            s = sd[bn + ".weight"].cpu() / torch.sqrt(sd[bn + ".running_var"].cpu() + BN_EPS)
            w = w * s.view(-1, 1, 1, 1)
            b0 = b if b is not None else torch.zeros_like(s)
            b = (b0 - sd[bn + ".running_mean"].cpu()) * s + sd[bn + ".bias"].cpu()
        return w, b

    def _register(self, key: str, w: torch.Tensor, b: Optional[torch.Tensor]):
        cout, cin, ks, _ = w.shape
        bias = None if b is None else self._dev(b)
        wd = w.to(self.dev)                                  # (the images are built on the device: _scatter_image)
        self.pw[key] = (self._dev(pack_conv_weight(wd, self.dev), torch.int16), bias, cout, cin, ks)
        if self.conv_wy and ks == 3 and cout % 64 == 0 and cin % 16 == 0:
            # static 3x3 weights also as the Winograd F(2,3)-along-y image (conv_wy.hip: 2/3 of the matrix work); which form a launch takes is
            # decided per launch in conv_launch (the 16-row Winograd tiles need a launch that fills the chip)
            self.pw_wy[key] = self._dev(pack_conv_weight_wy(wd, self.dev), torch.int16)

    def _add_conv(self, sd, key: str, bn: Optional[str] = None):
        self._conv_src[key] = ("conv", key, bn)
        self._register(key, *self._fold(sd, key, bn))

    def _padded(self, sd, key: str, bn: Optional[str], cin_p: int, cout_p: int):
        w, b = self._fold(sd, key, bn)
        cout, cin, ks, _ = w.shape
        wp = torch.zeros(cout_p, cin_p, ks, ks)
        wp[:cout, :cin] = w
        bp = None
        if b is not None:
            bp = torch.zeros(cout_p)
            bp[:cout] = b
        return wp, bp

    def _add_conv_padded(self, sd, key: str, bn: Optional[str], cin_p: int, cout_p: int):
        """A conv with zero input / output channels appended up to (cin_p, cout_p): the conv kernels take multiples of 16 input channels.
        An appended output channel is 0 (zero weights, zero bias; ReLU(0) = 0) and an appended input channel meets zero weights."""
        self._conv_src[key] = ("padded", key, bn, cin_p, cout_p)
        self._register(key, *self._padded(sd, key, bn, cin_p, cout_p))

    def _add_window_conv(self, sd, d: str):
        self._conv_src[d + ".win"] = ("win", d)
        self._register(d + ".win", *fuse_window_conv(sd, d, self.cfg["num_in_ch"], self.cfg["slid_win"]))

    def _conv_weight(self, src: tuple) -> torch.Tensor:
        """The fp32 weight [cout, cin, k, k] a static conv was registered with, derived again from the state_dict (no copy is kept)."""
        sd = self._sd_ref
        if src[0] == "conv":
            return self._fold(sd, src[1], src[2])[0]
        if src[0] == "padded":
            return self._padded(sd, *src[1:])[0]
        return fuse_window_conv(sd, src[1], self.cfg["num_in_ch"], self.cfg["slid_win"])[0]

    def _build_f16(self) -> None:
        """The fp16 weight images of the static convs (precision "fp16"), built once, on the first fp16 forward: fp16(W) and, where the
        Winograd-y image exists, fp16(U) with U in float64 -- both rounded once.  Refuses any operand beyond +-65504, naming its conv;
        an OSConv's dynamic weights are gated averages of its bank (every gate in (0, 1), the kernel weights a softmax): |W''| <= max |bank|,
        |U| <= 1.5 max |bank|."""
        if self.pw16:
            return
        imgs, imgs_wy = {}, {}
        for key, src in self._conv_src.items():
            w = self._conv_weight(src)
            check_f16_range(f"conv {key!r}", w.numpy())
            imgs[key] = pack_conv_weight_f16(w)
            if key in self.pw_wy:
                u = wy_transform_f64(w)
                check_f16_range(f"conv {key!r} (Winograd-y transform)", u)
                imgs_wy[key] = _f16_image(*conv_wy_pack_index(w.shape[0], w.shape[1]), u)
        for key in self.osc:
            bank = self._sd_ref[key + ".weight"].detach().to("cpu", torch.float64).numpy()
            check_f16_range(f"OSConv {key!r}", bank * (1.5 if self.osc[key]["cout"] % 64 == 0 else 1.0))
        for key, img in imgs.items():
            self.pw16[key] = self._dev(img, torch.int16)
        for key, img in imgs_wy.items():
            self.pw16_wy[key] = self._dev(img, torch.int16)

    def _add_osconv(self, sd, key: str):
        bank = sd[key + ".weight"].to(self.dev, torch.float32)    # [K, cout, cin, 3, 3]
        knum, cout, cin = bank.shape[:3]
        packed = torch.stack([pack_conv_part(bank[k], self.dev) for k in range(knum)], 0)
        a = key + ".attention"
        bn_s = sd[a + ".bn.weight"].cpu() / torch.sqrt(sd[a + ".bn.running_var"].cpu() + BN_EPS)
        bn_b = sd[a + ".bn.bias"].cpu() - sd[a + ".bn.running_mean"].cpu() * bn_s
        hidden = sd[a + ".fc.weight"].shape[0]
        g = lambda k: self._dev(sd[k].reshape(sd[k].shape[0], -1) if sd[k].dim() > 1 else sd[k])
        elems = packed.shape[1]
        ent = dict(cin=cin, cout=cout, knum=knum, hidden=hidden, bank=self._dev(packed), nunits=elems // 8,
                   l1_w=g(key + ".scale_routing.0.weight"), l1_b=g(key + ".scale_routing.0.bias"),
                   l2_w=g(key + ".scale_routing.2.weight"), l2_b=g(key + ".scale_routing.2.bias"),
                   fc_w=g(a + ".fc.weight"), bn_scale=self._dev(bn_s), bn_shift=self._dev(bn_b),
                   ch_w=g(a + ".channel_fc.weight"), ch_b=g(a + ".channel_fc.bias"),
                   fl_w=g(a + ".filter_fc.weight"), fl_b=g(a + ".filter_fc.bias"),
                   sp_w=g(a + ".spatial_fc.weight"), sp_b=g(a + ".spatial_fc.bias"),
                   kn_w=g(a + ".kernel_fc.weight"), kn_b=g(a + ".kernel_fc.bias"),
                   **self._osc_scratch(cin, cout, knum, elems))
        self.osc[key] = ent

    def _osc_scratch(self, cin: int, cout: int, knum: int, elems: int) -> dict:
        """Per-engine scratch of one OSConv (routing vectors, gates, the generated weight images), NB_MAX copies: one per clip of a batched
        launch sequence (the tensors handed around are clip 0's; `_bstride` knows the distance to the next)."""
        nb = self.NB_MAX
        al = lambda n, unit: ((n * unit + 255) // 256) * 256 // unit          # copies stay 256-byte aligned
        out = {}
        for name, n, dt in (("v1", 2 * cin, torch.float32), ("v2", cin, torch.float32), ("att", cin + cout + 9 + knum, torch.float32),
                            ("wdyn", 2 * elems, torch.int16), ("wdyn_wy", 2 * (elems * 4 // 3) if cout % 64 == 0 else 0, torch.int16)):      # (12 taps instead of 9)
            unit = 4 if dt == torch.float32 else 2
            pitch = al(n, unit)
            full = torch.empty(nb * pitch, device=self.dev, dtype=dt)
            self._keep.append(full)
            t = full[:n]
            self._bstride[t.data_ptr()] = pitch * unit
            out[name] = t
        return out

    def _add_rcab_fold(self, sd, r: str):
        """What savsr_rcab_gate_weights_batch reads for one RCAB (`rcab_w`): the fp32 master parts of conv `.2` in the element order of the
        direct and -- where the Winograd-y image exists -- the Winograd-y image, its bias, and the gate's layers (rcab_fold_tables)."""
        w, b = self._fold(sd, r + ".2", None)
        w1, b1, w2, b2, cm = self.se[r]
        a, cz = rcab_fold_tables(w, b, sd[r + ".3.attention.1.weight"], sd[r + ".3.attention.1.bias"])
        wd = w.to(self.dev)
        self.rcab_w[r] = dict(a=self._dev(a), cz=self._dev(cz), w2=w2, b2=b2, cm=cm, bias=self.pw[r + ".2"][1], master=self._dev(pack_conv_part(wd, self.dev)),
                            master_wy=self._dev(pack_conv_part_wy(wd, self.dev)) if (r + ".2") in self.pw_wy else None)

    def _rcab_scratch(self) -> dict:
        """Per-engine scratch of the folded RCABs, reused by every RCAB of the stream (each conv.2 has read its image before the next gate
        launch overwrites it: stream order): the generated image (the larger, Winograd-y, size where that form exists), g b and g, NB_MAX
        copies each -- one per clip of a batched launch sequence, as _osc_scratch."""
        c, nb = self.nf, self.NB_MAX
        elems = conv_pack_index(c, c, 3)[1]
        if c % 64 == 0:
            elems = max(elems, conv_wy_pack_index(c, c)[1])
        out = {}
        for name, n, dt in (("wimg", 2 * elems, torch.int16), ("bias", c, torch.float32), ("gate", c, torch.float32)):
            unit = 4 if dt == torch.float32 else 2
            pitch = ((n * unit + 255) // 256) * 256 // unit          # copies stay 256-byte aligned
            full = torch.empty(nb * pitch, device=self.dev, dtype=dt)
            self._keep.append(full)
            t = full[:n]
            self._bstride[t.data_ptr()] = pitch * unit
            out[name] = t
        return out

    def _upload(self, host: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return {k: self._dev(v, torch.int16 if v.dtype == torch.int16 else torch.float32) for k, v in host.items()}

    def _pack_satu_nf(self, sd, c: int):
        """The width-generic SATU (savsr_satu_nf_*, num_feat = c)."""
        self.satu_nf_t = self._upload(pack_satu_nf(sd, c))
        self.satu_nf_w = struct_of(SatuNfWeights, self.satu_nf_t, C=c)

    def _pack_satu(self, sd):
        """Every SATU operand of this engine's form.  The *_t dicts keep the tensors the structs point at."""
        c = self.nf
        heads = self._upload(pack_satu_heads(sd))
        self.tail_w = self._dev(sd["tail.weight"].reshape(-1, c * 9))
        self.tail_b = self._dev(sd["tail.bias"])
        if c != 64 or self.cfg["num_in_ch"] != 3:
            # the width-generic SATU (num_feat 32, or any num_in_ch != 3: Wt with 9 num_in_ch live rows); the phase table's weights
            # (savsr_satu_phase_table reads the body / head pointers only) travel in a savsr_satu_weights whose other pointers name the
            # generic form's tensors
            self._pack_satu_nf(sd, c)
            self.satu_t = heads
            self.satu_w = struct_of(SatuWeights, heads, self.satu_nf_t, rename={"wbe": "wbe_w"})
            self.satu_tail_t, self.satu_w_tail, self.satu_tailq_t, self.satu_w_tailq = None, None, None, None      # (the tuned 64-wide forms)
            return
        self.satu_nf_t, self.satu_nf_w = None, None
        self.satu_t = {**heads, **self._upload(pack_satu_tuned(sd, "plain"))}
        self.satu_w = struct_of(SatuWeights, self.satu_t)
        # the tail-projected forms (include/savsr_hip.h, savsr_satu_*_tail): heads and kernel_conv of the plain form, the rest projected
        self.satu_tail_t, self.satu_tailq_t = self._upload(pack_satu_tuned(sd, "p27")), self._upload(pack_satu_tuned(sd, "q"))
        self.satu_w_tail = struct_of(SatuWeights, self.satu_t, self.satu_tail_t)
        self.satu_w_tailq = struct_of(SatuWeights, self.satu_t, self.satu_tailq_t)

    def _pack_all(self, sd):
        cfg = self.cfg
        self._sd_ref = sd          # (the module's own tensors: the lazily built fp16 images are derived from them, _build_f16)
        for d in ("f2p_win", "p2f_win"):
            self._add_window_conv(sd, d)
            for k in range(cfg["w1_num_block"]):
                b = f"{d}.blocks.{k}"
                for i in range(3):
                    self._add_conv(sd, f"{b}.conv0.{i}")
                    self._add_conv(sd, f"{b}.conv2.{i}")
                if k >= 1:
                    self._add_osconv(sd, b + ".osconv")
                else:
                    self._add_conv(sd, b + ".conv1")
            self._add_conv(sd, d + ".merge")
        from .archs.savsr_arch import frame_sample_indices, iteration_window
        center = cfg["num_frame"] // 2 if cfg["center_frame_idx"] is None else cfg["center_frame_idx"]
        self.iter_win = iteration_window(cfg["num_frame"], cfg["interval"], center)      # frames per propagation direction (:597-604)
        self.fwd_idx, self.bwd_idx = frame_sample_indices(cfg["num_frame"], cfg["interval"])   # frame_sample (:638-659)
        if cfg["interval"] != 0 and (len(self.fwd_idx) < self.iter_win or len(self.bwd_idx) < self.iter_win):
            raise ValueError("num_frame / interval: the sampled frame lists are shorter than the iteration window")
        steps = self.iter_win - cfg["slid_win"] + 1
        self.n_l2 = (self.iter_win - cfg["fusion_win"] + 1) // 2
        for i in range(self.n_l2):
            u = f"h_win.{i}"
            for j in range(steps - 2 * i):
                self._add_conv(sd, f"{u}.conv_h.{j}")
            for k in range(cfg["w2_num_block"]):
                b = f"{u}.blocks.{k}"
                for j in range(cfg["fusion_win"]):
                    self._add_conv(sd, f"{b}.conv0.{j}")
                    self._add_conv(sd, f"{b}.conv2.{j}")
                self._add_osconv(sd, b + ".osconv")
            self._add_conv(sd, u + ".merge")
        self._add_conv(sd, "h_win_conv_h")
        for g in range(cfg["n_resgroups"]):
            for k in range(cfg["n_resblocks"]):
                r = f"RG.{g}.residual_group.{k}.rcab"
                self._add_conv(sd, r + ".0")
                self._add_conv(sd, r + ".2")
                a = r + ".3.attention"
                cm = sd[a + ".1.weight"].shape[0]
                self.se[r] = (self._dev(sd[a + ".1.weight"].reshape(cm, -1)), self._dev(sd[a + ".1.bias"]),
                              self._dev(sd[a + ".3.weight"].reshape(-1, cm)), self._dev(sd[a + ".3.bias"]), cm)
                self._add_rcab_fold(sd, r)
            self._add_conv(sd, f"RG.{g}.conv")
            m = f"adapt.{g}.mask"
            q = sd[m + ".0.weight"].shape[0]                                         # num_feat / 4 (:189-204)
            if q % 16 == 0:
                self._add_conv(sd, m + ".0", bn=m + ".1")
                self._add_conv(sd, m + ".4", bn=m + ".5")
                self._add_conv(sd, m + ".7", bn=m + ".8")
                self._add_conv(sd, m + ".11", bn=m + ".12")
            else:                   # (num_feat = 32: 8 mask channels, carried as 16 -- osadapt takes the width from the packed conv)
                qp = (q + 15) // 16 * 16
                self._add_conv_padded(sd, m + ".0", m + ".1", self.nf, qp)
                self._add_conv_padded(sd, m + ".4", m + ".5", qp, qp)
                self._add_conv_padded(sd, m + ".7", m + ".8", qp, qp)
                self._add_conv_padded(sd, m + ".11", m + ".12", qp, 1)
            self._add_osconv(sd, f"adapt.{g}.adapt")
        self._add_conv(sd, "conv_last")
        self.gamma = float(sd["gamma"].reshape(-1)[0])
        self._pack_satu(sd)
        self.se_gate = torch.empty(self.nf, device=self.dev)
        self.rcab_scr = self._rcab_scratch()
