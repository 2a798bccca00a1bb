"""MI355X-native SAVSR behind the reference's ARCH_REGISTRY / forward() surface.

Drop-in for the class registered as `SAVSR` at /root/reference/lbasicsr/archs/savsr_arch.py:574:
same constructor kwargs (:576-589, `network_g` of options/test/SAVSR/*.yml), `.set_scale()`
(:635-636), `__call__(lq[b,t,3,h,w]) -> [b,3,H,W]`, and a parameter tree whose 791
state_dict keys/shapes equal the reference's, so `savsr_best.pth` loads with strict=True.

What differs is everything below that surface.  The modules here only HOLD parameters (they
are the checkpoint schema); no torch operator of theirs ever runs.  `forward()` hands the
clip to `savsr_amd.engine.HipEngine`, which re-lays the weights out once and then drives the
hand-written gfx950 kernels of libsavsr_hip.so.  On a machine without that library, or with
the module on a CPU device, `forward()` raises -- there is no eager fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn

from ..registry import ARCH_REGISTRY


class _Holder(nn.Module):
    """A parameter container; calling it is a bug (the HIP engine does the arithmetic)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(f"{type(self).__name__} holds parameters only; run SAVSR.forward()")


def _seq(mods):
    return nn.Sequential(*mods)


class ScaleAttention(_Holder):
    """Parameters of the reference's ScaleAttention (savsr_arch.py:16-60)."""

    def __init__(self, cin, cout, ksize=3, knum=8, reduction=0.0625, min_channel=16):
        super().__init__()
        hidden = max(int(cin * reduction), min_channel)
        self.fc = nn.Conv2d(cin, hidden, 1, bias=False)
        self.bn = nn.BatchNorm2d(hidden)
        self.channel_fc = nn.Conv2d(hidden, cin, 1)
        self.filter_fc = nn.Conv2d(hidden, cout, 1)
        self.spatial_fc = nn.Conv2d(hidden, ksize * ksize, 1)
        self.kernel_fc = nn.Conv2d(hidden, knum, 1)
        for m in (self.fc, self.channel_fc, self.filter_fc, self.spatial_fc, self.kernel_fc):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            if m.bias is not None:
                nn.init.zeros_(m.bias)


class OSConv2d(_Holder):
    """Kernel bank + attention + scale routing of OSConv (savsr_arch.py:99-134)."""

    def __init__(self, cin, cout, ksize=3, knum=8):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(knum, cout, cin, ksize, ksize))
        for k in range(knum):
            nn.init.kaiming_normal_(self.weight.data[k], mode="fan_out", nonlinearity="relu")
        self.attention = ScaleAttention(cin, cout, ksize, knum)
        self.scale_routing = _seq([nn.Linear(cin + 2, cin * 2), nn.ReLU(True), nn.Linear(cin * 2, cin), nn.ReLU(True)])


class OSAdapt(_Holder):
    """savsr_arch.py:186-208: mask branch (indices match the reference Sequential) + OSConv."""

    def __init__(self, ch, ratio=4):
        super().__init__()
        q = ch // ratio
        self.mask = _seq([
            nn.Conv2d(ch, q, 3, 1, 1), nn.BatchNorm2d(q), nn.ReLU(True), nn.AvgPool2d(2),
            nn.Conv2d(q, q, 3, 1, 1), nn.BatchNorm2d(q), nn.ReLU(True),
            nn.Conv2d(q, q, 3, 1, 1), nn.BatchNorm2d(q), nn.ReLU(True),
            nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False),
            nn.Conv2d(q, 1, 3, 1, 1), nn.BatchNorm2d(1), nn.Sigmoid()])
        self.adapt = OSConv2d(ch, ch)


class STAUpsample(_Holder):
    """savsr_arch.py:217-260."""

    def __init__(self, ch, num_experts=4, st_ksize=5):
        super().__init__()
        def expert(o, i):
            w = torch.empty(num_experts, o, i, 1, 1)
            for n in range(num_experts):
                nn.init.kaiming_uniform_(w[n], a=math.sqrt(5))
            return nn.Parameter(w)
        self.weight_compress = expert(ch // 8, ch)
        self.weight_expand = expert(ch, ch // 8)
        self.kernel_conv = _seq([nn.Conv2d(ch, ch * st_ksize ** 2, 1), nn.LeakyReLU(0.1, True)])
        self.body = _seq([nn.Conv2d(4, 64, 1), nn.ReLU(True), nn.Conv2d(64, 64, 1), nn.ReLU(True)])
        self.routing = _seq([nn.Conv2d(64, num_experts, 1), nn.Sigmoid()])
        self.offset = nn.Conv2d(64, 2, 1)
        self.st_offset = nn.Conv2d(64, 2, 1)
        self.fusion = nn.Conv2d(2 * ch, ch, 1)


class ResidualBlock(_Holder):
    """savsr_arch.py:379-397."""

    def __init__(self, nf, nfr, use_osconv):
        super().__init__()
        self.conv0 = _seq([nn.Conv2d(nf, nf, 3, 1, 1) for _ in range(nfr)])
        if use_osconv:
            self.osconv = OSConv2d(nf * nfr, nf)
        else:
            self.conv1 = nn.Conv2d(nf * nfr, nf, 1)
        self.conv2 = _seq([nn.Conv2d(2 * nf, nf, 3, 1, 1) for _ in range(nfr)])


class WindowUnit_l1(_Holder):
    """savsr_arch.py:418-442."""

    def __init__(self, cin, nf, win, nblock):
        super().__init__()
        self.conv_c = nn.Conv2d(cin, nf, 3, 1, 1)
        self.conv_sup = nn.Conv2d(cin * (win - 1), nf, 3, 1, 1)
        self.blocks = _seq([ResidualBlock(nf, 3, use_osconv=(i >= 1)) for i in range(nblock)])
        self.merge = nn.Conv2d(3 * nf, nf, 3, 1, 1)


class WindowUnit_l2(_Holder):
    """savsr_arch.py:467-483."""

    def __init__(self, nf, win, slid, nblock):
        super().__init__()
        self.conv_h = _seq([nn.Conv2d(2 * nf, nf, 3, 1, 1) for _ in range(win)])
        self.blocks = _seq([ResidualBlock(nf, slid, True) for _ in range(nblock)])
        self.merge = nn.Conv2d(slid * nf, 2 * nf, 3, 1, 1)


class ChannelAttention(_Holder):
    def __init__(self, nf, squeeze=16):
        super().__init__()
        self.attention = _seq([nn.AdaptiveAvgPool2d(1), nn.Conv2d(nf, nf // squeeze, 1), nn.ReLU(True),
                               nn.Conv2d(nf // squeeze, nf, 1), nn.Sigmoid()])


class RCAB(_Holder):
    def __init__(self, nf, squeeze=16):
        super().__init__()
        self.rcab = _seq([nn.Conv2d(nf, nf, 3, 1, 1), nn.ReLU(True), nn.Conv2d(nf, nf, 3, 1, 1), ChannelAttention(nf, squeeze)])


class ResidualGroup(_Holder):
    def __init__(self, nf, nblock, squeeze=16):
        super().__init__()
        self.residual_group = _seq([RCAB(nf, squeeze) for _ in range(nblock)])
        self.conv = nn.Conv2d(nf, nf, 3, 1, 1)


def iteration_window(num_frame: int, interval: int, center_frame_idx: int) -> int:
    """Frames each propagation direction iterates over (savsr_arch.py:597-604): all of them without frame sampling,
    center + 1 / + 2 (even / odd centre index) with it."""
    if interval == 0:
        return num_frame
    return center_frame_idx + 1 if center_frame_idx % 2 == 0 else center_frame_idx + 2


def frame_sample_indices(num_frame: int, interval: int):
    """SAVSR.frame_sample (savsr_arch.py:638-659) as index lists: (past -> future frames, future -> past frames).  Both hold
    the centre frame (num_frame // 2: the method computes its own, whatever center_frame_idx the module was given)."""
    index = list(range(num_frame))
    if interval == 0:
        return index, index
    c = num_frame // 2
    if c % 2 == 0:
        fwd = index[1::interval + 1]
        fwd.insert(c // 2, c)
        bwd = index[::interval + 1]
    else:
        fwd = index[::interval + 1]
        fwd.insert(c // 2 + 1, c)
        bwd = index[1::interval + 1]
        if len(fwd) != len(bwd):
            bwd.append(fwd[-1])
            bwd.insert(0, fwd[0])
    return fwd, bwd


@ARCH_REGISTRY.register()
class SAVSR(nn.Module):
    def __init__(self, num_in_ch=3, num_feat=64, num_frame=7, slid_win=3, fusion_win=5, interval=0, w1_num_block=4,
                 w2_num_block=2, n_resgroups=4, n_resblocks=8, downsample_scale=2, center_frame_idx=None):
        super().__init__()
        self.cfg = dict(num_in_ch=num_in_ch, num_feat=num_feat, num_frame=num_frame, slid_win=slid_win,
                        fusion_win=fusion_win, interval=interval, w1_num_block=w1_num_block, w2_num_block=w2_num_block,
                        n_resgroups=n_resgroups, n_resblocks=n_resblocks, downsample_scale=downsample_scale,
                        center_frame_idx=center_frame_idx)
        self.scale: Tuple[float, float] = (4, 4)
        self.center_frame_idx = num_frame // 2 if center_frame_idx is None else center_frame_idx
        self.num_frame, self.num_feat = num_frame, num_feat
        iter_win = iteration_window(num_frame, interval, self.center_frame_idx)
        self.iter_win, self.interval = iter_win, interval
        if iter_win < slid_win:
            raise ValueError("num_frame / interval leave fewer frames than the sliding window")
        if (iter_win - fusion_win + 1) // 2 > 1:
            # two pyramid levels: the reference constructs them (:616-618) but its forward fails (WindowUnit_l2 :488 reads
            # win_size inputs, the level above returns win_size - fusion_win + 1) -- nothing to be a drop-in for
            raise ValueError("more than one pyramid level (num_frame - fusion_win + 1 >= 4 without frame sampling): "
                             "the reference's own forward raises an IndexError for this configuration")
        self.f2p_win = WindowUnit_l1(num_in_ch, num_feat, slid_win, w1_num_block)
        self.p2f_win = WindowUnit_l1(num_in_ch, num_feat, slid_win, w1_num_block)
        self.h_win = _seq([WindowUnit_l2(num_feat, (iter_win - slid_win + 1) - 2 * i, fusion_win, w2_num_block)
                           for i in range((iter_win - fusion_win + 1) // 2)])
        self.h_win_act = nn.LeakyReLU(0.2, True)
        self.h_win_conv_h = nn.Conv2d(2 * num_feat, num_feat, 3, 1, 1)
        self.RG = nn.ModuleList([ResidualGroup(num_feat, n_resblocks) for _ in range(n_resgroups)])
        self.adapt = nn.ModuleList([OSAdapt(num_feat) for _ in range(n_resgroups)])
        self.gamma = nn.Parameter(torch.ones(1))
        self.conv_last = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.upsample = STAUpsample(num_feat)
        self.tail = nn.Conv2d(num_feat, num_in_ch, 3, 1, 1)
        self._engine = None
        self._engine_sig = None
        self._sig_tensors = None
        self.precision = "fp32"
        self.self_ensemble = False

    PRECISIONS = ("fp32", "fp16")

    def set_precision(self, precision: str):
        """Operand precision of the convs: "fp32" (default: split-bf16 products, fp32-equivalent) or "fp16" (operands of every static,
        OSConv, OSAdapt-mask, pyramid and trunk conv rounded to fp16, one fp16 MFMA per product, fp32 accumulation; SATU, tail, gates
        and pools unchanged).  Module state like set_scale: not in state_dict(), kept across load_state_dict / .to()."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {self.PRECISIONS}, got {precision!r}")
        self.precision = precision

    def set_self_ensemble(self, on: bool = True):
        """Geometric self-ensemble ("+" results, EDSR+ / RCAN+): every clip runs in its 8 flip / transpose variants -- a transposed one at the
        swapped scale (sw, sh) -- and the output is the mean of the 8 inverse-transformed outputs.  Off by default;
        covers forward, forward_many, upscale_video and VideoUpscaler, and composes with set_precision.  Module state like set_precision: not
        in state_dict(), kept across load_state_dict / .to()."""
        self.self_ensemble = bool(on)

    def set_scale(self, scale: Union[tuple, float, int]):
        """savsr_arch.py:635-636; a bare number means a symmetric scale."""
        if isinstance(scale, (int, float)):
            scale = (scale, scale)
        self.scale = tuple(scale)

    # ---- engine management ---------------------------------------------------------------
    def _apply(self, fn, *a, **k):          # .to() / .cuda() / .float() move the parameters
        self._engine = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)

    def _signature(self):
        if self._engine is None or self._sig_tensors is None:
            self._sig_tensors = list(self.state_dict(keep_vars=True).values())
        return (str(self.gamma.device), sum(t._version for t in self._sig_tensors), self._sig_tensors[0].data_ptr())

    def engine(self):
        """The HipEngine for the current parameters (rebuilt when they move or change in place)."""
        sig = self._signature()
        if self._engine is None or sig != self._engine_sig:
            from ..engine import HipEngine
            self._engine = HipEngine(self.state_dict(), self.cfg, self.gamma.device)
            self._sig_tensors = list(self.state_dict(keep_vars=True).values())
            self._engine_sig = self._signature()
        self._engine.set_precision(self.precision)
        return self._engine

    def forward_many(self, clips, scales):
        """Extension for mixed-scale streams (BASELINE config 5; the reference's flow would call set_scale + forward per clip):
        clips[i]: [t, c, h, w] on the GPU, scales[i]: (sh, sw) -> list of [c, H, W]; independent clips overlap on HIP streams."""
        if self.training:
            raise RuntimeError("savsr_amd.SAVSR implements the inference path only; call .eval() first")
        with torch.no_grad():
            return self.engine().forward_many(list(zip(clips, [tuple(s) if not isinstance(s, (int, float)) else (s, s) for s in scales])),
                                              ensemble=self.self_ensemble)

    def upscale_video(self, frames: torch.Tensor, scale=None, padding: str = "reflection", out: str = "float", pixel_format: str = "rgb",
                      size=None, cuts=None, scene_threshold=10.0, colour: str = "bt601", out_colour: Optional[str] = None, depth: int = 8,
                      out_depth: Optional[int] = None, siting: Optional[str] = None, out_siting: Optional[str] = None,
                      chroma_filter: Optional[str] = None, crop=None, crop_limit=24, bars: str = "keep", fields: Optional[str] = None,
                      pulldown: Optional[str] = None, pulldown_cycle: int = 5, *, surface=None, out_surface=None,
                      scan: Optional[str] = None, dither: Optional[str] = None, deinterlacer: str = "yadif",
                      field_rate: str = "double", combed: Optional[str] = None, comb_threshold: int = 9, comb_pixels: int = 40,
                      denoise: Optional[str] = None, denoise_radius: int = 4, denoise_strength=(4, 9),
                      denoise_chroma_strength=None, spatial_denoise: Optional[str] = None, spatial_patch: int = 3, spatial_search: int = 7,
                      spatial_strength=3.0, spatial_chroma_strength=None, deblock: Optional[str] = None, deblock_block: int = 8,
                      deblock_strength=(25, 13), deblock_chroma_strength=None, deblock_origin=(0, 0), deblock_chroma_origin=None,
                      deblock_grid: Optional[str] = None, dering: Optional[str] = None, dering_strength=(4, 2),
                      dering_chroma_strength=None, dering_damping: int = 5) -> torch.Tensor:
        """A whole LR video -> its SR video.  frames: [N, c, h, w] float on the GPU, or [N, h, w, c] uint8 on the GPU or the host
        (c = num_in_ch).  Frame i is SAVSR.forward on its num_frame window by generate_frame_indices with `padding` (replicate,
        reflection, reflection_circle, circle; lbasicsr/data/data_util.py:63-112).  scale: a number or (sh, sw), default set_scale's.
        Returns [N, c, H, W] fp32, or with out="uint8" [N, H, W, c] uint8 = tensor2img(frame, rgb2bgr=False) of each fp32 frame.
        pixel_format="i420", size=(h, w): frames are [N, i420_bytes(h, w)] uint8 (GPU or host), planar YUV 4:2:0 as in a Y4M file
        (savsr_amd/yuv.py: BT.601 limited range, the reference's rgb2ycbcr / ycbcr2rgb), converted to fp32 RGB on the GPU without an
        8-bit rounding; num_in_ch = 3.  out="i420", with either input format: [N, i420_bytes(H, W)] uint8, the fp32 frames converted and
        rounded once, in YUV.
        colour: the colour space of I420 input, one of savsr_amd.yuv.COLOURS: "bt601" (the default: BT.601 limited range), "bt709"
        (limited range; what players take untagged HD video for), "bt601-full", "bt709-full" (full range, Y4M's XCOLORRANGE=FULL).
        out_colour: that of I420 output; None = the same as colour.  The two sides are independent (the network works in RGB), so
        colour="bt601", out_colour="bt709" also converts an SD source into what an HD player expects.  colour goes with
        pixel_format="i420" and out_colour with out="i420".
        depth: the bit depth of I420 input, 8, 10 or 12.  10 and 12: frames are [N, 2 * i420_bytes(h, w)] uint8, every sample a
        little-endian 16-bit word (Y4M's C420p10 / C420p12), from a 2-byte aligned base pointer.  out_depth: that of I420 output;
        None = the same as depth (8 for RGB input).  The two are independent: depth=8, out_depth=10 keeps the two bits of the fp32
        result that the 8-bit rounding throws away, which is what a 10-bit HEVC / AV1 encoder wants.  10 and 12 bits are defined for
        the limited-range colour spaces (bt601, bt709) only.
        pixel_format="i422" / "i444", out="i422" / "i444": planar YUV 4:2:2 / 4:4:4 (Y4M's C422 / C444 and their p10 / p12 forms), frames
        of savsr_amd.yuv.frame_bytes(h, w, depth, chroma) bytes; size, colour, out_colour, depth and out_depth apply to them as to I420.
        The two sides are independent: pixel_format="i420", out="i444" keeps the network's full-resolution chroma, and RGB in with
        out="i422" is allowed.
        siting: where the chroma samples of 4:2:0 / 4:2:2 input lie, None or one of savsr_amd.yuv.SITINGS: "centre" (JPEG, MPEG-1; Y4M's
        C420jpeg), "left" (MPEG-2, H.264, HEVC 4:2:0 and every standard 4:2:2; C420mpeg2), "topleft" (C420paldv; 4:2:0 only).  With a
        siting, chroma is reconstructed by linear interpolation at the positions it names; None (the default) models none and replicates
        the nearest sample, as ever.  out_siting: that of YUV output; "left" / "topleft" filter cosited axes with [1 2 1] / 4, None and
        "centre" take the block mean.  The two are independent; siting goes with a YUV pixel_format and out_siting with a YUV out, and
        4:4:4 has nothing to resample (any siting gives the bytes of None).
        chroma_filter: None or "bicubic", for a luma-only checkpoint (num_in_ch = 1) on YUV video: pixel_format and out in "i420" / "i422" /
        "i444" are then accepted; the Y plane goes through the network (Y / 255 of the codes at 8 bits, the extra bits kept at 10 / 12,
        whatever the colour space: it is not converted, so out_colour must equal colour) and every output frame's U and V are resampled
        from its own input frame at the network's scale by a siting-aware Keys bicubic, samples to samples (savsr_amd/yuv.py
        "Luma-only checkpoints"); depth, out_depth, the out layout, siting and out_siting apply.  out="float" / "uint8" return the luma
        alone ([N, 1, H, W] / [N, H, W, 1]).  pixel_format / out = "y400": grey-scale frames, the Y plane alone (Y4M's Cmono), of
        yuv.frame_bytes(h, w, depth, "400") bytes, for num_in_ch = 1 only and without chroma_filter; YUV in, "y400" out drops the chroma,
        "y400" in, a chroma layout out is refused.  None (the default) runs what ran before the argument existed.
        cuts: None (one scene), a strictly increasing list of frame indices 0 < k < N (frame k starts a new scene), or "auto" (found on
        the GPU: savsr_amd.detect_cuts with scene_threshold, in per cent of the largest possible frame change; the default is ffmpeg
        scdet's and is not validated on real footage).  Windows stop at cuts: the result is, bit for bit, upscale_video on every scene
        alone, concatenated, a scene too short for `padding` taking "replicate" (savsr_amd/scenes.py); with cuts only N >= 1 is required.
        crop: None, a rect (y0, x0, ah, aw) or "auto", for letterboxed, pillarboxed and window-boxed video.  The frames are cropped to the
        rect before anything else looks at them: the result is, bit for bit, upscale_video on the video cropped by hand
        (savsr_amd.active.crop_frames) with every other argument the same, so the bars cost no network time and do not move the network's
        global pools.  A rect lies inside the frame with ah, aw >= 2 and sits on the input layout's chroma block (an off-block rect is
        refused with the aligned one it could have been).  "auto": savsr_amd.detect_active_area on the whole video with crop_limit, the
        largest mean of a black line on the 8-bit scale (ffmpeg cropdetect's rule and default; not validated on real footage).
        bars="keep" (the default) returns full-size frames, the picture at savsr_amd.active.place's corner in nominal black
        (active.insert_frames); bars="drop" returns the picture alone, get_hw(ah, aw, scale).  None (the default) runs what ran before.
        fields: None, "tff" or "bff", for interlaced video (top / bottom field first).  The N frames are deinterlaced into 2N progressive
        frames at the field rate before anything else looks at them (savsr_amd.deinterlace: ffmpeg yadif's rule in integers, on the GPU):
        the result is, bit for bit, upscale_video on savsr_amd.deinterlace(frames, fields, ...) with every other argument the same, so the
        length check, the crop, the cuts (explicit ones index the 2N frames: a cut at source frame k is 2k) and the windows all see the
        progressive video.  uint8 and planar frames only (float frames have no integer samples).  None (the default) runs what ran before.
        pulldown: None, "tff" or "bff", for telecined film (3:2 pulldown) with that field order; pulldown_cycle (default 5): one frame in
        so many is the repeated one.  The N frames become the N - N // pulldown_cycle film frames before anything else looks at them
        (savsr_amd.pulldown: every frame keeps its first field and takes the second from itself or its predecessor, whichever combs less;
        of every cycle the woven frame closest to its predecessor is dropped; on the GPU, two host synchronisations): the result is, bit
        for bit, upscale_video on savsr_amd.remove_pulldown(frames, pulldown, ...) with every other argument the same, and explicit cuts
        index the film frames.  Not together with fields.  No cadence tracking; see savsr_amd/pulldown.py for the limits.  None (the
        default) runs what ran before.
        surface, out_surface (keyword only): None or a savsr_amd.surface.Surface, for planar samples that do not lie as a Y4M file has them:
        a hardware decoder's NV12 / P010 surfaces with a row pitch and padded lines (Surface.nv12(pitch=..., lines=...), .nv21, .nv16, .p010,
        .p012, .p210, .p212), a capture card's packed 4:2:2 (Surface.uyvy(), .yuyv()), a software decoder's planar frames with a linesize
        (Surface.planar(pitch=...)).  pixel_format, size and depth still say which samples a frame has; `surface` says where they lie, and
        frames are [N, stride] uint8 with stride >= the surface's bytes.  They are unpacked on the GPU in front of everything else and the
        result is packed behind everything else: the call is, bit for bit, upscale_video on savsr_amd.unpack_surface(frames, surface,
        pixel_format, size, depth), and its result savsr_amd.pack_surface(result, out_surface, out, (H, W), out_depth), in which every byte
        no sample maps to is 0.  surface goes with a planar pixel_format ("i420", "i422", "i444", "y400"), out_surface with a planar out;
        pixel_format="nv12" stays an unknown format.  None (the default) runs what ran before.
        scan (keyword only): None or "detect", for video whose scan the caller does not know (a decoder's tensors carry no tag, and tags
        are often wrong).  "detect" runs savsr_amd.detect_scan on the unpacked frames on the GPU, right after surface= unpacking and in
        front of everything else (one more kernel launch and one host synchronisation), and continues exactly as if the verdict's
        kwargs() had been given: the result is, bit for bit, upscale_video(frames, **savsr_amd.detect_scan(frames, ...).kwargs(), ...)
        with every other argument the same -- fields=order for interlaced video, pulldown=order for telecined film, neither for
        progressive video and for video that shows no evidence (static, flat) -- so the length check and the cuts see the frame count the
        verdict implies.  Not together with fields, pulldown or a pulldown_cycle other than 5; uint8 and planar frames only.  The
        detector's rule and thresholds are this project's own and are not validated on real footage; one verdict per video
        (savsr_amd/scan.py has the limits).  None (the default) runs what ran before.
        dither (keyword only): None or one of savsr_amd.dither.DITHERS ("ordered"), for the integer outputs (out="uint8", "i420" / "i422" /
        "i444" at any depth, "y400" and the Y plane of the luma-only path).  None rounds the fp32 result to the nearest code, as ever.
        "ordered" writes floor(t + theta(y, x)) instead, t the value in output code units and theta a threshold in (0, 1) from a 16 x 16
        Bayer matrix at the sample's position in its own plane (Cb / Cr at their chroma-sample coordinates; the channels of a packed pixel
        share one threshold, so the dither is grey): a smooth gradient, which a x4 result stretches over four times as many pixels,
        keeps its mean over every 16 x 16 block to 1/256 of a code instead of turning into bands.  savsr_amd/dither.py is the
        specification and the kernels equal it bit for bit: the result is that module's rule applied to the out="float" result.  Exact
        codes pass unchanged, limited range stays in range without a clip, and the pattern is static in time, so any chunking gives the
        same bytes.  One pattern (no blue noise, no error diffusion); the luma-only path's resampled Cb / Cr keep rint; not validated on
        real footage; the gain is largest at 8 bits.  Refused with out="float" (nothing to quantise).  With the self-ensemble the merge
        stays fp32 and the dithered quantiser runs after it.
        deinterlacer, field_rate (keyword only): how fields= (or an interlaced verdict of scan="detect") is carried out.  deinterlacer:
        "yadif" (the default) or "bwdif", ffmpeg bwdif's rule (savsr_amd.deinterlace.bwdif_matrix: yadif's temporal clamp around the
        w3fdif interpolation filters), under which still areas -- captions, logos, locked-off shots -- come back as they are.  field_rate:
        "double" (the default: 2N frames) or "same": N frames, the first field in time of every source frame, so the network runs
        once per source frame; explicit cuts then index the N frames (a cut at source frame k is k).  The property holds with both:
        the result is upscale_video on savsr_amd.deinterlace(frames, fields, ..., method=deinterlacer, rate=field_rate).  Refused when
        not at their defaults without fields= or scan="detect", and together with pulldown=.  Not validated on real footage.
        combed, comb_threshold, comb_pixels (keyword only): for hybrid material -- telecined film with video-rate inserts, titles or
        effects, a stream cut inside a cadence.  combed: None (the default: what ran before), "yadif" or "bwdif".  After the field match
        every woven frame is measured for residual combing (savsr_amd.comb_windows: a second-field sample is combed iff its match
        measure exceeds 2 * comb_threshold; a frame is combed iff some 16 x 16 window, one every 8 rows and pixels, holds comb_pixels
        of them); the combed frames alone are deinterlaced at same rate by that method, from the woven frames beside them, and the
        decimation reads the cleaned frames (ffmpeg's fieldmatch -> yadif=deint=interlaced -> decimate chain).  The property holds: the
        result is upscale_video on savsr_amd.remove_pulldown(frames, pulldown, ..., combed=combed, comb_threshold=..., comb_pixels=...).
        Goes with pulldown= or scan="detect" (where it applies to a telecine verdict and is ignored for the others); refused with
        fields=, and comb_threshold / comb_pixels are refused without combed=.  Still two host synchronisations.  What remains: the
        decimation drops one of every pulldown_cycle frames of a true-video insert (judder, not combing); a cleaned frame has half its
        rows interpolated; small or low-contrast combing stays below the rule; one verdict per video.  The defaults are fieldmatch's
        cthresh and combpel rescaled to the window; they are not validated on footage.
        denoise, denoise_radius, denoise_strength, denoise_chroma_strength (keyword only): temporal noise reduction in front of the
        network, for tape, tuner and sensor noise and MPEG-2 flicker, which a network trained on clean downsamples would enlarge as
        detail.  denoise: None (the default: what ran before) or "ata": every sample becomes the rounded mean of itself and the same
        sample of up to denoise_radius (1 .. 16, default 4: nine frames) frames on either side -- two independent walks, each taking
        the next frame's sample while it differs by at most a and the walk's differences sum to at most b, denoise_strength = (a, b)
        in 8-bit code units at every depth, 0 <= a <= b <= 255, default (4, 9) (savsr_amd/denoise.py: ffmpeg atadenoise's serial rule
        in integers, on the GPU; the walks end at the video's ends).  Chroma planes take denoise_chroma_strength (None: the same).
        The stage runs after surface= unpacking, scan="detect" and fields= / pulldown= (it needs progressive frames) and in front of
        the crop, the cuts and the windows: the result is, bit for bit, upscale_video on savsr_amd.denoise_video(v', ...) with every
        other argument the same, v' the deinterlaced or pulldown-removed video; the rule is per sample, so it commutes with crop=
        exactly, and cuts="auto" scores the denoised frames.  uint8 and planar frames only; the denoise_ options are refused without
        denoise=.  Static samples pass unchanged and no sample moves by more than min(a, b).  Temporal only -- no spatial or
        motion-compensated filtering, so moving texture is not denoised at all; the taps read across scene cuts, where only the
        thresholds stop them; one strength per video.  The defaults are parameters: nothing is validated on footage or on trained
        weights.
        spatial_denoise, spatial_patch, spatial_search, spatial_strength, spatial_chroma_strength (keyword only): spatial noise
        reduction in front of the network, for grain, tuner and sensor noise on what moves, which denoise= leaves untouched.
        spatial_denoise: None (the default: what ran before) or "nlm": non-local means on the GPU, every frame on its own -- a sample
        becomes the weighted mean of the samples within spatial_search (1 .. 7, default 7: a 15 x 15 window) of it inside the plane,
        weighted by exp(-SSD / ((2 P + 1)^2 h^2)) from an integer table, SSD the squared difference of the (2 P + 1)^2 patches around
        the two, P = spatial_patch (1 .. 3, default 3), h = spatial_strength in 8-bit code units at every depth (0 < h <= 32, default
        3.0; savsr_amd/nlmeans.py is the rule in integers).  Chroma planes take spatial_chroma_strength (None: the same); every
        channel of packed frames is a plane of its own.  The stage runs after denoise= and after the crop, in front of the cuts and
        the windows: with crop=None the result is, bit for bit, upscale_video on savsr_amd.denoise_spatial(v', ...), v' the video
        after fields= / pulldown= / denoise=; with crop=rect and bars="drop" it is upscale_video on
        denoise_spatial(crop_frames(v', rect), ...), and with bars="keep" the picture inside the bars is those bytes (the rule does
        not commute with a crop: the bars never enter a patch).  cuts="auto" scores the filtered frames, crop="auto" reads the
        unfiltered ones.  uint8 and planar frames only; the spatial_ options are refused without spatial_denoise=.  One strength per
        video, no joint-channel weights, the centre weight is not corrected for noise, the search stops at 15 x 15.  The defaults are
        parameters: nothing is validated on footage or on trained weights, and nothing is pinned to ffmpeg's output.
        deblock, deblock_block, deblock_strength, deblock_chroma_strength (keyword only): deblocking in front of the network, for the
        8 x 8 block edges of MPEG-2 and low-bitrate H.264 sources, which neither denoiser removes and a x4 network enlarges onto a
        32-pixel grid.  deblock: None (the default: what ran before), "weak" or "strong": across the vertical edges of a grid of
        deblock_block (4, 8 or 16, default 8) samples whose first edges lie at deblock_origin, then across the horizontal ones, the 2 ("weak")
        or 3 ("strong") samples on either side of an edge move towards each other by 1/2, (1/4,) 1/8 of the step across it where that
        step is below a and the steps beside it are below b, deblock_strength = (a, b), ints in 0 .. 255 in 8-bit code units at every
        depth, default (25, 13) (savsr_amd/deblock.py is the rule in integers).  Chroma planes take deblock_chroma_strength (None: the
        same) and the same block in their own samples; every channel of packed frames is a plane of its own.  The block grid belongs
        to the coded frame, so the stage runs on the frames as decoded: right after surface= unpacking and after scan="detect" has
        read the unfiltered frames, in front of fields= / pulldown=, denoise=, the crop, spatial_denoise= and the cuts.  It filters
        the two fields as planes of their own (vertical block deblock_block // 2: weak below 8, no vertical pass at block 4) exactly
        when the video is treated as interlaced -- fields= or pulldown= given, or an interlaced or telecine verdict of scan="detect".
        The result is, bit for bit, upscale_video on savsr_amd.deblock_video(frames, ..., interlaced=I) with every other argument the
        same, I as just said; crop= then crops the filtered frames, so crop="auto" reads filtered frames.  uint8 and planar frames
        only; the deblock_ options are refused without deblock=.  deblock_origin = (oy, ox), deblock_chroma_origin (keyword only): the
        grid's first edges, 0 <= o < deblock_block, default (0, 0): a video whose bars or overscan were cropped by c samples before it
        arrived has them at (-c) mod block.  oy must be even where the stage runs field by field.  The chroma planes of 4:2:0 / 4:2:2
        frames have an origin of their own, in chroma samples, which must be named beside a luma origin other than (0, 0); elsewhere
        None means the same origin.  deblock_grid="auto" (keyword only) finds block and origins from the frames instead
        (savsr_amd/grid.py; savsr_amd.detect_grid is the call): the statistics of the frames the deblocker will read, summed over the
        video on the GPU, one more host synchronisation, an exact rule on the host.  The result is, bit for bit, the call with
        `verdict.kwargs()` given, and with a "no grid" verdict the call with deblock=None, so a clean source passes through
        untouched; chroma planes that show no grid of the luma's block are left alone.  It is refused together with a deblock_block or
        an origin other than the defaults.  The detector's rule and defaults are this project's own and are not validated on footage;
        grids of scaled video, block sizes other than 4 / 8 / 16 and block 4 on noise-free material are not found, and periodic
        picture content can fake a grid.  One grid and one strength per video, no adaptation to the stream's quantiser,
        ringing and mosquito noise are left to dering= (next).  The defaults are ffmpeg deblock's thresholds as parameters: nothing is
        validated on footage or on trained weights, and nothing is pinned to ffmpeg's output.
        dering, dering_strength, dering_chroma_strength, dering_damping (keyword only): deringing in front of the network, for the
        oscillations a coarsely quantised 8 x 8 DCT puts around every sharp edge inside a block (ringing, mosquito noise), which the
        deblocker and both denoisers leave and a x4 network enlarges as texture.  dering: None (the default: what ran before) or
        "cdef": every 8 x 8 block of a plane, on a grid at the plane's origin, gets one of eight directions from its line sums; every
        sample then moves by a constrained sum of four taps along its block's direction and eight across it, clamped to the minimum
        and maximum of the sample and its taps.  dering_strength = (p, s), ints 0 <= p <= 15 (along; scaled by the block's directional
        variance, nothing on a flat block) and 0 <= s <= 4 (across), default (4, 2); dering_damping, an int in 3 .. 6, default 5: a
        tap whose difference is large against its strength counts less, then not at all; all in 8-bit code units at every depth
        (savsr_amd/dering.py is the rule in integers; the idea is that of AV1's CDEF, the definition this project's).  Chroma planes
        take dering_chroma_strength (None: the same); every channel of packed frames is a plane of its own.  Ringing belongs to the
        coded frame as the block grid does, and codecs dering after they deblock: the stage runs right behind deblock= on the frames
        as decoded -- after surface= unpacking and after scan="detect" and deblock_grid="auto" have read their frames, in front of
        fields= / pulldown=, denoise=, the crop, spatial_denoise= and the cuts -- field by field (each field with blocks of its own)
        exactly when the deblocker would.  The result is, bit for bit, upscale_video on savsr_amd.dering_video(
        savsr_amd.deblock_video(frames, ...), ..., interlaced=I) with every other argument the same.  uint8 and planar frames only;
        the dering_ options are refused without dering=.  One strength per video and no per-block signalling such as a bitstream
        carries; the 8 x 8 analysis grid starts at the plane's origin and does not follow deblock_origin; chroma gets a direction of
        its own rather than the luma's; the stage also smooths fine noise.  The defaults are parameters: nothing is validated on
        footage or on trained weights, and nothing is pinned to libaom's or ffmpeg's output.
        denoise_strength="auto" / spatial_strength="auto" (beside denoise= / spatial_denoise=): the strength from the noise level of the
        frames (savsr_amd/noise.py; savsr_amd.estimate_noise is the call): the 8 x 8 cell sums of the absolute second difference
        [1 -2 1]^T (x) [1 -2 1], summed over the video on the GPU, one launch per plane and one more host synchronisation each, then
        an exact rule on the host (the mean of the quietest quarter of the cells that are not flat, over 245).  Each is measured on the
        frames its stage will read: the temporal one right in front of the temporal denoiser, the spatial one right in front of the
        spatial denoiser, behind denoise= and the crop.  The result is, bit for bit, the call with `verdict.denoise_kwargs()` /
        `verdict.spatial_kwargs()` given, and where no noise is found (sigma below 1/2 code, or too few cells) the call without that
        stage, so a clean source passes through untouched; an explicit chroma strength beside "auto" wins over the found one.  One
        figure per video, a white-noise model (coarse grain, subsampled chroma and clipped levels read low, texture over most of the
        frame reads high); the measure, its constants and the gains are this project's own and are not validated on footage or on
        trained weights.
        With set_self_ensemble(True) every frame is the self-ensemble of its window.  Arguments are checked before anything runs on the
        GPU.  Streaming form: savsr_amd.VideoUpscaler."""
        from ..video import upscale_video
        return upscale_video(self, frames, scale, padding, out, pixel_format, size, cuts, scene_threshold, colour, out_colour, depth, out_depth,
                             siting, out_siting, chroma_filter, crop, crop_limit, bars, fields, pulldown, pulldown_cycle, surface=surface,
                             out_surface=out_surface, scan=scan, dither=dither, deinterlacer=deinterlacer, field_rate=field_rate, combed=combed,
                             comb_threshold=comb_threshold, comb_pixels=comb_pixels, denoise=denoise, denoise_radius=denoise_radius,
                             denoise_strength=denoise_strength, denoise_chroma_strength=denoise_chroma_strength,
                             spatial_denoise=spatial_denoise, spatial_patch=spatial_patch, spatial_search=spatial_search,
                             spatial_strength=spatial_strength, spatial_chroma_strength=spatial_chroma_strength, deblock=deblock,
                             deblock_block=deblock_block, deblock_strength=deblock_strength, deblock_chroma_strength=deblock_chroma_strength,
                             deblock_origin=deblock_origin, deblock_chroma_origin=deblock_chroma_origin, deblock_grid=deblock_grid, dering=dering,
                             dering_strength=dering_strength, dering_chroma_strength=dering_chroma_strength, dering_damping=dering_damping)

    def forward(self, x: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
        if self.training:
            raise RuntimeError("savsr_amd.SAVSR implements the inference path only; call .eval() first")
        if x.dim() != 5:
            raise ValueError("expected lq of shape [b, t, c, h, w]")
        if taps is not None and self.self_ensemble:
            raise ValueError("taps are single-pass diagnostics: set_self_ensemble(False) to collect them")
        with torch.no_grad():
            return self.engine().forward(x, self.scale, taps, ensemble=self.self_ensemble)
