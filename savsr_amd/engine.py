"""Host-side driver of the HIP kernels for the SAVSR inference path.

`HipEngine` = the launch sequence that replaces `SAVSR.forward` (/root/reference/lbasicsr/archs/savsr_arch.py:692-742): the stage
functions (bidirectional propagation, pyramid fusion, RCAN trunk + OSAdapt, SATU, tail), their capture into hipGraphs per
(shape, scale), the fan-out of independent clips over HIP streams and the batching of equal clips into the launches.  The entry points
`forward`, `forward_many` and `forward_video` differ in how they cut their clips into launch units (`chunk_units`, `many_units`,
`video_units`) and in where a unit's clips come from; `_fan_out` deals the units over the streams, `_run_unit` runs one, and `_flow` owns
the state (`nb`, `form_nb`, `conv_algo`) a frame's launches depend on.  What it stands on lives next door:

    packing.py   WeightPacking   state_dict -> split-bf16 weight images, OSConv banks, SATU matrices (once per engine)
    cache.py     ContextCache    (shape, scale) buffer contexts, arena, liveness plan, byte budget, eviction limbo
    launch.py    Launcher        descriptors + C-ABI calls: convs, OSConv weight generation, SATU tables / plans / stages
    config.py    EngineConfig    every SAVSR_* switch, read once when the engine is built

PyTorch is used for device memory and streams only: every arithmetic step is a call into libsavsr_hip.so through the C ABI of
include/savsr_hip.h.  There is no CPU / eager-PyTorch fallback.
"""
from __future__ import annotations

import gc
import os
import sys
import time
import weakref
from contextlib import contextmanager
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ConvDesc, OSConvAttnDesc, SatuTiling, SatuWeights      # noqa: F401
from .cache import ContextCache
from .config import EngineConfig
from .dither import dither_id
from .launch import MAX_SUM_BLOCKS, Launcher, Src, _ptr      # noqa: F401
from .packing import (BN_EPS, CONV_TH, CONV_TW, WeightPacking, acc_row, conv_pack_geometry, conv_pack_index, conv_wy_pack_index, get_hw,      # noqa: F401  (re-exported:
                      pack_conv_part, pack_conv_weight, pack_conv_weight_wy, satu_axis_tables, split_bf16_image, window_record)                            # tests and tools import them from here)
from .video import VideoSpec, video_spec
from .yuv import CHROMAS, COLOURS, SITINGS, chroma_hw, layout_name


class HipEngine(WeightPacking, ContextCache, Launcher):
    def __init__(self, state: Dict[str, torch.Tensor], cfg: dict, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError("savsr_amd runs on an AMD GPU only (device 'cuda' under PyTorch-ROCm); "
                               "there is no CPU fallback")
        self.lib = _lib.load()
        self.dev = device
        self.knobs = kn = EngineConfig.from_env()        # every SAVSR_* switch, read here and nowhere else (config.py)
        # clips per batched launch sequence the library's batch limits allow: 6 convs (a block's two directions x 3 streams) and 2 OSConvs per clip
        self.NB_MAX = max(1, min(int(self.lib.savsr_conv2d_max_batch()) // 6, int(self.lib.savsr_osconv_weights_max_batch()) // 2))
        with torch.cuda.device(device):                      # per device: every kernel's > 64 KiB dynamic-LDS attribute, before any capture
            _lib.check(self.lib.savsr_prepare_device(), "savsr_prepare_device")
        self.cfg = dict(cfg)
        self.nf = cfg["num_feat"]
        if self.nf not in (32, 64):
            raise RuntimeError(self.num_feat_limit(self.nf))
        why = self.window_limit(cfg)
        if why is not None:
            raise RuntimeError(why)
        self.nch, self.sw = cfg["num_in_ch"], cfg["slid_win"]
        self.rw = window_record(self.nch, self.sw)                 # floats per pixel of a packed input window
        self.pw: Dict[str, tuple] = {}      # conv key -> (wimage, bias, cout, cin, ks)
        self.pw_wy: Dict[str, torch.Tensor] = {}      # conv key -> Winograd-y weight image (static 3x3 convs with cout % 64 == 0)
        # Precision mode (set_precision): "fp32" = the split-bf16 products; "fp16" = fp16 operands in every conv launch (savsr_conv2d_batch_f16,
        # savsr_osconv_weights_batch_f16), everything else unchanged.  The fp16 images of the static convs are built on the first fp16 forward.
        self.precision = "fp32"
        self.pw16: Dict[str, torch.Tensor] = {}       # conv key -> fp16 image (direct form)
        self.pw16_wy: Dict[str, torch.Tensor] = {}    # conv key -> fp16 Winograd-y image
        self._conv_src: Dict[str, tuple] = {}         # conv key -> how its weight derives from the state_dict (packing.py::_conv_weight)
        # Per-stream state: a sibling engine (clone_for_stream) owns its own `osc` / `rcab_scr` scratch, `se_gate`, what _init_caches creates (buffer
        # contexts, hr_sched), `nb` / `_bstride` / `form_nb`, `conv_algo`, `satu_events` / `_st`, `_siblings` / `_streams` and the lazily made
        # `_cap_stream` / `_side_stream`.  EVERY other attribute is shared with the siblings by reference (packed weights, knobs, HR plans,
        # census, host_stats, ...): a new shared attribute needs nothing in clone_for_stream, a new per-stream one is reset there.
        self.osc: Dict[str, dict] = {}      # osconv key -> tensors
        self.se: Dict[str, tuple] = {}
        self.rcab_w: Dict[str, dict] = {}     # RCAB prefix -> what the folded form reads (packing.py::_add_rcab_fold)
        # RCAB with the SE gate folded into conv.2's weights (savsr_rcab_gate_weights_batch): 1 = in the throughput flow, 2 = in both flows,
        # 0 = conv, conv, SE pass everywhere (SAVSR_RCAB_FOLD; `rcab`)
        self.rcab_fold = kn.rcab_fold
        self._keep: List[torch.Tensor] = []
        self._init_caches()
        self.satu_events: Optional[list] = None     # bench.py: (start, end, clips) HIP events around the SATU stage(s) of a launch sequence
        self._st: Optional[int] = None              # cached stream handle while a frame's launches are being issued (_stream)
        self._cap_stream: Optional[torch.cuda.Stream] = None      # capture stream (_capture) and table stream (_plan_hr_tiling), made on first use
        self._side_stream: Optional[torch.cuda.Stream] = None
        # Clips of ONE (shape, scale) batched into the launches (round 5).  A small clip is launch-latency-bound -- 330 dependent launches at ~11 us
        # each whatever its size (tools/probe_small_clips.py) -- and more than three streams do not help (a conv workgroup holds its CU's LDS).  With
        # nb clips in one launch sequence every named buffer holds nb copies (`_bstride`: bytes between them), every conv / OSConv descriptor is
        # issued once per clip INSIDE the same batched launch (savsr_conv2d_batch takes 24 convs since ABI 27) and the per-clip kernels (SE gate,
        # SATU, tail, ...) are looped: 151 + 63 + nb x ~116 launches for nb clips instead of nb x 330.  Results are those of a one-clip launch
        # sequence of the SAME flow bit for bit (the convs of a batched launch are independent and their form is chosen by `form_nb`, not `nb`).
        # Which clips share a launch sequence: clip_unit (up to SAVSR_CLIP_BATCH, default 4, clips of one (shape, scale) when the LR frame has at
        # most SAVSR_CLIP_BATCH_MAX_PX pixels).
        self.nb = 1
        # Clips the conv-form rule of a launch counts (conv_launch): `clip_batch` for every frame of the throughput flow whose shape is eligible for
        # batching, 1 otherwise -- whatever `nb` the launch sequence at hand really carries.  A unit of 1, 2 or 3 clips of a folder therefore takes
        # the same form in every launch, and a clip's output does not depend on its group (remainders of a folder, the world-size partition).
        self.form_nb = 1
        self._bstride: Dict[int, int] = {}
        self.clip_batch = max(1, min(self.NB_MAX, kn.clip_batch))
        self.clip_batch_max_px = kn.clip_batch_max_px
        self.census: Optional[dict] = None          # bench.py: per-launch matrix-work census (_count_conv), shared with the sibling engines
        # SAVSR_CAPTURE_AFTER = n: a (shape, scale) context's first n frames run EAGERLY and the hipGraphs are captured on visit n + 1 (eager,
        # captured and replayed frames are the same launch sequence: bit-identical results).  Default 0 = capture on the first visit, by
        # measurement (bench.py --config run_test --emulate-world 8, cProfile of a rank's cold pass): the Python launch sequence of one frame costs
        # ~8 ms of host time -- more than the 4-5 ms the GPU needs for a Vid4-sized frame -- and a capture is that same sequence issued once, so
        # eager frames are host-bound and a block of >= 3 frames is already faster captured (8 + 4.5 n against 8 n ms).
        self.capture_after = kn.capture_after
        self.host_stats = {"captures": 0, "capture_s": 0.0, "plan_s": 0.0, "eager_frames": 0}     # shared with the sibling engines (bench.py)
        self.conv_algo = _lib.CONV_DIRECT           # CONV_DIRECT_THROUGHPUT while several clips are in flight (forward_many / batches)
        self._hr_choice: Dict[tuple, int] = {}      # (h, w, sh, sw) -> timed choice of the HR kernel's wave split; shared with the sibling engines
        self._hr_table = self._load_hr_plans()      # scale -> plan measured once per build of the SATU kernels (savsr_amd/hr_plans.json)
        self.use_graphs = kn.graphs
        # The SATU -> tail form every frame runs, chosen here once (the per-form methods _satu_lrcat ... _tail_clip dispatch on it):
        #   "q"    row-summed: savsr_satu_hr_tail_q writes 9 planes + seams, savsr_tail_gather_q (num_feat 64, 3 channels)
        #   "p27"  the tuned kernels' 27 tail-projected planes, savsr_tail_gather (SAVSR_SATU_Q=0)
        #   "nf"   width-generic savsr_satu_nf_* (num_feat != 64 or num_in_ch != 3; records of satu_nf_rec floats): 9 num_in_ch planes
        #          (tail_planes; 27 at num_in_ch = 3), savsr_tail_gather / savsr_tail_gather_nch
        self.satu_generic = self.nf != 64 or self.nch != 3
        self.satu_form = "nf" if self.satu_generic else ("q" if kn.satu_q else "p27")
        self.tail_planes = 9 * self.nch
        self.satu_nf_rec = int(self.lib.savsr_satu_nf_lrcat_floats(self.nf)) if self.satu_generic else 0
        # static-weight 3x3 convs in the Winograd F(2,3)-along-y form (SAVSR_CONV_WINOGRAD_Y); SAVSR_CONV_WY=0: the direct kernel everywhere
        self.conv_wy = kn.conv_wy
        # OSConv weight generation as ONE launch (savsr_osconv_attn_desc.fused: the routing recomputed in every aggregation workgroup; bit-identical).
        # OFF: measured slower -- one clip 8.96 -> 9.77 ms, three in flight 120.3 -> 118.0 HR Mpixel/s (A/B/A on one lease): a workgroup pulling
        # the 0.8 MB of routing weights + pool partials through ONE CU takes ~40 us longer than the two extra launches it saves
        self.osconv_fused = kn.osconv_fused
        self.reuse_buffers = kn.reuse_buffers      # liveness-planned LR buffers (release()); 0: every name its own memory
        self.wy_min_tiles = kn.wy_min_tiles          # launches with at least this many 16-row tiles take the Winograd form ...
        self.wy_min_tiles_tp = kn.wy_min_tiles_tp    # ... or this many with several clips in flight (throughput tiling)
        self.n_streams = kn.streams   # launch units of a batch in flight concurrently ...
        # ... fewer when the frames are large (streams_for): a launch of a >= 40 kpx frame fills the chip on its own, a second stream fills the
        # launch boundaries and the conv tails, a third only adds contention (config 2, 16-24 clips per step on one lease: 4 clips x 2 streams
        # 130.4-130.9, x 3 streams 130.1 HR Mpixel/s; the YAML workflow 151 vs 145 frames/s); small clips are launch-latency-bound and want the
        # third (config 5: 329 clips/s with 3 streams, 311 with 2)
        self.n_streams_large, self.streams_large_px = kn.streams_large, kn.streams_large_px
        self._siblings: List["HipEngine"] = []
        self._luma_tables: Dict[tuple, tuple] = {}      # chroma resampler tables on the device (`_chroma_tables`)
        self._streams: List[torch.cuda.Stream] = []
        self._pack_all({k: v.detach() for k, v in state.items()})

    satu_q = property(lambda self: self.satu_form == "q", doc="The row-summed SATU form (bench.py, tools/time_satu.py).")

    @staticmethod
    def num_feat_limit(nf: int) -> str:
        """Why a checkpoint of this num_feat does not run (engine build)."""
        msg = f"num_feat = {nf} is not supported: the HIP SATU kernels are built for num_feat 64 (tuned) and 32 (savsr_satu_nf_*)"
        if nf > 64:
            msg += (f"; beyond that, OSConv weight generation (savsr_osconv_weights_batch) takes cin <= 320 and hidden <= 32, and the pyramid "
                    f"fusion's OSConvs at num_feat = {nf} have cin = {5 * nf}")
        return msg

    @staticmethod
    def window_limit(cfg: dict) -> Optional[str]:
        """Why a checkpoint of this num_in_ch / slid_win / fusion_win does not run (engine build); None when it does."""
        nch, sw, fw = cfg["num_in_ch"], cfg["slid_win"], cfg["fusion_win"]
        if not 1 <= nch <= 3:
            return (f"num_in_ch = {nch} is not supported: the SATU / tail fold keeps the tail conv's 9 * num_in_ch rows inside the 32-row MFMA "
                    f"tile of the LRcat record, so num_in_ch <= 3")
        if sw < 3 or sw % 2 == 0:
            return (f"slid_win = {sw} is not supported: the window is the centre frame with the same number of support frames on each side, "
                    f"so slid_win is odd and >= 3 (at slid_win = 1 the reference builds conv_sup with 0 input channels)")
        if nch * sw > 32:
            return f"num_in_ch * slid_win = {nch * sw} is not supported: the packed input window holds at most 32 channels per pixel"
        from .archs.savsr_arch import iteration_window
        center = cfg["num_frame"] // 2 if cfg["center_frame_idx"] is None else cfg["center_frame_idx"]
        iw = iteration_window(cfg["num_frame"], cfg["interval"], center)
        if (iw - fw + 1) // 2 >= 1 and iw - sw + 1 < fw:
            return (f"the pyramid level takes fusion_win = {fw} inputs but the propagation yields iter_win - slid_win + 1 = {iw - sw + 1}: "
                    f"the reference's WindowUnit_l2.forward raises an IndexError for this configuration")
        return None

    NB_MAX = 4                  # (class default; the instance reads the library's batch limits: 24 convs / 8 OSConvs per launch => 4 clips)

    HR_PLANS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hr_plans.json")

    def _load_hr_plans(self) -> Dict[tuple, tuple]:
        """The HR stage's launch plan per scale as measured for THIS build of the SATU kernels (tools/tune_hr_plans.py writes the file with the
        library's savsr_source_hash_satu()): every rank of a multi-GPU run, and every run, then launches the same plan without timing the
        candidates on its first frame of a (folder, scale) -- eight ranks used to make eight measurements and could pick eight plans.  A table
        from another build is ignored (the engine measures, as before); so is an entry whose plan is not feasible for the offsets of the loaded
        weights.  Results never depend on the plan (bit-identical in every plan)."""
        if not self.knobs.hr_plans:
            return {}
        try:
            import json
            with open(self.HR_PLANS_FILE) as f:
                t = json.load(f)
            if t.get("satu_source_hash") != self.lib.savsr_source_hash_satu().decode():
                return {}
            # entry: [variant, tile rows, tile columns / 32, LR h, LR w of the measurement]
            return {tuple(float(v) for v in k.split(",")): (tuple(int(x) for x in p[:3]), int(p[3]), int(p[4])) for k, p in t.get("plans", {}).items() if len(p) >= 5}
        except (OSError, ValueError, AttributeError):
            return {}

    def clone_for_stream(self) -> "HipEngine":
        """A sibling engine for another HIP stream: a shallow copy of this one -- packed weights, knobs, HR plans, census and host_stats
        shared by reference -- whose per-stream state (listed in __init__) is its own, so two launch units can be in flight on two streams."""
        e = HipEngine.__new__(HipEngine)
        e.__dict__.update(self.__dict__)
        # the per-stream state, and nothing else (_bstride first: _osc_scratch records the clip strides of the new scratch in it)
        e.nb, e._bstride, e.form_nb, e.conv_algo = 1, {}, 1, _lib.CONV_DIRECT
        e.osc = {k: dict(ent, **e._osc_scratch(ent["cin"], ent["cout"], ent["knum"], ent["nunits"] * 8)) for k, ent in self.osc.items()}
        e.se_gate = torch.empty_like(self.se_gate)
        e.rcab_scr = e._rcab_scratch()
        e._init_caches()               # its own buffer contexts and hr_sched; the byte budget, SATU axis tables and count caps stay shared
        e.max_shapes, e.max_scales, e._budget, e._axes = self.max_shapes, self.max_scales, self._budget, self._axes
        self._budget["engines"].append(weakref.ref(e))
        e.satu_events, e._st = None, None
        e._siblings, e._streams = [], []
        e._cap_stream = e._side_stream = None
        return e

    PRECISIONS = ("fp32", "fp16")

    def set_precision(self, mode: str) -> None:
        """The operand precision of the conv launches, for this engine and its stream siblings (SAVSR.set_precision)."""
        if mode not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {self.PRECISIONS}, got {mode!r}")
        self.precision = mode
        for e in self._siblings:
            e.precision = mode

    def _ensure_precision(self) -> None:
        """Before a frame is issued (never inside a capture): the fp16 images exist when the mode needs them."""
        if self.precision == "fp16" and not self.pw16:
            self._build_f16()

    def _graph_key(self, throughput: bool):
        """Key of a context's captured graphs: the flow and, for fp16, the precision (a graph is never replayed in the other mode; the
        context's buffers are shared)."""
        return throughput if self.precision == "fp32" else (throughput, self.precision)

    # ------------------------------------------------------------------ network pieces
    def residual_blocks(self, groups: List[Tuple[str, List[Src], str]], hp: int, wp: int, scale, use_osconv: bool) -> List[List[Src]]:
        """ResidualBlock (savsr_arch.py:399-415), cat-free, for several independent blocks of the same
        shape at once (the two propagation directions): the per-stream convs of all of them go out as
        single batched launches.  groups: (weight prefix, input streams, buffer tag)."""
        nf = self.nf
        L = ACT_LRELU
        x1s, d0 = [], []
        for pfx, xs, tag in groups:
            n = len(xs)
            x1 = [self.full(self.buf(f"{tag}.x1.{i}", hp, wp, nf)) for i in range(n)]
            pb = self.pool_buf(pfx + ".osconv", hp, wp, n * nf) if use_osconv else None     # OSConv pools cat(x1) (:146)
            d0 += [self.conv_desc(f"{pfx}.conv0.{i}", [xs[i]], x1[i], hp, wp, L, 0.2,
                                  pool=(pb, i * nf, n * nf) if use_osconv else None) for i in range(n)]
            x1s.append(x1)
        self.conv_launch(d0, "conv0")
        bases, d1 = [], []
        if use_osconv:                                   # the groups' OSConvs are independent: one batched weight generation
            keys = [pfx + ".osconv" for pfx, _, _ in groups]
            wy = self.osconv_wy(len(groups), nf, hp, wp)      # the dynamic convs below go out as ONE launch: its form decides the image's
            wds = self.osconv_launch(keys, [self.osconv_desc(k, x1, hp, wp, scale, pooled=True, wy=wy) for k, x1 in zip(keys, x1s)])
        for gi, ((pfx, xs, tag), x1) in enumerate(zip(groups, x1s)):
            base = self.full(self.buf(f"{tag}.base", hp, wp, nf))
            if use_osconv:
                d1.append(self.conv_desc(pfx + ".osconv", x1, base, hp, wp, L, 0.2, weights=wds[gi]))
            else:
                d1.append(self.conv_desc(pfx + ".conv1", x1, base, hp, wp, L, 0.2))
            bases.append(base)
        self.conv_launch(d1, "osconv" if use_osconv else "conv1")
        outs, d2 = [], []
        for (pfx, xs, tag), x1, base in zip(groups, x1s, bases):
            o = [self.full(self.buf(f"{tag}.out.{i}", hp, wp, nf)) for i in range(len(xs))]
            d2 += [self.conv_desc(f"{pfx}.conv2.{i}", [base, x1[i]], o[i], hp, wp, L, 0.2, res1=xs[i]) for i in range(len(xs))]
            outs.append(o)
        self.conv_launch(d2, "conv2")
        for x1, base in zip(x1s, bases):                 # the block's temporaries are dead (their last readers are enqueued)
            self.release(*x1, base)
        return outs

    def residual_block(self, pfx: str, xs: List[Src], hp: int, wp: int, scale, use_osconv: bool, tag: str) -> List[Src]:
        return self.residual_blocks([(pfx, xs, tag)], hp, wp, scale, use_osconv)[0]

    def windows_l1(self, units: List[Tuple[str, Src, Src, Src, str]], hp: int, wp: int, scale):
        """WindowUnit_l1 (savsr_arch.py:444-464) for independent units at once (f2p and p2f of one
        recurrence step).  units: (prefix, packed window [hp][wp][16], h_past, merge output, tag)."""
        nf = self.nf
        hcs = [self.buf(f"{tag}.hcs", hp, wp, 2 * nf) for _, _, _, _, tag in units]       # h_c | h_sup from one fused conv
        self.conv_launch([self.conv_desc(pfx + ".win", [win], self.full(h), hp, wp, ACT_LRELU, 0.2)
                          for (pfx, win, _, _, _), h in zip(units, hcs)], "win")
        feats = [[self.full(h, nf, 0), self.full(h, nf, nf), past] for (_, _, past, _, _), h in zip(units, hcs)]
        for k in range(self.cfg["w1_num_block"]):
            prev = feats
            feats = self.residual_blocks([(f"{u[0]}.blocks.{k}", f, f"{u[4]}.b{k}") for u, f in zip(units, feats)], hp, wp, scale, k >= 1)
            if k >= 1:                                   # the previous block's outputs (this block's inputs / residuals) are dead
                for f in prev:
                    self.release(*f)
        self.conv_launch([self.conv_desc(u[0] + ".merge", f, u[3], hp, wp) for u, f in zip(units, feats)], "merge")
        for f in feats:
            self.release(*f)
        self.release(*hcs)
        return [u[3] for u in units]

    def rcab(self, pfx: str, x: Src, out: Src, hp: int, wp: int, tag: str) -> Src:
        """savsr_arch.py:527-549.  `rcab_fold`: the gate is evaluated from conv.0's output (its pool partials and border lines) and multiplied
        into conv.2's weights and bias, whose epilogue then writes out = x + g (.) conv.2(r1) itself -- no pass over r2, x and out.  By default in the throughput flow only:
        with one clip in flight the gate launch (a handful of workgroups) takes longer than the 44 MB pass it replaces."""
        nf = self.nf
        part = self.pool_buf("se", hp, wp, nf)
        if self.rcab_fold >= 2 or (self.rcab_fold == 1 and self.conv_algo == _lib.CONV_DIRECT_THROUGHPUT):
            assert x.pix == nf and out.pix == nf
            r1 = self.conv(pfx + ".0", [x], self.full(self.buf(f"{tag}.t1", hp, wp, nf)), hp, wp, ACT_RELU, pool=(part, 0, nf))
            # (the form of the conv launch below decides the image's, as for an OSConv)
            wd = self.rcab_gate_weights(pfx, r1, part, hp, wp, wy=self.osconv_wy(1, nf, hp, wp))
            return self.conv(pfx + ".2", [r1], out, hp, wp, ACT_NONE, res1=x, weights=wd)
        r1 = self.conv(pfx + ".0", [x], self.full(self.buf(f"{tag}.t1", hp, wp, nf)), hp, wp, ACT_RELU)
        r2 = self.conv(pfx + ".2", [r1], self.full(self.buf(f"{tag}.t2", hp, wp, nf)), hp, wp, ACT_NONE, pool=(part, 0, nf))
        nblk = self.pool_rows(hp, wp)
        w1, b1, w2, b2, cm = self.se[pfx]
        st = self._stream()
        assert x.pix == nf and out.pix == nf
        # (one launch for all clips of a batched launch sequence: grid.y = clip, byte strides between the clips' operands)
        _lib.check(self.lib.savsr_se_scale_residual_batch(part.data_ptr(), nblk, 1.0 / (hp * wp), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                                          nf, cm, r2.ptr, x.ptr, out.ptr, hp * wp, self.nb, self._bs(part), r2.bs, x.bs, out.bs, st),
                   "savsr_se_scale_residual")
        return out

    def osadapt(self, g: int, x: Src, share: Optional[Src], out: Src, hp: int, wp: int, scale, pooled: bool = False) -> Src:
        """savsr_arch.py:186-214 fused with `+ gamma * share` of :732 (share=None: OSAdapt alone).
        pooled=True: the conv that produced x already wrote the pool partials of adapt.{g}.adapt."""
        m = f"adapt.{g}.mask"
        st = self._stream()
        c4 = self.pw[m + ".0"][2]
        h2, w2 = hp // 2, wp // 2
        m1 = self.conv(m + ".0", [x], self.full(self.buf("ad.m1", hp, wp, c4)), hp, wp, ACT_RELU)
        m2 = self.buf("ad.m2", h2, w2, c4)
        for b in range(self.nb):
            _lib.check(self.lib.savsr_avgpool2(m1.ptr + b * m1.bs, m2.data_ptr() + b * self._bs(m2), c4, hp, wp, st), "savsr_avgpool2")
        m3 = self.conv(m + ".4", [self.full(m2)], self.full(self.buf("ad.m3", h2, w2, c4)), h2, w2, ACT_RELU)
        m4 = self.conv(m + ".7", [m3], self.full(self.buf("ad.m4", h2, w2, c4)), h2, w2, ACT_RELU)
        m5 = self.buf("ad.m5", hp, wp, c4)
        for b in range(self.nb):
            _lib.check(self.lib.savsr_upsample2x(m4.ptr + b * m4.bs, m5.data_ptr() + b * self._bs(m5), c4, h2, w2, st), "savsr_upsample2x")
        mask = self.buf("ad.mask", hp, wp, 1)
        self.conv(m + ".11", [self.full(m5)], self.full(mask), hp, wp, ACT_SIGMOID)
        wd = self.osconv_weights(f"adapt.{g}.adapt", [x], hp, wp, scale, pooled=pooled, wy=self.osconv_wy(1, self.nf, hp, wp))
        return self.conv(f"adapt.{g}.adapt", [x], out, hp, wp, ACT_NONE, mul_px=mask, res1=x, res2=share,
                         res2_scale=self.gamma, weights=wd)

    # ------------------------------------------------------------------ diagnostics
    def time_satu_parts(self, lq: torch.Tensor, scale, timer) -> dict:
        """Diagnostics (tools/scale_sweep.py, bench.py): the SATU LR / HR launches and the tail of the product path, each timed
        alone by `timer(fn) -> us` on the tensors of a real frame of the latency flow.  lq: [T, num_in_ch, h, w] on the device."""
        lq = lq.contiguous()
        with self._frame(lq, False):
            self._select(lq.shape, scale)
            c = self._stage_body(lq, scale)
            out = torch.empty(self.nch, c["H"], c["W"], device=self.dev)
            lrcat = self._satu_lr_clip(c)
            self._stage_satu(c, scale)
            return {"satu_lr_us": timer(lambda: self._satu_lr_clip(c)),
                    "satu_hr_us": timer(lambda: self._satu_hr_clip(lrcat, c, scale)),
                    "tail_us": timer(lambda: self._stage_tail(c, lq, out))}

    # ------------------------------------------------------------------ whole frame
    def _stage_body(self, lq: torch.Tensor, scale) -> dict:
        with HipEngine._StageStream(self):
            return self._stage_body_impl(lq, scale)

    def _stage_body_impl(self, lq: torch.Tensor, scale) -> dict:
        """Everything up to the SATU inputs (savsr_arch.py:692-734).  lq: [T, num_in_ch, h, w] on device."""
        cfg, nf = self.cfg, self.nf
        if lq.dim() == 5:          # [nb, T, num_in_ch, h, w]: nb clips of one (shape, scale) in one launch sequence (see `nb`)
            assert lq.shape[0] == self.nb and lq.is_contiguous() and cfg["interval"] == 0
        else:
            assert self.nb == 1
        T, cin, h_in, w_in = lq.shape[-4:]
        clip_bytes = 4 * T * cin * h_in * w_in
        assert T == cfg["num_frame"] and cin == cfg["num_in_ch"] == self.nch
        if self.census is not None:
            k = "frames_tp" if self.conv_algo == _lib.CONV_DIRECT_THROUGHPUT else "frames_b1"
            self.census[k] = self.census.get(k, 0) + self.nb
        if h_in < 2 or w_in < 2:
            raise ValueError("SAVSR needs h, w >= 2")
        hp, wp = h_in + (h_in & 1), w_in + (w_in & 1)              # pad_spatial to even (savsr_arch.py:670-690)
        st = self._stream()
        sw, fw = cfg["slid_win"], cfg["fusion_win"]
        rw = self.rw
        if cfg["interval"] == 0:
            wins = self.buf("windows", T - sw + 1, hp, wp, rw)
            for b in range(self.nb):
                self._pack_windows(lq.data_ptr() + b * clip_bytes, wins.data_ptr() + b * self._bs(wins), T, h_in, w_in, hp, wp, st)
            # window q is centred at frame t = q + sw // 2
            win_b = win_f = lambda t: Src(wins, rw, rw, 0, float_off=(t - sw // 2) * hp * wp * rw, bs=self._bs(wins))
            T = self.iter_win
        else:
            # frame_sample (:638-659, :699): each direction walks its own sub-sequence of the clip -- gathered (a device copy of
            # iter_win frames) and packed into its own window buffer
            T = self.iter_win
            packs = []
            for tag, idx in (("f", self.fwd_idx), ("b", self.bwd_idx)):
                sel = self.buf("frames_" + tag, T, cin, h_in, w_in)
                for k, fi in enumerate(idx[:T]):
                    sel[k].copy_(lq[fi])
                wb = self.buf("windows_" + tag, T - sw + 1, hp, wp, rw)
                self._pack_windows(sel.data_ptr(), wb.data_ptr(), T, h_in, w_in, hp, wp, st)
                packs.append(wb)
            win_f = lambda t, wb=packs[0]: Src(wb, rw, rw, 0, float_off=(t - sw // 2) * hp * wp * rw)
            win_b = lambda t, wb=packs[1]: Src(wb, rw, rw, 0, float_off=(t - sw // 2) * hp * wp * rw)
        steps = T - sw + 1
        zero = self.buf("zero", hp, wp, nf)
        if self.nb == 1:
            zero.zero_()      # hidden state restarts from zero every window (savsr_arch.py:705-706)
        else:                 # (every clip's copy: the whole allocation behind the name)
            self._cur["raw"][zero.data_ptr()].zero_()
        hb = hf = self.full(zero)
        hpair = [self.buf(f"hpair{i}", hp, wp, 2 * nf) for i in range(steps)]   # cat(f2p[i], p2f[i]) of :721, written in place
        for idx in range(steps):                                                    # :708-719, both directions per launch
            cur_b, cur_f = T - 1 - sw // 2 - idx, idx + sw // 2
            hb, hf = self.windows_l1([("f2p_win", win_b(cur_b), hb, self.full(hpair[steps - 1 - idx], nf, 0), "f2p"),
                                      ("p2f_win", win_f(cur_f), hf, self.full(hpair[idx], nf, nf), "p2f")], hp, wp, scale)
        self.release(zero, *([wins] if cfg["interval"] == 0 else packs))             # (liveness: dead once the recurrence is through)
        # pyramid fusion (:616-618, :485-501, :721-722)
        level: List[Src] = [self.full(t) for t in hpair]
        for i in range(self.n_l2):
            u = f"h_win.{i}"
            ws = steps - 2 * i
            hfs = [self.full(self.buf(f"l2.{i}.hf{j}", hp, wp, nf)) for j in range(ws)]       # :488: ws independent convs, one launch
            self.conv_launch([self.conv_desc(f"{u}.conv_h.{j}", [level[j]], hfs[j], hp, wp, ACT_LRELU, 0.2) for j in range(ws)], "conv_h")
            self.release(*level)                         # this level's inputs (hpair at level 0) are dead
            nxt: List[Src] = []
            for j in range(ws - fw + 1):
                swf = hfs[j:j + fw]
                for k in range(cfg["w2_num_block"]):
                    prev = swf
                    swf = self.residual_block(f"{u}.blocks.{k}", swf, hp, wp, scale, True, f"l2.{i}.{j}.b{k}")
                    if k >= 1:
                        self.release(*prev)
                nxt.append(self.conv(u + ".merge", swf, self.full(self.buf(f"l2.{i}.o{j}", hp, wp, 2 * nf)), hp, wp))
                if cfg["w2_num_block"] >= 1:
                    self.release(*swf)
            self.release(*hfs)                           # (the windows of a level overlap: released once all of them are through)
            level = nxt
        align = self.conv("h_win_conv_h", [level[0]], self.full(self.buf("align", hp, wp, nf)), hp, wp, ACT_LRELU, 0.2)   # :723
        share = align
        hcur = align
        for g in range(cfg["n_resgroups"]):                                         # :728-732
            xin = hcur
            r = xin
            for k in range(cfg["n_resblocks"]):
                r = self.rcab(f"RG.{g}.residual_group.{k}.rcab", r, self.full(self.buf(f"rg.r{k & 1}", hp, wp, nf)), hp, wp, "rg")
            rg = self.conv(f"RG.{g}.conv", [r], self.full(self.buf("rg.out", hp, wp, nf)), hp, wp, res1=xin,
                           pool=(self.pool_buf(f"adapt.{g}.adapt", hp, wp, nf), 0, nf))      # OSAdapt's OSConv pools this tensor
            hcur = self.osadapt(g, rg, share, self.full(self.buf(f"rg.h{g & 1}", hp, wp, nf)), hp, wp, scale, pooled=True)
        hfeat = self.conv("conv_last", [hcur], self.full(self.buf("hfeat", hp, wp, nf)), hp, wp, res1=share)   # :733-734
        self.seal_buffers()                              # the LR buffer plan of this shape is final (align / hfeat / SATU buffers are never shared)
        H, W = get_hw(h_in, w_in, scale)
        return dict(align=align, hfeat=hfeat, wp=wp, h=h_in, w=w_in, H=H, W=W, **self._satu_outputs(H, W))

    def _pack_windows(self, lq_ptr: int, out_ptr: int, T: int, h: int, w: int, hp: int, wp: int, st: int) -> None:
        """Input windows of one clip (savsr_arch.py:448-454, :661-668, :670-690): the shipped 3-channel, 3-frame form through its own
        kernel, every other num_in_ch / slid_win through savsr_pack_windows_nch."""
        if self.nch == 3 and self.sw == 3:
            _lib.check(self.lib.savsr_pack_windows(lq_ptr, out_ptr, T, h, w, hp, wp, st), "savsr_pack_windows")
        else:
            _lib.check(self.lib.savsr_pack_windows_nch(lq_ptr, out_ptr, T, self.nch, self.sw, h, w, hp, wp, st), "savsr_pack_windows_nch")

    # ------------------------------------------------------------------ SATU -> tail, per form (`satu_form`; `form` = another form's for taps)
    _LRCAT = {"q": "satu.lrcat_tailq", "p27": "satu.lrcat_tail", "nf": "satu.lrcat_nf"}

    def _satu_lrcat(self, h: int, w: int, form: Optional[str] = None) -> torch.Tensor:
        """The LRcat buffer of a form's LR stage: the one spelling of its name and record (satu_lr / satu_nf_lr write it)."""
        form = form or self.satu_form
        return self.buf(self._LRCAT[form], h, w, self.satu_nf_rec if form == "nf" else _lib.SATU_LRCAT_TAIL)

    def _satu_outputs(self, H: int, W: int, form: Optional[str] = None) -> dict:
        """What a form's HR stage writes and its tail reads: q9 + seam, or p27 with tail_planes rows (the 27 planes -- 99.5 MB at 720x1280
        -- exist only where a form needs them)."""
        plane = self.hr_plane(H, W)
        if (form or self.satu_form) == "q":
            return dict(plane=plane, q9=self.sbuf("satu.q9", 9, plane), seam=self.sbuf("satu.seam", self.seam_floats(H, W)))
        return dict(plane=plane, p27=self.sbuf("satu.p27", self.tail_planes, plane))

    def _satu_lr_clip(self, c: dict, b: int = 0, form: Optional[str] = None) -> torch.Tensor:
        """LR stage of clip b of a launch sequence (crops of :737 via (row pitch, h, w)) -> its LRcat buffer."""
        form = form or self.satu_form
        if form == "nf":
            return self.satu_nf_lr(c["hfeat"], c["align"], c["wp"], c["h"], c["w"], b=b)
        return self.satu_lr(c["hfeat"], c["align"], c["wp"], c["h"], c["w"], tail_form=True, q=form == "q", b=b)

    def _satu_hr_clip(self, lrcat: torch.Tensor, c: dict, scale, b: int = 0, form: Optional[str] = None):
        """HR stage of clip b into the form's outputs (the row-summed form adds the tail's horizontal taps itself: 9 planes + seams)."""
        form = form or self.satu_form
        if form == "nf":
            self.satu_nf_hr(lrcat, c["h"], c["w"], scale, c["p27"], c["plane"], b=b)
        elif form == "q":
            self.satu_hr(lrcat, c["h"], c["w"], scale, c["q9"], c["plane"], tail_form=True, seam=c["seam"], b=b)
        else:
            self.satu_hr(lrcat, c["h"], c["w"], scale, c["p27"], c["plane"], tail_form=True, b=b)

    def _satu_clip(self, c: dict, scale, b: int = 0, form: Optional[str] = None):
        """LR then HR stage of clip b."""
        self._satu_hr_clip(self._satu_lr_clip(c, b, form), c, scale, b, form)

    def _satu_prepare(self, h: int, w: int, scale):
        """The HR stage on the form's own LRcat / output buffers, outside a capture: the SATU tables of (size, scale) and, where one is
        needed, the measured choice of the HR launch plan (the buffers' contents do not matter)."""
        c = dict(h=h, w=w)
        lrcat = self._satu_lrcat(h, w)
        c.update(self._satu_outputs(*get_hw(h, w, scale)))
        self._satu_hr_clip(lrcat, c, scale)

    def _tail_clip(self, c: dict, lq: torch.Tensor, out: torch.Tensor, b: int = 0):
        """What is left of :738-739 for clip b (lq [nb, T, nch, h, w] and out [nb, nch, H, W] contiguous): the nine shifted taps per colour,
        the tail bias, the bilinear residual."""
        nch, h, w, H, W = self.nch, c["h"], c["w"], c["H"], c["W"]
        T = lq.shape[-4]
        center = T // 2 if self.cfg["center_frame_idx"] is None else self.cfg["center_frame_idx"]
        cptr = lq.data_ptr() + 4 * (b * T + center) * nch * h * w          # unpadded centre frame (:696)
        optr = out.data_ptr() + 4 * b * nch * H * W
        tb, st = self.tail_b.data_ptr(), self._stream()
        if self.satu_form == "q":
            q9, seam = c["q9"], c["seam"]
            _lib.check(self.lib.savsr_tail_gather_q(q9.data_ptr() + b * self._bs(q9), c["plane"], seam.data_ptr() + b * self._bs(seam), seam.numel(),
                                                    tb, cptr, h, w, H, W, optr, st), "savsr_tail_gather_q")
            return
        p = c["p27"].data_ptr() + b * self._bs(c["p27"])
        if nch != 3:           # the 9 nch planes of the width-generic HR stage
            _lib.check(self.lib.savsr_tail_gather_nch(p, c["plane"], nch, tb, cptr, h, w, H, W, optr, st), "savsr_tail_gather_nch")
        else:
            _lib.check(self.lib.savsr_tail_gather(p, c["plane"], tb, cptr, h, w, H, W, optr, st), "savsr_tail_gather")

    def _stage_satu(self, c: dict, scale):
        with HipEngine._StageStream(self):
            return self._stage_satu_impl(c, scale)

    def _stage_satu_impl(self, c: dict, scale):
        """SATU in the tail-projected form (savsr_arch.py:315-376 with the channel contraction of :738 folded in), per clip of the launch
        sequence."""
        for b in range(self.nb):
            self._satu_clip(c, scale, b)

    def _stage_tail(self, c: dict, lq: torch.Tensor, out: torch.Tensor):
        with HipEngine._StageStream(self):
            return self._stage_tail_impl(c, lq, out)

    def _stage_tail_impl(self, c: dict, lq: torch.Tensor, out: torch.Tensor):
        for b in range(self.nb):
            self._tail_clip(c, lq, out, b)

    def _satu_standalone(self, c: dict, scale) -> torch.Tensor:
        """STAUpsample.forward as such ([64][H][W]; tests / taps only -- the product path never materialises it)."""
        o = self.sbuf("satu.out", self.nf, c["plane"])
        self.satu(c["hfeat"], c["align"], c["wp"], c["h"], c["w"], scale, o, c["plane"])
        return o[:, : c["H"] * c["W"]].view(self.nf, c["H"], c["W"])

    def forward_one(self, lq: torch.Tensor, scale, out: torch.Tensor, taps: Optional[dict] = None, throughput: bool = False):
        """Eager launch sequence.  lq: [T, c, h, w] fp32 contiguous on device (c = num_in_ch); out: [c, H, W] (or [nb, T, c, h, w] ->
        [nb, c, H, W]: nb clips of one (shape, scale) in one launch sequence).  throughput: the frame's flow (`_flow`) -- the latency flow
        unless asked otherwise, whatever ran on this engine before."""
        with self._frame(lq, throughput):
            assert self.nb == 1 or taps is None
            return self._forward_one(lq, scale, out, taps)

    def _forward_one(self, lq: torch.Tensor, scale, out: torch.Tensor, taps: Optional[dict] = None):
        self._select(lq.shape, scale)
        try:
            c = self._stage_body(lq, scale)
        except BaseException:
            self._abort_frame()
            raise
        self._satu_timed(lambda: self._stage_satu(c, scale))
        if taps is not None:                   # channel-last [hp][wp][64] tensors; SATU output planar
            taps["align_feat"] = c["align"].t
            taps["h_feat"] = c["hfeat"].t
            if self.satu_form != "nf":      # (STAUpsample's own output: a tap of the tuned 64-wide kernels only; the generic form leaves it out)
                taps["satu"] = self._satu_standalone(c, scale)
            if "p27" not in c:              # the 27-plane form beside the row-summed one the frame runs (taps only)
                c.update(self._satu_outputs(c["H"], c["W"], "p27"))
                self._satu_clip(c, scale, 0, "p27")
            taps["p27"] = c["p27"][:, : c["H"] * c["W"]].view(-1, c["H"], c["W"])      # (9 num_in_ch planes)
        self._stage_tail(c, lq, out)
        return out

    def _forward_graphed(self, lq: torch.Tensor, scale, out: torch.Tensor, throughput: bool = False):
        """hipGraph replay of the same launch sequence (three graphs: body | SATU | tail, so the SATU
        stage can be bracketed by HIP events).  The ~1400 launches of a frame cost ~11 us of host time
        each when issued from Python; captured once per (shape, scale) they replay in tens of us.
        throughput=True (several clips in flight on different streams): the convs are launched as
        SAVSR_CONV_DIRECT_THROUGHPUT -- the direct kernel's results bit for bit, its own captured graphs.  (Round 4: a launch's conv FORM --
        direct or Winograd-y -- depends on its tile count and on this mode (conv_launch), so a frame in throughput mode can differ from the
        one-clip flow by the two forms' rounding, ~1e-5; each mode is bitwise reproducible.)
        lq [nb, T, c, h, w] / out [nb, c, H, W]: nb clips of one (shape, scale) in ONE launch sequence (see `nb`), its own context and graphs."""
        with self._frame(lq, throughput):
            return self._forward_graphed_impl(lq, scale, out, throughput)

    def _frame(self, lq: torch.Tensor, throughput: bool):
        """What every frame passes through before its launches (eager, captured or replayed; never inside a capture): the fp16 images exist
        when the mode needs them, and the `with` block runs in the flow of lq's clips ([T, c, h, w] or [nb, T, c, h, w])."""
        self._ensure_precision()
        nb = int(lq.shape[0]) if lq.dim() == 5 else 1
        assert nb <= self.NB_MAX
        return self._flow(nb, throughput, int(lq.shape[-2]), int(lq.shape[-1]))

    @contextmanager
    def _flow(self, nb: int, throughput: bool, h: int, w: int):
        """The one owner of the flow state: inside the block `nb`, `form_nb` and `conv_algo` -- which decide the kernels a launch takes and the
        size of the buffers -- are those of a launch sequence of nb clips of h x w LR pixels; after it they are what they were before,
        exceptions included.  The two flows of a frame.
        Latency (one clip in flight, `net(lq)` with b = 1): 8-row direct conv tiles, Winograd-y from 200 tiles.
        Throughput (several clips in flight: b >= 2, forward_many): 16-row tiles, Winograd-y from 100 tiles, counted as if `clip_batch` clips
        shared every launch when the shape is eligible for batching (`form_nb`).  Each flow is bitwise reproducible and independent of the
        grouping; the two differ from each other by the conv forms' rounding (~1e-5)."""
        prev = self.nb, self.form_nb, self.conv_algo
        self.nb, self.form_nb, self.conv_algo = ((nb, HipEngine.clip_unit(self, h, w), _lib.CONV_DIRECT_THROUGHPUT) if throughput else
                                                 (nb, 1, _lib.CONV_DIRECT))          # (class-qualified: the host test runs this on a stub)
        try:
            yield
        finally:
            self.nb, self.form_nb, self.conv_algo = prev

    def _set_flow(self, lq: torch.Tensor, throughput: bool) -> None:
        """Select the flow of lq's clips and leave it selected, for stage functions called one by one outside a frame (tests, tools)."""
        with self._flow(self.nb, throughput, int(lq.shape[-2]), int(lq.shape[-1])):
            selected = self.form_nb, self.conv_algo
        self.form_nb, self.conv_algo = selected

    def clip_unit(self, h: int, w: int) -> int:
        """Clips of one (shape, scale) that share a launch sequence (see `nb`) for LR frames of h x w: `clip_batch` where the frame is small
        enough to be launch-latency-bound, 1 otherwise (and for clips sampled with an interval)."""
        return self.clip_batch if (self.cfg["interval"] == 0 and h * w <= self.clip_batch_max_px) else 1

    def _forward_graphed_impl(self, lq: torch.Tensor, scale, out: torch.Tensor, throughput: bool = False):
        sc = self._select(lq.shape, scale)
        if sc["graphs"] is None:
            sc["graphs"] = {}
        gk = self._graph_key(throughput)
        g = sc["graphs"].get(gk)
        if g is None:
            used = sc.setdefault("uses", {}).get(gk, 0)
            if used < self.capture_after:            # the context's first frames: eager (see capture_after)
                sc["uses"][gk] = used + 1
                self.host_stats["eager_frames"] += 1
                return self._forward_one(lq, scale, out)
            s_in = torch.empty_like(lq)
            s_out = torch.empty_like(out)
            s_in.copy_(lq)
            # Everything a capture cannot hold happens here, once per (size, scale): the SATU tables (host arithmetic, H2D copies,
            # one read-back of the offset range) and the measured choice of the HR launch plan, on this context's own LRcat / P
            # buffers (their contents do not matter: no control flow of the HR kernel depends on the feature values).  The kernels'
            # LDS attributes were set by savsr_prepare_device.  There is no eager run of the frame: the launch sequence is issued
            # exactly once, into the capture, and the buffers it names are allocated there (arena chunks from the graphs' pool).
            _t0 = time.perf_counter()
            self._satu_prepare(int(lq.shape[-2]), int(lq.shape[-1]), scale)
            # (no host synchronisation here: the capture stream waits for this one -- `_capture` --, and a plan that had to be MEASURED has
            # synchronised on its own events.  A sync per new context stalled the host behind the units already queued on this stream, 38 ms a
            # time with three streams in flight: 2.6 s of a 6.5 s cold pass of the YAML workflow, during which the other streams got nothing new.)
            _t1 = time.perf_counter()
            graphs = [torch.cuda.CUDAGraph() for _ in range(3)]
            ev = self.satu_events
            self.satu_events = None
            box = {}
            try:
                self._capture(graphs[0], None, lambda: box.update(c=self._stage_body(s_in, scale)))
                _t2 = time.perf_counter()
                self._capture(graphs[1], graphs[0].pool(), lambda: self._stage_satu(box["c"], scale))
                self._capture(graphs[2], graphs[0].pool(), lambda: self._stage_tail(box["c"], s_in, s_out))
            except BaseException:
                self._abort_frame()
                raise
            finally:
                self.satu_events = ev
            self._charge(sc, s_in.numel() * 4 + s_out.numel() * 4)
            _t3 = time.perf_counter()
            self.host_stats["captures"] += 1
            self.host_stats["plan_s"] += _t1 - _t0
            self.host_stats["capture_s"] += _t3 - _t1
            if self.knobs.profile_capture:
                print(f"[capture] {tuple(lq.shape)} x{scale}: plan {1e3 * (_t1 - _t0):.1f} ms, body {1e3 * (_t2 - _t1):.1f} ms "
                      f"(python launches {1e3 * box.get('t_launch', 0):.1f}), satu+tail {1e3 * (_t3 - _t2):.1f} ms", file=sys.stderr, flush=True)
            # The captured launches bake in the raw device pointers of this (size, scale)'s SATU tables (phase table, per-pixel
            # expansion, row / column index and coordinate arrays).  Replays never go through satu_axes(), so its LRU neither sees
            # them nor may it free them: the graph tuple owns a reference and the tables live exactly as long as the graph does.
            g = (s_in, s_out, graphs, self.satu_axes(lq.shape[-2], lq.shape[-1], scale))
            if g[3].get("ptab") is not None and not sc.get("ptab_charged"):
                self._charge(sc, g[3]["ptab"].numel() * 4)               # (the per-pixel table lives as long as a graph that names it)
                sc["ptab_charged"] = True
            sc["graphs"][gk] = g
        s_in, s_out, graphs = g[:3]
        s_in.copy_(lq)
        graphs[0].replay()
        self._satu_timed(graphs[1].replay)
        graphs[2].replay()
        out.copy_(s_out)
        return out

    def _satu_timed(self, fn) -> None:
        """fn() = the SATU stage of a launch sequence, launched or replayed -- between two HIP events where bench.py asks for them."""
        if self.satu_events is None:
            return fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        self.satu_events.append((ev0, ev1, self.nb))      # (start, end, clips whose SATU stages lie between them)

    def _capture(self, graph: "torch.cuda.CUDAGraph", pool, fn) -> None:
        """Record fn()'s launches into `graph` on a side stream.  This is torch.cuda.graph() without its entry ritual
        (device-wide synchronize + gc.collect() + empty_cache() per graph: tens of ms, and the emptied cache turns the next
        shape's allocations into fresh hipMallocs) -- a YAML sweep captures one graph set per (folder, scale, stream)."""
        cur = torch.cuda.current_stream()
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream(device=self.dev)
        cap = self._cap_stream
        cap.wait_stream(cur)
        # No cyclic garbage collection while a capture is open: a collector run triggered by the ~330 descriptor allocations of a frame could
        # finalise some OTHER object that owns device memory or a graph (an engine of an earlier test module, a dropped model), and freeing
        # device memory inside a capture aborts the process.  Objects that die by reference count are ours and die outside captures.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(cap):
                if pool is None:
                    graph.capture_begin()
                else:
                    graph.capture_begin(pool=pool)
                try:
                    fn()
                finally:
                    graph.capture_end()
        finally:
            if gc_was_on:
                gc.enable()
        cur.wait_stream(cap)

    def streams_for(self, px: float) -> int:
        """HIP streams (launch units in flight) for frames of `px` LR pixels on average."""
        return self.n_streams_large if px >= self.streams_large_px else self.n_streams

    def _fan_out(self, units: list, px: float, run) -> None:
        """Deal launch units round-robin over ns HIP streams: unit u is issued by run(engine, unit) under stream u % ns with that stream's
        engine (this one or a sibling).  ns = `streams_for(px)` for LR frames of `px` pixels on average, at most one per unit; 1 with
        SAVSR_GRAPHS=0 (diagnostics: one unit after the other).  The streams first wait for the caller's stream, which then waits for all of
        them.  A tensor run returns -- allocated under its stream, for the caller -- is record_stream'ed to the caller's stream: its block
        is not recycled on the side stream while the caller's still reads it."""
        self._ensure_precision()      # (on the caller's stream, which every unit's stream waits for: the engines share the fp16 images)
        ns = min(self.streams_for(px), len(units)) if self.use_graphs else 1
        while len(self._siblings) < ns - 1:
            self._siblings.append(self.clone_for_stream())
        while len(self._streams) < ns:
            self._streams.append(torch.cuda.Stream(device=self.dev))
        engines, streams = ([self] + self._siblings)[:ns], self._streams[:ns]
        for e in engines:             # (bench.py: the SATU stages of every stream's units are timed)
            e.satu_events = self.satu_events
        cur = torch.cuda.current_stream()
        for s in streams:
            s.wait_stream(cur)
        for u, unit in enumerate(units):
            with torch.cuda.stream(streams[u % ns]):
                made = run(engines[u % ns], unit)
            if made is not None:
                made.record_stream(cur)
        for s in streams:
            cur.wait_stream(s)

    def _run_unit(self, lq_u: torch.Tensor, scale, out_u: torch.Tensor) -> None:
        """One launch unit of the throughput flow on this engine under the current stream: lq_u [nb, T, c, h, w] fp32 contiguous -> out_u
        [nb, c, H, W].  One clip runs as [T, c, h, w] -> [c, H, W] (the one-clip context and graphs); SAVSR_GRAPHS=0: the same flow, eagerly."""
        if lq_u.shape[0] == 1:
            lq_u, out_u = lq_u[0], out_u[0]
        (self._forward_graphed if self.use_graphs else self.forward_one)(lq_u, scale, out_u, throughput=True)

    def _input(self, t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        """An input as the kernels read it (`dtype`, contiguous); it has to be on the engine's device already."""
        if t.device != self.dev:
            raise RuntimeError(f"input on {t.device}, engine on {self.dev}")
        return t.to(dtype).contiguous()

    def forward_many(self, items, ensemble: bool = False) -> List[torch.Tensor]:
        """A stream of independent clips of MIXED shapes / scales (BASELINE config 5): items = [(lq [T, c, h, w], (sh, sw))] ->
        [out [c, H, W]] (c = num_in_ch).  Launch unit u (`many_units`) runs on HIP stream u % ns with that stream's sibling engine (`_fan_out`), so
        small clips (whose ~360 launches are latency-bound) overlap.  Every clip's result is that of the throughput flow (`_flow`) whatever
        the grouping: forward_many(items)[i] == forward_many([items[i]])[0] bit for bit; against the one-clip latency flow of `forward` it
        agrees to the conv forms' rounding (~1e-5) where a launch takes another form.
        ensemble=True: every clip is the self-ensemble of its 8 variants (`_ensemble`)."""
        items = [(self._input(lq), sc) for lq, sc in items]
        if ensemble:
            clips = [(lq, list(range(int(lq.shape[0]))), tuple(sc),
                      torch.empty((self.nch,) + get_hw(lq.shape[-2], lq.shape[-1], sc), device=self.dev, dtype=torch.float32)) for lq, sc in items]
            self._ensemble(clips, False)
            return [cl[3] for cl in clips]
        # (a lone clip, or SAVSR_STREAMS=1, takes the throughput flow too: what forward_many returns for a clip does not depend on how many
        # came with it or on how many streams carry them; SAVSR_GRAPHS=0 issues that flow eagerly, one clip per unit)
        units = many_units([(lq.shape, sc) for lq, sc in items], self.clip_unit if self.use_graphs else (lambda h, w: 1), self.clip_batch)
        outs: List[Optional[torch.Tensor]] = [None] * len(items)

        def run(eng: "HipEngine", unit: List[int]):
            sc = items[unit[0]][1]
            lqb = torch.stack([items[i][0] for i in unit], 0) if len(unit) > 1 else items[unit[0]][0][None]          # (a lone clip: no copy)
            outb = torch.empty((len(unit), self.nch) + get_hw(lqb.shape[-2], lqb.shape[-1], sc), device=self.dev, dtype=torch.float32)
            eng._run_unit(lqb, sc, outb)
            for j, i in enumerate(unit):
                outs[i] = outb[j]
            return outb
        self._fan_out(units, sum(lq.shape[-2] * lq.shape[-1] for lq, _ in items) / max(1, len(items)), run)
        return outs

    def forward_video(self, frames: torch.Tensor, windows: List[List[int]], scale, spec: Optional[VideoSpec] = None,
                      ensemble: bool = False) -> torch.Tensor:
        """The sequence path (SAVSR.upscale_video, VideoUpscaler): frames on the device, as `spec` (a video.VideoSpec, taken on trust:
        there is no invalid one) says -- packed, [N, h, w, c] uint8 or [N, c, h, w] fp32, or planar, [N, spec.inp.frame_bytes(h, w)] uint8
        with (h, w) = spec.size; windows[i] = the num_frame frame indices of output frame i in clip order (harness.window_indices) ->
        [len(windows), c, H, W] fp32, [len(windows), H, W, c] uint8 (tensor2img(x, rgb2bgr=False) per frame) or
        [len(windows), spec.out.frame_bytes(H, W)] uint8 planar frames (`spec.out_kind`).  spec=None: packed frames in, fp32 out.
        Launch units and streams are forward_many's (up to `clip_unit` consecutive windows per unit, balanced; units dealt round-robin over
        `streams_for` streams; throughput flow), so frame i equals forward_many on the gathered window i bit for bit.  A unit's windows are
        gathered from `frames` into a unit-sized fp32 clip batch on the unit's stream and its result is quantised there; nothing is gathered
        or converted on the host.  The two sides differ in one gather and one quantiser each, chosen once:
            packed           savsr_video_gather_u8 / _f32                        savsr_video_quantize_u8
            planar YUV       savsr_video_gather_yuvs: any layout, depth,          savsr_video_quantize_yuvs
                             colour space and siting -> fp32 planar RGB
            luma-only        savsr_video_gather_luma: the Y plane of YUV or       savsr_video_quantize_luma: into the Y plane of the
            (spec.luma)      grey-scale frames, c = 1                             output frames, or of [n, H, W, 1] uint8
        With spec.dither the quantiser is the entry's `_d` form with the dither's id (savsr_amd/dither.py is the specification); without
        one, the entries above, as ever.
        On the luma-only path the U and V planes of planar output frames never pass the network: `_resample_chroma` fills them first, on
        the caller's stream (savsr_amd/yuv.py "Luma-only checkpoints" is the specification).
        ensemble=True: frame i is the self-ensemble of window i (`_ensemble`, gathered by savsr_ensemble_gather_*).  Planar frames are
        converted once to fp32 (the same gather with the identity list) and take the fp32 path; the merge quantises packed uint8 itself,
        every other quantiser runs after the fp32 merge, the packed one too when it dithers.  Chroma never enters the ensemble of a luma-only network."""
        if spec is None:
            spec = video_spec(self.nch)
        elif not isinstance(spec, VideoSpec):
            raise ValueError(f"spec must be a savsr_amd.video.VideoSpec (video.video_spec builds one), got {type(spec).__name__}")
        src, dst, kind, luma = spec.inp, spec.out, spec.out_kind, spec.luma
        if src.planar:
            h, w = spec.size
            fb = src.frame_bytes(h, w)
            if frames.dtype != torch.uint8 or frames.dim() != 2 or int(frames.shape[1]) != fb:
                raise ValueError(f"{layout_name(src.layout)} frames of {h} x {w} are [N, {fb}] uint8, got {frames.dtype} {tuple(frames.shape)}")
            u8, N, c = True, int(frames.shape[0]), 1 if luma else 3
        else:
            u8, N, c, h, w = _frames_layout(frames)
        frames = self._input(frames, torch.uint8 if u8 else torch.float32)
        T = self.cfg["num_frame"]
        if c != self.nch:
            raise ValueError(f"frames have {c} channels, the network num_in_ch = {self.nch}")
        for win in windows:
            if len(win) != T or min(win) < 0 or max(win) >= N:
                raise ValueError(f"window {win}: {T} indices in [0, {N}) expected")
        H, W = get_hw(h, w, scale)
        n = len(windows)
        if kind == "planar":
            out = torch.empty(n, dst.frame_bytes(H, W), device=self.dev, dtype=torch.uint8)
        else:
            out = (torch.empty(n, H, W, c, device=self.dev, dtype=torch.uint8) if kind == "uint8" else
                   torch.empty(n, c, H, W, device=self.dev, dtype=torch.float32))
        if n == 0:
            return out
        if T > _lib.VIDEO_MAX_SLOTS:
            raise ValueError(f"num_frame = {T}: the window gather takes at most {_lib.VIDEO_MAX_SLOTS} frames per launch")
        idx_t = _lib.C.c_int32
        did = dither_id(spec.dither)          # 0: the quantisers as they were
        if luma:
            def gather(idx, to, st):
                _lib.check(self.lib.savsr_video_gather_luma(frames.data_ptr(), N, fb, h, w, src.depth, (idx_t * len(idx))(*idx), len(idx), to.data_ptr(), st),
                           "savsr_video_gather_luma")
        elif src.planar:
            colour, chroma, siting = _yuv_ids(src)

            def gather(idx, to, st):
                _lib.check(self.lib.savsr_video_gather_yuvs(frames.data_ptr(), N, h, w, (idx_t * len(idx))(*idx), len(idx), colour, src.depth, chroma,
                                                            siting, to.data_ptr(), st), "savsr_video_gather_yuvs")
        else:
            fn = self.lib.savsr_video_gather_u8 if u8 else self.lib.savsr_video_gather_f32

            def gather(idx, to, st):
                _lib.check(fn(frames.data_ptr(), N, c, h, w, (idx_t * len(idx))(*idx), len(idx), to.data_ptr(), st), "savsr_video_gather")
        if luma:
            od, ofb = (dst.depth, dst.frame_bytes(H, W)) if kind == "planar" else (8, H * W)          # (uint8: Y planes with nothing between them)

            def quantize_frames(x, to, nb, st):
                if did:
                    _lib.check(self.lib.savsr_video_quantize_luma_d(x.data_ptr(), nb, H, W, od, did, to.data_ptr(), ofb, st), "savsr_video_quantize_luma_d")
                else:
                    _lib.check(self.lib.savsr_video_quantize_luma(x.data_ptr(), nb, H, W, od, to.data_ptr(), ofb, st), "savsr_video_quantize_luma")
        elif kind == "planar":
            out_colour, out_chroma, out_siting = _yuv_ids(dst)

            def quantize_frames(x, to, nb, st):
                if did:
                    _lib.check(self.lib.savsr_video_quantize_yuvs_d(x.data_ptr(), nb, H, W, out_colour, dst.depth, out_chroma, out_siting, did,
                                                                    to.data_ptr(), st), "savsr_video_quantize_yuvs_d")
                else:
                    _lib.check(self.lib.savsr_video_quantize_yuvs(x.data_ptr(), nb, H, W, out_colour, dst.depth, out_chroma, out_siting, to.data_ptr(), st),
                               "savsr_video_quantize_yuvs")
        else:
            def quantize_frames(x, to, nb, st):
                if did:
                    _lib.check(self.lib.savsr_video_quantize_u8_d(x.data_ptr(), nb, c, H, W, did, to.data_ptr(), st), "savsr_video_quantize_u8_d")
                else:
                    _lib.check(self.lib.savsr_video_quantize_u8(x.data_ptr(), nb, c, H, W, to.data_ptr(), st), "savsr_video_quantize_u8")

        def quantize(x, to, st):
            for a in range(0, int(x.shape[0]), 65535):          # (the entries take 1 .. 65535 frames)
                nb = min(65535, int(x.shape[0]) - a)
                quantize_frames(x[a:a + nb], to[a:a + nb], nb, st)
        if luma and kind == "planar" and dst.yuv:
            self._resample_chroma(frames, windows, out, src, dst, h, w, H, W)
        if ensemble:
            st = torch.cuda.current_stream().cuda_stream
            if src.planar:
                f32 = torch.empty(N, c, h, w, device=self.dev, dtype=torch.float32)
                for a in range(0, N, _lib.VIDEO_MAX_SLOTS):
                    gather(list(range(a, min(N, a + _lib.VIDEO_MAX_SLOTS))), f32[a:], st)
                frames = f32
            fused = kind == "uint8" and not luma and spec.dither is None          # the merge quantises packed uint8 itself (undithered)
            merged = out if kind == "float" or fused else torch.empty(n, c, H, W, device=self.dev, dtype=torch.float32)
            self._ensemble([(frames, win, tuple(scale), merged[i]) for i, win in enumerate(windows)], fused)
            if merged is not out:
                quantize(merged, out, st)
            return out

        def run(eng: "HipEngine", unit: Tuple[int, int]):
            i0, i1 = unit
            nb = i1 - i0
            st = torch.cuda.current_stream().cuda_stream
            lqb = torch.empty(nb, T, c, h, w, device=self.dev, dtype=torch.float32)
            gather([f for win in windows[i0:i1] for f in win], lqb, st)
            o = out[i0:i1] if kind == "float" else torch.empty(nb, c, H, W, device=self.dev, dtype=torch.float32)
            eng._run_unit(lqb, scale, o)
            if kind != "float":
                quantize(o, out[i0:i1], st)
        # (SAVSR_GRAPHS=0: forward_many's eager flow, one window per unit)
        self._fan_out(video_units(n, T, self.clip_unit(h, w) if self.use_graphs else 1), h * w, run)
        return out

    def _chroma_tables(self, h: int, w: int, H: int, W: int, lay: str, out_lay: str, siting: Optional[str], out_siting: Optional[str]):
        """yuv.chroma_tables on the device, cached per (h, w, H, W, layouts, sitings): ((ymin, ysize, wy, taps_y), (xmin, xsize, wx, taps_x)).
        One entry per distinct key, a few KB each, kept for the engine's life: a video has one key; a caller that streams many distinct
        shapes through one engine grows it by that much."""
        key = (h, w, H, W, lay, out_lay, siting, out_siting)
        t = self._luma_tables.get(key)
        if t is None:
            from .yuv import chroma_tables
            t = tuple((torch.from_numpy(a).to(self.dev), torch.from_numpy(b).to(self.dev), torch.from_numpy(np.ascontiguousarray(c)).to(self.dev),
                       int(c.shape[1])) for a, b, c in chroma_tables(h, w, H, W, lay, out_lay, siting, out_siting))
            self._luma_tables[key] = t
        return t

    def _resample_chroma(self, frames: torch.Tensor, windows: List[List[int]], out: torch.Tensor, src, dst, h: int, w: int, H: int, W: int) -> None:
        """The U and V planes of the luma-only path's output frames, on the caller's stream: output frame i takes them from its own input
        frame, the centre of window i, resampled to the output's layout and depth at the network's scale (savsr_video_resample_chroma with
        `_chroma_tables`); runs of consecutive centres share a launch, one per plane."""
        T, n = self.cfg["num_frame"], len(windows)
        (ym, ys, wy, ty), (xm, xs, wx, tx) = self._chroma_tables(h, w, H, W, src.layout, dst.layout, src.siting, dst.siting)
        (ch, cw), (cH, cW) = chroma_hw(h, w, src.layout), chroma_hw(H, W, dst.layout)
        fb, ofb = src.frame_bytes(h, w), dst.frame_bytes(H, W)
        si, so = (1 if src.depth == 8 else 2), (1 if dst.depth == 8 else 2)
        st = torch.cuda.current_stream().cuda_stream
        centres = [win[T // 2] for win in windows]
        a = 0
        while a < n:
            b = a + 1
            while b < n and centres[b] == centres[b - 1] + 1 and b - a < 65535:
                b += 1
            for plane in range(2):
                _lib.check(self.lib.savsr_video_resample_chroma(
                    frames[centres[a]:].data_ptr(), b - a, fb, (h * w + plane * ch * cw) * si, ch, cw, src.depth, out[a:].data_ptr(), ofb,
                    (H * W + plane * cH * cW) * so, cH, cW, dst.depth, ym.data_ptr(), ys.data_ptr(), wy.data_ptr(), ty, xm.data_ptr(),
                    xs.data_ptr(), wx.data_ptr(), tx, st), "savsr_video_resample_chroma")
            a = b

    def forward(self, lq: torch.Tensor, scale, taps: Optional[dict] = None, ensemble: bool = False) -> torch.Tensor:
        """lq: [b, T, c, h, w] -> [b, c, H, W], c = num_in_ch (savsr_arch.py:692-742).  ensemble=True: every clip is the self-ensemble of its
        8 variants (`_ensemble`; taps are single-pass diagnostics and refused with it)."""
        if ensemble and taps is not None:
            raise ValueError("taps are single-pass diagnostics: switch the self-ensemble off to collect them")
        lq = self._input(lq)
        b, t, c, h, w = lq.shape
        if t != self.cfg["num_frame"] or c != self.nch:
            raise ValueError(f"expected lq [b, {self.cfg['num_frame']}, {self.nch}, h, w] (num_frame, num_in_ch), got {tuple(lq.shape)}")
        H, W = get_hw(h, w, scale)
        out = torch.empty(b, self.nch, H, W, device=self.dev, dtype=torch.float32)
        if ensemble:
            frames = lq.view(b * t, c, h, w)
            self._ensemble([(frames, list(range(i * t, (i + 1) * t)), tuple(scale), out[i]) for i in range(b)], False)
            return out
        if b >= 2 and self.n_streams >= 2 and self.use_graphs and taps is None:
            # clips are independent (no cross-clip state, savsr_arch.py:705-706): keep n_streams of them in flight on separate HIP streams so one
            # clip's load/store-bound kernel phases overlap another's MFMA phases ... and up to `clip_unit` consecutive clips per launch sequence
            # (see `nb`): the batch shares one (shape, scale).  Units: `chunk_units`, contiguous slices of the batch (no copy)
            self._fan_out(chunk_units(b, self.clip_unit(h, w)), h * w, lambda eng, u: eng._run_unit(lq[u[0]:u[1]], scale, out[u[0]:u[1]]))
            return out
        for i in range(b):      # the latency flow; samples are independent (OSConv groups=b, savsr_arch.py:166-167)
            if self.use_graphs and taps is None:
                self._forward_graphed(lq[i], scale, out[i])
            else:
                self.forward_one(lq[i], scale, out[i], taps if i == 0 else None, throughput=False)
        return out

    # ------------------------------------------------------------------ self-ensemble (SAVSR.set_self_ensemble)
    ENSEMBLE_CLIPS = 8          # clips whose 8 variants go through one forward_many call (64 outputs alive at a time)

    @staticmethod
    def ensemble_plan(h: int, w: int, scale) -> List[Tuple[Tuple[int, int], Tuple[float, float]]]:
        """Variant k = 0 .. 7 of an h x w clip at (sh, sw): (LR size, scale) the network runs it at.  Bits: k & 1 flips the width, k >> 1 & 1
        the height, k >> 2 transposes -- a transposed clip runs at the swapped scale (sw, sh), so its output is the [W, H] transpose of the
        plain [H, W] one (get_hw is symmetric under the swap)."""
        sh, sw = float(scale[0]), float(scale[1])
        return [((w, h), (sw, sh)) if k >> 2 else ((h, w), (sh, sw)) for k in range(8)]

    def _ensemble(self, clips, out_u8: bool) -> None:
        """Geometric self-ensemble of independent clips.  clips = [(frames, window, (sh, sw), out)]: frames [N, h, w, c] uint8 or [N, c, h, w]
        fp32 on the device, window = the num_frame frame indices of the clip, out = [c, H, W] fp32 or (out_u8) [H, W, c] uint8.
        Each clip is gathered in its 8 variants (savsr_ensemble_gather_*, on this stream), the variants of up to ENSEMBLE_CLIPS clips run as
        ONE forward_many batch -- its grouping puts the 4 plain variants of a small clip in one launch sequence and the 4 transposed ones in
        another, large frames run 8 units -- and every clip's 8 outputs are merged (savsr_ensemble_merge, fused quantisation for uint8).
        Variant k's output is forward_many([T_k(clip)], [s_k])[0] bit for bit.  The merge runs on this stream after forward_many has made it
        wait for every unit's stream (events, no device sync); the outputs were record_stream'ed to it there.  The gathered clips are
        allocated on this stream and read on the unit streams, which it has waited for before it frees them."""
        T = self.cfg["num_frame"]
        st = torch.cuda.current_stream().cuda_stream
        for g0 in range(0, len(clips), self.ENSEMBLE_CLIPS):
            group = clips[g0:g0 + self.ENSEMBLE_CLIPS]
            items = []
            for frames, win, sc, _ in group:
                u8, N, c, h, w = _frames_layout(frames)
                if c != self.nch or len(win) != T:
                    raise ValueError(f"ensemble clip of {len(win)} frames x {c} channels: num_frame = {T}, num_in_ch = {self.nch} expected")
                gather = self.lib.savsr_ensemble_gather_u8 if u8 else self.lib.savsr_ensemble_gather_f32
                idx = (_lib.C.c_int32 * T)(*win)
                for k, ((hk, wk), sk) in enumerate(self.ensemble_plan(h, w, sc)):
                    lq = torch.empty(T, c, hk, wk, device=self.dev, dtype=torch.float32)
                    _lib.check(gather(frames.data_ptr(), N, c, h, w, idx, T, k, lq.data_ptr(), st), "savsr_ensemble_gather")
                    items.append((lq, sk))
            res = self.forward_many(items)
            for j, (_, _, sc, out) in enumerate(group):
                outs = res[8 * j: 8 * j + 8]
                c, H, W = (int(v) for v in outs[0].shape)
                ptrs = [o.data_ptr() for o in outs]
                base = min(ptrs)
                offs = (_lib.C.c_int64 * 8)(*[(p - base) // 4 for p in ptrs])
                _lib.check(self.lib.savsr_ensemble_merge(base, offs, c, H, W, int(out_u8), out.data_ptr(), st), "savsr_ensemble_merge")


def balanced_units(n: int, cap: int) -> List[Tuple[int, int]]:
    """[start, end) ranges of n items in the fewest units of at most `cap` items, their sizes as even as possible, larger ones first:
    10 items at cap 3 -> 3 + 3 + 2 + 2, not 3 + 3 + 3 + 1 (a lone clip would need a capture of its own)."""
    k = -(-n // cap)
    units, a = [], 0
    for u in range(k):
        m = n // k + (1 if u < n % k else 0)
        units.append((a, a + m))
        a += m
    return units


def chunk_units(n: int, cap: int) -> List[Tuple[int, int]]:
    """`forward`'s launch units: consecutive [start, end) chunks of `cap` clips, not balanced (16 at 4 -> 4 + 4 + 4 + 4, 10 at 4 -> 4 + 4 + 2)."""
    return [(a, min(a + cap, n)) for a in range(0, n, cap)]


def many_units(clips, clip_unit, clip_batch: int) -> List[List[int]]:
    """`forward_many`'s launch units (lists of clip indices) for clips = [(shape, (sh, sw))]: the clips that may share a launch sequence
    (clip_unit(h, w) > 1) grouped by (shape, scale), every group cut into balanced units of at most `clip_batch`; every other clip a
    group of its own; the units ordered by their first clip."""
    groups: Dict[object, List[int]] = {}
    for i, (shape, sc) in enumerate(clips):
        groups.setdefault((tuple(shape), float(sc[0]), float(sc[1])) if clip_unit(shape[-2], shape[-1]) > 1 else i, []).append(i)
    return sorted((idxs[a:b] for idxs in groups.values() for a, b in balanced_units(len(idxs), clip_batch)), key=lambda u: u[0])


def video_units(n: int, T: int, cb: int) -> List[Tuple[int, int]]:
    """`forward_video`'s launch units: balanced ranges of at most `cb` consecutive windows of T frames that fit one gather launch."""
    return balanced_units(n, max(1, min(cb, _lib.VIDEO_MAX_SLOTS // T)))


def _yuv_ids(side) -> Tuple[int, int, int]:
    """(colour space, chroma layout, siting) of a planar YUV side (video.Side) as the C ABI numbers them: the positions in yuv.COLOURS and
    yuv.CHROMAS; the siting's position in yuv.SITINGS plus one, 0 = not modelled."""
    return COLOURS.index(side.colour), CHROMAS.index(side.layout), 0 if side.siting is None else SITINGS.index(side.siting) + 1


def _frames_layout(frames: torch.Tensor) -> Tuple[bool, int, int, int, int]:
    """(uint8?, N, c, h, w) of a frame stack: [N, h, w, c] uint8 or [N, c, h, w] float."""
    N, a, b, d = (int(v) for v in frames.shape)
    return (True, N, d, a, b) if frames.dtype == torch.uint8 else (False, N, a, b, d)
