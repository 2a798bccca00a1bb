"""Case table of the sequence-path goldens (SAVSR.upscale_video), shared by tools/gen_golden_video.py and tests/test_video.py /
test_gpu_video.py."""

PADDINGS = ("replicate", "reflection", "reflection_circle", "circle")
# generate_frame_indices lists in the fixture: every mode, num_frame in INDEX_NUM_FRAMES, video lengths 1 .. INDEX_MAX_N (the lengths too
# short for a mode included: their lists reach outside the video, which is what upscale_video refuses)
INDEX_NUM_FRAMES = (5, 7, 9)
INDEX_MAX_N = 12

# (name, ctor kwargs, N, h, w, scale, padding); the reference SAVSR run per window on synth_clip(N, c, h, w, seed=7)[0] with
# synth_state_dict(seed=3); goldens: tools/gen_golden_video.py -> tests/golden/video_outputs.npz (sr [N, c, H, W])
VIDEO_CASES = [(f"t7_{p}", {}, 7, 8, 10, (2.5, 3.0), p) for p in PADDINGS] + [
    ("c1_nf32", dict(num_in_ch=1, num_feat=32), 6, 9, 14, (2.5, 3.0), "reflection"),          # width-generic SATU, one channel
    ("t7_i1", dict(interval=1), 6, 8, 11, (2.0, 3.0), "replicate"),                           # frame sampling
]
VIDEO_SEED, WEIGHT_SEED = 7, 3
