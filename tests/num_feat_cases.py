"""Case table of the num_feat = 32 goldens, shared by tools/gen_golden_num_feat.py and tests/test_num_feat.py / test_gpu_num_feat.py."""

# (name, ctor kwargs, h, w, scale); goldens: tools/gen_golden_num_feat.py -> tests/golden/num_feat_outputs.npz
NUM_FEAT_CASES = [
    ("nf32_t7", dict(num_feat=32), 13, 17, (2.7, 3.3)),                            # odd LR size, asymmetric non-integer scale
    ("nf32_t5", dict(num_feat=32, num_frame=5), 11, 14, (3.5, 2)),                 # 5 frames: no pyramid level
    ("nf32_t9_i1", dict(num_feat=32, num_frame=9, interval=1), 10, 12, (4, 4)),    # frame sampling, even centre index
]
