"""Case table of the num_in_ch / slid_win goldens, shared by tools/gen_golden_channels.py and tests/test_channels.py /
test_gpu_channels.py."""

# (name, ctor kwargs, h, w, scale); goldens: tools/gen_golden_channels.py -> tests/golden/channels_outputs.npz
CHANNEL_CASES = [
    ("c1_nf64", dict(num_in_ch=1), 13, 17, (2.7, 3.3)),                                             # odd LR size, asymmetric scale
    ("c1_nf32_t9_i1", dict(num_in_ch=1, num_feat=32, num_frame=9, interval=1), 10, 12, (4, 4)),     # frame sampling, even centre index
    ("c2_nf32", dict(num_in_ch=2, num_feat=32), 11, 14, (3.5, 2)),
    ("c2_nf64_t7_i1", dict(num_in_ch=2, num_frame=7, interval=1), 12, 14, (2, 3)),                  # frame sampling, odd centre index
    ("sw5_t5_nf64", dict(num_frame=5, slid_win=5), 12, 13, (2.5, 3.0)),                             # tuned SATU, 15-channel windows
    ("sw7_t7_fw7", dict(num_frame=7, slid_win=7, fusion_win=7), 10, 11, (3, 2.5)),                  # 21 channels: 32-float windows
    ("c1_t5_sw5", dict(num_in_ch=1, num_frame=5, slid_win=5), 9, 12, (1.5, 4)),
    ("sw5_nf32_t9_i1", dict(num_feat=32, num_frame=9, interval=1, slid_win=5), 10, 12, (2.5, 2.5)),
]
