"""Test option files in the reference's YAML layout must parse: a sample, and files of the shipped YAMLs'
42 datasets (workloads.YAML_SCALES)."""
import os

import pytest

import savsr_amd
from savsr_amd.options import parse_test_options, yaml_load

SAMPLE = """
name: test_SAVSR_sample
model_type: ASVSRModel
num_gpu: 1
manual_seed: 0
datasets:
  test_01:
    name: Vid4_x4
    type: ASVideoTestDataset
    dataroot_gt: datasets/Vid4/GT
    io_backend:
      type: disk
    cache_data: false
    num_frame: 7
    padding: reflection
    use_arbitrary_scale_downsampling: true
    downsampling_scale: !!python/tuple [1.5, 4]
    downsampling_mode: torch
network_g:
  type: SAVSR
  num_in_ch: 3
  num_feat: 64
  num_frame: 7
  slid_win: 3
  fusion_win: 5
  interval: 0
  w1_num_block: 4
  w2_num_block: 2
  n_resgroups: 4
  n_resblocks: 8
  center_frame_idx: ~
path:
  pretrain_network_g: experiments/pretrained_models/SAVSR/savsr_best.pth
  strict_load_g: true
  resume_state: ~
val:
  save_img: true
  suffix: ~
  metrics:
    psnr_y:
      type: calculate_psnr
      crop_border: 0
      test_y_channel: true
    ssim_y:
      type: calculate_ssim
      crop_border: 0
      test_y_channel: true
"""


def _check(opt):
    ds = list(opt["datasets"].values())
    assert all(isinstance(d["downsampling_scale"], tuple) and len(d["downsampling_scale"]) == 2 for d in ds)
    assert all(d["phase"] == "test" for d in ds)
    assert opt["network_g"]["center_frame_idx"] is None and opt["path"]["resume_state"] is None
    net = savsr_amd.build_network(opt["network_g"])
    assert type(net).__name__ == "SAVSR"
    for m in opt["val"]["metrics"].values():
        assert m["type"] in savsr_amd.METRIC_REGISTRY
    assert opt["path"]["visualization"].endswith(os.path.join(opt["name"], "visualization"))


def test_sample_yaml():
    opt = parse_test_options(SAMPLE)
    assert opt["datasets"]["test_01"]["downsampling_scale"] == (1.5, 4)
    _check(opt)


def _scale_list_yaml(tmp_path, dataset):
    """A test option file in the shipped YAMLs' layout: the SAMPLE's settings with one dataset per scale of
    workloads.YAML_SCALES (42: x4.0 ... x1.1 and the 12 asymmetric pairs), written to a file."""
    from savsr_amd.utils import workloads
    head, rest = SAMPLE.split("datasets:\n", 1)
    tail = rest[rest.index("network_g:"):]
    blocks = []
    for i, (sh, sw) in enumerate(workloads.YAML_SCALES, 1):
        blocks.append(f"""  test_{i:02d}:
    name: {dataset}_x{sh}_{sw}
    type: ASVideoTestDataset
    dataroot_gt: datasets/{dataset}/GT
    io_backend:
      type: disk
    cache_data: false
    num_frame: 7
    padding: reflection
    use_arbitrary_scale_downsampling: true
    downsampling_scale: !!python/tuple [{sh}, {sw}]
    downsampling_mode: torch
""")
    text = head.replace("test_SAVSR_sample", f"test_SAVSR_{dataset}_asBI") + "datasets:\n" + "".join(blocks) + tail
    path = tmp_path / f"test_SAVSR_{dataset}_asBI.yml"
    path.write_text(text)
    return str(path), workloads.YAML_SCALES


@pytest.mark.parametrize("dataset", ["Vid4", "UDM10"])
def test_scale_list_yaml_parses(tmp_path, dataset):
    path, scales = _scale_list_yaml(tmp_path, dataset)
    opt = parse_test_options(path)
    assert len(opt["datasets"]) == 42
    assert [d["downsampling_scale"] for d in opt["datasets"].values()] == [tuple(s) for s in scales]
    assert yaml_load(path)["model_type"] == "ASVSRModel"
    _check(opt)


def _resolves(opt):
    """`model_type` and every dataset `type` resolve through the registries (YAML surface)."""
    assert savsr_amd.MODEL_REGISTRY.get(opt["model_type"]).__name__ == opt["model_type"]
    for d in opt["datasets"].values():
        assert savsr_amd.DATASET_REGISTRY.get(d["type"]).__name__ == d["type"]


def test_sample_yaml_registry_resolution():
    _resolves(parse_test_options(SAMPLE))
    with pytest.raises(KeyError):
        savsr_amd.MODEL_REGISTRY.get("NoSuchModel")


@pytest.mark.parametrize("dataset", ["Vid4", "UDM10"])
def test_scale_list_yaml_registry_resolution(tmp_path, dataset):
    _resolves(parse_test_options(_scale_list_yaml(tmp_path, dataset)[0]))


def test_model_and_dataset_refuse_cpu():
    """No CPU fallback behind the YAML surface either: without a GPU both constructors raise."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    opt = parse_test_options(SAMPLE)
    with pytest.raises(RuntimeError):
        savsr_amd.build_model(opt)
    with pytest.raises(RuntimeError):
        savsr_amd.build_dataset(opt["datasets"]["test_01"])
