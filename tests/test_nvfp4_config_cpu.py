"""CPU: PetitNvFp4Config / PetitNvFp4LinearMethod host logic (petit.py) and PerTensorScaleParameter shard loading."""
import pytest
import torch

from sglang_npu_amd import quantization
from sglang_npu_amd.linear import ColumnParallelLinear
from sglang_npu_amd.parameter import PerTensorScaleParameter
from sglang_npu_amd.quantization import PetitNvFp4Config, PetitNvFp4LinearMethod, UnquantizedLinearMethod


def _hf(**changes):
    q = {"quant_algo": "NVFP4", "group_size": 16, "kv_cache_quant_algo": None, "exclude_modules": ["lm_head", "model.layers.*.mlp.gate"]}
    q.update(changes)
    return {"quantization": {k: v for k, v in q.items() if v is not ...}}


def test_registry_and_from_config():
    assert quantization.get_quantization_config("petit_nvfp4") is PetitNvFp4Config
    cfg = PetitNvFp4Config.from_config(_hf())
    assert cfg.get_name() == "petit_nvfp4" and cfg.is_checkpoint_nvfp4_serialized and cfg.group_size == 16
    assert cfg.kv_cache_quant_algo == "auto" and cfg.get_config_filenames() == ["hf_quant_config.json"]
    assert PetitNvFp4Config.override_quantization_method({"quant_method": "ModelOpt"}, None) == \
        ("petit_nvfp4" if torch.version.hip else None)
    assert PetitNvFp4Config.override_quantization_method({"quant_method": "awq"}, None) is None


@pytest.mark.parametrize("changes,match", [({"quant_algo": "FP8"}, "only supports: NVFP4"), ({"group_size": 32}, "group_size=16"),
                                           ({"exclude_modules": ...}, "requires group size")])
def test_from_config_rejects(changes, match):
    with pytest.raises(ValueError, match=match):
        PetitNvFp4Config.from_config(_hf(**changes))


def test_create_weights_and_excluded_layers():
    cfg = PetitNvFp4Config.from_config(_hf())
    layer = ColumnParallelLinear(64, [32, 16], quant_config=cfg, prefix="model.layers.0.mlp.gate_up_proj")
    assert isinstance(layer.quant_method, PetitNvFp4LinearMethod)
    got = {n: (tuple(p.shape), p.dtype) for n, p in layer.named_parameters()}
    assert got == {"weight": ((48, 32), torch.uint8), "weight_scale": ((48, 4), torch.float8_e4m3fn),
                   "weight_scale_2": ((2,), torch.float32), "input_scale": ((2,), torch.float32)}
    with pytest.raises(ValueError, match="not multiple of 16"):
        ColumnParallelLinear(72, [32], quant_config=cfg)
    for prefix in ("lm_head", "model.layers.11.mlp.gate"):  # a listed name, a wildcard
        assert isinstance(ColumnParallelLinear(64, [32], quant_config=cfg, prefix=prefix).quant_method, UnquantizedLinearMethod)


def test_per_tensor_scale_parameter_loads_by_shard():
    p = PerTensorScaleParameter(data=torch.zeros(3), weight_loader=None)
    for value, (sid, loader) in enumerate([("q", p.load_qkv_weight), ("k", p.load_qkv_weight), ("v", p.load_qkv_weight),
                                           (1, p.load_merged_column_weight)], start=1):
        loader(torch.tensor([float(value)]) if value & 1 else torch.tensor(float(value)), shard_id=sid, shard_offset=0, shard_size=8)
    assert p.data.tolist() == [1.0, 4.0, 3.0]
    p.load_row_parallel_weight(torch.tensor([7.0, 8.0, 9.0]))
    assert p.data.tolist() == [7.0, 8.0, 9.0]
    with pytest.raises(AssertionError):
        p.load_qkv_weight(torch.tensor(1.0), shard_id="o")
