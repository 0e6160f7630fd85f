"""CPU: the "w8a8_int8" config, the parameters its linear method creates, `ignore`, and the refusal of CPU tensors."""
import pytest
import torch

from sglang_npu_amd.quantization import W8A8Int8Config, get_quantization_config


def test_registry_and_create_weights():
    from sglang_npu_amd.linear import MergedColumnParallelLinear
    assert get_quantization_config("w8a8_int8") is W8A8Int8Config
    cfg = W8A8Int8Config.from_config({"quant_method": "w8a8_int8"})
    assert cfg.get_name() == "w8a8_int8" and cfg.get_supported_act_dtypes() == [torch.float16, torch.bfloat16]
    layer = MergedColumnParallelLinear(528, [256, 136], quant_config=cfg)
    assert type(layer.quant_method).__name__ == "W8A8Int8LinearMethod"
    assert layer.weight.shape == (392, 528) and layer.weight.dtype == torch.int8
    assert type(layer.weight_scale).__name__ == "ChannelQuantScaleParameter"
    assert layer.weight_scale.shape == (392, 1) and layer.weight_scale.dtype == torch.float32


def test_ignored_prefixes_get_the_unquantised_method():
    from sglang_npu_amd.linear import MergedColumnParallelLinear, RowParallelLinear
    cfg = W8A8Int8Config.from_config({"ignore": ["lm_head", "re:.*layers\\.0\\.mlp\\.(gate|up)_proj"],
                                      "packed_modules_mapping": {"gate_up_proj": ["gate_proj", "up_proj"]}})
    name = lambda layer: type(layer.quant_method).__name__  # noqa: E731
    assert name(RowParallelLinear(64, 32, quant_config=cfg, prefix="lm_head")) == "UnquantizedLinearMethod"
    assert name(RowParallelLinear(64, 32, quant_config=cfg, prefix="model.layers.0.mlp.down_proj")) == "W8A8Int8LinearMethod"
    assert name(MergedColumnParallelLinear(64, [32, 32], quant_config=cfg, prefix="model.layers.0.mlp.gate_up_proj")) == \
        "UnquantizedLinearMethod"
    assert name(MergedColumnParallelLinear(64, [32, 32], quant_config=cfg, prefix="model.layers.1.mlp.gate_up_proj")) == \
        "W8A8Int8LinearMethod"


def test_ops_refuse_cpu_tensors():
    from sglang_npu_amd import ops
    a, s = torch.zeros(2, 64, dtype=torch.int8), torch.ones(2, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.per_token_quant_int8(torch.zeros(2, 64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.int8_scaled_mm(a, torch.zeros(8, 64, dtype=torch.int8).t(), s, torch.ones(8, 1), torch.bfloat16)
