"""CPU: the block-FP8 ("fp8", weight_block_size [128, 128]) config, its parameters and their sharding by the harness
layers, and the dispatcher schema of fp8_blockwise_scaled_mm."""
import pytest
import torch

from sglang_npu_amd import distributed as D
from sglang_npu_amd.quantization import Fp8Config, Fp8LinearMethod, get_quantization_config

CFG = {"quant_method": "fp8", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}


@pytest.fixture(autouse=True)
def _restore_tp():
    yield
    D.set_tp_group(D.GroupCoordinator(None, 0, 1, None))


def test_config_registry_and_validity_checks():
    assert get_quantization_config("fp8") is Fp8Config
    cfg = Fp8Config.from_config(CFG)
    assert cfg.get_name() == "fp8" and cfg.is_checkpoint_fp8_serialized and cfg.weight_block_size == [128, 128]
    for bad in ([128], [128, 128, 128]):
        with pytest.raises(ValueError, match="2 dimensions"):
            Fp8Config.from_config({**CFG, "weight_block_size": bad})
    with pytest.raises(ValueError, match="dynamic activation scheme"):
        Fp8Config.from_config({**CFG, "activation_scheme": "static"})
    with pytest.raises(NotImplementedError, match="per-tensor"):
        Fp8LinearMethod(Fp8Config.from_config({"quant_method": "fp8", "activation_scheme": "dynamic"}))
    with pytest.raises(NotImplementedError, match="static"):
        Fp8LinearMethod(Fp8Config(True, "static"))


def test_create_weights_shapes():
    from sglang_npu_amd.linear import RowParallelLinear
    layer = RowParallelLinear(640, 272, quant_config=Fp8Config.from_config(CFG))
    assert type(layer.quant_method).__name__ == "Fp8LinearMethod"
    assert layer.weight.shape == (272, 640) and layer.weight.dtype == torch.float8_e4m3fn
    assert type(layer.weight_scale_inv).__name__ == "BlockQuantScaleParameter"
    assert layer.weight_scale_inv.shape == (3, 5) and layer.weight_scale_inv.dtype == torch.float32  # ceil(272 / 128) = 3


def test_tp2_loaders_give_each_rank_its_slices():
    from sglang_npu_amd.linear import MergedColumnParallelLinear, QKVParallelLinear, RowParallelLinear
    cfg, tp, g = Fp8Config.from_config(CFG), 2, torch.Generator().manual_seed(0)
    w = lambda n, k: torch.randn(n, k, generator=g).to(torch.float8_e4m3fn)  # noqa: E731
    s = lambda n, k: torch.rand(-(-n // 128), k // 128, generator=g)  # noqa: E731
    hidden, head, Hq, Hkv = 256, 128, 4, 2
    gate_up = [(w(n, hidden), s(n, hidden)) for n in (256, 512)]
    qkv = {sid: (w(h * head, hidden), s(h * head, hidden)) for sid, h in (("q", Hq), ("k", Hkv), ("v", Hkv))}
    wd, sd = w(272, 512), s(272, 512)

    def load(layer, shards):
        for sid, (wt, sc) in shards:
            layer.weight.weight_loader(layer.weight, wt, *sid)
            layer.weight_scale_inv.weight_loader(layer.weight_scale_inv, sc, *sid)
        return layer.weight.data.view(torch.uint8), layer.weight_scale_inv.data

    def rows(t, rank):  # this rank's half of the output rows (weight rows or scale block rows)
        n = t.shape[0] // tp
        return t[rank * n:(rank + 1) * n]

    for rank in range(tp):
        D.set_tp_group(D.GroupCoordinator(None, rank, tp, None))
        got_w, got_s = load(MergedColumnParallelLinear(hidden, [256, 512], quant_config=cfg),
                            [((i,), ws) for i, ws in enumerate(gate_up)])
        assert torch.equal(got_w, torch.cat([rows(wt, rank) for wt, _ in gate_up]).view(torch.uint8))
        assert torch.equal(got_s, torch.cat([rows(sc, rank) for _, sc in gate_up]))
        got_w, got_s = load(QKVParallelLinear(hidden, head, Hq, Hkv, quant_config=cfg), [((sid,), ws) for sid, ws in qkv.items()])
        assert torch.equal(got_w, torch.cat([rows(qkv[sid][0], rank) for sid in "qkv"]).view(torch.uint8))
        assert torch.equal(got_s, torch.cat([rows(qkv[sid][1], rank) for sid in "qkv"]))
        got_w, got_s = load(RowParallelLinear(512, 272, quant_config=cfg), [((), (wd, sd))])
        assert torch.equal(got_w, wd[:, rank * 256:(rank + 1) * 256].contiguous().view(torch.uint8))
        assert torch.equal(got_s, sd[:, rank * 2:(rank + 1) * 2])
    with pytest.raises(ValueError, match="block_n"):  # 384 / 2 = 192 output rows per rank: not whole blocks
        MergedColumnParallelLinear(hidden, [256, 384], quant_config=cfg)


def test_dispatcher_schema_is_the_reference_string():
    from sglang_npu_amd import torch_ops
    torch_ops.register()
    assert str(torch.ops.sgl_kernel.fp8_blockwise_scaled_mm.default._schema) == (
        "sgl_kernel::fp8_blockwise_scaled_mm(Tensor mat_a, Tensor mat_b, Tensor scales_a, Tensor scales_b, "
        "ScalarType out_dtype) -> Tensor")
