"""GPU: the NVFP4 weight-only linear (csrc/gemm_nvfp4.hip) -- ops.nvfp4_gemm bit for bit against the fp64 product of the
dequantised weight on operands for which fp32 accumulation is exact (the construction of exact_gemm.py), through all three
kernel forms; realistic data under the per-element bound; the repack round trip; PetitNvFp4LinearMethod."""
import pytest
import torch

from conftest import assert_elem_close
from exact_gemm import assert_bits_equal, check_exactness, exact_bias, round_once

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEN = set()
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def _dequant(weight, weight_scale):
    """uint8 [N, K / 2] (low nibble = even k; sign(1) exp(2) man(1)) x e4m3 [N, K / 16] -> fp64 [N, K]."""
    codes = torch.stack([weight & 15, weight >> 4], dim=-1).reshape(weight.shape[0], -1).long()
    w = torch.where(codes >= 8, -E2M1[codes & 7], E2M1[codes & 7])  # (-0.0 stays a zero)
    return w * weight_scale.to(torch.float64).repeat_interleave(16, dim=1)


def _exact_emax(K):
    emax = 8
    while K * 90 * (1 << (emax + 4)) >= 1 << 24:
        emax -= 1
    return emax


def _exact_weight(N, K, g):
    """Every byte value as a weight byte; group scales (1 + m / 8) 2^e with all eight mantissas and e in [-emax, 0]: against
    integers in [-8, 8] every product is a multiple of 2^-(emax + 4) and at most 6 * 1.875 * 8 = 90."""
    emax = _exact_emax(K)
    assert emax == {512: 4, 528: 4, 1024: 3, 4096: 1}[K]
    check_exactness(K, 90 << (emax + 4), f"nvfp4 exact case K={K}")
    weight = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scale = ((1 + torch.randint(0, 8, (N, K // 16), generator=g) / 8.0)
             * torch.exp2(-torch.randint(0, emax + 1, (N, K // 16), generator=g).float())).to(torch.float8_e4m3fn)
    return weight, scale


def _exact_case(M, N, K, dt, bias, g):
    x = torch.randint(-8, 9, (M, K), generator=g).to(dt)
    weight, scale = _exact_weight(N, K, g)
    ws2 = torch.tensor(0.25)
    b = exact_bias(N, dt, g) if bias else None
    ref = round_once(x.double() @ _dequant(weight, scale).t() * ws2.double(), dt, b, f"nvfp4 M={M} N={N} K={K}",
                     bias_after_round=True)
    return x, weight, scale, ws2, b, ref


# M: ragged fragments, the streamer / tile boundary (64 | 65), more than two row tiles.  (272, 1024): a partial column
# tile; (512, 4096): four K slices in the streamer; (136, 528): N % 16 != 0 and K % 128 != 0 (no prepared form exists).
@pytest.mark.parametrize("N,K,prepared", [(128, 512, True), (128, 512, False), (272, 1024, True), (512, 4096, True),
                                          (136, 528, False)])
@pytest.mark.parametrize("M", [1, 3, 17, 64, 65, 129, 300])
def test_nvfp4_gemm_bit_exact(M, N, K, prepared):
    from sglang_npu_amd import ops
    v = M + N // 128 + K // 512 + int(prepared)
    dt = torch.float16 if v & 1 else torch.bfloat16
    what = f"nvfp4 M={M} N={N} K={K} prepared={prepared} {dt} bias={bool(v & 2)}"
    x, weight, scale, ws2, bias, ref = _exact_case(M, N, K, dt, bool(v & 2), torch.Generator().manual_seed(1000 * M + N + K))
    w, s = weight.to(DEV), scale.to(DEV)
    if prepared:
        w, s = ops.nvfp4_repack(w, s)
    out = ops.nvfp4_gemm(x.to(DEV), w, s, ws2.to(DEV), None if bias is None else bias.to(DEV))
    kernel = ops.nvfp4_last_kernel()
    SEEN.add(kernel)
    assert kernel == ("nvfp4_generic" if not prepared else "nvfp4_tiled" if M > 64 else "nvfp4_stream"), what
    assert_bits_equal(out.cpu(), ref, what)


def test_every_kernel_form_ran():
    assert SEEN == {"nvfp4_stream", "nvfp4_tiled", "nvfp4_generic"}


def _modelopt_quantize(w):
    """ModelOpt's NVFP4 rule: global scale amax / (6 * 448), group scale (group amax / 6) / global in e4m3, codes to nearest."""
    ws2 = w.abs().max() / (6.0 * 448.0)
    scale = (w.reshape(w.shape[0], -1, 16).abs().amax(-1) / 6.0 / ws2).to(torch.float8_e4m3fn)
    t = w / (scale.float().repeat_interleave(16, dim=1) * ws2)
    codes = ((t.abs().unsqueeze(-1) - E2M1.float()).abs().argmin(-1) | ((t < 0).long() << 3)).to(torch.uint8)
    return codes[:, 0::2] | (codes[:, 1::2] << 4), scale, ws2.float()


# K = 2048: an fp32 matmul of the same operands, rounded to the output type, stays inside the bound on the CPU (largest
# error / bound over the four cases 0.87 in bf16 and 0.49 in fp16), so the shape needs no shrinking.
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M", [5, 200])
def test_nvfp4_gemm_realistic(M, dt):
    from sglang_npu_amd import ops
    N, K = 256, 2048
    g = torch.Generator().manual_seed(M)
    weight, scale, ws2 = _modelopt_quantize(torch.randn(N, K, generator=g) * K ** -0.5)
    x = torch.randn(M, K, generator=g).to(dt)
    ref = x.double() @ _dequant(weight, scale).t() * ws2.double()
    w, s = ops.nvfp4_repack(weight.to(DEV), scale.to(DEV))
    out = ops.nvfp4_gemm(x.to(DEV), w, s, ws2.to(DEV))
    assert_elem_close(out, ref, dt, what=f"nvfp4 realistic M={M} {dt}")


def test_repack_round_trip():
    from sglang_npu_amd import ops
    g = torch.Generator().manual_seed(7)
    weight = torch.randint(0, 256, (272, 512), generator=g, dtype=torch.uint8).to(DEV)
    scale = torch.randint(0, 127, (272, 64), generator=g, dtype=torch.uint8).view(torch.float8_e4m3fn).to(DEV)
    w, s = ops.nvfp4_repack(weight, scale)
    assert w.shape == (17, 8 * 1024) and s.shape == (17, 1024) and s.dtype == torch.uint8
    # the layout formula of include/sgl_mi355.h for (n, k) = (37, 300): block 2, unit 9, row 5
    assert w.view(-1)[((2 * 32 + 9) * 16 + 5) * 16 + 6] == weight[37, 150]
    assert s.view(-1)[((2 * 32 + 9) * 16 + 5) * 2 + 0] == scale.view(torch.uint8)[37, 18]
    w2, s2 = ops.nvfp4_repack(w, s, inverse=True)
    assert torch.equal(w2, weight) and torch.equal(s2.view(torch.uint8), scale.view(torch.uint8))


def _loaded_layer(shards, K):
    from sglang_npu_amd.linear import MergedColumnParallelLinear
    from sglang_npu_amd.quantization import PetitNvFp4Config
    cfg = PetitNvFp4Config.from_config({"quantization": {"quant_algo": "NVFP4", "group_size": 16,
                                                         "kv_cache_quant_algo": None, "exclude_modules": []}})
    with torch.device(DEV):
        layer = MergedColumnParallelLinear(K, [w.shape[0] for w, _, _ in shards], quant_config=cfg)
    for i, (w, s, s2) in enumerate(shards):
        layer.weight.weight_loader(layer.weight, w, i)
        layer.weight_scale.weight_loader(layer.weight_scale, s, i)
        layer.weight_scale_2.weight_loader(layer.weight_scale_2, s2, i)
        layer.input_scale.weight_loader(layer.input_scale, torch.tensor(1.0), i)
    layer.quant_method.process_weights_after_loading(layer)
    return layer


def test_layer_runs_the_gemm(monkeypatch):
    from sglang_npu_amd import ops, quantization
    g = torch.Generator().manual_seed(3)
    K = 512
    # exact operands (see _exact_weight): the generic kernel sums in another order than the MFMA kernels, and only sums that
    # are exact in any order can be asked to agree bit for bit
    shards = [tuple(t.to(DEV) for t in (*_exact_weight(n, K, g), torch.tensor(s2))) for n, s2 in ((256, 0.25), (384, 0.5))]
    layer = _loaded_layer(shards, K)
    monkeypatch.setattr(quantization, "PRESHUFFLE_FP8_WEIGHTS", False)
    layer_c = _loaded_layer(shards, K)
    assert layer.weight.shape == (640 // 16, 8 * K) and layer_c.weight.shape == (640, K // 2)
    assert layer.weight_scale_2 == max(shards[0][2], shards[1][2]) != min(shards[0][2], shards[1][2])
    assert not hasattr(layer, "input_scale")
    for rows in (5, 200):
        x = torch.randint(-8, 9, (rows, K), generator=g).bfloat16().to(DEV)
        out = layer(x)[0]
        assert torch.equal(out, ops.nvfp4_gemm(x, layer.weight, layer.weight_scale, layer.weight_scale_2)), rows
        assert torch.equal(out, layer_c(x)[0]), rows
    ptr = layer.weight.data_ptr()
    layer.quant_method.process_weights_after_loading(layer)
    assert layer.weight.data_ptr() == ptr and torch.equal(layer(x)[0], out)
