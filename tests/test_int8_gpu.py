"""GPU: the W8A8 INT8 linear (csrc/quant_int8.hip, csrc/gemm_int8.hip) -- ops.per_token_quant_int8 and ops.int8_scaled_mm bit
for bit against plain torch on the CPU (fp32 elementwise ops there are IEEE; the int32 accumulator is an fp64 matmul of the
integer operands, exact because |acc| < 2^53), through every kernel form, W8A8Int8LinearMethod and the dispatcher."""
import pytest
import torch

from exact_gemm import FP16_MAX, assert_bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEN = set()


def _quant_ref(x):
    """test/srt/cpu/utils.py:23-31 in fp32 on the CPU: both divisions correctly rounded, torch.round = ties to even.
    The multiplier is a tensor / tensor division on purpose: torch evaluates `127 / absmax` (a Python number over a
    tensor) as absmax.reciprocal() * 127, two roundings, which is one ulp off the quotient for about a fifth of all rows."""
    xf = x.float().cpu()
    absmax = xf.abs().amax(dim=-1, keepdim=True).clamp_min(1e-10)
    return torch.round(xf * (torch.full_like(absmax, 127.0) / absmax)).to(torch.int8), absmax / 127.0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [64, 528, 4096])
@pytest.mark.parametrize("T", [1, 5, 67])
def test_per_token_quant_bit_exact(T, K, dt):
    from sglang_npu_amd import ops
    g = torch.Generator().manual_seed(100 * T + K)
    x = (torch.randn(T, K, generator=g) * 3).to(dt)
    # absmax exactly 127 makes the multiplier exactly 1, so 0.5, 1.5 and 2.5 are exact ties: half-to-even gives 0, 2, 2
    ties = (torch.randn(1, K, generator=g) * 3).to(dt)
    ties[0, :8] = torch.tensor([127.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -127.0]).to(dt)
    zero = torch.zeros(1, K, dtype=dt)
    if T == 1:  # one row cannot be all three: three one-row calls
        inputs = [x, ties, zero]
    else:
        x[0], x[T - 1] = ties[0], zero[0]
        inputs = [x]
    for xi in inputs:
        q_ref, s_ref = _quant_ref(xi)
        q, s = ops.per_token_quant_int8(xi.to(DEV))
        assert q.dtype == torch.int8 and s.dtype == torch.float32 and s.shape == (xi.shape[0], 1)
        assert torch.equal(s.cpu(), s_ref), f"scale T={T} K={K} {dt}"
        assert torch.equal(q.cpu(), q_ref), f"q T={T} K={K} {dt}"
    # what the two special rows ask of the kernel (on the reference, so that the inputs cannot drift away from it)
    assert _quant_ref(ties)[0][0, :8].tolist() == [127, 0, 0, 2, -2, 2, -2, -127]
    assert _quant_ref(zero)[1][0, 0] == torch.tensor(1e-10) / 127.0 and not _quant_ref(zero)[0].any()


def _gemm_ref(a, w, sa, sb, dt, bias, what):
    """The epilogue of int8_gemm_kernel.cu / epilogue_per_row_per_col_scale.h:278,301, one fp32 rounding per step."""
    acc = a.double() @ w.double().t()
    r = acc.float() * (sb.view(1, -1) * sa.view(-1, 1))
    if bias is not None:
        r = r + bias.float().view(1, -1)
    assert float(r.abs().max()) < FP16_MAX, what
    return r.to(dt)


# M: ragged fragments, the streamer / tile boundary (64 | 65), more than two row tiles.  (272, 1024): a partial column
# tile; (512, 4096): two K slices in the streamer; (136, 528): N % 16 != 0 and a K tail (no fragment-major form exists).
@pytest.mark.parametrize("N,K,shuffled", [(128, 512, True), (128, 512, False), (272, 1024, True), (272, 1024, False),
                                          (512, 4096, True), (512, 4096, False), (136, 528, False)])
@pytest.mark.parametrize("M", [1, 3, 17, 64, 65, 129, 300])
def test_int8_scaled_mm_bit_exact(M, N, K, shuffled):
    from sglang_npu_amd import ops
    v = M + N // 128 + K // 512 + int(shuffled)
    dt = torch.float16 if v & 1 else torch.bfloat16
    what = f"int8 M={M} N={N} K={K} shuffled={shuffled} {dt} bias={bool(v & 2)}"
    g = torch.Generator().manual_seed(1000 * M + N + K)
    a = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8)
    w = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    sa, sb = 1e-2 * torch.rand(M, 1, generator=g), 1e-3 * torch.rand(N, 1, generator=g)
    bias = torch.randn(N, generator=g).to(dt) if v & 2 else None
    ref = _gemm_ref(a, w, sa, sb, dt, bias, what)
    wd = w.to(DEV)
    mat_b = ops.int8_shuffle_weight(wd) if shuffled else wd.t()
    out = ops.int8_scaled_mm(a.to(DEV), mat_b, sa.to(DEV), sb.to(DEV), dt, None if bias is None else bias.to(DEV))
    kernel = ops.int8_last_kernel()
    SEEN.add(kernel)
    assert kernel == ("int8_tiled" if M > 64 else "int8_stream" if shuffled else "int8_stream_rowmajor"), what
    assert_bits_equal(out.cpu(), ref, what)


def test_every_kernel_form_ran():
    assert SEEN == {"int8_stream", "int8_stream_rowmajor", "int8_tiled"}


def _loaded_layer(shards, K):
    from sglang_npu_amd.linear import MergedColumnParallelLinear
    from sglang_npu_amd.quantization import W8A8Int8Config
    with torch.device(DEV):
        layer = MergedColumnParallelLinear(K, [q.shape[0] for q, _ in shards], quant_config=W8A8Int8Config.from_config({}))
    for i, (q, s) in enumerate(shards):
        layer.weight.weight_loader(layer.weight, q, i)
        layer.weight_scale.weight_loader(layer.weight_scale, s, i)
    layer.quant_method.process_weights_after_loading(layer)
    return layer


def test_layer_runs_quant_then_gemm(monkeypatch):
    from sglang_npu_amd import ops, quantization
    g = torch.Generator(device=DEV).manual_seed(3)
    K, shards = 512, []
    for n in (256, 384):  # per-channel symmetric weight quantisation of random bf16
        w = (torch.randn(n, K, generator=g, device=DEV) * K ** -0.5).bfloat16().float()
        s = w.abs().amax(dim=1, keepdim=True) / 127.0
        shards.append((torch.round(w / s).to(torch.int8), s))
    layer = _loaded_layer(shards, K)
    monkeypatch.setattr(quantization, "PRESHUFFLE_FP8_WEIGHTS", False)
    layer_t = _loaded_layer(shards, K)
    assert layer.weight.shape == (640 // 16, 16 * K) and layer_t.weight.shape == (K, 640) and layer_t.weight.stride(0) == 1
    for rows in (5, 200):
        x = torch.randn(rows, K, generator=g, device=DEV).bfloat16()
        out = layer(x)[0]
        q, s = ops.per_token_quant_int8(x)
        assert torch.equal(out, ops.int8_scaled_mm(q, layer.weight, s, layer.weight_scale, x.dtype)), rows
        assert torch.equal(out, layer_t(x)[0]), rows
    ptr = layer.weight.data_ptr()
    layer.quant_method.process_weights_after_loading(layer)
    assert layer.weight.data_ptr() == ptr and torch.equal(layer(x)[0], out)


def test_dispatcher_reaches_the_same_kernel():
    from sglang_npu_amd import ops, torch_ops
    torch_ops.register()
    g = torch.Generator(device=DEV).manual_seed(5)
    a = torch.randint(-128, 128, (7, 512), generator=g, device=DEV, dtype=torch.int8)
    w = torch.randint(-128, 128, (128, 512), generator=g, device=DEV, dtype=torch.int8)
    sa, sb = torch.rand(7, 1, generator=g, device=DEV), torch.rand(128, 1, generator=g, device=DEV)
    assert torch.equal(torch.ops.sgl_kernel.int8_scaled_mm(a, w.t(), sa, sb, torch.bfloat16, None),
                       ops.int8_scaled_mm(a, w.t(), sa, sb, torch.bfloat16))
