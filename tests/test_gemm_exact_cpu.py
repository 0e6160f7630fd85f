"""The exact-arithmetic GEMM references (tests/exact_gemm.py) tied to the project's parity anchor, without a GPU: on exact
inputs the pinned C oracle's own fp32 summation order is exact too, so the helper's fp64-then-round-once references must
equal it BIT FOR BIT; and the generators' preconditions must raise when violated (never skip, never pass quietly)."""
import pytest
import torch

import oracle
import exact_gemm as eg


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", [16, 128, 1408])
@pytest.mark.parametrize("N", [16, 72])
@pytest.mark.parametrize("M", [1, 7])
def test_fp8_reference_equals_the_oracle_bit_for_bit(M, N, K, bias, dt):
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + bias)
    c = eg.exact_fp8_case(M, N, K, dt, bias, g)
    got = oracle.fp8_scaled_mm(c.a, c.w.t(), c.sa, c.sb, dt, c.bias)
    assert torch.equal(_bits(got), _bits(c.ref))
    # the case is not trivial: scales of different magnitude, and results that needed rounding
    assert c.sa.numel() == 1 or float(c.sa.max() / c.sa.min()) >= 2.0 ** 6
    assert float(c.sb.max() / c.sb.min()) >= 2.0 ** 5
    assert bool((c.a.float() == c.a.float().round()).all()) and float(c.a.float().abs().max()) <= 16


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M", [1, 7])
def test_awq_reference_equals_the_oracle_bit_for_bit(M, bias):
    """oracle.awq_gemm adds the bias as torch's `out.add_(bias)` does -- to the ROUNDED 16-bit product (awq.py:413-417) -- so
    its counterpart is the bias_after_round form; the one-rounding form (the k-packed kernels' epilogue) differs from it only
    through that second rounding and agrees with it wherever there is no bias."""
    K, N, G = 256, 128, 128
    g = torch.Generator().manual_seed(M + bias)
    c = eg.exact_awq_case(M, K, N, G, bias, g)
    w = oracle.awq_dequantize(c.qweight, c.scales, c.qzeros)
    # (w - z) * s with power-of-two scales is exact in fp16
    nib_range = w.double().abs() / c.scales.double().abs().repeat_interleave(G, 0)
    assert bool((nib_range == nib_range.round()).all()) and float(nib_range.max()) <= 15
    assert bool((c.scales < 0).any()) and bool((c.scales > 0).any())
    got = oracle.awq_gemm(c.x, c.qweight, c.scales, c.qzeros, c.bias)
    assert torch.equal(_bits(got), _bits(eg.awq_reference(c.x, w, c.bias, bias_after_round=True)))
    if not bias:
        assert torch.equal(_bits(got), _bits(eg.awq_reference(c.x, w)))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_linear16_reference_is_exact_in_any_summation_order(dt):
    """No oracle entry point for linear16: its reference is held to fp32 sums taken forwards, backwards and in slices."""
    g = torch.Generator().manual_seed(3)
    c = eg.exact_linear16_case(7, 40, 1024, dt, True, g)
    prod = c.a.float().unsqueeze(1) * c.w.float().unsqueeze(0)          # [M, N, K] fp32 products, each exact
    fwd = prod.cumsum(-1)[..., -1]
    bwd = prod.flip(-1).cumsum(-1)[..., -1]
    sliced = prod.view(7, 40, 8, 128).sum(-1).sum(-1)
    for acc in (fwd, bwd, sliced):
        assert torch.equal(_bits((acc + c.bias.float()).to(dt)), _bits(c.ref))


def test_preconditions_raise_when_violated():
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="2\\^24"):
        eg.exact_fp8_case(1, 16, 65600, torch.bfloat16, False, g, A=16)
    eg.exact_fp8_case(1, 16, 65600, torch.bfloat16, False, g)  # A = 8 by the rule: fine
    with pytest.raises(ValueError, match="e4m3"):
        eg.exact_fp8_case(1, 16, 16, torch.bfloat16, False, g, A=17)
    with pytest.raises(ValueError, match="2\\^24"):
        eg.exact_linear16_case(1, 16, 65536, torch.bfloat16, False, g)
    with pytest.raises(ValueError, match="2\\^24"):
        eg.exact_awq_case(1, 4096, 128, 128, False, g, emax=6)
    assert eg.awq_emax(4096) == 5 and eg.awq_emax(2176) == 6 and eg.awq_emax(512) == 8
    # fp16 range checks, on the reference itself
    with pytest.raises(ValueError, match="does not fit fp16"):
        eg.round_once(torch.tensor([[70000.0]], dtype=torch.float64), torch.float16, None, "x")
    with pytest.raises(ValueError, match="subnormal"):
        eg.round_once(torch.tensor([[2.0 ** -15, 1.0]], dtype=torch.float64), torch.float16, None, "x")
    with pytest.raises(ValueError, match="not representable in fp32"):
        eg.round_once(torch.tensor([[1.0 + 2.0 ** -30]], dtype=torch.float64), torch.bfloat16, None, "x")
    eg.round_once(torch.tensor([[2.0 ** -30, 0.0]], dtype=torch.float64), torch.bfloat16, None, "x")  # bf16 has fp32's range


def test_assert_bits_equal_reports_where_and_how():
    ref = torch.zeros(256, 128, dtype=torch.bfloat16)
    eg.assert_bits_equal(ref.clone(), ref, "same")
    out = ref.clone()
    out[130:134, 70] = 2.0  # rows 2..5 mod 128, column 6 mod 64; two steps of 1.0 away
    with pytest.raises(AssertionError) as e:
        eg.assert_bits_equal(out, ref, "probe", step=torch.tensor(1.0, dtype=torch.float64))
    msg = str(e.value)
    assert "4 of 32768 elements differ" in msg and "(row 130, col 70)" in msg
    assert "rows mod 128" in msg and "2: 1" in msg and "cols mod 64 -> count {6: 4}" in msg
    assert "whole number of scale steps at 4 and within one output ulp at 0 of 4" in msg and "k-step" in msg
    near = torch.full((2, 8), 1.0, dtype=torch.bfloat16)
    off = near.clone()
    off[1, 3] = 1.0 + 2.0 ** -7  # the neighbouring bf16 value: a rounding slip, although 2^13 steps of 2^-20 away
    with pytest.raises(AssertionError, match="within one output ulp at 1 of 1 differing elements \\(rounding / epilogue order\\?\\)"):
        eg.assert_bits_equal(off, near, "ulp", step=torch.tensor(2.0 ** -20, dtype=torch.float64))
    out[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="5 of 32768"):
        eg.assert_bits_equal(out, ref, "nan counts as different")


@pytest.mark.parametrize("M,N,K,shuffled,variant", [
    (2048, 7168, 512, True, "tiled3 128x256"),
    (2048, 4352, 512, True, "tiled3 128x192"),
    (1024, 24576, 512, True, "tiled3 256x256"),
    (1000, 24592, 512, True, "tiled3 256x256"),
    (1024, 6144, 512, True, "tiled3_ks2 cb=3"),
    (1024, 8192, 512, True, "tiled3_ks2 cb=4"),
    (1537, 4112, 512, True, "tiled3_ks2 cb=4"),
    (2048, 6144, 512, False, "tiled2 84"),
    (300, 512, 1024, False, "tiled2 22"),
    (2048, 2304, 512, False, "tiled2 2"),
    (300, 512, 1024, True, "tiled2 22"),
    (300, 512, 1008, False, "tiled"),
])
def test_the_variant_rule_reaches_every_tiled_form_at_the_shapes_the_gpu_suite_uses(M, N, K, shuffled, variant):
    assert eg.fp8_tiled_variant(M, N, K, shuffled) == variant


def test_oneshot_step_counts():
    admitted = [s for s in range(1, 33) if eg.fp8_oneshot_split(s)]
    assert admitted == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16, 18, 20, 21, 24, 28, 32]
