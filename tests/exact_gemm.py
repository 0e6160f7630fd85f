"""Inputs on which a GEMM with fp32 accumulation is EXACT, and the bit-exact references that go with them.

Every GEMM family of the library accumulates products in fp32 in an order of its own (split-K slices, slabs, k groups,
MFMA blocking).  On operands that are small integers times a power of two, every product and every partial sum -- in any
order -- is an integer multiple of one quantum and stays below 2^24 quanta, so fp32 holds all of them exactly and the
only rounding left is the one to the 16-bit output.  The result of any correct kernel is then ONE bit pattern, and the
tests compare with torch.equal on the whole output: no tolerance, no scalar of the tensor, no sampled rows.

* FP8 (fp8_scaled_mm): operands integers in [-A, A] (exact in e4m3 up to 16), K A^2 < 2^24; per-token and per-channel
  scales powers of two, so acc * w_scale * x_scale is exact in fp32 as well.  Without bias the output is the fp64
  product rounded once; with bias it is round16(fp32(acc sb sa) + fp32(bias)) -- the epilogue order of the oracle
  (x w_scale, x x_scale, + bias, one rounding); an fma gives the same bits because the product is exact.
* linear16: x and W integers / 16 with |i| <= 16: products are multiples of 2^-8, |sum| <= K, exact while K 2^8 < 2^24.
* AWQ: (w - z) s with power-of-two group scales (of both signs) is exact in fp16; x integers / 8 with |i| <= 32; sums
  are multiples of 2^-(emax + 3) bounded by 15 K, exact while 15 K 2^(emax + 3) < 2^24 for scales 2^-2 .. 2^-emax.

The generators assert their own preconditions (the inequality above; for fp16 outputs max |ref| < 65504 and no non-zero
|ref| below 2^-14, i.e. no fp16 subnormals): a case that violates one is an error of the test, never a skip.

A plain helper module, not a conftest: it defines no fixtures and changes nothing about collection."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

TWO24 = 1 << 24
FP16_MAX = 65504.0
FP16_MIN_NORMAL = 2.0 ** -14


class ExactCase(NamedTuple):
    a: torch.Tensor                 # [M, K] activations (fp8 / 16-bit)
    w: torch.Tensor                 # [N, K] row-major weight (fp8 / 16-bit); AWQ: the dequantised [K, N] fp16 weight
    sa: Optional[torch.Tensor]      # [M, 1] float32 powers of two (FP8 only)
    sb: Optional[torch.Tensor]      # [N, 1] float32 powers of two (FP8 only)
    bias: Optional[torch.Tensor]    # [N] in the output dtype, or None
    ref: torch.Tensor               # [M, N] in the output dtype: the one correct bit pattern
    step: torch.Tensor              # quantum of the unrounded result per element (broadcastable to [M, N], float64)


def fp8_amax(K: int) -> int:
    """Largest operand magnitude the issue's rule gives: 16 up to K = 16384, 8 beyond."""
    return 16 if K <= 16384 else 8


def check_exactness(K: int, worst_product_quanta: int, what: str) -> None:
    """The exactness inequality: K products of at most `worst_product_quanta` quanta each stay below 2^24 quanta."""
    if K * worst_product_quanta >= TWO24:
        raise ValueError(f"{what}: K * {worst_product_quanta} = {K * worst_product_quanta} >= 2^24: fp32 partial sums are "
                         "not exact for these operands")


def check_fp16_range(ref32: torch.Tensor, dt: torch.dtype, what: str) -> None:
    """fp16 outputs: nothing overflows and nothing lands in the subnormals (whose handling is not what is under test)."""
    if dt != torch.float16:
        return
    mag = ref32.abs()
    if float(mag.max()) >= FP16_MAX:
        raise ValueError(f"{what}: max |ref| = {float(mag.max())} does not fit fp16")
    nz = mag[mag > 0]
    if nz.numel() and float(nz.min()) < FP16_MIN_NORMAL:
        raise ValueError(f"{what}: a non-zero |ref| = {float(nz.min())} is an fp16 subnormal")


def _pow2(exponents: torch.Tensor) -> torch.Tensor:
    return torch.exp2(exponents.to(torch.float32))


def _randint(lo: int, hi: int, shape, g: torch.Generator) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device)


def exact_bias(N: int, dt: torch.dtype, g: torch.Generator) -> torch.Tensor:
    """Integers / 64 in [-8, 8]: exact in both 16-bit types, and a multiple of every quantum used here down to 2^-14 -- so
    a bias cannot cancel a result into the fp16 subnormals -- while the sum still needs a genuine rounding."""
    return (_randint(-512, 512, (N,), g).to(torch.float32) / 64.0).to(dt)


def round_once(acc64: torch.Tensor, dt: torch.dtype, bias: Optional[torch.Tensor], what: str,
               bias_after_round: bool = False) -> torch.Tensor:
    """fp64 exact value -> the 16-bit output.  The value must be exact in fp32 (asserted), so fp64 -> fp32 -> 16 bit is ONE
    rounding.  bias: round16(fp32(value) + fp32(bias)); bias_after_round (torch's `out.add_(bias)` on a 16-bit result):
    round16(fp32(round16(value)) + fp32(bias))."""
    r32 = acc64.to(torch.float32)
    if not torch.equal(r32.to(torch.float64), acc64):
        raise ValueError(f"{what}: the exact result is not representable in fp32 (precondition of the construction)")
    if bias is None:
        check_fp16_range(r32, dt, what)
        return r32.to(dt)
    if bias_after_round:
        check_fp16_range(r32, dt, what)
        r32 = r32.to(dt).to(torch.float32)
    r32 = r32 + bias.to(torch.float32).view(1, -1)
    check_fp16_range(r32, dt, what)
    return r32.to(dt)


def fp8_scale_exponents(M: int, N: int, dt: torch.dtype, g: torch.Generator):
    """Power-of-two scales whose magnitudes differ by 2^20 across rows and 2^10 across columns (bf16).  fp16 outputs have
    five exponent bits: rows 2^-3 .. 2^-9 and columns 2^0 .. 2^-5, so that one quantum sa sb >= 2^-14 (no subnormals) and
    2^-3 max |acc| < 65504 (asserted on the reference)."""
    (a_hi, a_lo), (b_hi, b_lo) = ((-3, -9), (0, -5)) if dt == torch.float16 else ((0, -20), (0, -10))
    ea, eb = _randint(a_lo, a_hi, (M, 1), g), _randint(b_lo, b_hi, (N, 1), g)
    # both ends of each range are always present, whatever the draw
    ea[0], ea[-1] = a_hi, a_lo
    eb[0], eb[-1] = b_hi, b_lo
    return ea, eb


def fp8_reference(a, w, sa, sb, dt, bias=None, what="fp8 reference") -> torch.Tensor:
    acc = a.to(torch.float64) @ w.to(torch.float64).t()
    return round_once(acc * sb.to(torch.float64).view(1, -1) * sa.to(torch.float64).view(-1, 1), dt, bias, what)


def exact_fp8_case(M: int, N: int, K: int, dt: torch.dtype, bias: bool, g: torch.Generator, A: Optional[int] = None) -> ExactCase:
    A = fp8_amax(K) if A is None else A
    what = f"exact_fp8_case(M={M}, N={N}, K={K}, A={A})"
    if A > 16:
        raise ValueError(f"{what}: integers above 16 are not all exact in e4m3")
    check_exactness(K, A * A, what)
    a = _randint(-A, A, (M, K), g).to(torch.float32).to(torch.float8_e4m3fn)
    w = _randint(-A, A, (N, K), g).to(torch.float32).to(torch.float8_e4m3fn)
    ea, eb = fp8_scale_exponents(M, N, dt, g)
    sa, sb = _pow2(ea), _pow2(eb)
    b = exact_bias(N, dt, g) if bias else None
    ref = fp8_reference(a, w, sa, sb, dt, b, what)
    return ExactCase(a, w, sa, sb, b, ref, sa.to(torch.float64) * sb.to(torch.float64).view(1, -1))


def linear16_reference(x, w, bias=None, what="linear16 reference") -> torch.Tensor:
    return round_once(x.to(torch.float64) @ w.to(torch.float64).t(), x.dtype, bias, what)


def exact_linear16_operands(M: int, N: int, K: int, dt: torch.dtype, g: torch.Generator):
    check_exactness(K, 256, f"exact_linear16 (K={K})")
    x = (_randint(-16, 16, (M, K), g).to(torch.float32) / 16.0).to(dt)
    w = (_randint(-16, 16, (N, K), g).to(torch.float32) / 16.0).to(dt)
    return x, w


def exact_linear16_case(M: int, N: int, K: int, dt: torch.dtype, bias: bool, g: torch.Generator) -> ExactCase:
    x, w = exact_linear16_operands(M, N, K, dt, g)
    b = exact_bias(N, dt, g) if bias else None
    ref = linear16_reference(x, w, b, f"exact_linear16_case(M={M}, N={N}, K={K})")
    return ExactCase(x, w, None, None, b, ref, torch.tensor(2.0 ** -8, dtype=torch.float64, device=x.device))


def awq_emax(K: int) -> int:
    """Smallest scale 2^-emax for which 15 K 2^(emax + 3) < 2^24 (at most 2^-8, at least 2^-2)."""
    emax = 8
    while emax >= 2 and 15 * K * (1 << (emax + 3)) >= TWO24:
        emax -= 1
    if emax < 2:
        raise ValueError(f"exact_awq_case: K = {K} leaves no exact scale range (15 K 2^5 >= 2^24)")
    return emax


class AwqCase(NamedTuple):
    x: torch.Tensor                 # [M, K] fp16, integers / 8
    qweight: torch.Tensor           # [K, N / 8] int32
    scales: torch.Tensor            # [K / G, N] fp16, +- powers of two
    qzeros: torch.Tensor            # [K / G, N / 8] int32
    bias: Optional[torch.Tensor]
    step: torch.Tensor


def exact_awq_case(M: int, K: int, N: int, G: int, bias: bool, g: torch.Generator, emax: Optional[int] = None) -> AwqCase:
    emax = awq_emax(K) if emax is None else emax
    check_exactness(K, 15 * (1 << (emax + 3)), f"exact_awq_case(K={K}, emax={emax})")
    imax = torch.iinfo(torch.int32).max
    qw = torch.randint(0, imax, (K, N // 8), dtype=torch.int32, generator=g, device=g.device)
    qz = torch.randint(0, imax, (K // G, N // 8), dtype=torch.int32, generator=g, device=g.device)
    e = -_randint(2, emax, (K // G, N), g)
    sign = 1.0 - 2.0 * (_randint(0, 3, (K // G, N), g) == 0).to(torch.float32)  # a quarter of the scales negative
    sc = (sign * _pow2(e)).to(torch.float16)
    x = (_randint(-32, 32, (M, K), g).to(torch.float32) / 8.0).to(torch.float16)
    b = exact_bias(N, torch.float16, g) if bias else None
    return AwqCase(x, qw, sc, qz, b, torch.tensor(2.0 ** -(emax + 3), dtype=torch.float64, device=x.device))


def awq_reference(x, w_dequant, bias=None, bias_after_round=False, what="awq reference") -> torch.Tensor:
    """x [M, K] @ the dequantised fp16 weight [K, N] (awq_dequantize, pinned bit-exact elsewhere), rounded once."""
    return round_once(x.to(torch.float64) @ w_dequant.to(torch.float64), x.dtype, bias, what, bias_after_round)


def _top(counts: torch.Tensor, n: int = 6) -> str:
    vals, idx = torch.sort(counts, descending=True)
    return ", ".join(f"{int(i)}: {int(v)}" for v, i in zip(vals[:n].tolist(), idx[:n].tolist()) if v > 0)


def assert_bits_equal(out: torch.Tensor, ref: torch.Tensor, what: str, step: Optional[torch.Tensor] = None) -> None:
    """torch.equal on the whole output, with a failure report that points at a wave, a tile or a k-step."""
    assert out.shape == ref.shape and out.dtype == ref.dtype, f"{what}: {tuple(out.shape)} {out.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    if torch.equal(out, ref):
        return
    try:
        from sglang_npu_amd import ops
        kernel = ops.fp8_last_kernel()
    except Exception:  # noqa: BLE001  (no library here: the report goes without the name)
        kernel = "?"
    o, r = out.to(torch.float64), ref.to(torch.float64)
    bad = (o != r) | torch.isnan(o)
    rows, cols = torch.nonzero(bad, as_tuple=True)
    r0, c0 = int(rows[0]), int(cols[0])
    msg = (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ (last fp8 kernel '{kernel}'); first at (row {r0}, col {c0}): "
           f"got {float(o[r0, c0])!r}, expected {float(r[r0, c0])!r}; rows mod 128 -> count {{{_top(torch.bincount(rows % 128, minlength=128))}}}; "
           f"cols mod 64 -> count {{{_top(torch.bincount(cols % 64, minlength=64))}}}")
    if step is not None:
        q = ((o - r) / step.to(o.device).expand_as(o))[bad]
        q = q[torch.isfinite(q)]
        whole = int((q == q.round()).sum())
        # one output ulp apart at most is what a rounding or epilogue-order slip gives; a lost k-step moves by whole steps AND far
        frac_bits = 7 if out.dtype == torch.bfloat16 else 10
        mag = torch.maximum(o.abs(), r.abs())[bad]
        ulp = torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** -126))) - frac_bits)
        near = int(((o - r).abs()[bad] <= ulp).sum())
        nbad = int(bad.sum())
        hint = "rounding / epilogue order?" if near == nbad else ("a dropped or duplicated k-step?" if whole == nbad else "mixed")
        msg += (f"; out - ref is a whole number of scale steps at {whole} and within one output ulp at {near} of {nbad} differing "
                f"elements ({hint})")
    raise AssertionError(msg)


# --- run_gemm's variant rules (csrc/gemm_fp8.hip), recomputed from the shape: fp8_last_kernel() names the family only ---
def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def fp8_tiled_variant(M: int, N: int, K: int, shuffled: bool) -> str:
    """Which tiled kernel and which of its forms run_gemm picks above 256 rows (or wherever the weight streamer declined), by
    the rule's own inputs: grid_b (256 x 256 tiles), grid_s (128 x 128), grid_4 / grid_c3 (128 x 256 / 128 x 192), cost3 /
    cost4 (tiles on the busiest CU x tile width) and cb."""
    if K % 128 != 0:
        return "tiled"
    grid_s = _cdiv(M, 128) * _cdiv(N, 128)
    grid_b = _cdiv(M, 256) * _cdiv(N, 256)
    v2 = 84 if grid_b >= 192 else (22 if grid_s <= 256 else 2)
    tiles_m3 = _cdiv(M, 128)
    grid_4, grid_c3 = tiles_m3 * _cdiv(N, 256), tiles_m3 * _cdiv(N, 192)
    cost4, cost3 = _cdiv(grid_4, 256) * 4, _cdiv(grid_c3, 256) * 3
    cb = 3 if cost3 < cost4 else 4
    grid_3 = grid_c3 if cb == 3 else grid_4
    if shuffled and K % 512 == 0 and grid_3 >= 192:
        if grid_3 <= 256:
            return f"tiled3_ks2 cb={cb}"
        if _cdiv(M, 256) <= 4 and 384 <= grid_b <= 512:
            return "tiled3 256x256"
        return f"tiled3 128x{64 * cb}"
    return f"tiled2 {v2}"


def fp8_oneshot_split(steps: int) -> int:
    """S of launch_oneshot's K / 128 = WK * S (S <= 4, WK <= 8), 0 where the one-shot kernel declines."""
    for c in (1, 2, 3, 4):
        if steps % c == 0 and steps // c <= 8:
            return c
    return 0
