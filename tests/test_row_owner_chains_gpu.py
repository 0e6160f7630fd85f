"""The decode row-owner kernels after their load chains were shortened (RoPE + KV write from partials with v heads on waves
of their own and every load in front of the first store; partial sums fetched four or eight slices at a time by the real
slice count), and the per-token quantiser they feed.  These are re-orderings of loads, not of arithmetic, so every comparison is
torch.equal against the sequence the project treats as the definition: fp8_gemm_finalize followed by the plain kernel for
the from-partials forms, the oracle's per_token_quant_fp8 for the quantiser.

ops.GemmPartials is built by hand from a random fp32 tensor [slices, M, N] plus random scales, so the slice count is free:
1-4 take the four-at-a-time form, 5-8 the eight-at-a-time form, 9 its loop over batches."""
import itertools

import pytest
import torch

import oracle
from sglang_npu_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _partials(g, slices, M, N, dtype, with_bias):
    """A split-K GEMM "in flight": fp32 partial sums whose slice sum is O(1) after the scales."""
    ws = torch.randn(slices, M, N, device=DEV, generator=g) * 40.0
    sa = torch.rand(M, device=DEV, generator=g) * 1e-1 + 1e-2
    sb = torch.rand(N, device=DEV, generator=g) * 1e-1 + 1e-2
    bias = torch.randn(N, device=DEV, generator=g).to(dtype) if with_bias else None
    return ops.GemmPartials(ws.reshape(-1), slices, sa, sb, bias, M, N, dtype)


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [8, 4096, 4104, 14336, 16392])  # one vector; one round of 512 threads; a part-empty last round; long rows
def test_per_token_quant_matches_the_oracle(K, dtype):
    g = torch.Generator().manual_seed(K)
    x_all = (torch.randn(65, K, generator=g) * 3).to(dtype)
    x_all[1].zero_()            # an all-zero row: scale 0, all-zero bytes
    x_all[2, :-1] *= 0.01
    x_all[2, -1] = 200.0        # a row whose maximum sits in its last element
    for rows in (1, 3, 64, 65):
        x = x_all[:rows].contiguous()
        q_ref, s_ref = torch.empty(rows, K, dtype=torch.uint8), torch.empty(rows)
        oracle.per_token_quant_fp8(x, q_ref, s_ref)
        q = torch.full((rows, K), 0x55, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
        s = torch.full((rows, 1), -1.0, device=DEV)
        ops.sgl_per_token_quant_fp8(x.to(DEV), q, s)
        assert torch.equal(q.view(torch.uint8).cpu(), q_ref), f"rows={rows}: bytes differ"
        assert torch.equal(s.view(-1).cpu(), s_ref), f"rows={rows}: scales differ"
        if rows >= 3:
            assert s_ref[1] == 0 and not q_ref[1].any()
            assert s_ref[2] == torch.tensor(200.0) / 448.0 and q_ref[2, -1] == 0x7E  # 448 = 0x7E in e4m3fn


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_per_token_quant_single_special_rows(dtype):
    """One row alone: all zeros, and the maximum in the last element (the last thread's last lane)."""
    for K in (8, 4096, 4104, 14336, 16392):
        zero = torch.zeros(1, K, dtype=dtype)
        last = torch.full((1, K), 0.5, dtype=dtype)
        last[0, -1] = -96.0
        for x in (zero, last):
            q_ref, s_ref = torch.empty(1, K, dtype=torch.uint8), torch.empty(1)
            oracle.per_token_quant_fp8(x, q_ref, s_ref)
            q = torch.full((1, K), 0x55, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
            s = torch.full((1, 1), -1.0, device=DEV)
            ops.sgl_per_token_quant_fp8(x.to(DEV), q, s)
            assert torch.equal(q.view(torch.uint8).cpu(), q_ref) and torch.equal(s.view(-1).cpu(), s_ref), f"K={K}"
        assert s_ref[0] == torch.tensor(96.0) / 448.0


# ------------------------------------------------------------------------------------------------ RoPE + KV write
_POOLS = {"16bit": None, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


@pytest.mark.parametrize("pool", list(_POOLS))
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(4, 1), (32, 8)])
def test_rope_kv_from_partials_equals_finalize_then_rope_kv(heads, D, pool):
    """q and the written K / V pool rows equal finalize + apply_rope_and_set_kv_buffer; every pool row not named in `loc` keeps
    its sentinel.  bf16 throughout, fp16 for the five-token cases with 2, 4 and 9 slices."""
    Hq, Hk = heads
    N = (Hq + 2 * Hk) * D
    n_slots = 12
    g = torch.Generator(device=DEV).manual_seed(Hq * 1000 + D)
    for T, slices, with_bias in itertools.product((1, 5), (1, 2, 4, 5, 8, 9), (False, True)):
        dtype = torch.float16 if (T == 5 and slices in (2, 4, 9)) else torch.bfloat16
        part = _partials(g, slices, T, N, dtype, with_bias)
        full = part.finalize()
        pos = torch.randint(0, 300, (T,), device=DEV, generator=g)
        loc64 = (torch.randperm(n_slots - 1, device=DEV, generator=g)[:T] + 1).long()
        untouched = torch.ones(n_slots, dtype=torch.bool, device=DEV)
        untouched[loc64] = False
        pdt = _POOLS[pool] or dtype
        sentinel = torch.full((n_slots, Hk, D), 0x3C, dtype=torch.uint8, device=DEV)  # 1.0 in e5m2, 1.5 in e4m3; 16-bit: 0x3C3C
        if pool == "16bit":
            sentinel = torch.full((n_slots, Hk, D), 0x3C3C, dtype=torch.int16, device=DEV)
        for rot_dim, neox, loc in itertools.product((D, D // 2), (True, False), (loc64, loc64.int())):
            cache = torch.randn(320, rot_dim, device=DEV, generator=g)
            kb_ref, vb_ref = sentinel.clone().view(pdt), sentinel.clone().view(pdt)
            kb, vb = sentinel.clone().view(pdt), sentinel.clone().view(pdt)
            q_ref, k_ref, v_ref = full.clone().split([Hq * D, Hk * D, Hk * D], dim=-1)
            ops.apply_rope_and_set_kv_buffer(pos, q_ref, k_ref, v_ref, D, cache, kb_ref, vb_ref, loc, neox)
            q = ops.rope_set_kv_from_partials(part, pos, Hq, Hk, D, cache, kb, vb, loc, neox)
            what = f"T={T} slices={slices} bias={with_bias} rot={rot_dim} neox={neox} loc={loc.dtype}"
            assert torch.equal(q, q_ref), "q: " + what
            raw = lambda t: t.view(sentinel.dtype)  # noqa: E731
            assert torch.equal(raw(kb), raw(kb_ref)), "K pool: " + what
            assert torch.equal(raw(vb), raw(vb_ref)), "V pool: " + what
            assert torch.equal(raw(kb)[untouched], sentinel[untouched]), "K pool rows outside loc: " + what
            assert torch.equal(raw(vb)[untouched], sentinel[untouched]), "V pool rows outside loc: " + what
            assert not torch.equal(raw(kb)[loc64], sentinel[loc64]) and not torch.equal(raw(vb)[loc64], sentinel[loc64])


# ------------------------------------------------------------------------------------------------ norm / activation
@pytest.fixture(scope="module")
def norm_inputs():
    g = torch.Generator(device=DEV).manual_seed(7)
    out = {}
    for dtype in (torch.bfloat16, torch.float16):
        out[dtype] = dict(weight=(torch.rand(4096, device=DEV, generator=g) + 0.5).to(dtype),
                          residual=torch.randn(64, 4096, device=DEV, generator=g).to(dtype))
    return out


@pytest.mark.parametrize("slices", [1, 2, 3, 4, 5, 7, 8, 9])
@pytest.mark.parametrize("N", [128, 4096])
def test_norm_and_activation_from_partials_equal_finalize_then_plain(N, slices, norm_inputs):
    g = torch.Generator(device=DEV).manual_seed(N + slices)
    for M, dtype, with_bias in itertools.product((1, 7, 64), (torch.bfloat16, torch.float16), (False, True)):
        part = _partials(g, slices, M, N, dtype, with_bias)
        full = part.finalize()
        wn = norm_inputs[dtype]["weight"][:N].contiguous()
        res0 = norm_inputs[dtype]["residual"][:M, :N].contiguous()
        what = f"M={M} {dtype} bias={with_bias}"
        # add + RMSNorm + quant
        r_ref, r = res0.clone(), res0.clone()
        q_ref, s_ref, _ = ops.rmsnorm_quant_fp8(full.clone(), wn, 1e-5, residual=r_ref)
        q, s = ops.rmsnorm_quant_fp8_from_partials(part, r, wn, 1e-5)
        assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(s, s_ref) and torch.equal(r, r_ref), \
            "rmsnorm_quant_fp8_from_partials: " + what
        # add + RMSNorm with the 16-bit row (+ its quantisation)
        x_ref, r_ref, r = full.clone(), res0.clone(), res0.clone()
        ops.fused_add_rmsnorm(x_ref, r_ref, wn, 1e-5)
        qx_ref = torch.empty(M, N, dtype=torch.float8_e4m3fn, device=DEV)
        sx_ref = torch.empty(M, 1, device=DEV)
        ops.sgl_per_token_quant_fp8(x_ref, qx_ref, sx_ref)
        out, q, s = ops.fused_add_rmsnorm_from_partials(part, r, wn, 1e-5, with_fp8=True)
        assert torch.equal(out, x_ref) and torch.equal(r, r_ref), "fused_add_rmsnorm_from_partials: " + what
        assert torch.equal(q.view(torch.uint8), qx_ref.view(torch.uint8)) and torch.equal(s, sx_ref), \
            "fused_add_rmsnorm_from_partials (fp8): " + what
        assert torch.equal(ops.fused_add_rmsnorm_from_partials(part, res0.clone(), wn, 1e-5), x_ref)
        # SiLU * mul + quant: the N outputs as [gate | up]
        q_ref, s_ref = ops.silu_and_mul_quant_fp8(full)
        q, s = ops.silu_and_mul_quant_fp8_from_partials(part)
        assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(s, s_ref), \
            "silu_and_mul_quant_fp8_from_partials: " + what
