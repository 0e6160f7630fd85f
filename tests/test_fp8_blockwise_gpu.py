"""GPU: the block-scaled FP8 GEMM (csrc/gemm_fp8_block.hip; 128 x 128 weight blocks, 1 x 128 activation groups) --
ops.fp8_blockwise_scaled_mm bit for bit on exact operands through every kernel form, within a derived per-element bound on
realistic values, and through Fp8LinearMethod on harness layers."""
import pytest
import torch

from conftest import assert_elem_close
from exact_gemm import assert_bits_equal, check_exactness, exact_bias, round_once

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEN = set()


def _expand(s, rows, dim):
    """One scale per 128 -> one per element along `dim` (the last block may be partial)."""
    return s.repeat_interleave(128, dim=dim).narrow(dim, 0, rows)


def _dequant(q, s_rows):
    """[R, K] FP8 and its per-(row, k-block) scales [R, K / 128] -> fp64."""
    return q.to(torch.float64) * _expand(s_rows.to(torch.float64), q.shape[1], 1)


def _mat_b(w, shuffled):
    from sglang_npu_amd import ops
    return ops.fp8_shuffle_weight(w) if shuffled else w.t()


# M: ragged fragments, the streamer / tile boundary (64 | 65), more than two row tiles.  (N, K): 272 = a partial last scale
# block and a partial last tile; K > 1024 = more than one K slice in the streamer.  Layout, dtype, scales_a layout and bias
# alternate over the grid so that each meets every kernel form.
@pytest.mark.parametrize("shuffled", [True, False])
@pytest.mark.parametrize("N,K", [(128, 512), (272, 1024), (512, 2048), (384, 4096)])
@pytest.mark.parametrize("M", [1, 3, 17, 64, 65, 129, 300])
def test_exact_arithmetic(M, N, K, shuffled):
    from sglang_npu_amd import ops
    v = M + N // 128 + K // 512 + int(shuffled)
    dt = torch.float16 if v & 1 else torch.bfloat16
    m_major, bias = bool(v & 2), bool(v & 4)
    what = f"block fp8 M={M} N={N} K={K} shuffled={shuffled} {dt} m_major={m_major} bias={bias}"
    A = 4 if K <= 2048 else 2
    check_exactness(K, A * A * 256, what)  # every partial sum is a multiple of 2^-8 bounded by K A^2
    g = torch.Generator(device=DEV).manual_seed(1000 * M + N + K)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g, device=DEV)  # noqa: E731
    a = ri(-A, A, M, K).float().to(torch.float8_e4m3fn)
    w = ri(-A, A, N, K).float().to(torch.float8_e4m3fn)
    KB, NB = K // 128, -(-N // 128)
    sa = torch.exp2(ri(-4, 0, M, KB).float())
    sb = torch.exp2(ri(-4, 0, KB, NB).float())
    b = exact_bias(N, dt, g) if bias else None
    acc = _dequant(a, sa) @ _dequant(w, _expand(sb.t(), N, 0)).t()
    ref = round_once(acc, dt, b, what, bias_after_round=True)
    sa_arg = sa.t().contiguous().t() if m_major else sa
    out = ops.fp8_blockwise_scaled_mm(a, _mat_b(w, shuffled), sa_arg, sb, dt, b)
    kernel = ops.fp8_last_kernel()
    SEEN.add(kernel)
    assert kernel == ("block_tiled" if M > 64 else "block_stream" if shuffled else "block_stream_rowmajor"), what
    assert ops.fp8_blockwise_split_k(M, K) == (-(-K // 1024) if M <= 64 else 1), what
    assert_bits_equal(out, ref, what, torch.tensor(2.0 ** -8, dtype=torch.float64))


def test_every_kernel_form_ran():
    assert SEEN == {"block_stream", "block_stream_rowmajor", "block_tiled"}


def _accumulation_term(a_deq, w_deq):
    """First-order worst case of K fp32 additions in any order plus two scale multiplications per 128-k block."""
    K = a_deq.shape[1]
    return ((K + K / 64) * 2.0 ** -24 * (a_deq.abs() @ w_deq.abs().t())).float().cpu()


def _quant_act(x):
    from sglang_npu_amd import ops
    q = torch.empty_like(x, dtype=torch.float8_e4m3fn)
    s = torch.empty(x.shape[0], x.shape[1] // 128, dtype=torch.float32, device=x.device)
    ops.sgl_per_token_group_quant_fp8(x, q, s, 128, 1e-10, -448.0, 448.0, False)
    return q, s


def _block_quant_weight(w):
    """amax / 448 per 128 x 128 block: (e4m3 [N, K], weight_scale_inv [ceil(N/128), K/128])."""
    N, K = w.shape
    nb = -(-N // 128)
    pad = torch.zeros(nb * 128, K, device=w.device)
    pad[:N] = w
    s = pad.view(nb, 128, K // 128, 128).abs().amax(dim=(1, 3)).clamp_min(1e-12) / 448.0
    return (w / _expand(_expand(s, N, 0), K, 1)).to(torch.float8_e4m3fn), s


@pytest.mark.parametrize("shuffled", [True, False])
@pytest.mark.parametrize("M,N,K", [(5, 256, 1024), (200, 512, 2048)])
def test_realistic_values(M, N, K, shuffled):
    from sglang_npu_amd import ops
    g = torch.Generator(device=DEV).manual_seed(M)
    q, s = _quant_act(torch.randn(M, K, generator=g, device=DEV).bfloat16())
    wq, ws = _block_quant_weight(torch.randn(N, K, generator=g, device=DEV) * K ** -0.5)
    a_deq, w_deq = _dequant(q, s), _dequant(wq, _expand(ws, N, 0))
    out = ops.fp8_blockwise_scaled_mm(q, _mat_b(wq, shuffled), s, ws.t(), torch.bfloat16)
    assert_elem_close(out, a_deq @ w_deq.t(), torch.bfloat16, what=f"M={M} N={N} K={K} shuffled={shuffled}",
                      extra=_accumulation_term(a_deq, w_deq))


def test_layers_load_and_run():
    from sglang_npu_amd import ops
    from sglang_npu_amd.linear import MergedColumnParallelLinear, RowParallelLinear
    from sglang_npu_amd.quantization import Fp8Config
    cfg = Fp8Config.from_config({"quant_method": "fp8", "activation_scheme": "dynamic", "weight_block_size": [128, 128]})
    g = torch.Generator(device=DEV).manual_seed(3)
    with torch.device(DEV):
        layers = [(MergedColumnParallelLinear(512, [256, 384], quant_config=cfg), [256, 384], 512),
                  (RowParallelLinear(640, 272, quant_config=cfg), [272], 640)]  # K = 640: no fragment-major form
    for layer, widths, K in layers:
        shards = [_block_quant_weight(torch.randn(n, K, generator=g, device=DEV) * K ** -0.5) for n in widths]
        for i, (wq, ws) in enumerate(shards):
            sid = (i,) if len(widths) > 1 else ()
            layer.weight.weight_loader(layer.weight, wq, *sid)
            layer.weight_scale_inv.weight_loader(layer.weight_scale_inv, ws, *sid)
        layer.quant_method.process_weights_after_loading(layer)
        assert ops.is_wshuffled(layer.weight) == (K % 512 == 0)
        w_deq = torch.cat([_dequant(wq, _expand(ws, wq.shape[0], 0)) for wq, ws in shards])
        for rows in (3, 200):
            x = torch.randn(rows, K, generator=g, device=DEV).bfloat16()
            out = layer(x)[0]
            a_deq = _dequant(*_quant_act(x))
            assert_elem_close(out, a_deq @ w_deq.t(), torch.bfloat16, what=f"{type(layer).__name__} rows={rows}",
                              extra=_accumulation_term(a_deq, w_deq))
        ptr = layer.weight.data_ptr()
        layer.quant_method.process_weights_after_loading(layer)  # re-entry: same storage, same output
        assert layer.weight.data_ptr() == ptr and torch.equal(layer(x)[0], out)
