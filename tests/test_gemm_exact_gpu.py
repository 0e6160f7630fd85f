"""Exact-arithmetic parity of every GEMM dispatch branch: torch.equal on the WHOLE output, no tolerance.

The inputs (tests/exact_gemm.py) make fp32 accumulation exact in any summation order, so a kernel's result has one correct
bit pattern whatever its split-K, slab, k-group or MFMA blocking -- the fp64 product rounded once (+ the fp32 bias add).
Per-token scales span 2^20 and per-channel scales 2^10, so a small row gets no slack from a large one; every row and every
column block of every tile is compared.  Each FP8 case names the kernel family it must reach (ops.fp8_last_kernel()) and,
for the tiled kernels, the variant by recomputing the dispatch rule's inputs (exact_gemm.fp8_tiled_variant)."""
import pytest
import torch

from sglang_npu_amd import ops
import exact_gemm as eg

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP16 = torch.bfloat16, torch.float16


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device=DEV).manual_seed(seed)


def _rows_of_wider_buffer(a: torch.Tensor, pad: int) -> torch.Tensor:
    """The same rows inside a buffer whose row stride is K + pad; the padding holds all-ones bytes (NaN in e4m3 and in both
    16-bit types), so that anything read past a row's K shows."""
    M, K = a.shape
    es = a.element_size()
    wide = torch.full((M, (K + pad) * es), 0xFF, dtype=torch.uint8, device=a.device)
    wide[:, :K * es] = a.contiguous().view(torch.uint8)
    return wide.view(a.dtype)[:, :K]


def _fp8_check(M, N, K, shuffled, dt, bias, seed, family=None, partials=False, strided=(False, True), slices=None):
    c = eg.exact_fp8_case(M, N, K, dt, bias, _gen(seed))
    wt = ops.fp8_shuffle_weight(c.w) if shuffled else c.w.t()
    names = []
    for st in strided:
        a = _rows_of_wider_buffer(c.a, 256) if st else c.a
        what = f"fp8 M={M} N={N} K={K} {'shuffled' if shuffled else 'row-major'} {dt} bias={bias} strided={st} partials={partials}"
        if partials:
            part = ops.fp8_scaled_mm_partials(a, wt, c.sa, c.sb, dt, c.bias)
            assert part is not None, f"{what}: no partials form"
            names.append(ops.fp8_last_kernel())
            plan = ops.fp8_gemm_plan(M, N, K, shuffled, part.ws.numel(), "partials", a.stride(0) if M > 1 else K)
            if slices is not None:
                assert slices[0] <= part.num_slices <= slices[1], (what, part.num_slices)
            out = part.finalize()
        else:
            out = ops.fp8_scaled_mm(a, wt, c.sa, c.sb, dt, c.bias)
            names.append(ops.fp8_last_kernel())
            plan = ops.fp8_gemm_plan(M, N, K, shuffled, a_stride=a.stride(0) if M > 1 else K)
        assert plan.family == names[-1], f"{what}: the plan says '{plan.family}', '{names[-1]}' ran"
        if family is not None:
            assert names[-1] == family, f"{what}: ran '{names[-1]}', the case is meant for '{family}'"
        eg.assert_bits_equal(out, c.ref, f"{what} [{names[-1]}]", c.step)
    return names


def _alt(i: int):
    """bias and output type alternate across the cases of a list: all four combinations come up."""
    return (BF16 if (i // 2) % 2 == 0 else FP16), i % 2 == 0


# ------------------------------------------------------------------------------------------------ FP8: the tiled kernels
_TILED = [
    (2048, 7168, 512, True, "tiled3 128x256"),
    (2048, 4352, 512, True, "tiled3 128x192"),
    (1024, 24576, 512, True, "tiled3 256x256"),
    (1000, 24592, 512, True, "tiled3 256x256"),   # ragged in both directions
    (1024, 6144, 512, True, "tiled3_ks2 cb=3"),
    (1024, 8192, 512, True, "tiled3_ks2 cb=4"),
    (1537, 4112, 512, True, "tiled3_ks2 cb=4"),   # ragged
    (2048, 6144, 512, False, "tiled2 84"),
    (300, 512, 1024, False, "tiled2 22"),
    (2048, 2304, 512, False, "tiled2 2"),
    (300, 512, 1024, True, "tiled2 22"),
    (300, 512, 1008, False, "tiled"),             # K tail
]


@pytest.mark.parametrize("i", range(len(_TILED)), ids=[f"{t[4].replace(' ', '_')}-{t[0]}x{t[1]}x{t[2]}-{'fm' if t[3] else 'rm'}" for t in _TILED])
def test_fp8_tiled_variants_are_exact(i):
    M, N, K, shuffled, variant = _TILED[i]
    assert eg.fp8_tiled_variant(M, N, K, shuffled) == variant  # the rule's inputs, recomputed: this shape is that variant
    dt, bias = _alt(i)
    _fp8_check(M, N, K, shuffled, dt, bias, 100 + i, family=variant.split()[0])


@pytest.mark.parametrize("M", [300, 512])
def test_fp8_tiled3_raw_split_k_partials_are_exact(M):
    _fp8_check(M, 4096, 8192, True, FP16 if M == 300 else BF16, M == 300, 200 + M, family="tiled3_rawk", partials=True, slices=(2, 4))


# ------------------------------------------------------------------------------------------------ FP8: the weight streamer
@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("N,K,shuffled,family", [
    (12800, 512, True, "wstream"),
    (12808, 512, False, "wstream"),     # ragged N (row-major only: the fragment-major layout needs N % 16 == 0)
    (12800, 640, False, "oneshot"),     # five k-steps: no phase length divides them, the one-shot kernel takes K / 128 = 5 x 1
])
def test_fp8_wstream_direct_is_exact(M, N, K, shuffled, family):
    dt, bias = _alt(M)
    _fp8_check(M, N, K, shuffled, dt, bias, 300 + M + N + K, family=family, strided=(M % 2 == 1,))


def test_fp8_astat_direct_is_exact():
    _fp8_check(16, 20480, 576, False, BF16, True, 401, family="astat_direct")  # wide N with a 64-byte K tail


_SLAB = [
    (16, 4096, 10240, True, "wstream_slab"),    # 40 Mi weights at up to 32 rows
    (64, 6144, 4096, False, "wstream_slab"),    # 20 Mi above 32 rows where the one-shot kernel would qualify
    (64, 4096, 5120, True, "wstream_slab"),     # (40 k-steps: not a one-shot shape) the 8 Mi threshold
    (65, 4096, 2048, True, "wstream_slab"),     # 128-row phases from 8 Mi
    (128, 4096, 2048, False, "wstream_slab"),
    (100, 12800, 512, True, "wstream"),         # 128-row phases, direct
    (129, 4096, 14336, True, "wstream_slab"),   # 256-row phases
    (256, 4096, 14336, False, "wstream_slab"),
]


@pytest.mark.parametrize("i", range(len(_SLAB)), ids=[f"{t[0]}x{t[1]}x{t[2]}-{'fm' if t[3] else 'rm'}" for t in _SLAB])
def test_fp8_wstream_slabs_and_wide_phases_are_exact(i):
    M, N, K, shuffled, family = _SLAB[i]
    dt, bias = _alt(i)
    _fp8_check(M, N, K, shuffled, dt, bias, 500 + i, family=family)


# ------------------------------------------------------------------------------------------------ FP8: one-shot, skinny, astat
_ONESHOT_STEPS = [s for s in range(1, 33) if eg.fp8_oneshot_split(s)]  # every K <= 4096 the rule K / 128 = WK x S admits


@pytest.mark.parametrize("steps", _ONESHOT_STEPS)
@pytest.mark.parametrize("N", [256, 72])
def test_fp8_oneshot_every_admitted_step_count_is_exact(steps, N):
    for j, M in enumerate((1, 33, 64)):
        dt, bias = _alt(steps + j)
        _fp8_check(M, N, 128 * steps, False, dt, bias, 600 + steps + N + M, family="oneshot", strided=(j == 1,))


@pytest.mark.parametrize("steps", [4, 8, 12, 16, 20, 24, 28, 32])
def test_fp8_oneshot_on_the_fragment_major_weight_is_exact(steps):
    """K % 512 == 0 is the layout's own granularity: these are the step counts a shuffled weight can have."""
    for j, M in enumerate((1, 33, 64)):
        dt, bias = _alt(steps // 4 + j)
        _fp8_check(M, 256, 128 * steps, True, dt, bias, 700 + steps + M, family="oneshot", strided=(j == 2,))


@pytest.mark.parametrize("steps", [11, 13, 17, 27, 30])
def test_fp8_step_counts_the_oneshot_rule_rejects(steps):
    """No S <= 4 with K / 128 / S <= 8 (27 and 30 pass run_gemm's coarse `oneshot_ok`, which only sets a slab threshold, but
    launch_oneshot itself declines them): a row-major weight falls through to the skinny kernel and must be exact there; a
    fragment-major weight cannot exist at these K (launch_wstream and the layout want K % 512 == 0) -- fp8_shuffle_weight
    declines with its documented error before any GEMM is asked."""
    K = 128 * steps
    assert eg.fp8_oneshot_split(steps) == 0
    for j, M in enumerate((1, 33, 64)):
        dt, bias = _alt(steps + j)
        _fp8_check(M, 256, K, False, dt, bias, 800 + steps + M, family="skinny", strided=(j == 0,))
    w = torch.zeros(256, K, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="K % 512 == 0 required"):
        ops.fp8_shuffle_weight(w)


@pytest.mark.parametrize("M,N,K", [(7, 48, 208), (64, 12288, 208), (33, 12288, 208), (16, 1000, 144)])
def test_fp8_skinny_defaults_are_exact(M, N, K):
    """(nb, wk) = (2, 8) below N = 12288 and (4, 4) from there, each row bucket; K % 128 != 0 keeps every other kernel out."""
    dt, bias = _alt(M)
    _fp8_check(M, N, K, False, dt, bias, 900 + M + N, family="skinny")


def test_fp8_astat_long_k_is_exact():
    assert eg.fp8_amax(65600) == 8
    _fp8_check(16, 1024, 65600, False, FP16, True, 950, family="astat")


# ------------------------------------------------------------------------------------------------ FP8: 70B per-rank shapes
@pytest.mark.parametrize("M", [1, 64, 512, 1024])
@pytest.mark.parametrize("N,K", [(1280, 8192), (8192, 1024), (7168, 8192), (8192, 3584)])
def test_fp8_70b_rank_shapes_are_exact_on_both_layouts(M, N, K):
    dt, bias = _alt(M + N // 1024)
    c = eg.exact_fp8_case(M, N, K, dt, bias, _gen(M + N + K))
    for shuffled in (False, True):
        wt = ops.fp8_shuffle_weight(c.w) if shuffled else c.w.t()
        what = f"70B rank shape M={M} N={N} K={K} {'shuffled' if shuffled else 'row-major'} {dt} bias={bias}"
        out = ops.fp8_scaled_mm(c.a, wt, c.sa, c.sb, dt, c.bias)
        eg.assert_bits_equal(out, c.ref, f"{what} [{ops.fp8_last_kernel()}]", c.step)
        assert ops.fp8_gemm_plan(M, N, K, shuffled).family == ops.fp8_last_kernel(), what
        part = ops.fp8_scaled_mm_partials(c.a, wt, c.sa, c.sb, dt, c.bias)
        if part is not None:  # the split-K half, wherever it is offered
            name = ops.fp8_last_kernel()
            assert part.num_slices >= 1
            eg.assert_bits_equal(part.finalize(), c.ref, f"{what} partials x{part.num_slices} [{name}]", c.step)


# ------------------------------------------------------------------------------------------------ linear16
def _l16_check(x, w, bias, ref, what):
    for st in (False, True):
        xs = _rows_of_wider_buffer(x, 64) if st else x
        eg.assert_bits_equal(ops.linear16(xs, w, bias), ref, f"{what} strided={st}", torch.tensor(2.0 ** -8, dtype=torch.float64))


@pytest.mark.parametrize("dt", [BF16, FP16])
@pytest.mark.parametrize("M", [1, 16, 17, 64, 65, 128])
@pytest.mark.parametrize("N,K,form", [
    (1000, 768, "row-major"),        # unsplit streamer, N % 16 != 0, 12 k-steps
    (144, 256, "fm-unsplit"),        # fragment-major, a single phase: the split-K form declines (one slice)
    (25600, 256, "fm-unsplit"),      # fragment-major, wide N: unsplit by the N >= 25600 rule
    (144, 1024, "fm-splitk"),        # fragment-major, narrow N: K slices + finalize
    (4096, 2048, "fm-splitk"),
])
def test_linear16_streamer_branches_are_exact(M, N, K, form, dt):
    c = eg.exact_linear16_case(M, N, K, dt, (M + N // 16) % 2 == 0, _gen(M + N + K))
    what = f"linear16 {form} M={M} N={N} K={K} {dt} bias={c.bias is not None}"
    if form == "row-major":
        return _l16_check(c.a, c.w, c.bias, c.ref, what)
    wsh = ops.linear16_shuffle_weight(c.w)
    part = ops.linear16_partials(c.a, wsh, c.bias)  # offered exactly where linear16 itself takes the split-K form
    if form == "fm-splitk":
        assert part is not None and part.num_slices >= 2, what
        eg.assert_bits_equal(part.finalize(), c.ref, f"{what} partials x{part.num_slices}")
    else:
        assert part is None, f"{what}: meant for the unsplit kernel, but the split-K form took it"
    _l16_check(c.a, wsh, c.bias, c.ref, what)


_L16_SHARED = {}


def _l16_shared(dt):
    """One 1000 x 8192 activation, one 4096 x 8192 weight and their exact fp64 product per dtype: the K = 8192 tiled cases are
    row / column prefixes of it."""
    if dt not in _L16_SHARED:
        x, w = eg.exact_linear16_operands(1000, 4096, 8192, dt, _gen(77))
        _L16_SHARED[dt] = (x, w, x.double() @ w.double().t(), eg.exact_bias(4096, dt, _gen(78)))
    return _L16_SHARED[dt]


@pytest.mark.parametrize("dt", [BF16, FP16])
@pytest.mark.parametrize("M,N,K,slices", [
    (129, 512, 256, 0),       # 128 x 128 tiles, unsplit
    (300, 1040, 512, 0),      # ... ragged
    (300, 16400, 256, 0),     # >= 192 tiles of 128 x 256: the wide tile, ragged
    (300, 2048, 4096, 4),     # 64 k-steps: at most four slices of sixteen
    (1000, 3584, 8192, 2), (1000, 2576, 8192, 3), (1000, 2304, 8192, 4), (1000, 1920, 8192, 5),
    (1000, 1536, 8192, 6), (1000, 1408, 8192, 7), (300, 1024, 8192, 8),
])
def test_linear16_tiled_form_is_exact_at_every_slice_count(M, N, K, slices, dt):
    """More than 128 rows on the fragment-major weight.  The slice rule (ops._linear16_tiled_slices) returns 0 (unsplit) or
    min(640 // tiles, K / 1024) >= 2: every value it can take up to K = 8192 is run, the uneven ones (3, 5, 6, 7 slices of
    128 k-steps) included."""
    assert ops._linear16_tiled_slices(M, N, K) == slices
    use_bias = (N // 16 + slices) % 2 == 0
    if K == 8192:
        x, w, acc, b = _l16_shared(dt)
        x, w, bias = x[:M], w[:N], (b[:N].contiguous() if use_bias else None)
        ref = eg.round_once(acc[:M, :N], dt, bias, "linear16 tiled")
    else:
        c = eg.exact_linear16_case(M, N, K, dt, use_bias, _gen(M + N + K))
        x, w, bias, ref = c.a, c.w, c.bias, c.ref
    _l16_check(x, ops.linear16_shuffle_weight(w), bias, ref, f"linear16 tiled M={M} N={N} K={K} slices={slices} {dt} bias={use_bias}")


# ------------------------------------------------------------------------------------------------ AWQ
_AWQ_SHARED = {}
_AWQ_ROWS = 2100


def _awq_shared(K, N):
    """Per (K, N): the checkpoint tensors, the repacked ones, ops.awq_dequantize's weight (pinned bit-exact to the reference by
    the golden tests), 2100 activation rows and their exact fp64 product -- every test takes row prefixes."""
    if (K, N) not in _AWQ_SHARED:
        c = eg.exact_awq_case(_AWQ_ROWS, K, N, 128, True, _gen(K + N))
        w = ops.awq_dequantize(c.qweight, c.scales, c.qzeros)
        # the premise of the construction, on the kernel's own output: (w - z) * s came out as an integer in [-15, 15] times s
        ratio = w.double() / c.scales.double().repeat_interleave(128, 0)
        assert bool((ratio == ratio.round()).all()) and float(ratio.abs().max()) <= 15
        wp, sz = ops.awq_repack(c.qweight, c.scales, c.qzeros)
        _AWQ_SHARED[(K, N)] = (c, w, wp, sz, c.x.double() @ w.double())
    return _AWQ_SHARED[(K, N)]


_AWQ_SHAPES = [(512, 128), (2176, 1000), (4096, 4096)]


@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("K,N", _AWQ_SHAPES)
def test_awq_gemm_is_exact(M, K, N):
    """ops.awq_gemm is AWQLinearMethod.apply: the bias is added to the ROUNDED product, as torch's `out.add_(bias)` does
    (awq.hip; oracle.awq_gemm the same) -- round16(fp32(round16(acc)) + fp32(bias)).  The first rounding is outside the
    one-rounding argument, so the reference is that re-derived two-rounding form, still compared bit for bit."""
    c, w, _, _, acc = _awq_shared(K, N)
    bias = c.bias if M % 2 else None
    ref = eg.round_once(acc[:M], FP16, bias, "awq_gemm", bias_after_round=True)
    out = ops.awq_gemm(c.x[:M].contiguous(), c.qweight, c.scales, c.qzeros, bias)
    eg.assert_bits_equal(out, ref, f"awq_gemm M={M} K={K} N={N} bias={bias is not None}", c.step)


@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("K,N", _AWQ_SHAPES)
def test_awq_gemm_packed_and_its_partials_are_exact(M, K, N):
    c, w, wp, sz, acc = _awq_shared(K, N)
    bias = c.bias if M % 2 == 0 else None
    ref = eg.round_once(acc[:M], FP16, bias, "awq_gemm_packed")
    what = f"awq_gemm_packed M={M} K={K} N={N} bias={bias is not None}"
    for st in (False, True):
        x = _rows_of_wider_buffer(c.x[:M], 64) if st else c.x[:M]
        eg.assert_bits_equal(ops.awq_gemm_packed(x, wp, sz, 128, bias), ref, f"{what} strided={st}", c.step)
    part = ops.awq_gemm_packed_partials(c.x[:M], wp, sz, 128, bias)
    if (K, N) == (4096, 4096):  # narrow N, long K: the split-K form (the other two shapes may run unsplit: nothing to hand over)
        assert part is not None and part.num_slices >= 2, what
    if part is not None:
        eg.assert_bits_equal(part.finalize(), ref, f"{what} partials x{part.num_slices}", c.step)


@pytest.mark.parametrize("M,K,N", [(M, K, N) for K, N in _AWQ_SHAPES for M in (65, 128, 200)] + [(1024, 4096, 4096), (2100, 4096, 4096)])
def test_awq_gemm_packed_tiled_is_exact(M, K, N):
    """64-row tiles at the small shapes; 1024 and 2100 rows of 4096 x 4096 reach the 128-row tiles with three and two stages
    (256 and more than 512 tiles of 128 x 128)."""
    c, w, wp, sz, acc = _awq_shared(K, N)
    bias = c.bias if M % 2 else None
    ref = eg.round_once(acc[:M], FP16, bias, "awq_gemm_packed_tiled")
    out = ops.awq_gemm_packed_tiled(c.x[:M], wp, sz, 128, bias)
    eg.assert_bits_equal(out, ref, f"awq_gemm_packed_tiled M={M} K={K} N={N} bias={bias is not None}", c.step)
