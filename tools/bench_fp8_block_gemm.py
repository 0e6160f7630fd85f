"""Block-scaled FP8 GEMM (ops.fp8_blockwise_scaled_mm) against its per-channel twin (ops.fp8_scaled_mm) on the four
Llama-3-8B layer shapes: same weight and activation bytes, same run, alternating.

    python tools/bench_fp8_block_gemm.py [--out profiles/fp8_block_gemm.txt]

Times are device-event times per call over `--iters` back-to-back launches (median of `--rounds` alternating rounds, after a
warm-up of every shape); the operands are re-used, so a weight that fits the Infinity Cache is read from there by both."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sglang_npu_amd import ops  # noqa: E402

SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
ROWS = [1, 64, 1024, 4096]


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fp8_block_gemm.txt")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = ["# us per call, MI355X; block = fp8_blockwise_scaled_mm (128 x 128 weight blocks, 1 x 128 activation groups),",
             "# channel = fp8_scaled_mm (per token / per channel); both on the fragment-major weight, bf16 out",
             f"# median of {a.rounds} alternating rounds of {a.iters} launches",
             f"{'layer':8} {'N':>6} {'K':>6} {'M':>5} {'block us':>9} {'channel us':>10} {'ratio':>6}  kernels"]
    for name, N, K in SHAPES:
        w = ((torch.rand(N, K, device=dev, generator=g) - 0.5) * 8).to(torch.float8_e4m3fn)
        wf = ops.fp8_shuffle_weight(w)
        sb_blk = torch.rand(K // 128, N // 128, device=dev, generator=g) * 1e-2
        sb_ch = torch.rand(N, 1, device=dev, generator=g) * 1e-2
        for M in ROWS:
            x = ((torch.rand(M, K, device=dev, generator=g) - 0.5) * 8).to(torch.float8_e4m3fn)
            sa_blk = torch.rand(M, K // 128, device=dev, generator=g)
            sa_ch = torch.rand(M, 1, device=dev, generator=g)
            blk = lambda: ops.fp8_blockwise_scaled_mm(x, wf, sa_blk, sb_blk, torch.bfloat16)  # noqa: E731
            ch = lambda: ops.fp8_scaled_mm(x, wf, sa_ch, sb_ch, torch.bfloat16)  # noqa: E731
            blk()
            k_blk = ops.fp8_last_kernel()
            ch()
            k_ch = ops.fp8_last_kernel()
            timed(blk, 5), timed(ch, 5)
            tb, tc = [], []
            for _ in range(a.rounds):
                tb.append(timed(blk, a.iters))
                tc.append(timed(ch, a.iters))
            b, c = statistics.median(tb), statistics.median(tc)
            lines.append(f"{name:8} {N:6d} {K:6d} {M:5d} {b:9.1f} {c:10.1f} {b / c:6.2f}  {k_blk} / {k_ch}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
