"""NVFP4 weight-only GEMM (ops.nvfp4_gemm, prepared layout) on the four Llama-3-8B layer shapes beside the other ways this
backend runs the same layer: the AWQ INT4 kernels (ops.awq_gemm_packed up to 64 rows, ops.awq_gemm_packed_tiled above) and
the 16-bit weight (ops.linear16 on the fragment-major copy up to 128 rows, F.linear above).  Same run, alternating.

    python tools/bench_nvfp4_gemm.py [--out profiles/nvfp4_gemm.txt]

Times are device-event times per call over `--iters` back-to-back launches (median of `--rounds` alternating rounds, after a
warm-up of every shape); the operands are re-used, so a weight that fits the Infinity Cache is read from there by all.
`hbm` is the fraction of 8 TB/s the NVFP4 call reaches on K N 0.5625 + activation + output bytes."""
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
    ap.add_argument("--out", default="profiles/nvfp4_gemm.txt")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = ["# us per call, MI355X; fp4 = nvfp4_gemm (prepared layout) with fp16 / bf16 activations; awq = awq_gemm_packed (M <= 64) /",
             "# awq_gemm_packed_tiled, fp16, group 128; w16 = linear16 on the fragment-major bf16 weight (M <= 128) / F.linear;",
             "# hbm = (K N 0.5625 + 2 M K + 2 M N) bytes / 8 TB/s / fp4-f16 time",
             f"# median of {a.rounds} alternating rounds of {a.iters} launches",
             f"{'layer':8} {'N':>6} {'K':>6} {'M':>5} {'fp4 f16':>9} {'fp4 bf16':>9} {'awq':>9} {'w16':>9} {'hbm':>6}  kernel"]
    for name, N, K in SHAPES:
        weight = torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8)
        scale = (torch.rand(N, K // 16, device=dev, generator=g) + 0.5).to(torch.float8_e4m3fn)
        w4, s4 = ops.nvfp4_repack(weight, scale)
        ws2 = torch.tensor(1e-3, device=dev)
        wp, sz = ops.awq_repack(torch.randint(0, 2 ** 31 - 1, (K, N // 8), device=dev, generator=g, dtype=torch.int32),
                                (torch.rand(K // 128, N, device=dev, generator=g) * 1e-2).half(),
                                torch.randint(0, 2 ** 31 - 1, (K // 128, N // 8), device=dev, generator=g, dtype=torch.int32))
        w16 = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).bfloat16()
        w16s = ops.linear16_shuffle_weight(w16)
        for M in ROWS:
            xh = torch.randn(M, K, device=dev, generator=g).half()
            xb = xh.bfloat16()
            fns = [lambda: ops.nvfp4_gemm(xh, w4, s4, ws2), lambda: ops.nvfp4_gemm(xb, w4, s4, ws2),
                   (lambda: ops.awq_gemm_packed(xh, wp, sz, 128)) if M <= 64 else (lambda: ops.awq_gemm_packed_tiled(xh, wp, sz, 128)),
                   (lambda: ops.linear16(xb, w16s)) if M <= 128 else (lambda: torch.nn.functional.linear(xb, w16))]
            for fn in fns:
                fn()
                timed(fn, 5)
            fns[0]()
            kernel = ops.nvfp4_last_kernel()
            t = [[] for _ in fns]
            for _ in range(a.rounds):
                for i, fn in enumerate(fns):
                    t[i].append(timed(fn, a.iters))
            m = [statistics.median(x) for x in t]
            hbm = (K * N * 0.5625 + 2 * M * K + 2 * M * N) / 8e12 * 1e6 / m[0]
            lines.append(f"{name:8} {N:6d} {K:6d} {M:5d} {m[0]:9.1f} {m[1]:9.1f} {m[2]:9.1f} {m[3]:9.1f} {hbm:6.2f}  {kernel}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
