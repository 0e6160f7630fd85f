"""W8A8 INT8 GEMM (ops.int8_scaled_mm) beside the per-channel FP8 GEMM (ops.fp8_scaled_mm) on the four Llama-3-8B layer
shapes: the same number of weight and activation bytes, same run, alternating.

    python tools/bench_int8_gemm.py [--out profiles/int8_gemm.txt]

Times are device-event times per call over `--iters` back-to-back launches (median of `--rounds` alternating rounds, after a
warm-up of every shape); the operands are re-used, so a weight that fits the Infinity Cache is read from there by both.
The last column is the bound the INT8 call's time is a fraction of: weight + activation + output bytes at 8 TB/s up to 64
rows (`hbm`), 2 M N K operations at the dense 8-bit MFMA peak of 5 P op/s above (`mfma`)."""
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
    ap.add_argument("--out", default="profiles/int8_gemm.txt")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = ["# us per call, MI355X; int8 = int8_scaled_mm, fp8 = fp8_scaled_mm (both per token / per channel scales),",
             "# both on the fragment-major weight, bf16 out; share = bound / int8 time (hbm: bytes at 8 TB/s, mfma: ops at 5 P/s)",
             f"# median of {a.rounds} alternating rounds of {a.iters} launches",
             f"{'layer':8} {'N':>6} {'K':>6} {'M':>5} {'int8 us':>9} {'fp8 us':>9} {'ratio':>6} {'share':>10}  kernels"]
    for name, N, K in SHAPES:
        w8 = torch.randint(-128, 128, (N, K), device=dev, generator=g, dtype=torch.int8)
        wi = ops.int8_shuffle_weight(w8)
        wf = ops.fp8_shuffle_weight(((torch.rand(N, K, device=dev, generator=g) - 0.5) * 8).to(torch.float8_e4m3fn))
        sb = torch.rand(N, 1, device=dev, generator=g) * 1e-2
        for M in ROWS:
            xi = torch.randint(-128, 128, (M, K), device=dev, generator=g, dtype=torch.int8)
            xf = ((torch.rand(M, K, device=dev, generator=g) - 0.5) * 8).to(torch.float8_e4m3fn)
            sa = torch.rand(M, 1, device=dev, generator=g) * 1e-2
            i8 = lambda: ops.int8_scaled_mm(xi, wi, sa, sb, torch.bfloat16)  # noqa: E731
            f8 = lambda: ops.fp8_scaled_mm(xf, wf, sa, sb, torch.bfloat16)  # noqa: E731
            i8()
            f8()
            kernels = f"{ops.int8_last_kernel()} / {ops.fp8_last_kernel()}"
            timed(i8, 5), timed(f8, 5)
            ti, tf = [], []
            for _ in range(a.rounds):
                ti.append(timed(i8, a.iters))
                tf.append(timed(f8, a.iters))
            i, f = statistics.median(ti), statistics.median(tf)
            bound = ("hbm", (N * K + M * K + 2 * M * N) / 8e12) if M <= 64 else ("mfma", 2 * M * N * K / 5e15)
            lines.append(f"{name:8} {N:6d} {K:6d} {M:5d} {i:9.1f} {f:9.1f} {i / f:6.2f} {bound[1] * 1e6 / i:5.2f} {bound[0]:>4}  {kernels}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
