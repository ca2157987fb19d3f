"""Time model.hadamard_transform by the FWHT kernels (kernels=True) against the two dense fp32 GEMMs
(kernels=False) on an MI355X: 4096 x 4096 and 11008 x 4096 fp16 weights, plain and signed, forward and
inverse.  The two paths alternate in one process after warm-up; each figure is the median of `--reps` device-
event timings.  GB/s is against the algorithmic bytes of the kernel path: one read of W, one write and one
read of the (m, pc) fp32 intermediate, one write of the result, plus one write and one read of the rows of the
column transform's workspace that its two passes touch when pr > 256 (forward: the blocks of 256 rows that
hold a row of W; inverse: all pr).  Peak memory is what one call allocates above the operands with the
scratch cache released first, so the kernel path's figure includes its workspace; `kernel_held_MiB` is the
workspace that stays cached after the call.  Prints one JSON line per case and fails when the
kernel path at 11008 x 4096 is less than `--bar` times faster than the GEMM path of the same run.

    python tools/bench_hadamard_weight.py [--reps 10] [--bar 4]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ee274_convexcaldera_llm_quantization_amd import model as M  # noqa: E402
from ee274_convexcaldera_llm_quantization_amd import scratch  # noqa: E402
from ee274_convexcaldera_llm_quantization_amd.linear import hadamard_sign_vector  # noqa: E402

HBM_GBS = 8000.0  # MI355X nominal HBM3E rate


def algorithmic_bytes(m, n, inverse, w_bytes):
    pr, pc = M._next_pow2(m), M._next_pow2(n)
    ends = pr * pc * 4 + m * n * (4 if inverse else w_bytes)    # the padded fp32 matrix and W (fp32 when recovered)
    ws_rows = pr if inverse else -(-m // 256) * 256             # pass 1 skips the blocks of 256 rows past n_in
    return ends + 2 * m * pc * 4 + (2 * ws_rows * pc * 4 if pr > 256 else 0)


def call_memory(fn):
    """(MiB one call allocates at its peak, MiB still held afterwards) with nothing cached beforehand."""
    scratch.release()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    held = torch.cuda.memory_allocated() - base - out.numel() * out.element_size()
    return peak / 2 ** 20, held / 2 ** 20


def timed(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bar", type=float, default=4.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (a CPU run measures nothing)"
    dev, worst = "cuda:0", None
    for m, n in ((4096, 4096), (11008, 4096)):
        W = (0.02 * torch.randn(m, n, generator=torch.Generator().manual_seed(0))).half().to(dev)
        for signed in (False, True):
            signs = (hadamard_sign_vector(1, m), hadamard_sign_vector(2, n)) if signed else None
            Wt, shp = M.hadamard_transform(W, signs=signs, kernels=True)
            for inverse in (False, True):
                def run(kernels):
                    if inverse:
                        return M.hadamard_transform(Wt, inverse=True, original_shape=shp, signs=signs, kernels=kernels)
                    return M.hadamard_transform(W, signs=signs, kernels=kernels)[0]
                a, b = run(False), run(True)  # warm-up of both paths, and the difference between them
                diff = float((a - b).norm() / a.norm())
                del a, b
                t = {False: [], True: []}
                for _ in range(args.reps):  # alternate the two paths
                    for kernels in (False, True):
                        torch.cuda.synchronize()
                        t[kernels] += timed(lambda: run(kernels), 1)
                peak = {kernels: call_memory(lambda: run(kernels)) for kernels in (False, True)}
                ms_g, ms_k = statistics.median(t[False]), statistics.median(t[True])
                gbs = algorithmic_bytes(m, n, inverse, 2) / ms_k / 1e6
                ratio = ms_g / ms_k
                print(json.dumps(dict(shape=[m, n], signed=signed, inverse=inverse, gemm_ms=round(ms_g, 3),
                                      kernel_ms=round(ms_k, 3), speedup=round(ratio, 2), kernel_GBps=round(gbs, 1),
                                      hbm_fraction=round(gbs / HBM_GBS, 3), gemm_peak_MiB=round(peak[False][0]),
                                      kernel_peak_MiB=round(peak[True][0]), kernel_held_MiB=round(peak[True][1]),
                                      rel_diff=diff)), flush=True)
                if m == 11008:
                    worst = ratio if worst is None else min(worst, ratio)
    print(json.dumps(dict(bar=args.bar, worst_speedup_11008x4096=round(worst, 2), passed=worst >= args.bar)))
    return 0 if worst >= args.bar else 1


if __name__ == "__main__":
    sys.exit(main())
