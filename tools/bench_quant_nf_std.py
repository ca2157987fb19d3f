"""Micro-benchmark of the standardised NF quantiser (cq_quantize_nf_std) against the absmax NF
quantiser (cq_quantize_nf) at the engine's call form: B whole-matrix blocks of fp32, idx + deq +
weighted error.  The two entries are timed in the same process, alternating, after a warm-up, with
device events; the figures are medians over the rounds.

Algorithmic bytes per element: 13 for the absmax form (x read twice, idx 1, deq 4), 17 for the
standardised form with its two statistics passes (x read three times), 13 if it had one.
Bar: t(nf_std) <= (17 / 13) * 1.10 * t(nf), both measured in this run.

Usage: python tools/bench_quant_nf_std.py [B] [rounds]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import ee274_convexcaldera_llm_quantization_amd._lib as K

HBM_ACHIEVABLE = 6.3e12  # bytes/s
dev = "cuda:0"
K.load()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
BITS = 4


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


ok = True
for m, n in ((4096, 4096), (4096, 11008)):
    numel = m * n
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, numel, device=dev, generator=g) * 0.02
    w = torch.rand(n, device=dev, generator=g) + 0.5
    err = torch.empty(B, dtype=torch.float64, device=dev)

    def std_form():
        K.quantize_nf_std(x, numel, BITS, err_w=w, err_ncols=n, err_out=err)

    def absmax_form():
        K.quantize_nf(x, numel, BITS, err_w=w, err_ncols=n, err_out=err)

    for _ in range(2):
        std_form()
        absmax_form()
    torch.cuda.synchronize()
    ts, ta = [], []
    for _ in range(ROUNDS):
        ts.append(timed(std_form))
        ta.append(timed(absmax_form))
    t_std, t_abs = statistics.median(ts), statistics.median(ta)
    elems = B * numel
    bar = 17 / 13 * 1.10
    met = t_std <= bar * t_abs
    ok = ok and met
    print(f"B={B} {m}x{n} fp32 whole-matrix, nf{BITS}, idx + deq + error, median of {ROUNDS}:")
    print(f"  cq_quantize_nf_std {t_std * 1e3:8.3f} ms  {17 * elems / t_std / 1e12:5.2f} TB/s at 17 B/element "
          f"({17 * elems / t_std / HBM_ACHIEVABLE:.0%} of 6.3 TB/s); min {min(ts) * 1e3:.3f} max {max(ts) * 1e3:.3f}")
    print(f"  cq_quantize_nf     {t_abs * 1e3:8.3f} ms  {13 * elems / t_abs / 1e12:5.2f} TB/s at 13 B/element "
          f"({13 * elems / t_abs / HBM_ACHIEVABLE:.0%} of 6.3 TB/s); min {min(ta) * 1e3:.3f} max {max(ta) * 1e3:.3f}")
    print(f"  ratio {t_std / t_abs:.3f}, bar (17 / 13) * 1.10 = {bar:.3f}: {'met' if met else 'MISSED'}", flush=True)
    del x, w, err
print("bar met at every shape" if ok else "bar MISSED")
