#!/usr/bin/env python
"""Packed linear input gradient (cq_linear_backward_input: dx = dy (gs (Q + L R)) from the codes)
against torch.matmul(dy, dense_weight().half()) in the same process, and against the same run's
forward prefill launch (cq_linear_forward) of the same layer.

Shapes 4096^2 and 11008 x 4096; 2-bit codes with r = 128 and 4-bit codes with r = 256; T = 512 and
2048 (the fine-tuning regime).

Method (tools/bench_linear.py's): each timed unit is one pass over `copies` distinct layers of the
shape (enough copies that the packed weights alone exceed the 256 MB Infinity Cache), captured
once in a HIP graph; the three graphs alternate; HIP events around each replay; the median over
the rounds divided by `copies` is the time per call.  Prints one JSON line per point and a table,
and writes both to --out (default profiles/linear_backward_bench.txt).  Recorded, not gated.

--factor-bits {2, 4}: the backward of the layer with L and R as codes of that width
(cq_linear_packed_backward_input) beside the backward of the same layer with its factors as fp16
(cq_linear_backward_input, the entry and kernels the fp16-factor layer has always taken), same run,
two graphs alternating.  --hadamard: the Hadamard layer's backward (transform, inner input
gradient, transform; what its autograd function launches) beside the plain padded layer's input
gradient alone.  Both append to --out (default profiles/linear_backward_packed_bench.txt).
"""
from __future__ import annotations

import argparse
import copy as _copy
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_linear import CACHE_BYTES, make_layer, replay_ms, timed_graph  # noqa: E402

SHAPES = ((4096, 4096), (11008, 4096))
CONFIGS = ((2, 128), (4, 256))   # (code bits, rank)
TOKENS = (512, 2048)


def bench_point(m, n, bits, r, T, dev, rounds):
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    lin = make_layer(m, n, bits, r, dev, seed=m + n + bits)
    pbytes = lin.packed_bytes()
    copies = max(2, int(CACHE_BYTES // pbytes) + 1)
    layers = [lin] + [_copy.deepcopy(lin) for _ in range(copies - 1)]
    w16 = lin.dense_weight().half()
    dense = [w16] + [w16.clone() for _ in range(copies - 1)]
    g = torch.Generator(device=dev).manual_seed(T)
    dy = torch.randn(T, m, device=dev, generator=g).half()
    x = torch.randn(T, n, device=dev, generator=g).half()
    dx = torch.empty(T, n, device=dev, dtype=torch.float16)
    a = K.linear_backward_args(dy, lin.codes, lin.qscale, lin.gscale, lin.L, lin.R, dx, m=m, n=n, bits=bits)
    ws = K.workspace(K.load().cq_linear_backward_workspace(ctypes.byref(a)), dev)

    def backward(i):
        q = layers[i]
        K.linear_backward_input(dy, q.codes, q.qscale, q.gscale, q.L, q.R, dx, m=m, n=n, bits=bits, ws=ws)

    # results agree before anything is timed
    backward(copies - 1)
    ref = torch.matmul(dy, dense[-1])
    rel = float((dx.float() - ref.float()).norm() / ref.float().norm())
    assert rel < 2e-2, rel
    graphs = [timed_graph(backward, copies), timed_graph(lambda i: torch.matmul(dy, dense[i]), copies),
              timed_graph(lambda i: layers[i](x), copies)]
    for _ in range(2):
        for gr in graphs:
            replay_ms(gr)
    ts = [[] for _ in graphs]
    for _ in range(rounds):  # alternate
        for gr, t in zip(graphs, ts):
            t.append(replay_ms(gr) / copies)
    ms_b, ms_d, ms_f = (statistics.median(t) for t in ts)
    flops = 2.0 * T * (m * n + r * (m + n))
    out = dict(m=m, n=n, bits=bits, r=r, T=T, copies=copies, backward_ms=ms_b, dense_ms=ms_d, forward_ms=ms_f,
               backward_min_ms=min(ts[0]), dense_min_ms=min(ts[1]), forward_min_ms=min(ts[2]),
               backward_tflops=flops / (ms_b * 1e-3) / 1e12, backward_over_dense=ms_b / ms_d,
               backward_over_forward=ms_b / ms_f, packed_bytes=pbytes, dense_bytes=2 * m * n,
               workspace_bytes=int(ws.numel()), rel_diff=rel)
    del graphs, layers, dense
    torch.cuda.empty_cache()
    return out


def _alternate(graphs, copies, rounds):
    """Median and minimum ms per call of each graph, the graphs alternating."""
    for _ in range(2):
        for gr in graphs:
            replay_ms(gr)
    ts = [[] for _ in graphs]
    for _ in range(rounds):
        for gr, t in zip(graphs, ts):
            t.append(replay_ms(gr) / copies)
    return [statistics.median(t) for t in ts], [min(t) for t in ts]


def bench_factor_point(m, n, bits, r, T, dev, rounds, factor_bits):
    """The coded-factor backward beside the fp16-factor backward of the same layer."""
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    coded, plain = make_layer(m, n, bits, r, dev, seed=m + n + bits, factor_bits=factor_bits)
    copies = max(2, int(CACHE_BYTES // coded.packed_bytes()) + 1)
    lc = [coded] + [_copy.deepcopy(coded) for _ in range(copies - 1)]
    lp = [plain] + [_copy.deepcopy(plain) for _ in range(copies - 1)]
    dy = torch.randn(T, m, device=dev, generator=torch.Generator(device=dev).manual_seed(T)).half()
    dxc, dxp = (torch.empty(T, n, device=dev, dtype=torch.float16) for _ in range(2))
    a = K.linear_backward_args(dy, plain.codes, plain.qscale, plain.gscale, plain.L, plain.R, dxp, m=m, n=n, bits=bits)
    ws = K.workspace(K.load().cq_linear_backward_workspace(ctypes.byref(a)), dev)

    def back_coded(i):
        q = lc[i]
        K.linear_packed_backward_input(dy, q.codes, q.qscale, q.gscale, None, None, dxc, m=m, n=n, bits=bits, r=r,
                                       L_codes=(q.L_codes, q.lscale, q.L_bits), R_codes=(q.R_codes, q.rscale, q.R_bits),
                                       ws=ws)

    def back_plain(i):
        q = lp[i]
        K.linear_backward_input(dy, q.codes, q.qscale, q.gscale, q.L, q.R, dxp, m=m, n=n, bits=bits, ws=ws)

    back_coded(copies - 1), back_plain(copies - 1)
    rel = float((dxc.float() - dxp.float()).norm() / dxp.float().norm())
    assert rel < 2e-2, rel       # the fp16 factors are the codes' values rounded to fp16
    (ms_c, ms_p), (min_c, min_p) = _alternate([timed_graph(back_coded, copies), timed_graph(back_plain, copies)],
                                               copies, rounds)
    out = dict(m=m, n=n, bits=bits, r=r, factor_bits=factor_bits, T=T, copies=copies, coded_ms=ms_c, fp16_ms=ms_p,
               coded_min_ms=min_c, fp16_min_ms=min_p, coded_over_fp16=ms_c / ms_p, coded_bytes=coded.packed_bytes(),
               fp16_bytes=plain.packed_bytes(), rel_diff=rel)
    del lc, lp
    torch.cuda.empty_cache()
    return out


def bench_hadamard_point(m, n, bits, r, T, dev, rounds):
    """The Hadamard layer's backward beside the plain padded layer's input gradient."""
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    pr, pc = 1 << (m - 1).bit_length(), 1 << (n - 1).bit_length()
    had = HadamardCalderaLinear(make_layer(pr, pc, bits, r, dev, seed=m + n + bits), n, m, None)
    copies = max(2, int(CACHE_BYTES // had.packed_bytes()) + 1)
    layers = [had] + [_copy.deepcopy(had) for _ in range(copies - 1)]
    g = torch.Generator(device=dev).manual_seed(T)
    dy = torch.randn(T, m, device=dev, generator=g).half()
    dyh = torch.empty(T, pr, device=dev, dtype=torch.float16)
    dxh = torch.empty(T, pc, device=dev, dtype=torch.float32)
    dx = torch.empty(T, n, device=dev, dtype=torch.float16)
    q0 = had.inner
    a = K.linear_backward_args(dyh, q0.codes, q0.qscale, q0.gscale, q0.L, q0.R, dxh, m=pr, n=pc, bits=bits)
    ws = K.workspace(K.load().cq_linear_backward_workspace(ctypes.byref(a)), dev)

    def inner_only(i):
        q = layers[i].inner
        K.linear_backward_input(dyh, q.codes, q.qscale, q.gscale, q.L, q.R, dxh, m=pr, n=pc, bits=bits, ws=ws)

    def back_had(i):      # the launches of the layer's autograd backward
        K.hadamard_rows(dy, dyh, n_in=m, n_out=pr, P=pr)
        inner_only(i)
        K.hadamard_rows(dxh, dx, n_in=pc, n_out=n, P=pc)

    def transforms(i):
        K.hadamard_rows(dy, dyh, n_in=m, n_out=pr, P=pr)
        K.hadamard_rows(dxh, dx, n_in=pc, n_out=n, P=pc)

    # the hand-launched sequence is what autograd runs
    x = torch.randn(T, n, device=dev, generator=g).half().requires_grad_()
    had(x).backward(dy)
    back_had(0)
    assert torch.equal(x.grad, dx)
    (ms_h, ms_i, ms_t), mins = _alternate([timed_graph(f, copies) for f in (back_had, inner_only, transforms)],
                                          copies, rounds)
    out = dict(m=m, n=n, pr=pr, pc=pc, bits=bits, r=r, T=T, copies=copies, hadamard_ms=ms_h, inner_ms=ms_i,
               transforms_ms=ms_t, hadamard_min_ms=mins[0], inner_min_ms=mins[1], transforms_min_ms=mins[2],
               hadamard_over_inner=ms_h / ms_i)
    del layers
    torch.cuda.empty_cache()
    return out


def packed_main(a, dev):
    """--factor-bits / --hadamard: lines and table appended to a.out."""
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes]
    configs = [tuple(int(v) for v in c.split(",")) for c in a.configs]
    points = [(m, n, bits, r, T) for m, n in shapes for bits, r in configs for T in a.tokens]
    if a.hadamard:
        lines = ["# Backward of the Hadamard-basis layer (cq_hadamard_rows, cq_linear_backward_input on the padded grid,",
                 "# cq_hadamard_rows; fp16 dy and dx) against the plain padded layer's input gradient alone and the two",
                 f"# transforms alone; one MI355X, one process, the three graphs alternating, median of {a.rounds}; ms per call:",
                 "#   python tools/bench_linear_backward.py --hadamard"]
        rows = [bench_hadamard_point(*p, dev, a.rounds) for p in points]
        table = ["", "| m x n | padded | bits, r | T | Hadamard backward ms | padded layer backward ms | transforms ms | "
                 "Hadamard / padded |", "|---|---|---|---|---|---|---|---|"]
        table += [f"| {q['m']} x {q['n']} | {q['pr']} x {q['pc']} | {q['bits']}, {q['r']} | {q['T']} | "
                  f"{q['hadamard_ms']:.4f} | {q['inner_ms']:.4f} | {q['transforms_ms']:.4f} | "
                  f"{q['hadamard_over_inner']:.2f} |" for q in rows]
    else:
        lines = [f"# Input gradient with {a.factor_bits}-bit L and R codes (cq_linear_packed_backward_input, fp16 dx) against "
                 "the same layer with",
                 "# fp16 factors (cq_linear_backward_input); one MI355X, one process, the two graphs alternating, median of "
                 f"{a.rounds}; ms per call:",
                 f"#   python tools/bench_linear_backward.py --factor-bits {a.factor_bits}"]
        rows = [bench_factor_point(*p, dev, a.rounds, a.factor_bits) for p in points]
        table = ["", "| m x n | bits, r | factor bits | T | coded backward ms | fp16-factor backward ms | coded / fp16 | "
                 "coded MB | fp16-factor MB |", "|---|---|---|---|---|---|---|---|---|"]
        table += [f"| {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['factor_bits']} | {q['T']} | {q['coded_ms']:.4f} | "
                  f"{q['fp16_ms']:.4f} | {q['coded_over_fp16']:.2f} | {q['coded_bytes'] / 1e6:.1f} | "
                  f"{q['fp16_bytes'] / 1e6:.1f} |" for q in rows]
    lines += [json.dumps(q) for q in rows]
    print("\n".join(lines + table), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines + table) + "\n\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--shapes", type=str, nargs="*", default=[f"{m}x{n}" for m, n in SHAPES])
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS], help="bits,rank")
    ap.add_argument("--factor-bits", type=int, default=0, choices=(0, 2, 4),
                    help="L and R as uniform codes of this width: the coded backward beside the fp16-factor backward")
    ap.add_argument("--hadamard", action="store_true",
                    help="the Hadamard layer's backward beside the plain padded layer's input gradient")
    ap.add_argument("--out", default=None, help="default profiles/linear_backward_bench.txt; with --factor-bits or "
                                                "--hadamard profiles/linear_backward_packed_bench.txt, appended to")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_backward.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    packed = a.factor_bits or a.hadamard
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "linear_backward_packed_bench.txt" if packed else "linear_backward_bench.txt")
    if packed:
        return packed_main(a, dev)
    lines = ["# Packed linear input gradient (cq_linear_backward_input, fp16 dx) against torch.matmul(dy, dense fp16 W) and",
             "# the forward prefill launch of the same layer; one MI355X, one process, the three graphs alternating,",
             f"# median of {a.rounds}; ms per call:",
             "#   python tools/bench_linear_backward.py"]
    rows = []
    for shp in a.shapes:
        m, n = (int(v) for v in shp.split("x"))
        for bits, r in (tuple(int(v) for v in c.split(",")) for c in a.configs):
            for T in a.tokens:
                res = bench_point(m, n, bits, r, T, dev, a.rounds)
                rows.append(res)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
    table = ["", "| m x n | bits, r | T | backward ms | dense fp16 dy W ms | forward prefill ms | backward / dense | "
             "backward / forward | backward TFLOP/s | packed MB | dense MB | workspace MB |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for q in rows:
        table.append(f"| {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | {q['backward_ms']:.4f} | "
                     f"{q['dense_ms']:.4f} | {q['forward_ms']:.4f} | {q['backward_over_dense']:.2f} | "
                     f"{q['backward_over_forward']:.2f} | {q['backward_tflops']:.1f} | {q['packed_bytes'] / 1e6:.1f} | "
                     f"{q['dense_bytes'] / 1e6:.1f} | {q['workspace_bytes'] / 1e6:.2f} |")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")


if __name__ == "__main__":
    main()
