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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--shapes", type=str, nargs="*", default=[f"{m}x{n}" for m, n in SHAPES])
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS], help="bits,rank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_backward_bench.txt"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_backward.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
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
