#!/usr/bin/env python
"""The dense-GEMM path of a packed layer (CalderaLinear.dense_prefill_tokens: cq_linear_dequant into a
shared fp16 scratch buffer, then the dense GEMM) against the packed prefill kernels it would replace,
same process, same GPU, with its two parts and a write-rate yardstick timed beside it.

Shapes 4096^2, 11008 x 4096, 4096 x 11008; 2-bit codes with r = 128 and 4-bit codes with r = 256.
Forward at T in {64, 512, 2048}, five graphs per point:
    packed        the layer as it stands (cq_linear_forward), the baseline
    dense path    the same layer with dense_prefill_tokens set
    materialise   cq_linear_dequant alone, into one fp16 buffer
    F.linear      on a resident dense fp16 weight: the GEMM alone
    copy          a device copy of one dense fp16 weight into that buffer: the same bytes written,
                  read from memory instead of decoded
Backward (dx only) at T in {512, 2048}, four graphs: the packed input gradient
(cq_linear_backward_input), the dense path's (materialise + dy16 @ W16), materialise alone, the
GEMM dy16 @ W alone.

Method (tools/bench_linear.py's): each timed unit is one pass over `copies` distinct layers of the
shape, enough that the packed weights alone exceed the Infinity Cache, captured once in a HIP graph;
the graphs of a point alternate; HIP events around each replay; median of the rounds divided by
`copies`, with the smallest and largest round beside it.  One JSON line per point, tables at the end,
everything also written to --out.
"""
from __future__ import annotations

import argparse
import copy as _copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_linear import CACHE_BYTES, CONFIGS, SHAPES, make_layer, replay_ms, timed_graph  # noqa: E402

TOKENS = (64, 512, 2048)
BWD_TOKENS = (512, 2048)
THRESHOLD = 17   # below every measured T: the dense path is taken whenever it is set


def _time(graphs, copies, rounds):
    for _ in range(2):
        for g in graphs:
            replay_ms(g)
    ts = [[] for _ in graphs]
    for _ in range(rounds):  # alternate
        for g, t in zip(graphs, ts):
            t.append(replay_ms(g) / copies)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def _fields(names, stats):
    out = {}
    for name, (med, lo, hi) in zip(names, stats):
        out[name + "_ms"], out[name + "_min_ms"], out[name + "_max_ms"] = med, lo, hi
    return out


def bench_shape(m, n, bits, r, tokens, bwd_tokens, dev, rounds, emit):
    import torch.nn.functional as F
    from ee274_convexcaldera_llm_quantization_amd import linear as LIN
    lin = make_layer(m, n, bits, r, dev, seed=m + n + bits)
    pbytes = lin.packed_bytes()
    copies = max(2, int(CACHE_BYTES // pbytes) + 1)
    layers = [lin] + [_copy.deepcopy(lin) for _ in range(copies - 1)]
    w16 = lin.materialize()
    ref = lin.dense_weight()
    rel_w = float((w16.float() - ref).norm() / ref.norm())
    assert rel_w < 1e-3, rel_w
    dense = [w16] + [w16.clone() for _ in range(copies - 1)]
    buf = torch.empty_like(w16)
    gen = torch.Generator(device=dev)

    def set_dense(on):
        for layer in layers:
            layer.dense_prefill_tokens = THRESHOLD if on else None

    g_mat = timed_graph(lambda i: layers[i].materialize(out=buf), copies)
    g_copy = timed_graph(lambda i: buf.copy_(dense[i]), copies)
    for T in tokens:
        x = torch.randn(T, n, device=dev, generator=gen.manual_seed(T)).half()
        set_dense(False)
        yp = layers[-1](x)
        gp = timed_graph(lambda i: layers[i](x), copies)
        set_dense(True)
        yd = layers[-1](x)
        gd = timed_graph(lambda i: layers[i](x), copies)
        set_dense(False)
        rel = float((yp.float() - yd.float()).norm() / yp.float().norm())
        assert rel < 2e-3, rel
        gl = timed_graph(lambda i: F.linear(x, dense[i]), copies)
        names = ("packed", "dense_path", "materialise", "gemm", "copy")
        res = dict(dir="fwd", m=m, n=n, bits=bits, r=r, T=T, copies=copies, packed_bytes=pbytes, dense_bytes=2 * m * n,
                   rel_diff=rel, **_fields(names, _time([gp, gd, g_mat, gl, g_copy], copies, rounds)))
        res["packed_over_dense_path"] = res["packed_ms"] / res["dense_path_ms"]
        res["materialise_over_copy"] = res["materialise_ms"] / res["copy_ms"]
        emit(res)
        del gp, gd, gl
    for T in bwd_tokens:
        dy = torch.randn(T, m, device=dev, generator=gen.manual_seed(T + 1)).half()
        x2 = torch.empty(T, n, device=dev, dtype=torch.float16)   # saved activations: not read for dx alone

        def dx_of(i):
            layer = layers[i]
            return LIN._packed_backward(layer, dy, x2, layer.L, layer.R, (True, False, False), torch.float16,
                                        (None, None))[0]

        set_dense(False)
        dp = dx_of(copies - 1)
        gp = timed_graph(dx_of, copies)
        set_dense(True)
        dd = dx_of(copies - 1)
        gd = timed_graph(dx_of, copies)
        set_dense(False)
        rel = float((dp.float() - dd.float()).norm() / dp.float().norm())
        assert rel < 2e-3, rel
        gl = timed_graph(lambda i: torch.mm(dy, dense[i]), copies)
        names = ("packed", "dense_path", "materialise", "gemm")
        res = dict(dir="bwd", m=m, n=n, bits=bits, r=r, T=T, copies=copies, packed_bytes=pbytes, dense_bytes=2 * m * n,
                   rel_diff=rel, **_fields(names, _time([gp, gd, g_mat, gl], copies, rounds)))
        res["packed_over_dense_path"] = res["packed_ms"] / res["dense_path_ms"]
        emit(res)
        del gp, gd, gl
    del g_mat, g_copy, layers, dense
    from ee274_convexcaldera_llm_quantization_amd import scratch
    scratch.release()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--bwd-tokens", type=int, nargs="*", default=list(BWD_TOKENS))
    ap.add_argument("--shapes", type=str, nargs="*", default=[f"{m}x{n}" for m, n in SHAPES])
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_dequant.txt"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_dequant.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    lines = ["# Dense-GEMM path of a packed layer (dense_prefill_tokens) against the packed prefill kernels, with",
             "# cq_linear_dequant alone, the dense GEMM alone and a device copy of one dense fp16 weight; one MI355X, one",
             f"# process, the graphs of a point alternating, median of {a.rounds} (smallest and largest beside it); ms per call:",
             "#   python tools/bench_linear_dequant.py"]
    rows = []

    def emit(res):
        rows.append(res)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    for shp in a.shapes:
        m, n = (int(v) for v in shp.split("x"))
        for bits, r in (tuple(int(v) for v in c.split(",")) for c in a.configs):
            bench_shape(m, n, bits, r, a.tokens, a.bwd_tokens, dev, a.rounds, emit)

    def cell(q, name):
        return f"{q[name + '_ms']:.4f} ({q[name + '_min_ms']:.4f}-{q[name + '_max_ms']:.4f})"

    table = ["", "Forward, ms per call: median (smallest-largest)", "",
             "| m x n | bits, r | T | packed | dense path | materialise | F.linear | copy | packed / dense path | "
             "materialise / copy |", "|---|---|---|---|---|---|---|---|---|---|"]
    for q in (q for q in rows if q["dir"] == "fwd"):
        table.append(f"| {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | {cell(q, 'packed')} | "
                     f"{cell(q, 'dense_path')} | {cell(q, 'materialise')} | {cell(q, 'gemm')} | {cell(q, 'copy')} | "
                     f"{q['packed_over_dense_path']:.2f} | {q['materialise_over_copy']:.2f} |")
    table += ["", "Backward (dx), ms per call: median (smallest-largest)", "",
              "| m x n | bits, r | T | packed | dense path | materialise | dy @ W | packed / dense path |",
              "|---|---|---|---|---|---|---|---|"]
    for q in (q for q in rows if q["dir"] == "bwd"):
        table.append(f"| {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | {cell(q, 'packed')} | "
                     f"{cell(q, 'dense_path')} | {cell(q, 'materialise')} | {cell(q, 'gemm')} | "
                     f"{q['packed_over_dense_path']:.2f} |")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")


if __name__ == "__main__":
    main()
