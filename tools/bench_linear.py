#!/usr/bin/env python
"""Packed linear forward (CalderaLinear / cq_linear_forward) against what a user does today:
torch.nn.functional.linear on the dense fp16 weight gs (Q + L R), same process, same GPU.

Shapes 4096^2, 11008 x 4096, 4096 x 11008; 2-bit codes with r = 128 and 4-bit codes with r = 256;
T in {1, 8, 16, 64, 512, 2048}.

Method: each timed unit is one pass over `copies` distinct layers of the shape (enough copies that
the packed weights alone exceed the 256 MB Infinity Cache, so neither side is served from cache,
as in a model whose layers follow one another), captured once in a HIP graph so that host launch
cost is the same for both (none).  Packed and dense passes alternate; HIP events around each
replay; the median over the rounds divided by `copies` is the time per call.  Algorithmic bytes =
codes + L + R + x + y for the packed layer (weight + x + y for the dense one); the fraction is of
the 6.3 TB/s streaming rate.  Prints one JSON line per point and a table at the end.

--factor-bits 2 | 4: L and R are uniform codes of that width with one scale each, and every point
times three graphs in the same process, alternating as above: the layer with its factors as
packed codes (cq_linear_packed_forward), the same layer with those factors stored as fp16
(cq_linear_forward, the path without this option) and the dense fp16 F.linear.  `copies` is
sized by the smaller, coded layer.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_BPS = 6.3e12
SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))
CONFIGS = ((2, 128), (4, 256))   # (code bits, rank)
TOKENS = (1, 8, 16, 64, 512, 2048)
CACHE_BYTES = 600e6


def make_layer(m, n, bits, r, dev, seed, factor_bits=0):
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, row_bytes
    g = torch.Generator(device=dev).manual_seed(seed)
    rb = row_bytes(n, bits)
    codes = torch.randint(0, 256, (m, rb), dtype=torch.uint8, device=dev, generator=g)
    if bits == 4:  # offset-binary 15 is not a code (k = 7: 0..14)
        codes = torch.where(codes & 0x0F == 0x0F, codes & 0xFE, codes)
        codes = torch.where(codes & 0xF0 == 0xF0, codes & 0xEF, codes)
    else:          # 3 is not a 2-bit code (k = 1: 0..2)
        for sh in (0, 2, 4, 6):
            codes = torch.where((codes >> sh) & 3 == 3, codes & (0xFF ^ (1 << sh)), codes)
    if factor_bits:
        # (coded layer, the same layer with its factors as fp16): L = (cL / k) s, entries up to 0.05
        from ee274_convexcaldera_llm_quantization_amd.linear import pack_rows
        k = 2 ** (factor_bits - 1) - 1
        cl = torch.randint(-k, k + 1, (m, r), device=dev, generator=g, dtype=torch.int8)
        cr = torch.randint(-k, k + 1, (r, n), device=dev, generator=g, dtype=torch.int8)
        kw = dict(qscale=0.05, gscale=1.3, bits=bits, in_features=n, out_features=m)
        coded = CalderaLinear(codes, None, None, None, L_codes=(pack_rows(cl, factor_bits), 0.05, factor_bits),
                              R_codes=(pack_rows(cr, factor_bits), 0.05, factor_bits), **kw)
        L, R = coded.factors()
        return coded, CalderaLinear(codes, L, R, None, **kw)
    L = (torch.randn(m, r, device=dev, generator=g) * 0.02).half()
    R = (torch.randn(r, n, device=dev, generator=g) * 0.02).half()
    return CalderaLinear(codes, L, R, None, qscale=0.05, gscale=1.3, bits=bits, in_features=n, out_features=m)


def timed_graph(fn, copies):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(min(copies, 2)):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(copies):
            fn(i)
    return graph


def replay_ms(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_point(m, n, bits, r, T, dev, rounds):
    import torch.nn.functional as F
    import copy as _copy
    lin = make_layer(m, n, bits, r, dev, seed=m + n + bits)
    pbytes = lin.packed_bytes()
    copies = max(2, int(CACHE_BYTES // pbytes) + 1)
    layers = [lin] + [_copy.deepcopy(lin) for _ in range(copies - 1)]
    w16 = lin.dense_weight().half()
    dense = [w16] + [w16.clone() for _ in range(copies - 1)]
    x = torch.randn(T, n, device=dev, generator=torch.Generator(device=dev).manual_seed(T)).half()
    # results agree before anything is timed
    yp, yd = layers[-1](x), F.linear(x, dense[-1])
    rel = float((yp.float() - yd.float()).norm() / yd.float().norm())
    assert rel < 2e-2, rel
    gp = timed_graph(lambda i: layers[i](x), copies)
    gd = timed_graph(lambda i: F.linear(x, dense[i]), copies)
    for _ in range(2):
        replay_ms(gp), replay_ms(gd)
    tp, td = [], []
    for _ in range(rounds):  # alternate
        tp.append(replay_ms(gp) / copies)
        td.append(replay_ms(gd) / copies)
    ms_p, ms_d = statistics.median(tp), statistics.median(td)
    io = 2 * T * n + 2 * T * m
    bytes_p, bytes_d = pbytes + io, 2 * m * n + io
    out = dict(m=m, n=n, bits=bits, r=r, T=T, branch="decode" if T <= 16 else "prefill", copies=copies,
               packed_ms=ms_p, dense_ms=ms_d, packed_min_ms=min(tp), dense_min_ms=min(td),
               packed_bytes=bytes_p, dense_bytes=bytes_d,
               packed_frac_stream=bytes_p / (ms_p * 1e-3) / STREAM_BPS,
               dense_frac_stream=bytes_d / (ms_d * 1e-3) / STREAM_BPS,
               speedup=ms_d / ms_p, rel_diff=rel)
    del gp, gd, layers, dense
    torch.cuda.empty_cache()
    return out


def bench_factor_point(m, n, bits, r, T, dev, rounds, factor_bits):
    """Coded factors vs the same layer with fp16 factors vs dense fp16, one process, alternating."""
    import torch.nn.functional as F
    import copy as _copy
    coded, plain = make_layer(m, n, bits, r, dev, seed=m + n + bits, factor_bits=factor_bits)
    cbytes, pbytes = coded.packed_bytes(), plain.packed_bytes()
    copies = max(2, int(CACHE_BYTES // cbytes) + 1)
    lc = [coded] + [_copy.deepcopy(coded) for _ in range(copies - 1)]
    lp = [plain] + [_copy.deepcopy(plain) for _ in range(copies - 1)]
    w16 = coded.dense_weight().half()
    dense = [w16] + [w16.clone() for _ in range(copies - 1)]
    x = torch.randn(T, n, device=dev, generator=torch.Generator(device=dev).manual_seed(T)).half()
    yc, yp, yd = lc[-1](x), lp[-1](x), F.linear(x, dense[-1])
    rel = float((yc.float() - yd.float()).norm() / yd.float().norm())
    rel_p = float((yc.float() - yp.float()).norm() / yp.float().norm())
    assert rel < 2e-2 and rel_p < 2e-3, (rel, rel_p)
    graphs = [timed_graph(lambda i: lc[i](x), copies), timed_graph(lambda i: lp[i](x), copies),
              timed_graph(lambda i: F.linear(x, dense[i]), copies)]
    for _ in range(2):
        for g in graphs:
            replay_ms(g)
    ts = [[], [], []]
    for _ in range(rounds):  # alternate
        for g, t in zip(graphs, ts):
            t.append(replay_ms(g) / copies)
    ms_c, ms_p, ms_d = (statistics.median(t) for t in ts)
    io = 2 * T * n + 2 * T * m
    out = dict(m=m, n=n, bits=bits, r=r, factor_bits=factor_bits, T=T, branch="decode" if T <= 16 else "prefill",
               copies=copies, coded_ms=ms_c, fp16_factors_ms=ms_p, dense_ms=ms_d, coded_min_ms=min(ts[0]),
               fp16_factors_min_ms=min(ts[1]), dense_min_ms=min(ts[2]), coded_bytes=cbytes + io,
               fp16_factors_bytes=pbytes + io, dense_bytes=2 * m * n + io,
               coded_frac_stream=(cbytes + io) / (ms_c * 1e-3) / STREAM_BPS,
               fp16_factors_frac_stream=(pbytes + io) / (ms_p * 1e-3) / STREAM_BPS,
               speedup_vs_fp16_factors=ms_p / ms_c, speedup_vs_dense=ms_d / ms_c, rel_diff=rel,
               rel_diff_fp16_factors=rel_p)
    del graphs, lc, lp, dense
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--shapes", type=str, nargs="*", default=[f"{m}x{n}" for m, n in SHAPES])
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS], help="bits,rank")
    ap.add_argument("--factor-bits", type=int, default=0, choices=(0, 2, 4),
                    help="L and R as uniform codes of this width: coded vs fp16 factors vs dense (0: fp16 factors only)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    rows = []
    for shp in a.shapes:
        m, n = (int(v) for v in shp.split("x"))
        for bits, r in (tuple(int(v) for v in c.split(",")) for c in a.configs):
            for T in a.tokens:
                if a.factor_bits:
                    res = bench_factor_point(m, n, bits, r, T, dev, a.rounds, a.factor_bits)
                else:
                    res = bench_point(m, n, bits, r, T, dev, a.rounds)
                rows.append(res)
                print(json.dumps(res), flush=True)
    if a.factor_bits:
        print(f"\n| m x n | bits, r | T | {a.factor_bits}-bit factors ms | fp16 factors ms | dense fp16 ms | fp16 factors / coded "
              "| dense / coded | coded MB | fp16-factor MB | coded % of 6.3 TB/s | fp16 factors % of 6.3 TB/s |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|")
        for q in rows:
            print(f"| {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | {q['coded_ms']:.4f} | "
                  f"{q['fp16_factors_ms']:.4f} | {q['dense_ms']:.4f} | {q['speedup_vs_fp16_factors']:.2f} | "
                  f"{q['speedup_vs_dense']:.2f} | {q['coded_bytes'] / 1e6:.1f} | {q['fp16_factors_bytes'] / 1e6:.1f} | "
                  f"{100 * q['coded_frac_stream']:.1f} | {100 * q['fp16_factors_frac_stream']:.1f} |")
        return
    print("\n| m x n | bits, r | T | packed ms | dense fp16 ms | dense / packed | packed MB | packed % of 6.3 TB/s |"
          " dense % of 6.3 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for q in rows:
        print(f"| {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | {q['packed_ms']:.4f} | {q['dense_ms']:.4f} | "
              f"{q['speedup']:.2f} | {q['packed_bytes'] / 1e6:.1f} | {100 * q['packed_frac_stream']:.1f} | "
              f"{100 * q['dense_frac_stream']:.1f} |")


if __name__ == "__main__":
    main()
