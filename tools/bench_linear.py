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

--hadamard: the layer decomposed in the Hadamard basis (HadamardCalderaLinear: cq_hadamard_rows, the
packed layer of the padded shape, cq_hadamard_rows).  Shapes 4096^2 and 4096 x 11008 (padded to
4096 x 16384), 2-bit, r = 128.  Every point times five graphs in the same process, alternating as
above: the Hadamard layer; the plain CalderaLinear of the padded shape (its inner layer alone, on
the padded fp16 x); dense fp16 F.linear on the m x n weight; the two transform launches alone; the
same two transforms as fp16 matmuls x @ H with dense normalised Hadamard matrices (distinct copies
of H up to the cache size, so H comes from memory like the weights).  Written to --out (default
profiles/linear_forward_hadamard.txt) as well as printed.
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


HADAMARD_SHAPES = ((4096, 4096), (4096, 11008))


def bench_hadamard_point(m, n, bits, r, T, dev, rounds):
    """Hadamard layer, its inner layer alone, dense fp16, the two transforms alone, and the two
    transforms as dense fp16 matmuls; one process, alternating."""
    import torch.nn.functional as F
    import copy as _copy
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    from ee274_convexcaldera_llm_quantization_amd.model import normalized_hadamard
    pr, pc = 1 << (m - 1).bit_length(), 1 << (n - 1).bit_length()
    had = HadamardCalderaLinear(make_layer(pr, pc, bits, r, dev, seed=m + n + bits), n, m, None)
    pbytes = had.packed_bytes()
    copies = max(2, int(CACHE_BYTES // pbytes) + 1)
    layers = [had] + [_copy.deepcopy(had) for _ in range(copies - 1)]
    w16 = had.dense_weight().half()
    dense = [w16] + [w16.clone() for _ in range(copies - 1)]
    g = torch.Generator(device=dev).manual_seed(T)
    x = torch.randn(T, n, device=dev, generator=g).half()
    xpad = torch.zeros(T, pc, device=dev, dtype=torch.float16)
    xpad[:, :n] = x
    yh, yd = layers[-1](x), F.linear(x, dense[-1])
    rel = float((yh.float() - yd.float()).norm() / yd.float().norm())
    assert rel < 2e-2, rel
    # the transforms alone, on preallocated buffers: x -> xh (fp16), y32 -> y (fp16)
    xh = torch.empty(T, pc, device=dev, dtype=torch.float16)
    y32 = torch.randn(T, pr, device=dev, generator=g)
    y = torch.empty(T, m, device=dev, dtype=torch.float16)

    def transforms(i):
        K.hadamard_rows(x, xh, n_in=n, n_out=pc, P=pc)
        K.hadamard_rows(y32, y, n_in=pr, n_out=m, P=pr)

    # the same as matmuls with dense H (fp16; symmetric); distinct copies up to the cache size
    def h_copies(P):
        H = normalized_hadamard(P, dev).half()
        k = min(copies, max(1, int(CACHE_BYTES // (2 * P * P)) + 1))
        return [H] + [H.clone() for _ in range(k - 1)]

    H2s, H1s = h_copies(pc), h_copies(pr)
    y16 = y32.half()
    ref = (xpad.float() @ H2s[0].float())
    got = torch.empty_like(xh)
    K.hadamard_rows(x, got, n_in=n, n_out=pc, P=pc)
    assert float((got.float() - ref).norm() / ref.norm()) < 2e-3

    def matmuls(i):
        torch.matmul(xpad, H2s[i % len(H2s)])
        torch.matmul(y16, H1s[i % len(H1s)])

    graphs = [timed_graph(lambda i: layers[i](x), copies), timed_graph(lambda i: layers[i].inner(xpad), copies),
              timed_graph(lambda i: F.linear(x, dense[i]), copies), timed_graph(transforms, copies),
              timed_graph(matmuls, copies)]
    for _ in range(2):
        for gr in graphs:
            replay_ms(gr)
    ts = [[] for _ in graphs]
    for _ in range(rounds):  # alternate
        for gr, t in zip(graphs, ts):
            t.append(replay_ms(gr) / copies)
    ms = [statistics.median(t) for t in ts]
    out = dict(m=m, n=n, pr=pr, pc=pc, bits=bits, r=r, T=T, branch="decode" if T <= 16 else "prefill", copies=copies,
               h_copies=[len(H2s), len(H1s)], hadamard_ms=ms[0], padded_plain_ms=ms[1], dense_ms=ms[2],
               transforms_ms=ms[3], matmul_transforms_ms=ms[4], hadamard_min_ms=min(ts[0]),
               padded_plain_min_ms=min(ts[1]), dense_min_ms=min(ts[2]), transforms_min_ms=min(ts[3]),
               matmul_transforms_min_ms=min(ts[4]), packed_bytes=pbytes, dense_bytes=2 * m * n,
               hadamard_over_plain=ms[0] / ms[1], dense_over_hadamard=ms[2] / ms[0],
               matmul_over_kernel=ms[4] / ms[3], rel_diff=rel)
    del graphs, layers, dense, H2s, H1s
    torch.cuda.empty_cache()
    return out


def hadamard_main(a, dev):
    lines = ["# Packed layer in the Hadamard basis (HadamardCalderaLinear) against the plain CalderaLinear of the padded",
             "# shape, dense fp16 F.linear, its two cq_hadamard_rows launches alone and the same two transforms as fp16",
             "# matmuls with dense H; one MI355X, one process, the five graphs alternating, median of "
             f"{a.rounds}; ms per call:",
             "#   python tools/bench_linear.py --hadamard"]
    rows = []
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes]
    configs = [tuple(int(v) for v in c.split(",")) for c in a.configs]
    for m, n in shapes:
        for bits, r in configs:
            for T in a.tokens:
                res = bench_hadamard_point(m, n, bits, r, T, dev, a.rounds)
                rows.append(res)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
    table = ["", "| m x n (padded) | bits, r | T | Hadamard layer ms | padded plain ms | dense fp16 ms | 2 transforms ms | "
             "2 matmul transforms ms | Hadamard / plain | dense / Hadamard | matmul / kernel |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for q in rows:
        table.append(f"| {q['m']} x {q['n']} ({q['pr']} x {q['pc']}) | {q['bits']}, {q['r']} | {q['T']} | "
                     f"{q['hadamard_ms']:.4f} | {q['padded_plain_ms']:.4f} | {q['dense_ms']:.4f} | "
                     f"{q['transforms_ms']:.4f} | {q['matmul_transforms_ms']:.4f} | {q['hadamard_over_plain']:.2f} | "
                     f"{q['dense_over_hadamard']:.2f} | {q['matmul_over_kernel']:.2f} |")
    gate = [q for q in rows if (q["pr"], q["pc"], q["T"]) == (4096, 4096, 1)]
    for q in gate:
        verdict = "faster than" if q["transforms_ms"] < q["matmul_transforms_ms"] else "NOT faster than"
        table.append(f"\nT = 1, P = 4096: the two transform launches take {q['transforms_ms'] * 1e3:.2f} us, "
                     f"{verdict} the two fp16 x @ H matmuls on dense 32 MB H ({q['matmul_transforms_ms'] * 1e3:.2f} us).")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--shapes", type=str, nargs="*", default=None,
                    help=f"m x n (default {' '.join(f'{m}x{n}' for m, n in SHAPES)}; --hadamard: "
                         f"{' '.join(f'{m}x{n}' for m, n in HADAMARD_SHAPES)})")
    ap.add_argument("--configs", type=str, nargs="*", default=None,
                    help=f"bits,rank (default {' '.join(f'{b},{r}' for b, r in CONFIGS)}; --hadamard: 2,128)")
    ap.add_argument("--factor-bits", type=int, default=0, choices=(0, 2, 4),
                    help="L and R as uniform codes of this width: coded vs fp16 factors vs dense (0: fp16 factors only)")
    ap.add_argument("--hadamard", action="store_true",
                    help="the Hadamard-basis layer against the padded plain layer, dense fp16 and the transforms alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_forward_hadamard.txt"),
                    help="where --hadamard writes its lines and table")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    hshapes, hconfigs = (HADAMARD_SHAPES, ((2, 128),)) if a.hadamard else (SHAPES, CONFIGS)
    if a.shapes is None:
        a.shapes = [f"{m}x{n}" for m, n in hshapes]
    if a.configs is None:
        a.configs = [f"{b},{r}" for b, r in hconfigs]
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    if a.hadamard:
        return hadamard_main(a, dev)
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
