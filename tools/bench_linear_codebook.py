#!/usr/bin/env python
"""NF4 / NF2 codebook Q (cq_linear_codebook_forward) beside the uniform packed layer
(cq_linear_forward) of the same shape, bits and rank: both stream the same bytes, so the uniform
layer is the yardstick and the difference is the table decode.

Shapes 4096^2, 11008 x 4096, 4096 x 11008; 2-bit with r = 128 (NF2) and 4-bit with r = 256 (NF4);
T in {1, 8, 16, 64, 512, 2048}.  Method of tools/bench_linear.py: a timed unit is one pass over
`copies` distinct layers (their weights exceed the Infinity Cache), captured in a HIP graph; the
uniform and the NF pass alternate in one process; HIP events around each replay; median of the
rounds, divided by `copies`.  `spread` is max - min of the uniform layer's own samples: at T <= 16 an
NF excess beyond it is a cost of the decode, not noise.  Prints one JSON line per point and a
table, and writes both to --out (default profiles/linear_codebook_bench.txt).
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

from bench_linear import CACHE_BYTES, CONFIGS, SHAPES, STREAM_BPS, TOKENS, make_layer, replay_ms, timed_graph  # noqa: E402


def make_nf_layer(uniform, dev, seed):
    """The NF layer beside `uniform`: random level indices in the same bytes, the same factors."""
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinear, Q_FORMAT_NF
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    codes = torch.randint(0, 256, tuple(uniform.codes.shape), dtype=torch.uint8, device=dev, generator=g)
    return CalderaLinear(codes, uniform.L, uniform.R, None, qscale=0.05, gscale=1.3, bits=uniform.bits,
                         in_features=uniform.in_features, out_features=uniform.out_features, q_format=Q_FORMAT_NF)


def bench_point(m, n, bits, r, T, dev, rounds):
    import torch.nn.functional as F
    uni = make_layer(m, n, bits, r, dev, seed=m + n + bits)
    nf = make_nf_layer(uni, dev, seed=m + n + bits)
    assert nf.packed_bytes() == uni.packed_bytes()
    pbytes = uni.packed_bytes()
    copies = max(2, int(CACHE_BYTES // pbytes) + 1)
    lu = [uni] + [_copy.deepcopy(uni) for _ in range(copies - 1)]
    ln = [nf] + [_copy.deepcopy(nf) for _ in range(copies - 1)]
    x = torch.randn(T, n, device=dev, generator=torch.Generator(device=dev).manual_seed(T)).half()
    # the NF result agrees with its dense weight before anything is timed
    yn, yd = ln[-1](x), F.linear(x, nf.dense_weight().half())
    rel = float((yn.float() - yd.float()).norm() / yd.float().norm())
    assert rel < 2e-2, rel
    gu = timed_graph(lambda i: lu[i](x), copies)
    gn = timed_graph(lambda i: ln[i](x), copies)
    for _ in range(2):
        replay_ms(gu), replay_ms(gn)
    tu, tn = [], []
    for _ in range(rounds):  # alternate
        tu.append(replay_ms(gu) / copies)
        tn.append(replay_ms(gn) / copies)
    ms_u, ms_n = statistics.median(tu), statistics.median(tn)
    nbytes = pbytes + 2 * T * n + 2 * T * m
    out = dict(m=m, n=n, bits=bits, r=r, T=T, branch="decode" if T <= 16 else "prefill", copies=copies,
               uniform_ms=ms_u, nf_ms=ms_n, uniform_min_ms=min(tu), uniform_max_ms=max(tu), nf_min_ms=min(tn),
               nf_max_ms=max(tn), uniform_spread_ms=max(tu) - min(tu), excess_ms=ms_n - ms_u, nf_over_uniform=ms_n / ms_u,
               bytes=nbytes, uniform_frac_stream=nbytes / (ms_u * 1e-3) / STREAM_BPS,
               nf_frac_stream=nbytes / (ms_n * 1e-3) / STREAM_BPS, rel_diff=rel)
    del gu, gn, lu, ln
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--shapes", type=str, nargs="*", default=[f"{m}x{n}" for m, n in SHAPES])
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS], help="bits,rank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_codebook_bench.txt"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_codebook.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    lines = ["# NF codebook Q (cq_linear_codebook_forward) beside the uniform packed layer (cq_linear_forward), same",
             f"# shape, bits, rank and bytes; one MI355X, one process, the two graphs alternating, median of {a.rounds};",
             "# ms per call:", "#   python tools/bench_linear_codebook.py"]
    rows = []
    for shp in a.shapes:
        m, n = (int(v) for v in shp.split("x"))
        for bits, r in (tuple(int(v) for v in c.split(",")) for c in a.configs):
            for T in a.tokens:
                res = bench_point(m, n, bits, r, T, dev, a.rounds)
                rows.append(res)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
    table = ["", "| m x n | Q, r | T | uniform ms | NF ms | NF / uniform | excess us | uniform spread us | uniform % of 6.3 TB/s "
             "| NF % of 6.3 TB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for q in rows:
        table.append(f"| {q['m']} x {q['n']} | NF{q['bits']}, {q['r']} | {q['T']} | {q['uniform_ms']:.4f} | {q['nf_ms']:.4f} | "
                     f"{q['nf_over_uniform']:.3f} | {q['excess_ms'] * 1e3:.2f} | {q['uniform_spread_ms'] * 1e3:.2f} | "
                     f"{100 * q['uniform_frac_stream']:.1f} | {100 * q['nf_frac_stream']:.1f} |")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")


if __name__ == "__main__":
    main()
