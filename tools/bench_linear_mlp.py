#!/usr/bin/env python
"""Fused gated pair (CalderaGatedMLP.glu / cq_linear_glu_forward) against the best unfused path: the
grouped gate / up launch pair (CalderaLinearGroup), then F.silu, then the product; same process, same GPU.

Shape: gate / up of 11008 x 4096; 2-bit codes with r = 128 and 4-bit codes with r = 256, fp16 factors,
fp16 activations; T in {1, 8, 16, 64, 512, 2048}.

Method (that of tools/bench_linear_group.py): each timed unit is one pass over `copies` distinct pairs,
enough that the packed weights alone come to bench_linear.CACHE_BYTES = 600 MB, over twice the 256 MB
Infinity Cache, captured once in a HIP graph so that neither side pays host launch cost.  The fused graph
holds one cq_linear_glu_forward per pair (two launches), the baseline graph one cq_linear_group_forward
(two launches) and the two elementwise torch launches, on the very same layers.  Before anything is timed
the fused h is compared with silu(v_g) v_u formed in fp64 from the members' own fp32 outputs, under the bar
of tests/linear_glu_cases.py for an fp16 h (8 2^-24 |h*| + 1e-37 + 2^-11 |h*| + 2^-25).  The two graphs
alternate; HIP events around each replay; seven rounds; per side the median, minimum and maximum of the
time per pair.

Gate: at T <= 16 a point fails unless the fused median lies below the baseline's minimum.  Prefill points
are reported with the same figures.  Prints one JSON line per point and a table, and writes both to --out.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPE = (11008, 4096)
CONFIGS = ((2, 128), (4, 256))   # (code bits, rank)
TOKENS = (1, 8, 16, 64, 512, 2048)
DECODE_MAX = 16


def check_outputs(mlp, x):
    """The fused fp16 h against silu(v_g) v_u from the members' fp32 outputs; returns worst error / bar."""
    h = mlp.glu(x)
    x32 = x.float()                                    # the layers cast back to fp16 (exact) and return fp32
    vg, vu = mlp.gate_proj._forward_alone(x32), mlp.up_proj._forward_alone(x32)
    assert vg.dtype == torch.float32 and h.dtype == torch.float16
    hs = torch.nn.functional.silu(vg.double()) * vu.double()
    bar = (8 * 2.0 ** -24 + 2.0 ** -11) * hs.abs() + 1e-37 + 2.0 ** -25
    worst = float(((h.double() - hs).abs() / bar).max())
    assert worst <= 1.0, f"fused h misses the bar: {worst} bars"
    return worst


def bench_point(bits, r, T, dev, rounds):
    import torch.nn.functional as F
    from bench_linear import CACHE_BYTES, make_layer, replay_ms, timed_graph
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaGatedMLP, CalderaLinearGroup
    m, n = SHAPE
    first = [make_layer(m, n, bits, r, dev, seed=m + n + bits + 17 * i) for i in range(2)]
    pair_bytes = sum(lin.packed_bytes() for lin in first)
    copies = max(2, int(CACHE_BYTES // pair_bytes) + 1)
    pairs = [first] + [[copy.deepcopy(lin) for lin in first] for _ in range(copies - 1)]
    # max_fused_tokens=None: the fused launch at every T, also where the module's default limit falls back
    mlps = [CalderaGatedMLP(g, u, torch.nn.Identity(), max_fused_tokens=None) for g, u in pairs]
    groups = [CalderaLinearGroup(p) for p in pairs]      # the fused path neither uses nor disturbs them
    x = torch.randn(T, n, device=dev, generator=torch.Generator(device=dev).manual_seed(T)).half()

    def baseline(i):
        g, u = groups[i](x)
        return F.silu(g) * u

    with torch.no_grad():
        worst = check_outputs(mlps[-1], x)
        gf = timed_graph(lambda i: mlps[i].glu(x), copies)
        gb = timed_graph(baseline, copies)
    for _ in range(2):
        replay_ms(gf), replay_ms(gb)
    tf, tb = [], []
    for _ in range(rounds):  # alternate
        tf.append(replay_ms(gf) / copies)
        tb.append(replay_ms(gb) / copies)
    ms_f, ms_b = statistics.median(tf), statistics.median(tb)
    out = dict(m=m, n=n, bits=bits, r=r, T=T, branch="decode" if T <= DECODE_MAX else "prefill", copies=copies,
               pair_bytes=pair_bytes, worst_error_in_bars=worst,
               fused_ms=ms_f, fused_min_ms=min(tf), fused_max_ms=max(tf),
               baseline_ms=ms_b, baseline_min_ms=min(tb), baseline_max_ms=max(tb),
               speedup=ms_b / ms_f, below_baseline_min=bool(ms_f < min(tb)))
    for g in groups:
        g.dissolve()
    del gf, gb, groups, mlps, pairs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS], help="bits,rank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_mlp_bench.txt"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_mlp.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    lines = ["# Fused gated pair (one cq_linear_glu_forward) against the grouped gate / up launch pair + F.silu + product",
             "# on the same layers; one MI355X, one process, HIP-graph replays over distinct pairs beyond the Infinity",
             f"# Cache, the two graphs alternating, median of {a.rounds} with min / max; ms per pair:",
             "#   python tools/bench_linear_mlp.py"]
    rows = []
    for bits, r in (tuple(int(v) for v in c.split(",")) for c in a.configs):
        for T in a.tokens:
            res = bench_point(bits, r, T, dev, a.rounds)
            rows.append(res)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    table = ["", "| pair | bits, r | T | fused us (min .. max) | baseline us (min .. max) | baseline / fused | "
             "fused median < baseline min |", "|---|---|---|---|---|---|---|"]
    for q in rows:
        table.append(f"| 2 x {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | "
                     f"{q['fused_ms'] * 1e3:.2f} ({q['fused_min_ms'] * 1e3:.2f} .. {q['fused_max_ms'] * 1e3:.2f}) | "
                     f"{q['baseline_ms'] * 1e3:.2f} ({q['baseline_min_ms'] * 1e3:.2f} .. "
                     f"{q['baseline_max_ms'] * 1e3:.2f}) | {q['speedup']:.3f} | "
                     f"{'yes' if q['below_baseline_min'] else 'NO'} |")
    bad = [q for q in rows if q["T"] <= DECODE_MAX and not q["below_baseline_min"]]
    slow_prefill = [q for q in rows if q["T"] > DECODE_MAX and q["fused_ms"] > q["baseline_ms"]]
    table.append("")
    table.append(f"T <= {DECODE_MAX}: {'every point passes the gate' if not bad else f'{len(bad)} point(s) FAIL the gate'}; "
                 f"prefill points slower fused: {len(slow_prefill)}")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
