#!/usr/bin/env python
"""Hadamard-basis sets that share an input: HadamardLinearGroup (q / k / v) and HadamardGatedMLP.glu
(gate / up + silu + product) against the same layers each run alone; same process, same GPU.

Shapes: 3 x 4096 x 4096 (grouped) and 2 x 11008 x 4096 (padded 16384 x 4096; gated), each with 2-bit codes
and r = 128 and with 4-bit codes and r = 256, fp16 factors, fp16 activations; T in {1, 8, 16, 64, 512}.

Method (that of tools/bench_linear_group.py): each timed unit is one pass over `copies` distinct sets,
enough that the packed weights alone come to bench_linear.CACHE_BYTES = 600 MB, over twice the 256 MB
Infinity Cache, captured once in a HIP graph so that neither side pays host launch cost.  Baseline: every
layer of the set through its own forward (four launches each: transform, z, codes + L, transform) and, for
the gated set, F.silu and the product -- code this change leaves as it is.  Candidate: the group (four
launches) resp. the fused module's glu (four launches), on the very same layers.  Before anything is timed
the group's outputs are compared with the members' bit for bit, and the fused h with silu(v_g) v_u formed in
fp64 from the members' own fp32 outputs under the bar of tests/linear_glu_cases.py for an fp16 h
(8 2^-24 |h*| + 1e-37 + 2^-11 |h*| + 2^-25; where |h*| passes fp16's range -- column 0 of these random
weights -- h must be the overflow).  The two graphs alternate; HIP events around each replay; seven
rounds; per side the median, minimum and maximum of the time per set.

Gate: at T <= 16 a point fails unless the candidate's median lies below the baseline's minimum.  Prefill
points are reported with the same figures.  Prints one JSON line per point and a table, and writes both to
--out.
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

SETS = {"qkv": (3, 4096, 4096), "mlp": (2, 11008, 4096)}   # (layers, out_features, in_features)
CONFIGS = ((2, 128), (4, 256))   # (code bits, rank)
TOKENS = (1, 8, 16, 64, 512)
DECODE_MAX = 16


def make_set(count, m, n, bits, r, dev, seed):
    from bench_linear import make_layer
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardCalderaLinear
    pr, pc = 1 << (m - 1).bit_length(), 1 << (n - 1).bit_length()
    return [HadamardCalderaLinear(make_layer(pr, pc, bits, r, dev, seed=seed + 17 * i), n, m).to(dev)
            for i in range(count)]


def check_glu(mlp, x):
    """The fused fp16 h against silu(v_g) v_u from the members' fp32 outputs; returns worst error / bar."""
    h = mlp.glu(x)
    x32 = x.float()                                    # exact: the same x^, and the members return fp32
    vg, vu = mlp.gate_proj._forward_alone(x32), mlp.up_proj._forward_alone(x32)
    assert vg.dtype == torch.float32 and h.dtype == torch.float16
    hs = torch.nn.functional.silu(vg.double()) * vu.double()
    bar = (8 * 2.0 ** -24 + 2.0 ** -11) * hs.abs() + 1e-37 + 2.0 ** -25
    # the random weights' rows do not sum to zero, so column 0 of H1's output (the row sum / sqrt(pr)) is
    # two orders above the rest and its h can pass fp16's range: there h must be the overflow, not a number
    inside = hs.abs() < 65504.0
    worst = float(((h.double() - hs).abs() / bar)[inside].max())
    assert worst <= 1.0, f"fused h misses the bar: {worst} bars"
    assert bool((h[~inside].float().abs() >= 65504.0).all()), "fused h is finite where silu(v_g) v_u passes fp16's range"
    return worst


def bench_point(kind, sets, T, dev, rounds, meta):
    import torch.nn.functional as F
    from bench_linear import replay_ms, timed_graph
    from ee274_convexcaldera_llm_quantization_amd.linear import HadamardGatedMLP, HadamardLinearGroup
    copies = len(sets)
    n = sets[0][0].in_features
    x = torch.randn(T, n, device=dev, generator=torch.Generator(device=dev).manual_seed(T)).half()
    with torch.no_grad():
        if kind == "qkv":
            groups = [HadamardLinearGroup(s) for s in sets]
            cand = lambda i: groups[i](x)                                            # noqa: E731
            base = lambda i: [lin._forward_alone(x) for lin in sets[i]]              # noqa: E731
            for y, w in zip(cand(copies - 1), base(copies - 1)):
                assert torch.equal(y, w), "the group does not keep the members' bits"
            worst = 0.0
        else:
            groups = []
            mlps = [HadamardGatedMLP(g, u, torch.nn.Identity(), max_fused_tokens=None) for g, u in sets]
            cand = lambda i: mlps[i].glu(x)                                          # noqa: E731
            base = lambda i: F.silu(sets[i][0]._forward_alone(x)) * sets[i][1]._forward_alone(x)   # noqa: E731
            worst = check_glu(mlps[-1], x)
        gc = timed_graph(cand, copies)
        gb = timed_graph(base, copies)
    for _ in range(2):
        replay_ms(gc), replay_ms(gb)
    tc, tb = [], []
    for _ in range(rounds):  # alternate
        tc.append(replay_ms(gc) / copies)
        tb.append(replay_ms(gb) / copies)
    ms_c, ms_b = statistics.median(tc), statistics.median(tb)
    out = dict(meta, T=T, branch="decode" if T <= DECODE_MAX else "prefill", copies=copies, worst_error_in_bars=worst,
               candidate_ms=ms_c, candidate_min_ms=min(tc), candidate_max_ms=max(tc),
               baseline_ms=ms_b, baseline_min_ms=min(tb), baseline_max_ms=max(tb),
               speedup=ms_b / ms_c, below_baseline_min=bool(ms_c < min(tb)))
    for g in groups:
        g.dissolve()
    del gc, gb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--sets", type=str, nargs="*", default=list(SETS), help="qkv and / or mlp")
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS], help="bits,rank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hadamard_group_bench.txt"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hadamard_group.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    from bench_linear import CACHE_BYTES
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    lines = ["# Hadamard-basis sets: HadamardLinearGroup (q / k / v) and HadamardGatedMLP.glu (gate / up + silu + product)",
             "# against the same layers each run alone (+ F.silu + product); one MI355X, one process, HIP-graph replays",
             f"# over distinct sets beyond the Infinity Cache, the two graphs alternating, median of {a.rounds} with",
             "# min / max; ms per set:",
             "#   python tools/bench_hadamard_group.py"]
    rows = []
    for kind in a.sets:
        count, m, n = SETS[kind]
        for bits, r in (tuple(int(v) for v in c.split(",")) for c in a.configs):
            first = make_set(count, m, n, bits, r, dev, seed=m + n + bits)
            set_bytes = sum(lin.packed_bytes() for lin in first)
            copies = max(2, int(CACHE_BYTES // set_bytes) + 1)
            sets = [first] + [[copy.deepcopy(lin) for lin in first] for _ in range(copies - 1)]
            meta = dict(set=kind, layers=count, m=m, n=n, bits=bits, r=r, set_bytes=set_bytes)
            for T in a.tokens:
                res = bench_point(kind, sets, T, dev, a.rounds, meta)
                rows.append(res)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
            del sets, first
            torch.cuda.empty_cache()
    table = ["", "| set | bits, r | T | candidate us (min .. max) | baseline us (min .. max) | baseline / candidate | "
             "candidate median < baseline min |", "|---|---|---|---|---|---|---|"]
    for q in rows:
        table.append(f"| {q['layers']} x {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | "
                     f"{q['candidate_ms'] * 1e3:.2f} ({q['candidate_min_ms'] * 1e3:.2f} .. "
                     f"{q['candidate_max_ms'] * 1e3:.2f}) | "
                     f"{q['baseline_ms'] * 1e3:.2f} ({q['baseline_min_ms'] * 1e3:.2f} .. "
                     f"{q['baseline_max_ms'] * 1e3:.2f}) | {q['speedup']:.3f} | "
                     f"{'yes' if q['below_baseline_min'] else 'NO'} |")
    bad = [q for q in rows if q["T"] <= DECODE_MAX and not q["below_baseline_min"]]
    slow_prefill = [q for q in rows if q["T"] > DECODE_MAX and q["candidate_ms"] > q["baseline_ms"]]
    table.append("")
    table.append(f"T <= {DECODE_MAX}: {'every point passes the gate' if not bad else f'{len(bad)} point(s) FAIL the gate'}; "
                 f"prefill points slower than the baseline: {len(slow_prefill)}")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
