#!/usr/bin/env python
"""Grouped packed forward (CalderaLinearGroup / cq_linear_group_forward) against the same layers called
one after the other through their own single-layer entries, same process, same GPU.

Sets: q/k/v (3 x 4096 x 4096) and gate/up (2 x 11008 x 4096); 2-bit codes with r = 128 and 4-bit codes
with r = 256, fp16 factors; T in {1, 8, 16, 64, 512}.

Method (that of tools/bench_linear.py): each timed unit is one pass over `copies` distinct sets, enough
that the packed weights alone come to bench_linear.CACHE_BYTES = 600 MB, over twice the 256 MB Infinity
Cache, captured once in a HIP graph so that neither side pays host launch cost.  The grouped graph holds one cq_linear_group_forward per set (two
launches), the other graph each member's own entry (two launches per member) on the very same
layers -- the single-layer entries, which the grouped code does not change; the outputs are compared
bit for bit before anything is timed.  The two graphs alternate; HIP events around each replay; seven
rounds; per side the median, minimum, maximum and spread (max - min) of the time per set.

Gate: at T <= 16 a point fails when the grouped median exceeds the ungrouped median by more than the
ungrouped side's own spread.  Prefill points are reported with the same figure.  Prints one JSON line
per point and a table, and writes both to --out.
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

SETS = {"qkv": ((4096, 4096),) * 3, "gate_up": ((11008, 4096),) * 2}
CONFIGS = ((2, 128), (4, 256))   # (code bits, rank)
TOKENS = (1, 8, 16, 64, 512)
DECODE_MAX = 16


def bench_point(name, bits, r, T, dev, rounds):
    from bench_linear import CACHE_BYTES, make_layer, replay_ms, timed_graph
    from ee274_convexcaldera_llm_quantization_amd.linear import CalderaLinearGroup
    first = [make_layer(m, n, bits, r, dev, seed=m + n + bits + 17 * i) for i, (m, n) in enumerate(SETS[name])]
    set_bytes = sum(lin.packed_bytes() for lin in first)
    copies = max(2, int(CACHE_BYTES // set_bytes) + 1)
    sets = [first] + [[copy.deepcopy(lin) for lin in first] for _ in range(copies - 1)]
    groups = [CalderaLinearGroup(layers) for layers in sets]
    n = SETS[name][0][1]
    x = torch.randn(T, n, device=dev, generator=torch.Generator(device=dev).manual_seed(T)).half()
    with torch.no_grad():
        # the same bits before anything is timed
        for yg, lin in zip(groups[-1](x), sets[-1]):
            assert torch.equal(yg, lin._forward_alone(x))
        gg = timed_graph(lambda i: groups[i](x), copies)
        gu = timed_graph(lambda i: [lin._forward_alone(x) for lin in sets[i]], copies)
    for _ in range(2):
        replay_ms(gg), replay_ms(gu)
    tg, tu = [], []
    for _ in range(rounds):  # alternate
        tg.append(replay_ms(gg) / copies)
        tu.append(replay_ms(gu) / copies)
    ms_g, ms_u = statistics.median(tg), statistics.median(tu)
    spread_u = max(tu) - min(tu)
    out = dict(set=name, members=len(first), m=SETS[name][0][0], n=n, bits=bits, r=r, T=T,
               branch="decode" if T <= DECODE_MAX else "prefill", copies=copies, set_bytes=set_bytes,
               grouped_ms=ms_g, grouped_min_ms=min(tg), grouped_max_ms=max(tg), grouped_spread_ms=max(tg) - min(tg),
               ungrouped_ms=ms_u, ungrouped_min_ms=min(tu), ungrouped_max_ms=max(tu), ungrouped_spread_ms=spread_u,
               speedup=ms_u / ms_g, slower_by_ms=ms_g - ms_u, within_gate=bool(ms_g - ms_u <= spread_u))
    for g in groups:
        g.dissolve()
    del gg, gu, groups, sets
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=list(TOKENS))
    ap.add_argument("--sets", type=str, nargs="*", default=list(SETS), choices=list(SETS))
    ap.add_argument("--configs", type=str, nargs="*", default=[f"{b},{r}" for b, r in CONFIGS], help="bits,rank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_group_bench.txt"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_group.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    lines = ["# Grouped packed forward (one cq_linear_group_forward per set) against the same layers through their own",
             "# single-layer entries; one MI355X, one process, HIP-graph replays over distinct sets beyond the Infinity",
             f"# Cache, the two graphs alternating, median of {a.rounds} with min / max; ms per set:",
             "#   python tools/bench_linear_group.py"]
    rows = []
    for name in a.sets:
        for bits, r in (tuple(int(v) for v in c.split(",")) for c in a.configs):
            for T in a.tokens:
                res = bench_point(name, bits, r, T, dev, a.rounds)
                rows.append(res)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
    table = ["", "| set | bits, r | T | grouped us (min .. max) | ungrouped us (min .. max) | ungrouped / grouped | "
             "grouped - ungrouped us | ungrouped spread us | within gate |", "|---|---|---|---|---|---|---|---|---|"]
    for q in rows:
        table.append(f"| {q['members']} x {q['m']} x {q['n']} | {q['bits']}, {q['r']} | {q['T']} | "
                     f"{q['grouped_ms'] * 1e3:.2f} ({q['grouped_min_ms'] * 1e3:.2f} .. {q['grouped_max_ms'] * 1e3:.2f}) | "
                     f"{q['ungrouped_ms'] * 1e3:.2f} ({q['ungrouped_min_ms'] * 1e3:.2f} .. "
                     f"{q['ungrouped_max_ms'] * 1e3:.2f}) | {q['speedup']:.3f} | {q['slower_by_ms'] * 1e3:+.2f} | "
                     f"{q['ungrouped_spread_ms'] * 1e3:.2f} | {'yes' if q['within_gate'] else 'NO'} |")
    bad = [q for q in rows if q["T"] <= DECODE_MAX and not q["within_gate"]]
    slow_prefill = [q for q in rows if q["T"] > DECODE_MAX and not q["within_gate"]]
    table.append("")
    table.append(f"T <= {DECODE_MAX}: {'every point within the gate' if not bad else f'{len(bad)} point(s) OUTSIDE the gate'}; "
                 f"prefill points slower grouped by more than the ungrouped spread: {len(slow_prefill)}")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
