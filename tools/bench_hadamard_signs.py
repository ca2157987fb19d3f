#!/usr/bin/env python
"""cq_hadamard_rows of this tree against the same entry of another build (--lib, e.g. the parent revision from
tools/probes/build_rev_lib.sh), and cq_hadamard_signed_rows beside it; same process, same GPU.

Shapes: P = 4096, T in {1, 512}, the two transforms of a 4096 x 4096 Hadamard-basis layer: "in" (fp16 x ->
fp16 x^) and "out" (fp32 inner output + bias -> fp16 y).  The signed entry runs "in" with sign_in and "out"
with sign_out, as the layer does.

Method: a timed unit is one pass over `copies` distinct (x, y) pairs, enough that a pass moves 600 MB at
T = 512 (over twice the Infinity Cache; at T = 1 a pass is 256 launches of 16 KB rows: launch-bound, which
is what a decode step pays), captured once in a HIP graph per variant.  Variants: the other build twice
("other", "other again": the spread of repeated runs of one code object), this tree's unsigned entry, the
signed entry.  The graphs alternate, HIP events around each replay, --rounds rounds after two warm-up
rounds; per variant the median, minimum and maximum of the time per call.  Before anything is timed the
tree's unsigned output is compared with the other build's bit for bit, and the signed one with the unsigned
entry on the flipped input / its flipped output.  One JSON line per point, a table, both written to --out.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 4096
TOKENS = (1, 512)
PASS_BYTES = 600e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="another build of libcaldera_hip.so (ABI 5)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hadamard_signs_bench.txt"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hadamard_signs.py needs a HIP device (no CPU timing)")
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    from bench_linear import replay_ms, timed_graph
    from ee274_convexcaldera_llm_quantization_amd.linear import hadamard_sign_vector
    K.load()
    other = ctypes.CDLL(os.path.abspath(a.lib))
    other.cq_abi_version.restype = ctypes.c_int
    assert other.cq_abi_version() == K.ABI_VERSION, "the other build speaks another ABI"
    other.cq_hadamard_rows.restype = ctypes.c_int
    other.cq_hadamard_rows.argtypes = [ctypes.POINTER(K.HadamardArgs), ctypes.c_void_p]
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    signs = hadamard_sign_vector(7, P).to(dev)
    pm = signs.float()
    bias = torch.randn(P, device=dev, generator=gen)

    def other_rows(x, y, b):
        args = K.hadamard_args(x, y, n_in=P, n_out=P, P=P, bias=b)
        st = other.cq_hadamard_rows(ctypes.byref(args), K._stream(x.device))
        assert st == 0, st

    lines = ["# cq_hadamard_rows, this tree against --lib, and cq_hadamard_signed_rows; P = 4096; one MI355X, one",
             f"# process, HIP-graph replays over distinct buffers, the graphs alternating, median of {a.rounds} with",
             "# min / max; us per call:", "#   python tools/bench_hadamard_signs.py --lib <other build>"]
    rows = []
    for form, xdt, b in (("in", torch.float16, None), ("out", torch.float32, bias)):
        for T in TOKENS:
            per_call = T * P * (xdt.itemsize + 2)
            copies = 256 if T == 1 else max(2, int(PASS_BYTES // per_call) + 1)
            xs = [torch.randn(T, P, device=dev, generator=gen).to(xdt) for _ in range(copies)]
            ys = [torch.empty(T, P, dtype=torch.float16, device=dev) for _ in range(copies)]
            skw = dict(sign_in=signs) if form == "in" else dict(sign_out=signs)
            variants = {
                "other": lambda i: other_rows(xs[i], ys[i], b),
                "other again": lambda i: other_rows(xs[i], ys[i], b),
                "tree": lambda i: K.hadamard_rows(xs[i], ys[i], n_in=P, n_out=P, P=P, bias=b),
                "signed": lambda i: K.hadamard_signed_rows(xs[i], ys[i], n_in=P, n_out=P, P=P, bias=b, **skw),
            }
            # results agree before anything is timed
            y_o, y_t, y_s = (torch.empty_like(ys[0]) for _ in range(3))
            other_rows(xs[0], y_o, b)
            K.hadamard_rows(xs[0], y_t, n_in=P, n_out=P, P=P, bias=b)
            assert torch.equal(y_o, y_t), "this tree's unsigned entry does not keep the other build's bits"
            K.hadamard_signed_rows(xs[0], y_s, n_in=P, n_out=P, P=P, **skw)
            want = torch.empty_like(y_s)
            if form == "in":
                K.hadamard_rows(xs[0] * pm.to(xdt), want, n_in=P, n_out=P, P=P)
            else:
                K.hadamard_rows(xs[0], want, n_in=P, n_out=P, P=P)
                want = want * pm.half()
            assert torch.equal(y_s, want), "the signed entry is not the unsigned one between flips"
            graphs = {name: timed_graph(fn, copies) for name, fn in variants.items()}
            times = {name: [] for name in graphs}
            for r in range(a.rounds + 2):
                for name, g in graphs.items():
                    t = replay_ms(g) * 1e3 / copies
                    if r >= 2:
                        times[name].append(t)
            res = dict(form=form, T=T, P=P, copies=copies, bytes_per_call=per_call)
            for name, ts in times.items():
                key = name.replace(" ", "_")
                res.update({f"{key}_us": statistics.median(ts), f"{key}_min_us": min(ts), f"{key}_max_us": max(ts)})
            rows.append(res)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            del graphs, xs, ys
            torch.cuda.empty_cache()
    table = ["", "| form | T | other us (min .. max) | other again | tree, unsigned | tree, signed |", "|---|---|---|---|---|---|"]
    for q in rows:
        cell = lambda k: f"{q[k + '_us']:.2f} ({q[k + '_min_us']:.2f} .. {q[k + '_max_us']:.2f})"  # noqa: E731
        table.append(f"| {q['form']} | {q['T']} | {cell('other')} | {cell('other_again')} | {cell('tree')} | {cell('signed')} |")
    print("\n".join(table))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
