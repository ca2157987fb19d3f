"""Probe (no product change): how does sgram_spmm's time split between the sweep and the phases
around it?  Times it at the bench shape on the real ELL and with every slice width set to 0
(staging and output pass only; results wrong by design, timing only), one HIP-event pair per
repetition, and prints a checksum of the real P for comparing two builds.

  python tools/probe_spmm_phases.py [B] [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ee274_convexcaldera_llm_quantization_amd")]
import torch  # noqa: E402

import ee274_convexcaldera_llm_quantization_amd._lib as K  # noqa: E402
from ee274_convexcaldera_llm_quantization_amd import scratch, sgram  # noqa: E402

dev = "cuda:0"
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
m = n = 4096
g = torch.Generator(device=dev).manual_seed(0)
W = torch.empty(B, m, n, device=dev, dtype=torch.float16)
for b in range(B):
    W[b] = torch.randn(m, n, device=dev, generator=g).half()
packed = torch.empty(B, m * n // 4, dtype=torch.uint8, device=dev)
s = torch.empty(B, device=dev)
K.q_update_x3(W, None, None, 2, packed=packed, scale=s)
SG = sgram.SparseGram(B, m, n, dev)
SG.count(packed)
stride = -(-int(max(sgram.MAX_DENSITY, SG.density) * m * n) // 4096) * 4096
ell = scratch.get("sgram.ell", (B * stride,), torch.int32, dev)
P = scratch.get("sgram.P", (B, m, m), torch.float32, dev)
K.sgram_fill(packed, m, n, SG.row_nnz, SG.perm, SG.slice_off, ell, stride)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def timed(f):
    f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        ev[0].record()
        f()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return out


t0 = timed(lambda: K.sgram_spmm(W, packed, s, None, ell, SG.perm, SG.slice_off, stride, P))
pi = P.view(torch.int32).to(torch.int64)
print("P checksum", int(pi.sum().item()), flush=True)
del pi
zero = torch.zeros_like(SG.slice_off)
t1 = timed(lambda: K.sgram_spmm(W, packed, s, None, ell, SG.perm, zero, stride, P))
print(f"B={B} density {SG.density:.4%}")
print("spmm real ELL ms:", " ".join(f"{t:.3f}" for t in t0), f" min {min(t0):.3f} spread {max(t0) - min(t0):.3f}")
print("spmm width-0 (staging + output only) ms:", " ".join(f"{t:.3f}" for t in t1), f" min {min(t1):.3f}")
