"""What the recurrence epilogue of a Chebyshev filter launch costs: the
filter product at the bench shape (k = 4096, p = 192), single and split, timed with HIP
events in the argument sets solver._filter_x3 uses:
    (a) a middle step   C = a A G + b P + c D, the next iterate's fp16 halves out (P aliases C)
    (b) the plain product C = A G (no P, D, halves)
    (c) the last step   (a) without halves, with the transposed output Ct
(a) - (b) is the epilogue.  --lean: the outputs nothing reads are not asked for (a single
middle step without lo halves, the last step without C).
--lib: another build of the library (an A/B on one machine).
    python tools/bench_epilogue.py 128 256 [--lean] [--n 20] [--lib PATH]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import ee274_convexcaldera_llm_quantization_amd._lib as K

dev = "cuda:0"
argv = sys.argv[1:]
lean = "--lean" in argv


def _opt(name, default):
    if name not in argv:
        return default
    i = argv.index(name)
    v = argv[i + 1]
    del argv[i:i + 2]
    return v


n_it = int(_opt("--n", 20))
lib = _opt("--lib", None)
K.load() if lib is None else K.load(lib)
batches = [int(x) for x in argv if x.isdigit()] or [128, 256]
k, p, xs = 4096, 192, 2.0 ** 6


def bench(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


Bmax = max(batches)
g = torch.Generator(device=dev).manual_seed(0)
Gh = torch.empty(Bmax, k, k, device=dev, dtype=torch.float16)
Gl = torch.empty_like(Gh)
for b in range(Bmax):  # symmetric G, one matrix at a time (bounded memory)
    Y = torch.randn(k, k // 4, device=dev, generator=g) * 0.05
    h, l, _, _ = K.sym_split_f16((Y @ Y.T).unsqueeze(0), xs, blocked=True)
    Gh[b].copy_(h[0]); Gl[b].copy_(l[0])
del Y, h, l
print(f"# k={k} p={p} launches timed per figure: {n_it}  lean={lean}  "
      f"lib={lib or 'default'}", flush=True)
print("# kind    B    (a) middle  (b) plain  (c) last   (a)-(b)  share of (a)   [ms per launch]", flush=True)
for B in batches:
    X = torch.randn(B, k, p, device=dev, generator=g) / k ** 0.5
    xt = [torch.empty(B, p, k, device=dev) for _ in range(2)]
    xh = [torch.empty(B, p, k, device=dev, dtype=torch.float16) for _ in range(2)]
    xl = [torch.empty_like(xh[0]) for _ in range(2)]
    K.transpose_split(X, out=xt[0], hi=xh[0], lo=xl[0], scale=xs, blocked=True)
    xt[1].copy_(xt[0])
    out = torch.empty(B, k, p, device=dev)
    ovf = torch.zeros(B, dtype=torch.int32, device=dev)
    act = torch.ones(B, dtype=torch.int32, device=dev)
    inv = torch.full((B,), 1.0 / xs / xs, device=dev)
    # coefficients that keep the iterate bounded when P aliases C over many launches
    al = torch.full((B,), 1e-3, device=dev); be = torch.full((B,), -0.25, device=dev); ga = torch.full((B,), 0.1, device=dev)
    gh, gl = Gh[:B], Gl[:B]
    for single in (True, False):
        common = dict(alpha_v=al, beta_v=be, gamma_v=ga, out_scale=xs, overflow=ovf, b_blocked=True, active=act,
                      a_blocked=True, o_blocked=True, single=single)
        ol = None if (lean and single) else xl[1]
        mid = lambda: K.gemm_x3(xh[0], xl[0], gh, gl, inv, xt[1], P=xt[1], D=xt[0], out_h=xh[1], out_l=ol, **common)
        plain = lambda: K.gemm_x3(xh[0], xl[0], gh, gl, inv, xt[1], b_blocked=True, a_blocked=True, single=single)
        last = lambda: K.gemm_x3(xh[0], xl[0], gh, gl, inv, None if lean else xt[1], P=xt[1], D=xt[0], Ct=out, **common)
        ta, tb, tc = bench(mid, n_it), bench(plain, n_it), bench(last, n_it)
        print(f"{'single' if single else 'split '} {B:4d}   {ta:8.3f}   {tb:8.3f}   {tc:8.3f}   {ta - tb:7.3f}   "
              f"{100 * (ta - tb) / ta:5.1f} %", flush=True)
    del X, xt, xh, xl, out
print(f"# overflow flags raised: {int(ovf.sum())}", flush=True)
