"""Host-seeded inputs and plain numpy references of every library entry that reads a column, row
or error weight at a batch stride (ABI 5, include/caldera_hip.h): tests/test_gpu_weight_strides.py
runs the kernels on them, tests/test_weight_stride_refs_host.py checks the references themselves.

A case is one entry on one set of inputs.  Its reference is evaluated per matrix from the
header's formula with ONE weight row, ref(b, w_row): fp64 where the entry accumulates (error
sums, products), numpy fp32 (each operation correctly rounded, as the kernels' are) where the
outputs are bit-exact by contract (codes, scales, dequantised values, residuals, split halves).
tol[name] is the bar of the existing shared-vector test of the same entry: None = bit-exact,
a float = relative, "bound" = an elementwise bound the reference returns as name + "_bound".
`weighted` names the outputs that depend on the weights.

Weights (common to every case): B = 3 rows, row b = F[b] * 10^u, u uniform in [-2, 1] per
column from a seed of its own -- positive, different in scale and in pattern per matrix.  Host
RNG only, so the inputs are the same bytes on every machine."""
import numpy as np

from oracle import caldera_oracle as O

B = 3
F = (1.0, 7.0, 0.13)
f32, f64 = np.float32, np.float64
U24 = 2.0 ** -24


def weights(n, seed):
    """(B, n) fp32: row b = F[b] * 10^u_b, u_b ~ U[-2, 1] from seed + 1000 b."""
    return np.stack([F[b] * 10.0 ** np.random.default_rng(seed + 1000 * b).uniform(-2.0, 1.0, n)
                     for b in range(B)]).astype(f32)


def pack_codes(c, bits):
    """Offset-binary (c + k), MSB-first packed codes of the header: 4 (2-bit) or 2 (4-bit) per byte."""
    k = 2 ** (bits - 1) - 1
    per = 8 // bits
    u = (np.asarray(c).astype(np.int32) + k).astype(np.uint8).reshape(-1, per)
    out = np.zeros(u.shape[0], dtype=np.uint8)
    for i in range(per):
        out |= u[:, i] << (bits * (per - 1 - i))
    return out


def planted(m, n, seed, n_out=40):
    """test_gpu_codebook._planted: small normal values with a few planted outliers."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((m, n)) * 0.02).astype(f32)
    idx = rng.integers(0, m * n, n_out)
    x.reshape(-1)[idx] = (rng.choice([-1.0, 1.0], n_out) * rng.uniform(0.2, 0.5, n_out)).astype(f32)
    return x


def sparse_codes(rng, shape, density):
    """2-bit codes in {-1, 0, 1} with about `density` nonzeros."""
    return np.where(rng.random(shape) < density, rng.choice([-1, 1], size=shape), 0).astype(np.int8)


def kblock(x):
    """(rows, cols) -> the K-blocked layout over the columns: (r, c) at (c / 32) rows 32 + r 32 + c % 32."""
    r, c = x.shape
    return np.ascontiguousarray(x.reshape(r, c // 32, 32).transpose(1, 0, 2)).reshape(-1)


def split16(x, s):
    """hi = f16(x s), lo = f16(x s - hi) of an fp32 array at the fp32 scale s."""
    xs = (x.astype(f32) * f32(s)).astype(f32)
    h = xs.astype(np.float16)
    return h, (xs - h.astype(f32)).astype(np.float16)


def pow2_for(bound):
    """The split scale 2^(14 - e) for bound in [2^(e-1), 2^e) (cq_residual_split)."""
    bound = f32(bound)
    e = int(np.frexp(bound)[1]) if bound > 0 and np.isfinite(bound) else 0
    return f32(np.ldexp(1.0, 14 - e))


class Case:
    def __init__(self, id, entry, inp, ref, tol, weighted, **kw):
        self.id, self.entry, self.inp, self.ref, self.tol, self.weighted, self.kw = id, entry, inp, ref, tol, weighted, kw

    @property
    def w(self):
        return self.inp["w"]

    def ref_batch(self, w):
        """Per-matrix references for weights (B, n) (row b for matrix b) or (n,) (shared)."""
        w = np.asarray(w)
        return [self.ref(b, w if w.ndim == 1 else w[b]) for b in range(B)]


def werr(d, x, w, n):
    """sum_ij w[j % n] (d_ij - x_ij)^2 with the fp32 difference squared in fp32, summed in fp64
    (the kernels' error sums: test_gpu_codebook.py's 1e-6 bar)."""
    df = (d.astype(f32) - x.astype(f32)).astype(f32).reshape(-1, n)
    return f64(((df * df).astype(f64) * w.astype(f64)[None, :]).sum())


# ------------------------------------------------------------------------------ the cases
def _wsq(dt, m, n):
    rng = np.random.default_rng(m * 1000 + n)
    x = (rng.standard_normal((B, m * n)) * 0.5).astype(dt)
    inp = dict(x=x, w=weights(n, 11 + n), n=n)

    def ref(b, w):
        return {"out": f64((x[b].astype(f64).reshape(m, n) ** 2 * w.astype(f64)).sum())}
    return Case(f"wsq-{np.dtype(dt).name}-{m}x{n}", "weighted_sqsum", inp, ref, {"out": 1e-6}, {"out"})


def _uniform(bits, block):
    m, n = 32, 64
    bs = m * n if block == "all" else block
    rng = np.random.default_rng(bits * 10 + (block != "all"))
    x = rng.standard_normal((B, m * n)).astype(f32)
    inp = dict(x=x, w=weights(n, 21 + bits), n=n, bits=bits, bs=bs)
    fixed = []
    for b in range(B):
        c, s = O.quantize_uniform(x[b], bits, bs)
        fixed.append((c.reshape(-1), s.reshape(-1), O.dequantize_uniform(c, s, bits, (m * n,))))

    def ref(b, w):
        c, s, d = fixed[b]
        out = {"codes": c, "scale": s, "deq": d, "err": werr(d, x[b], w, n)}
        if bits <= 4:
            out["packed"] = pack_codes(c, bits)
        return out
    tol = {"codes": None, "scale": None, "deq": None, "packed": None, "err": 1e-6}
    return Case(f"uniform-b{bits}-bs{block}", "quantize_uniform", inp, ref, tol, {"err"})


def _codebook(method, bits, block):
    m, n = 64, 256
    bs = m * n if block == "all" else block
    x = np.stack([planted(m, n, seed=300 + 10 * bits + b, n_out=10 * (b + 1)) for b in range(B)]).reshape(B, -1)
    inp = dict(x=x, w=weights(n, 31 + bits), n=n, bits=bits, bs=bs, method=method)
    fixed = []
    for b in range(B):
        q = O.LowMemoryQuantizer(bits, method, bs)
        c, p, _ = q.quantize_block(x[b].reshape(m, n))
        fixed.append((c, p, q.dequantize_block(c, p, (m * n,))))

    def ref(b, w):
        c, p, d = fixed[b]
        out = {"deq": d, "err": werr(d, x[b], w, n)}
        if method.startswith("nf"):
            out.update(idx=c.reshape(-1), scale=np.asarray(p).reshape(-1))
        else:
            out.update(packed=c.reshape(-1), bmin=p[0].reshape(-1), bscale=p[1].reshape(-1), vals=p[2], oidx=p[3])
        return out
    tol = {k: None for k in ("deq", "idx", "scale", "packed", "bmin", "bscale", "vals", "oidx")}
    tol["err"] = 1e-6
    return Case(f"{method}-bs{block}", "quantize_" + ("nf" if method.startswith("nf") else "bbint"), inp, ref, tol,
                {"err"})


def _quantised_q(W32, bits):
    """Whole-matrix uniform codes of 0.9 W per matrix: (codes, scale (B,), deq)."""
    cs, ss, ds = [], [], []
    for b in range(B):
        c, s = O.quantize_uniform((W32[b] * f32(0.9)).astype(f32), bits, W32[b].size)
        cs.append(c.reshape(-1))
        ss.append(s.reshape(-1)[0])
        ds.append(O.dequantize_uniform(c, s, bits, W32[b].shape))
    return np.stack(cs), np.asarray(ss, dtype=f32), np.stack(ds)


def _build_residual(dt, bits):
    m, n = 32, 64
    rng = np.random.default_rng(41 + (bits or 0) + (dt == f32))
    W = (rng.standard_normal((B, m, n)) * 0.7).astype(dt)
    W32 = W.astype(f32)
    inp = dict(W=W, w=weights(n, 41), m=m, n=n, bits=bits)
    if bits is None:
        deq = np.zeros_like(W32)
    else:
        c, s, deq = _quantised_q(W32, 2 if bits == 32 else bits)
        inp.update(qscale=s, packed=deq if bits == 32 else np.stack([pack_codes(c[b], bits) for b in range(B)]))

    def ref(b, w):
        res = (W32[b] - deq[b]).astype(f32)
        return {"res": res, "Y": (res * w[None, :]).astype(f32)}
    return Case(f"build_residual-{np.dtype(dt).name}-b{bits}", "build_residual", inp, ref, {"res": None, "Y": None},
                {"Y"})


def _gemm_werr(M, N, Kd):
    rng = np.random.default_rng(M + N + Kd)
    A = rng.standard_normal((B, M, Kd)).astype(f32)
    Bm = rng.standard_normal((B, Kd, N)).astype(f32)
    D = rng.standard_normal((B, M, N)).astype(f32)
    inp = dict(A=A, Bm=Bm, D=D, w=weights(N, 51 + N))

    def ref(b, w):
        E = D[b].astype(f64) - A[b].astype(f64) @ Bm[b].astype(f64)
        return {"err": f64((E * E * w.astype(f64)).sum())}
    return Case(f"gemm_werr-{M}x{N}x{Kd}", "gemm", inp, ref, {"err": 1e-5}, {"err"})


X3_SA, X3_SB = 2.0 ** 10, 2.0 ** 14


def _gemm_x3(tag, M, N, Kd, **kw):
    """C = (A B^T) diag(colw) + gamma D; B exactly fp16 at its split scale, so b_exact applies."""
    rng = np.random.default_rng(M + N + Kd)
    lda = kw.get("lda", M)   # K-blocked A: rows held, a multiple of 8, of which the first M are used
    A = rng.standard_normal((B, lda, Kd)).astype(f32)
    Bm = (rng.standard_normal((B, N, Kd)) * 0.05).astype(np.float16).astype(f32)
    D = rng.standard_normal((B, M, N)).astype(f32)
    gam = rng.standard_normal(B).astype(f32)
    inp = dict(A=A, Bm=Bm, D=D, gam=gam, w=weights(N, 61 + N), M=M, N=N)
    prod = [A[b, :M].astype(f64) @ Bm[b].astype(f64).T for b in range(B)]

    def ref(b, w):
        return {"C": prod[b] * w.astype(f64)[None, :] + f64(gam[b]) * D[b].astype(f64)}
    # (test_gemm_x3_matches_fp64's column bound is below 1e-6 relative on these shapes)
    return Case(f"gemm_x3-{tag}", "gemm_x3", inp, ref, {"C": 1e-6}, {"C"}, **kw)


def _residual_split(m, n, bits, with_hi, dt=np.float16):
    rng = np.random.default_rng(m + n + (bits or 0) + with_hi)
    W = (rng.standard_normal((B, m, n)) * 0.5).astype(dt)
    W32 = W.astype(f32)
    w = weights(n, 71 + n)
    wh = (w * w).astype(f32)
    inp = dict(W=W, w=w, w_hi=wh if with_hi else None, m=m, n=n, bits=bits, wmax=np.abs(W32).max(axis=(1, 2)))
    c, s, deq = _quantised_q(W32, 2)
    inp.update(qscale=s, packed=deq if bits == 32 else np.stack([pack_codes(c[b], 2) for b in range(B)]))

    def ref(b, w_row):
        """cq_residual_split of the header with ycol = w_row, ycol_hi = w_row^2 and the per-matrix
        bounds max(w_row), max(w_row)^2."""
        res = (W32[b] - deq[b]).astype(f32)
        Y = (res * w_row[None, :]).astype(f32)
        ymax = f32(w_row.max())
        sc = pow2_for((inp["wmax"][b] + s[b]).astype(f32) * ymax)
        out = {"res": res, "Y": Y, "scale": sc, "sq": f64((Y.astype(f64) ** 2).sum())}
        th, tl = split16(Y.T, sc)
        out["thi"], out["tlo"] = kblock(th), kblock(tl)
        if with_hi:
            sch = pow2_for((inp["wmax"][b] + s[b]).astype(f32) * f32(ymax * ymax))
            h, lo = split16((res * (w_row * w_row).astype(f32)[None, :]).astype(f32), sch)
            out["scale_hi"] = sch
        else:
            h, lo = split16(Y, sc)
        out["hi"], out["lo"] = kblock(h), kblock(lo)
        return out
    tol = {k: None for k in ("res", "Y", "scale", "scale_hi", "hi", "lo", "thi", "tlo")}
    tol["sq"] = 1e-12
    weighted = {"Y", "scale", "sq", "hi", "lo", "thi", "tlo"} | ({"scale_hi"} if with_hi else set())
    return Case(f"residual_split-{np.dtype(dt).name}-{m}x{n}-b{bits}-hi{int(with_hi)}", "residual_split", inp, ref, tol,
                weighted)


SGRAM_S = np.asarray([2.5, 3.0, 0.75], dtype=f32)


def _sgram(k, L, form, rows=None):
    """Sparse-code Gram pieces: corr[b] = sum_{c != 0} wcol[l] (s^2 - 2 s c W) (fp64) and P = (W - (s/2) c)
    diag(wcol) c^T (fp32 chains: the elementwise bound of test_gpu_codes.py, (terms + 3) u sum |terms|).
    rows: the rows of P the reference evaluates (None: all)."""
    rng = np.random.default_rng(k * 7 + L)
    W = (rng.standard_normal((B, k, L)) * 0.7).astype(np.float16)
    c = sparse_codes(rng, (B, k, L), 0.02)
    inp = dict(W=W, c=c, s=SGRAM_S, w=weights(L, 81 + L), k=k, L=L, form=form,
               packed=np.stack([pack_codes(c[b], 2) for b in range(B)]),
               rows=np.arange(k) if rows is None else np.asarray(rows))

    def ref(b, w):
        s, cb = f64(SGRAM_S[b]), c[b].astype(f64)
        Wb = W[b].astype(f64)
        wd = w.astype(f64)
        corr = f64((wd[None, :] * (s * s - 2.0 * s * cb * Wb) * (cb != 0)).sum())
        E = (Wb[inp["rows"]] - 0.5 * s * cb[inp["rows"]]) * wd[None, :]
        nz = (cb != 0).sum(1).astype(f64)
        return {"corr": corr, "P": E @ cb.T, "P_bound": (np.abs(E) @ np.abs(cb).T) * (nz[None, :] + 3.0) * U24 + 1e-30}
    return Case(f"sgram-{form}-k{k}-L{L}", "sgram", inp, ref, {"corr": 1e-9, "P": "bound"}, {"corr", "P"})


def _codes(rows, cols, r):
    rng = np.random.default_rng(rows * 3 + cols)
    c = sparse_codes(rng, (B, rows, cols), 0.05)
    X = rng.standard_normal((B, cols, r)).astype(f32)
    W = rng.standard_normal((B, rows, cols)).astype(np.float16)
    inp = dict(c=c, X=X, W=W, s=SGRAM_S, w=weights(cols, 91 + cols), roww=weights(rows, 95 + rows), rows=rows, cols=cols,
               r=r, packed=np.stack([pack_codes(c[b], 2) for b in range(B)]))

    def ref(b, w, roww=None):
        """colw = w; roww = this matrix's row weights unless given.  The three weightings of
        cq_codes_matmul and cq_codes_ysq_corr's norm correction."""
        rw = (inp["roww"][b] if roww is None else roww).astype(f64)
        cb, Xb, wd = c[b].astype(f64), X[b].astype(f64), w.astype(f64)
        nz = (cb != 0).sum(1, keepdims=True).astype(f64) + 2.0
        plain, plain_abs = cb @ Xb, np.abs(cb) @ np.abs(Xb)
        col, col_abs = (cb * wd[None, :]) @ Xb, (np.abs(cb) * wd[None, :]) @ np.abs(Xb)
        s = f64(SGRAM_S[b])
        out = {"colw": col, "colw_bound": col_abs * nz * U24 + 1e-30,
               "roww": rw[:, None] * plain, "roww_bound": rw[:, None] * plain_abs * nz * U24 + 1e-30,
               "both": rw[:, None] * col, "both_bound": rw[:, None] * col_abs * nz * U24 + 1e-30,
               "corr": f64((wd[None, :] * (s * s - 2.0 * s * cb * W[b].astype(f64)) * (cb != 0)).sum())}
        return out
    tol = {"colw": "bound", "roww": "bound", "both": "bound", "corr": 1e-9}
    return Case(f"codes-{rows}x{cols}-r{r}", "codes", inp, ref, tol, {"colw", "both", "corr"})


def _q_update(tag, m, n, r, bits, dt, **kw):
    """cq_q_update_x3: codes / scale of res = W - L R quantised whole, err = sum err_w[j] (deq - res)^2.
    r = 0: res = W exactly (oracle codes, bit-exact).  r > 0: res in fp64; codes and scale at the
    bars of test_q_update_x3_with_lr_matches_fp64_residual (codes equal except within 1e-4 code
    units of a tie, scale to 1e-6).  err at 1e-6 in both (test_gpu_codebook.py's bar: with |L R|
    ~ 1e-2 |W| the fp32-grade residual moves an error term by ~1e-8 relative)."""
    rng = np.random.default_rng(m + 3 * n + 7 * r + bits)
    W = (rng.standard_normal((B, m, n)) * 0.02).astype(dt)
    for b in range(B):
        W[b, 5 + b, 9 + 2 * b] = 0.5 + 0.1 * b      # a planted maximum per matrix
    inp = dict(W=W, w=weights(n, 101 + n), m=m, n=n, r=r, bits=bits)
    if r:
        inp["L"] = np.linalg.qr(rng.standard_normal((B, m, r)))[0].astype(f32) if m >= r else (
            rng.standard_normal((B, m, r)) / np.sqrt(r)).astype(f32)
        inp["R"] = (rng.standard_normal((B, r, n)) * 0.01).astype(f32)
    k = f64(2 ** (bits - 1) - 1)

    def ref(b, w):
        if r == 0:
            c, s = O.quantize_uniform(W[b].astype(f32), bits, m * n)
            d = O.dequantize_uniform(c, s, bits, (m, n))
            out = {"codes": c.reshape(-1), "scale": f32(s.reshape(-1)[0]), "err": werr(d, W[b], w, n)}
        else:
            res = W[b].astype(f64) - inp["L"][b].astype(f64) @ inp["R"][b].astype(f64)
            s = np.abs(res).max()
            t = res / s * k
            c = np.rint(t)
            out = {"codes": c.reshape(-1).astype(np.int16), "scale": f64(s),
                   "tie": (np.abs(np.abs(t - np.floor(t)) - 0.5) < 1e-4).reshape(-1),
                   "err": f64((((c / k * s - res) ** 2) * w.astype(f64)[None, :]).sum())}
        if bits <= 4:
            out["packed"] = pack_codes(out["codes"], bits)
        return out
    tol = {"codes": None, "packed": None, "scale": None if r == 0 else 1e-6, "tie": None, "err": 1e-6}
    return Case(f"q_update-{tag}", "q_update_x3", inp, ref, tol, {"err"}, **kw)


def _specs():
    """(entry, constructor, arguments) of every case; nothing is built here."""
    sp = []
    sp += [("weighted_sqsum", _wsq, (dt, 24, n), {}) for dt in (np.float16, f32) for n in (64, 52)]
    sp += [("quantize_uniform", _uniform, (bits, block), {}) for bits in (2, 8) for block in (64, "all")]
    sp += [("quantize_nf" if m.startswith("nf") else "quantize_bbint", _codebook, (m, b, block), {})
           for m, b in (("nf4", 4), ("nf2", 2), ("bbint4", 4), ("bbint2", 2)) for block in (64, "all")]
    sp += [("build_residual", _build_residual, (dt, bits), {}) for dt in (np.float16, f32) for bits in (2, 4, 32, None)]
    sp += [("gemm", _gemm_werr, (37, 53, 29), {}), ("gemm", _gemm_werr, (128, 128, 16), {})]
    sp += [("gemm_x3", _gemm_x3, a, kw) for a, kw in (
        (("onepass-192x768x256", 192, 768, 256), {}), (("ragged-100x1000x32", 100, 1000, 32), dict(lda=104)),
        (("ksplit5-192x768x256", 192, 768, 256), dict(ksplit=5)),
        (("ct-100x1000x32", 100, 1000, 32), dict(lda=104, ct=True)),
        (("ksplit5-ct-192x768x256", 192, 768, 256), dict(ksplit=5, ct=True)),
        (("exactb-128x1024x2048", 128, 1024, 2048), dict(lda=192, b_exact=True)),
        (("exactb-ksplit5-128x1024x2048", 128, 1024, 2048), dict(lda=192, b_exact=True, ksplit=5)),
        (("scalar-100x1002x32", 100, 1002, 32), dict(blocked=False)))]
    sp += [("residual_split", _residual_split, (m, n, bits, hi), {})
           for m, n in ((32, 64), (64, 128)) for bits in (2, 32) for hi in (False, True)]
    sp += [("residual_split", _residual_split, (32, 64, 2, True), dict(dt=f32))]
    sp += [("sgram", _sgram, a, {}) for a in ((64, 64, "r8held"), (256, 64, "r8"), (64, 4864, "r4"), (256, 4864, "r4"),
                                             (64, 9664, "lsplit"), (256, 9664, "lsplit"), (64, 19136, "r2"),
                                             (256, 18752, "r2"))]
    sp += [("sgram", _sgram, (2752, 2752, "r8held-nb2"), dict(rows=np.arange(0, 2752, 43)))]
    sp += [("codes", _codes, (64, 128, 32), {}), ("codes", _codes, (128, 64, 200), {})]
    sp += [("q_update_x3", _q_update, a, kw) for a, kw in (
        (("stream-n1024", 64, 1024, 0, 2, np.float16), dict(known=True)),
        (("stream-n1040", 64, 1040, 0, 2, np.float16), dict(known=True)),
        (("stream-f32-b4-n1024", 64, 1024, 0, 4, f32), dict(known=True)),
        (("panel-256x64-r32", 256, 64, 32, 2, np.float16), {}), (("tile-64x64-r288", 64, 64, 288, 2, np.float16), {}),
        (("nonvec-64x52-r32", 64, 52, 32, 2, np.float16), {}))]
    return sp


def _id(fn, a, kw):
    """The case's name from its constructor's arguments (the constructors use the same formats)."""
    dn = lambda dt: np.dtype(dt).name   # noqa: E731
    if fn is _wsq:
        return f"wsq-{dn(a[0])}-{a[1]}x{a[2]}"
    if fn is _uniform:
        return f"uniform-b{a[0]}-bs{a[1]}"
    if fn is _codebook:
        return f"{a[0]}-bs{a[2]}"
    if fn is _build_residual:
        return f"build_residual-{dn(a[0])}-b{a[1]}"
    if fn is _gemm_werr:
        return "gemm_werr-%dx%dx%d" % a
    if fn is _gemm_x3:
        return f"gemm_x3-{a[0]}"
    if fn is _residual_split:
        return f"residual_split-{dn(kw.get('dt', np.float16))}-{a[0]}x{a[1]}-b{a[2]}-hi{int(a[3])}"
    if fn is _sgram:
        return f"sgram-{a[2]}-k{a[0]}-L{a[1]}"
    if fn is _codes:
        return "codes-%dx%d-r%d" % a
    return f"q_update-{a[0]}"


SPECS = {_id(fn, a, kw): (entry, fn, a, kw) for entry, fn, a, kw in _specs()}
_CACHE = {}


def case(cid):
    """The case of that name, built on first use (inputs and references are shared by the tests
    and never written)."""
    if cid not in _CACHE:
        _, fn, a, kw = SPECS[cid]
        _CACHE[cid] = fn(*a, **kw)
        assert _CACHE[cid].id == cid
    return _CACHE[cid]


def ids(entry=None):
    return [cid for cid, sp in SPECS.items() if entry is None or sp[0] == entry]


def differs(a, b, tol, bound=None):
    """How far reference b (another matrix's weight row) is from reference a, in units of the bar:
    for a bit-exact output the fraction of elements that differ (bar: 1 %), for a relative bar
    |a - b| / (tol |a|) as a norm ratio, for an elementwise bound the largest |a - b| / bound."""
    a, b = np.asarray(a), np.asarray(b)
    if tol is None:
        return float((a != b).mean()) / 0.01
    if tol == "bound":
        return float((np.abs(a - b) / bound).max())
    return float(np.linalg.norm((a - b).ravel()) / (tol * np.linalg.norm(a.ravel())))
