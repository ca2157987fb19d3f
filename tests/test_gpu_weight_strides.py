"""Per-matrix weight strides (ABI 5, include/caldera_hip.h) kernel by kernel: every entry that
reads a column, row or error weight at a batch stride, on the inputs and plain references of
tests/weight_stride_cases.py (B = 3 matrices, weights (B, n) whose rows differ in scale and
pattern).  Two assertions per entry and dispatch branch:

1. against the reference: matrix b's outputs equal the reference evaluated with weight row b,
   at the bar of the existing shared-vector test of the same entry (codes, scales, dequantised
   values, residuals and split halves bit-exact; error sums 1e-6 relative; products at the
   bounds of test_gpu_codes.py / test_gemm_resid_and_werr / test_gemm_x3_colw_epilogue);
2. against the shared-vector run: matrix b's outputs equal, bit for bit, those of the same call
   on a batch of B copies of matrix b with the 1-D vector w[b] (the same batch size, so the
   same launch geometry and summation order -- caldera_batch's promise).

The weights live inside a larger NaN-filled buffer (at least 64 NaN floats before row 0 and
after row B - 1), so a read outside the B rows poisons the result; a read of a neighbouring row
fails assertion 1 (tests/test_weight_stride_refs_host.py shows that a wrong row is at least 100
bars away).  pad = 64 floats keeps the rows 16-byte aligned (the vector kernels), pad = 65
breaks the alignment where an entry's dispatch looks at it (cq_weighted_sqsum, cq_q_update_x3:
the scalar and non-vector kernels then run on the same data).

Which branch a shape enters was read from each launcher's dispatch condition (csrc/); the
sparse-Gram forms are queried (sgram_rows, sgram_split) and asserted."""
import numpy as np
import pytest
import torch

import weight_stride_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = C.B
NOT_BATCHED = {"w", "w_hi", "roww", "rows"}


@pytest.fixture(scope="module")
def K():
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    K.load()
    return K


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def wbuf(w, pad=64):
    """The weights (B, n) or (n,) as a contiguous view into a NaN-filled flat buffer, `pad` floats in."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    flat = torch.full((pad + w.size + 64 + 3,), float("nan"), device=DEV)
    flat[pad:pad + w.size] = dev(w.reshape(-1))
    v = flat[pad:pad + w.size].view(w.shape)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (pad % 4 == 0)
    assert torch.isnan(flat[:pad]).all() and torch.isnan(flat[pad + w.size:]).all() and pad >= 64
    return v


def copies(inp, b):
    """The inputs of a batch of B copies of matrix b ("_b": which one)."""
    out = {k: (np.repeat(v[b:b + 1], B, axis=0) if isinstance(v, np.ndarray) and k not in NOT_BATCHED and v.shape[0] == B
               else v) for k, v in inp.items()}
    out["_b"] = b
    return out


def check_ref(case, b, got, ref, names=None):
    """Assertion 1 for matrix b: got[name][b] against ref[name] at case.tol[name]."""
    for name in (names or [n for n in ref if not n.endswith("_bound") and n in got]):
        tol, g, r = case.tol[name], got[name][b].cpu().numpy(), np.asarray(ref[name])
        g = g.reshape(r.shape)
        if tol is None:
            assert np.array_equal(g, r), (case.id, b, name, int((g != r).sum()))
        elif tol == "bound":
            assert (np.abs(g.astype(np.float64) - r) <= ref[name + "_bound"]).all(), (case.id, b, name)
        else:
            err = float(np.linalg.norm((g.astype(np.float64) - r).ravel()) / np.linalg.norm(r.ravel()))
            print(f"{case.id} matrix {b} {name}: relative deviation {err:.2e} (bar {tol:.0e})")
            assert err <= tol, (case.id, b, name, err)


def check_same(case, b, got, rep):
    """Assertion 2 for matrix b: bit-equal to position b of the run on copies with the shared vector."""
    assert set(got) == set(rep)
    for name in got:
        assert torch.equal(got[name][b], rep[name][b]), (case.id, b, name)


def both(case, run, pad=64, names=None):
    got = run(case.inp, wbuf(case.w, pad))
    for b in range(B):
        check_ref(case, b, got, case.ref(b, case.w[b]), names)
        check_same(case, b, got, run(copies(case.inp, b), wbuf(case.w[b], pad)))
    return got


ids = C.ids


# ------------------------------------------------------------------------------ weighted_sqsum
@pytest.mark.parametrize("pad", [64, 65])
@pytest.mark.parametrize("cid", ids("weighted_sqsum"))
def test_weighted_sqsum(K, cid, pad):
    """cq_weighted_sqsum (cq_quant.hip): the 8-wide kernel needs numel % 8 == 0, ncols % 8 == 0,
    w_stride % 4 == 0 and 16-byte aligned x and w -- 24 x 64 at pad 64; 24 x 52 (ncols % 8 != 0)
    and every shape at pad 65 take wsq_partial_kernel, the scalar fallback.  fp16 and fp32 x."""
    c = C.case(cid)
    both(c, lambda inp, w: {"out": K.weighted_sqsum(dev(inp["x"]), w, inp["n"])}, pad)


# ------------------------------------------------------------------------------ uniform quantiser
@pytest.mark.parametrize("cid", ids("quantize_uniform"))
def test_quantize_uniform(K, cid):
    """cq_quantize_uniform with err_out: quant_known_dispatch after the absmax kernel, for blocks
    of 64 and the whole matrix; 2-bit (packed) and 8-bit codes."""
    c = C.case(cid)

    def run(inp, w):
        o = K.quantize_uniform(dev(inp["x"]), inp["bs"], inp["bits"], codes=True, packed=inp["bits"] <= 4, deq=True,
                               err_w=w, err_ncols=inp["n"])
        return {k: v for k, v in o.items() if v is not None}
    both(c, run)


@pytest.mark.parametrize("bits", [2, 8])
def test_quantize_known_max(K, bits):
    """cq_quantize_uniform_known_max (whole matrix, max|x| given as bits)."""
    c = C.case(f"uniform-b{bits}-bsall")

    def run(inp, w):
        x = dev(inp["x"])
        numel = x.shape[1]
        mx = dev(np.abs(inp["x"]).max(axis=1).astype(np.float32)).view(torch.int32)
        o = {"codes": torch.empty(B, numel, dtype=K.code_dtype(bits), device=DEV),
             "deq": torch.empty(B, numel, device=DEV), "scale": torch.empty(B, 1, device=DEV),
             "err": torch.empty(B, dtype=torch.float64, device=DEV)}
        if bits <= 4:
            o["packed"] = torch.empty(B, numel * bits // 8, dtype=torch.uint8, device=DEV)
        K.quantize_known_max(x, mx, bits, codes=o["codes"], packed=o.get("packed"), deq=o["deq"], scale=o["scale"],
                             err_w=w, err_ncols=inp["n"], err_out=o["err"])
        return o
    both(c, run)


# ------------------------------------------------------------------------------ codebook quantisers
@pytest.mark.parametrize("cid", ids("quantize_nf"))
def test_quantize_nf(K, cid):
    """cq_quantize_nf: blocks of 64 (<= 4096) take nf_block_kernel, the whole 64 x 256 matrix
    (16384 > 4096) cb_absmax_kernel + nf_known_kernel; NF4 and NF2."""
    c = C.case(cid)

    def run(inp, w):
        err = torch.empty(B, dtype=torch.float64, device=DEV)
        o = K.quantize_nf(dev(inp["x"]), inp["bs"], inp["bits"], err_w=w, err_ncols=inp["n"], err_out=err)
        return {**o, "err": err}
    both(c, run)


@pytest.mark.parametrize("cid", ids("quantize_bbint"))
def test_quantize_bbint(K, cid):
    """cq_bbint_stats + cq_bbint_emit (the emit kernel reads the error weights); bbint4 and bbint2,
    blocks of 64 and the whole matrix, planted 6-sigma outliers."""
    c = C.case(cid)

    def run(inp, w):
        err = torch.empty(B, dtype=torch.float64, device=DEV)
        o = K.quantize_bbint(dev(inp["x"]), inp["bs"], inp["bits"], err_w=w, err_ncols=inp["n"], err_out=err)
        off = np.concatenate([[0], np.cumsum(o["n_out"])])
        return {"packed": o["packed"], "deq": o["deq"], "bmin": o["bmin"], "bscale": o["bscale"], "err": err,
                "vals": [o["vals"][off[b]:off[b + 1]] for b in range(B)],
                "oidx": [o["idx"][off[b]:off[b + 1]] for b in range(B)]}
    both(c, run)


# ------------------------------------------------------------------------------ build_residual
@pytest.mark.parametrize("cid", ids("build_residual"))
def test_build_residual(K, cid):
    """cq_build_residual: fp16 and fp32 W; 2- and 4-bit packed codes, a dense fp32 Q (bits 32), no codes."""
    c = C.case(cid)

    def run(inp, w):
        Ws = dev(inp["W"])
        o = {"Y": torch.full(Ws.shape, float("nan"), device=DEV), "res": torch.full(Ws.shape, float("nan"), device=DEV)}
        bits = inp["bits"]
        K.build_residual(Ws, None if bits is None else dev(inp["packed"]).view(B, -1),
                         None if bits is None else dev(inp["qscale"]), 2 if bits is None else bits, w, Y=o["Y"], res=o["res"])
        return o
    both(c, run)


# ------------------------------------------------------------------------------ fp32 GEMM, EPI_WERR
@pytest.mark.parametrize("cid", ids("gemm"))
def test_gemm_werr(K, cid):
    """cq_gemm_f32 EPI_WERR: a ragged tile (37, 53, 29) and a full one (128, 128, 16)."""
    c = C.case(cid)

    def run(inp, w):
        err = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
        K.gemm(dev(inp["A"]), dev(inp["Bm"]), D=dev(inp["D"]), epi=K.EPI_WERR, w=w, err_out=err)
        return {"err": err}
    both(c, run)


# ------------------------------------------------------------------------------ split-fp16 GEMM, colw
@pytest.mark.parametrize("cid", ids("gemm_x3"))
def test_gemm_x3_colw(K, cid):
    """cq_gemm_x3 colw, read in three places (cq_x3.hip): the 192 x 384 kernel's vector epilogue
    (one pass: 192 x 768 x 256 two full tiles, 100 x 1000 x 32 ragged), its scalar epilogue
    (N = 1002, N % 4 != 0), and the split-K epilogue kernel (ksplit = 5); with C^T and with
    b_exact (test_gemm_x3_colw_epilogue's shape).  colw keeps a product off the square-tile
    kernel (its dispatch requires !colw).  Besides the two assertions: C equals the plain
    product's columns scaled afterwards plus gamma D bit for bit (that test's bar), C^T = C
    transposed, and the column errors against fp64 are within test_gemm_x3_matches_fp64's bound."""
    c = C.case(cid)
    kw = c.kw
    blocked = kw.get("blocked", True)
    M, N = c.inp["M"], c.inp["N"]

    def run(inp, w, plain=False):
        A, Bm = dev(inp["A"]), dev(inp["Bm"])
        Ah, Al = K.split_f16(A, C.X3_SA, blocked=blocked)
        Bh, Bl = K.split_f16(Bm, C.X3_SB, blocked=blocked)
        assert not Bl.any()
        inv = torch.full((B,), 1.0 / (C.X3_SA * C.X3_SB), device=DEV)
        o = {"C": torch.full((B, M, N), float("nan"), device=DEV)}
        if kw.get("ct"):
            o["Ct"] = torch.full((B, N, M), float("nan"), device=DEV)
        extra = {} if plain else dict(D=dev(inp["D"]), gamma_v=dev(inp["gam"]), colw=w)
        if blocked:
            extra.update(lda=A.shape[1], M=M)
        K.gemm_x3(Ah, Al, Bh, None if kw.get("b_exact") else Bl, inv, o["C"], a_blocked=blocked, b_blocked=blocked,
                  b_exact=bool(kw.get("b_exact")), ksplit=kw.get("ksplit", 1), Ct=o.get("Ct"), **extra)
        return o
    w = wbuf(c.w)
    got = both(c, run, names=["C"])
    C0 = run(c.inp, None, plain=True)["C"]
    assert torch.equal(got["C"], C0 * w.view(B, 1, N) + dev(c.inp["gam"]).view(B, 1, 1) * dev(c.inp["D"]))
    if "Ct" in got:
        assert torch.equal(got["Ct"], got["C"].transpose(1, 2))
    for b in range(B):     # column errors within 3x those of the fp32 product (at least 1e-6)
        ref = torch.from_numpy(c.ref(b, c.w[b])["C"])
        A, Bm = torch.from_numpy(c.inp["A"][b, :M]), torch.from_numpy(c.inp["Bm"][b])
        c32 = (A @ Bm.T) * torch.from_numpy(c.w[b]) + float(c.inp["gam"][b]) * torch.from_numpy(c.inp["D"][b])
        err = ((got["C"][b].cpu().double() - ref).norm(dim=0) / ref.norm(dim=0)).max().item()
        err32 = ((c32.double() - ref).norm(dim=0) / ref.norm(dim=0)).max().item()
        assert err < max(3 * err32, 1e-6), (cid, b, err, err32)


# ------------------------------------------------------------------------------ residual_split
@pytest.mark.parametrize("cid", ids("residual_split"))
def test_residual_split(K, cid):
    """cq_residual_split with per-matrix ycol (+ ycol_hi) and per-matrix bounds ycol_max_v /
    ycol_hi_max_v: 2-bit codes and a dense Q (bits 32), one row step (32 x 64) and two (64 x 128),
    every output (res, Y, hi/lo, thi/tlo, scale, sq, scale_hi), bit-exact against the header's
    arithmetic restated in numpy fp32 (sq: fp64, 1e-12)."""
    c = C.case(cid)
    with_hi = c.inp["w_hi"] is not None

    def run(inp, w):
        Ws = dev(inp["W"])
        m, n = inp["m"], inp["n"]
        e = lambda: torch.full((B, m * n), float("nan"), dtype=torch.float16, device=DEV)   # noqa: E731
        o = {"res": torch.full((B, m, n), float("nan"), device=DEV), "Y": torch.full((B, m, n), float("nan"), device=DEV),
             "hi": e(), "lo": e(), "thi": e(), "tlo": e(), "scale": torch.empty(B, device=DEV),
             "sq": torch.empty(B, dtype=torch.float64, device=DEV)}
        rows = w if w.dim() == 2 else w.view(1, -1).expand(B, -1)
        ymax = rows.amax(dim=1).contiguous()
        kw = {}
        if with_hi:
            o["scale_hi"] = torch.empty(B, device=DEV)
            kw = dict(ycol_hi=wbuf(inp["w_hi"][inp["_b"]] if "_b" in inp else inp["w_hi"]), ycol_hi_max=(ymax * ymax).contiguous(), scale_hi=o["scale_hi"])
        K.residual_split(Ws, dev(inp["packed"]).view(B, -1), dev(inp["qscale"]), inp["bits"], dev(inp["wmax"]), ycol=w,
                         ycol_max=ymax, res=o["res"], Y=o["Y"], hi=o["hi"], lo=o["lo"], thi=o["thi"], tlo=o["tlo"],
                         scale=o["scale"], sq=o["sq"], **kw)
        return o
    both(c, run)


# ------------------------------------------------------------------------------ sparse-code Gram
def _sgram_run(K, inp, w):
    k, L = inp["k"], inp["L"]
    W, packed, s = dev(inp["W"]), dev(inp["packed"]), dev(inp["s"])
    ns = -(-k // 64)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=DEV)   # noqa: E731
    row_nnz, perm, nz1, sw1 = i32(B * k), i32(B * k), i32(B * k), i32(B * ns)
    slice_off = torch.empty(B * (ns + 1), dtype=torch.int64, device=DEV)
    total = torch.empty(B, dtype=torch.int64, device=DEV)
    corr = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    Lh = K.sgram_split(k, L)
    K.sgram_count(packed, k, L, row_nnz, perm, slice_off, total, W=W, qscale=s, wcol=w,
                  corr_ws=torch.empty(B * k, dtype=torch.float64, device=DEV), corr_out=corr, Lh=Lh, row_nnz1=nz1,
                  slice_w1=sw1)
    stride = int(total.max().item()) + 64
    ell = torch.empty(B * stride, dtype=torch.int32, device=DEV)
    K.sgram_fill(packed, k, L, row_nnz, perm, slice_off, ell, stride, Lh=Lh, slice_w1=sw1)
    P = torch.full((B, k, k), float("nan"), device=DEV)
    K.sgram_spmm(W, packed, s, w, ell, perm, slice_off, stride, P, Lh=Lh, slice_w1=sw1)
    return {"corr": corr, "P_all": P, "P": P[:, dev(inp["rows"])]}


@pytest.mark.parametrize("cid", ids("sgram"))
def test_sgram_count_corr_and_spmm(K, cid):
    """cq_sgram_count's norm correction and cq_sgram_spmm with per-matrix wcol, in every form of
    the SpMM launcher (cq_sgram.hip, cq_sgram_spmm), each at its smallest contraction length:
    R = 8 staged rows (L <= 4800) with the results held in registers (k <= L: k = L = 64) and
    not (k = 256 > L = 64); R = 4 (L = 4864) with the LDS output block; the l-split (R = 2
    lengths whose half slab and output block fit: L = 9664, Lh = 4864); R = 2 unsplit (the half
    slab plus the k x 4 block no longer fit: L = 19136 at k = 64, 18752 at k = 256); and the
    register-held form with two row blocks per workgroup (k = L = 2752: 344 blocks x 3 matrices
    / 512 = 2; its reference covers every 43rd row of P, assertion 2 all of it)."""
    c = C.case(cid)
    k, L, form = c.inp["k"], c.inp["L"], c.inp["form"]
    R, Lh = K.sgram_rows(L), K.sgram_split(k, L)
    assert R == {"r8": 8, "r4": 4, "r2": 2, "ls": 2}[form[:2]] and (Lh < L) == (form == "lsplit")
    # the launcher's own conditions, restated: results held in registers, row blocks per workgroup
    held = k <= L and -(-(-(-k // 64)) // 16) * R <= 32 and R == 8
    nblk = -(-k // R)
    nb = max(1, min(8, nblk * B // 512, nblk)) if held else 1
    assert held == form.startswith("r8held") and nb == (2 if form.endswith("nb2") else 1)
    got = both(c, lambda inp, w: _sgram_run(K, inp, w), names=["corr", "P"])
    assert torch.isfinite(got["P_all"]).all()


# ------------------------------------------------------------------------------ sparse-code products
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("cid", ids("codes"))
def test_codes_matmul_and_ysq_corr(K, cid, trans):
    """cq_codes_matmul with colw alone, roww alone (the m > n shapes' row weights) and both,
    plain and transposed output, RV = 1 (r = 32) and RV = 4 (r = 200) columns per lane; and
    cq_codes_ysq_corr's colw."""
    c = C.case(cid)
    rows, cols, r = c.inp["rows"], c.inp["cols"], c.inp["r"]

    def run(inp, w):
        packed, X = dev(inp["packed"]), dev(inp["X"])
        rw = wbuf(inp["roww"][inp["_b"]] if "_b" in inp else inp["roww"])
        o = {}
        for name, kw in (("colw", dict(colw=w)), ("roww", dict(roww=rw)), ("both", dict(colw=w, roww=rw))):
            out = torch.full((B, r, rows) if trans else (B, rows, r), float("nan"), device=DEV)
            K.codes_matmul(packed, rows, cols, X, r, out, trans=trans, **kw)
            o[name] = out.transpose(1, 2) if trans else out
        if not trans:
            o["corr"] = K.codes_ysq_corr(packed, dev(inp["W"]), dev(inp["s"]), w)
        return o
    both(c, run)


# ------------------------------------------------------------------------------ fused Q update
def _q_run(K, inp, w, *, known=False, hint=None, codes=True):
    W = dev(inp["W"])
    m, n, r, bits = inp["m"], inp["n"], inp["r"], inp["bits"]
    L, R = (dev(inp["L"]), dev(inp["R"])) if r else (None, None)
    o = {"scale": torch.full((B,), float("nan"), device=DEV),
         "err": torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)}
    if bits <= 4:
        o["packed"] = torch.empty(B, m * n * bits // 8, dtype=torch.uint8, device=DEV)
    if codes:
        o["codes"] = torch.empty(B, m * n, dtype=K.code_dtype(bits), device=DEV)
    if hint is not None:
        o["fallback"] = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    K.q_update_x3(W, L, R, bits, codes=o.get("codes"), packed=o.get("packed"), scale=o["scale"], err_w=w,
                  err_out=o["err"], absmax_in=K.absmax(W) if known else None, scale_hint=hint,
                  fallback_out=o.get("fallback"))
    return o


def _q_check(case, b, got, ref):
    """Assertion 1 of the Q update: r = 0 bit-exact codes / scale; r > 0 the code and scale bars of
    test_q_update_x3_with_lr_matches_fp64_residual; err 1e-6 (see weight_stride_cases._q_update)."""
    m, n, bits = case.inp["m"], case.inp["n"], case.inp["bits"]
    import ee274_convexcaldera_llm_quantization_amd._lib as K
    codes = got["codes"][b] if "codes" in got else K.unpack_codes(got["packed"][b:b + 1], m * n, bits)[0]
    codes = codes.cpu().numpy().astype(np.int16)
    if "packed" in got:
        assert np.array_equal(got["packed"][b].cpu().numpy(), C.pack_codes(codes, bits))
    scale, err = float(got["scale"][b]), float(got["err"][b])
    if case.inp["r"] == 0:
        assert np.array_equal(codes, ref["codes"]) and scale == float(ref["scale"])
    else:
        flips = codes != ref["codes"]
        assert not (flips & ~ref["tie"]).any(), (case.id, b, int(flips.sum()))
        assert abs(scale - ref["scale"]) <= 1e-6 * ref["scale"]
    dev_ = abs(err - ref["err"]) / ref["err"]
    print(f"{case.id} matrix {b}: err relative deviation {dev_:.2e} (bar {case.tol['err']:.0e})")
    assert dev_ <= case.tol["err"], (case.id, b, err, ref["err"])


def _q_both(K, case, pad=64, **kw):
    got = _q_run(K, case.inp, wbuf(case.w, pad), **kw)
    for b in range(B):
        _q_check(case, b, got, case.ref(b, case.w[b]))
        check_same(case, b, got, _q_run(K, copies(case.inp, b), wbuf(case.w[b], pad), **kw))
    return got


@pytest.mark.parametrize("cid", ["q_update-stream-n1024", "q_update-stream-n1040", "q_update-stream-f32-b4-n1024"])
def test_q_update_stream(K, cid):
    """(a) r = 0 with max|W| known: quant_w_stream_kernel.  64 x 1024: 3 workgroups, a grid stride
    of 12288 elements = 12 rows, so each thread keeps its 16 weights across its groups (ewfix);
    64 x 1040: 12288 % 1040 != 0, the weights are reloaded per group."""
    c = C.case(cid)
    assert (3 * 256 * 16 % c.inp["n"] == 0) == (c.inp["n"] == 1024)
    _q_both(K, c, known=True)


def test_q_update_row_panel(K):
    """(b) the row-panel kernel, two passes (r = 32 <= 256, m % 16 == 0, n % 32 == 0, aligned):
    the geometry of test_q_update_list_at_capacity (m = 8 list regions of rows, n = 64)."""
    c = C.case("q_update-panel-256x64-r32")
    rows, _ = K.q_update_list_geometry(8 * 48, 64, 32)
    assert 8 * rows == c.inp["m"]
    _q_both(K, c, codes=False)


def test_q_update_candidate_lists(K):
    """(c) the single-recompute path (scale_hint, 2-bit packed codes, fp16 W) on the same shape:
    matrix 1's hint is 20 % high, so its list cannot be complete and it falls back to the second
    recompute while matrices 0 and 2 take their codes from the lists.  fallback_out as
    test_q_update_single_recompute_matches_two_pass asserts it; codes and scales bit-equal to the
    two-pass call with the same per-matrix weights, error sums to that test's 1e-7 (lists) and
    1e-12 (fallback); and both assertions of this file."""
    c = C.case("q_update-panel-256x64-r32")
    assert K.q_update_list_geometry(c.inp["m"], c.inp["n"], c.inp["r"]) is not None
    w = wbuf(c.w)
    two = _q_run(K, c.inp, w, codes=False)
    hi = torch.tensor([1.0, 1.2, 1.0], device=DEV)
    got = _q_run(K, c.inp, w, codes=False, hint=two["scale"] * hi)
    assert got["fallback"].tolist() == [0, 1, 0]
    assert torch.equal(got["packed"], two["packed"]) and torch.equal(got["scale"], two["scale"])
    for b in range(B):
        e, e0 = float(got["err"][b]), float(two["err"][b])
        assert abs(e - e0) <= (1e-12 if b == 1 else 1e-7) * e0, (b, e, e0)
        _q_check(c, b, got, c.ref(b, c.w[b]))
        inp = copies(c.inp, b)
        s = _q_run(K, inp, wbuf(c.w[b]), codes=False)["scale"]
        rep = _q_run(K, inp, wbuf(c.w[b]), codes=False, hint=s * hi)
        assert rep["fallback"].tolist() == [0, 1, 0]
        check_same(c, b, got, rep)


def test_q_update_tile_kernel(K):
    """(d) r = 288 > 256 keeps the row-panel kernel out: q_update_v_kernel (the 192 x 384 tile)."""
    _q_both(K, C.case("q_update-tile-64x64-r288"))


@pytest.mark.parametrize("pad", [64, 65])
def test_q_update_non_vector_kernel(K, pad):
    """(e) n = 52 (n % 16 != 0): q_update_x3_kernel, the non-vector form, with aligned and with
    misaligned weights."""
    _q_both(K, C.case("q_update-nonvec-64x52-r32"), pad)


@pytest.mark.parametrize("cid", ["q_update-panel-256x64-r32", "q_update-stream-n1024"])
def test_q_update_misaligned_weights_leave_the_vector_kernels(K, cid):
    """pad = 65: err_w is not 16-byte aligned, so the vector, row-panel and streaming kernels are
    out (vk false in cq_q_update_x3) and the non-vector kernel runs on the same data."""
    _q_both(K, C.case(cid), 65, known="stream" in cid)
