"""GPU-resident CALDERA engine (batched).  The hot path of the reference,
RCR/src/caldera/decomposition/alg.py:24-302, re-designed for MI355X:

  * B same-shape weight matrices are decomposed in lockstep, so the tall-skinny rank-r
    GEMMs and the one-workgroup-per-matrix p x p solvers fill the 256 CUs;
  * Q is never materialised in fp32 inside the loop: it lives as packed int2/int4 codes
    plus one scale, and is dequantised on the fly where it is consumed;
  * diagonal H (None, identity, or diag_embed(h) as main.py:163-165 passes) is a column
    weight vector — H_sqrt @ eigvecs (alg.py:66-68, :211) become exact column scalings;
  * the activation-aware error (alg.py:286-302) is fused into the producing kernel (the
    quantiser for Q updates, a GEMM epilogue for LR updates), accumulated in fp64;
  * the full SVD (alg.py:217) is replaced by RankRSolver (solver.py), warm-started
    across outer iterations.

State per matrix follows CalderaDecomposition (dataclasses.py:87-106).  Selection of the
best iterate reproduces alg.py:105-107 exactly (strict <, only once every update kind in
update_order has run).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from . import _lib as K
from . import qlog
from .overlap import run_to_end
from . import scratch
from . import sgram
from .solver import GRAM_PROBE, LPLR_PROBE, QUANT_PROBE, X3_SCALE, RandSVD, RankRSolver
from . import solver as _solver


@dataclass
class EngineParams:
    """Subset of CalderaParams (dataclasses.py:11-84) the engine consumes."""
    compute_quantized_component: bool = True
    compute_low_rank_factors: bool = True
    Q_bits: int = 2
    L_bits: int = 2
    R_bits: int = 2
    rank: int = 64
    iters: int = 20
    lplr_iters: int = 5
    activation_aware_LR: bool = True
    update_order: list = field(default_factory=list)
    method_Q: str = "uniform"
    method_LR: str = "uniform"
    rand_svd: bool = False
    sigma_reg: float = 0.0

    @classmethod
    def from_caldera_params(cls, qp):
        return cls(compute_quantized_component=qp.compute_quantized_component,
                   compute_low_rank_factors=qp.compute_low_rank_factors,
                   Q_bits=qp.Q_bits, L_bits=qp.L_bits, R_bits=qp.R_bits, rank=qp.rank,
                   iters=qp.iters, lplr_iters=qp.lplr_iters,
                   activation_aware_LR=qp.activation_aware_LR,
                   update_order=list(qp.update_order),
                   method_Q=qlog.engine_method(qp.quant_factory_Q),
                   method_LR=qlog.engine_method(qp.quant_factory_LR),
                   rand_svd=qp.rand_svd, sigma_reg=qp.sigma_reg)


# solver test tightening for activation-weighted Y (see _lr_update)
WEIGHTED_TOL_FACTOR = 0.25

# below this relative error the Pythagorean LR error (||Y||^2 - ||R||_h^2, fp32-grade R) has
# lost more than ~1e-5 absolute accuracy to cancellation; such errors are recomputed directly
PYTH_MIN_ERR = 3e-2


def _uniform_k(bits):
    return 2 ** (bits - 1) - 1


class _Weights:
    """Column weights derived from a diagonal H (alg.py:44-68 for diagonal H).

    err   : diag of the H used by activation_aware_error (after the sigma_reg shift)
    ycol  : diag of H_sqrt (data-aware) — Y = residual * ycol  (alg.py:211)
    rinv  : 1/sqrt(eigenvalues) in original column order (alg.py:223)
    lplr  : weights of ||(res - L R) H_sqrt||^2 (alg.py:182): ycol^2 (aware) / h^2 (not)

    Shared H: (n,) vectors and a float ycol_max.  Per-matrix diagonal H (`batched`, h (B, n):
    main.py:163-165 gives every layer its own Hall[name]): (B, n) vectors, row b matrix b's,
    and ycol_max (B,) fp32 -- the kernels read row b at a batch stride (ABI 5).  Every row takes
    the same arithmetic as a shared h would (the sigma_reg shift only where that row needs
    it), so a matrix gets the same weights in a mixed batch as alone.  The flags (identity,
    err_unit) choose code paths and must agree over the batch (`kind` groups callers' matrices).
    """

    dense = False

    def __init__(self, h: torch.Tensor | None, n: int, p: EngineParams, dev, batched: bool = False):
        f32 = torch.float32
        if batched:
            self._init_batched(h.to(device=dev, dtype=f32), n, p, dev)
            return
        if h is not None and h.dim() == 2:
            self._init_dense(h.to(device=dev, dtype=f32), n, p, dev)
            return
        if h is None:
            h = torch.ones(n, dtype=f32, device=dev)
        h = h.to(device=dev, dtype=f32)
        if not p.activation_aware_LR:
            self.err = h
            self.err_unit = bool(torch.all(h == 1.0).item())
            self.ycol = None
            self.ycol_max = 1.0
            self.rinv = None
            self.lplr = h * h
            self.identity = False
            return
        # optimized_eigh (alg.py:11-23): allclose(H, I) -> eigenvalues exactly 1
        ident = bool(torch.all(torch.abs(h - 1.0) <= 1e-8 + 1e-5).item())
        lam = torch.ones_like(h) if ident else h.clone()
        herr = h.clone()
        lmin = lam.min()
        if float(lmin.item()) < p.sigma_reg:  # alg.py:59-64 (fp32 arithmetic, as torch)
            shift = torch.tensor(p.sigma_reg, dtype=f32, device=dev) - lmin
            herr = herr + shift
            lam = lam + shift
        self.identity = ident and bool(torch.all(lam == 1.0).item())
        self.err = herr
        sq = torch.sqrt(lam)
        self.ycol = None if self.identity else sq
        self.ycol_max = 1.0 if self.identity else float(sq.max().item())
        self.rinv = None if self.identity else 1.0 / sq
        self.lplr = None if self.identity else lam  # ||Y - L (R*ycol)||^2 uses unit weights
        self.err_unit = bool(torch.all(herr == 1.0).item())

    @staticmethod
    def kind(h: torch.Tensor | None, n: int, p: EngineParams, dev) -> tuple:
        """(identity, err_unit) of one matrix's diagonal h: matrices batched with per-matrix
        weights must agree on them (they select code paths, not values)."""
        w = _Weights(h, n, p, dev)
        return (w.identity, w.err_unit)

    def _init_batched(self, h: torch.Tensor, n: int, p: EngineParams, dev):
        """Per-matrix diagonal H, h (B, n): row b is what _Weights(h[b]) computes for that
        matrix alone (alg.py:11-23, :44-68), evaluated for all rows at once."""
        f32 = torch.float32
        B = h.shape[0]
        assert h.dim() == 2 and h.shape[1] == n
        h = h.contiguous()
        if not p.activation_aware_LR:
            unit = torch.all(h == 1.0, dim=1).tolist()
            if len(set(unit)) > 1:
                raise ValueError("per-matrix H: unit and non-unit error weights in one batch (group by _Weights.kind)")
            self.err = h
            self.err_unit = unit[0]
            self.ycol = None
            self.ycol_max = 1.0
            self.rinv = None
            self.lplr = (h * h).contiguous()
            self.identity = False
            return
        ident = torch.all(torch.abs(h - 1.0) <= 1e-8 + 1e-5, dim=1)  # optimized_eigh per matrix
        lam = torch.where(ident.view(B, 1), torch.ones_like(h), h)
        herr = h.clone()
        lmin = lam.min(dim=1).values
        # alg.py:59-64 per matrix: the comparison in double as float(lmin.item()) < sigma_reg,
        # the shift in fp32 (sigma_reg - lmin) added only to the rows that need it
        need = (lmin.double() < p.sigma_reg).view(B, 1)
        shift = (torch.tensor(p.sigma_reg, dtype=f32, device=dev) - lmin).view(B, 1)
        herr = torch.where(need, herr + shift, herr)
        lam = torch.where(need, lam + shift, lam)
        identity = (ident & torch.all(lam == 1.0, dim=1)).tolist()
        err_unit = torch.all(herr == 1.0, dim=1).tolist()
        if len(set(identity)) > 1 or len(set(err_unit)) > 1:
            raise ValueError("per-matrix H: identity and non-identity weights in one batch (group by _Weights.kind)")
        self.identity = identity[0]
        self.err = herr.contiguous()
        sq = torch.sqrt(lam).contiguous()
        self.ycol = None if self.identity else sq
        self.ycol_max = 1.0 if self.identity else sq.max(dim=1).values.contiguous()
        self.rinv = None if self.identity else (1.0 / sq).contiguous()
        self.lplr = None if self.identity else lam.contiguous()
        self.err_unit = err_unit[0]


    def _init_dense(self, H, n, p: EngineParams, dev):
        """Non-diagonal H (alg.py:44-68).  H's eigendecomposition is a one-off setup step
        (torch.linalg.eigh on the device, i.e. rocSOLVER; the reference calls
        torch.linalg.eigh too); everything per iteration is GEMMs in libcaldera_hip.so:

        data-aware: Hs = (H + H^T)/2 = V diag(lam) V^T, lam shifted by sigma_reg - lam_min
          when lam_min < sigma_reg (:59-64).  H_sqrt V = V diag(sqrt lam) =: Vs, so
          Y = res @ H_sqrt @ V = res @ Vs (:211), R = R~ diag(1/sqrt lam) V^T = R~ @ Vinv^T
          with Vinv = V diag(1/sqrt lam) (:219-225), (R H_sqrt)(R H_sqrt)^T = (R Vs)(R Vs)^T
          for the LPLR normal equations (:162-169) and ||X H_sqrt||^2 = ||X Vs||^2 (:182).
        not data-aware: H_sqrt = H itself (:47-49); the LPLR error ||X H||^2 uses H as given.
        error (:286-302): tr(E H E^T) = sum_k lam_k ||E v_k||^2 over the eigenpairs of the
          symmetrised H (shifted for data-aware, as the reference reassigns H)."""
        self.dense = True
        self.identity = False
        self.ycol = self.rinv = self.lplr = None
        self.err = None
        self.err_unit = True
        self.ycol_max = 1.0
        Hs = (H + H.t()) * 0.5
        lam, V = torch.linalg.eigh(Hs)
        V = V.contiguous()
        if p.activation_aware_LR:
            lmin = lam.min()
            if float(lmin.item()) < p.sigma_reg:
                lam = lam + (torch.tensor(p.sigma_reg, dtype=lam.dtype, device=dev) - lmin)
            sq = torch.sqrt(lam)
            self.Vs = K.scale_rc(V, colscale=sq)[0]
            self.Vinv = K.scale_rc(V, colscale=1.0 / sq)[0]
            self.H_lplr = None
        else:
            self.Vs = self.Vinv = None
            self.H_lplr = H.contiguous()
        self.Ve, self.lam_e = V.contiguous(), lam.contiguous()

    def dense_err(self, E: torch.Tensor, tmp: torch.Tensor) -> torch.Tensor:
        """tr(E H E^T) per matrix = sum_k lam_k ||E v_k||^2 (E (B, m, n) fp32; tmp same shape)."""
        K.gemm(E, self.Ve, C=tmp)
        return K.weighted_sqsum(tmp, self.lam_e, self.lam_e.numel())


class BatchState:
    """Per-batch decomposition state.  Uniform Q lives as packed codes + one scale per
    matrix (dequantised on the fly); the codebook methods (nf4/nf2/bbint) keep their dense
    fp32 Q (`Qd`, with a bound `Qbound` on |Q|) and per-matrix (codes, params) items in the
    reference's return layout.  Codebook L/R idxs/scales are per-matrix lists likewise."""

    def __init__(self, B, m, n, r, p: EngineParams, dev):
        self.B, self.m, self.n, self.r = B, m, n, r
        f32 = torch.float32
        numel = m * n
        self.dense_q = p.method_Q != "uniform"
        self.Qd = self.Qbound = None
        self.q_items = [None] * B
        self.q_packed = p.Q_bits <= 4 and numel % 4 == 0 and not self.dense_q
        if self.dense_q:
            numel = 1  # the uniform code buffers are unused
        self.qcode_numel = numel * p.Q_bits // 8 if self.q_packed else numel
        qdt = torch.uint8 if self.q_packed else K.code_dtype(p.Q_bits)
        self.Qc = torch.zeros((B, self.qcode_numel), dtype=qdt, device=dev)  # codes (Q=0: see has_Q)
        self.Qs = torch.zeros(B, dtype=f32, device=dev)
        self.has_Q = False
        self.L = torch.zeros((B, m, r), dtype=f32, device=dev)
        self.R = torch.zeros((B, r, n), dtype=f32, device=dev)
        self.has_LR = False
        self.L_idxs = self.R_idxs = None
        self.L_scale = self.R_scale = None
        self._vers = None  # best-state snapshots (snapshot_into / materialize)
        self._pick = None

    def snapshot_into(self, dst: "BatchState", sel: list[int]):
        """Make the current state of matrices `sel` dst's best (alg.py:96-107).  Nothing is
        copied: every Q and LR update writes fresh tensors (codes, scales, factors), so a
        snapshot keeps references to the current tensors and, per matrix, which snapshot it
        picked; materialize() assembles dst's tensors once, at the end of the run."""
        B = self.B
        if self.dense_q and self.has_Q:
            # codebook Q: every Q update allocates fresh tensors, so the snapshot keeps views
            if dst.Qd is None:
                dst.Qd = [None] * B
            for b in sel:
                dst.Qd[b] = self.Qd[b]
                dst.q_items[b] = self.q_items[b]
        if isinstance(self.L_idxs, list):
            if not isinstance(dst.L_idxs, list):
                dst.L_idxs, dst.R_idxs = [None] * B, [None] * B
                dst.L_scale, dst.R_scale = [None] * B, [None] * B
            for b in sel:
                dst.L_idxs[b], dst.R_idxs[b] = self.L_idxs[b], self.R_idxs[b]
                dst.L_scale[b], dst.R_scale[b] = self.L_scale[b], self.R_scale[b]
            idxs = None
        else:
            idxs = (self.L_idxs, self.R_idxs, self.L_scale, self.R_scale) if self.L_idxs is not None else None
        if dst._vers is None:  # version 0: dst's own (zero) tensors, for matrices never picked
            dst._vers = {0: (dst.Qc, dst.Qs, dst.L, dst.R, None)}
            dst._pick = [0] * B
        vid = max(dst._vers) + 1
        dst._vers[vid] = (self.Qc, self.Qs, self.L, self.R, idxs)
        for b in sel:
            dst._pick[b] = vid
        live = set(dst._pick)
        dst._vers = {v: t for v, t in dst._vers.items() if v in live}
        for b in sel:
            dst.flag_Q[b] = self.has_Q
            dst.flag_LR[b] = self.has_LR

    def materialize(self):
        """The picked snapshot's tensors per matrix (snapshot_into): references when every
        matrix picked the same snapshot, else one gather per snapshot used."""
        if self._vers is None:
            return
        picks = self._pick
        used = sorted(set(picks))
        if len(used) == 1:
            qc, qs, L, R, idxs = self._vers[used[0]]
            self.Qc, self.Qs, self.L, self.R = qc, qs, L, R
            if idxs is not None:
                self.L_idxs, self.R_idxs, self.L_scale, self.R_scale = idxs
        else:
            # the snapshot most matrices picked becomes the result in place (the snapshots are
            # dead after this); the others' matrices are gathered into it
            base = max(used, key=lambda v: sum(1 for x in picks if x == v))
            qc, qs, L, R, idxs = self._vers[base]
            out = [qc, qs, L, R]
            oidx = list(idxs) if idxs is not None else None
            if oidx is None and any(self._vers[v][4] is not None for v in used):
                ref = next(self._vers[v][4] for v in used if self._vers[v][4] is not None)
                oidx = [torch.zeros_like(t) for t in ref]
            for v in used:
                if v == base:
                    continue
                sel = [b for b in range(self.B) if picks[b] == v]
                idx = torch.tensor(sel, dtype=torch.long, device=qc.device)
                # version 0 (never picked: the initial zero state) takes the picked snapshots'
                # shapes -- its own L / R have width rank, an LR update's min(rank, m, n)
                src = self._vers[v] if v else (*[torch.zeros_like(t) for t in out], None)
                for d, s in zip(out, src[:4]):
                    d.index_copy_(0, idx, s.index_select(0, idx))
                if oidx is not None and src[4] is not None:
                    for d, s in zip(oidx, src[4]):
                        d.index_copy_(0, idx, s.index_select(0, idx))
            self.Qc, self.Qs, self.L, self.R = out
            if oidx is not None:
                self.L_idxs, self.R_idxs, self.L_scale, self.R_scale = oidx
        self._vers = None


class CalderaEngine:
    """Decomposes a batch of B weight matrices (B, m, n) with shared params and H."""

    def __init__(self, params: EngineParams, *, solver_tol: float = 1e-5, solver_p: int | None = None,
                 filter_precision: str = "f16x3", profile: bool = False, solver_kwargs: dict | None = None):
        self.p = params
        self.solver_kwargs = dict(solver_kwargs or {})
        self.solver_tol = solver_tol
        # tolerances of the first LR updates (then solver_tol): the codes of the next Q update
        # are decided on the L R of the one before it (alg.py:262), see DESIGN.md §6
        self.solver_tol_steps = None
        # per LR update: degrees of extra full outer iterations after the solver's test passed
        self.solver_refine_steps = None
        self._lr_step = 0
        self.solver_p = solver_p
        self.filter_precision = filter_precision
        self.profile = profile
        self.timings = {}
        self.solver = None
        self._qfb = None  # (B,) int32 on the device: Q updates that took the second L R recompute
        self.q_single_recompute = True  # 2-bit Q updates: one L R recompute + candidate lists
        self.lplr_fused_err = True   # LPLR error from the normal-equation pieces (False: error GEMM)
        self.lplr_x3 = True          # LPLR m x n x r products on split-fp16 MFMAs where the halves exist
        self.sparse_gram = True      # G from the sparse 2-bit codes where it applies (sgram.py)
        self.r_from_codes = True     # with it, R = U^T W - s U^T c and ||Y||^2 without a residual pass
        self.lplr_trace = None       # list -> per-LPLR-iteration errors are appended (diagnostics)
        self._s_bm = None            # split scale of the last Y Rw^T product (lplr_rhs -> lplr_L_from)
        for meth in (params.method_Q, params.method_LR):
            if meth not in qlog.METHODS:
                raise NotImplementedError(f"Quantization method '{meth}' not supported yet.")

    @property
    def q_fallbacks(self) -> int:
        """Q updates (summed over the batch) whose candidate list could not be complete, so
        that L R was recomputed a second time (cq_q_update_x3); reads the device counter."""
        return 0 if self._qfb is None else int(self._qfb.sum().item())

    # ------------------------------------------------------------------ pieces
    def _q_update(self, st: BatchState, Ws, res_buf, wts: _Weights, den):
        """maybe_update_Q / update_Q_non_data_aware (alg.py:253-283) + error (:286-302)."""
        p = self.p
        B, m, n = st.B, st.m, st.n
        Kdim = st.L.shape[-1] if (p.compute_low_rank_factors and st.has_LR) else 0
        if st.dense_q:
            return self._q_update_codebook(st, Ws, res_buf, wts, Kdim)
        # fresh code / scale tensors for every update: the best-state snapshots keep references
        # to earlier ones instead of copying them (BatchState.snapshot_into)
        prev_qs = st.Qs
        st.Qc = torch.empty_like(st.Qc)
        st.Qs = torch.empty_like(st.Qs)
        if Kdim % 32 == 0:
            # fused: res = W - L R recomputed per tile on split-fp16 products, never stored
            err = torch.empty(B, dtype=torch.float64, device=Ws.device)
            Lm = st.L if Kdim else None
            Rm = st.R if Kdim else None
            # algorithmic bytes of a quantise call: W read once, packed codes
            # written; the rank-r recompute adds 2 m n r flops (fp32-equivalent)
            ev = QUANT_PROBE.start("lr" if Kdim else "w", 2.0 * B * m * n * Kdim,
                                   B * (m * n * Ws.element_size() + m * n * p.Q_bits / 8.0 + 4))
            # first Q step: res = W, whose max |.| is already known (self._wmax): one pass over W
            amax = self._wmax if not Kdim else None
            ew = None if wts.err_unit else wts.err  # unit weights: the same sums without the loads
            if st.q_packed:
                # the previous scale lets a 2-bit update recompute L R once (candidate lists;
                # cq_q_update_x3); the per-matrix count of second recomputes is accumulated on
                # the device (q_fallbacks)
                hint = prev_qs if (Kdim and st.has_Q and self.q_single_recompute) else None
                fb = None
                if hint is not None:
                    if self._qfb is None or self._qfb.numel() != B:
                        self._qfb = torch.zeros(B, dtype=torch.int32, device=Ws.device)
                    fb = torch.empty(B, dtype=torch.int32, device=Ws.device)
                K.q_update_x3(Ws, Lm, Rm, p.Q_bits, packed=st.Qc, scale=st.Qs, err_w=ew, err_out=err, events=ev,
                              absmax_in=amax, scale_hint=hint, fallback_out=fb)
                if fb is not None:
                    self._qfb += fb
            else:
                K.q_update_x3(Ws, Lm, Rm, p.Q_bits, codes=st.Qc, scale=st.Qs, err_w=ew, err_out=err, events=ev,
                              absmax_in=amax)
            st.has_Q = True
            return err
        absmax = torch.zeros(B, dtype=torch.int32, device=Ws.device)  # |res| max as uint32 bits
        Lm = st.L[:, :, :Kdim]
        Rm = st.R[:, :Kdim, :]
        # res = W - L R  (alg.py:262; RESID epilogue also produces |res| max for the quantiser)
        K.gemm(Lm, Rm, C=res_buf, D=Ws, epi=K.EPI_RESID, absmax=absmax, batch=B)
        err = torch.empty(B, dtype=torch.float64, device=Ws.device)
        x = res_buf.view(B, m * n)
        if st.q_packed:
            K.quantize_known_max(x, absmax, p.Q_bits, packed=st.Qc, scale=st.Qs, err_w=wts.err,
                                 err_ncols=n, err_out=err)
        else:
            K.quantize_known_max(x, absmax, p.Q_bits, codes=st.Qc, scale=st.Qs, err_w=wts.err,
                                 err_ncols=n, err_out=err)
        st.has_Q = True
        return err

    def _q_update_codebook(self, st: BatchState, Ws, res_buf, wts: _Weights, Kdim):
        """Q update with a codebook quantiser (nf4/nf2/bbint4/bbint2/nf4_std/nf2_std): res = W - L R
        (alg.py:262) into the fp32 work buffer, then the whole-matrix quantiser
        (alg.py:245-250) with the error sum_j h_j (deq - res)^2 fused."""
        p = self.p
        B, m, n = st.B, st.m, st.n
        dev = Ws.device
        if Kdim:
            absmax = torch.zeros(B, dtype=torch.int32, device=dev)
            K.gemm(st.L, st.R, C=res_buf, D=Ws, epi=K.EPI_RESID, absmax=absmax, batch=B)
        else:
            K.build_residual(Ws, None, None, 2, None, res=res_buf)
        x = res_buf.view(B, m * n)
        err = torch.empty(B, dtype=torch.float64, device=dev)
        items, deq = self._quantize_whole(x, p.method_Q, p.Q_bits, err_w=wts.err, err_ncols=n, err_out=err)
        st.Qd = deq.view(B, m, n)
        st.Qbound = K.absmax(st.Qd)
        st.q_items = items
        st.has_Q = True
        return err

    def _quantize_whole(self, x, method, bits, **err):
        """quantize_matrix (alg.py:245-250) of B matrices x (B, numel) with a codebook method:
        returns ([(A_idxs (1, ...), params)] per matrix in the reference's layout, deq (B, numel))."""
        B, numel = x.shape
        if method in ("nf4", "nf2"):
            out = K.quantize_nf(x, numel, qlog.code_bits(method, bits), **err)
            return [(out["idx"][b].view(1, -1), out["scale"][b].view(1, 1)) for b in range(B)], out["deq"]
        if method in ("nf4_std", "nf2_std"):  # params: the pair (mean, std)
            out = K.quantize_nf_std(x, numel, qlog.code_bits(method, bits), **err)
            return [(out["idx"][b].view(1, -1), (out["mean"][b].view(1, 1), out["std"][b].view(1, 1)))
                    for b in range(B)], out["deq"]
        cb = qlog.code_bits(method, bits)
        if numel % (8 // cb):
            raise RuntimeError(f"{method}: {numel} elements do not pack {8 // cb} codes per byte")
        out = K.quantize_bbint(x, numel, cb, **err)
        items, off = [], 0
        for b in range(B):
            k = out["n_out"][b]
            qlog.log_outliers(id(self) + b, k)  # one reference quantizer call per matrix
            items.append((out["packed"][b].view(1, -1),
                          (out["bmin"][b].view(1, 1), out["bscale"][b].view(1, 1), out["vals"][off:off + k],
                           out["idx"][off:off + k])))
            off += k
        return items, out["deq"]

    def _lr_update(self, st: BatchState, Ws, Y, res, wts: _Weights, den):
        """maybe_update_LR / update_LR / LR_init (alg.py:115-235) + error (:286-302)."""
        p = self.p
        B, m, n = st.B, st.m, st.n
        dev = Ws.device
        quantized = p.L_bits < 16 or p.R_bits < 16
        weighted = p.activation_aware_LR and (wts.ycol is not None or wts.dense)
        if self._w_finite is None:  # once per run (one small read-back)
            self._w_finite = bool(torch.isfinite(self._wmax).all().item())
        if not self._w_finite:
            # the reference's LR_init SVD (alg.py:217 / :232) raises on a non-finite residual
            raise torch.linalg.LinAlgError("linalg.svd: The algorithm failed to converge because the input "
                                           "matrix contained non-finite values.")
        if self.solver is None and p.rand_svd:  # torch.svd_lowrank branch (alg.py:213-216, :228-231)
            self.solver = RandSVD(B, m, n, p.rank, dev)
        if self.solver is None:
            # the solver's test bounds the relative error of the rank-r projection of Y in the
            # weighted space; the caller compares Q + L R unweighted, where the columns with
            # small h_j amplify it (2.4-4.5x at main.py's real Hessians, tools/crit_probe.py):
            # weighted problems run to a 4x tighter test
            self.solver = RankRSolver(B, m, n, p.rank, dev, tol=self.solver_tol, p=self.solver_p,
                                      filter_precision=self.filter_precision, **self.solver_kwargs)
            if not self.solver.left and self._n_true < n:
                self.solver.valid_k = self._n_true
        sv = self.solver
        if isinstance(sv, RankRSolver):
            # per-LR-step tolerance (solver_tol_steps[i] for the i-th LR update, then
            # solver_tol); weighted problems run to a tighter test (WEIGHTED_TOL_FACTOR)
            steps = self.solver_tol_steps or ()
            tol = steps[self._lr_step] if self._lr_step < len(steps) else self.solver_tol
            sv.tol = tol if weighted is False else tol * WEIGHTED_TOL_FACTOR
            # refinement iterations after convergence for the first LR steps (solver_refine_steps[i]:
            # filter degrees of the extra full outer iterations of the i-th LR update)
            rs = self.solver_refine_steps or ()
            sv.refine = tuple(rs[self._lr_step]) if self._lr_step < len(rs) else ()
        self._lr_step += 1
        y_split = None
        gram = None
        ysq = None
        lplr_halves = None
        self._r_lite = False
        if st.dense_q and st.has_Q:
            qsrc, qsc, qbits = st.Qd, st.Qbound, 32
        else:
            qsrc, qsc, qbits = (st.Qc, st.Qs, p.Q_bits) if st.has_Q else (None, None, p.Q_bits)
        if wts.dense:
            # res = W - Q; data-aware Y = res @ H_sqrt @ V = res @ Vs (alg.py:211)
            K.build_residual(Ws, qsrc, qsc, qbits, None, res=res)
            if weighted:
                K.gemm(res, wts.Vs, C=Y)
        elif sv.x3 and not sv.direct and m % 32 == 0 and n % 64 == 0 and (st.q_packed or st.dense_q):
            # one pass: the solver's Gram operand halves, ||Y||^2 and, for m <= n, the halves of
            # Y^T (operand of R = U^T Y on split-fp16 products); res / Y in fp32 only where a
            # later step still reads them (quantised factors, wide-right shapes)
            if self._yh is None:  # cached scratch (scratch.py)
                # shaped as the Gram operand (Y, or Y^T when m > n): the split products take
                # their M / K from these shapes
                gshape = (B, m, n) if sv.left else (B, n, m)
                self._yh = scratch.get("lr.yh", gshape, torch.float16, dev)
                self._yl = scratch.get("lr.yl", gshape, torch.float16, dev)
                self._ys = torch.empty(B, dtype=torch.float32, device=dev)
            ysq = torch.empty(B, dtype=torch.float64, device=dev)
            # the LR error then comes by Pythagoras (below), which needs the error weights to be
            # Y's own column weights: an H that passes allclose(H, I) (optimized_eigh, alg.py:11-23:
            # unit eigenvalues) but is not exactly 1 keeps its h in the error (alg.py:286-302),
            # so that case writes res and takes the fused error GEMM
            pyth_ok = wts.ycol is not None or wts.err_unit
            x3_r = sv.left and not quantized and p.activation_aware_LR and pyth_ok
            # quantised factors with unweighted Y (= res): the LPLR loop's m x n x r products run
            # on split-fp16 MFMAs from these halves (Y for Y R^T, res^T = Y^T for L^T res)
            x3_lplr = sv.left and quantized and not weighted and self.lplr_x3
            # sparse 2-bit codes: G = A - s (P + P^T) (sgram.py) instead of the dense Gram of
            # Y's halves, which are then only written where another product reads them
            sparse_g = (self.sparse_gram and sv.left and st.has_Q and st.q_packed and not st.dense_q
                        and sgram.applicable(m, n, Ws, p.Q_bits, True, wts.dense))
            # R = U^T Y without a residual pass (2-bit codes, unquantised factors): U^T (W diag(ycol))
            # from W's transposed halves written once per run, minus s (U^T c) diag(ycol) from the
            # sparse codes (cq_codes_matmul); ||Y||^2 = ||W diag(ycol)||^2 + the codes' correction
            # (cq_codes_matmul takes r <= 256 columns of U: larger ranks keep the residual pass)
            lite = (sparse_g and x3_r and not x3_lplr and p.Q_bits == 2 and self.r_from_codes
                    and sv.r <= K.CODES_MATMUL_MAX_R)
            # m > n (gate/up projections): the same sparse-code Gram on the transposed problem,
            # G = Y^T Y = (W^T - s c^T)(W^T - s c^T)^T from W^T (once per run) and c^T (per step);
            # unweighted Y and unquantised factors (L = W V - s c V from W's halves and the codes)
            tall = (self.sparse_gram and not sv.left and st.has_Q and st.q_packed and not st.dense_q and not weighted
                    and not quantized and p.Q_bits == 2 and self.r_from_codes
                    # nothing writes res on this path: the LR error must come by Pythagoras
                    # (pyth_right below, unit error weights); codes_matmul takes r <= 256
                    and wts.err_unit and wts.ycol is None and sv.r <= K.CODES_MATMUL_MAX_R
                    and sgram.applicable(n, m, Ws, p.Q_bits, True, wts.dense))
            if tall and self._sg_A is None:  # once per run: W^T, A = W^T W, W's halves, ||W||^2
                self._wt16 = K.transpose_f16(Ws, out=scratch.get("sgram.wt", (B, n, m), torch.float16, dev))
                self._sg_A = scratch.get("sgram.A", (B, n, n), torch.float32, dev)
                self._sg = sgram.SparseGram(B, n, m, dev)
                self._sg_w = None
                Gh, Gl = sv.gram_halves(dev)
                self._wth = scratch.get("lr.wth", (B, m, n), torch.float16, dev)
                self._wtl = None  # W's halves are exact (lo = 0, sgram.gram_A): b_exact products
                self._ysw = torch.empty(B, dtype=torch.float32, device=dev)
                self._wsq = torch.empty(B, dtype=torch.float64, device=dev)
                with GRAM_PROBE.timed("gram_A", 1.0 * n * n * m * B, 2.0 * m * n * B + 4.0 * n * n * B):
                    sgram.gram_A(self._wt16, None, 1.0, self._wmax, self._sg_A, Gh, Gl, X3_SCALE, self._yh,
                                 self._yl, ys=self._ysw, wth=self._wth, wtl=self._wtl, wsq=self._wsq)
            if tall:
                ct = scratch.get("sgram.codes_t", st.Qc.shape, torch.uint8, dev)
                K.codes_transpose(st.Qc, m, n, out=ct)
                if self._sg.count(ct, self._wt16, st.Qs) > sgram.MAX_DENSITY * m * n:
                    tall = False  # too many nonzero codes this step: dense Gram
                else:
                    sparse_g = lite = True
            if sparse_g and not tall and self._sg_A is None:  # once per run: A = W diag(w) W^T
                self._sg_A = scratch.get("sgram.A", (B, m, m), torch.float32, dev)
                self._sg = sgram.SparseGram(B, m, n, dev, split=not weighted)
                self._sg_w = (wts.ycol * wts.ycol).contiguous() if weighted else None
                Gh, Gl = sv.gram_halves(dev)
                if lite:
                    self._wth = scratch.get("lr.wth", (B, n, m), torch.float16, dev)
                    # W^T's halves are exact (lo = 0, sgram.gram_A), not written; diagonal H
                    # enters R = (U^T W) diag(ycol) in the product's epilogue
                    self._wtl = None
                    self._ysw = torch.empty(B, dtype=torch.float32, device=dev)
                    self._wsq = torch.empty(B, dtype=torch.float64, device=dev)
                # fp16 MFMA work: one product over the upper half (H = I: W's halves are W and 0),
                # else the three split products; bytes: the operand halves read once, A written
                nprod = 3.0 if weighted else 1.0
                with GRAM_PROBE.timed("gram_A", nprod * m * m * n * B, (4.0 if weighted else 2.0) * m * n * B
                                      + 4.0 * m * m * B):
                    sgram.gram_A(Ws, wts.ycol if weighted else None, wts.ycol_max if weighted else 1.0, self._wmax,
                                 self._sg_A, Gh, Gl, X3_SCALE, self._yh, self._yl,
                                 **(dict(ys=self._ysw, wth=self._wth, wtl=self._wtl, wsq=self._wsq) if lite else {}))
            if sparse_g and not tall:
                # (the codes' norm correction of ||Y||^2 comes with the count where it is used)
                corr = dict(W=Ws, qscale=st.Qs, wcol=self._sg_w) if lite and self._wth is not None else {}
                if self._sg.count(st.Qc, **corr) > sgram.MAX_DENSITY * m * n:
                    sparse_g = False  # too many nonzero codes this step: dense Gram
            lite = lite and sparse_g and self._wth is not None
            self._r_lite = lite
            if lite:
                self.lr_steps_from_codes += 1
                # no pass over Y at all: ||Y||^2 from ||W diag(ycol)||^2 and the nonzero codes
                ysq = self._wsq + self._sg.ysq_corr
            else:
                halves = ({} if sparse_g and not x3_lplr else dict(hi=self._yh, lo=self._yl)) if sv.left else \
                    dict(thi=self._yh, tlo=self._yl)
                if x3_r or x3_lplr:
                    if self._yth is None:
                        self._yth = scratch.get("lr.yth", (B, n, m), torch.float16, dev)
                        self._ytl = scratch.get("lr.ytl", (B, n, m), torch.float16, dev)
                    halves.update(thi=self._yth, tlo=self._ytl)
                # m > n: Y's own halves (K-blocked over n) for L = Y V on split-fp16 products
                x3_yv = not sv.left and self.lplr_x3
                if x3_yv:
                    if self._yrh is None:
                        self._yrh = scratch.get("lr.yrh", (B, m, n), torch.float16, dev)
                        self._yrl = scratch.get("lr.yrl", (B, m, n), torch.float16, dev)
                    halves.update(hi=self._yrh, lo=self._yrl)
                K.residual_split(Ws, qsrc, qsc, qbits, self._wmax,
                                 ycol=wts.ycol if weighted else None, ycol_max=wts.ycol_max if weighted else 1.0,
                                 res=None if x3_r else res, Y=Y if (weighted and not x3_r) else None,
                                 scale=self._ys, sq=ysq, **halves)
            if sparse_g:
                # tall: the Gram of Y^T's rows from W^T and the transposed codes
                gw, qc = (self._wt16, ct) if tall else (Ws, st.Qc)
                qs, A, SG, w = st.Qs, self._sg_A, self._sg, self._sg_w

                def fill(Gh, Gl, gscale, ginv, G32=None):
                    SG.gram(gw, qc, qs, w, A, ysq, Gh, Gl, gscale, ginv, X3_SCALE, G32=G32, counted=True)

                gram = dict(fill=fill, ysq=ysq)
            else:
                y_split = (self._yh, self._yl, self._ys, ysq)
            if x3_lplr:
                lplr_halves = dict(yh=self._yh, yl=self._yl, ys=self._ys, yth=self._yth, ytl=self._ytl)
        else:
            K.build_residual(Ws, qsrc, qsc, qbits, wts.ycol, Y=Y if weighted else None, res=res)
        Ysrc = Y if weighted else res  # Y = res * sqrt(h) (alg.py:211); identity H: Y = res
        Y = Ysrc
        if gram is not None:
            vecs, theta = yield from sv.solve_iter(Ysrc, gram=gram)
        else:
            vecs, theta = yield from sv.solve_iter(Ysrc, y_split=y_split)
        rand = isinstance(sv, RandSVD)
        r = sv.r
        S = torch.sqrt(theta.clamp_min(0.0))  # singular values (fp64)
        S32 = S.float()
        tiny = (S32 <= S32[:, :1] * 1e-30) | (S32 == 0)
        L = torch.empty((B, m, r), dtype=torch.float32, device=dev)
        R = torch.empty((B, r, n), dtype=torch.float32, device=dev)
        yv2 = None  # ||Y V||^2 of the right-side Pythagorean error (m > n)
        if sv.left:
            U = vecs  # (B, m, r) view, ld p
            if p.activation_aware_LR:
                L.copy_(U)
                # R = (U^T Y) diag(1/sqrt(lam))   (alg.py:219-225); randomized: S Vh as returned
                if rand:
                    R.copy_(sv.SVh)
                elif self._r_lite:
                    self._ut_w(sv, R, st, wts.ycol if weighted else None)
                elif (y_split is not None or gram is not None) and self._yth is not None:
                    self._ut_y(sv, R)
                else:
                    K.gemm(U, Ysrc, ta=True, C=R)
                if wts.rinv is not None:
                    K.scale_rc(R, colscale=wts.rinv, out=R)
                elif wts.dense:  # R = R~ diag(1/sqrt lam) V^T
                    R = K.gemm(R.clone(), wts.Vinv, tb=True, C=R)
            else:
                sq = torch.sqrt(S32)
                K.scale_rc(U, colscale=sq, out=L)  # L = U sqrt(S)
                if rand:
                    R.copy_(sv.SVh)
                elif (y_split is not None or gram is not None) and self._yth is not None:
                    self._ut_y(sv, R)  # S Vh
                else:
                    K.gemm(U, Ysrc, ta=True, C=R)  # S Vh
                rs = torch.where(tiny, torch.zeros_like(sq), 1.0 / sq.clamp_min(1e-30))
                K.scale_rc(R, rowscale=rs, out=R)  # R = sqrt(S) Vh
        else:
            V = vecs  # (B, n, r)
            inv = torch.where(tiny, torch.zeros_like(S32), 1.0 / S32.clamp_min(1e-30))
            # unit error weights (H = I, or not data-aware with h = 1) and unquantised factors:
            # L R = Y V V^T in both branches below, so the error is ||Y||^2 - ||Y V||^2
            # (Pythagoras, V orthonormal) from the Y V product the factors need anyway
            pyth_right = (not quantized and not rand and not wts.dense and wts.ycol is None and wts.err_unit)
            if p.activation_aware_LR:
                self._y_times_v(sv, Ysrc, V, L, st)  # Y V
                if pyth_right:
                    yv2 = K.weighted_sqsum(L, None, r)
                K.scale_rc(L, colscale=inv, out=L)   # U = Y V / S
                K.scale_rc(V, trans=True, rowscale=S32, colscale=wts.rinv, out=R)  # S V^T diag(rinv)
                if wts.dense:
                    R = K.gemm(R.clone(), wts.Vinv, tb=True, C=R)
            else:
                sq = torch.sqrt(S32)
                self._y_times_v(sv, Ysrc, V, L, st)
                if pyth_right:
                    yv2 = K.weighted_sqsum(L, None, r)
                K.scale_rc(L, colscale=torch.where(tiny, torch.zeros_like(sq), 1.0 / sq.clamp_min(1e-30)), out=L)
                K.scale_rc(V, trans=True, rowscale=sq, out=R)
        self._lplr_err2 = None
        if quantized:
            L, R = yield from self._lplr(st, Y, res, L, R, wts, ysq=ysq, halves=lplr_halves)
        st.L, st.R = L, R
        st.has_LR = True
        if self._lplr_err2 is not None and wts.identity and wts.err_unit:
            # H = I: the activation-aware numerator ||res - L R||^2 (alg.py:286-302) of the kept
            # iterate is the LPLR loop's own fused error of that iterate (alg.py:182) -- no
            # separate m x n x r error GEMM.  Small errors (cancellation in ||Y||^2 - 2<L, Y R^T>
            # + <L^T L, R R^T>) are recomputed directly by run_iter, as for the Pythagorean form.
            self._pyth = True
            return self._lplr_err2
        # activation-aware error: sum_j h_j (res - L R)^2  (alg.py:286-302, diagonal H)
        if wts.dense:
            return self._state_error(st, Ws, res, wts)
        if sv.left and p.activation_aware_LR and not quantized and not rand and (wts.ycol is not None or wts.err_unit):
            # L = U (orthonormal columns), L R = U U^T Y diag(1/sqrt(h)) with h the error
            # weights, so the weighted residual is (I - U U^T) Y and, by Pythagoras,
            # sum_j h_j (res - L R)_ij^2 = ||Y||^2 - ||U^T Y||^2 = ||Y||^2 - sum_j h_j R_ij^2
            # (two fp64 reductions instead of an m x n x r product; U orthonormal to ~1e-7)
            ysq = K.weighted_sqsum(Ysrc, None, n) if ysq is None else ysq
            self._pyth = True  # run_iter recomputes small errors directly (cancellation)
            return ysq - K.weighted_sqsum(R, wts.err if wts.ycol is not None else None, n)
        if yv2 is not None:
            # ||res - L R||^2 = ||Y||^2 - ||Y V||^2 (unit weights, Y = res); small errors are
            # recomputed directly by run_iter (cancellation), as for the left-side identity
            ysq = K.weighted_sqsum(Ysrc, None, n) if ysq is None else ysq
            self._pyth = True
            return ysq - yv2
        err = torch.empty(B, dtype=torch.float64, device=dev)
        K.gemm(L, R, D=res, epi=K.EPI_WERR, w=wts.err, err_out=err)
        return err

    def _y_times_v(self, sv, Ysrc, V, L, st=None):
        """L = Y V (m > n; V = the first r columns of the solver's Ritz block, n x r): from Y's
        K-blocked halves (written by cq_residual_split) as the split-fp16 product L^T = V^T Y^T
        (A = the block's transposed split, rows r of p), transposed into L; the fp32 MFMA GEMM
        when the halves are not there.  Sparse-code step (self._r_lite): Y = W - s c, so
        L^T = V^T W^T (W's halves, once per run) - s (c V)^T (cq_codes_matmul, in the epilogue)."""
        if self._r_lite:
            X = sv.X
            B, n, p = X.shape
            r, m = L.shape[2], L.shape[1]
            xh, xl = sv.split_block_t(X)
            cv = scratch.get("lr.utc", (B, r, m), torch.float32, L.device)
            K.codes_matmul(st.Qc, m, n, X, r, cv, trans=True)
            Lt = torch.empty((B, r, m), dtype=torch.float32, device=L.device)
            lc = L.is_contiguous() and _solver.TRANSPOSED_OUT   # L^T's product also writes L (Ct): no transpose pass
            K.gemm_x3(xh, xl, self._wth, self._wtl, 1.0 / (self._ysw * X3_SCALE), Lt, a_blocked=True, b_blocked=True,
                      lda=p, M=r, D=cv, gamma_v=-st.Qs, b_exact=self._wtl is None, Ct=L if lc else None)
            if not lc:
                K.transpose_split(Lt, out=L)
            return
        if self._yrh is None or isinstance(sv, RandSVD) or sv.direct:
            K.gemm(Ysrc, V, C=L)
            return
        X = sv.X
        B, n, p = X.shape
        r = L.shape[2]
        xh, xl = sv.split_block_t(X)
        Lt = torch.empty((B, r, L.shape[1]), dtype=torch.float32, device=L.device)
        lc = L.is_contiguous() and _solver.TRANSPOSED_OUT
        K.gemm_x3(xh, xl, self._yrh, self._yrl, 1.0 / (self._ys * X3_SCALE), Lt, a_blocked=True, b_blocked=True,
                  lda=p, M=r, Ct=L if lc else None)
        if not lc:
            K.transpose_split(Lt, out=L)

    def _ut_w(self, sv, R, st, ycol):
        """R~ = U^T Y = (U^T W) diag(ycol) - s (U^T c) diag(ycol) (m <= n, 2-bit Q = s c): the first
        term a split-fp16 product of the block's transposed halves with W^T's exact halves
        (written once per run by sgram.gram_A; two products, b_exact) with diag(ycol) applied in
        its epilogue (colw), the second from the codes' transpose by the sparse product
        cq_codes_matmul, subtracted in the same epilogue (gamma = -s)."""
        X = sv.X  # (B, m, p), orthonormal columns
        B, m, p = X.shape
        r, n = R.shape[1], R.shape[2]
        dev = X.device
        xh, xl = sv.split_block_t(X)
        ct = scratch.get("lr.codes_t", st.Qc.shape, torch.uint8, dev)
        K.codes_transpose(st.Qc, m, n, out=ct)
        utc = scratch.get("lr.utc", (B, r, n), torch.float32, dev)
        K.codes_matmul(ct, n, m, X, r, utc, roww=ycol, trans=True)
        inv = 1.0 / (self._ysw * X3_SCALE)
        K.gemm_x3(xh, xl, self._wth, self._wtl, inv, R, a_blocked=True, b_blocked=True, lda=p, M=r, D=utc,
                  gamma_v=-st.Qs, b_exact=self._wtl is None, colw=None if ycol is None else ycol.contiguous())

    def _ut_y(self, sv, R):
        """R = U^T Y (U = the solver's Ritz block, first r columns; m <= n) as a split-fp16
        product: A = X^T halves (the block's transposed split, rows r of p), B = Y^T halves
        written by cq_residual_split (K-blocked over m)."""
        X = sv.X  # (B, m, p), orthonormal columns
        B, m, p = X.shape
        r = R.shape[1]
        xh, xl = sv.split_block_t(X)
        inv = 1.0 / (self._ys * X3_SCALE)
        K.gemm_x3(xh, xl, self._yth, self._ytl, inv, R, a_blocked=True, b_blocked=True, lda=p, M=r)

    def _solve_normal(self, M64, rows: int):
        """Whitening of the r x r normal matrix A^T A of an lstsq with A (rows x r):
        Wt Wt^T = M^{-1}; columns of A dependent at gelsy's rcond = eps32 * max(rows, r)
        (torch.linalg.lstsq's default) are dropped, giving the basic solution."""
        rc = float(torch.finfo(torch.float32).eps) * max(rows, M64.shape[-1])
        Wt32, _, info = K.spd_whiten(M64, rcond2=rc * rc)
        return Wt32, info

    def _lplr_rw(self, R, wts: _Weights):
        """R H_sqrt as the L step's lstsq operand (alg.py:163): R V diag(sqrt lam) for dense H,
        R * sqrt(h) for diagonal H, R itself for H = I or non-data-aware (alg.py:167)."""
        if self.p.activation_aware_LR and wts.dense:
            return K.gemm(R, wts.Vs, C=torch.empty_like(R))  # R H_sqrt V
        if self.p.activation_aware_LR and wts.ycol is not None:
            return K.scale_rc(R, colscale=wts.ycol)
        return R

    def lplr_rhs(self, R, Ysrc, wts: _Weights, Bm, halves=None, r_bound=None):
        """The L step's normal-equation pieces for the current R: Bm = Y Rw^T (m x r, into Bm)
        and Mr = Rw Rw^T (r x r, fp64 Gram).  halves (unweighted Y): Y's K-blocked split-fp16
        halves from cq_residual_split; the product then runs on split-fp16 MFMAs (fp32-grade,
        3 fp16 products) instead of the fp32 MFMA GEMM, and leaves the split scale of Bm for
        the next product in self._s_bm (from the product's own |Bm| max, no pass over Bm).
        r_bound (B,) fp32: max|Rw| when known (a quantised R is bounded by its quantiser's scale,
        attained by its largest code), so its split needs no pass over Rw either."""
        Rw = self._lplr_rw(R, wts)
        B_, m, n = Ysrc.shape
        r = R.shape[1]
        ev = LPLR_PROBE.start("Y_Rw^T", 2.0 * B_ * m * n * r, 4.0 * B_ * (m * n + n * r + m * r))
        if ev is not None:
            ev[0].record()
        if halves is not None:
            sR = K.pow2_from_absmax(r_bound.clone()) if r_bound is not None and Rw is R else K.pow2_scale(Rw, 14)
            rh, rl = K.split_f16(Rw, sR, hi=halves["rwh"], lo=halves["rwl"], blocked=True)
            amx = torch.empty(B_, dtype=torch.float32, device=Rw.device)
            K.gemm_x3(halves["yh"], halves["yl"], rh, rl, 1.0 / (halves["ys"] * sR), Bm, a_blocked=True,
                      b_blocked=True, absmax_out=amx)
            self._s_bm = K.pow2_from_absmax(amx)
        else:
            K.gemm(Ysrc, Rw, tb=True, C=Bm)                # m x r
        if ev is not None:
            ev[1].record()
        return Bm, K.gram_f64(Rw, Rw, ta=True, tb=True)     # r x r

    @staticmethod
    def _mm_x3(A, B_nk, C, tB=False, sA=None, sB=None, scale_out=False):
        """C = A B_nk^T (tB: A B_nk, B_nk then given as K x N) on split-fp16 MFMAs (three fp16
        products, fp32 accumulation; per-matrix power-of-two scales): the LPLR loop's
        normal-equation GEMMs (m x r x r, r x r x n), fp32-grade at a fraction of the fp32 MFMA
        time.  A (B, M, K), C (B, M, N) fp32.  sA / sB: the operands' split scales when already
        known (pow2_scale's value, e.g. from the producing product's |C| max); scale_out: also
        return C's split scale for the next product (C, sC)."""
        sA = K.pow2_scale(A, 14) if sA is None else sA
        ah, al = K.split_f16(A, sA)
        sB = K.pow2_scale(B_nk, 14) if sB is None else sB
        if tB:
            Bt, kk, nn = B_nk.shape
            bh = torch.empty((Bt, nn, kk), dtype=torch.float16, device=A.device)
            bl = torch.empty_like(bh)
            K.transpose_split(B_nk, hi=bh, lo=bl, scale=sB)
        else:
            bh, bl = K.split_f16(B_nk, sB)
        if not scale_out:
            return K.gemm_x3(ah, al, bh, bl, 1.0 / (sA * sB), C)
        amx = torch.empty(A.shape[0], dtype=torch.float32, device=A.device)
        K.gemm_x3(ah, al, bh, bl, 1.0 / (sA * sB), C, absmax_out=amx)
        return C, K.pow2_from_absmax(amx)

    def lplr_L_from(self, Bm, Mr, n, L, x3=False):
        """L = Bm Mr^{-1} through the whitening Wr Wr^T = Mr^{-1} (rank-revealing at gelsy's
        rcond for A = (R H_sqrt)^T, n x r).  Mr is overwritten.  x3: the two m x r x r GEMMs on
        split-fp16 MFMAs."""
        Wr, _ = self._solve_normal(Mr, n)
        if x3:
            sW = K.pow2_scale(Wr, 14)  # (r x r: small)
            sBm, self._s_bm = self._s_bm, None
            T1, sT1 = self._mm_x3(Bm, Wr, torch.empty_like(L), tB=True, sA=sBm, sB=sW, scale_out=True)  # (Y Rw^T) Wr
            self._mm_x3(T1, Wr, L, sA=sT1, sB=sW)                                                    # ... Wr^T
            return L
        T1 = K.gemm(Bm, Wr, C=torch.empty_like(L))          # (Y Rw^T) Wr
        K.gemm(T1, Wr, tb=True, C=L)                       # ... Wr^T
        return L

    def lplr_L_step(self, R, Ysrc, wts: _Weights, L, tmp_mr=None):
        """L step of the LPLR loop (alg.py:162-169), before quantisation:
        L = lstsq((R H_sqrt)^T, (res H_sqrt)^T)^T = (Y Rw^T)(Rw Rw^T)^{-1} with Rw = R H_sqrt
        (data-aware; Ysrc = Y = res H_sqrt) or Rw = R, Ysrc = res (alg.py:167).  Normal
        equations: fp64 Gram of Rw, rank-revealing SPD whitening at gelsy's rcond, fp32 GEMMs.
        R (B, r, n), Ysrc (B, m, n), L (B, m, r) output."""
        Bm, Mr = self.lplr_rhs(R, Ysrc, wts, torch.empty_like(L) if tmp_mr is None else tmp_mr)
        return self.lplr_L_from(Bm, Mr, R.shape[-1], L)

    def lplr_R_step(self, L, res, R, tmp_rn=None, Ml=None, halves=None, l_bound=None):
        """R step of the LPLR loop (alg.py:175-177), before quantisation:
        R = lstsq(L, res) = (L^T L)^{-1} L^T res (unweighted, as the reference).
        L (B, m, r) dequantised, res (B, m, n), R (B, r, n) output.  Returns (R, L^T L).
        l_bound (B,) fp32: max|L| when known (the quantiser's scale)."""
        m = L.shape[1]
        if tmp_rn is None:
            tmp_rn = torch.empty_like(R)
        if Ml is None:
            Ml = K.gram_f64(L, L)                          # r x r
        Wl, _ = self._solve_normal(Ml.clone(), m)  # A = L: m x r (the whitening overwrites its input)
        B_, _, n = res.shape
        r = L.shape[2]
        ev = LPLR_PROBE.start("L^T_res", 2.0 * B_ * m * n * r, 4.0 * B_ * (m * n + n * r + m * r))
        if ev is not None:
            ev[0].record()
        sCt = None
        if halves is not None:  # L^T res on split-fp16 MFMAs: A = L^T halves, B = res^T halves
            sL = K.pow2_from_absmax(l_bound.clone()) if l_bound is not None else K.pow2_scale(L, 14)
            K.transpose_split(L, hi=halves["lth"], lo=halves["ltl"], scale=sL, blocked=True)
            amx = torch.empty(B_, dtype=torch.float32, device=L.device)
            K.gemm_x3(halves["lth"], halves["ltl"], halves["yth"], halves["ytl"], 1.0 / (sL * halves["ys"]),
                      tmp_rn, a_blocked=True, b_blocked=True, absmax_out=amx)
            sCt = K.pow2_from_absmax(amx)
            Ct = tmp_rn
        else:
            Ct = K.gemm(L, res, ta=True, C=tmp_rn)         # r x n
        if ev is not None:
            ev[1].record()
        if halves is not None and r % 32 == 0:  # the two r x r x n GEMMs on split-fp16 MFMAs
            Wlt = K.transpose_split(Wl, out=torch.empty_like(Wl))[0]
            sWl = K.pow2_scale(Wl, 14)  # (r x r: small; Wl^T has the same maximum)
            T2, sT2 = self._mm_x3(Wlt, Ct, torch.empty_like(tmp_rn), tB=True, sA=sWl, sB=sCt,
                                  scale_out=True)                                  # Wl^T Ct
            self._mm_x3(Wl, T2, R, tB=True, sA=sWl, sB=sT2)                        # Wl T2
            return R, Ml
        T2 = K.gemm(Wl, Ct, ta=True, C=torch.empty_like(tmp_rn))
        K.gemm(Wl, T2, C=R)
        return R, Ml

    def _lplr(self, st, Y, res, L0, R0, wts: _Weights, ysq=None, halves=None):
        """Quantised-factor LPLR loop, alg.py:144-195 (data-aware lstsq in normal-equation form
        with fp64 Grams; quantise L^T and R as whole matrices, alg.py:171-180).

        Data-aware with diagonal H (the callers' case, main.py:163-196): the iteration error
        ||(res - L R) H_sqrt||^2 = ||Y - L Rw||^2 (alg.py:182) is assembled from pieces the
        loop needs anyway -- ||Y||^2 - 2 <L, Y Rw^T> + <L^T L, Rw Rw^T>, where Y Rw^T and
        Rw Rw^T of the new R are the next L step's normal equations and L^T L is the R step's
        -- instead of a separate m x n x r error GEMM.  Best-iterate bookkeeping (strict <,
        alg.py:184-188) stays on the device (no host sync per LPLR iteration) for uniform
        quantisers."""
        p = self.p
        B, m, n = st.B, st.m, st.n
        r = R0.shape[1]
        dev = res.device
        aware = p.activation_aware_LR
        R = R0
        best_err = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
        cb = p.method_LR != "uniform"
        best_items = [None] * B
        resH = None
        # uniform quantisers keep only the kept iterate's codes and scales (its L, R are their
        # dequantisation, rebuilt once after the loop); codebook methods keep the floats
        best = dict(L=torch.zeros((B, m, r), device=dev) if cb else None,
                    R=torch.zeros((B, r, n), device=dev) if cb else None,
                    Lc=torch.zeros((B, m * r), dtype=K.code_dtype(p.L_bits), device=dev),
                    Rc=torch.zeros((B, r * n), dtype=K.code_dtype(p.R_bits), device=dev),
                    Ls=torch.zeros(B, device=dev), Rs=torch.zeros(B, device=dev))
        Ysrc = Y if aware else res
        fused_err = aware and not wts.dense and self.lplr_fused_err
        L = torch.empty((B, m, r), dtype=torch.float32, device=dev)
        tmp_rn = torch.empty((B, r, n), dtype=torch.float32, device=dev)
        Rn = torch.empty((B, r, n), dtype=torch.float32, device=dev)
        err = torch.empty(B, dtype=torch.float64, device=dev)
        if halves is not None:
            f16 = torch.float16
            halves = dict(halves, rwh=torch.empty((B, r, n), dtype=f16, device=dev),
                          rwl=torch.empty((B, r, n), dtype=f16, device=dev),
                          lth=torch.empty((B, r, m), dtype=f16, device=dev),
                          ltl=torch.empty((B, r, m), dtype=f16, device=dev))
        Bm, Mr = self.lplr_rhs(R, Ysrc, wts, torch.empty((B, m, r), dtype=torch.float32, device=dev), halves)
        if fused_err and ysq is None:
            ysq = K.weighted_sqsum(Ysrc, None, n)
        # fp64 fused error of the kept iterate; L = R = 0 (nothing kept) leaves ||Y||^2
        best_err2 = ysq.clone() if fused_err and not cb else None
        for _ in range(p.lplr_iters):
            # --- L = lstsq((R H_sqrt)^T, (res H_sqrt)^T)^T   (alg.py:162-169)
            self.lplr_L_from(Bm, Mr, n, L, x3=halves is not None and r % 32 == 0)
            # --- quantise L^T as one block (alg.py:171-172)
            if cb:
                Lt = K.transpose_split(L, out=torch.empty((B, r, m), dtype=torch.float32, device=dev))[0]
                itemsL, deqLt = self._quantize_whole(Lt.view(B, r * m), p.method_LR, p.L_bits)
                L = K.transpose_split(deqLt.view(B, r, m), out=torch.empty((B, m, r), dtype=torch.float32,
                                                                            device=dev))[0]
            else:  # uniform: codes kept in L layout (absmax is order-free), reordered when kept
                qL = K.quantize_uniform(L.view(B, m * r), m * r, p.L_bits, codes=True, deq=True)
                L = qL["deq"].view(B, m, r)
            # --- R = lstsq(L, res) = (L^T L)^{-1} L^T res   (alg.py:175-177, unweighted)
            _, Ml = self.lplr_R_step(L, res, Rn, tmp_rn, halves=halves, l_bound=None if cb else qL["scale"].view(B))
            if cb:
                itemsR, deqR = self._quantize_whole(Rn.view(B, r * n), p.method_LR, p.R_bits)
                R = deqR.view(B, r, n)
            else:
                qR = K.quantize_uniform(Rn.view(B, r * n), r * n, p.R_bits, codes=True, deq=True)
                R = qR["deq"].view(B, r, n)
            # --- the next L step's normal equations; error ||(res - L R) H_sqrt||_F  (alg.py:182)
            Bm, Mr = self.lplr_rhs(R, Ysrc, wts, Bm, halves, r_bound=None if cb else qR["scale"].view(B))
            if fused_err:
                err = (ysq - 2.0 * K.batched_dot(L, Bm) + K.batched_dot(Ml, Mr)).clamp_min(0.0)
            elif aware:  # dense H (or the A/B switch lplr_fused_err off): the error GEMM
                K.gemm(L, self._lplr_rw(R, wts), D=Y, epi=K.EPI_WERR, err_out=err)
            else:
                if wts.dense:  # ||(res - L R) H||^2 with H_sqrt = H (alg.py:47-49, :182)
                    if resH is None:
                        resH = K.gemm(res, wts.H_lplr, C=torch.empty_like(res))
                    K.gemm(L, K.gemm(R, wts.H_lplr, C=torch.empty_like(R)), D=resH, epi=K.EPI_WERR, err_out=err)
                else:
                    K.gemm(L, R, D=res, epi=K.EPI_WERR, w=wts.lplr, err_out=err)
            e32 = torch.sqrt(err).float().double()  # torch.linalg.matrix_norm in fp32
            if fused_err and not cb:
                best_err2 = torch.where(e32 < best_err, err, best_err2)
            if self.lplr_trace is not None:
                self.lplr_trace.append(e32.clone())
            better = e32 < best_err                  # strict <, NaN never better (alg.py:184)
            if not cb:
                # device-side selection: no host round trip per LPLR iteration
                bm = better.view(B, 1)
                best["Lc"] = torch.where(bm, qL["codes"].view(B, m * r), best["Lc"])  # L layout
                best["Rc"] = torch.where(bm, qR["codes"].view(B, r * n), best["Rc"])
                best["Ls"] = torch.where(better, qL["scale"].view(B), best["Ls"])
                best["Rs"] = torch.where(better, qR["scale"].view(B), best["Rs"])
                best_err = torch.where(better, e32, best_err)
                continue
            yield
            sel = [b for b, ok in enumerate(better.tolist()) if ok]
            for b in sel:
                best["L"][b].copy_(L[b])
                best["R"][b].copy_(R[b])
                best_items[b] = (itemsL[b], itemsR[b])
                best_err[b] = e32[b]
        if cb:
            st.L_idxs = [it[0][0] if it else None for it in best_items]
            st.L_scale = [it[0][1] if it else None for it in best_items]
            st.R_idxs = [it[1][0] if it else None for it in best_items]
            st.R_scale = [it[1][1] if it else None for it in best_items]
        else:
            # the kept L, R are exactly the dequantised kept codes (qL/qR["deq"] is (c / k) s)
            best["L"] = K.dequantize_uniform(best["Lc"], best["Ls"], p.L_bits).view(B, m, r)
            best["R"] = K.dequantize_uniform(best["Rc"], best["Rs"], p.R_bits).view(B, r, n)
            st.L_idxs = best["Lc"].view(B, m, r).transpose(1, 2).reshape(B, m * r)  # L^T order
            st.R_idxs = best["Rc"]
            st.L_scale, st.R_scale = best["Ls"], best["Rs"]
        self._lplr_err2 = best_err2
        return best["L"], best["R"]

    # ------------------------------------------------------------------ driver
    def run(self, W: torch.Tensor, h: torch.Tensor | None = None, scale_W: bool = True,
            use_tqdm: bool = False):
        """W (B, m, n) fp16/fp32 on a HIP device; h: (n,) diagonal of H, (n, n) dense H, None,
        or a list of B per-matrix diagonals (each (n,) or None: distinct Hessians, main.py:163-165).
        Returns a list of per-matrix result dicts (see api.py for the dataclass view)."""
        return run_to_end(self.run_iter(W, h, scale_W, use_tqdm))

    def run_iter(self, W: torch.Tensor, h: torch.Tensor | None = None, scale_W: bool = True,
                 use_tqdm: bool = False, w_to_host: bool = False):
        """Generator form of run(): yields before each host synchronisation, so several
        engines can be interleaved on their own streams (overlap.run_interleaved).

        w_to_host: the results' "W" is a host copy of the scaled W (alg.py:81 keeps
        best_decomp.W on the CPU), copied by a helper thread on a side stream while the
        decomposition runs (the D2H transfer overlaps the kernels instead of following them)."""
        p = self.p
        if W.dim() == 2:
            W = W.unsqueeze(0)
        B, m, n = W.shape
        dev = W.device
        # every run starts cold: a reused engine's results do not depend on its earlier runs
        # (the solver's warm start, shape and buffers belong to one run)
        self.solver = None
        self._qfb = None
        self._lr_step = 0
        self.lr_steps_from_codes = 0  # LR updates that took the sparse-code path (no residual pass)
        if W.dtype not in (torch.float16, torch.float32):
            W = W.float()
        pad = (-n) % 4
        if pad and (p.method_Q != "uniform" or p.method_LR != "uniform" or (h is not None and h.dim() == 2)):
            raise NotImplementedError("caldera-mi355x: W.shape[1] % 4 != 0 needs uniform quantisers and a "
                                      "diagonal (or no) H")
        if p.compute_quantized_component and "Q" in p.update_order:
            qlog.check_method_bits(p.method_Q, p.Q_bits)  # get_quant_info (alg.py:238-242)
        if p.compute_low_rank_factors and "LR" in p.update_order and (p.L_bits < 16 or p.R_bits < 16):
            qlog.check_method_bits(p.method_LR, p.L_bits)
            qlog.check_method_bits(p.method_LR, p.R_bits)
        per_matrix = isinstance(h, (list, tuple))
        if per_matrix:
            # one diagonal per matrix, stacked (B, n); None = H = I for that matrix
            if len(h) != B:
                raise ValueError(f"{len(h)} per-matrix H for a batch of {B}")
            for x in h:
                if x is not None and (x.dim() != 1 or x.shape[0] != n):
                    raise NotImplementedError("per-matrix H must be diagonals of length n (dense H: one per batch)")
            h = torch.stack([torch.ones(n, dtype=torch.float32, device=dev) if x is None
                             else x.to(device=dev, dtype=torch.float32) for x in h])
        gs, Ws = K.rms_scale(W, scale_W)  # on the true numel (alg.py:38-42)
        Ws_out = Ws
        host_copy = self._start_host_copy(Ws) if w_to_host else None
        self._n_true = n
        if pad:
            # ragged n: zero columns up to a multiple of 4 (the kernels' vector width).  Zeros
            # quantise to code 0 (dequantised 0) and leave every whole-matrix absmax, the
            # residual, Y = res sqrt(h), R = U^T Y diag(1/sqrt h) and all error sums unchanged;
            # h is padded with max(h) so sigma_reg's shift (alg.py:59-64) is the same; the
            # solver keeps its block out of the padded rows when they are its rows (m > n).
            # Outputs are cut back to n columns in _finalize.
            n_true = n
            Ws = torch.nn.functional.pad(Ws, (0, pad))
            n = n + pad
            if h is not None and per_matrix:
                h = torch.cat([h, h.max(dim=1, keepdim=True).values.expand(B, pad)], dim=1)
            elif h is not None:
                h = torch.cat([h, h.max().expand(pad)])
        wts = _Weights(h, n, p, dev, batched=per_matrix)
        self._wmax = K.absmax(Ws)  # bound for the split scale of the LR-step residual
        self._w_finite = None
        self._sg_A = self._sg = self._sg_w = None  # sparse-code Gram (sgram.py): A per run
        self._yh = self._yl = self._ys = None
        self._yth = self._ytl = None
        self._yrh = self._yrl = None
        self._wth = self._wtl = self._ysw = self._wsq = self._wt16 = None
        self._r_lite = False
        if wts.dense:  # den = tr(W H W^T) (alg.py:298)
            self._etmp = torch.empty((B, m, n), dtype=torch.float32, device=dev)
            wf = torch.empty((B, m, n), dtype=torch.float32, device=dev)
            K.build_residual(Ws, None, None, 2, None, res=wf)
            den = wts.dense_err(wf, self._etmp)
            del wf
        else:
            den = K.weighted_sqsum(Ws, wts.err, n)
        r = p.rank
        st = BatchState(B, m, n, r, p, dev)
        best = BatchState(B, m, n, r, p, dev)
        best.flag_Q = [False] * B
        best.flag_LR = [False] * B
        errors = {mtx: [[] for _ in range(B)] for mtx in p.update_order}
        min_err = [math.inf] * B
        updated = {mtx: False for mtx in p.update_order}
        work = torch.empty((B, m, n), dtype=torch.float32, device=dev)  # Y / Q-residual buffer
        need_res = any(x == "LR" for x in p.update_order)
        res = torch.empty((B, m, n), dtype=torch.float32, device=dev) if need_res else None
        to_iter = range(p.iters)
        if use_tqdm:
            from tqdm import tqdm
            to_iter = tqdm(to_iter)
        for _ in to_iter:
            for mtx in p.update_order:
                num = None
                self._pyth = False
                if mtx == "LR" and p.compute_low_rank_factors:
                    num = yield from self._lr_update(st, Ws, work, res, wts, den)
                elif mtx == "Q" and p.compute_quantized_component:
                    num = self._q_update(st, Ws, work, wts, den)
                    if wts.dense:
                        num = self._state_error(st, Ws, work, wts)
                updated[mtx] = True
                if num is None:  # no update: error of the unchanged state
                    num = self._state_error(st, Ws, work, wts)
                e = torch.sqrt((num.float() / den.float()))  # fp32 ratio + sqrt (alg.py:297-301)
                yield
                e = e.tolist()
                if self._pyth and min(e) < PYTH_MIN_ERR:
                    # ||Y||^2 - ||U^T Y||^2 cancels when L R reproduces Y almost exactly (rank at
                    # or above the residual's effective rank): those errors are recomputed from
                    # the residual itself
                    e2 = torch.sqrt(self._state_error(st, Ws, work, wts).float() / den.float())
                    yield
                    e2 = e2.tolist()
                    e = [e2[b] if e[b] < PYTH_MIN_ERR else e[b] for b in range(B)]
                for b in range(B):
                    errors[mtx][b].append(float(e[b]))
                if all(updated.values()):
                    sel = [b for b in range(B) if e[b] < min_err[b]]
                    for b in sel:
                        min_err[b] = e[b]
                    if sel:
                        st.snapshot_into(best, sel)
        if self.solver is not None:
            self.solver.release()  # G, halves, blocks: ~300 MB per 4096^2 matrix
        self._yh = self._yl = None
        self._yth = self._ytl = None
        self._yrh = self._yrl = None
        if host_copy is not None:
            Ws_out = host_copy()  # joins the copy thread: the host tensor
        best.materialize()
        out = self._finalize(best, st, W, Ws_out, gs, errors, wts, spare=(work, res))
        if pad:
            out = [self._cut_columns(d, m, n, n_true) for d in out]
            for lp in self.last_packed:  # packed codes stay in the padded (m, n + pad) grid
                lp["R"] = lp["R"][:, :n_true]
                if "R_codes" in lp:
                    lp["R_codes"] = lp["R_codes"][:, :n_true]
                lp["n_padded"] = n
        return out

    @staticmethod
    def _start_host_copy(Ws: torch.Tensor):
        """Copy Ws (B, m, n) to a pageable host tensor on a side stream from a helper thread
        (a pageable D2H copy blocks its calling thread, not the device); returns a join()
        that yields the host tensor."""
        import threading
        dev = Ws.device
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        side = torch.cuda.Stream(dev)
        host = torch.empty(Ws.shape, dtype=Ws.dtype)
        err = []

        def work():
            try:
                with torch.cuda.device(dev), torch.cuda.stream(side):
                    side.wait_event(ready)
                    host.copy_(Ws)
            except BaseException as e:  # re-raised on join
                err.append(e)

        t = threading.Thread(target=work, daemon=True)
        t.start()

        def join():
            t.join()
            if err:
                raise err[0]
            return host
        return join

    @staticmethod
    def _cut_columns(d, m, n_pad, n):
        """Drop the zero-padding columns of a result dict (ragged n)."""
        d["Q"] = d["Q"][:, :n]
        if torch.is_tensor(d["Q_idxs"]):
            d["Q_idxs"] = d["Q_idxs"].view(m, n_pad)[:, :n].reshape(1, m * n)
        r = d["R"].shape[0]
        d["R"] = d["R"][:, :n]
        if torch.is_tensor(d["R_idxs"]):
            d["R_idxs"] = d["R_idxs"].view(r, n_pad)[:, :n].reshape(1, r * n)
        return d

    def _state_error(self, st, Ws, work, wts):
        B, m, n = st.B, st.m, st.n
        if st.dense_q and st.has_Q:
            K.build_residual(Ws, st.Qd, None, 32, None, res=work)
        else:
            K.build_residual(Ws, st.Qc if st.has_Q else None, st.Qs if st.has_Q else None, self.p.Q_bits,
                             None, res=work)
        if wts.dense:  # E = W - Q - L R, then tr(E H E^T)
            if st.has_LR:
                K.gemm(st.L, st.R, C=work, D=work, epi=K.EPI_RESID,
                       absmax=torch.zeros(B, dtype=torch.int32, device=Ws.device))
            return wts.dense_err(work, self._etmp)
        err = torch.empty(B, dtype=torch.float64, device=Ws.device)
        K.gemm(st.L, st.R, D=work, epi=K.EPI_WERR, w=wts.err, err_out=err)
        return err

    def _finalize(self, best, st, W, Ws, gs, errors, wts, spare=(None, None)):
        """Per-matrix result dicts.  `best` is allocated by this run, so the results are views
        of its batched tensors (no per-matrix copies); uniform Q is unpacked and dequantised
        for the whole batch in one launch each, into this run's B x m x n work buffers (no
        large allocation at the end of a run)."""
        p = self.p
        B, m, n = best.B, best.m, best.n
        dev = W.device
        out = []
        gsl = gs.tolist()
        qs = best.Qs.tolist()
        # compact (storage / gather) form: packed codes as kept by the engine
        self.last_packed = [dict(codes=best.Qc[b], Q_scale=qs[b], L=best.L[b], R=best.R[b], global_scale=gsl[b],
                                 errors={k: v[b] for k, v in errors.items()})
                            for b in range(B)]
        if best.dense_q and p.method_Q in ("nf4", "nf2") and any(best.flag_Q):
            # NF Q with a kept iterate: the level indices packed in the storage layout of the
            # uniform codes (MSB-first, flat over the (m, n) grid) with the matrix's one scale, so
            # the compact form carries Q (torch ops at the end of a run: not on the hot path)
            bits = qlog.code_bits(p.method_Q, p.Q_bits)
            per = 8 // bits
            kept = [b for b in range(B) if best.flag_Q[b]]
            scales = torch.cat([best.q_items[b][1].reshape(1) for b in kept]).tolist()
            for b, sc in zip(kept, scales):
                idx = best.q_items[b][0].reshape(-1, per)
                codes = torch.zeros(idx.shape[0], dtype=torch.uint8, device=idx.device)
                for i in range(per):
                    codes |= idx[:, i] << (bits * (per - 1 - i))
                self.last_packed[b].update(codes=codes, Q_scale=sc, Q_method=p.method_Q)
        if torch.is_tensor(best.L_idxs):
            # uniform L, R with a kept iterate: the factors' integer codes, (m, r) and (r, n), and
            # their scales -- L = (L_codes / k_L) L_scale exactly, so a consumer need not store
            # the factors dense (views of the kept codes: L_idxs is in L^T order)
            r = best.L.shape[2]
            ls, rs = best.L_scale.tolist(), best.R_scale.tolist()
            for b, lp in enumerate(self.last_packed):
                if best.flag_LR[b]:
                    lp.update(L_codes=best.L_idxs[b].view(r, m).t(), R_codes=best.R_idxs[b].view(r, n),
                              L_scale=ls[b], R_scale=rs[b])
        codes_all = Qall = None
        if not best.dense_q and any(best.flag_Q):
            work, res = spare
            if best.q_packed:
                cbuf = None
                if res is not None and res.is_contiguous():
                    cbuf = res.view(-1).view(torch.int8)[: B * m * n].view(B, m * n)
                codes_all = K.unpack_codes(best.Qc, m * n, p.Q_bits, out=cbuf)
            else:
                codes_all = best.Qc
            # dequantize_block (quantization.py:103-105) on the reference int codes -- read from
            # the packed form when there is one (the same code values: 1 byte per 4 or 2 codes
            # instead of 1 per code, and no wait for the unpack)
            qbuf = work.view(-1) if work is not None and work.is_contiguous() else None
            if best.q_packed and p.Q_bits <= 4 and best.Qc.is_contiguous():
                Qall = K.dequantize_uniform(best.Qc, best.Qs, p.Q_bits, packed=True, numel=B * m * n,
                                            out=qbuf).view(B, m, n)
            else:
                Qall = K.dequantize_uniform(codes_all, best.Qs, p.Q_bits, out=qbuf).view(B, m, n)
        for b in range(B):
            d = {}
            if best.flag_Q[b] and best.dense_q:
                d["Q"] = best.Qd[b]
                d["Q_idxs"], d["Q_scale"] = best.q_items[b]
            elif best.flag_Q[b]:
                d["Q"] = Qall[b]
                d["Q_idxs"] = codes_all[b].view(1, m * n)
                d["Q_scale"] = best.Qs[b].view(1, 1)
            else:
                d["Q"] = torch.zeros((m, n), dtype=torch.float32, device=dev)
                d["Q_idxs"] = None
                d["Q_scale"] = 1
            d["L"] = best.L[b]
            d["R"] = best.R[b]
            if isinstance(best.L_idxs, list) and best.flag_LR[b] and best.L_idxs[b] is not None:
                d["L_idxs"], d["R_idxs"] = best.L_idxs[b], best.R_idxs[b]
                d["L_scale"], d["R_scale"] = best.L_scale[b], best.R_scale[b]
            elif torch.is_tensor(best.L_idxs) and best.flag_LR[b]:
                d["L_idxs"] = best.L_idxs[b].view(1, -1)
                d["R_idxs"] = best.R_idxs[b].view(1, -1)
                d["L_scale"] = best.L_scale[b].view(1, 1)
                d["R_scale"] = best.R_scale[b].view(1, 1)
            else:
                d["L_idxs"] = d["R_idxs"] = None
                d["L_scale"] = d["R_scale"] = 1
            d["W"] = Ws[b]
            d["global_scale"] = gsl[b]
            d["errors"] = {k: v[b] for k, v in errors.items()}
            out.append(d)
        return out
