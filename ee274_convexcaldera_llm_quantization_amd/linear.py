"""CalderaLinear: an `nn.Linear` replacement that runs y = x (gs (Q + L R))^T (+ bias) from
the compressed form -- packed 2/4-bit codes, one scale, fp16 rank-r factors, a global scale
-- through cq_linear_forward (csrc/cq_linear.hip), never forming the dense weight.  A 4096^2
layer at 2-bit and r = 128 holds 4 MB of codes and 2 MB of factors where the dense fp16
weight `model.apply_caldera_quantization` writes back by default holds 32 MB.

The codes are kept in the inference layout of include/caldera_hip.h (rows padded to 16
bytes with code 0); the storage layout of `engine.last_packed` / `sharding.MatrixResult` is
converted once at construction with torch ops (not on the hot path).

CALDERA's own configurations quantise L and R too (2/4-bit uniform, one scale each).  Such a
factor is kept as its packed codes in the same inference layout (`L_codes`: out_features rows
of rank codes, `R_codes`: rank rows of in_features codes) with `lscale` / `rscale`, has no
fp16 buffer, and is applied by cq_linear_packed_forward: a quarter (4-bit) or an eighth
(2-bit) of the fp16 factor's bytes, and no second rounding of (c / k) s to fp16.

Every layer back-propagates dx from its packed form (csrc/cq_linear_bwd.hip:
cq_linear_backward_input, with a coded factor cq_linear_packed_backward_input), and
HadamardCalderaLinear around it with cq_hadamard_rows on dy and dx; fp16 factors can be
trained over the frozen codes, coded ones stay frozen.

Q may also be an NF4 / NF2 codebook (`q_format` = Q_FORMAT_NF): `codes` then holds the level
indices in the same layout, `qscale` the matrix scale, and the layer runs through
cq_linear_codebook_forward / cq_linear_codebook_backward_input with
Q = I[idx] (s / D), I the integer levels (include/caldera_hip.h).  Factors stay fp16 or uniform.

`materialize()` gives the dense weight gs (Q + L R) from any of these forms by one kernel
(cq_linear_dequant, csrc/cq_linear_dequant.hip).  With `dense_prefill_tokens` set a layer hands long
prefill (and the input gradient at that length) to the dense fp16 GEMM on a weight materialised
into one scratch buffer that all layers of a stream share; the default, None, changes nothing.

Layers that read the same activation (q / k / v, gate / up) can form a `CalderaLinearGroup`: the set
runs as one z launch and one code + L launch (cq_linear_group_forward), every output with the bits of
the layer run alone, and the model's own calls `q_proj(h)`, `k_proj(h)`, `v_proj(h)` stay as they are
(`model.group_shared_input_layers`).

A gated MLP block `down_proj(act(gate_proj(x)) * up_proj(x))` can become a `CalderaGatedMLP`: its gate / up
pair runs as one z launch and one code + L launch whose epilogue applies the activation and the product
(cq_linear_glu_forward), so neither pre-activation is written and the two elementwise launches are gone
(`model.fuse_gated_mlps`).

A Hadamard-basis layer may carry the +-1 sign vectors of the randomised transform
H1 diag(su) pad(W) diag(sv) H2 (`HadamardCalderaLinear(sign_seeds=)`, `hadamard_sign_vector`): its transforms,
its group's and its fused block's then run through the cq_hadamard_signed_* entries, which flip exactly;
without seeds, the default, nothing about a layer changes.
"""
from __future__ import annotations

import weakref

import torch

from . import _lib as K

SUPPORTED_BITS = (2, 4)
Q_FORMAT_UNIFORM, Q_FORMAT_NF = K.QFMT_UNIFORM, K.QFMT_NF
# Q quantiser methods with packed codes -> (q_format, bits)
Q_METHODS = {"uniform": (Q_FORMAT_UNIFORM, None), "nf4": (Q_FORMAT_NF, 4), "nf2": (Q_FORMAT_NF, 2)}
NF_TAIL_INDEX = {4: 8, 2: 0}  # the index a row's tail holds (NF4: level 0; NF2 has no zero level)


def q_method_format(Q_method: str, Q_bits: int) -> int:
    """The q_format of a Q quantiser method at Q_bits; raises for a method without packed codes
    (bbint*) and for nf4 / nf2 at other bits than 4 / 2."""
    method = str(Q_method).lower()
    if method in ("bbint4", "bbint2"):
        raise ValueError(f"CalderaLinear: Q method {method!r} has no packed form: its codes are affine per block "
                         "(one minimum and one scale per block) plus an outlier list, not one scale per matrix")
    if method not in Q_METHODS:
        raise ValueError(f"CalderaLinear: unknown Q method {Q_method!r} (uniform, nf4, nf2)")
    fmt, bits = Q_METHODS[method]
    if bits is not None and bits != Q_bits:
        raise ValueError(f"CalderaLinear: Q method {method!r} needs Q_bits = {bits}, got {Q_bits}")
    return fmt


def q_method_name(q_format: int, bits: int) -> str:
    return "uniform" if q_format == Q_FORMAT_UNIFORM else f"nf{bits}"


def _k(bits: int) -> int:
    return 2 ** (bits - 1) - 1


def _check_bits(bits):
    if bits not in SUPPORTED_BITS:
        raise ValueError(f"CalderaLinear: Q bits {bits} not in {SUPPORTED_BITS} (no packed codes)")


def _check_factor_bits(bits, what):
    if bits not in SUPPORTED_BITS:
        raise ValueError(f"CalderaLinear: {what} bits {bits} not in {SUPPORTED_BITS} (no packed factor codes)")


def row_bytes(n: int, bits: int) -> int:
    """Bytes per row of the inference layout: ceil(n bits / 8) rounded up to 16."""
    return -(-(n * bits) // 128) * 16


def pack_rows(c: torch.Tensor, bits: int) -> torch.Tensor:
    """(m, n) integer codes in [-k, k] -> (m, row_bytes) uint8 inference layout (offset-binary,
    MSB-first, the row's tail filled with code 0)."""
    k, per = _k(bits), 8 // bits
    m, n = c.shape
    rb = row_bytes(n, bits)
    u = torch.full((m, rb * per), k, dtype=torch.uint8, device=c.device)
    u[:, :n] = (c.to(torch.int16) + k).to(torch.uint8)
    u = u.view(m, rb, per)
    out = torch.zeros((m, rb), dtype=torch.uint8, device=c.device)
    for i in range(per):
        out |= u[:, :, i] << (bits * (per - 1 - i))
    return out


def unpack_bytes(b: torch.Tensor, bits: int) -> torch.Tensor:
    """uint8 (..., nbytes) packed codes -> int8 (..., nbytes * 8 / bits) codes in [-k, k]."""
    k, per = _k(bits), 8 // bits
    parts = [((b >> (bits * (per - 1 - i))) & (2 ** bits - 1)) for i in range(per)]
    u = torch.stack(parts, dim=-1).reshape(*b.shape[:-1], b.shape[-1] * per)
    return (u.to(torch.int16) - k).to(torch.int8)


def pack_index_rows(idx: torch.Tensor, bits: int) -> torch.Tensor:
    """(m, n) NF level indices in [0, 2^bits) -> (m, row_bytes) uint8 inference layout (the index
    itself, MSB-first, the row's tail filled with NF_TAIL_INDEX)."""
    per = 8 // bits
    m, n = idx.shape
    rb = row_bytes(n, bits)
    u = torch.full((m, rb * per), NF_TAIL_INDEX[bits], dtype=torch.uint8, device=idx.device)
    u[:, :n] = idx.to(torch.uint8)
    u = u.view(m, rb, per)
    out = torch.zeros((m, rb), dtype=torch.uint8, device=idx.device)
    for i in range(per):
        out |= u[:, :, i] << (bits * (per - 1 - i))
    return out


def unpack_index_bytes(b: torch.Tensor, bits: int) -> torch.Tensor:
    """uint8 (..., nbytes) packed level indices -> uint8 (..., nbytes * 8 / bits) indices."""
    per = 8 // bits
    parts = [((b >> (bits * (per - 1 - i))) & (2 ** bits - 1)) for i in range(per)]
    return torch.stack(parts, dim=-1).reshape(*b.shape[:-1], b.shape[-1] * per)


def check_dense_prefill_tokens(tokens):
    """`tokens` as a `dense_prefill_tokens` value: None, or an int above the decode branch's token
    count (the dense path replaces the prefill kernels only)."""
    if tokens is None:
        return None
    if isinstance(tokens, bool) or not isinstance(tokens, int) or tokens <= K.LINEAR_DECODE_MAX_TOKENS:
        raise ValueError(f"CalderaLinear: dense_prefill_tokens must be None or an int > "
                         f"{K.LINEAR_DECODE_MAX_TOKENS} (the decode kernels' token count), got {tokens!r}")
    return tokens


def _operands(lin, L16=None, R16=None):
    """The factor operands the layer hands to every entry, (L, R, r, L_codes, R_codes): L / R the fp16 factor --
    L16 / R16 when given (masters rounded to fp16, or the factors a backward saved), else the layer's buffer --
    or None for a coded factor and at rank 0; L_codes / R_codes a coded factor as its (codes, scale, bits) and
    None otherwise.  A coded factor's fp16 buffer is None and a rank-0 layer's is an (m, 0) / (0, n) tensor,
    which no entry is given."""
    r = lin.rank
    if not r:
        return None, None, 0, None, None
    L_codes = None if lin.L_codes is None else (lin.L_codes, lin.lscale, lin.L_bits)
    R_codes = None if lin.R_codes is None else (lin.R_codes, lin.rscale, lin.R_bits)
    return (None if L_codes is not None else lin.L if L16 is None else L16,
            None if R_codes is not None else lin.R if R16 is None else R16, r, L_codes, R_codes)


def _entry_family(lin, r, L_codes, R_codes):
    """Which entries run the layer, forward and backward alike: (prefix, keywords) with `_lib`'s
    <prefix>forward / <prefix>backward_input and the keywords that family takes.  A codebook Q takes
    linear_codebook_*, a uniform Q with a coded factor linear_packed_*, fp16 factors (or none) linear_*."""
    m, n, bits = lin.out_features, lin.in_features, lin.bits
    if lin.q_format != Q_FORMAT_UNIFORM:
        return "linear_codebook_", dict(m=m, n=n, bits=bits, q_format=lin.q_format, r=r, L_codes=L_codes, R_codes=R_codes)
    if L_codes is not None or R_codes is not None:
        return "linear_packed_", dict(m=m, n=n, bits=bits, r=r, L_codes=L_codes, R_codes=R_codes)
    return "linear_", dict(m=m, n=n, bits=bits)


def _dequant(lin, w: torch.Tensor, L16=None, R16=None):
    """cq_linear_dequant of the layer into w (out_features, in_features) fp16 / bf16 / fp32.
    L16 / R16: the fp16 factors to use instead of the layer's buffers (masters rounded to fp16)."""
    L, R, r, L_codes, R_codes = _operands(lin, L16, R16)
    return K.linear_dequant(lin.codes, lin.qscale, lin.gscale, L, R, w, m=lin.out_features, n=lin.in_features,
                            bits=lin.bits, q_format=lin.q_format, r=r, L_codes=L_codes, R_codes=R_codes)


def _dense_scratch(lin, L16, R16):
    """The layer's fp16 weight, freshly materialised into the stream's shared scratch buffer (one
    per stream, as large as the largest layer that used it; the next dense-path call on the stream
    overwrites it, which stream order makes safe)."""
    from . import scratch
    m, n = lin.out_features, lin.in_features
    W16 = scratch.get_flat("linear.dense_weight", m * n, torch.float16, lin.codes.device).view(m, n)
    return _dequant(lin, W16, L16, R16)


def _mm_into(a16, b16, out):
    """out = a16 @ b16 with fp16 operands and the GEMM's fp32 accumulation: rounded once, to out's
    dtype (fp16: the GEMM's own output rounding; fp32: none)."""
    if out.dtype == torch.float16:
        return torch.mm(a16, b16, out=out)
    return out.copy_(torch.mm(a16, b16, out_dtype=torch.float32))


def _use_dense(lin, T: int) -> bool:
    return lin.dense_prefill_tokens is not None and T >= lin.dense_prefill_tokens


def _launch_packed(lin, x2: torch.Tensor, y: torch.Tensor, L16=None, R16=None):
    """The entry `CalderaLinear.forward` takes for this layer, on given fp16 x2 (T, in_features)
    and y (T, out_features): cq_linear_packed_forward with a coded factor, else cq_linear_forward.
    L16 / R16: the fp16 factors to use instead of the layer's buffers (masters rounded to fp16).

    Dense path (`lin.dense_prefill_tokens` set and T >= it): W16 = f16(gs (Q + L R)) from
    cq_linear_dequant (the fp32 weight of its contract, rounded once to fp16) into the shared
    scratch buffer, then the dense GEMM x2 W16^T with fp32 accumulation.  Without a bias an fp16 y is
    that fp32 sum rounded once; otherwise the sum stays fp32, the bias is added in fp32 and the
    result is rounded once when y is fp16.  So against the packed kernels the dense path adds one
    fp16 rounding of each weight and nothing else."""
    if _use_dense(lin, x2.shape[0]):
        W16 = _dense_scratch(lin, L16, R16)
        if lin.bias is None:
            return _mm_into(x2, W16.t(), y)
        y32 = torch.mm(x2, W16.t(), out_dtype=torch.float32)
        y32 += lin.bias
        return y.copy_(y32)
    L, R, *factors = _operands(lin, L16, R16)
    prefix, kw = _entry_family(lin, *factors)
    getattr(K, prefix + "forward")(x2, lin.codes, lin.qscale, lin.gscale, L, R, lin.bias, y, **kw)
    return y


def _fp16_factors(L, R):
    """The kernels' fp16 operands of the fp16 factors L, R (buffers or masters; None: coded or rank 0)."""
    return (None if L is None else L.detach().to(torch.float16), None if R is None else R.detach().to(torch.float16))


def _packed_backward(lin, dy16, x2, L16, R16, needs, dx_dtype, factor_dtypes):
    """(dx2, dL, dR) of one packed layer for dy16 (T, m) fp16 and the saved fp16 x2 (T, n): dx2 (T, n)
    in dx_dtype (fp32 | fp16) from the packed codes -- cq_linear_packed_backward_input with a coded
    factor, else cq_linear_backward_input -- and, for trainable (hence fp16) factors,
    dL = gs dy^T (x R^T) and dR = gs (dy L)^T x.  With `lin.dense_prefill_tokens` set and T >= it,
    dx2 = dy16 W16 by the dense GEMM on a fresh materialisation (`_launch_packed`'s rounding
    sequence: each weight to fp16 once, fp32 accumulation, one rounding to dx_dtype)."""
    n, r, gs = lin.in_features, lin.rank, lin.gscale
    need_x, need_L, need_R = needs
    T = dy16.shape[0]
    dx2 = dL = dR = u = None
    if need_x:
        dx2 = torch.empty((T, n), dtype=dx_dtype, device=dy16.device)
        if _use_dense(lin, T):
            # the dense path of `_launch_packed`, mirrored: dx = dy16 W16 from a fresh materialisation
            # (the scratch buffer does not outlive the forward); u is left to the torch product below
            _mm_into(dy16, _dense_scratch(lin, L16, R16), dx2)
        else:
            L, R, *factors = _operands(lin, L16, R16)
            prefix, kw = _entry_family(lin, *factors)
            # u = dy L for dR, from the kernel that forms it anyway (not linear_packed_*: a layer with a coded
            # factor trains none)
            if need_R and R is not None and prefix != "linear_packed_":
                u = torch.empty((T, r), dtype=torch.float32, device=dy16.device)
            getattr(K, prefix + "backward_input")(dy16, lin.codes, lin.qscale, gs, L, R, dx2, u_out=u, **kw)
    # the factor gradients are T-reductions of T m r and T r n flops (r / n of the code term):
    # torch matmul in fp32, z and u kept in fp32
    if need_L:
        z = x2.float() @ R16.float().t()
        dL = ((dy16.float().t() @ z) * gs).to(factor_dtypes[0])
    if need_R:
        if u is None:
            u = dy16.float() @ L16.float()
        dR = ((u.t() @ x2.float()) * gs).to(factor_dtypes[1])
    return dx2, dL, dR


def _rows(t, cols):
    """t as a (T, cols) matrix with unit column stride whose rows do not overlap."""
    t2 = t.reshape(-1, cols)
    if t2.stride(1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < cols):
        t2 = t2.contiguous()
    return t2


def _check_last_dim(x, n):
    if x.shape[-1] != n:
        raise ValueError(f"CalderaLinear: last dimension {x.shape[-1]} != in_features {n}")


def _fp16_rows(x, n):
    """x as the fp16 (T, n) matrix with unit column stride the packed kernels read.  (The Hadamard transforms
    read x in its own dtype and from rows that do not overlap: `_rows`, `_hadamard_input`.)"""
    x2 = x.reshape(-1, n).to(torch.float16)
    return x2 if x2.stride(1) == 1 else x2.contiguous()


def _out_dtype(dtype):
    """The dtype the packed kernels write for an activation of `dtype`: fp16 and fp32 as they are, anything
    else is computed in fp32 and cast."""
    return dtype if dtype in (torch.float16, torch.float32) else torch.float32


def _like_input(y2, x, m):
    """The (T, m) result y2 in x's dtype and with x's leading dimensions."""
    return y2.to(x.dtype).reshape(*x.shape[:-1], m)


class _PackedLinearFunction(torch.autograd.Function):
    """y = x (gs (Q + L R))^T (+ bias) with a graph: the forward is `CalderaLinear.forward`'s launch
    (cq_linear_forward, or cq_linear_packed_forward with a coded factor: the same bits), the
    backward gives dx from the packed codes (cq_linear_backward_input resp.
    cq_linear_packed_backward_input) and, for trainable factors, dL = gs dy^T (x R^T) and
    dR = gs (dy L)^T x.  The codes, the bias and a coded factor are frozen.  L, R: the layer's fp16
    buffers or its master parameters, rounded to fp16 for the kernels (their gradient passes
    straight through that rounding); None for a coded factor."""

    @staticmethod
    def forward(ctx, x, L, R, lin):
        x2 = _fp16_rows(x, lin.in_features)
        L16, R16 = _fp16_factors(L, R)
        y = torch.empty((x2.shape[0], lin.out_features), dtype=_out_dtype(x.dtype), device=x.device)
        _launch_packed(lin, x2, y, L16, R16)
        ctx.lin, ctx.x_shape, ctx.x_dtype = lin, x.shape, x.dtype
        ctx.factor_dtypes = (None if L is None else L.dtype, None if R is None else R.dtype)
        ctx.save_for_backward(x2, L16, R16)
        return _like_input(y, x, lin.out_features)

    @staticmethod
    def backward(ctx, gy):
        lin = ctx.lin
        x2, L16, R16 = ctx.saved_tensors
        dy16 = _rows(gy, lin.out_features).to(torch.float16)  # once: every gradient uses these values
        dx2, dL, dR = _packed_backward(lin, dy16, x2, L16, R16, ctx.needs_input_grad[:3], _out_dtype(ctx.x_dtype),
                                       ctx.factor_dtypes)
        dx = None if dx2 is None else dx2.to(ctx.x_dtype).reshape(ctx.x_shape)
        return dx, dL, dR, None


class _HadamardLinearFunction(torch.autograd.Function):
    """`HadamardCalderaLinear.forward` with a graph: the inference path's three launch groups (the same
    bits), and a backward that mirrors them.  H is symmetric, so dy goes through cq_hadamard_rows
    with n_in and n_out swapped (out_features -> pr, written as the fp16 dy^ the inner backward
    takes), the inner layer's backward gives the fp32 dx^ from the packed codes, and dx^ goes through
    cq_hadamard_rows (pc -> in_features) into x's dtype; no torch arithmetic on that path.  The
    inner factors' gradients come from the saved x^ and dy^: in the Hadamard basis, the one the
    factors live in.  The bias is frozen.  A signed layer takes cq_hadamard_signed_rows for both: dy
    goes in with sign_in = su, dx comes out with sign_out = sv, and x^ and dy^ are those of the signed basis.

    One function and not three chained ones: autograd casts the gradient of an input to that
    input's dtype, so across an edge the fp32 dx^ of the fp16 x^ would be rounded to fp16 (and the
    fp16 dy^ of the fp32 inner output widened and narrowed again)."""

    @staticmethod
    def forward(ctx, x, L, R, had):
        L16, R16 = _fp16_factors(L, R)
        x2, xh, y = had._forward_launches(x, L16, R16)
        ctx.had, ctx.x_shape, ctx.x_dtype, ctx.x2_dtype = had, x.shape, x.dtype, x2.dtype
        ctx.factor_dtypes = (None if L is None else L.dtype, None if R is None else R.dtype)
        ctx.save_for_backward(xh, L16, R16)
        return _like_input(y, x, had.out_features)

    @staticmethod
    def backward(ctx, gy):
        had = ctx.had
        xh, L16, R16 = ctx.saved_tensors
        pr, pc = had.padded_shape
        gy2 = _rows(gy, had.out_features)
        if gy2.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            gy2 = gy2.float()
        T = gy2.shape[0]
        dyh = torch.empty((T, pr), dtype=torch.float16, device=gy.device)
        _transform(had, gy2, dyh, n_in=had.out_features, n_out=pr, P=pr, sign_in="sign_out")
        dxh, dL, dR = _packed_backward(had.inner, dyh, xh, L16, R16, ctx.needs_input_grad[:3], torch.float32,
                                       ctx.factor_dtypes)
        dx = None
        if dxh is not None:
            dx2 = torch.empty((T, had.in_features), dtype=ctx.x2_dtype, device=gy.device)
            _transform(had, dxh, dx2, n_in=pc, n_out=had.in_features, P=pc, sign_out="sign_in")
            dx = dx2.to(ctx.x_dtype).reshape(ctx.x_shape)
        return dx, dL, dR, None


class _GroupMember:
    """What `CalderaLinear` and `HadamardCalderaLinear` share beside `torch.nn.Module`: the back-reference to a
    group, the `forward` that defers to it, the head of `_forward_alone` and `_apply`.  A subclass provides
    `_packed` (the `CalderaLinear` whose operands the kernels read: the layer itself, or `inner`),
    `_with_graph(x, L, R)` (its autograd function) and `_without_graph(x, L16, R16)` (its inference launches)."""

    @property
    def group(self):
        """The `CalderaLinearGroup` (for a `HadamardCalderaLinear`: the `HadamardLinearGroup`) this layer is a
        member of, or None.  A plain attribute kept in `__dict__`: no buffer, no state, not a submodule."""
        return self.__dict__.get("_group")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        group = self.__dict__.get("_group")
        if group is not None:  # a member of a group: the set's launches for the whole group
            return group._member_forward(self, x)
        return self._forward_alone(x)

    def _forward_alone(self, x: torch.Tensor) -> torch.Tensor:
        """The layer's own launches, whether it is in a group or not."""
        packed = self._packed
        if not x.is_cuda or not packed.codes.is_cuda:
            raise RuntimeError("CalderaLinear needs HIP device tensors (no CPU fallback)")
        _check_last_dim(x, self.in_features)
        trainable = packed.factors_trainable
        if torch.is_grad_enabled() and (x.requires_grad
                                        or (trainable and (packed.L.requires_grad or packed.R.requires_grad))):
            # a coded factor has no fp16 operand (None); rank 0 has none at all
            return self._with_graph(x, packed.L if packed.rank else None, packed.R if packed.rank else None)
        # no graph: the inference launches (on the masters rounded to fp16 while the factors train)
        L16, R16 = _fp16_factors(packed.L, packed.R) if trainable else (None, None)
        return self._without_graph(x, L16, R16)

    def _apply(self, fn, *args, **kwargs):
        """Moves follow the model (`.to(device)`, `.cuda()`); dtype casts do not: `model.half()` or
        `.to(torch.bfloat16)` leave the codes, the fp16 factors, the int8 sign vectors and the fp32 bias as stored
        (the kernels' operand types; a cast would only lose bits), forward returns x's dtype anyway."""
        def keep_dtype(t):
            out = fn(t)
            return out if out.dtype == t.dtype else t.to(out.device)
        return super()._apply(keep_dtype, *args, **kwargs)


class CalderaLinear(_GroupMember, torch.nn.Module):
    """One compressed layer.  Buffers (so `state_dict()` carries them): `codes` (out_features,
    row_bytes) uint8 inference layout, `L` (out_features, rank) and `R` (rank, in_features) fp16,
    `bias` (out_features,) fp32 or None.  A factor given by its codes has `L_codes`
    (out_features, row_bytes(rank, L_bits)) resp. `R_codes` (rank, row_bytes(in_features, R_bits))
    uint8 instead, with `lscale` / `rscale`, and its fp16 buffer is None.  Plain attributes:
    qscale, gscale, bits, in_features, out_features, rank, lscale, rscale, L_bits, R_bits (16 =
    fp16 factor), q_format (Q_FORMAT_UNIFORM: `codes` are offset-binary uniform codes;
    Q_FORMAT_NF: NF4 / NF2 level indices, qscale the matrix scale; no buffer of its own), also
    carried as the state dict's extra state.

    forward(x): any leading dimensions, last = in_features, on a HIP device (there is no CPU
    path).  x is cast to fp16 and the result returned in x's dtype: bf16 activations beyond
    fp16's range (|x| > 65504) would overflow, as would |x R^T|.

    Training: with grad mode on and x requiring grad (or the factors trainable, see
    `enable_factor_training`) the layer returns a result with a graph, whatever the factor
    format; the backward gives dx = dy (gs (Q + L R)) from the packed codes
    (cq_linear_backward_input; cq_linear_packed_backward_input with a coded factor) and the
    gradients of trainable factors.  The incoming gradient is cast to fp16 once, so |dy| <= 65504
    (and |dy L|), and gradients below fp16's subnormals (6e-8) vanish: use the usual loss scaling.
    The codes and the bias stay frozen, and so does a coded factor (a buffer without a gradient)
    and the fp16 factor beside it: only a layer with two fp16 factors trains them."""

    def __init__(self, codes, L, R, bias=None, *, qscale, gscale, bits, in_features, out_features, L_codes=None,
                 R_codes=None, q_format=Q_FORMAT_UNIFORM):
        """L_codes / R_codes: (uint8 inference-layout codes, scale, bits) of a coded factor,
        whose fp16 L / R is then None."""
        super().__init__()
        _check_bits(bits)
        if q_format not in (Q_FORMAT_UNIFORM, Q_FORMAT_NF):
            raise ValueError(f"CalderaLinear: unknown q_format {q_format!r}")
        if q_format == Q_FORMAT_NF and not (float(qscale) >= 0.0 and float(qscale) != float("inf")):
            raise ValueError(f"CalderaLinear: NF scale {float(qscale)} is not finite and >= 0")
        self.q_format = int(q_format)
        m, n = int(out_features), int(in_features)
        if codes.dtype != torch.uint8 or tuple(codes.shape) != (m, row_bytes(n, bits)):
            raise ValueError(f"CalderaLinear: codes must be uint8 {(m, row_bytes(n, bits))} (inference layout), "
                             f"got {codes.dtype} {tuple(codes.shape)}")
        if (L_codes is not None and L is not None) or (R_codes is not None and R is not None):
            raise ValueError("CalderaLinear: a factor is given by its codes or as fp16, not both")
        if (L is None and L_codes is None) != (R is None and R_codes is None):
            raise ValueError("CalderaLinear: one factor without the other")
        r = int(R_codes[0].shape[0]) if R_codes is not None else 0 if R is None else int(R.shape[0])
        if r > K.LINEAR_MAX_RANK:
            raise ValueError(f"CalderaLinear: rank {r} > {K.LINEAR_MAX_RANK}")
        dev = codes.device
        if r == 0:
            L, R, L_codes, R_codes = torch.zeros((m, 0), device=dev), torch.zeros((0, n), device=dev), None, None
        self.in_features, self.out_features, self.rank, self.bits = n, m, r, int(bits)
        self.qscale, self.gscale = float(qscale), float(gscale)
        self.lscale = self.rscale = 1.0
        self.L_bits = self.R_bits = 16
        packed = {}
        for what, spec, fp, shape in (("L", L_codes, L, (m, r)), ("R", R_codes, R, (r, n))):
            if spec is None:
                if tuple(fp.shape) != shape:
                    raise ValueError(f"CalderaLinear: {what} {tuple(fp.shape)} does not fit {shape} (L {(m, r)} / "
                                     f"R {(r, n)})")
                packed[what] = None
                continue
            t, scale, fbits = spec
            _check_factor_bits(fbits, what)
            want = (shape[0], row_bytes(shape[1], fbits))
            if t.dtype != torch.uint8 or tuple(t.shape) != want:
                raise ValueError(f"CalderaLinear: {what}_codes must be uint8 {want} (inference layout), got "
                                 f"{t.dtype} {tuple(t.shape)}")
            scale = float(scale)
            if not (scale >= 0.0 and scale != float("inf")):
                raise ValueError(f"CalderaLinear: {what} scale {scale} is not finite and >= 0")
            setattr(self, what.lower() + "scale", scale)
            setattr(self, what + "_bits", int(fbits))
            packed[what] = t.detach().contiguous()
        self.register_buffer("codes", codes.contiguous())
        self.register_buffer("L", None if packed["L"] is not None else L.detach().to(torch.float16).contiguous())
        self.register_buffer("R", None if packed["R"] is not None else R.detach().to(torch.float16).contiguous())
        self.register_buffer("L_codes", packed["L"])
        self.register_buffer("R_codes", packed["R"])
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).contiguous())

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_codes(cls, c, L, R, bias=None, *, qscale, gscale, bits, L_codes=None, R_codes=None,
                   q_format=Q_FORMAT_UNIFORM):
        """From (m, n) integer codes in [-k, k]; with q_format = Q_FORMAT_NF from an (m, n) integer
        matrix of NF level indices in [0, 2^bits).  L_codes = (cL, sL, bits) / R_codes = (cR, sR,
        bits): a factor as (m, r) resp. (r, n) integer codes in [-k, k] with its scale, i.e.
        L = (cL / k) sL; its fp16 L / R is then None."""
        _check_bits(bits)
        m, n = c.shape
        if q_format == Q_FORMAT_NF:
            if c.dtype.is_floating_point or (c.numel() and (int(c.min()) < 0 or int(c.max()) >= 2 ** bits)):
                raise ValueError(f"CalderaLinear.from_codes: NF indices must be an integer matrix in [0, {2 ** bits})")
            qcodes = pack_index_rows(c, bits)
        else:
            qcodes = pack_rows(c, bits)

        def packed(spec, what):
            if spec is None:
                return None
            cf, scale, fbits = spec
            _check_factor_bits(fbits, what)
            if cf.dim() != 2 or cf.dtype.is_floating_point or int(cf.abs().max() if cf.numel() else 0) > _k(fbits):
                raise ValueError(f"CalderaLinear.from_codes: {what} codes must be an integer matrix in "
                                 f"[-{_k(fbits)}, {_k(fbits)}]")
            return pack_rows(cf, fbits), scale, fbits

        return cls(qcodes, L, R, bias, qscale=qscale, gscale=gscale, bits=bits, in_features=n,
                   out_features=m, L_codes=packed(L_codes, "L"), R_codes=packed(R_codes, "R"), q_format=q_format)

    @classmethod
    def from_result(cls, res, bias=None):
        """From a `sharding.MatrixResult` (what `engine.last_packed`, `pack_results` and
        `load_results` hold): storage-layout codes on the (m, extra["n_padded"] or n) grid."""
        _check_bits(res.Q_bits)
        m, n = res.m, res.n
        npad = int(res.extra.get("n_padded", n)) if res.extra else n
        nbytes = m * npad * res.Q_bits // 8
        flat = res.codes.reshape(-1)
        if flat.dtype != torch.uint8 or flat.numel() != nbytes or (m * npad * res.Q_bits) % 8:
            raise ValueError(f"CalderaLinear.from_result: {res.name}: codes are not {nbytes} packed bytes")
        # an NF result stores the level index as it is, in the same storage layout
        q_format = q_method_format(getattr(res, "Q_method", "uniform"), res.Q_bits)
        if q_format == Q_FORMAT_NF:
            qcodes = pack_index_rows(unpack_index_bytes(flat, res.Q_bits).view(m, npad)[:, :n], res.Q_bits)
        else:
            qcodes = pack_rows(unpack_bytes(flat, res.Q_bits).view(m, npad)[:, :n], res.Q_bits)
        # a coded factor travels in the inference layout already (its fp32 array has zero rows)
        Lc = getattr(res, "L_codes", None)
        Rc = getattr(res, "R_codes", None)
        return cls(qcodes, None if Lc is not None else res.L,
                   None if Rc is not None else res.R[:, :n], bias, qscale=res.Q_scale, gscale=res.global_scale,
                   bits=res.Q_bits, in_features=n, out_features=m,
                   L_codes=None if Lc is None else (Lc, res.L_scale, res.L_bits),
                   R_codes=None if Rc is None else (Rc, res.R_scale, res.R_bits), q_format=q_format)

    @classmethod
    def from_decomposition(cls, dec, Q_bits, bias=None, *, L_bits=None, R_bits=None, Q_method="uniform"):
        """From a CalderaDecomposition with uniform Q: packs `Q_idxs` (the reference's int codes,
        (1, m n)) with `Q_scale`; L, R are rounded to fp16.  L_bits / R_bits (2 | 4; None: fp16):
        that factor was quantised uniformly at those bits and is kept as its codes instead --
        `L_idxs` ((1, r m), in L^T order) with `L_scale`, `R_idxs` ((1, r n)) with `R_scale`,
        each one scale.  Q_method "nf4" / "nf2" (the decomposition does not say how Q was
        quantised, so it must be passed): `Q_idxs` is the uint8 level indices, `Q_scale` the one
        scale of the matrix; Q_method must agree with Q_bits.  bbint methods have no packed form."""
        _check_bits(Q_bits)
        q_format = q_method_format(Q_method, Q_bits)
        for what, fbits in (("L", L_bits), ("R", R_bits)):
            if fbits is not None:
                _check_factor_bits(fbits, what)
        if dec.Q_idxs is None or dec.Q is None:
            raise ValueError("CalderaLinear.from_decomposition: the decomposition has no Q")
        qs = dec.Q_scale
        one_scale = not ((torch.is_tensor(qs) and qs.numel() != 1) or isinstance(qs, (tuple, list, dict)))
        if q_format == Q_FORMAT_NF:
            if not torch.is_tensor(dec.Q_idxs) or dec.Q_idxs.dtype != torch.uint8 or not one_scale:
                raise ValueError(f"CalderaLinear.from_decomposition: Q_method {Q_method!r} needs uint8 level indices "
                                 "and one scale (the NF quantiser with one block per matrix)")
        elif not torch.is_tensor(dec.Q_idxs) or dec.Q_idxs.dtype != torch.int8 or not one_scale:
            raise ValueError("CalderaLinear.from_decomposition: Q is not uniformly quantised with one scale "
                             "(nf / bbint codebooks have no packed codes unless Q_method names nf4 / nf2)")
        m, n = dec.Q.shape
        if dec.Q_idxs.numel() != m * n:
            raise ValueError("CalderaLinear.from_decomposition: Q_idxs does not hold m x n codes")
        qscale = float(qs.reshape(-1)[0]) if torch.is_tensor(qs) else float(qs)
        r = dec.R.shape[0]

        def factor(what, fbits, rows, cols, transposed):
            if fbits is None:
                return None
            idxs, scale = getattr(dec, what + "_idxs", None), getattr(dec, what + "_scale", None)
            if (not torch.is_tensor(idxs) or idxs.dtype != torch.int8 or isinstance(scale, (tuple, list, dict))
                    or (torch.is_tensor(scale) and scale.numel() != 1)):
                raise ValueError(f"CalderaLinear.from_decomposition: {what} is not uniformly quantised with one "
                                 "scale (nf / bbint codebooks have no packed codes)")
            if idxs.numel() != rows * cols:
                raise ValueError(f"CalderaLinear.from_decomposition: {what}_idxs does not hold {rows} x {cols} codes")
            cf = idxs.reshape(cols, rows).t() if transposed else idxs.reshape(rows, cols)
            return cf, (float(scale.reshape(-1)[0]) if torch.is_tensor(scale) else float(scale)), fbits

        Lc = factor("L", L_bits, m, r, True)
        Rc = factor("R", R_bits, r, n, False)
        return cls.from_codes(dec.Q_idxs.reshape(m, n), None if Lc else dec.L, None if Rc else dec.R, bias,
                              qscale=qscale, gscale=float(dec.global_scale), bits=Q_bits, L_codes=Lc, R_codes=Rc,
                              q_format=q_format)

    def to_result(self, name: str):
        """The layer as a `sharding.MatrixResult` (storage layout: codes on the (m, n padded to
        4) grid, fp32 factors; a coded factor as its codes, its fp32 array with zero rows), e.g.
        for `sharding.save_results`; `from_result` inverts it."""
        from .sharding import MatrixResult
        m, n, per = self.out_features, self.in_features, 8 // self.bits
        npad = n + (-n) % 4
        codes = self.codes[:, :npad // per].contiguous().reshape(-1)
        extra = {"n_padded": npad} if npad != n else {}
        dev = self.codes.device
        # a coded factor: its codes as they are (inference layout) and an fp32 array of zero rows
        L = self.L.detach().float() if self.L_codes is None else torch.zeros((0, self.rank), device=dev)
        R = self.R.detach().float() if self.R_codes is None else torch.zeros((0, n), device=dev)
        return MatrixResult(name, m, n, self.rank, self.bits, codes, self.qscale, L, R, self.gscale, {}, extra,
                            L_codes=self.L_codes, R_codes=self.R_codes, L_scale=self.lscale, R_scale=self.rscale,
                            L_bits=self.L_bits, R_bits=self.R_bits, Q_method=q_method_name(self.q_format, self.bits))

    # ------------------------------------------------------------------ state
    def get_extra_state(self):
        return {"qscale": self.qscale, "gscale": self.gscale, "bits": self.bits, "in_features": self.in_features,
                "out_features": self.out_features, "rank": self.rank, "lscale": self.lscale, "rscale": self.rscale,
                "L_bits": self.L_bits, "R_bits": self.R_bits, "q_format": self.q_format}

    def set_extra_state(self, state):
        """A state saved before factor codes existed has no lscale / rscale / L_bits / R_bits, one
        saved before codebook Q no q_format: the layer keeps its own (the defaults)."""
        for key, v in state.items():
            setattr(self, key, v)

    def extra_repr(self):
        fac = "" if self.L_bits == self.R_bits == 16 else f", L_bits={self.L_bits}, R_bits={self.R_bits}"
        fmt = "" if self.q_format == Q_FORMAT_UNIFORM else f", q_format={q_method_name(self.q_format, self.bits)}"
        return (f"in_features={self.in_features}, out_features={self.out_features}, bits={self.bits}{fmt}, "
                f"rank={self.rank}{fac}, bias={self.bias is not None}")

    def packed_bytes(self) -> int:
        """Bytes a forward streams for the weights: codes + L + R (fp16 or codes) (+ bias)."""
        return sum(t.numel() * t.element_size()
                   for t in (self.codes, self.L, self.R, self.L_codes, self.R_codes, self.bias) if t is not None)

    def factors(self):
        """(L, R) as fp32 (out_features, rank) / (rank, in_features): an fp16 factor as stored, a
        coded one as c (scale / k) with the fp32 division the kernel makes."""
        def deq(codes, scale, bits, cols):
            c = unpack_bytes(codes, bits)[:, :cols].float()
            return c * (torch.tensor(scale, dtype=torch.float32) / torch.tensor(float(_k(bits)), dtype=torch.float32))
        L = self.L.detach().float() if self.L_codes is None else deq(self.L_codes, self.lscale, self.L_bits, self.rank)
        R = (self.R.detach().float() if self.R_codes is None
             else deq(self.R_codes, self.rscale, self.R_bits, self.in_features))
        return L, R

    def dense_weight(self) -> torch.Tensor:
        """gs (Q + L R) as a dense fp32 (out_features, in_features) tensor, by torch ops (checks
        and baselines only): Q = c (s / k), a coded factor likewise; an NF layer's Q = I[idx] (s / D)
        with the integer levels I and the fp32 division the kernel makes."""
        if self.q_format == Q_FORMAT_NF:
            idx = unpack_index_bytes(self.codes, self.bits)[:, :self.in_features].long()
            c = torch.tensor(K.NF_LEVELS[self.bits], dtype=torch.float32, device=idx.device)[idx]
            k = K.NF_DENOM[self.bits]
        else:
            k = _k(self.bits)
            c = unpack_bytes(self.codes, self.bits)[:, :self.in_features].float()
        sk = (torch.tensor(self.qscale, dtype=torch.float32) / torch.tensor(float(k), dtype=torch.float32)).item()
        L, R = self.factors()
        return self.gscale * (c * sk + L @ R)

    def materialize(self, dtype=torch.float16, out=None) -> torch.Tensor:
        """gs (Q + L R) as a dense (out_features, in_features) device tensor from the packed form by
        cq_linear_dequant (csrc/cq_linear_dequant.hip): the fp32 weight of that entry's contract,
        rounded once to dtype (fp16, bf16 or fp32).  out: the tensor to fill instead of a new one (its
        dtype counts; may be a view with a row stride and unit column stride).  While the factors
        are trainable the masters rounded to fp16 are used, as forward does.  There is no CPU path."""
        if not self.codes.is_cuda or (out is not None and not out.is_cuda):
            raise RuntimeError("CalderaLinear needs HIP device tensors (no CPU fallback)")
        if out is None:
            if dtype not in (torch.float16, torch.bfloat16, torch.float32):
                raise ValueError(f"CalderaLinear.materialize: dtype {dtype} not fp16, bf16 or fp32")
            out = torch.empty((self.out_features, self.in_features), dtype=dtype, device=self.codes.device)
        L16, R16 = _fp16_factors(self.L, self.R) if self.factors_trainable else (None, None)
        return _dequant(self, out, L16, R16)

    @property
    def dense_prefill_tokens(self):
        """None (the default: every forward and backward is the packed kernels'), or the token count T
        from which the layer materialises its fp16 weight into one scratch buffer shared by all
        layers of the stream and runs the dense GEMM instead of the prefill kernels, forward and
        input gradient alike (`_launch_packed`).  An int above `_lib.LINEAR_DECODE_MAX_TOKENS`.  A
        plain attribute: not part of `state_dict()` nor of the extra state."""
        return self.__dict__.get("_dense_prefill_tokens")

    @dense_prefill_tokens.setter
    def dense_prefill_tokens(self, tokens):
        self.__dict__["_dense_prefill_tokens"] = check_dense_prefill_tokens(tokens)

    # ------------------------------------------------------------------ fine-tuning
    @property
    def factors_trainable(self) -> bool:
        """True between `enable_factor_training` and `freeze_factors`."""
        return "L" in self._parameters

    def enable_factor_training(self, master_dtype=torch.float32):
        """Replace the fp16 buffers `L` and `R` by `nn.Parameter`s of the same names (state-dict keys
        unchanged), widened exactly to master_dtype, and return them.  Every forward rounds them to
        fp16 for the kernel; the gradient passes straight through that rounding, in master_dtype.
        The codes and the bias stay frozen buffers."""
        if self.L_codes is not None or self.R_codes is not None:
            raise ValueError("CalderaLinear.enable_factor_training: a coded factor has no gradient "
                             f"(L_bits={self.L_bits}, R_bits={self.R_bits})")
        if self.rank == 0:
            raise ValueError("CalderaLinear.enable_factor_training: rank 0, no factors to train")
        if not self.factors_trainable:
            for name in ("L", "R"):
                master = getattr(self, name).detach().to(master_dtype)
                delattr(self, name)
                self.register_parameter(name, torch.nn.Parameter(master))
        return [self.L, self.R]

    def freeze_factors(self):
        """Round the master factors to fp16 (nearest even) and keep them as buffers again: the
        layer is the inference layer `to_result`, `packed_bytes` and `state_dict` know."""
        if self.factors_trainable:
            for name in ("L", "R"):
                stored = getattr(self, name).detach().to(torch.float16).contiguous()
                delattr(self, name)
                self.register_buffer(name, stored)
        return self

    # ------------------------------------------------------------------ forward (`_GroupMember`)
    @property
    def _packed(self):
        return self

    def _with_graph(self, x, L, R):
        return _PackedLinearFunction.apply(x, L, R, self)

    def _without_graph(self, x, L16, R16):
        x2 = _fp16_rows(x, self.in_features)
        y = torch.empty((x2.shape[0], self.out_features), dtype=_out_dtype(x.dtype), device=x.device)
        _launch_packed(self, x2, y, L16, R16)
        return _like_input(y, x, self.out_features)


def _next_pow2(n: int) -> int:
    return 1 << (int(n) - 1).bit_length()


SIGN_SEED_LIMIT = 1 << 53  # seeds are ints in [0, 2^53): they survive JSON (a results file's `extra`)
_M64 = (1 << 64) - 1


def mix64(x: int) -> int:
    """The 64-bit mix function of the sign vectors (splitmix64's), all arithmetic mod 2^64."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _check_sign_seed(seed, what="seed"):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < SIGN_SEED_LIMIT:
        raise ValueError(f"hadamard_sign_vector: {what} {seed!r} is not an int in [0, 2^53)")
    return seed


def hadamard_sign_vector(seed: int, length: int) -> torch.Tensor:
    """The +-1 vector (int8, CPU) of the randomised Hadamard transform for `seed`, an int in [0, 2^53):
    element i is -1 iff bit 63 of mix64(mix64(seed) + i) is set.  A counter-based hash this project defines,
    so a results file that stores the seed does not depend on a library's generator; a vector is a prefix
    of any longer one of the same seed."""
    import numpy as np
    _check_sign_seed(seed)
    length = int(length)
    if length < 0:
        raise ValueError(f"hadamard_sign_vector: length {length} is negative")
    x = np.arange(length, dtype=np.uint64) + np.uint64(mix64(seed))  # uint64 arrays wrap mod 2^64
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return torch.from_numpy(np.where((x >> np.uint64(63)).astype(bool), -1, 1).astype(np.int8))


class HadamardCalderaLinear(_GroupMember, torch.nn.Module):
    """A layer decomposed in the Hadamard basis (`model.apply_caldera_quantization(packed=True,
    packed_hadamard=True)`): `inner` is the CalderaLinear of W~ ~ gs (Q + L R) ~ H1 pad(W) H2 on
    the padded (pr, pc) = (next_pow2(out_features), next_pow2(in_features)) grid, H the
    normalised Sylvester-Hadamard matrices.  H is symmetric and orthogonal, so

        y = x W^T = (H1 (W~ (H2 pad(x))))[:out_features] + bias

    and forward is three launch groups with no torch arithmetic: cq_hadamard_rows on x (read in
    its own dtype, written as the fp16 the inner layer takes), the inner layer's packed forward
    into an fp32 buffer, cq_hadamard_rows on that (+ bias) written in x's dtype.  `inner` may
    use any Q / factor format CalderaLinear supports and has no bias; `bias` (out_features,)
    fp32 or None is added by the output transform.  Extra state: in_features, out_features.

    Training: with grad mode on and x requiring grad (or the inner factors trainable) forward
    runs the same launches with a graph (`_HadamardLinearFunction`); the backward transforms dy
    and dx with cq_hadamard_rows around the inner layer's input gradient, and the inner fp16
    factors train in the Hadamard basis (`enable_factor_training`).  The bias stays frozen.

    sign_seeds = (seed_out, seed_in), two ints in [0, 2^53): the layer is one of the randomised transform
    W~ ~ H1 diag(su) pad(W) diag(sv) H2 with su = hadamard_sign_vector(seed_out, out_features) and
    sv = hadamard_sign_vector(seed_in, in_features), held as the int8 buffers `sign_out` and `sign_in`, and

        y = su * (H1 (W~ (H2 (sv * pad(x)))))[:out_features] + bias

    through cq_hadamard_signed_rows for both transforms (the flips are exact; the backward mirrors them: dy
    goes in with sign_in = su, dx comes out with sign_out = sv, the factor gradients stay in the signed
    basis).  Extra state gains "sign_seeds".  With None, the default, there are no such buffers, no such key,
    and the launches are the unsigned entries': nothing about the layer differs from one built without the
    keyword."""

    sign_seeds = None  # the class default: a layer unpickled from before the keyword is unsigned

    def __init__(self, inner: CalderaLinear, in_features: int, out_features: int, bias=None, sign_seeds=None):
        super().__init__()
        m, n = int(out_features), int(in_features)
        pr, pc = _next_pow2(m), _next_pow2(n)
        if pr > K.HADAMARD_MAX_N or pc > K.HADAMARD_MAX_N:
            raise ValueError(f"HadamardCalderaLinear: padded shape {(pr, pc)} exceeds {K.HADAMARD_MAX_N} "
                             "(cq_hadamard_rows' largest transform)")
        if not isinstance(inner, CalderaLinear) or (inner.out_features, inner.in_features) != (pr, pc):
            raise ValueError(f"HadamardCalderaLinear: inner must be a CalderaLinear of the padded shape {(pr, pc)} "
                             f"for a {(m, n)} layer, got "
                             f"{(getattr(inner, 'out_features', None), getattr(inner, 'in_features', None))}")
        if inner.bias is not None:
            raise ValueError("HadamardCalderaLinear: the inner layer must have no bias (the output transform adds it)")
        if bias is not None and tuple(bias.shape) != (m,):
            raise ValueError(f"HadamardCalderaLinear: bias {tuple(bias.shape)} does not fit ({m},)")
        self.in_features, self.out_features = n, m
        self.inner = inner
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).contiguous())
        self.sign_seeds = None
        if sign_seeds is not None:
            seeds = tuple(sign_seeds)
            if len(seeds) != 2:
                raise ValueError(f"HadamardCalderaLinear: sign_seeds {sign_seeds!r} is not (seed_out, seed_in)")
            self.sign_seeds = (_check_sign_seed(seeds[0], "seed_out"), _check_sign_seed(seeds[1], "seed_in"))
            dev = inner.codes.device
            self.register_buffer("sign_out", hadamard_sign_vector(self.sign_seeds[0], m).to(dev))
            self.register_buffer("sign_in", hadamard_sign_vector(self.sign_seeds[1], n).to(dev))

    @property
    def padded_shape(self):
        return self.inner.out_features, self.inner.in_features

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_decomposition(cls, dec, Q_bits, original_shape, bias=None, L_bits=None, R_bits=None, Q_method="uniform",
                           sign_seeds=None):
        """From the CalderaDecomposition of H1 pad(W) H2 (as `CalderaLinear.from_decomposition`
        takes it, Q_method included) and W's own shape (out_features, in_features).  sign_seeds: the
        (seed_out, seed_in) of the sign vectors when the decomposed matrix was H1 diag(su) pad(W) diag(sv) H2."""
        m, n = (int(v) for v in original_shape)
        if max(_next_pow2(m), _next_pow2(n)) > K.HADAMARD_MAX_N:
            raise ValueError(f"HadamardCalderaLinear: padded shape {(_next_pow2(m), _next_pow2(n))} exceeds "
                             f"{K.HADAMARD_MAX_N} (cq_hadamard_rows' largest transform)")
        inner = CalderaLinear.from_decomposition(dec, Q_bits, None, L_bits=L_bits, R_bits=R_bits, Q_method=Q_method)
        return cls(inner, n, m, bias, sign_seeds)

    @classmethod
    def from_result(cls, res, bias=None):
        """From a `sharding.MatrixResult` of the padded layer whose extra["hadamard"] holds the
        original [out_features, in_features] and, for a signed layer, extra["hadamard_signs"] the
        [seed_out, seed_in] (what `to_result` writes)."""
        shape = (res.extra or {}).get("hadamard")
        if shape is None or len(shape) != 2:
            raise ValueError(f"HadamardCalderaLinear.from_result: {res.name}: extra has no \"hadamard\": [m, n]")
        m, n = int(shape[0]), int(shape[1])
        signs = (res.extra or {}).get("hadamard_signs")
        if signs is not None and len(signs) != 2:
            raise ValueError(f"HadamardCalderaLinear.from_result: {res.name}: extra[\"hadamard_signs\"] {signs!r} is not "
                             "[seed_out, seed_in]")
        return cls(CalderaLinear.from_result(res, None), n, m, bias,
                   None if signs is None else (int(signs[0]), int(signs[1])))

    def to_result(self, name: str):
        """`inner.to_result(name)` (the padded layer) with extra["hadamard"] = [out_features,
        in_features] and, for a signed layer, extra["hadamard_signs"] = [seed_out, seed_in];
        `from_result` inverts it."""
        res = self.inner.to_result(name)
        res.extra = dict(res.extra or {})
        res.extra["hadamard"] = [self.out_features, self.in_features]
        if self.sign_seeds is not None:
            res.extra["hadamard_signs"] = list(self.sign_seeds)
        return res

    # ------------------------------------------------------------------ state
    def get_extra_state(self):
        state = {"in_features": self.in_features, "out_features": self.out_features}
        if self.sign_seeds is not None:
            state["sign_seeds"] = tuple(self.sign_seeds)
        return state

    def set_extra_state(self, state):
        for key, v in state.items():
            setattr(self, key, tuple(v) if key == "sign_seeds" else v)

    def extra_repr(self):
        signs = "" if self.sign_seeds is None else f", sign_seeds={self.sign_seeds}"
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}{signs}"

    def packed_bytes(self) -> int:
        """Bytes a forward streams for the weights: the inner layer's (+ bias)."""
        return self.inner.packed_bytes() + (0 if self.bias is None else self.bias.numel() * self.bias.element_size())

    def dense_weight(self) -> torch.Tensor:
        """(H1 inner.dense_weight() H2)[:out_features, :in_features] as dense fp32, by torch ops
        (checks and baselines only); a signed layer's rows and columns carry su and sv."""
        from .model import normalized_hadamard
        Wt = self.inner.dense_weight()
        pr, pc = self.padded_shape
        H1, H2 = normalized_hadamard(pr, Wt.device), normalized_hadamard(pc, Wt.device)
        W = (H1 @ Wt @ H2)[:self.out_features, :self.in_features]
        if self.sign_seeds is not None:
            W = W * self.sign_out.to(W.device, torch.float32)[:, None] * self.sign_in.to(W.device, torch.float32)[None, :]
        return W.contiguous()

    def materialize(self, dtype=torch.float16, out=None) -> torch.Tensor:
        """(H1 W~ H2)[:out_features, :in_features] as a dense device tensor by kernels alone: the inner
        layer's `materialize` in fp32, cq_hadamard_rows on its rows (W~ H2, cut to in_features
        columns), then on the rows of the transposed result (H1 that, cut to out_features), which is
        rounded once to dtype (fp16, bf16 or fp32).  A signed layer takes cq_hadamard_signed_rows for both,
        with sign_out = sv on the first and su on the second.  Not a hot path: two fp32 temporaries of
        the padded size.  out: as `CalderaLinear.materialize`."""
        if out is not None and not out.is_cuda:
            raise RuntimeError("CalderaLinear needs HIP device tensors (no CPU fallback)")
        if out is not None:
            dtype = out.dtype
        if dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise ValueError(f"HadamardCalderaLinear.materialize: dtype {dtype} not fp16, bf16 or fp32")
        pr, pc = self.padded_shape
        m, n = self.out_features, self.in_features
        Wt = self.inner.materialize(torch.float32)
        A = torch.empty((pr, n), dtype=torch.float32, device=Wt.device)
        _transform(self, Wt, A, n_in=pc, n_out=n, P=pc, sign_out="sign_in")
        At = A.t().contiguous()
        Wo = torch.empty((n, m), dtype=dtype, device=Wt.device)
        _transform(self, At, Wo, n_in=pr, n_out=m, P=pr, sign_out="sign_out")
        if out is None:
            return Wo.t().contiguous()
        if tuple(out.shape) != (m, n):
            raise ValueError(f"HadamardCalderaLinear.materialize: out {tuple(out.shape)} does not fit {(m, n)}")
        return out.copy_(Wo.t())

    @property
    def dense_prefill_tokens(self):
        """`inner.dense_prefill_tokens`: the inner layer's launch takes the dense path, the
        transforms around it stay as they are."""
        return self.inner.dense_prefill_tokens

    @dense_prefill_tokens.setter
    def dense_prefill_tokens(self, tokens):
        self.inner.dense_prefill_tokens = tokens

    # ------------------------------------------------------------------ fine-tuning
    @property
    def factors_trainable(self) -> bool:
        """`inner.factors_trainable`."""
        return self.inner.factors_trainable

    def enable_factor_training(self, master_dtype=torch.float32):
        """`inner.enable_factor_training`: the parameters are `inner.L` and `inner.R`, factors of the
        weight in the Hadamard basis, and their gradients are taken in that basis."""
        return self.inner.enable_factor_training(master_dtype)

    def freeze_factors(self):
        self.inner.freeze_factors()
        return self

    # ------------------------------------------------------------------ forward
    def _forward_launches(self, x, L16=None, R16=None):
        """The three launch groups on x: (x2, x^, y) with x2 the (T, in_features) view they read, x^
        the fp16 (T, pc) transform the inner layer takes and y (T, out_features) in x2's dtype.
        L16 / R16: the inner layer's fp16 factors when they are not its buffers."""
        pr = self.padded_shape[0]
        x2, xh = _hadamard_input(self, x)
        T = x2.shape[0]
        y32 = torch.empty((T, pr), dtype=torch.float32, device=x.device)
        _launch_packed(self.inner, xh, y32, L16, R16)
        y = torch.empty((T, self.out_features), dtype=x2.dtype, device=x.device)
        _transform(self, y32, y, n_in=pr, n_out=self.out_features, P=pr, bias=self.bias, sign_out="sign_out")
        return x2, xh, y

    @property
    def _packed(self):
        return self.inner

    def _with_graph(self, x, L, R):
        return _HadamardLinearFunction.apply(x, L, R, self)

    def _without_graph(self, x, L16, R16):
        return _like_input(self._forward_launches(x, L16, R16)[2], x, self.out_features)


def _group_operands(lin):
    """`_lib.linear_group_args`' member dict of one layer: the operands `_launch_packed` passes."""
    L, R, r, L_codes, R_codes = _operands(lin)
    return dict(codes=lin.codes, qscale=lin.qscale, gscale=lin.gscale, L=L, R=R, bias=lin.bias, m=lin.out_features,
                n=lin.in_features, bits=lin.bits, r=r, L_codes=L_codes, R_codes=R_codes)


def _own_inference_launch(x, packed, limit) -> bool:
    """Whether a grouped or fused launch of the `CalderaLinear` layers `packed` is their own inference launch
    for x: no autograd graph is needed, the token count does not exceed `limit` (None: no limit), no layer has
    trainable factors and no layer's `dense_prefill_tokens` is reached."""
    if torch.is_grad_enabled() and x.requires_grad:
        return False
    T = x.numel() // max(x.shape[-1], 1)
    if limit is not None and T > limit:
        return False
    return not any(lin.factors_trainable or _use_dense(lin, T) for lin in packed)


class _SharedInputGroup:
    """The protocol `CalderaLinearGroup` and `HadamardLinearGroup` share: a plain object over layers that
    read the same activation; each member keeps a back-reference in its `__dict__["_group"]` and calls
    `_member_forward` from its `forward`.  The members' rules that both groups have are checked here, in one
    order; a subclass names its member type (`_member_type`) and the largest set (`_max_members`), words the
    refusal of another type (`_wrong_type`), and adds its own rules: `_member_free(i, lin)` raises for a
    member that is taken in some other way, `_misfit(members, labels)` gives the reason why the first
    len(members) members do not fit one launch (or None), `_token_limit()` the largest token count of the
    grouped launch (None: no limit).  It provides `_launch(x)` (the grouped launches: the members' outputs in
    member order).  Members provide `_forward_alone(x)` and `_packed` (`_GroupMember`)."""

    def __init__(self, members):
        members = list(members)
        who, kind = type(self).__name__, self._member_type
        if not 1 <= len(members) <= self._max_members():
            raise ValueError(f"{who}: {len(members)} members, not 1 .. {self._max_members()}")
        labels = [f"member {i}" for i in range(len(members))]
        for i, lin in enumerate(members):
            if not isinstance(lin, kind):
                raise ValueError(f"{who}: member {i} {self._wrong_type(lin)}")
            if any(lin is other for other in members[:i]):
                raise ValueError(f"{who}: member {i} is given twice")
            if lin.__dict__.get("_group") is not None:
                raise ValueError(f"{who}: member {i} is already in a group (dissolve() it first)")
            self._member_free(i, lin)
            device, first = lin._packed.codes.device, members[0]
            if device != first._packed.codes.device:
                raise ValueError(f"{who}: member {i}: device {device} differs from member 0's "
                                 f"{first._packed.codes.device}")
            if lin.in_features != first.in_features:
                raise ValueError(f"{who}: member {i}: in_features {lin.in_features} differs from member 0's "
                                 f"{first.in_features}")
            why = self._misfit(members[:i + 1], labels)
            if why is not None:
                raise ValueError(f"{who}: {why}")
        self.members = tuple(members)
        self._key = None    # (weakref of x, x._version, x.data_ptr()) of the kept outputs
        self._kept = {}     # id(member) -> its output for that x, until claimed
        for lin in self.members:
            lin.__dict__["_group"] = self

    def _wrong_type(self, lin):
        return f"is a {type(lin).__name__}, not a {self._member_type.__name__}"

    def _member_free(self, i, lin):
        pass

    def _token_limit(self):
        return None

    def _grouped(self, x) -> bool:
        """Whether the grouped launches are the members' own inference launches for this x."""
        return _own_inference_launch(x, [lin._packed for lin in self.members], self._token_limit())

    def __len__(self):
        return len(self.members)

    def __getstate__(self):  # a weak reference does not pickle; the kept outputs are transient
        return {"members": self.members, "_key": None, "_kept": {}}

    def dissolve(self):
        """Remove the members' back-references: every layer runs alone again."""
        for lin in self.members:
            if lin.__dict__.get("_group") is self:
                del lin.__dict__["_group"]
        self._key, self._kept = None, {}

    def __call__(self, x: torch.Tensor):
        self._key, self._kept = None, {}
        if not self._grouped(x):
            return tuple(lin._forward_alone(x) for lin in self.members)
        return self._launch(x)

    def _member_forward(self, member, x):
        """`member.forward(x)` of a grouped layer, see `CalderaLinearGroup`'s docstring."""
        if member not in self.members:
            # a shallow copy of a member (e.g. a DataParallel replica) still points here: it is not ours
            return member._forward_alone(x)
        if x.is_inference() or not self._grouped(x):
            # an inference tensor has no version counter: a write in place could not be told from the
            # x the kept outputs belong to, so none are kept for it
            self._key, self._kept = None, {}
            return member._forward_alone(x)
        key = self._key
        if (key is not None and key[0]() is x and key[1] == x._version and key[2] == x.data_ptr()
                and id(member) in self._kept):
            return self._kept.pop(id(member))
        self._key, self._kept = None, {}   # another x (or a second call with this one): start over
        ys = self._launch(x)
        self._kept = {id(lin): y for lin, y in zip(self.members, ys) if lin is not member}
        self._key = (weakref.ref(x), x._version, x.data_ptr())
        return ys[self.members.index(member)]


class CalderaLinearGroup(_SharedInputGroup):
    """Packed layers that read the same activation (q / k / v, gate / up), run as one z launch and
    one code + L launch (cq_linear_group_forward) instead of two launches each; every member's output
    has the bits the member computes alone.  A plain object, not a module: the members stay where they
    are in the model, and their state dict, extra state, `to_result`, `packed_bytes` and `_apply` do
    not know about it.  Each member keeps a back-reference in its `__dict__` (`CalderaLinear.group`).

    members: 1 .. `_lib.LINEAR_GROUP_MAX` `CalderaLinear` layers on one device that share
    in_features, bits and q_format, and, among those with rank > 0, L_bits and R_bits; none of them in
    another group.  A `HadamardCalderaLinear` is refused (its transforms are per layer): sets of those form a
    `HadamardLinearGroup`.
    ValueError names the member and the attribute.

    group(x) -> the members' outputs in member order, each shaped and typed as member(x).

    member(x) of a grouped layer runs the whole group on the first call with a given x, returns its
    own output and keeps the siblings' until they are claimed: a sibling called with the same x (the
    same tensor object, at the same version and data pointer) gets its kept output, which is then
    dropped.  A call with any other x starts over and releases what was not claimed.  x itself is
    held through a weak reference only.  So `q_proj(h)`, `k_proj(h)`, `v_proj(h)` of unchanged model
    code are one launch pair.  (A write to x's memory that does not bump its version counter, e.g.
    through `x.data`, is not seen.)

    The grouped launch is taken only where it is the members' own inference launch: no autograd graph
    is needed (grad mode off, or x does not require grad), no member has trainable factors, and no
    member's `dense_prefill_tokens` applies at this token count.  Otherwise every member runs alone,
    as without a group.

    member(x) also runs alone when x is an inference tensor (one made under `torch.inference_mode()`):
    it has no version counter, so a kept output could outlive a write to x.  Use `torch.no_grad()`
    for the transparent path, or call group(x), which keeps nothing and launches grouped there too.

    The back-reference is an ordinary attribute, so a shallow copy of a member (`nn.DataParallel`'s
    replicas) carries it without being a member: such a copy runs alone, on its own operands.
    `copy.deepcopy` or pickling of a single grouped layer takes the group, and with it the siblings,
    along; copy the model that holds them all, or `dissolve()` first."""

    _member_type = CalderaLinear

    def _max_members(self):
        return K.LINEAR_GROUP_MAX

    def _wrong_type(self, lin):
        if isinstance(lin, HadamardCalderaLinear):
            return "is a HadamardCalderaLinear: its input and output transforms are per layer, it cannot be grouped"
        return super()._wrong_type(lin)

    def _misfit(self, members, labels):  # as each member is reached: the first misfit in member order is reported
        return _formats_fit(members, labels)

    def _launch(self, x):
        """One cq_linear_group_forward on x: `CalderaLinear.forward`'s x handling and output dtype."""
        n = self.members[0].in_features
        _check_last_dim(x, n)
        x2 = _fp16_rows(x, n)
        ys = [torch.empty((x2.shape[0], lin.out_features), dtype=_out_dtype(x.dtype), device=x.device)
              for lin in self.members]
        K.linear_group_forward(x2, [_group_operands(lin) for lin in self.members], ys, self.members[0].q_format)
        return tuple(_like_input(y, x, lin.out_features) for y, lin in zip(ys, self.members))


def _formats_fit(layers, labels, what=""):
    """None when the `CalderaLinear` layers `layers` fit one cq_linear_group_forward -- bits and q_format shared,
    L_bits and R_bits shared among those with rank > 0 (a rank-0 layer fits any factor format) -- else the
    reason for the first layer that does not, as "<label>: <what><attribute> a differs from <label>'s b" with
    the layers called by `labels`."""
    ranked = None
    for i, lin in enumerate(layers):
        for attr in ("bits", "q_format"):
            if getattr(lin, attr) != getattr(layers[0], attr):
                return (f"{labels[i]}: {what}{attr} {getattr(lin, attr)} differs from {labels[0]}'s "
                        f"{getattr(layers[0], attr)}")
        if lin.rank > 0:
            if ranked is None:
                ranked = i
            for attr in ("L_bits", "R_bits"):
                if getattr(lin, attr) != getattr(layers[ranked], attr):
                    return (f"{labels[i]}: {what}{attr} {getattr(lin, attr)} differs from {labels[ranked]}'s "
                            f"{getattr(layers[ranked], attr)}")
    return None


def _hadamard_entry(had, name):
    """(entry, signed): `_lib`'s hadamard_<name> for an unsigned layer, hadamard_signed_<name> for a signed one,
    looked up when called.  The one place that tells the two apart: an unsigned layer launches the unsigned
    entries, with their keywords."""
    if had.sign_seeds is None:
        return getattr(K, "hadamard_" + name), False
    return getattr(K, "hadamard_signed_" + name), True


def _transform(had, x, y, *, n_in, n_out, P, bias=None, sign_in=None, sign_out=None):
    """cq_hadamard_rows on x into y for an unsigned layer, cq_hadamard_signed_rows for a signed one.  sign_in /
    sign_out: which of the layer's vectors, "sign_in" (sv) or "sign_out" (su), flips the transform's input resp.
    output (None: no flip); an unsigned layer has neither vector and its entry neither keyword."""
    entry, signed = _hadamard_entry(had, "rows")
    if not signed:
        return entry(x, y, n_in=n_in, n_out=n_out, P=P, bias=bias)
    return entry(x, y, n_in=n_in, n_out=n_out, P=P, bias=bias, sign_in=sign_in and getattr(had, sign_in),
                 sign_out=sign_out and getattr(had, sign_out))


def _hadamard_input(had, x):
    """(x2, x^) of `HadamardCalderaLinear._forward_launches`: the (T, in_features) view of x the input
    transform reads and the fp16 (T, pc) transform every layer with this in_features takes."""
    n, pc = had.in_features, had.padded_shape[1]
    _check_last_dim(x, n)
    x2 = x.reshape(-1, n)
    if x2.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        x2 = x2.float()
    if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < n):  # `_rows`' rule
        x2 = x2.contiguous()
    xh = torch.empty((x2.shape[0], pc), dtype=torch.float16, device=x.device)
    # signed: x^ = H2 (sv * pad(x)), which every signed layer with this in_features and seed_in takes
    _transform(had, x2, xh, n_in=n, n_out=pc, P=pc, sign_in="sign_in")
    return x2, xh


def _signs_fit(layers, labels):
    """None when the `HadamardCalderaLinear` layers share one x^ -- all unsigned, or all signed with the same
    seed_in -- else the reason for the first layer that does not, the layers called by `labels`."""
    first = layers[0].sign_seeds
    for had, label in zip(layers[1:], labels[1:]):
        seeds = had.sign_seeds
        if (seeds is None) != (first is None):
            return (f"{label}: sign_seeds {seeds} but {labels[0]}'s are {first}: signed and unsigned layers do not "
                    "share the input transform")
        if seeds is not None and seeds[1] != first[1]:
            return f"{label}: sign seed_in {seeds[1]} differs from {labels[0]}'s {first[1]}"
    return None


# The largest token count at which `HadamardLinearGroup` takes the grouped launches; None: no limit.  Measured on
# 3 x 4096 x 4096 (tools/bench_hadamard_group.py): grouped is faster at every T measured, decode and
# prefill (2-bit, r = 128: 33.4 against 61.6 us at T = 1, 158.5 against 435.2 us at T = 64, 264.2 against 449.5 us
# at T = 512; 4-bit, r = 256: 37.0 / 70.5, 178.8 / 492.7, 257.1 / 497.0 us), so there is none.  `HadamardGatedMLP`'s
# `max_fused_tokens` defaults to None for the same reason (2 x 11008 x 4096: 527.2 against 607.5 us at T = 512 at
# 2 bits, 463.0 against 527.6 us at 4 bits).
HADAMARD_GROUP_TOKEN_LIMIT = None


class HadamardLinearGroup(_SharedInputGroup):
    """`HadamardCalderaLinear` layers that read the same activation (q / k / v, gate / up), run as four
    launches instead of four each: one input transform (they share x^ = H2 pad(x)), the inner layers'
    grouped launch pair (cq_linear_group_forward), and one grouped output transform
    (cq_hadamard_group_rows) per distinct padded output width, members bucketed in member order -- one
    when all pr agree, two with GQA's smaller k / v.  Every member's output has the bits the member
    computes alone.  A plain object with `CalderaLinearGroup`'s protocol: group(x), the transparent
    member(x) with outputs kept per x, inference tensors and shallow copies running alone, `dissolve()`.

    members: 1 .. `_lib.HADAMARD_GROUP_MAX` `HadamardCalderaLinear` layers on one device that share
    in_features (hence pc and x^) and whose inner layers share bits and q_format and, among those with
    rank > 0, L_bits and R_bits; none of them in another group, none of their inner layers in a
    `CalderaLinearGroup`; all unsigned, or all signed with one seed_in (they share x^; seed_out is per
    member).  ValueError names the member and the attribute.  Signed members run the signed input transform
    once and cq_hadamard_signed_group_rows; unsigned ones the launches they always had.

    The grouped launches are taken where they are the members' own inference launches (no autograd graph
    needed, no inner layer with trainable factors, no `dense_prefill_tokens` reached) and the token count
    does not exceed `HADAMARD_GROUP_TOKEN_LIMIT`; otherwise every member runs alone.  The inner group
    entry is called on the inner layers' operands directly: no `CalderaLinearGroup` is made or disturbed."""

    _member_type = HadamardCalderaLinear

    def _max_members(self):
        return K.HADAMARD_GROUP_MAX

    def _member_free(self, i, had):
        if had.inner.__dict__.get("_group") is not None:
            raise ValueError(f"{type(self).__name__}: member {i}: inner is in a CalderaLinearGroup (dissolve() it first)")

    def _misfit(self, members, labels):  # on the whole set, after every member's own rules
        if len(members) < len(labels):
            return None
        return _formats_fit([had.inner for had in members], labels, "inner ") or _signs_fit(members, labels)

    def _token_limit(self):
        return HADAMARD_GROUP_TOKEN_LIMIT

    def _launch(self, x):
        """`HadamardCalderaLinear._forward_launches` for every member: x^ once, the inner layers grouped,
        the output transforms grouped by padded width."""
        x2, xh = _hadamard_input(self.members[0], x)
        T = x2.shape[0]
        y32 = [torch.empty((T, had.padded_shape[0]), dtype=torch.float32, device=x.device) for had in self.members]
        K.linear_group_forward(xh, [_group_operands(had.inner) for had in self.members], y32,
                               self.members[0].inner.q_format)
        ys = [torch.empty((T, had.out_features), dtype=x2.dtype, device=x.device) for had in self.members]
        entry, signed = _hadamard_entry(self.members[0], "group_rows")
        buckets = {}  # pr -> the members' transforms, in member order
        for had, v, y in zip(self.members, y32, ys):
            pr = had.padded_shape[0]
            t = dict(x=v, y=y, n_in=pr, n_out=had.out_features, P=pr, bias=had.bias)
            if signed:
                t["sign_out"] = had.sign_out
            buckets.setdefault(pr, []).append(t)
        for transforms in buckets.values():
            entry(transforms)
        return tuple(_like_input(y, x, had.out_features) for y, had in zip(ys, self.members))


ACTIVATIONS = {"silu": K.ACT_SILU, "identity": K.ACT_IDENTITY}
# Q bits -> the largest token count at which `CalderaGatedMLP` takes the fused launch by default.  Measured on
# 2 x 11008 x 4096 (tools/bench_linear_mlp.py): at 2 bits (r = 128) the fused launch is faster at
# every T measured up to 2048, so there is no limit; at 4 bits (r = 256) it is level with the grouped pair +
# silu + product at T = 64 (170.4 against 170.6 us) and slower at T = 512 (353.0 against 350.2 us) and
# T = 2048 (1104 against 1077 us), so above 64 tokens the block takes the unfused formula.
FUSED_TOKEN_LIMIT = {2: None, 4: 64}


def _act_torch(act: int, g: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.silu(g) if act == K.ACT_SILU else g


def _pair_fit(gate, up, kind, what="", refused=None):
    """None when `gate` and `up` are two layers of type `kind` on one device with the same shape whose packed
    layers fit one launch (`_formats_fit`, their attributes called "<what><attribute>"), else the reason as a
    string that names the attribute.  refused: (another type, the words for a layer of it)."""
    for name, lin in (("gate_proj", gate), ("up_proj", up)):
        if refused is not None and isinstance(lin, refused[0]):
            return f"{name} {refused[1]}"
        if not isinstance(lin, kind):
            return f"{name} is a {type(lin).__name__}, not a {kind.__name__}"
    if gate is up:
        return "gate_proj and up_proj are the same layer"
    packed = (gate._packed, up._packed)
    if packed[1].codes.device != packed[0].codes.device:
        return f"up_proj: device {packed[1].codes.device} differs from gate_proj's {packed[0].codes.device}"
    for attr in ("in_features", "out_features"):
        if getattr(up, attr) != getattr(gate, attr):
            return f"up_proj: {attr} {getattr(up, attr)} differs from gate_proj's {getattr(gate, attr)}"
    return _formats_fit(packed, ("gate_proj", "up_proj"), what)


def glu_fit(gate, up):
    """None when the layers `gate` and `up` fit cq_linear_glu_forward, else the reason as a string that
    names the attribute."""
    return _pair_fit(gate, up, CalderaLinear, refused=(
        HadamardCalderaLinear, "is a HadamardCalderaLinear: its input and output transforms are per layer, it does "
                               "not fit the fused launch"))


def hadamard_glu_fit(gate, up):
    """None when the `HadamardCalderaLinear` layers `gate` and `up` fit `HadamardGatedMLP`'s fused launches,
    else the reason as a string that names the attribute."""
    return (_pair_fit(gate, up, HadamardCalderaLinear, "inner ")
            or _signs_fit((gate, up), ("gate_proj", "up_proj")))


class _GatedMLP(torch.nn.Module):
    """What `CalderaGatedMLP` and `HadamardGatedMLP` share: the construction checks, the three submodules, the
    choice between the fused launches and the formula, and `forward`.  A subclass provides `_misfit(gate, up)`
    (its fit function, looked up when called), `_auto_limit` (whether `max_fused_tokens` may be "auto":
    `FUSED_TOKEN_LIMIT` for the gate's Q bits) and `_fused_launches(x, gate, up, act)`."""

    def __init__(self, gate_proj, up_proj, down_proj, act, max_fused_tokens):
        super().__init__()
        who = type(self).__name__
        if act not in ACTIVATIONS:
            raise ValueError(f"{who}: act {act!r} not in {tuple(ACTIVATIONS)}")
        why = self._misfit(gate_proj, up_proj)
        if why is not None:
            raise ValueError(f"{who}: {why}")
        if not isinstance(down_proj, torch.nn.Module):
            raise ValueError(f"{who}: down_proj is a {type(down_proj).__name__}, not a module")
        named = ("auto", None) if self._auto_limit else (None,)
        if max_fused_tokens not in named and (isinstance(max_fused_tokens, bool)
                                              or not isinstance(max_fused_tokens, int)):
            words = "\"auto\", None" if self._auto_limit else "None"
            raise ValueError(f"{who}: max_fused_tokens {max_fused_tokens!r} is not {words} or an int")
        self.act = act
        self.max_fused_tokens = max_fused_tokens
        self.gate_proj, self.up_proj, self.down_proj = gate_proj, up_proj, down_proj

    def extra_repr(self):
        return f"act={self.act}"

    def _fused(self, x) -> bool:
        """Whether the fused launches are the layers' own inference launches for this x."""
        gate, up = self.gate_proj, self.up_proj
        if self._misfit(gate, up) is not None:
            return False
        limit = self.max_fused_tokens
        if self._auto_limit and limit == "auto":
            limit = FUSED_TOKEN_LIMIT.get(gate.bits)
        return _own_inference_launch(x, (gate._packed, up._packed), limit)

    def glu(self, x: torch.Tensor) -> torch.Tensor:
        gate, up = self.gate_proj, self.up_proj
        act = ACTIVATIONS[self.act]
        if not self._fused(x):
            return _act_torch(act, gate(x)) * up(x)
        return self._fused_launches(x, gate, up, act)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.down_proj(self.glu(x))


class CalderaGatedMLP(_GatedMLP):
    """A gated MLP block `down_proj(act(gate_proj(x)) * up_proj(x))` whose gate / up pair runs as one z
    launch and one code + L launch that applies the activation and the product in its epilogue
    (cq_linear_glu_forward): no separate activation and product launches, one (T, m) intermediate
    instead of three, one rounding instead of three.

    gate_proj, up_proj: `CalderaLinear` layers on one device that share in_features, out_features, bits
    and q_format, and, when both have rank > 0, L_bits and R_bits.  A `HadamardCalderaLinear` does not
    fit.  ValueError names the attribute.  down_proj: any module.  act: "silu" (the default) or
    "identity" (a bilinear GLU).  The three layers are submodules under exactly these names, so a state
    dict of the original MLP loads into this module and back.

    glu(x) -> act(gate_proj(x)) * up_proj(x), shaped (..., out_features) in x's dtype.  The fused launch
    is taken only where it is the members' own inference launch (`CalderaLinearGroup._grouped`'s
    conditions): no autograd graph is needed, neither layer has trainable factors, no
    `dense_prefill_tokens` applies at this token count, and the token count does not exceed
    `max_fused_tokens` ("auto", the default: `FUSED_TOKEN_LIMIT` for the layers' Q bits, which is where the
    fused launch was measured slower than the unfused path; None: no limit; or an int).  There x is cast to fp16 and h is computed in x's dtype when that is fp16
    or fp32, otherwise in fp32 and then cast, as `CalderaLinear.forward` does.  The pre-activations have
    the bits of the layers' own fp32 outputs; against the unfused formula on fp16 tensors the fused
    result skips the roundings of gate(x), up(x) and act(gate(x)).  Otherwise glu(x) is the formula
    through the layers' ordinary forwards (gradients flow; a `CalderaLinearGroup` they belong to still
    serves them).  The fused path calls the entry on the layers' operands directly: it neither uses nor
    disturbs a group.

    If the two layers stop fitting after construction (one of them replaced or unpacked), glu(x) takes
    the formula as well."""

    _auto_limit = True

    def __init__(self, gate_proj, up_proj, down_proj, act="silu", max_fused_tokens="auto"):
        super().__init__(gate_proj, up_proj, down_proj, act, max_fused_tokens)

    def _misfit(self, gate, up):
        return glu_fit(gate, up)

    def _fused_launches(self, x, gate, up, act):
        n, m = gate.in_features, gate.out_features
        _check_last_dim(x, n)
        x2 = _fp16_rows(x, n)
        h = torch.empty((x2.shape[0], m), dtype=_out_dtype(x.dtype), device=x.device)
        K.linear_glu_forward(x2, _group_operands(gate), _group_operands(up), h, gate.q_format, act)
        return _like_input(h, x, m)


class HadamardGatedMLP(_GatedMLP):
    """A gated MLP block `down_proj(act(gate_proj(x)) * up_proj(x))` whose gate and up are
    `HadamardCalderaLinear` layers, run as four launches: the input transform once (the two share
    x^ = H2 pad(x)), the inner layers' grouped launch pair (cq_linear_group_forward) into two fp32
    (T, pr) buffers, and one output transform of both with the activation and the product in its
    epilogue (cq_hadamard_glu_rows).  The activation cannot sit in the inner pair's epilogue: it comes
    after H1.

    gate_proj, up_proj: `HadamardCalderaLinear` layers on one device that share in_features and
    out_features and whose inner layers share bits and q_format and, when both have rank > 0, L_bits and
    R_bits; both unsigned, or both signed with one seed_in (then the input transform and the gated output
    transform are the signed entries, cq_hadamard_signed_glu_rows with the two layers' sign_out).
    ValueError names the attribute.  down_proj: any module.  act: "silu" (the default) or
    "identity".  The three layers are submodules under exactly these names: state-dict keys are those of
    the original block.

    glu(x) -> act(gate_proj(x)) * up_proj(x), shaped (..., out_features) in x's dtype.  The fused launches
    are taken only where they are the layers' own inference launches: no autograd graph is needed, neither
    inner layer has trainable factors, no `dense_prefill_tokens` applies at this token count, the padded
    width pr does not exceed `_lib.HADAMARD_GLU_MAX_N` (two rows of 32768 do not fit the LDS), the token
    count does not exceed `max_fused_tokens` (None, the default: no limit; or an int), and the two layers
    still fit.  There the pre-activations have the bits of the layers' own fp32 outputs (bias included), h32
    is `cq_linear_glu_forward`'s epilogue sequence on them, and h is rounded once to x's dtype (fp16, bf16 or
    fp32; anything else is computed in fp32 and cast): against the unfused formula on fp16 tensors the
    fused result skips the roundings of gate(x), up(x) and act(gate(x)) -- one rounding instead of three.
    Otherwise glu(x) is the formula through the layers' ordinary forwards (gradients flow; a
    `HadamardLinearGroup` they belong to still serves them).  The fused path calls the entries on the
    layers' operands directly: it neither uses nor disturbs a group."""

    _auto_limit = False

    def __init__(self, gate_proj, up_proj, down_proj, act="silu", max_fused_tokens=None):
        super().__init__(gate_proj, up_proj, down_proj, act, max_fused_tokens)

    def _misfit(self, gate, up):
        return hadamard_glu_fit(gate, up)

    def _fused(self, x) -> bool:
        return super()._fused(x) and self.gate_proj.padded_shape[0] <= K.HADAMARD_GLU_MAX_N

    def _fused_launches(self, x, gate, up, act):
        x2, xh = _hadamard_input(gate, x)
        T, pr, m = x2.shape[0], gate.padded_shape[0], gate.out_features
        v = [torch.empty((T, pr), dtype=torch.float32, device=x.device) for _ in range(2)]
        K.linear_group_forward(xh, [_group_operands(gate.inner), _group_operands(up.inner)], v, gate.inner.q_format)
        h = torch.empty((T, m), dtype=x2.dtype, device=x.device)
        entry, signed = _hadamard_entry(gate, "glu_rows")
        signs = dict(sign_g=gate.sign_out, sign_u=up.sign_out) if signed else {}
        entry(v[0], v[1], h, n_in=pr, n_out=m, P=pr, bias_g=gate.bias, bias_u=up.bias, act=act, **signs)
        return _like_input(h, x, m)
