"""CalderaLinear: an `nn.Linear` replacement that runs y = x (gs (Q + L R))^T (+ bias) from
the compressed form -- packed 2/4-bit codes, one scale, fp16 rank-r factors, a global scale
-- through cq_linear_forward (csrc/cq_linear.hip), never forming the dense weight.  A 4096^2
layer at 2-bit and r = 128 holds 4 MB of codes and 2 MB of factors where the dense fp16
weight `model.apply_caldera_quantization` writes back by default holds 32 MB.

The codes are kept in the inference layout of include/caldera_hip.h (rows padded to 16
bytes with code 0); the storage layout of `engine.last_packed` / `sharding.MatrixResult` is
converted once at construction with torch ops (not on the hot path).
"""
from __future__ import annotations

import torch

from . import _lib as K

SUPPORTED_BITS = (2, 4)


def _k(bits: int) -> int:
    return 2 ** (bits - 1) - 1


def _check_bits(bits):
    if bits not in SUPPORTED_BITS:
        raise ValueError(f"CalderaLinear: Q bits {bits} not in {SUPPORTED_BITS} (no packed codes)")


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


class CalderaLinear(torch.nn.Module):
    """One compressed layer.  Buffers (so `state_dict()` carries them): `codes` (out_features,
    row_bytes) uint8 inference layout, `L` (out_features, rank) and `R` (rank, in_features) fp16,
    `bias` (out_features,) fp32 or None.  Plain attributes: qscale, gscale, bits, in_features,
    out_features, rank (also carried as the state dict's extra state).

    forward(x): any leading dimensions, last = in_features, on a HIP device (there is no CPU
    path).  x is cast to fp16 and the result returned in x's dtype: bf16 activations beyond
    fp16's range (|x| > 65504) would overflow, as would |x R^T|."""

    def __init__(self, codes, L, R, bias=None, *, qscale, gscale, bits, in_features, out_features):
        super().__init__()
        _check_bits(bits)
        m, n = int(out_features), int(in_features)
        if codes.dtype != torch.uint8 or tuple(codes.shape) != (m, row_bytes(n, bits)):
            raise ValueError(f"CalderaLinear: codes must be uint8 {(m, row_bytes(n, bits))} (inference layout), "
                             f"got {codes.dtype} {tuple(codes.shape)}")
        r = 0 if L is None else int(L.shape[1])
        if r > K.LINEAR_MAX_RANK:
            raise ValueError(f"CalderaLinear: rank {r} > {K.LINEAR_MAX_RANK}")
        dev = codes.device
        if r == 0:
            L, R = torch.zeros((m, 0), device=dev), torch.zeros((0, n), device=dev)
        if tuple(L.shape) != (m, r) or tuple(R.shape) != (r, n):
            raise ValueError(f"CalderaLinear: L {tuple(L.shape)} / R {tuple(R.shape)} do not fit {(m, r)} / {(r, n)}")
        self.in_features, self.out_features, self.rank, self.bits = n, m, r, int(bits)
        self.qscale, self.gscale = float(qscale), float(gscale)
        self.register_buffer("codes", codes.contiguous())
        self.register_buffer("L", L.detach().to(torch.float16).contiguous())
        self.register_buffer("R", R.detach().to(torch.float16).contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).contiguous())

    def _apply(self, fn, *args, **kwargs):
        """Moves follow the model (`.to(device)`, `.cuda()`); dtype casts do not: `model.half()` or
        `.to(torch.bfloat16)` leave the codes, the fp16 factors and the fp32 bias as stored (the
        kernel's operand types; a cast would only lose bits), forward returns x's dtype anyway."""
        def keep_dtype(t):
            out = fn(t)
            return out if out.dtype == t.dtype else t.to(out.device)
        return super()._apply(keep_dtype, *args, **kwargs)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_codes(cls, c, L, R, bias=None, *, qscale, gscale, bits):
        """From (m, n) integer codes in [-k, k]."""
        _check_bits(bits)
        m, n = c.shape
        return cls(pack_rows(c, bits), L, R, bias, qscale=qscale, gscale=gscale, bits=bits, in_features=n,
                   out_features=m)

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
        c = unpack_bytes(flat, res.Q_bits).view(m, npad)[:, :n]
        return cls.from_codes(c, res.L, res.R[:, :n], bias, qscale=res.Q_scale, gscale=res.global_scale,
                              bits=res.Q_bits)

    @classmethod
    def from_decomposition(cls, dec, Q_bits, bias=None):
        """From a CalderaDecomposition with uniform Q: packs `Q_idxs` (the reference's int codes,
        (1, m n)) with `Q_scale`; L, R are rounded to fp16."""
        _check_bits(Q_bits)
        if dec.Q_idxs is None or dec.Q is None:
            raise ValueError("CalderaLinear.from_decomposition: the decomposition has no Q")
        qs = dec.Q_scale
        if (not torch.is_tensor(dec.Q_idxs) or dec.Q_idxs.dtype != torch.int8
                or (torch.is_tensor(qs) and qs.numel() != 1) or isinstance(qs, (tuple, list, dict))):
            raise ValueError("CalderaLinear.from_decomposition: Q is not uniformly quantised with one scale "
                             "(nf / bbint codebooks have no packed codes)")
        m, n = dec.Q.shape
        if dec.Q_idxs.numel() != m * n:
            raise ValueError("CalderaLinear.from_decomposition: Q_idxs does not hold m x n codes")
        qscale = float(qs.reshape(-1)[0]) if torch.is_tensor(qs) else float(qs)
        return cls.from_codes(dec.Q_idxs.reshape(m, n), dec.L, dec.R, bias, qscale=qscale,
                              gscale=float(dec.global_scale), bits=Q_bits)

    def to_result(self, name: str):
        """The layer as a `sharding.MatrixResult` (storage layout: codes on the (m, n padded to
        4) grid, fp32 factors), e.g. for `sharding.save_results`; `from_result` inverts it."""
        from .sharding import MatrixResult
        m, n, per = self.out_features, self.in_features, 8 // self.bits
        npad = n + (-n) % 4
        codes = self.codes[:, :npad // per].contiguous().reshape(-1)
        extra = {"n_padded": npad} if npad != n else {}
        return MatrixResult(name, m, n, self.rank, self.bits, codes, self.qscale, self.L.float(), self.R.float(),
                            self.gscale, {}, extra)

    # ------------------------------------------------------------------ state
    def get_extra_state(self):
        return {"qscale": self.qscale, "gscale": self.gscale, "bits": self.bits, "in_features": self.in_features,
                "out_features": self.out_features, "rank": self.rank}

    def set_extra_state(self, state):
        for key, v in state.items():
            setattr(self, key, v)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bits={self.bits}, "
                f"rank={self.rank}, bias={self.bias is not None}")

    def packed_bytes(self) -> int:
        """Bytes a forward streams for the weights: codes + L + R (+ bias)."""
        return sum(t.numel() * t.element_size() for t in (self.codes, self.L, self.R, self.bias) if t is not None)

    def dense_weight(self) -> torch.Tensor:
        """gs (Q + L R) as a dense fp32 (out_features, in_features) tensor, by torch ops (checks
        and baselines only): Q = c (s / k)."""
        k = _k(self.bits)
        c = unpack_bytes(self.codes, self.bits)[:, :self.in_features].float()
        sk = (torch.tensor(self.qscale, dtype=torch.float32) / torch.tensor(float(k), dtype=torch.float32)).item()
        return self.gscale * (c * sk + self.L.float() @ self.R.float())

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda or not self.codes.is_cuda:
            raise RuntimeError("CalderaLinear needs HIP device tensors (no CPU fallback)")
        if x.shape[-1] != self.in_features:
            raise ValueError(f"CalderaLinear: last dimension {x.shape[-1]} != in_features {self.in_features}")
        x2 = x.reshape(-1, self.in_features).to(torch.float16)
        if x2.stride(1) != 1:
            x2 = x2.contiguous()
        ydt = x.dtype if x.dtype in (torch.float16, torch.float32) else torch.float32
        y = torch.empty((x2.shape[0], self.out_features), dtype=ydt, device=x.device)
        K.linear_forward(x2, self.codes, self.qscale, self.gscale, self.L if self.rank else None,
                         self.R if self.rank else None, self.bias, y, m=self.out_features, n=self.in_features,
                         bits=self.bits)
        return y.to(x.dtype).reshape(*x.shape[:-1], self.out_features)
