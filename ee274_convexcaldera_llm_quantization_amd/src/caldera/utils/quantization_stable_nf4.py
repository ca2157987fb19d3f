"""Drop-in for RCR/src/caldera/utils/quantization_stable_nf4.py (QuantizerFactory /
LowMemoryQuantizer with the standardised NF4 / NF2 quantiser).

Same names, constructor arguments, return layouts and exceptions as the reference
(quantization_stable_nf4.py:5-261): nf4 / nf2 standardise a block, z = (x - mean) / std with the
unbiased std floored at epsilon, and carry the pair (mean, std) as parameters instead of the one
absmax scale of quantization.py.  The arithmetic runs in libcaldera_hip.so on the HIP device
(cq_quantize_nf_std / cq_dequant_nf_std; "uniform" is the uniform path of quantization.py).  A CPU
tensor is quantised on the current HIP device and the results are returned on the CPU; without a
HIP device the call raises (there is no CPU fallback).

Deviation: a block of one element has no unbiased std; the reference returns NaN parameters
there, this module raises ValueError.

`nf_variant = "standardized"` on the factory and the quantiser tells the engine
(EngineParams.from_caldera_params) which NF quantiser a factory with method nf4 / nf2 stands for.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import List

import torch

from ._engine_import import kernels as _K

_BITWIDTHS = [2, 4, 8, 16]
_QUANTIZER_METHODS = ["uniform", "nf4", "nf2"]


class AbstractQuantizer(ABC):
    @abstractmethod
    def quantize_block(self, weight): ...

    @abstractmethod
    def dequantize_block(self, weight_quant, weight_params, weight_shape): ...


def _to_device(t: torch.Tensor):
    if t.is_cuda:
        return t, None
    if not torch.cuda.is_available():
        raise RuntimeError("caldera-mi355x: no HIP device available (this engine has no CPU path)")
    return t.to(torch.device("cuda", torch.cuda.current_device())), t.device


class LowMemoryQuantizer(AbstractQuantizer):
    """quantization_stable_nf4.py:17-230.  Codes and parameters have the reference's shapes and
    dtypes: nf4 / nf2 return (idx (nblk, bs) uint8, (mean (nblk, 1), std (nblk, 1)) fp32, shape)."""

    nf_variant = "standardized"

    def __init__(self, num_bits: int = 2, method: str = "uniform", block_size: int = 64):
        self.num_bits = num_bits
        assert self.num_bits in _BITWIDTHS, "Bit-width not supported!"
        self.method = method.lower()
        if self.method not in _QUANTIZER_METHODS:
            raise NotImplementedError(f"Quantization method '{self.method}' not supported yet.")
        self.block_size = block_size
        if self.method == "nf4" and self.num_bits != 4:
            raise ValueError("NF4 quantization supports only 4 bits.")
        if self.method == "nf2" and self.num_bits != 2:
            raise ValueError("NF2 quantization supports only 2 bits.")

    def quantize_block(self, weight: torch.Tensor, epsilon: float = 1e-8):
        if len(weight.shape) != 2:
            raise ValueError(
                f"Support only for 2D matrix, but your input has {len(weight.shape)} dimensions."
            )
        total = weight.shape[0] * weight.shape[1]
        if total % self.block_size != 0:
            raise ValueError(
                f"Weight with shape {weight.shape[0]} x {weight.shape[1]} "
                f"is not divisible by block size {self.block_size}"
            )
        bs = self.block_size
        if self.method != "uniform" and bs < 2:
            raise ValueError(f"{self.method}: block size {bs} has no unbiased std (the reference returns NaN)")
        x, home = _to_device(weight)
        x = x.detach().to(torch.float32).contiguous().view(1, total)

        def back(t):
            return t.to(home) if home is not None else t

        if self.method == "uniform":
            out = _K.quantize_uniform(x, bs, self.num_bits, epsilon, codes=True, deq=False)
            return back(out["codes"].view(-1, bs)), back(out["scale"].view(-1, 1)), weight.shape
        out = _K.quantize_nf_std(x, bs, self.num_bits, epsilon, idx=True, deq=False)
        params = (back(out["mean"].view(-1, 1)), back(out["std"].view(-1, 1)))
        return back(out["idx"].view(-1, bs)), params, weight.shape

    def dequantize_block(self, weight_quant: torch.Tensor, weight_params, weight_shape: List[int]):
        c, home = _to_device(weight_quant)
        c = c.contiguous()
        if self.method == "uniform":
            s, _ = _to_device(weight_params)
            out = _K.dequantize_uniform(c, s.contiguous().float(), self.num_bits)
        elif self.method in ("nf4", "nf2"):
            mean, std = (_to_device(t)[0].contiguous().float() for t in weight_params)
            out = _K.dequantize_nf_std(c.to(torch.uint8), mean, std, self.num_bits)
        else:
            raise NotImplementedError(f"Dequantization method '{self.method}' not implemented.")
        out = out.view(-1).reshape(weight_shape)
        return out.to(home) if home is not None else out


class QuantizerFactory:
    nf_variant = "standardized"

    def __init__(self, method="uniform", block_size=64):
        self.method = method
        self.block_size = block_size

    def get_quantizer(self, num_bits, device="cpu"):
        return LowMemoryQuantizer(num_bits=num_bits, method=self.method, block_size=self.block_size)

    def __str__(self):
        return f"QuantizerFactory(method={self.method}, block_size={self.block_size})"
