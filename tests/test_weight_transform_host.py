"""The weight transform's host side, no GPU: cq_hadamard_cols' additive ABI and refusals, the Python layer's errors."""
import ctypes

import pytest
import torch

from ee274_convexcaldera_llm_quantization_amd import _lib as K
from ee274_convexcaldera_llm_quantization_amd import model as M
from test_abi_and_api_host import _struct_fields


def _args(**kw):
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    a = K.HadamardColsArgs(base, 12, base + (1 << 15), 12, 10, 60, 64, 64, None, None)
    a._buf = buf
    for key, v in kw.items():
        setattr(a, key, v)
    return a, base


def test_the_abi_is_additive_and_the_entry_validates_without_a_device():
    lib = K.load()
    assert [f for f, _ in K.HadamardColsArgs._fields_] == _struct_fields("cq_hadamard_cols_args")
    assert ctypes.sizeof(K.HadamardColsArgs) == 72 and K.HadamardColsArgs.sign_in.offset == 56
    assert {"cq_hadamard_cols", "cq_hadamard_cols_workspace"} <= set(K.EXPORTS) and lib.cq_abi_version() == 5
    assert lib.cq_hadamard_cols(None, None, 0, None) == K.CQ_EINVAL
    for kw, word in ((dict(P=48), "power of two"), (dict(P=0), "power of two"), (dict(P=65536, n_in=1), "power of two"),
                     (dict(n_in=0), "n_in"), (dict(n_in=65), "n_in"), (dict(n_out=0), "n_out"), (dict(n_out=65), "n_out"),
                     (dict(cols=-1), "cols"), (dict(ldx=9), "leading dimension"), (dict(ldy=9), "leading dimension"),
                     (dict(x=None), "null x or y"), (dict(y=None), "null x or y")):
        a, base = _args(**kw)
        assert lib.cq_hadamard_cols(ctypes.byref(a), None, 0, None) == K.CQ_EINVAL, kw
        msg = lib.cq_last_error().decode()
        assert word in msg and "cq_hadamard_cols" in msg, (kw, msg)
    for kw, word in ((dict(x=2), "x is not aligned"), (dict(y=1), "y is not aligned"), (dict(y=64 - (1 << 15)), "x and y overlap")):
        a, _ = _args()
        for key, off in kw.items():
            setattr(a, key, getattr(a, key) + off)
        assert lib.cq_hadamard_cols(ctypes.byref(a), None, 0, None) == K.CQ_EINVAL, kw
        assert word in lib.cq_last_error().decode(), (kw, lib.cq_last_error())
    a, _ = _args(cols=0)
    assert lib.cq_hadamard_cols(ctypes.byref(a), None, 0, None) == 0            # no launch, no device needed
    assert lib.cq_hadamard_cols_workspace(ctypes.byref(_args(P=256)[0])) == 0   # one pass: no workspace
    a, _ = _args(P=512, n_in=8, n_out=8)
    assert lib.cq_hadamard_cols_workspace(ctypes.byref(a)) == 512 * 10 * 4
    assert lib.cq_hadamard_cols(ctypes.byref(a), None, 0, None) == K.CQ_EWORKSPACE
    assert lib.cq_hadamard_cols(ctypes.byref(a), a.x, 512 * 10 * 4 - 1, None) == K.CQ_EWORKSPACE
    assert lib.cq_hadamard_cols(ctypes.byref(a), a.y - 64, 20480, None) == K.CQ_EINVAL and b"workspace overlaps" in lib.cq_last_error()


def test_the_python_layer_raises_the_documented_errors():
    x, y = torch.zeros(60, 10), torch.zeros(64, 10)
    a = K.hadamard_cols_args(x, y, n_in=60, n_out=64, P=64, sign_in=torch.ones(64, dtype=torch.int8))
    assert (a.ldx, a.ldy, a.cols, a.n_in, a.n_out, a.P) == (10, 10, 10, 60, 64, 64) and a.sign_in and not a.sign_out
    for kw, word in ((dict(P=48), "power of two"), (dict(n_in=59), r"x \(60, 10\)"), (dict(sign_out=torch.ones(64)), "int8"),
                     (dict(sign_in=torch.ones(59, dtype=torch.int8)), "59")):
        with pytest.raises(ValueError, match="cq_hadamard_cols: .*" + word):
            K.hadamard_cols_args(x, y, **{**dict(n_in=60, n_out=64, P=64), **kw})
    with pytest.raises(RuntimeError, match="HIP"):
        K.hadamard_cols(x, y, n_in=60, n_out=64, P=64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.hadamard_transform(torch.zeros(12, 40), kernels=True)
    nothing = dict(decompose=lambda *a: pytest.fail("decomposed"), device="cpu")
    big = torch.nn.ModuleDict({"language_q_proj": torch.nn.Linear(K.HADAMARD_MAX_N + 1, 1, bias=False, device="meta")})
    with pytest.raises(ValueError, match="hadamard_kernels=True needs hadamard=True or packed_hadamard=True"):
        M.apply_caldera_quantization(big, None, M.driver_params(), hadamard_kernels=True, **nothing)
    with pytest.raises(ValueError, match="hadamard_kernels=True: .*exceeds 32768"):
        M.apply_caldera_quantization(big, None, M.driver_params(), hadamard=True, hadamard_kernels=True,
                                     selection=M.LayerSelection(layers=None, min_dim=0), **nothing)
