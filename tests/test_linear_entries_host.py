"""The five forward entries of the packed linear layer share their host code (csrc/cq_linear.hip); what
they do before any launch is the same for each: tokens = 0 is CQ_OK with nothing done, whatever the
workspace, and a missing workspace at r > 0 is CQ_EINVAL.  No device is needed: neither case launches."""
import ctypes

import pytest
import torch

import ee274_convexcaldera_llm_quantization_amd._lib as K


def _member(p, base, tokens, with_y=True):
    """A valid 4-bit layer with fp16 factors of rank 8 on host memory, into the packed struct p."""
    p.x, p.ldx, p.tokens, p.m, p.n, p.r, p.bits = base, 64, tokens, 16, 64, 8, 4
    p.codes, p.code_stride, p.qscale, p.gscale = base + 256, 32, 1.0, 1.0
    p.L, p.ldl, p.R, p.ldr = base + 2048, 8, base + 3072, 64
    if with_y:
        p.y, p.y_dtype, p.ldy = base + 8192, K.CQ_F32, 16
    if hasattr(p, "l_bits"):
        p.l_bits = p.r_bits = 16


def _single(base, tokens):
    a = K.LinearArgs()
    _member(a, base, tokens)
    return a


def _packed(base, tokens):
    a = K.LinearPackedArgs()
    _member(a, base, tokens)
    return a


def _codebook(base, tokens):
    a = K.LinearCodebookArgs()
    _member(a.p, base, tokens)
    a.q_format = K.QFMT_NF
    return a


def _group(base, tokens):
    arr = (K.LinearPackedArgs * 2)()
    for p in arr:
        _member(p, base, tokens)
    g = K.LinearGroupArgs()
    g.count, g.q_format = 2, K.QFMT_UNIFORM
    g.members = ctypes.cast(arr, ctypes.POINTER(K.LinearPackedArgs))
    g._keep = arr
    return g


def _glu(base, tokens):
    a = K.LinearGluArgs()
    for p in (a.gate, a.up):
        _member(p, base, tokens, with_y=False)
    a.q_format, a.act = K.QFMT_UNIFORM, K.ACT_SILU
    a.h, a.h_dtype, a.ldh = base + 16384, K.CQ_F32, 16
    return a


ENTRIES = {"cq_linear": _single, "cq_linear_packed": _packed, "cq_linear_codebook": _codebook,
           "cq_linear_group": _group, "cq_linear_glu": _glu}


@pytest.mark.parametrize("name", ENTRIES)
def test_forward_entry_with_no_tokens_or_no_workspace(name):
    lib = K.load()
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 15) // 16 * 16
    forward, workspace = getattr(lib, name + "_forward"), getattr(lib, name + "_workspace")
    a = ENTRIES[name](base, 0)
    assert workspace(ctypes.byref(a)) == 0
    assert forward(ctypes.byref(a), None, 0, None) == 0                # CQ_OK
    assert forward(ctypes.byref(a), base + 1, 0, None) == 0            # the workspace is not looked at
    a = ENTRIES[name](base, 1)
    need = workspace(ctypes.byref(a))
    assert need > 0
    assert forward(ctypes.byref(a), None, need, None) == K.CQ_EINVAL
    assert name + "_forward: workspace must be 16-byte aligned" in lib.cq_last_error().decode()
    assert forward(ctypes.byref(a), base + 8, need, None) == K.CQ_EINVAL
    assert "workspace" in lib.cq_last_error().decode()
