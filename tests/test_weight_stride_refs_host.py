"""The references of tests/weight_stride_cases.py, checked on the host (no GPU):

* discrimination: for every case and every pair b != b', the reference of matrix b evaluated
  with matrix b''s weight row differs from the one evaluated with its own row by at least 100
  times that output's bar (bit-exact outputs: in at least 1 % of the elements; a single value
  must differ).  A kernel that reads the wrong matrix's row therefore fails the fp64 assertion
  of tests/test_gpu_weight_strides.py instead of passing it within tolerance.  It depends on the
  inputs alone, so it is asserted here and the seeds are fixed so that it holds;
* a (B, n) weight array with B equal rows reproduces the shared (n,) reference exactly;
* the weights are positive and their rows differ in scale and in pattern."""
import numpy as np
import pytest

import weight_stride_cases as C

IDS = C.ids()


def test_weights_are_positive_and_rows_differ():
    w = C.weights(64, 5)
    assert w.shape == (C.B, 64) and w.dtype == np.float32 and (w > 0).all()
    for b in range(C.B):
        u = np.log10(w[b] / C.F[b])
        assert u.min() >= -2.0 - 1e-6 and u.max() <= 1.0 + 1e-6
        for b2 in range(b):
            assert abs(np.corrcoef(np.log(w[b]), np.log(w[b2]))[0, 1]) < 0.5


def test_pack_codes_layout():
    """Offset-binary, MSB-first: 2-bit codes (-1, 0, 1, 0) -> 0b00_01_10_01, 4-bit (-7, 7) -> 0x0e."""
    assert C.pack_codes(np.array([-1, 0, 1, 0]), 2).tolist() == [0b00011001]
    assert C.pack_codes(np.array([-7, 7, 0, 1]), 4).tolist() == [0x0E, 0x78]


@pytest.mark.parametrize("cid", IDS)
def test_wrong_row_is_100_bars_away(cid):
    c = C.case(cid)
    for b in range(C.B):
        own = c.ref(b, c.w[b])
        for b2 in range(C.B):
            if b2 == b:
                continue
            other = c.ref(b, c.w[b2])
            for name in c.weighted:
                tol = c.tol[name]
                d = C.differs(own[name], other[name], tol, own.get(name + "_bound"))
                need = 1.0 if tol is None else 100.0
                assert d >= need, (cid, b, b2, name, d)
            for name in set(own) - c.weighted:   # and nothing else moves with the weights
                if not name.endswith("_bound"):
                    assert np.array_equal(np.asarray(own[name]), np.asarray(other[name])), (cid, name)


@pytest.mark.parametrize("cid", IDS)
def test_equal_rows_reproduce_the_shared_reference(cid):
    c = C.case(cid)
    for b0 in (1,):
        tiled = c.ref_batch(np.tile(c.w[b0], (C.B, 1)))
        shared = c.ref_batch(c.w[b0])
        for t, s in zip(tiled, shared):
            assert set(t) == set(s)
            for name in t:
                assert np.array_equal(np.asarray(t[name]), np.asarray(s[name])), (cid, b0, name)


def test_codes_row_weights_discriminate():
    """cq_codes_matmul's roww (the m > n shapes): the same condition for the row weights."""
    for c in map(C.case, C.ids("codes")):
        for b in range(C.B):
            own = c.ref(b, c.w[b])
            for b2 in range(C.B):
                if b2 != b:
                    other = c.ref(b, c.w[b], roww=c.inp["roww"][b2])
                    for name in ("roww", "both"):
                        assert C.differs(own[name], other[name], "bound", own[name + "_bound"]) >= 100.0
