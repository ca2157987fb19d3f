"""The rank-r solver's host-side decisions (solver.py), on CPU tensors and numpy: the layout of
an outer iteration's read-back, the per-matrix stall rule, the frozen set's snapshot, refill and
retake rule, and the probe's context manager.  No device calls."""
import numpy as np
import torch

from ee274_convexcaldera_llm_quantization_amd import solver as S


def test_check_round_trip_and_layout():
    B, p = 4, 6
    theta = torch.arange(B * p, dtype=torch.float64).reshape(B, p) + 0.5
    res = torch.tensor([1e-3, 2e-4, float("inf"), 5e-7], dtype=torch.float64)
    ovf = torch.tensor(3, dtype=torch.int32).double()
    unconv = torch.tensor([2.0], dtype=torch.float64)
    chk = S._pack_check(ovf, theta, res, unconv)
    # overflow, theta[:, 0], theta[:, p - 1], resid, unconv
    assert chk.dtype == torch.float64 and chk.shape == (3 * B + 2,)
    want = [3.0] + [0.5, 6.5, 12.5, 18.5] + [5.5, 11.5, 17.5, 23.5] + [1e-3, 2e-4, float("inf"), 5e-7] + [2.0]
    assert chk.tolist() == want
    c = S._unpack_check(chk, B)
    assert c.overflow == 3.0 and c.n_unconv == 2 and isinstance(c.n_unconv, int)
    for got, exp in ((c.top, theta[:, 0]), (c.bottom, theta[:, p - 1]), (c.resid, res)):
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (B,)
        assert np.array_equal(got, exp.numpy())
    zero = S._unpack_check(S._pack_check(torch.zeros((), dtype=torch.float64), theta, res, 0 * unconv), B)
    assert zero.overflow == 0 and zero.n_unconv == 0


def test_new_stalls():
    tol = 1e-5
    inf = np.inf
    none = np.zeros(5, dtype=bool)
    # matrix: 0 converging, 1 flat above tol, 2 flat below tol, 3 cheap iterations only before
    # (no finite best-before), 4 flat above tol but already stalled
    h0 = np.array([1e-2, 1e-4, 4e-6, inf, 1e-4])
    h1 = np.array([1e-3, 9.95e-5, 4e-6, inf, 1e-4])
    h2 = np.array([1e-4, 9.9e-5, 4e-6, 1e-4, 1e-4])
    already = np.array([False, False, False, False, True])
    for hist in ([], [h0], [h0, h1]):   # fewer than three entries: nothing
        assert not S._new_stalls(hist, h1, none, tol).any()
    got = S._new_stalls([h0, h1, h2], h2, already, tol)
    assert got.dtype == bool and got.tolist() == [False, True, False, False, False]
    assert S._new_stalls([h0, h1, h2], h2, none, tol).tolist() == [False, True, False, False, True]
    # four iterations: best of the last two against the best of the two before them
    h3 = np.array([1e-5 * 2, 9.85e-5, 4e-6, 9.9e-5, 9.7e-5])
    #   0: 2e-5 vs 1e-3 -> converging;  1: 9.85e-5 > 0.98 * 9.95e-5 -> stalls;  2: below tol
    #   3: before = min(inf, inf) -> never;  4: 9.7e-5 <= 0.98 * 1e-4 -> still improving
    assert S._new_stalls([h0, h1, h2, h3], h3, none, tol).tolist() == [False, True, False, False, False]
    # exactly at the ratio is not a stall (strictly above STALL_RATIO x best-before)
    a, b = np.array([1.0]), np.array([S.STALL_RATIO])
    assert S.STALL_RATIO == 0.98 and not S._new_stalls([a, b, b], b, np.zeros(1, dtype=bool), tol).any()
    # a matrix whose every entry is inf (cheap iterations only)
    c = np.array([inf])
    assert not S._new_stalls([c, c, c, c], c, np.zeros(1, dtype=bool), tol).any()


def _state(B, k, p, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, k, p, generator=g)
    Z = torch.randn(B, k, p, generator=g)
    theta = torch.randn(B, p, generator=g, dtype=torch.float64)
    ends = theta[:, [0, p - 1]].numpy().copy()
    resid = torch.rand(B, generator=g, dtype=torch.float64).numpy()
    return X, Z, theta, ends, resid


def test_frozen_take_restore():
    B, k, p = 5, 7, 4
    X, Z, theta, ends, resid = _state(B, k, p, 1)
    live = np.array([True, False, True, False, False])
    fr = S._Frozen.take(live, X, Z, theta, ends, resid, "cpu")
    assert fr.mask.tolist() == [False, True, False, True, True] and fr.index.tolist() == [1, 3, 4]
    # the snapshot owns its data: later changes of the state do not reach it
    keep = [t.clone() for t in (X, Z, theta)] + [ends.copy(), resid.copy()]
    for t in (X, Z, theta):
        t.add_(1.0)
    ends += 1.0
    resid += 1.0
    # the next iteration's results: other numbers everywhere
    Xn, Zn, theta_n, ends_n, resid_n = _state(B, k, p, 2)
    new = [t.clone() for t in (Xn, Zn, theta_n)]
    theta_in = theta_n
    chk = S._pack_check(torch.zeros((), dtype=torch.float64), theta_n, torch.from_numpy(resid_n),
                        torch.zeros(1, dtype=torch.float64))
    check = S._unpack_check(chk, B)
    theta_out = fr.restore(Xn, Zn, theta_n, check)
    assert theta_out is not theta_in and torch.equal(theta_in, new[2])      # out of place
    f, lv = fr.mask, ~fr.mask
    for got, old, fresh in ((Xn, keep[0], new[0]), (Zn, keep[1], new[1]), (theta_out, keep[2], new[2])):
        assert torch.equal(got[f], old[f]) and torch.equal(got[lv], fresh[lv])
    assert np.array_equal(check.top[f], keep[3][f, 0]) and np.array_equal(check.top[lv], ends_n[lv, 0])
    assert np.array_equal(check.bottom[f], keep[3][f, 1]) and np.array_equal(check.bottom[lv], ends_n[lv, 1])
    assert np.array_equal(check.resid[f], keep[4][f]) and np.array_equal(check.resid[lv], resid_n[lv])
    assert check.overflow == 0 and check.n_unconv == 0


def test_frozen_update_rules():
    B, k, p = 4, 6, 4
    st = _state(B, k, p, 3)

    def upd(fr, live):
        return S._Frozen.update(fr, np.array(live), *st, "cpu")

    assert upd(None, [True] * B) is None                     # nothing frozen yet
    a = upd(None, [True, False, True, True])                 # first frozen matrix: snapshot
    assert a is not None and a.mask.tolist() == [False, True, False, False]
    b = upd(a, [True, False, False, True])                   # the set grew: a new snapshot
    assert b is not a and b.mask.tolist() == [False, True, True, False] and b.index.tolist() == [1, 2]
    assert upd(b, [True, False, False, True]) is b           # the same set: kept
    c = upd(b, [True, True, False, True])                    # a matrix came back: retaken
    assert c is not b and c.mask.tolist() == [False, False, True, False]
    assert upd(c, [True] * B) is None                        # a refinement reopened all: dropped


def test_group_probe_timed_off_and_on():
    pr = S._GroupProbe()
    ran = []
    with pr.timed("kind", 1.0, 2.0):    # off: no event exists, nothing is recorded
        ran.append(1)
    assert ran == [1] and pr.meta == [] and pr.summary() == {}

    class Ev:
        def __init__(self):
            self.n = 0

        def record(self):
            self.n += 1
            order.append(self)

    order = []
    pr.on, pr.pool, pr.meta = True, [(Ev(), Ev())], []
    with pr.timed("kind", 1.0, 2.0):
        order.append("body")
    a, b = pr.pool[0]
    assert order == [a, "body", b] and pr.meta == [("kind", 1.0, 2.0)]
    with pr.timed("kind", 1.0, 2.0):    # the pool is full: the body alone
        order.append("body2")
    assert order == [a, "body", b, "body2"] and (a.n, b.n) == (1, 1) and len(pr.meta) == 1
