"""Cases and the fp64 reference of the packed linear layer's input gradient with coded factors
(include/caldera_hip.h, cq_linear_packed_backward_input):

    u~[t, q] = uscale * sum_i dy[t, i] lam[i, q]
    dx[t, j] = gs * ((s / k) * sum_i dy[t, i] c[i, j] + sum_q u~[t, q] rho[q, j])

lam is the L codes (lb 2 | 4) or the fp16 L (16), rho the R codes or the fp16 R; uscale is the fp32
product of the coded factors' scale / k (each one fp32 division).  Same pattern as
linear_backward_cases.py and linear_factor_cases.py, whose helpers are used here: host-seeded
numpy, the reference evaluated in fp64 from the operands as the kernel sees them.

Formats: every (Q, L, R) with Q in {2, 4}, L, R in {2, 4, 16} and at least one coded factor (16
combinations).  Shapes (m, n, r):

    (33, 64, 8)      unaligned dy rows; r below one 16-code piece
    (48, 198, 40)    n, r ragged; the L-code piece 32..47 straddles r            (every combination)
    (80, 898, 200)   two 128-column tiles of u; r not a multiple of 32; storage / inference strides differ
    (272, 512, 16)   9 row chunks: the ring wraps                                 (also T = 130)
    (160, 256, 128)  every mask-free loop runs on coded L (tile condition r >= 113; T = 64: 64 whole
                     tokens per workgroup of the u product) and on coded R (4 row chunks; T = 130: 128
                     whole tokens of the main kernel)                (every combination, also T = 130)
    (198, 48, 0)     codes only

T in {1, 5, 17, 64}.  Every shape meets (Q, L, R) = (2, 4, 4) and (2, 2, 2) at every T; the second
and the fifth meet the other 14 combinations at two T each.

Every case's coded operands are hostile: an L-code row's tail (columns r ..) holds random nonzero
codes (`ltail`), and the R codes are followed by 32 ceil(r / 32) - r more rows of random bytes
(`rrows`), which a 32-row chunk reaches.  Neither may change anything.

Exact cases: dy in -4..4, codes in -k..k, an fp16 factor in -2..2, s = k / 2, s_L = k_L / 2,
s_R = k_R / 2 (every scale / k is 0.5, uscale 0.25 or 0.5), gs = 4.  Every term is a multiple of
0.25; test_linear_packed_backward_host.py asserts on the case data that for every output the sum of
the absolute terms, the |hi| + |lo| of u~'s split included, stays below 2^24 such units and that u~
splits exactly into fp16 halves, so any summation order is exact and dx and u_out must match bit
for bit.  "exact16": (33, 64, 8) with dy in -1..1, so |dx| <= 2048 and fp16 dx must equal it too.

Random cases: dy ~ N(0, 1), random codes, s = 0.05, s_L = s_R = 0.3, gs = 1.7, an fp16 factor
~ 0.15 N(0, 1), with linear_backward_cases.py's elementwise worst-case bars on the dequantised
factors:

    |dx - dx64| <= (m + r + 32) 2^-24 A,   A = gs ((s / k) |dy| |c| + uscale |dy| |lam| |rho|)
    |u~ - u64|  <= (m + 8) 2^-24 uscale |dy| |lam|

The one rounding this entry adds (uscale on the complete u sum) is inside the 8 and the 32, which
counted 1 + 4 + 1 + 1 roundings beside the sums' (s / k, the split, the sum of both terms, gs).
dy[0, 0], dy[0, m - 1] and (T > 1) dy[1, 0] carry the largest magnitude of the case's dy.

Planted faults (`reference(case, fault)`), beside linear_backward_cases.py's, which act here on c,
lam and rho in the same way: "drop_uscale"; "lscale_for_lk" / "rscale_for_rk" (the scale where
scale / k belongs; 4 bits only: k = 1 at 2); "flip_L" / "flip_R" one factor code, moved to the
farthest code; "tr_block_R" the first 16 x 16 block of the R codes left untransposed; "L_tail" the
L-code tail read as real codes: u~'s pad columns r .. 16 ceil(r / 16) come from `ltail` and meet
R's last row (a clamped row load); "R_rows" R's rows >= r not zeroed: those pad columns of u~ meet
the rows `rrows` instead.  The last two need a piece of L codes that straddles r (r not a multiple
of 16), "R_rows" also coded R.

Which faults a random case must show (`fault_applies`) follows linear_backward_cases.py: a fault
in a bounded number of rows is small against a bar that grows with m (1 + r), so the row-local ones
are claimed where m (r + 1) <= ROW_LOCAL_LIMIT (that module's 25 000, which holds every shape
here) and the scale faults everywhere.  "flip_R" moves dx[t, 0] by one u~[t, 0] times the code's
step: a random-sign sum of m terms that no planted dy enlarges, against a bar that grows like
m (1 + r); a numpy run gave 5.6 and 6.2 bars at 2-bit R and T = 1 on (160, 256, 128) and
(80, 898, 200), and >= 50 on the other shapes, so it is claimed up to m (r + 1) = FLIP_R_LIMIT.
The smallest measured value of any claimed pair is stated in test_linear_packed_backward_host.py.
"""
from dataclasses import dataclass

import numpy as np

import linear_backward_cases as BC
from linear_cases import f16, f32, f64, inference_codes, pack_codes, row_bytes  # noqa: F401  (re-exported)

CHUNK_ROWS = BC.CHUNK_ROWS
ROW_LOCAL_LIMIT = BC.ROW_LOCAL_LIMIT  # m (r + 1) up to which a row-local fault is claimed on a random case
FLIP_R_LIMIT = 5000                   # ... "flip_R"


@dataclass(frozen=True)
class Case:
    kind: str       # "exact" | "exact16" | "random"
    m: int
    n: int
    r: int
    bits: int       # Q
    lb: int         # L: 2 | 4 | 16
    rb: int         # R
    T: int

    @property
    def id(self):
        return f"{self.kind}-m{self.m}n{self.n}r{self.r}b{self.bits}L{self.lb}R{self.rb}T{self.T}"

    @property
    def k(self):
        return 2 ** (self.bits - 1) - 1

    @property
    def kl(self):
        return 2 ** (self.lb - 1) - 1 if self.lb != 16 else None

    @property
    def kr(self):
        return 2 ** (self.rb - 1) - 1 if self.rb != 16 else None

    @property
    def r16(self):
        """End of the last 16-column piece of L codes that starts inside r."""
        return -(-self.r // 16) * 16

    @property
    def r32(self):
        return -(-self.r // 32) * 32

    @property
    def seed(self):
        return (self.m * 1000003 + self.n * 1009 + self.r * 101 + self.bits * 11 + self.lb * 307 + self.rb * 701
                + self.T + {"exact": 0, "exact16": 1, "random": 2}[self.kind] * 7919 + 40507)


SHAPES = ((33, 64, 8), (48, 198, 40), (80, 898, 200), (272, 512, 16), (160, 256, 128), (198, 48, 0))
ALIGNED = ((272, 512, 16), (160, 256, 128))
TOKENS = (1, 5, 17, 64)
COMBOS = tuple((q, lb, rb) for q in (2, 4) for lb in (2, 4, 16) for rb in (2, 4, 16) if (lb, rb) != (16, 16))


def _shapes():
    out = []
    for shp in SHAPES:                           # every shape meets (2, 4, 4) and (2, 2, 2)
        for T in TOKENS + ((130,) if shp in ALIGNED else ()):
            out.append((*shp, 2, 4, 4, T))
            out.append((*shp, 2, 2, 2, T))
    for shp, Ts in (((48, 198, 40), (17, 64)), ((160, 256, 128), (64, 130))):  # every other combination
        for combo in COMBOS:
            if combo not in ((2, 4, 4), (2, 2, 2)):
                out += [(*shp, *combo, T) for T in Ts]
    return out


EXACT = [Case("exact", *s) for s in _shapes()]
EXACT16 = [Case("exact16", 33, 64, 8, 2, lb, rb, T) for lb, rb in ((2, 2), (4, 16), (16, 4)) for T in (1, 5, 17)]
RANDOM = [Case("random", *s) for s in _shapes()]
ALL = EXACT + EXACT16 + RANDOM

_CACHE = {}


def inputs(case: Case):
    """dict(dy (T, m) f16, c (m, n) int8, lam (m, r) int8 codes | f16, rho (r, n) int8 codes | f16,
    s, sl, sr, gs (f32; sl / sr None for an fp16 factor), ltail (m, tail columns) int8 | None: the
    codes in the L rows' tails, rrows (r32 - r, R row bytes) uint8 | None: the bytes behind the R
    codes' last row); built once per case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    m, n, r, T = case.m, case.n, case.r, case.T
    c = rng.integers(-case.k, case.k + 1, (m, n)).astype(np.int8)
    random = case.kind == "random"

    def factor(bits, shape):
        if bits != 16:
            k = 2 ** (bits - 1) - 1
            return rng.integers(-k, k + 1, shape).astype(np.int8), f32(0.3) if random else f32(k / 2)
        if random:
            return (0.15 * rng.standard_normal(shape)).astype(f16), None
        return rng.integers(-2, 3, shape).astype(f16), None

    if random:
        dy = rng.standard_normal((T, m)).astype(f16)
        s, gs = f32(0.05), f32(1.7)
    else:
        da = 4 if case.kind == "exact" else 1
        dy = rng.integers(-da, da + 1, (T, m)).astype(f16)
        s, gs = f32(case.k / 2), f32(4.0)
    lam, sl = factor(case.lb, (m, r))
    rho, sr = factor(case.rb, (r, n))
    big = np.abs(dy.astype(f64)).max()
    for (t, i) in ((0, 0), (0, m - 1)) + (((1, 0),) if T > 1 else ()):
        dy[t, i] = f16(big if dy[t, i] >= 0 else -big)
    ltail = rrows = None
    if r and case.lb != 16:
        # nonzero codes (the tail's proper content is code 0) in every tail column of every row
        cols = row_bytes(r, case.lb) * 8 // case.lb - r
        ltail = rng.integers(1, case.kl + 1, (m, cols)).astype(np.int8) * rng.choice([-1, 1], (m, cols)).astype(np.int8)
    if r and case.rb != 16 and case.r32 > r:
        rrows = rng.integers(0, 256, (case.r32 - r, row_bytes(n, case.rb))).astype(np.uint8)
    out = dict(dy=dy, c=c, lam=lam, rho=rho, s=s, sl=sl, sr=sr, gs=gs, ltail=ltail, rrows=rrows)
    _CACHE[case] = out
    return out


def scales(case: Case, d=None):
    """(sk, uscale) as the kernel forms them: fp32 divisions, fp32 product."""
    d = inputs(case) if d is None else d
    sk = f32(d["s"] / f32(case.k))
    u = f32(1.0)
    if case.r and case.lb != 16:
        u = f32(d["sl"] / f32(case.kl))
    if case.r and case.rb != 16:
        skr = f32(d["sr"] / f32(case.kr))
        u = f32(u * skr) if case.lb != 16 else skr
    return sk, u


def unpack(b, bits):
    """uint8 (rows, nbytes) packed codes -> int8 (rows, nbytes * 8 / bits) codes in -k .. k + 1."""
    k, per = 2 ** (bits - 1) - 1, 8 // bits
    parts = [((b >> (bits * (per - 1 - i))) & (2 ** bits - 1)) for i in range(per)]
    return (np.stack(parts, axis=-1).reshape(b.shape[0], -1).astype(np.int16) - k).astype(np.int8)


def l_codes(case: Case):
    """The L operand as the entry takes it: (m, row bytes) uint8 with `ltail` in the rows' tails."""
    d = inputs(case)
    full = np.concatenate([d["lam"], d["ltail"]], axis=1)
    return pack_codes(full, case.lb).reshape(case.m, row_bytes(case.r, case.lb))


def r_codes(case: Case):
    """The R operand's buffer: (r32, row bytes) uint8 whose first r rows are the operand (tail = code
    0) and whose other rows hold `rrows`."""
    d = inputs(case)
    body = inference_codes(d["rho"], case.rb)
    return body if d["rrows"] is None else np.concatenate([body, d["rrows"]], axis=0)


GLOBAL_FAULTS = BC.GLOBAL_FAULTS + ("drop_uscale", "lscale_for_lk", "rscale_for_rk")
ROW_LOCAL_FAULTS = BC.ROW_LOCAL_FAULTS + ("flip_L", "flip_R", "tr_block_R", "L_tail", "R_rows")
FAULTS = ROW_LOCAL_FAULTS + GLOBAL_FAULTS


def fault_applies(case: Case, fault: str) -> bool:
    """Whether a planted fault exists for the case and, from its data's design, must show."""
    if case.kind == "exact16":
        return False
    if fault in ROW_LOCAL_FAULTS and case.kind == "random" and case.m * (case.r + 1) > ROW_LOCAL_LIMIT:
        return False   # see the module docstring
    if fault == "flip_R" and case.kind == "random" and case.m * (case.r + 1) > FLIP_R_LIMIT:
        return False
    if fault in ("swap_R", "drop_L_last", "drop_uscale"):
        return case.r > 0
    if fault == "s_for_sk":
        return case.bits == 4
    if fault == "pad_row":
        return case.m % CHUNK_ROWS != 0 and case.T > 1
    if fault in ("flip_L", "lscale_for_lk", "L_tail", "R_rows") and (case.lb == 16 or not case.r):
        return False
    if fault in ("flip_R", "rscale_for_rk", "tr_block_R", "R_rows") and (case.rb == 16 or not case.r):
        return False
    if fault == "lscale_for_lk":
        return case.lb == 4
    if fault == "rscale_for_rk":
        return case.rb == 4
    if fault in ("L_tail", "R_rows"):
        return case.r % 16 != 0
    return True


def reference(case: Case, fault: str | None = None):
    """(dx64 (T, n), u64 (T, r), bar, ubar): the fp64 reference (u64 is u~) and the elementwise bars
    of the random cases.  fault: one planted error (FAULTS), for checking that the cases can see it
    (the bars are then None)."""
    d = inputs(case)
    dy, c, lam, rho = (d[key].astype(f64) for key in ("dy", "c", "lam", "rho"))
    sk32, us32 = scales(case, d)
    sk, uscale, gs = f64(sk32), f64(us32), f64(d["gs"])
    m, r = case.m, case.r
    dyw = dy                    # dy as the products see it
    if fault == "flip_first":
        c[0, 0] = BC._flip(c[0, 0], case.k)
    elif fault == "flip_last":
        c[-1, -1] = BC._flip(c[-1, -1], case.k)
    elif fault == "tr_block":
        b = min(16, m, case.n)
        c[:b, :b] = c[:b, :b].T.copy()
    elif fault == "drop_last_rows":
        dyw = dy.copy()
        dyw[:, CHUNK_ROWS * ((m - 1) // CHUNK_ROWS):] = 0
    elif fault == "drop_gs":
        gs = f64(1.0)
    elif fault == "s_for_sk":
        sk = f64(d["s"])
    elif fault == "swap_R":
        rho[[0, 1]] = rho[[1, 0]]
    elif fault == "drop_L_last":
        lam[-1] = 0
    elif fault == "flip_L":
        lam[0, 0] = BC._flip(lam[0, 0], case.kl)
    elif fault == "flip_R":
        rho[0, 0] = BC._flip(rho[0, 0], case.kr)
    elif fault == "tr_block_R":
        b = min(16, r, case.n)
        rho[:b, :b] = rho[:b, :b].T.copy()
    elif fault == "drop_uscale":
        uscale = f64(1.0)
    elif fault == "lscale_for_lk":
        uscale = f64(f32(d["sl"]) * (f32(d["sr"] / f32(case.kr)) if case.rb != 16 else f32(1.0)))
    elif fault == "rscale_for_rk":
        uscale = f64((f32(d["sl"] / f32(case.kl)) if case.lb != 16 else f32(1.0)) * f32(d["sr"]))
    code = dyw @ c
    if fault == "pad_row":
        code[:-1, 0] += dy[1:, 0] * case.k
    u = uscale * (dyw @ lam)
    fac = u @ rho
    if fault in ("L_tail", "R_rows"):
        upad = uscale * (dy @ d["ltail"][:, :case.r16 - r].astype(f64))     # u~'s pad columns r .. r16
        if fault == "L_tail":
            fac += upad.sum(axis=1, keepdims=True) * rho[-1]
        else:
            fac += upad @ unpack(d["rrows"], case.rb)[:case.r16 - r, :case.n].astype(f64)
    dx = gs * (sk * code + fac)
    if fault is not None:       # the bars belong to the case, not to the fault
        return dx, u, None, None
    ady, al = np.abs(dy), np.abs(d["lam"].astype(f64))
    A = f64(d["gs"]) * (f64(sk32) * (ady @ np.abs(d["c"].astype(f64)))
                        + f64(us32) * (ady @ al) @ np.abs(d["rho"].astype(f64)))
    bar = (m + r + 32) * 2.0 ** -24 * A
    ubar = (m + 8) * 2.0 ** -24 * f64(us32) * (ady @ al)
    return dx, u, bar, ubar


def factor_operand(case: Case, which: str):
    """("codes", uint8 buffer, rows of it that are the operand, scale, bits) or ("fp16", array) of
    factor "lam" / "rho", the coded ones hostile (see `l_codes`, `r_codes`)."""
    d = inputs(case)
    if which == "lam":
        return ("fp16", d["lam"]) if case.lb == 16 else ("codes", l_codes(case), case.m, d["sl"], case.lb)
    return ("fp16", d["rho"]) if case.rb == 16 else ("codes", r_codes(case), case.r, d["sr"], case.rb)
