"""Cases and the fp64 reference of the packed layer's materialise kernel (include/caldera_hip.h,
cq_linear_dequant):

    W[i, j] = gs * (qs * V(code[i, j]) + fscale * sum_q lam[i, q] rho[q, j])        i < m, j < n

V = u - k and qs = s / k (uniform), V = I[idx] and qs = s / D (NF4 / NF2); lam / rho the fp16 factors
or their uniform codes; fscale the fp32 product of the coded factors' scale / k (1 for fp16), as in
linear_factor_cases.py and linear_codebook_cases.py.  Host-seeded numpy, the reference evaluated in
fp64 from the operands as the kernel sees them, qs and fscale formed in fp32 as the kernel forms them.

Shapes (m, n, r).  The kernel's workgroup tile is TILE = 128 rows x 128 columns, its R chunk 32 rows:
    (1, 8, 0)        one output row, codes only
    (12, 198, 5)     n bits / 8 is no multiple of 16, odd rows start unaligned in w
    (48, 198, 40)    every format combination; two R chunks, the second ragged
    (160, 256, 128)  every format combination; two row tiles, four whole R chunks
    (130, 520, 72)   two tiles each way, r no multiple of 32, three R chunks
    (257, 130, 16)   PAST_TILE: past one tile per workgroup in both directions (3 x 2 workgroups),
                     a last row tile of one row and a last column tile of two columns

Exact cases: s = k / 2 resp. D / 2 (qs = 0.5), gs = 4, fp16 factors integers in -2..2, coded factors
with scale = 2 k (scale / k = 2, so fscale is 2 or 4).  The factor sum is an integer of at most
49 r, f = fscale * sum an integer below 2^24, t = 0.5 V + f a multiple of 0.5 and w = 4 t an integer:
every intermediate is an fp32 value whatever the operation order, so the kernel must match bit for
bit (test_linear_dequant_host.py checks the magnitudes from the data).

Random cases: fp16 factors ~ 0.15 N(0, 1), coded factors with scale 0.3, s = 0.05, gs = 1.7, bar

    |w - w64| <= (r + 8) 2^-24 A[i, j],   A = |gs| (|qs V| + |fscale| sum_q |lam| |rho|)

r for the worst-case fp32 accumulation in any order, 8 for the scalar roundings (the header names
three: f, t, w).

Planted faults (`reference(case, fault)`):
    format_swap     offset-binary codes read as level indices (V = I[u]) resp. indices as codes (idx - k)
    nibble_order    the Q codes of a byte taken LSB-first
    s_for_sk        s applied where s / k (s / D) belongs (not uniform 2-bit: k = 1)
    drop_fscale     fscale left out (a coded factor)
    lscale_for_lk   lscale where lscale / k belongs (4-bit L codes; k = 1 at 2-bit)
    tr_block        the first 16 x 16 block of L transposed
    swap_r_chunks   the first two 32-row chunks of R in each other's place (r > 32)
    drop_last_chunk the rows of R from 32 floor((r - 1) / 32) on contribute nothing
    tail_as_codes   the Q code rows read back to back, the padded tails taken for codes (rows > 0, a tail)
    gs_on_q         gs applied to the Q term only
Against a random case's bar (numpy runs of these formulas, the smallest over the cases a fault is
claimed for in RANDOM_FAULTS; test_linear_dequant_host.py asserts >= 10): every fault changes a term
of the order of A itself, >= 1600 bars at r <= 128 (the smallest: format_swap at NF2, r = 128), so all
are claimed on every random case they apply to.  Where A is zero (code 0 and r = 0) the bar is zero
and the kernel's zero meets it.
"""
from dataclasses import dataclass

import numpy as np

import linear_codebook_cases as CC
from linear_cases import f16, f32, f64, inference_codes, row_bytes  # noqa: F401  (re-exported)

LEVELS, DENOM, TAIL_INDEX = CC.LEVELS, CC.DENOM, CC.TAIL_INDEX
index_codes = CC.index_codes
UNIFORM, NF = 0, 1
TILE = (128, 128)            # rows x columns per workgroup of csrc/cq_linear_dequant.hip
CHUNK_ROWS = 32              # rows of R per LDS chunk
PAST_TILE = (257, 130, 16)


@dataclass(frozen=True)
class Case:
    kind: str       # "exact" | "random"
    m: int
    n: int
    r: int
    fmt: int        # UNIFORM | NF
    bits: int       # Q bits
    lb: int = 16    # L: 2 | 4 | 16
    rb: int = 16    # R

    @property
    def id(self):
        fac = "" if self.lb == self.rb == 16 else f"L{self.lb}R{self.rb}"
        return f"{self.kind}-m{self.m}n{self.n}r{self.r}{'nf' if self.fmt == NF else 'u'}{self.bits}{fac}"

    @property
    def seed(self):
        return (self.m * 1000003 + self.n * 1009 + self.r * 101 + self.bits * 11 + self.fmt * 5 + self.lb * 307
                + self.rb * 701 + (0 if self.kind == "exact" else 7919) + 990001)


QFORMATS = ((UNIFORM, 2), (UNIFORM, 4), (NF, 2), (NF, 4))
ALL_FACTORS = tuple((lb, rb) for lb in (16, 4, 2) for rb in (16, 4, 2))
SOME_FACTORS = ((16, 16), (4, 4), (2, 16))
FULL_SHAPES = ((48, 198, 40), (160, 256, 128))
OTHER_SHAPES = ((1, 8, 0), (12, 198, 5), (130, 520, 72), PAST_TILE)


def _cases(kind):
    out = []
    for (fmt, bits) in QFORMATS:
        for (m, n, r) in FULL_SHAPES:
            out += [Case(kind, m, n, r, fmt, bits, lb, rb) for (lb, rb) in ALL_FACTORS]
        for (m, n, r) in OTHER_SHAPES:
            out += [Case(kind, m, n, r, fmt, bits, lb, rb) for (lb, rb) in (SOME_FACTORS if r else ((16, 16),))]
    return out


EXACT = _cases("exact")
RANDOM = _cases("random")
ALL = EXACT + RANDOM


def _kf(bits):
    return 2 ** (bits - 1) - 1


_CACHE = {}


def inputs(case: Case):
    """dict(q (m, n): int8 codes in [-k, k] | uint8 level indices, l (m, r) int8 codes | f16,
    rho (r, n) int8 codes | f16, s, sl, sr, gs (f32; sl / sr None for an fp16 factor)); built once per
    case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    m, n, r = case.m, case.n, case.r
    random = case.kind == "random"
    if case.fmt == NF:
        q = rng.integers(0, 2 ** case.bits, (m, n)).astype(np.uint8)
    else:
        k = _kf(case.bits)
        q = rng.integers(-k, k + 1, (m, n)).astype(np.int8)

    def factor(bits, shape):
        if bits != 16:
            k = _kf(bits)
            return rng.integers(-k, k + 1, shape).astype(np.int8), f32(0.3) if random else f32(2 * k)
        if random:
            return (0.15 * rng.standard_normal(shape)).astype(f16), None
        return rng.integers(-2, 3, shape).astype(f16), None

    l, sl = factor(case.lb, (m, r))
    rho, sr = factor(case.rb, (r, n))
    if random:
        s, gs = f32(0.05), f32(1.7)
    else:
        s = f32(DENOM[case.bits] / 2) if case.fmt == NF else f32(_kf(case.bits) / 2)
        gs = f32(4.0)
    out = dict(q=q, l=l, rho=rho, s=s, sl=sl, sr=sr, gs=gs)
    _CACHE[case] = out
    return out


def scales(case: Case, d=None, fault=None):
    """(qs, fscale) as the kernel forms them: fp32 divisions, fp32 product."""
    d = inputs(case) if d is None else d
    den = f32(DENOM[case.bits]) if case.fmt == NF else f32(_kf(case.bits))
    qs = d["s"] if fault == "s_for_sk" else f32(d["s"] / den)
    z = f32(1.0)
    if case.lb != 16:
        z = d["sl"] if fault == "lscale_for_lk" else f32(d["sl"] / f32(_kf(case.lb)))
    if case.rb != 16:
        skr = f32(d["sr"] / f32(_kf(case.rb)))
        z = f32(z * skr) if case.lb != 16 else skr
    if fault == "drop_fscale" or case.r == 0:
        z = f32(1.0)
    return qs, z


def q_operand(case: Case):
    """The Q codes in the inference layout: (m, row_bytes) uint8."""
    q = inputs(case)["q"]
    return index_codes(q, case.bits) if case.fmt == NF else inference_codes(q, case.bits)


def factor_operand(case: Case, which: str):
    """("codes", uint8 inference layout, scale, bits) or ("fp16", array) of factor "l" / "rho"."""
    d = inputs(case)
    bits = case.lb if which == "l" else case.rb
    if bits == 16:
        return "fp16", d[which]
    return "codes", inference_codes(d[which], bits), d["sl" if which == "l" else "sr"], bits


FAULTS = ("format_swap", "nibble_order", "s_for_sk", "drop_fscale", "lscale_for_lk", "tr_block", "swap_r_chunks",
          "drop_last_chunk", "tail_as_codes", "gs_on_q")
# faults that must move a random case by ten bars where they apply to it: all of them
RANDOM_FAULTS = FAULTS


def fault_applies(case: Case, fault: str) -> bool:
    """Whether a planted fault exists for the case and, from its data's design, must show."""
    coded = case.r > 0 and (case.lb != 16 or case.rb != 16)
    if fault == "drop_fscale":
        return coded
    if fault == "lscale_for_lk":
        return case.r > 0 and case.lb == 4
    if fault == "tr_block":
        return case.r >= 2 and case.m >= 2
    if fault == "swap_r_chunks":
        return case.r > CHUNK_ROWS
    if fault in ("drop_last_chunk", "gs_on_q"):
        return case.r > 0
    if fault == "tail_as_codes":
        return case.m > 1 and (case.n * case.bits) % 128 != 0
    if fault == "nibble_order":
        return case.n > 1
    if fault == "s_for_sk":
        return case.fmt == NF or case.bits != 2          # k = 1 at uniform 2-bit: s / k is s
    return True


def q_values(case: Case, fault: str | None = None):
    """(m, n) fp64 V as the (possibly faulty) decode sees them."""
    q = inputs(case)["q"]
    bits, k, per = case.bits, _kf(case.bits), 8 // case.bits
    nf = case.fmt == NF
    u = q.astype(np.int64) if nf else q.astype(np.int64) + k          # the stored field
    tail = TAIL_INDEX[bits] if nf else k
    if fault in ("nibble_order", "tail_as_codes"):
        width = row_bytes(case.n, bits) * per
        full = np.full((case.m, width), tail, dtype=np.int64)
        full[:, :case.n] = u
        if fault == "nibble_order":
            u = full.reshape(case.m, -1, per)[:, :, ::-1].reshape(case.m, width)[:, :case.n]
        else:
            u = full.reshape(-1)[:case.m * case.n].reshape(case.m, case.n)
    as_index = nf != (fault == "format_swap")
    if as_index:
        return LEVELS[bits][np.minimum(u, 2 ** bits - 1)]
    return (u - k).astype(f64)


def factors(case: Case, fault: str | None = None):
    """(lam (m, r), rho (r, n)) fp64, unscaled, as the (possibly faulty) product sees them."""
    d = inputs(case)
    lam, rho = d["l"].astype(f64), d["rho"].astype(f64)
    r = case.r
    if fault == "tr_block":
        b = min(16, case.m, r)
        lam = lam.copy()
        lam[:b, :b] = lam[:b, :b].T.copy()
    elif fault == "swap_r_chunks":
        pad = np.zeros((-(-r // CHUNK_ROWS) * CHUNK_ROWS, case.n))
        pad[:r] = rho
        pad[:2 * CHUNK_ROWS] = np.concatenate([pad[CHUNK_ROWS:2 * CHUNK_ROWS], pad[:CHUNK_ROWS]])
        rho = pad[:r]
    elif fault == "drop_last_chunk":
        rho = rho.copy()
        rho[CHUNK_ROWS * ((r - 1) // CHUNK_ROWS):] = 0
    return lam, rho


def reference(case: Case, fault: str | None = None):
    """(w64 (m, n), bar): the fp64 reference and the elementwise bar of the random cases.  fault: one
    planted error (FAULTS), for checking that the cases can see it."""
    d = inputs(case)
    qs32, z32 = scales(case, d, fault)
    qs, z, gs = f64(qs32), f64(z32), f64(d["gs"])
    V = q_values(case, fault)
    lam, rho = factors(case, fault)
    lr = z * (lam @ rho)
    w = gs * qs * V + lr if fault == "gs_on_q" else gs * (qs * V + lr)
    qs0, z0 = (f64(v) for v in scales(case, d))
    A = abs(gs) * (np.abs(qs0 * q_values(case)) + abs(z0) * (np.abs(d["l"].astype(f64)) @ np.abs(d["rho"].astype(f64))))
    return w, (case.r + 8) * 2.0 ** -24 * A


def exact_units(case: Case):
    """Of an exact case: the largest |fscale sum| + |0.5 V| per output in units of 0.5 (every partial
    result of any operation order stays below it), and the largest unscaled |sum_q lam rho|."""
    d = inputs(case)
    al, ar = np.abs(d["l"].astype(f64)), np.abs(d["rho"].astype(f64))
    z = f64(scales(case, d)[1])
    s = al @ ar
    units = np.abs(q_values(case)) + 2.0 * z * s
    return float(units.max()), float(s.max()) if s.size else 0.0
