"""Cases and the fp64 reference of the gated pair (include/caldera_hip.h, cq_linear_glu_forward): two
packed layers `gate` and `up` of the same shape on one activation x,

    h[t, i]   = a(v_g[t, i]) * v_u[t, i]                    a = identity | silu: v / (1 + exp(-v))
    v_l[t, i] = gs_l * (qs_l * sum_j x[t, j] V_l[i, j] + sum_q z~_l[t, q] l_l[i, q]) (+ bias_l[i])
    z~_l[t, q] = zscale_l * sum_j x[t, j] rho_l[q, j]

with V the uniform codes (qs = s / k) or the NF integer levels (qs = s / D), l / rho the fp16 factors or
their uniform codes and zscale the fp32 product of the coded factors' scale / k, exactly as in
linear_cases.py, linear_factor_cases.py and linear_codebook_cases.py.  The member dicts have the layout of
linear_group_cases.py, whose `scales`, `weights` and `factor_operand` are used on them as they are (a Case
here has the attributes fmt, bits, lb, rb they read); the packers and the level tables are those modules'.
Host-seeded numpy; the reference is evaluated in fp64 from the operands as the kernel sees them.

Random cases (all of ALL): x ~ N(0, 1), fp16 factors ~ 0.15 N(0, 1), coded factors with scale 0.3, s = 0.05
as in the modules above; gs_gate = 1.7 (theirs), gs_up = 0.45: a scale taken from the wrong member changes
v_u by a factor 3.8, which shows against the bar at n = 2600 too (there the bar is ~2 % of a typical |h|:
a factor 1.5 measured 9 bars on the 48 outputs of a T = 1 case).  A bias is N(0, 1); where both members have one, they differ.  The pad tail of every code row (Q, L
and R codes; NF indices) holds nonzero codes: the result must not depend on them.

Bars.  B_l is the forward bar of linear_cases.py / linear_codebook_cases.py for member l,

    B_l = (P n + r_l + 32) 2^-24 A_l,    A_l = gs_l (qs_l |x| |V_l|^T + zscale_l |x| |rho_l|^T |l_l|^T)

(P = 2 at NF2: two planes are two products per column; else 1).  With v = v64 + d, |d_g| <= B_g,
|d_u| <= B_u, and |silu'| <= 1.1 (its maximum is 1.0998 at v = 2.3994),

    |silu(v_g) v_u - silu(g64) u64| <= 1.1 |u64| B_g + |silu(g64)| B_u + 1.1 B_g B_u

and the epilogue's own arithmetic (expf <= 1 ulp; the add, the division and the multiply <= 1/2 ulp each:
5 2^-24, taken as 8) adds 8 2^-24 |h64|.  The end-to-end bar is the one the issue states,

    1.1 |u64| B_g + |silu(g64)| B_u + B_g B_u + 8 2^-24 |h64|

(B_g B_u is ~2^-40 of the first two terms here, so its factor 1.1 is immaterial; for the identity the same
expression with a = v is used, 1.1 then being slack).

Against the members' own fp32 outputs v (test_gpu_linear_glu.py) only the epilogue is in question:
|h - h*| <= 8 2^-24 |h*| + 1e-37 with h* = silu(v_g) v_u in fp64 from the fp32 v, plus one fp16 rounding,
2^-11 |h*| + 2^-25 (half an ulp of a normal, half the smallest subnormal), for fp16 h.

Exact cases (EXACT, act = identity): small integers as in linear_group_cases.py (x in -2..2, uniform codes
in -k..k, factors in -1..1, qs = 0.5, zscale in {0.25, 0.5, 1}, gs = 2 and 4, no bias), on the short shapes
and with uniform Q only (sums of NF levels are ~10^4 units, and their product would pass 2^24), so that
v_g, v_u and their product are integers below 2^24 in magnitude times a power of two: every summation
order and the one multiply are exact and h must equal the fp64 reference bit for bit.
test_linear_glu_host.py asserts that from the data.

Planted faults (`reference(case, act, fault)`), each a way the pair kernel can go wrong:
    act_on_up        the activation applied to up instead of gate            (silu only)
    product_dropped  h = a(v_g)
    exp_plus         silu with exp(+v): v / (1 + exp(v))                     (silu only)
    up_scale_of_gate up's gscale and bias taken from gate
    gate_rank_for_up up's L product run over gate's rank: columns >= r_gate of up dropped, columns
                     r_up .. r_gate read gate's z~ and l                     (r_gate != r_up)
"""
from dataclasses import dataclass

import numpy as np

import linear_cases as LC
import linear_codebook_cases as CC
import linear_factor_cases as FC  # noqa: F401  (the factor conventions restated above are this module's)
import linear_group_cases as GC
from linear_cases import f16, f32, f64, row_bytes  # noqa: F401  (re-exported)

ACT_IDENTITY, ACT_SILU = 0, 1
GS = (f32(1.7), f32(0.45))


@dataclass(frozen=True)
class Case:
    m: int
    n: int
    rg: int                 # gate's rank
    ru: int                 # up's
    bits: int               # Q: 2 | 4
    fmt: str                # "uniform" | "nf"
    T: int
    lb: int = 16            # L of the members with r > 0: 2 | 4 | 16
    rb: int = 16
    bias: int = 0           # 0: none, 1: gate only, 2: both
    kind: str = "random"    # | "exact"

    @property
    def id(self):
        fac = "" if self.lb == self.rb == 16 else f"L{self.lb}R{self.rb}"
        return (f"{self.kind}-m{self.m}n{self.n}r{self.rg}r{self.ru}-{self.fmt}{self.bits}{fac}-T{self.T}"
                + ("", "-biasg", "-biasgu")[self.bias])

    @property
    def ranks(self):
        return (self.rg, self.ru)

    @property
    def planes(self):
        return 2 if self.fmt == "nf" and self.bits == 2 else 1

    @property
    def seed(self):
        return (self.m * 1000003 + self.n * 1009 + self.rg * 101 + self.ru * 211 + self.bits * 11 + self.lb * 307
                + self.rb * 701 + self.T + self.bias * 5003 + (0 if self.fmt == "uniform" else 424243)
                + (0 if self.kind == "random" else 7919) + 55117)


SHAPES = ((33, 64, 8, 8),
          (48, 198, 40, 0),       # one member has no factors
          (80, 898, 200, 8),      # ranks differ; fewer rows than one prefill workgroup
          (272, 512, 16, 16),     # three prefill workgroups, the last one partial
          (48, 2600, 40, 40))     # decode waves own two chunks
TOKENS = (1, 5, 16, 17, 64, 130)
QFORMATS = (("uniform", 2), ("uniform", 4), ("nf", 4), ("nf", 2))
FACTOR_SHAPE = (48, 198, 40, 40)
FACTOR_FORMATS = ((4, 4), (2, 16))
F16_SHAPES = ((33, 64), (48, 198))    # the cases that also run with fp16 h


def _cases():
    out = []
    for fmt, bits in QFORMATS:
        out += [Case(*s, bits, fmt, T) for s in SHAPES for T in TOKENS]
        out += [Case(*FACTOR_SHAPE, bits, fmt, T, lb, rb) for lb, rb in FACTOR_FORMATS for T in (16, 17)]
        out += [Case(*SHAPES[0], bits, fmt, T, bias=b) for b in (1, 2) for T in (5, 17)]
    return out


ALL = _cases()
EXACT = [Case(m, n, rg, ru, bits, fmt, T, kind="exact")
         for (m, n, rg, ru) in SHAPES[:2] + (FACTOR_SHAPE,) for fmt, bits in QFORMATS[:2] for T in (5, 17)]
EXACT += [Case(*FACTOR_SHAPE, 2, "uniform", T, 2, 16, kind="exact") for T in (16, 17)]   # codes in -1..1


def has_f16(case: Case) -> bool:
    return (case.m, case.n) in F16_SHAPES


_CACHE = {}


def inputs(case: Case):
    """dict(x (T, n) f16, members [gate, up]: dict(m, r, V (m, n) int8 codes | uint8 indices, l (m, r) int8 |
    f16, rho (r, n) int8 | f16, s, sl, sr, gs (f32; sl / sr None for an fp16 factor), bias (m,) f32 | None));
    built once per case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    random = case.kind == "random"
    nf = case.fmt == "nf"
    x = (rng.standard_normal((case.T, case.n)) if random else rng.integers(-2, 3, (case.T, case.n))).astype(f16)

    def factor(bits, shape):
        if bits != 16:
            k = GC.k_of(bits)
            scale = f32(0.3) if random else (f32(k) if nf else f32(k / 2))
            return rng.integers(-k, k + 1, shape).astype(np.int8), scale
        if random:
            return (0.15 * rng.standard_normal(shape)).astype(f16), None
        return rng.integers(-1, 2, shape).astype(f16), None

    members = []
    for i, r in enumerate(case.ranks):
        if nf:
            V = rng.integers(0, 2 ** case.bits, (case.m, case.n)).astype(np.uint8)
            s = f32(0.05) if random else f32(CC.DENOM[case.bits] / 2)
        else:
            k = GC.k_of(case.bits)
            V = rng.integers(-k, k + 1, (case.m, case.n)).astype(np.int8)
            s = f32(0.05) if random else f32(k / 2)
        l, sl = factor(case.lb, (case.m, r))
        rho, sr = factor(case.rb, (r, case.n))
        bias = rng.standard_normal(case.m).astype(f32) if i < case.bias else None
        gs = GS[i] if random else f32(2.0 * (i + 1))
        members.append(dict(m=case.m, r=r, V=V, l=l, rho=rho, s=s, sl=sl, sr=sr, gs=gs, bias=bias))
    out = dict(x=x, members=members)
    _CACHE[case] = out
    return out


def _tailed(c, bits, rng):
    """(rows, cols) codes -> inference layout whose pad tail holds random nonzero codes."""
    rows, cols = c.shape
    k, per = GC.k_of(bits), 8 // bits
    rb = row_bytes(cols, bits)
    full = rng.integers(1, k + 1, (rows, rb * per)).astype(np.int8)
    full[:, :cols] = c
    return LC.pack_codes(full, bits).reshape(rows, rb)


def packed_codes(case: Case, mem):
    """The member's Q operand in the inference layout, the pad tail holding nonzero codes (NF: the last
    index, a nonzero level)."""
    if case.fmt == "nf":
        return CC.index_codes(mem["V"], case.bits, tail=2 ** case.bits - 1)
    return _tailed(mem["V"], case.bits, np.random.default_rng(case.seed + 1))


def factor_operand(case: Case, mem, which: str):
    """("codes", uint8 inference layout with nonzero tails, scale, bits) or ("fp16", array) of "l" / "rho"."""
    f = GC.factor_operand(case, mem, which)
    if f[0] == "fp16":
        return f
    return "codes", _tailed(mem[which], f[3], np.random.default_rng(case.seed + (2 if which == "l" else 3))), f[2], f[3]


def silu64(v, plus=False):
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(v if plus else -v))


def act64(act, v):
    return silu64(v) if act == ACT_SILU else v


FAULTS = ("act_on_up", "product_dropped", "exp_plus", "up_scale_of_gate", "gate_rank_for_up")


def fault_applies(case: Case, act: int, fault: str) -> bool:
    if fault in ("act_on_up", "exp_plus"):
        return act == ACT_SILU
    if fault == "gate_rank_for_up":
        return case.rg != case.ru
    return True


_TERMS = {}


def _terms(case: Case):
    """Per member, in fp64 and once per case (every reference, planted or not, is assembled from these; treat
    as read-only): core = qs x V^T + z~ l^T (T, m), its code part, z~ (T, r), l (m, r) and the bar B (T, m)."""
    if case in _TERMS:
        return _TERMS[case]
    d = inputs(case)
    x = d["x"].astype(f64)
    ax = np.abs(x)
    out = []
    for mem in d["members"]:
        qs32, z32 = GC.scales(case, mem)
        qs, zscale = f64(qs32), f64(z32)
        W = GC.weights(case, mem)
        l, rho = mem["l"].astype(f64), mem["rho"].astype(f64)
        z = zscale * (x @ rho.T)
        code = qs * (x @ W.T)
        A = f64(mem["gs"]) * (qs * (ax @ np.abs(W).T) + zscale * ((ax @ np.abs(rho).T) @ np.abs(l).T))
        out.append(dict(code=code, core=code + z @ l.T, z=z, l=l,
                        B=(case.planes * case.n + mem["r"] + 32) * 2.0 ** -24 * A))
    _TERMS[case] = out
    return out


def preactivations(case: Case, fault: str | None = None):
    """(v64, B) per member: the fp64 pre-activations (T, m) and the members' forward bars."""
    mems = inputs(case)["members"]
    vs, bars = [], []
    for i, (mem, t) in enumerate(zip(mems, _terms(case))):
        core, gs, bias = t["core"], f64(mem["gs"]), mem["bias"]
        if i == 1 and fault == "up_scale_of_gate":
            gs, bias = f64(mems[0]["gs"]), mems[0]["bias"]
        if i == 1 and fault == "gate_rank_for_up":
            tg = _terms(case)[0]
            rg, ru = case.rg, case.ru
            core = t["code"] + t["z"][:, :min(rg, ru)] @ t["l"][:, :min(rg, ru)].T
            if rg > ru:
                core = core + tg["z"][:, ru:rg] @ tg["l"][:, ru:rg].T
        v = gs * core
        if bias is not None:
            v = v + bias.astype(f64)
        vs.append(v)
        bars.append(t["B"])
    return vs, bars


def reference(case: Case, act: int, fault: str | None = None):
    """(h64, bar): the fp64 reference (T, m) from the operands and the end-to-end bar (module docstring)."""
    (g, u), (Bg, Bu) = preactivations(case, fault)
    if fault == "act_on_up":
        h = g * act64(act, u)
    elif fault == "exp_plus":
        h = silu64(g, plus=True) * u
    elif fault == "product_dropped":
        h = act64(act, g)
    else:
        h = act64(act, g) * u
    (g0, u0), _ = preactivations(case) if fault else ((g, u), None)
    a0 = act64(act, g0)
    bar = 1.1 * np.abs(u0) * Bg + np.abs(a0) * Bu + Bg * Bu + 8 * 2.0 ** -24 * np.abs(a0 * u0)
    return h, bar


def epilogue_reference(act: int, vg32, vu32):
    """(h*, bar32, bar16): h* = a(v_g) v_u in fp64 from the members' fp32 outputs, and the bars of an fp32
    and an fp16 h against it."""
    hs = act64(act, vg32.astype(f64)) * vu32.astype(f64)
    bar32 = 8 * 2.0 ** -24 * np.abs(hs) + 1e-37
    return hs, bar32, bar32 + 2.0 ** -11 * np.abs(hs) + 2.0 ** -25


def exact_units(case: Case):
    """Per member of an exact case: (units, unit, split_exact) as linear_group_cases.exact_units."""
    d = inputs(case)
    out = []
    for mem in d["members"]:
        x = np.abs(d["x"].astype(f64))
        qs, zscale = (f64(v) for v in GC.scales(case, mem))
        unit = min(qs, zscale)
        z = zscale * (d["x"].astype(f64) @ mem["rho"].astype(f64).T)
        hi = z.astype(f16)
        lo = (z - hi.astype(f64)).astype(f16)
        split = bool(np.array_equal(hi.astype(f64) + lo.astype(f64), z))
        za = np.abs(hi.astype(f64)) + np.abs(lo.astype(f64))
        total = qs * (x @ np.abs(GC.weights(case, mem)).T) + za @ np.abs(mem["l"].astype(f64)).T
        out.append((float(total.max() / unit), float(unit), split))
    return out
