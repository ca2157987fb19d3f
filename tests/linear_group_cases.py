"""Cases and the fp64 reference of the grouped packed forward (include/caldera_hip.h,
cq_linear_group_forward): several packed layers on one activation x,

    y_i[t, a]  = gs_i * (qs_i * sum_j x[t, j] V_i[a, j] + sum_q z~_i[t, q] l_i[a, q]) (+ bias_i[a])
    z~_i[t, q] = zscale_i * sum_j x[t, j] rho_i[q, j]

with V the uniform codes (qs = s / k) or the NF integer levels (qs = s / D), l / rho the fp16 factors
or their uniform codes and zscale the fp32 product of the coded factors' scale / k, exactly as in
linear_cases.py, linear_factor_cases.py and linear_codebook_cases.py (whose packers and level tables
are used here).  Host-seeded numpy, one x per group, the reference of every member in fp64 from the
operands as the kernel sees them.

All groups are exact: x in -4..4 (-1..1 when n > 2048, and for NF2 at n = 898, where 898 * 4 * 8165
would pass 2^24), codes in -k..k or level indices, fp16 factors in -2..2, s = k / 2 resp. D / 2 so
that qs = 0.5, coded factors with scale k / 2 (uniform Q, as linear_factor_cases.py) resp. k (NF Q, as
linear_codebook_cases.py).  gs_i = 4 * 2^(i mod 3): member 0 has the other modules' gs = 4, and a power
of two keeps every product exact while neighbouring members (also last -> first) differ, which the
fault "next_member_scale" needs.  test_linear_group_host.py asserts per member that the sum of the
absolute terms stays below 2^24 units and that z~ splits exactly into fp16 halves, so every summation
order gives the same fp32 value and the kernel must match bit for bit.

Member shapes put every boundary inside a tile that a wrong member lookup would cross: m is no
multiple of 16 nor of the prefill workgroup's 256 rows, r32 differs between members, one member has
rank 0, and one group has CQ_LINEAR_GROUP_MAX members.  Beyond the formats the grouped entry was asked
to be tested on, the n = 198 group also runs NF4 / NF2 codes with coded factors (4/4 and 2/fp16) at one
decode and one prefill token count: those are kernel instantiations of their own.

Planted faults (`reference(group, fault, order)`), each a way the member lookup can go wrong:
    next_member_scale   member i scaled by member i + 1's s / k and gs (the last by the first's)
    shared_z            member 1 reads member 0's z (columns beyond member 0's rank read as zero)
    row_shift           member 1's code rows start 16 rows early: its first tile reads member 0's last rows
    skip_rank0          members after a rank-0 member take the previous member's factor term
    last_member_dropped the last member's output is not written (zeros)
`order`: the members in another order (a permutation of indices), as the GPU test passes them.
"""
from dataclasses import dataclass

import numpy as np

import linear_cases as LC
import linear_codebook_cases as CC
from linear_cases import f16, f32, f64, inference_codes, row_bytes  # noqa: F401  (re-exported)

GROUP_MAX = 8


@dataclass(frozen=True)
class Group:
    n: int
    members: tuple          # ((m, r), ...)
    bits: int               # Q: 2 | 4
    T: int
    fmt: str = "uniform"    # "uniform" | "nf"
    lb: int = 16            # L of the members with r > 0: 2 | 4 | 16
    rb: int = 16
    bias: int = -1          # the member with a bias, or -1

    @property
    def id(self):
        fac = "" if self.lb == self.rb == 16 else f"L{self.lb}R{self.rb}"
        return f"n{self.n}x{len(self.members)}-{self.fmt}{self.bits}{fac}-T{self.T}"

    @property
    def count(self):
        return len(self.members)

    @property
    def seed(self):
        return (self.n * 1009 + len(self.members) * 7 + self.bits * 11 + self.lb * 307 + self.rb * 701 + self.T
                + (0 if self.fmt == "uniform" else 424243) + 9176)

    @property
    def reversed_order(self):
        return tuple(range(self.count - 1, -1, -1))


SHAPES = {198: ((33, 8), (272, 40), (48, 0)),
          898: ((80, 200), (33, 40)),
          2600: ((48, 40), (33, 264)),
          64: ((33, 8),)}                                    # a group of one
EIGHT = tuple((16 + i, 8) for i in range(GROUP_MAX))     # and one of GROUP_MAX members, at n = 64 too
TOKENS = (1, 5, 16, 17)


def _groups():
    out = []
    for bits in (2, 4):
        for n, members in list(SHAPES.items()) + [(64, EIGHT)]:
            for T in TOKENS + ((130,) if n == 198 else ()):
                out.append(Group(n, members, bits, T, bias=1 if n == 198 else -1))
        for n in (198, 898):   # coded factors 4/4 and 2/fp16, uniform Q
            for lb, rb in ((4, 4), (2, 16)):
                for T in TOKENS + ((130,) if n == 198 else ()):
                    out.append(Group(n, SHAPES[n], bits, T, lb=lb, rb=rb))
    for bits in (4, 2):        # NF4 and NF2, fp16 factors
        for n in (198, 898):
            for T in TOKENS + ((130,) if n == 198 else ()):
                out.append(Group(n, SHAPES[n], bits, T, fmt="nf"))
        for lb, rb in ((4, 4), (2, 16)):   # NF Q with coded factors (their own kernels), decode and prefill
            for T in (5, 17):
                out.append(Group(198, SHAPES[198], bits, T, fmt="nf", lb=lb, rb=rb))
    return out


ALL = _groups()


def k_of(bits):
    return 2 ** (bits - 1) - 1


def xamp(group):
    """The largest |x| of the group, see the module docstring."""
    if group.n > LC.LONG_N or (group.fmt == "nf" and group.bits == 2 and group.n >= 898):
        return 1
    return 4


_CACHE = {}


def inputs(group: Group):
    """dict(x (T, n) f16, members [dict(m, r, V (m, n) int8 codes | uint8 indices, l (m, r) int8 | f16,
    rho (r, n) int8 | f16, s, sl, sr, gs (f32; sl / sr None for an fp16 factor), bias (m,) f32 | None)]);
    built once per group and shared (treat as read-only)."""
    if group in _CACHE:
        return _CACHE[group]
    rng = np.random.default_rng(group.seed)
    xa = xamp(group)
    x = rng.integers(-xa, xa + 1, (group.T, group.n)).astype(f16)
    nf = group.fmt == "nf"

    def factor(bits, shape):
        if bits != 16:
            k = k_of(bits)
            return rng.integers(-k, k + 1, shape).astype(np.int8), f32(k) if nf else f32(k / 2)
        return rng.integers(-2, 3, shape).astype(f16), None

    members = []
    for i, (m, r) in enumerate(group.members):
        if nf:
            V = rng.integers(0, 2 ** group.bits, (m, group.n)).astype(np.uint8)
            s = f32(CC.DENOM[group.bits] / 2)
        else:
            k = k_of(group.bits)
            V = rng.integers(-k, k + 1, (m, group.n)).astype(np.int8)
            s = f32(k / 2)
        l, sl = factor(group.lb, (m, r))
        rho, sr = factor(group.rb, (r, group.n))
        bias = (rng.integers(-8, 9, m) * 0.5).astype(f32) if i == group.bias else None
        members.append(dict(m=m, r=r, V=V, l=l, rho=rho, s=s, sl=sl, sr=sr, gs=f32(4.0 * 2 ** (i % 3)), bias=bias))
    out = dict(x=x, members=members)
    _CACHE[group] = out
    return out


def scales(group: Group, mem):
    """(qs, zscale) of a member as the kernel forms them: fp32 divisions, fp32 product."""
    den = f32(CC.DENOM[group.bits]) if group.fmt == "nf" else f32(k_of(group.bits))
    qs = f32(mem["s"] / den)
    z = f32(1.0)
    if mem["r"] > 0:
        if group.lb != 16:
            z = f32(mem["sl"] / f32(k_of(group.lb)))
        if group.rb != 16:
            skr = f32(mem["sr"] / f32(k_of(group.rb)))
            z = f32(z * skr) if group.lb != 16 else skr
    return qs, z


def weights(group: Group, mem):
    """(m, n) fp64 V as the kernel decodes it: the codes, or the integer levels of the indices."""
    if group.fmt == "nf":
        return CC.LEVELS[group.bits][mem["V"].astype(np.int64)]
    return mem["V"].astype(f64)


def packed_codes(group: Group, mem):
    """The member's Q operand in the inference layout."""
    if group.fmt == "nf":
        return CC.index_codes(mem["V"], group.bits)
    return inference_codes(mem["V"], group.bits)


def factor_operand(group: Group, mem, which: str):
    """("codes", uint8 inference layout, scale, bits) or ("fp16", array) of factor "l" / "rho"."""
    bits = group.lb if which == "l" else group.rb
    if bits == 16:
        return "fp16", mem[which]
    return "codes", inference_codes(mem[which], bits), mem["sl" if which == "l" else "sr"], bits


FAULTS = ("next_member_scale", "shared_z", "row_shift", "skip_rank0", "last_member_dropped")


def fault_applies(group: Group, fault: str, order=None) -> bool:
    order = tuple(range(group.count)) if order is None else tuple(order)
    ranks = [group.members[i][1] for i in order]
    if fault in ("next_member_scale", "row_shift"):
        return group.count >= 2
    if fault == "shared_z":
        return group.count >= 2 and ranks[0] > 0 and ranks[1] > 0
    if fault == "skip_rank0":
        return 0 in ranks[:-1]
    return True


def _terms(group, x, mem):
    qs, zscale = (f64(v) for v in scales(group, mem))
    code = x @ weights(group, mem).T
    z = zscale * (x @ mem["rho"].astype(f64).T)
    return qs, code, z


def reference(group: Group, fault: str | None = None, order=None):
    """[y64 (T, m_i)] in the order given (default: the group's own), with one planted fault or none."""
    d = inputs(group)
    x = d["x"].astype(f64)
    order = tuple(range(group.count)) if order is None else tuple(order)
    mems = [d["members"][i] for i in order]
    terms = [_terms(group, x, mem) for mem in mems]
    out = []
    after_rank0 = False
    for i, mem in enumerate(mems):
        qs, code, z = terms[i]
        gs = f64(mem["gs"])
        lr = z @ mem["l"].astype(f64).T
        if fault == "next_member_scale":
            nxt = mems[(i + 1) % len(mems)]
            qs, gs = f64(scales(group, nxt)[0]), f64(nxt["gs"])
        elif fault == "shared_z" and i == 1:
            z0 = terms[0][2]
            zz = np.zeros_like(z)
            q = min(z.shape[1], z0.shape[1])
            zz[:, :q] = z0[:, :q]
            lr = zz @ mem["l"].astype(f64).T
        elif fault == "row_shift" and i == 1:
            prev = weights(group, mems[0])
            W = np.concatenate([prev[-16:], weights(group, mem)[:-16]])
            code = x @ W.T
        elif fault == "skip_rank0" and after_rank0:
            zp, lp = terms[i - 1][2], mems[i - 1]["l"].astype(f64)
            lrp = zp @ lp.T                                   # (T, m of the previous member); rank 0: zeros
            lr = lrp[:, np.arange(mem["m"]) % lrp.shape[1]]
        y = gs * (qs * code + lr)
        if mem["bias"] is not None:
            y = y + mem["bias"].astype(f64)
        if fault == "last_member_dropped" and i == len(mems) - 1:
            y = np.zeros_like(y)
        after_rank0 = after_rank0 or mem["r"] == 0
        out.append(y)
    return out


def exact_units(group: Group, mem):
    """(units, unit, split_exact) of one member: the largest per-output sum of absolute terms before gs
    in units of `unit` (the common divisor of every term: qs and zscale are 0.25, 0.5 or 1 and all other
    operands integers), and whether z~ splits exactly into fp16 halves hi + lo."""
    x = np.abs(inputs(group)["x"].astype(f64))
    qs, zscale = (f64(v) for v in scales(group, mem))
    unit = min(qs, zscale)
    xs = inputs(group)["x"].astype(f64)
    z = zscale * (xs @ mem["rho"].astype(f64).T)
    hi = z.astype(f16)
    lo = (z - hi.astype(f64)).astype(f16)
    split_exact = bool(np.array_equal(hi.astype(f64) + lo.astype(f64), z) and np.isfinite(hi.astype(f64)).all())
    za = np.abs(hi.astype(f64)) + np.abs(lo.astype(f64))       # both halves are multiplied with l
    total = qs * (x @ np.abs(weights(group, mem)).T) + za @ np.abs(mem["l"].astype(f64)).T
    # the z sum itself, before zscale: integers
    zsum = (x @ np.abs(mem["rho"].astype(f64)).T).max() if mem["r"] else 0.0
    return float(max(total.max() / unit, zsum)), float(unit), split_exact
