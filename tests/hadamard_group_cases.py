"""Cases and fp64 references of the grouped and the gated row-wise Hadamard transforms
(include/caldera_hip.h, cq_hadamard_group_rows and cq_hadamard_glu_rows).

Group: `count` transforms of the same `rows` and P, each with its own x, y, dtypes, strides, n_in, n_out
and bias; member i's reference is hadamard_cases' formula

    y_i[t, c] = s * sum_{j < n_in_i} (-1)^popcount(c & j) x_i[t, j] (+ bias_i[c])    c < n_out_i,  s = 1 / sqrt(P)

Gated pair: h[t, c] = a(v_g[t, c]) * v_u[t, c] with v_g, v_u that formula on (g, bias_g) and (u, bias_u), and
a the identity or silu, v / (1 + exp(-v)) (linear_glu_cases' helpers).

Inputs are host-seeded numpy (the bytes are the same on every machine): N(0, 1) held exactly in the
member's dtype; a bias is N(0, 1) fp32, and two biases of one case differ.  `pad` is the number of extra
elements in a row's stride (the tests fill them with NaN: they must be neither read nor written).

Bars.  B(x) = 1.01 (log2 P + 2) 2^-24 sum_j |x_j| / sqrt(P) is hadamard_cases' bar of one transform.  The
gated pair end to end takes linear_glu_cases' combination of its members' bars,

    1.1 |v_u64| B_g + |a(v_g64)| B_u + B_g B_u + 8 2^-24 |h64|

(|silu'| <= 1.1; the epilogue's expf, add, division and multiply are 5 2^-24, taken as 8).  Against the
entry's own fp32 pre-activations only the epilogue is in question: linear_glu_cases.epilogue_reference.

Parameter ranges: P in {4, 64, 512, 1024, 2048, 4096, 8192, 16384, 32768} -- one P per kernel instantiation
plus the rows-per-workgroup packing at P <= 256 -- rows in {1, 5, 17}, counts 1, 2, 3 and 8; n_in and n_out
cut per member (P, P - 5, P / 2 + 1, 1), every dtype on either side, bias on and off, padded strides.

Planted faults, each a way the kernels can go wrong:
    members_swapped    members 0 and 1 each transform the other's x           (group, count >= 2)
    n_out_of_member0   member 1 writes member 0's n_out columns: the columns between stay as they were
                       (taken as 0 here)                                      (group, n_out_0 < n_out_1)
    act_on_up          the activation applied to up instead of gate           (pair, silu)
    product_dropped    h = a(v_g)                                             (pair)
    exp_plus           silu with exp(+v)                                      (pair, silu)
    gate_bias_for_up   up's bias taken from gate                              (pair, gate has a bias)
"""
from dataclasses import dataclass

import numpy as np

import hadamard_cases as HC
import linear_glu_cases as UC
from hadamard_cases import f32, f64
from linear_glu_cases import ACT_IDENTITY, ACT_SILU  # noqa: F401  (re-exported)

XDT = HC.XDT
PS = (4, 64, 512, 1024, 2048, 4096, 8192, 16384, 32768)
GLU_MAX_N = 16384
ROWS = (1, 5, 17)
COUNTS = (1, 2, 3, 8)


def _held(v, dt):
    """fp32 array rounded to the values `dt` holds."""
    if dt == "f16":
        return v.astype(np.float16).astype(f32)
    if dt == "bf16":
        return HC.from_bf16_bits(HC.to_bf16_bits(v))
    return v.astype(f32)


def _cuts(P):
    return [c for c in (P, P - 5, P // 2 + 1, 1) if 1 <= c <= P]


@dataclass(frozen=True)
class Member:
    n_in: int
    n_out: int
    xdt: str
    ydt: str
    bias: bool
    pad_x: int
    pad_y: int


@dataclass(frozen=True)
class GroupCase:
    P: int
    rows: int
    members: tuple

    @property
    def id(self):
        return f"P{self.P}r{self.rows}x{len(self.members)}"

    @property
    def seed(self):
        return self.P * 1000003 + self.rows * 10007 + len(self.members) * 101 + 77


def _members(P, count, k):
    cuts = _cuts(P)
    out = []
    for i in range(count):
        j = i + k
        out.append(Member(n_in=cuts[j % len(cuts)], n_out=cuts[(j // 2 + i) % len(cuts)], xdt=XDT[(j + 2) % 3],
                          ydt=XDT[(2 * i + k) % 3], bias=bool((i + k) % 2), pad_x=(0, 3, 8)[j % 3],
                          pad_y=(0, 8, 5)[(i + 2 * k) % 3]))
    return tuple(out)


GROUP = [GroupCase(P, ROWS[(pi + ci) % 3], _members(P, count, pi + ci))
         for pi, P in enumerate(PS) for ci, count in enumerate(COUNTS)]


@dataclass(frozen=True)
class GluCase:
    P: int
    rows: int
    n_in: int
    n_out: int
    gdt: str
    udt: str
    hdt: str
    bias: int          # 0: none, 1: gate only, 2: both
    pad: int

    @property
    def id(self):
        return (f"P{self.P}r{self.rows}i{self.n_in}o{self.n_out}-{self.gdt}-{self.udt}-{self.hdt}"
                + ("", "-biasg", "-biasgu")[self.bias] + (f"-pad{self.pad}" if self.pad else ""))

    @property
    def seed(self):
        return (self.P * 1000003 + self.rows * 10007 + self.n_in * 101 + self.n_out * 13 + XDT.index(self.gdt) * 5
                + XDT.index(self.udt) * 3 + XDT.index(self.hdt) + self.bias * 7919 + self.pad * 31 + 4242)


def _glu_cases():
    out = []
    for pi, P in enumerate(p for p in PS if p <= GLU_MAX_N):
        cuts = _cuts(P)
        for k, rows in enumerate(ROWS):
            j = pi + k
            # the layers feed fp32; the other dtypes are the entry's own contract
            gdt, udt = ("f32", "f32") if k == 0 else (XDT[j % 3], XDT[(j + 1) % 3])
            out.append(GluCase(P, rows, cuts[j % len(cuts)], cuts[(j + k) % len(cuts)], gdt, udt, XDT[(j + 2) % 3],
                               bias=(j + 1) % 3, pad=(0, 8, 3)[k]))
    return out


GLU = _glu_cases()

_CACHE = {}


def group_inputs(case: GroupCase):
    """[dict(x (rows, n_in) fp32 exact in the member's xdt, bias (n_out,) f32 | None)] per member; built once
    per case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    out = []
    for mem in case.members:
        x = _held(rng.standard_normal((case.rows, mem.n_in)).astype(f32), mem.xdt)
        out.append(dict(x=x, bias=rng.standard_normal(mem.n_out).astype(f32) if mem.bias else None))
    _CACHE[case] = out
    return out


def glu_inputs(case: GluCase):
    """dict(g, u (rows, n_in) fp32 exact in gdt / udt, bias_g, bias_u (n_out,) f32 | None)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    g = _held(rng.standard_normal((case.rows, case.n_in)).astype(f32), case.gdt)
    u = _held(rng.standard_normal((case.rows, case.n_in)).astype(f32), case.udt)
    bg = rng.standard_normal(case.n_out).astype(f32) if case.bias >= 1 else None
    bu = rng.standard_normal(case.n_out).astype(f32) if case.bias >= 2 else None
    out = dict(g=g, u=u, bias_g=bg, bias_u=bu)
    _CACHE[case] = out
    return out


def transform64(x, P, n_out, bias=None):
    """(y64 (rows, n_out), bar (rows, 1)): hadamard_cases' reference and bar of one transform of x (rows, n_in)."""
    X = np.zeros((x.shape[0], P), dtype=f64)
    X[:, :x.shape[1]] = x.astype(f64)
    Xh = HC.hadamard64(X, P) if P > 1 else X
    y = Xh[:, :n_out] / np.sqrt(f64(P))
    if bias is not None:
        y = y + bias.astype(f64)
    bar = 1.01 * (np.log2(P) + 2) * 2.0 ** -24 * np.abs(x.astype(f64)).sum(1, keepdims=True) / np.sqrt(f64(P))
    return y, bar


GROUP_FAULTS = ("members_swapped", "n_out_of_member0")
GLU_FAULTS = ("act_on_up", "product_dropped", "exp_plus", "gate_bias_for_up")


def group_fault_applies(case: GroupCase, fault: str) -> bool:
    if len(case.members) < 2:
        return False
    if fault == "n_out_of_member0":
        return case.members[0].n_out < case.members[1].n_out
    return True


def glu_fault_applies(case: GluCase, act: int, fault: str) -> bool:
    if fault in ("act_on_up", "exp_plus"):
        return act == ACT_SILU
    if fault == "gate_bias_for_up":
        return case.bias >= 1
    return True


_REF = {}


def group_reference(case: GroupCase, fault: str | None = None):
    """[(y64 (rows, n_out_i), bar (rows, 1))] per member."""
    if (case, fault) in _REF:
        return _REF[(case, fault)]
    d = group_inputs(case)
    out = []
    for i, mem in enumerate(case.members):
        src = d[1 - i] if fault == "members_swapped" and i < 2 else d[i]
        y, _ = transform64(src["x"], case.P, mem.n_out, d[i]["bias"])
        if fault == "n_out_of_member0" and i == 1:
            y = y.copy()
            y[:, case.members[0].n_out:] = 0
        out.append((y, transform64(d[i]["x"], case.P, mem.n_out)[1]))
    _REF[(case, fault)] = out
    return out


def glu_reference(case: GluCase, act: int, fault: str | None = None):
    """(h64 (rows, n_out), bar): the fp64 reference from the inputs and the end-to-end bar (module docstring)."""
    if (case, act, fault) in _REF:
        return _REF[(case, act, fault)]
    d = glu_inputs(case)
    g, Bg = transform64(d["g"], case.P, case.n_out, d["bias_g"])
    u0, Bu = transform64(d["u"], case.P, case.n_out, d["bias_u"])
    u = transform64(d["u"], case.P, case.n_out, d["bias_g"])[0] if fault == "gate_bias_for_up" else u0
    if fault == "act_on_up":
        h = g * UC.act64(act, u)
    elif fault == "exp_plus":
        h = UC.silu64(g, plus=True) * u
    elif fault == "product_dropped":
        h = UC.act64(act, g)
    else:
        h = UC.act64(act, g) * u
    a0 = UC.act64(act, g)
    bar = 1.1 * np.abs(u0) * Bg + np.abs(a0) * Bu + Bg * Bu + 8 * 2.0 ** -24 * np.abs(a0 * u0)
    _REF[(case, act, fault)] = (h, bar)
    return h, bar
