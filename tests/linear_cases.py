"""Cases and the fp64 reference of the packed linear layer (include/caldera_hip.h, cq_linear_forward):

    y[t, i] = gs * ((s / k) * sum_j x[t, j] c[i, j] + sum_q z[t, q] L[i, q]) (+ bias[i])
    z[t, q] = sum_j x[t, j] R[q, j]                           k = 2^(bits-1) - 1

Inputs are host-seeded numpy, so the bytes are the same on every machine; the reference is
evaluated in fp64 from the operands as the kernel sees them (fp16 x, L, R; fp32 s, gs, bias;
s / k one fp32 division).

Exact cases: small integers (x in -4..4, codes in -k..k, L, R in -2..2, s = k / 2 so s / k = 0.5,
gs = 4): every partial result in any summation order is a multiple of 0.5 below 2^24 units, so
the kernel must match the reference bit for bit.  "exact16" cases are scaled down (x, L, R in
-1..1, r <= 8, n <= 64) so that y is an even integer of at most 2048 and fp16 output must equal
it too.

Random cases: x ~ N(0, 1), L, R ~ 0.15 N(0, 1) in fp16, s = 0.05, gs = 1.7, with the elementwise
worst-case fp32 bound for any summation order as the bar:

    |y - y64| <= (n + r + 32) 2^-24 A,   A = gs ((s / k) |x| |c|^T + |x| |R|^T |L|^T)

(the + 32 covers the scalings and z held as split fp16 halves).

x[0, 0], x[0, n - 1] and (T > 1) x[1, 0] are set to the largest magnitude of the case's x, so that
the planted single-code faults of test_linear_host.py show at every seed.

Long-K decode cases (n > 2048, and r = 264 with fp16 L): in decode (T <= 16) the waves of a
workgroup take the K chunks interleaved and load a wave's next chunk while they multiply this
one; only where a wave owns two chunks or more does that prefetch, and the rotation of the
registers after it, do anything.  decode_chunks() restates the split, and test_linear_host.py
checks that the cases reach every loop with two or three chunks per wave.  The exact cases with
n > 2048 take x from -1..1 (the sums of absolute terms must stay below 2^24 units).  Two faults
model the loop going wrong over wave 0's second chunk: "drop_chunk" (the chunk contributes
nothing) and "stale_x" (its weights meet the x of the wave's first chunk: a missing rotation);
"drop_R_chunk" / "stale_x_R" are the same in the z product and "drop_L_chunk" in the fp16-L loop.
Against the bar of a random case a whole chunk is small: the signal of CK random terms grows like
sqrt(CK) and the bar like n 2^-24 times the n + n r terms of A, so with plain random data these
faults measure 0.2 to 12 bars at n = 2600 and 0.2 to 5 at n = 8454.  The random long cases therefore
plant one output that hangs on the chunk without cancellation: over wave 0's second chunk row 0 of
the codes is k sign(x[0]) and row 0 of R is 0.3 sign(x[0]) (where the z product has a second
chunk), and row 0 of L is 0.45 e_0, so y[0, 0] is the code sum plus one z.
"""
from dataclasses import dataclass

import numpy as np

from weight_stride_cases import pack_codes

f16, f32, f64 = np.float16, np.float32, np.float64

DECODE_MAX_TOKENS = 16
# the decode split of csrc/cq_linear.hip (kDecodeWaves, kDecodeWavesZ, kDecodeSplitZ), restated
DECODE_WAVES, DECODE_WAVES_Z, DECODE_SPLIT_Z = 8, 2, 16
LONG_N = 2048


@dataclass(frozen=True)
class Case:
    kind: str       # "exact" | "exact16" | "random"
    m: int
    n: int
    r: int
    bits: int
    T: int
    bias: bool = False

    @property
    def id(self):
        return f"{self.kind}-m{self.m}n{self.n}r{self.r}b{self.bits}T{self.T}" + ("-bias" if self.bias else "")

    @property
    def k(self):
        return 2 ** (self.bits - 1) - 1

    @property
    def seed(self):
        return (self.m * 1000003 + self.n * 1009 + self.r * 101 + self.bits * 11 + self.T
                + {"exact": 0, "exact16": 1, "random": 2}[self.kind] * 7919)


_SHAPES = ([(33, 64, 8, b, T) for b in (2, 4) for T in (1, 5)]
           + [(48, 198, 40, b, T) for b in (2, 4) for T in (3, 16)]
           + [(80, 898, 200, b, T) for b in (2, 4) for T in (16, 17, 64)]
           + [(272, 512, 16, 2, 130)]
           + [(48, 198, 0, 2, T) for T in (3, 17)]
           # decode K loops past one chunk per wave, see the module docstring
           + [(48, 2600, 40, b, T) for b in (2, 4) for T in (1, 16)]
           + [(33, 8454, 40, b, T) for b in (2, 4) for T in (5, 16)]
           + [(48, 198, 264, b, T) for b in (2, 4) for T in (5, 16)])

EXACT = [Case("exact", *s) for s in _SHAPES] + [Case("exact", 33, 64, 8, 4, 5, bias=True)]
EXACT16 = [Case("exact16", 33, 64, 8, b, T) for b in (2, 4) for T in (1, 5, 17)]
RANDOM = [Case("random", *s) for s in _SHAPES] + [Case("random", 33, 64, 8, 2, 5, bias=True)]
ALL = EXACT + EXACT16 + RANDOM


def row_bytes(n, bits):
    """Bytes per row of the inference layout (rows padded to 16 bytes)."""
    return -(-(n * bits) // 128) * 16


def inference_codes(c, bits):
    """(m, n) codes -> (m, row_bytes) uint8 inference layout, the tail holding code 0."""
    m, n = c.shape
    rb = row_bytes(n, bits)
    full = np.zeros((m, rb * 8 // bits), dtype=np.int8)
    full[:, :n] = c
    return pack_codes(full, bits).reshape(m, rb)


def storage_codes(c, bits):
    """(m, n) codes -> flat storage-layout bytes on the (m, n padded to 4) grid and n_padded."""
    m, n = c.shape
    npad = n + (-n) % 4
    full = np.zeros((m, npad), dtype=np.int8)
    full[:, :n] = c
    return pack_codes(full, bits), npad


def chunk_k(width):
    """k per chunk of a K loop over rows of `width` bits (2 | 4 | 16): a lane's 16-byte loads."""
    return 256 if width == 2 else 128


def decode_chunks(case, waves=DECODE_WAVES, waves_z=DECODE_WAVES_Z, split_z=DECODE_SPLIT_Z):
    """{loop: (most, fewest)} chunks that one wave takes in the decode loops the case runs
    ({} for a prefill case).  Loops: "codes2" / "codes4" the layer's codes, "z128" the z product
    with fp16 or 4-bit R, "z256" with 2-bit R, "L16" the L product with fp16 L.  Chunk c of a loop
    goes to slot c mod slots; the slots are the workgroup's waves (codes, L) or the waves of all
    the workgroups that share 16 rows of R (z).  Works for the cases of linear_factor_cases.py too."""
    if case.T > DECODE_MAX_TOKENS:
        return {}
    lb, rb = getattr(case, "lb", 16), getattr(case, "rb", 16)

    def per_wave(nchunks, slots):
        return -(-nchunks // slots), nchunks // slots

    out = {f"codes{case.bits}": per_wave(-(-case.n // chunk_k(case.bits)), waves)}
    if case.r > 0:
        out[f"z{chunk_k(rb)}"] = per_wave(-(-case.n // chunk_k(rb)), waves_z * split_z)
        if lb == 16:
            out["L16"] = per_wave(-(-case.r // 32), waves)
    return out


def second_chunk(case, width, slots):
    """Columns [lo, hi) of the second chunk of the first slot of a decode K loop over n, or None."""
    lo = slots * chunk_k(width)
    if case.T > DECODE_MAX_TOKENS or case.n <= lo:
        return None
    return lo, min(lo + chunk_k(width), case.n)


def _sign(v):
    return np.where(v.astype(f64) >= 0, 1.0, -1.0)


_CACHE = {}


def inputs(case: Case):
    """dict(x (T, n) f16, c (m, n) int8, L (m, r) f16, R (r, n) f16, s, gs (f32), bias (m,) f32 | None);
    built once per case and shared (treat as read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(case.seed)
    m, n, r, k, T = case.m, case.n, case.r, case.k, case.T
    c = rng.integers(-k, k + 1, (m, n)).astype(np.int8)
    if case.kind == "random":
        x = rng.standard_normal((T, n)).astype(f16)
        L = (0.15 * rng.standard_normal((m, r))).astype(f16)
        R = (0.15 * rng.standard_normal((r, n))).astype(f16)
        s, gs = f32(0.05), f32(1.7)
        bias = rng.standard_normal(m).astype(f32) if case.bias else None
    else:
        xa, la = (4, 2) if case.kind == "exact" else (1, 1)
        if case.n > LONG_N:
            xa = 1
        x = rng.integers(-xa, xa + 1, (T, n)).astype(f16)
        L = rng.integers(-la, la + 1, (m, r)).astype(f16)
        R = rng.integers(-la, la + 1, (r, n)).astype(f16)
        s, gs = f32(k / 2), f32(4.0)
        bias = (rng.integers(-8, 9, m) * 0.5).astype(f32) if case.bias else None
    big = np.abs(x.astype(f64)).max()
    for (t, j) in ((0, 0), (0, n - 1)) + (((1, 0),) if T > 1 else ()):
        x[t, j] = f16(big if x[t, j] >= 0 else -big)
    if case.kind == "random" and case.n > LONG_N and case.T <= DECODE_MAX_TOKENS:
        # y[0, 0] hangs on wave 0's second chunk without cancellation, see the module docstring
        lo, hi = second_chunk(case, case.bits, DECODE_WAVES)
        c[0, lo:hi] = (k * _sign(x[0, lo:hi])).astype(np.int8)
        L[0, :] = 0
        L[0, 0] = f16(0.45)
        zc = second_chunk(case, 16, DECODE_WAVES_Z * DECODE_SPLIT_Z)
        if zc:
            R[0, zc[0]:zc[1]] = (0.3 * _sign(x[0, zc[0]:zc[1]])).astype(f16)
    out = dict(x=x, c=c, L=L, R=R, s=s, gs=gs, bias=bias)
    _CACHE[case] = out
    return out


LOOP_FAULTS = ("drop_chunk", "stale_x", "drop_R_chunk", "stale_x_R", "drop_L_chunk")
FAULTS = ("flip_last", "flip_first", "swap_L", "drop_R_last", "drop_gs", "s_for_sk", "pad_code") + LOOP_FAULTS


def fault_applies(case: Case, fault: str) -> bool:
    if fault in ("drop_chunk", "stale_x"):      # a wave of the code product has a second chunk
        return second_chunk(case, case.bits, DECODE_WAVES) is not None
    if fault in ("drop_R_chunk", "stale_x_R"):  # ... of the z product
        return case.r > 0 and second_chunk(case, 16, DECODE_WAVES_Z * DECODE_SPLIT_Z) is not None
    if fault == "drop_L_chunk":                 # ... of the fp16-L product (chunks of 32 columns of z)
        return case.T <= DECODE_MAX_TOKENS and case.r > DECODE_WAVES * 32
    if fault in ("flip_last", "flip_first", "pad_code") and case.kind == "random" and case.n * case.r > 10000:
        # one code against the bar: A's factor part has n r terms, so |x| dc over A falls like 1 / (n r)
        # while the bar's (n + r + 32) 2^-24 grows; ten bars hold with room up to n r ~ 10^4 (the rule
        # of linear_factor_cases.py), and at (48, 198, 264) a flip measures 6 to 23
        return False
    if fault in ("swap_L", "drop_R_last"):
        return case.r > 0
    if fault == "s_for_sk":
        return case.bits == 4
    if fault == "pad_code":  # a pad column exists and x's buffer holds a finite value there
        return row_bytes(case.n, case.bits) * 8 // case.bits > case.n and case.T > 1
    return True


def _flip(v, k):
    return -v if v != 0 else k


def reference(case: Case, fault: str | None = None):
    """(y64, bar): the fp64 reference (T, m) and the elementwise bar of the random cases.
    fault: one planted error (FAULTS), for checking that the cases can see it.  "pad_code"
    models a nonzero code in row 0's first pad column meeting what a contiguous x holds
    there: the first element of the next row.  The loop faults act on wave 0's second chunk:
    "drop_chunk" / "stale_x" on row 0 of the codes (the chunk contributes nothing / meets the x of
    columns 0 ...), "drop_R_chunk" / "stale_x_R" on all of R in the z product, "drop_L_chunk" on
    row 0 of L over columns 256 ... 287 of z."""
    d = inputs(case)
    x, L, R = d["x"].astype(f64), d["L"].astype(f64), d["R"].astype(f64)
    c = d["c"].astype(f64)
    k = f32(case.k)
    sk = f64(d["s"] / k)        # one fp32 division
    gs = f64(d["gs"])
    if fault == "flip_last":
        c[-1, -1] = _flip(c[-1, -1], case.k)
    elif fault == "flip_first":
        c[0, 0] = _flip(c[0, 0], case.k)
    elif fault == "swap_L":
        L[[0, 1]] = L[[1, 0]]
    elif fault == "drop_R_last":
        R[-1] = 0
    elif fault == "drop_gs":
        gs = f64(1.0)
    elif fault == "s_for_sk":
        sk = f64(d["s"])
    elif fault == "drop_L_chunk":
        L[0, DECODE_WAVES * 32:(DECODE_WAVES + 1) * 32] = 0
    code = x @ c.T
    if fault == "pad_code":
        code[:-1, 0] += x[1:, 0] * case.k
    elif fault in ("drop_chunk", "stale_x"):
        lo, hi = second_chunk(case, case.bits, DECODE_WAVES)
        code[:, 0] -= x[:, lo:hi] @ c[0, lo:hi]
        if fault == "stale_x":
            code[:, 0] += x[:, :hi - lo] @ c[0, lo:hi]
    z = x @ R.T
    if fault in ("drop_R_chunk", "stale_x_R"):
        lo, hi = second_chunk(case, 16, DECODE_WAVES_Z * DECODE_SPLIT_Z)
        z -= x[:, lo:hi] @ R[:, lo:hi].T
        if fault == "stale_x_R":
            z += x[:, :hi - lo] @ R[:, lo:hi].T
    lr = z @ L.T
    y = gs * (sk * code + lr)
    if d["bias"] is not None:
        y = y + d["bias"].astype(f64)
    A = f64(d["gs"]) * (f64(d["s"] / k) * (np.abs(x) @ np.abs(d["c"].astype(f64)).T)
                        + (np.abs(x) @ np.abs(d["R"].astype(f64)).T) @ np.abs(d["L"].astype(f64)).T)
    bar = (case.n + case.r + 32) * 2.0 ** -24 * A
    return y, bar
