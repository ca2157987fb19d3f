"""Every launch form of csrc/cq_quant.hip's uniform quantiser, dequantiser, code unpacker and RMS
scaler as one case each: tests/test_gpu_quant_forms.py runs the kernels on them,
tests/test_quant_forms_host.py checks on the host that each case reaches the form it names.

A case is (id, entry, a: its arguments, kernel: the kernel the host code launches for them,
traits: the loop forms inside that kernel that the shape is meant to reach, cond: the dispatch
condition in words).  No torch, no device: inputs come from a generator seeded by the case id,
references from the CPU oracle (oracle.caldera_oracle) and the packing order from
weight_stride_cases.pack_codes.

The dispatch predicates below restate the host code of cq_quant.hip from its numbers (kThreads
256, waves of 64, kMaxGrid 2048, 4096-element wave-per-block limit, 1024-element dequantise
chunks, 16 codes per unpack step, 8 elements per RMS step).  Alignment is passed as the byte
offset of a pointer from a 16-byte boundary.

`python tests/quant_form_cases.py` prints the table of DESIGN.md section 6.1 ("Kernel forms of
cq_quant.hip"); the host test holds the document to it."""
import os
import sys
import zlib

import numpy as np

if __name__ == "__main__":      # run as a script: the oracle package lives one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import caldera_oracle as O
from weight_stride_cases import pack_codes, werr

f16, f32, f64 = np.float16, np.float32, np.float64
EPS = f32(1e-8)
K_THREADS, WAVE, K_MAX_GRID = 256, 64, 2048
BLOCK_PATH_MAX = 4096          # quant_block_kernel: block_size <= 4096 and no error output
BLOCK_GRID_MAX = 4096          # its grid cap; kThreads / 64 = 4 waves (blocks) per workgroup


# ------------------------------------------------------------------------------ dispatch predicates
def ceil_div(a, b):
    return -(-a // b)


def grid_for(work, batch):
    """grid_for of cq_quant.hip: work / 1024 workgroups, capped at max(2048 / batch, 64)."""
    cap = max(max(1, K_MAX_GRID // max(1, batch)), 64)
    return max(1, min(ceil_div(work, K_THREADS * 4), cap))


def block_grid(nbt):
    """Workgroups of the wave-per-block kernel for nbt blocks in all."""
    return max(1, min(ceil_div(nbt, K_THREADS // WAVE), BLOCK_GRID_MAX))


def small_blocks(bs, err):
    return bs <= BLOCK_PATH_MAX and not err


def v16(total, bs, bits, packed, out_off, codes_off):
    """cq_dequant_uniform takes dequant16_kernel."""
    return total % 1024 == 0 and bs % 1024 == 0 and out_off % 16 == 0 and bits <= 8 and (packed or codes_off % 4 == 0)


def unpack16(ncodes, bits, codes_off, packed_off):
    """cq_unpack_codes takes unpack16_kernel."""
    return ncodes % 16 == 0 and codes_off % 16 == 0 and packed_off % (4 if bits == 2 else 8) == 0


def v8(numel, off):
    """cq_rms_scale takes rms_partial8_kernel."""
    return numel % 8 == 0 and off % 16 == 0


def _tf(b):
    return "true" if b else "false"


def known_kernel(bits, packed, err):
    return f"quant_known_kernel<{bits}, {_tf(packed and bits <= 4)}, {_tf(err)}>"


def quantize_kernel(bs, bits, packed, err):
    """The kernels cq_quantize_uniform launches."""
    if small_blocks(bs, err):
        return f"quant_block_kernel<{bits}>"
    return "absmax_atomic_kernel + " + known_kernel(bits, packed, err)


def dequant_kernel(total, bs, bits, fmt, out_off, codes_off):
    f = {"int8": 0, "int16": 1, "packed": 2}[fmt]
    name = "dequant16_kernel" if v16(total, bs, bits, fmt == "packed", out_off, codes_off) else "dequant_kernel"
    return f"{name}<{bits}, {f}>"


def unpack_kernel(ncodes, bits, codes_off, packed_off):
    return ("unpack16_kernel" if unpack16(ncodes, bits, codes_off, packed_off) else "unpack_kernel") + f"<{bits}>"


def rms_kernel(dtype, numel, off):
    dt = {f16: "CQ_F16", f32: "CQ_F32"}[dtype]
    return ("rms_partial8_kernel" if v8(numel, off) else "rms_partial_kernel") + f"<{dt}>"


# Loop forms inside the quantise kernels, as predicates of (B, numel, bs, bits, err)
def _absmax_switches(B, numel, bs):
    """A thread of absmax_atomic_kernel meets two blocks on consecutive grid-stride steps."""
    stride = grid_for(numel, B) * K_THREADS
    i = np.arange(0, max(0, min(stride, numel - stride)), dtype=np.int64)
    return bool(((i // bs) != ((i + stride) // bs)).any())


TRAITS = {
    # wave-per-block kernel
    "short_block": lambda B, numel, bs, bits, err: small_blocks(bs, err) and bs < WAVE,
    "byte_per_block": lambda B, numel, bs, bits, err: small_blocks(bs, err) and bs * bits == 8,
    "ragged_lanes": lambda B, numel, bs, bits, err: small_blocks(bs, err) and bs > WAVE and bs % WAVE != 0,
    "path_edge": lambda B, numel, bs, bits, err: small_blocks(bs, err) and bs == BLOCK_PATH_MAX,
    "wave_stride": lambda B, numel, bs, bits, err: (small_blocks(bs, err) and
                                                   B * (numel // bs) > block_grid(B * (numel // bs)) * (K_THREADS // WAVE)),
    "unpackable": lambda B, numel, bs, bits, err: small_blocks(bs, err) and bs % 4 != 0,
    # large-block path
    "first_past_edge": lambda B, numel, bs, bits, err: bs == BLOCK_PATH_MAX + 4,
    "multi_block": lambda B, numel, bs, bits, err: not small_blocks(bs, err) and numel // bs > 1,
    "single": lambda B, numel, bs, bits, err: not small_blocks(bs, err) and numel // bs == 1,
    "cur_switch": lambda B, numel, bs, bits, err: (not small_blocks(bs, err) and numel // bs > 1 and
                                                  _absmax_switches(B, numel, bs)),
    "forced_by_err": lambda B, numel, bs, bits, err: bs <= BLOCK_PATH_MAX and err,
    "grid_capped": lambda B, numel, bs, bits, err: (not small_blocks(bs, err) and
                                                   numel // 4 > grid_for(numel, B) * K_THREADS),
    "short4_store": lambda B, numel, bs, bits, err: not small_blocks(bs, err) and bits == 16 and numel // bs > 1,
}


# ------------------------------------------------------------------------------ inputs
def _seed(name):
    return zlib.crc32(name.encode())


SMALL_NEG = f32(2.0 ** -20)    # -max 2^-20: |scaled| <= 32767 / 2^20 < 0.5, so code 0 at every bit width


def block_values(rng, bs, j):
    """One block of bs fp32 values around ordinary ones at a scale of the block's own: the block
    maximum M at both signs, the exact ties +-M / 2 ((x / M) k = +-k / 2, a tie for every odd k),
    a small negative that rounds to code 0 and -0.0, at random places.  A block of 8 or more
    holds all of them; a shorter one holds the maximum (its sign alternates with the block index
    j) and a run of the others that rotates with j, and keeps at least one ordinary value."""
    x = (rng.standard_normal(bs) * rng.uniform(0.1, 10.0)).astype(f32)
    M = f32(f32(1.25) * np.abs(x).max())
    sg = f32(1.0 if j % 2 == 0 else -1.0)
    others = [-sg * M, M / f32(2), -M / f32(2), -M * SMALL_NEG, f32(-0.0)]
    if bs >= 8:
        vals = [sg * M] + others
    else:
        n = max(0, min(bs - 2, len(others)))
        vals = [sg * M] + [others[(j * n + t) % len(others)] for t in range(n)]
    x[rng.permutation(bs)[:len(vals)]] = np.asarray(vals, dtype=f32)
    return x


def quant_input(name, B, numel, bs):
    """(B, numel) fp32 of numel / bs blocks per matrix (block_values), from a seed of the name."""
    rng = np.random.default_rng(_seed(name))
    nbt = B * (numel // bs)
    return np.stack([block_values(rng, bs, j) for j in range(nbt)]).reshape(B, numel)


ZERO_BLOCK, TINY_BLOCK, NAN_BLOCK = (0, 1), (0, 2), (1, 1)     # (matrix, block) of the edge input


def edge_input(name):
    """B = 2, numel = 256, bs = 64 (four blocks a matrix): matrix 0 block 1 is all zero with both
    signs of zero, matrix 0 block 2 has max 1e-9 (below eps), matrix 1 block 1 holds one NaN;
    the other five blocks are block_values.  No infinities."""
    x = quant_input(name, 2, 256, 64).reshape(2, 4, 64)
    x[ZERO_BLOCK] = 0.0
    x[ZERO_BLOCK][1::2] = -0.0
    t = x[TINY_BLOCK]
    x[TINY_BLOCK] = (t / np.abs(t).max() * f32(1e-9)).astype(f32)
    x[NAN_BLOCK][17] = np.nan
    assert not np.isinf(x).any()
    return x.reshape(2, 256)


def err_weights(name, B, n):
    """(B, n) positive fp32 column weights 10^u, u ~ U[-2, 1], at a scale of each row's own."""
    rng = np.random.default_rng(_seed(name + "/w"))
    return np.stack([(1.0, 7.0, 0.13)[b % 3] * 10.0 ** rng.uniform(-2.0, 1.0, n) for b in range(B)]).astype(f32)


def unpack_np(packed, bits):
    """The inverse of pack_codes: int8 codes of offset-binary, MSB-first packed bytes."""
    k, per = 2 ** (bits - 1) - 1, 8 // bits
    p = np.asarray(packed, dtype=np.uint8).reshape(-1, 1).astype(np.int32)
    sh = np.asarray([bits * (per - 1 - t) for t in range(per)], dtype=np.int32)
    return (((p >> sh[None, :]) & (2 ** bits - 1)) - k).astype(np.int8).reshape(-1)


# ------------------------------------------------------------------------------ the cases
class Args(dict):
    __getattr__ = dict.__getitem__


class Case:
    def __init__(self, id, entry, a, kernel, cond, traits=(), group=None):
        self.id, self.entry, self.a, self.kernel, self.cond, self.traits, self.group = \
            id, entry, Args(a), kernel, cond, tuple(traits), group
        self._inp = self._ref = None

    @property
    def inp(self):
        """The case's inputs (numpy; built on first use, shared by the tests, never written)."""
        if self._inp is None:
            self._inp = _INPUTS[self.entry](self)
            for v in self._inp.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return self._inp

    @property
    def ref(self):
        if self._ref is None:
            self._ref = _REFS[self.entry](self)
        return self._ref


def _oracle_quant(x, bits, bs, B):
    """The oracle's codes, scale and dequantised values of x (B, numel), plus the packed codes
    where a block packs.  A NaN's int8 code is unspecified (numpy warns): silenced here, and the
    tests leave those codes out."""
    numel = x.shape[1]
    with np.errstate(invalid="ignore"):
        c, s = O.quantize_uniform(x.reshape(-1), bits, bs)
        d = O.dequantize_uniform(c, s, bits, (B, numel))
    out = {"codes": c.reshape(B, numel), "scale": s.reshape(B, numel // bs), "deq": d}
    if bits <= 4 and bs % 4 == 0:
        out["packed"] = pack_codes(c.reshape(-1), bits).reshape(B, numel * bits // 8)
    return out


def _quant_inputs(c):
    a = c.a
    inp = {"x": edge_input(c.group) if a.edge else quant_input(c.group, a.B, a.numel, a.bs)}
    if a.err in ("shared", "rows"):
        w = err_weights(c.group, a.B, a.ncols)
        inp["w"] = w[1] if a.err == "shared" else w
    return inp


def _quant_ref(c):
    a, x = c.a, c.inp["x"]
    out = _oracle_quant(x, a.bits, a.bs, a.B)
    if a.err:
        w = c.inp.get("w", np.ones(1, dtype=f32))
        with np.errstate(invalid="ignore"):
            out["err"] = np.asarray([werr(out["deq"][b], x[b], w if w.ndim == 1 else w[b], w.shape[-1])
                                     for b in range(a.B)])
    out["nan_blocks"] = np.isnan(x.reshape(a.B, -1, a.bs)).any(axis=2)
    return out


def _known_inputs(c):
    a = c.a
    x = quant_input(c.group, a.B, a.numel, 64)
    return {"x": x, "mx": (np.abs(x).max(axis=1) * f32(a.factor)).astype(f32)}


def _known_ref(c):
    """The oracle on each matrix with the given maximum appended as one more element of its single
    block, so that the oracle's own maximum is the given one; that element's outputs are dropped."""
    a, x, mx = c.a, c.inp["x"], c.inp["mx"]
    outs = [_oracle_quant(np.append(x[b], mx[b])[None, :], a.bits, a.numel + 1, 1) for b in range(a.B)]
    codes = np.stack([o["codes"][0, :-1] for o in outs])
    return {"codes": codes, "deq": np.stack([o["deq"][0, :-1] for o in outs]), "scale": mx.reshape(a.B, 1),
            "packed": pack_codes(codes.reshape(-1), a.bits).reshape(a.B, -1),
            "nan_blocks": np.zeros((a.B, 1), dtype=bool)}


def _dequant_inputs(c):
    """Oracle codes and scales of a quant_input; the group (total, bs, bits) shares them, so the
    int8 and the packed form, aligned or not, see equal values."""
    a = c.a
    q = _oracle_quant(quant_input(c.group, 1, a.total, a.bs), a.bits, a.bs, 1)
    return {"codes": q["packed"][0] if a.fmt == "packed" else q["codes"][0], "scale": q["scale"][0],
            "int_codes": q["codes"][0]}


def _dequant_ref(c):
    a = c.a
    return {"out": O.dequantize_uniform(c.inp["int_codes"].reshape(-1, a.bs), c.inp["scale"].reshape(-1, 1), a.bits,
                                        (a.total,))}


def _unpack_inputs(c):
    """Random bytes: every field value, the quantiser's unused top code (k + 1) included."""
    a = c.a
    rng = np.random.default_rng(_seed(c.group))
    return {"packed": rng.integers(0, 256, (a.B, a.numel * a.bits // 8), dtype=np.uint8)}


def _unpack_ref(c):
    return {"codes": unpack_np(c.inp["packed"], c.a.bits).reshape(c.a.B, c.a.numel)}


def _rms_inputs(c):
    """Two matrices at scales 0.02 and 1.3 (fp16: squares of the first reach fp16's subnormals)."""
    a = c.a
    rng = np.random.default_rng(_seed(c.group))
    W = rng.standard_normal((2,) + tuple(a.shape)) * np.asarray([0.02, 1.3])[:, None, None]
    return {"W": W.astype(a.dtype)}


def _rms_ref(c):
    W = c.inp["W"]
    gs = [O.global_scale_of(W[b]) for b in range(2)]
    return {"gs": np.asarray(gs, dtype=f64), "Ws": np.stack([O.scale_weight(W[b], gs[b]) for b in range(2)])}


_INPUTS = {"quantize_uniform": _quant_inputs, "quantize_known_max": _known_inputs, "dequantize_uniform": _dequant_inputs,
           "unpack_codes": _unpack_inputs, "rms_scale": _rms_inputs}
_REFS = {"quantize_uniform": _quant_ref, "quantize_known_max": _known_ref, "dequantize_uniform": _dequant_ref,
         "unpack_codes": _unpack_ref, "rms_scale": _rms_ref}


def _q(tag, B, numel, bs, bits, traits, *, err=None, ncols=None, outputs=None, edge=False):
    """cq_quantize_uniform.  err: None, "plain" (want_err, no weights), "shared" ((n,) weights) or
    "rows" ((B, n) weights).  outputs: what the call asks for besides scale (default: all)."""
    packs = bits <= 4 and bs % 4 == 0
    outputs = outputs or (("codes", "deq") + (("packed",) if packs else ()))
    a = dict(B=B, numel=numel, bs=bs, bits=bits, err=err, ncols=ncols, edge=edge, outputs=tuple(outputs),
             packed="packed" in outputs)
    cid = f"q-{tag}-B{B}-n{numel}-bs{bs}-b{bits}" + (f"-err_{err}" if err else "")
    path = "bs <= 4096, no err" if small_blocks(bs, bool(err)) else ("bs > 4096" if bs > BLOCK_PATH_MAX else "err wanted")
    cond = path + ("; " + ", ".join(traits) if traits else "")
    # the input depends on the shape alone, so the forms of one shape see equal values
    return Case(cid, "quantize_uniform", a, quantize_kernel(bs, bits, a["packed"], bool(err)), cond, traits,
                group=f"q-{'edge' if edge else tag}-{B}-{numel}-{bs}")


def _known(bits):
    a = dict(B=2, numel=4096, bits=bits, factor=1.5, err=None, bs=4096)
    return Case(f"known-B2-n4096-b{bits}", "quantize_known_max", a, known_kernel(bits, True, False),
                "given max 1.5 x the data's; nb == 1", ("single",), group="known-2-4096")


def _dq(tag, total, bs, bits, fmt, out_off=0, codes_off=0):
    kern = dequant_kernel(total, bs, bits, fmt, out_off, codes_off)
    why = {"vector": "total, bs % 1024 == 0, aligned", "bs512": "bs % 1024 != 0", "total4032": "total % 1024 != 0",
           "bits16": "bits > 8", "out+4": "out 4 bytes off 16", "codes+1": "int8 codes 1 byte off 4"}[tag]
    return Case(f"dq-{tag}-n{total}-bs{bs}-b{bits}-{fmt}", "dequantize_uniform",
                dict(total=total, bs=bs, bits=bits, fmt=fmt, out_off=out_off, codes_off=codes_off), kern, why,
                group=f"dq-{total}-{bs}-{bits}")


def _up(tag, B, numel, bits, out_off=0, packed_off=0):
    why = {"n20": "ncodes % 16 != 0", "B3n16": "ncodes = 48, aligned", "n4096": "aligned", "out+1": "codes 1 byte off 16",
           "packed+1": "packed 1 byte off 4 / 8"}[tag]
    return Case(f"up-{tag}-B{B}-n{numel}-b{bits}", "unpack_codes",
                dict(B=B, numel=numel, bits=bits, out_off=out_off, packed_off=packed_off),
                unpack_kernel(B * numel, bits, out_off, packed_off), why, group=f"up-{B}-{numel}-{bits}")


def _rms(dtype, shape, off):
    """off: elements between a 16-byte boundary and the first of W."""
    numel = shape[0] * shape[1]
    nm = np.dtype(dtype).name
    why = "numel % 8 != 0" if numel % 8 else ("W one element off 16 bytes" if off else "numel % 8 == 0, aligned")
    return Case(f"rms-{nm}-{shape[0]}x{shape[1]}" + (f"-off{off}" if off else ""), "rms_scale",
                dict(dtype=dtype, shape=shape, off=off, numel=numel),
                rms_kernel(dtype, numel, off * np.dtype(dtype).itemsize), why, group=f"rms-{nm}-{shape[0]}x{shape[1]}")


def _cases():
    cs = []
    # wave-per-block kernel: no error output
    cs += [_q("short", 3, 48, 4, b, ("short_block",) + (("byte_per_block",) if b == 2 else ())) for b in (2, 4, 8, 16)]
    cs += [_q("ragged", 2, 192, 96, b, ("ragged_lanes",)) for b in (2, 4, 8, 16)]
    cs += [_q("longest-ragged", 2, 8184, 4092, b, ("ragged_lanes",)) for b in (2, 4)]
    cs += [_q("edge-of-path", 1, 8192, 4096, b, ("path_edge",)) for b in (2, 16)]
    cs += [_q("wave-stride", 2, 32800, 4, b, ("wave_stride", "short_block")) for b in (2, 4)]
    cs += [_q("unpackable", 1, 36, 6, b, ("unpackable", "short_block")) for b in (4, 8)]
    # large-block path
    cs += [_q("past-edge", 2, 12300, 4100, b, ("first_past_edge", "multi_block", "cur_switch") +
              (("short4_store",) if b == 16 else ())) for b in (2, 4, 8, 16)]
    cs += [_q("past-edge", 2, 12300, 4100, b, ("first_past_edge", "multi_block", "cur_switch"), err=e, ncols=100)
           for b in (2, 8) for e in ("shared", "rows")]
    cs += [_q("err-forced", 2, 64, bs, b, ("forced_by_err", "multi_block"), err="plain") for bs in (4, 8) for b in (2, 4)]
    cs += [_q("grid-cap", 32, 65552, 16388, 2, ("grid_capped", "multi_block", "cur_switch"), err="plain",
              outputs=("packed",))]
    cs += [_known(b) for b in (2, 4)]
    # edge values, on both paths
    cs += [_q("edge-values", 2, 256, 64, b, ("forced_by_err", "multi_block") if e else (), err=e, edge=True)
           for e in (None, "plain") for b in (2, 4, 8, 16)]
    # dequantise
    cs += [_dq("vector", 4096, 1024, b, "int8") for b in (2, 4, 8)] + [_dq("vector", 4096, 1024, b, "packed") for b in (2, 4)]
    cs += [_dq("bs512", 4096, 512, 8, "int8"), _dq("bs512", 4096, 512, 4, "packed")]
    cs += [_dq("total4032", 4032, 64, 2, "int8"), _dq("total4032", 4032, 64, 2, "packed")]
    cs += [_dq("bits16", 4096, 1024, 16, "int16")]
    cs += [_dq("out+4", 4096, 1024, b, "int8", out_off=4) for b in (2, 4, 8)]
    cs += [_dq("out+4", 4096, 1024, b, "packed", out_off=4) for b in (2, 4)]
    cs += [_dq("codes+1", 4096, 1024, b, "int8", codes_off=1) for b in (2, 4, 8)]
    # unpack
    for b in (2, 4):
        cs += [_up("n20", 1, 20, b), _up("B3n16", 3, 16, b), _up("n4096", 1, 4096, b),
               _up("out+1", 1, 4096, b, out_off=1), _up("packed+1", 1, 4096, b, packed_off=1)]
    # RMS scale
    cs += [_rms(dt, sh, off) for dt in (f16, f32) for sh, off in (((33, 20), 0), ((8, 16), 0), ((8, 16), 1))]
    return cs


CASES = {c.id: c for c in _cases()}
assert len(CASES) == len(_cases()), "case ids are unique"


def case(cid):
    return CASES[cid]


def ids(entry=None):
    return [cid for cid, c in CASES.items() if entry is None or c.entry == entry]


def groups(entry):
    """The case ids of an entry by group (cases of a group run on equal values), groups of two or more."""
    g = {}
    for cid in ids(entry):
        g.setdefault(CASES[cid].group, []).append(cid)
    return {k: v for k, v in g.items() if len(v) > 1}


ENTRY_NAMES = {"quantize_uniform": "cq_quantize_uniform", "quantize_known_max": "cq_quantize_uniform_known_max",
               "dequantize_uniform": "cq_dequant_uniform", "unpack_codes": "cq_unpack_codes", "rms_scale": "cq_rms_scale"}


def design_table():
    """The "kernel forms of cq_quant.hip" table of DESIGN.md, one row per case."""
    rows = ["| entry | condition | kernel | case |", "|---|---|---|---|"]
    rows += [f"| `{ENTRY_NAMES[c.entry]}` | {c.cond} | `{c.kernel}` | `{c.id}` |" for c in CASES.values()]
    return "\n".join(rows)


if __name__ == "__main__":
    print(design_table())
