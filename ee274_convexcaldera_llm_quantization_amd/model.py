"""Layer-replacement caller: the reference's `apply_CALDERA_quantization`
(`main.py:135-251`) on the MI355X engine.

The reference walks `model.named_modules()`, and for each selected language-model
projection forms `H = diag_embed(Hall[name])` (main.py:163-165), runs `caldera()` with the
driver's parameters (main.py:167-182, `scale_W=False`), writes `out = Q + L @ R` back into
the module (main.py:199-202), and undoes the write when the relative Frobenius error
`||W - out|| / ||W||` exceeds `error_threshold` (main.py:212-220).  Everything else with a
weight is counted as unquantised language or vision parameters (main.py:242-251), and the
bit accounting of main.py:321-329 is reported.

Here the selection and accounting are the reference's (including its substring layer match,
`any(f'layers.{i}' in name ...)`, main.py:158), the Hessian diagonal is passed as a vector
(no n x n diag_embed), `Q + L R` is one fused HIP GEMM epilogue, and the Hadamard branch
(main.py:224-240, `H1 W H2` with normalised Sylvester matrices padded to powers of two) runs
as HIP GEMMs on the device instead of numpy on the host.  Layers that share a shape are
decomposed in one lockstep batch, each with its own Hessian diagonal (the engine reads
per-matrix weights at a batch stride; api.caldera_batch groups by code-path flags and
interleaves the groups on HIP streams), where the reference runs one caldera() per layer.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Callable, Sequence

import torch

from . import _lib as K

PROJ_KEYS = ("mlp.up_proj", "mlp.down_proj", "mlp.gate_proj", "q_proj", "k_proj", "v_proj", "o_proj")


@dataclass
class LayerSelection:
    """main.py:1-7, 147-160: which modules are decomposed."""
    scope: str = "language"                         # `'language' in name` (main.py:150)
    keys: Sequence[str] = PROJ_KEYS                 # main.py:155
    layers: Sequence[int] | None = tuple(range(17, 24))  # quantize_layer_start..end (main.py:2-4)
    min_dim: int = 500                              # both dims > 500 (main.py:157-158)
    limit: int = 10000                              # quantized_layer_limit (main.py:6)

    def in_scope(self, name: str, module) -> bool:
        return hasattr(module, "weight") and module.weight is not None and self.scope in name

    def selects(self, name: str, weight: torch.Tensor, counter: int) -> bool:
        return (any(k in name for k in self.keys)
                and weight.dim() == 2 and weight.size(0) > self.min_dim and weight.size(1) > self.min_dim
                and (self.layers is None or any(f"layers.{i}" in name for i in self.layers))
                and counter <= self.limit)


def driver_params(rank: int = 200):
    """The CalderaParams main.py:167-182 builds for every layer."""
    from .src.caldera.utils.dataclasses import CalderaParams
    from .src.caldera.utils.quantization import QuantizerFactory
    return CalderaParams(compute_quantized_component=True, compute_low_rank_factors=True, Q_bits=2,
                         L_bits=16, R_bits=16, rank=rank, iters=5, lplr_iters=5, activation_aware_LR=True,
                         update_order=["Q", "LR"],
                         quant_factory_Q=QuantizerFactory(method="uniform", block_size=64),
                         quant_factory_LR=QuantizerFactory(method="uniform", block_size=64),
                         rand_svd=False, sigma_reg=1e-8)


@dataclass
class LayerOutcome:
    name: str
    shape: tuple
    rel_error: float          # ||W - out||_F / ||W||_F (main.py:212)
    applied: bool             # False: error above the threshold, W restored (main.py:214-216)
    errors: dict = field(default_factory=dict)


@dataclass
class QuantizationReport:
    """Counters of main.py:140-143, 217-251 and the bit accounting of main.py:321-329."""
    quantized_param_count: int = 0
    unquantized_language_param_count: int = 0
    vision_param_count: int = 0
    layers: list = field(default_factory=list)
    skipped: list = field(default_factory=list)

    @property
    def total_bits(self) -> int:  # main.py:324 (2-bit quantised, 4-bit the rest)
        return self.quantized_param_count * 2 + self.unquantized_language_param_count * 4

    @property
    def prior_total_bits(self) -> int:  # main.py:326
        return self.quantized_param_count * 4 + self.unquantized_language_param_count * 4

    @property
    def bit_ratio(self) -> float | None:  # main.py:328-329
        d = self.prior_total_bits
        return self.total_bits / d if d else None

    @property
    def quantized_fraction(self) -> float | None:  # main.py:330
        d = self.quantized_param_count + self.unquantized_language_param_count
        return self.quantized_param_count / d if d else None


# ---------------------------------------------------------------------------- Hadamard
def normalized_hadamard(n: int, device, dtype=torch.float32) -> torch.Tensor:
    """Sylvester Hadamard / sqrt(n) (scipy.linalg.hadamard ordering, main.py:94-98)."""
    if n < 1 or n & (n - 1):
        raise ValueError("Hadamard order must be a power of two")
    Hm = torch.ones((1, 1), dtype=dtype, device=device)
    while Hm.shape[0] < n:
        Hm = torch.cat([torch.cat([Hm, Hm], 1), torch.cat([Hm, -Hm], 1)], 0)
    return Hm * (1.0 / math.sqrt(n))


def _next_pow2(n: int) -> int:
    return 1 << (n - 1).bit_length()


def hadamard_transform(W: torch.Tensor, inverse: bool = False, original_shape=None, signs=None):
    """main.py:108-133 on the device: forward pads W to powers of two and returns
    (H1 W H2, (rows, cols)); inverse returns (H1 W H2)[:rows, :cols] (H symmetric and
    orthogonal).  Two fp32 HIP GEMMs.

    signs = (su, sv), +-1 vectors of at least rows resp. cols entries (`linear.hadamard_sign_vector`): the
    randomised transform H1 diag(su) pad(W) diag(sv) H2.  Forward flips W's rows and columns in the padded
    matrix before the two GEMMs (the pad is zero), inverse flips the rows and columns of the cut result
    after them; every flip is a multiplication by +-1, which is exact."""
    rows, cols = (W.shape if not inverse else original_shape)
    pr, pc = _next_pow2(rows), _next_pow2(cols)
    dev = W.device
    H1, H2 = normalized_hadamard(pr, dev), normalized_hadamard(pc, dev)
    flip = None
    if signs is not None:
        su, sv = (s.to(dev, torch.float32) for s in signs)
        if su.dim() != 1 or sv.dim() != 1 or su.numel() < rows or sv.numel() < cols:
            raise ValueError(f"hadamard_transform: signs {tuple(su.shape)}, {tuple(sv.shape)} do not cover {(rows, cols)}")
        flip = su[:rows, None] * sv[None, :cols]
    if inverse:
        Wp = W.float().contiguous()
    else:
        Wp = torch.zeros((pr, pc), dtype=torch.float32, device=dev)
        Wp[:rows, :cols] = W.float() if flip is None else W.float() * flip
    T = K.gemm(H1, Wp, C=torch.empty((pr, pc), dtype=torch.float32, device=dev))
    out = K.gemm(T, H2, C=torch.empty((pr, pc), dtype=torch.float32, device=dev))
    if inverse:
        return out[:rows, :cols] if flip is None else out[:rows, :cols] * flip
    return out, (rows, cols)


def hadamard_sign_seeds(hadamard_signs: int, name: str, in_features: int):
    """(seed_out, seed_in) of the layer `name` under `apply_caldera_quantization(hadamard_signs=...)`, with
    mix64 = `linear.mix64` and b = mix64(hadamard_signs):

        seed_in  = mix64(b + 2 in_features)                   >> 11
        seed_out = mix64(b + 2 zlib.crc32(name.encode()) + 1) >> 11     (sums mod 2^64)

    Both are below 2^53.  seed_in depends on (hadamard_signs, in_features) alone, so all layers that read one
    activation share sv and with it the input transform (grouped and fused launches stay available);
    seed_out is per module name."""
    from .linear import SIGN_SEED_LIMIT, mix64
    if isinstance(hadamard_signs, bool) or not isinstance(hadamard_signs, int) or not 0 <= hadamard_signs < SIGN_SEED_LIMIT:
        raise ValueError(f"hadamard_signs {hadamard_signs!r} is not an int in [0, 2^53)")
    b = mix64(hadamard_signs)
    m64 = (1 << 64) - 1
    seed_in = mix64((b + 2 * int(in_features)) & m64) >> 11
    seed_out = mix64((b + 2 * zlib.crc32(name.encode()) + 1) & m64) >> 11
    return seed_out, seed_in


# ---------------------------------------------------------------------------- caller
def _reconstruct(dec, dev) -> torch.Tensor:
    """out = Q + L @ R (main.py:198) as one HIP GEMM with a D-epilogue, fp32."""
    Q = dec.Q.to(dev).float().contiguous()
    L = dec.L.to(dev).float().contiguous()
    R = dec.R.to(dev).float().contiguous()
    return K.gemm(L, R, C=torch.empty_like(Q), D=Q, gamma=1.0)


def _rel_error(W: torch.Tensor, out: torch.Tensor) -> float:
    """||W - out||_F / ||W||_F with fp64 sums (cq_weighted_sqsum)."""
    Wf = W.float().contiguous()
    num = K.weighted_sqsum((Wf - out).unsqueeze(0), None, Wf.shape[1])
    den = K.weighted_sqsum(Wf.unsqueeze(0), None, Wf.shape[1])
    return float(torch.sqrt(num / den).item())


def select_layers(model: torch.nn.Module, hessians=None, selection: LayerSelection | None = None,
                  log: Callable | None = None):
    """The module walk of main.py:146-251 without the decomposition: returns the jobs
    [(name, module, h)] in named_modules order and a report holding the unquantised-language
    and vision counters (quantised ones are added as jobs complete)."""
    sel = selection or LayerSelection()
    say = log or (lambda *a: None)
    rep = QuantizationReport()
    jobs = []
    counter = 1
    for name, module in model.named_modules():
        if sel.in_scope(name, module):
            w = module.weight
            if sel.selects(name, w, counter):
                h = None
                if hessians is not None:
                    h = hessians[name]  # main.py:163: KeyError for a layer without a Hessian
                counter += 1
                jobs.append((name, module, h))
            else:
                rep.unquantized_language_param_count += w.numel()
                rep.skipped.append(name)
                say(f"Skipped quantization for {name} with shape {tuple(w.size())}")
        elif hasattr(module, "weight") and module.weight is not None:
            rep.vision_param_count += module.weight.numel()
            say(f"Skipped quantization for {name} with shape {tuple(module.weight.size())}")
    return jobs, rep


def apply_caldera_quantization(model: torch.nn.Module, hessians=None, quant_params=None, *,
                               selection: LayerSelection | None = None, error_threshold: float = 0.99,
                               scale_W: bool = False, hadamard: bool = False, device="cuda",
                               max_batch: int = 64, keep_dtype: bool = True, decompose: Callable | None = None,
                               log: Callable | None = None, hadamard_gate: bool = False,
                               packed: bool = False, packed_factors: bool = False,
                               packed_hadamard: bool = False,
                               hadamard_signs: int | None = None) -> QuantizationReport:
    """main.py:135-251 on the MI355X engine.

    hessians: {module name: diagonal (n,) or dense (n, n)} — `Hall` (a missing name raises
      KeyError as `Hall[name]` does); None: H = I for every layer.
    quant_params: CalderaParams (default `driver_params()`, main.py:167-182).
    keep_dtype: write `out` back in the weight's dtype (the reference assigns the fp32 `out`,
      main.py:199, which only matters for a non-fp32 model).
    hadamard_gate: apply the 0.99 error gate and the bit accounting to the Hadamard branch
      too (off by default: main.py:221-240 writes the recovered weight unconditionally and
      counts nothing).
    decompose(quant_params, Ws, H) -> list of CalderaDecomposition: the engine unless given
      (tests pass a stand-in).  The engine runs every shape batch at once
      (`api.caldera_groups`: all batches interleaved on HIP streams).
    packed: a layer that passes the error gate is replaced by a `linear.CalderaLinear` built
      from its decomposition (2/4-bit codes + fp16 factors, applied by cq_linear_forward)
      instead of receiving the dense `out`; the gate and the counters are unchanged.  Needs
      uniform 2- or 4-bit Q, or nf4 / nf2 Q (taken from `quant_params.quant_factory_Q.method`:
      the layer then holds the level indices); a bbint Q raises ValueError before anything is
      decomposed (per-block affine codes plus an outlier list have no packed form), and so does a
      standardised nf4 / nf2 Q (a `quantization_stable_nf4` factory: its mean term); not with `hadamard` (the layer would need the transforms around
      it) and not with `scale_W=True`: like main.py, the gate and the dense write-back use
      Q + L R of the scaled W without its global scale, while a packed layer applies
      gs (Q + L R), so the two would be different models and the gate would judge a weight
      the layer does not apply.  Either combination raises ValueError.
    packed_factors: with packed=True, keep L and R as their packed 2/4-bit codes too (applied
      by cq_linear_packed_forward) instead of fp16: a quarter or an eighth of the factors'
      bytes and no second rounding.  Needs packed=True, the uniform LR quantiser
      (`quant_factory_LR.method`) and L_bits, R_bits in {2, 4}; anything else raises ValueError.
      The default keeps fp16 factors.
    packed_hadamard: with packed=True, decompose H1 pad(W) H2 exactly as `hadamard=True` does
      (including its ValueError when padding changes n under a Hessian) and replace a layer that
      passes the error gate by a `linear.HadamardCalderaLinear`: the packed layer of the padded
      shape between two cq_hadamard_rows transforms, instead of multiplying back into a dense
      weight.  The gate and the counters are those of packed=True, judged on the recovered
      (H1 (Q + L R) H2)[:m, :n]; `packed_factors` composes with it.  Needs packed=True; not with
      `hadamard=True` (that is main.py's dense write-back) and not with `scale_W=True`; a padded
      dimension above `_lib.HADAMARD_MAX_N` raises ValueError.
    hadamard_signs: with packed_hadamard=True, an int in [0, 2^53): decompose the randomised transform
      H1 diag(su) pad(W) diag(sv) H2 (CALDERA's and QuIP#'s incoherence processing) and build signed
      `linear.HadamardCalderaLinear` layers, each with the seeds `hadamard_sign_seeds(hadamard_signs, name,
      in_features)`: seed_in from in_features alone, so q / k / v and gate / up still share their input
      transform, seed_out from the module's name.  The decomposition, the recovered weight and the error
      gate are those of the signed transform; the Hessian is not transformed (as without signs).  Needs
      packed_hadamard=True: otherwise, or for a value outside the range, ValueError before anything is
      decomposed.  None, the default: the plain transform, as before.
    Returns the QuantizationReport (counters + per-layer outcomes)."""
    qp = quant_params if quant_params is not None else driver_params()
    if packed_hadamard and not packed:
        raise ValueError("apply_caldera_quantization: packed_hadamard=True needs packed=True")
    if hadamard_signs is not None:
        if not packed_hadamard:
            raise ValueError("apply_caldera_quantization: hadamard_signs needs packed_hadamard=True (the sign vectors "
                             "belong to the packed layer's transforms)")
        try:
            hadamard_sign_seeds(hadamard_signs, "", 1)
        except ValueError as e:
            raise ValueError(f"apply_caldera_quantization: {e}") from None
    if packed and hadamard:
        raise ValueError("apply_caldera_quantization: packed=True cannot be combined with hadamard=True (the dense "
                         "write-back of main.py); packed_hadamard=True runs the Hadamard branch packed")
    if packed and scale_W:
        raise ValueError("apply_caldera_quantization: packed=True cannot be combined with scale_W=True (the gate "
                         "and the write-back use Q + L R without the global scale; the packed layer applies it)")
    q_method = str(getattr(getattr(qp, "quant_factory_Q", None), "method", "uniform")).lower()
    if packed_factors:
        if not packed:
            raise ValueError("apply_caldera_quantization: packed_factors=True needs packed=True")
        method = str(getattr(getattr(qp, "quant_factory_LR", None), "method", "uniform")).lower()
        if method != "uniform":
            raise ValueError(f"apply_caldera_quantization: packed_factors=True needs the uniform LR quantiser, got "
                             f"{method!r}: codebook factors have no packed codes")
        if getattr(qp, "L_bits", None) not in (2, 4) or getattr(qp, "R_bits", None) not in (2, 4):
            raise ValueError(f"apply_caldera_quantization: packed_factors=True needs L_bits / R_bits in (2, 4), got "
                             f"{getattr(qp, 'L_bits', None)} / {getattr(qp, 'R_bits', None)}")
    if packed:
        # the Q quantiser must have a packed form (uniform, nf4, nf2: bbint raises), before
        # anything is decomposed
        from .linear import q_method_format
        if (getattr(getattr(qp, "quant_factory_Q", None), "nf_variant", None) == "standardized"
                and q_method in ("nf4", "nf2")):
            raise ValueError(f"apply_caldera_quantization: packed=True: the standardised {q_method} Q "
                             "(quantization_stable_nf4) has no packed form: Q = level * std + mean carries a "
                             "mean term that no packed kernel applies")
        q_method_format(q_method, getattr(qp, "Q_bits", None))
    say = log or (lambda *a: None)
    jobs, rep = select_layers(model, hessians, selection, say)
    transform = hadamard or packed_hadamard  # decompose H1 pad(W) H2
    if packed_hadamard:
        for name, module, _ in jobs:
            pshape = tuple(_next_pow2(d) for d in module.weight.shape)
            if max(pshape) > K.HADAMARD_MAX_N:
                raise ValueError(f"apply_caldera_quantization: packed_hadamard=True: {name}: padded shape {pshape} "
                                 f"exceeds {K.HADAMARD_MAX_N} (cq_hadamard_rows' largest transform)")
    # batches: same shape; every layer keeps its own Hessian (a list of per-matrix H, or one
    # shared H / None when the whole batch has the same object)
    groups: dict = {}
    for job in jobs:
        groups.setdefault(tuple(job[1].weight.shape), []).append(job)
    outcomes = {}
    seeds = {}    # name -> (seed_out, seed_in) with hadamard_signs
    batches = []  # (jobs, Ws, shapes, H)
    with torch.no_grad():
        for key, members in groups.items():
            for s in range(0, len(members), max_batch):
                part = members[s:s + max_batch]
                h = part[0][2] if all(j[2] is part[0][2] for j in part) else [j[2] for j in part]
                Ws, shapes = [], []
                for name, module, hj in part:
                    W = module.weight.data
                    if transform:  # main.py:224-232: transform, decompose the fp32 transform
                        if hj is not None and _next_pow2(W.shape[1]) != W.shape[1]:
                            raise ValueError(f"{name}: Hadamard padding changes n ({W.shape[1]}) but H is n x n")
                        if hadamard_signs is not None:
                            seeds[name] = hadamard_sign_seeds(hadamard_signs, name, W.shape[1])
                        Wt, shp = hadamard_transform(W.to(device), signs=_sign_vectors(seeds.get(name), W.shape))
                        Ws.append(Wt)
                        shapes.append(shp)
                    else:
                        Ws.append(W)
                batches.append((part, Ws, shapes, h))
        if decompose is None:
            from .api import caldera_groups
            all_decs = caldera_groups(qp, [(Ws, h) for _, Ws, _, h in batches], device=device, scale_W=scale_W)
        else:
            all_decs = [decompose(qp, Ws, h) for _, Ws, _, h in batches]
    for (part, Ws, shapes, h), decs in zip(batches, all_decs):
        with torch.no_grad():
            for (name, module, _), dec, i in zip(part, decs, range(len(part))):
                W = module.weight.data
                dev = W.device if W.device.type == "cuda" else torch.device(device)
                out = _reconstruct(dec, dev)
                if transform:
                    out = hadamard_transform(out, inverse=True, original_shape=shapes[i],
                                             signs=_sign_vectors(seeds.get(name), shapes[i])).contiguous()
                err = _rel_error(W.to(dev), out)
                if hadamard and not hadamard_gate:
                    # main.py:221-240: the Hadamard branch always writes the recovered
                    # weight back, with no error gate and no parameter counting
                    module.weight.data = out.to(W.dtype).to(W.device)
                    say(f"Applied CALDERA (Hadamard) to {name}.weight, shape: {tuple(W.shape)}")
                    outcomes[name] = LayerOutcome(name, tuple(W.shape), err, True, dict(dec.errors))
                    continue
                ok = err <= error_threshold
                if ok and packed:
                    from .linear import CalderaLinear, HadamardCalderaLinear
                    fbits = dict(L_bits=qp.L_bits, R_bits=qp.R_bits) if packed_factors else {}
                    bias = getattr(module, "bias", None)
                    if packed_hadamard:
                        lin = HadamardCalderaLinear.from_decomposition(dec, qp.Q_bits, shapes[i], bias=bias,
                                                                       Q_method=q_method, sign_seeds=seeds.get(name),
                                                                       **fbits)
                    else:
                        lin = CalderaLinear.from_decomposition(dec, qp.Q_bits, bias=bias, Q_method=q_method, **fbits)
                    _set_module(model, name, lin.to(W.device))
                    rep.quantized_param_count += W.numel()
                    say(f"Applied CALDERA (packed{', Hadamard' if packed_hadamard else ''}) to {name}.weight, shape: "
                        f"{tuple(W.shape)}")
                elif ok:
                    module.weight.data = (out.to(W.dtype) if keep_dtype else out).to(W.device)
                    rep.quantized_param_count += W.numel()
                    say(f"Applied CALDERA to {name}.weight, shape: {tuple(W.shape)}")
                else:
                    rep.unquantized_language_param_count += W.numel()
                    say(f"Error of the decomposition is greater than threshold for {name}. Skipping quantization")
                outcomes[name] = LayerOutcome(name, tuple(W.shape), err, ok, dict(dec.errors))
    rep.layers = [outcomes[j[0]] for j in jobs]
    return rep


def _sign_vectors(seeds, shape):
    """`hadamard_transform`'s signs for a layer of `shape` with the seeds (seed_out, seed_in), None for None."""
    if seeds is None:
        return None
    from .linear import hadamard_sign_vector
    return hadamard_sign_vector(seeds[0], shape[0]), hadamard_sign_vector(seeds[1], shape[1])


def _set_module(model: torch.nn.Module, name: str, new: torch.nn.Module):
    """Replace the submodule `name` (dotted, as named_modules gives it) of `model`."""
    parent_name, _, leaf = name.rpartition(".")
    parent = model.get_submodule(parent_name) if parent_name else model
    setattr(parent, leaf, new)


def apply_packed_results(model: torch.nn.Module, results, device=None) -> list:
    """Replace each `nn.Linear` named by a `sharding.MatrixResult` (e.g. from `load_results`) by
    a `linear.CalderaLinear` holding that result (the module's bias is kept); a result whose
    `extra` has "hadamard": [m, n] (a layer decomposed in the Hadamard basis, on the padded grid)
    is matched against that original shape and becomes a `linear.HadamardCalderaLinear` (a signed one, with
    the same sign vectors, when `extra` also has "hadamard_signs": [seed_out, seed_in]).  device: where
    the new layers live (default: each replaced module's own device).  KeyError for a result
    whose module the model does not have; returns the replaced names.  A `linear.CalderaLinearGroup` that a
    replaced module belonged to is dissolved (a plain packed layer holds no `weight` and is refused by
    the shape check like any other such module, its group left as it was)."""
    from .linear import CalderaLinear, HadamardCalderaLinear
    modules = dict(model.named_modules())
    done = []
    for res in results:
        if res.name not in modules or not res.name:
            raise KeyError(f"apply_packed_results: the model has no module {res.name!r}")
        mod = modules[res.name]
        w = getattr(mod, "weight", None)
        had = (res.extra or {}).get("hadamard")
        want = (res.m, res.n) if had is None else tuple(int(v) for v in had)
        if w is None or tuple(w.shape) != want:
            raise ValueError(f"apply_packed_results: {res.name}: weight {None if w is None else tuple(w.shape)} "
                             f"!= result {want}")
        cls = CalderaLinear if had is None else HadamardCalderaLinear
        lin = cls.from_result(res, bias=getattr(mod, "bias", None))
        _dissolve_group_of(mod)
        _set_module(model, res.name, lin.to(w.device if device is None else device))
        done.append(res.name)
    return done


def prepare_factor_finetuning(model: torch.nn.Module, master_dtype=torch.float32, *, hadamard=False,
                              coded_factors="refuse") -> list:
    """Make the low-rank factors of every packed layer trainable over its frozen codes (CALDERA's
    W ~ Q + L R with Q fixed, adapted LoRA-style with the factors already in place): calls
    `CalderaLinear.enable_factor_training(master_dtype)` on every `linear.CalderaLinear` with fp16
    factors and rank > 0 and returns the new parameters, for the optimiser.

    hadamard=True: a `linear.HadamardCalderaLinear` whose inner layer has fp16 factors is made
    trainable too; its parameters are `<name>.inner.L` and `<name>.inner.R`, factors of the weight
    in the Hadamard basis.  coded_factors="freeze": a layer with coded factors (a Hadamard layer
    whose inner has them counts as one) is left as it is: it back-propagates dx and trains nothing.

    ValueError, before anything is changed, naming the packed layers the keywords do not admit
    (the defaults: every layer with coded factors, every `linear.HadamardCalderaLinear`), or for
    a coded_factors that is neither "refuse" nor "freeze"."""
    from .linear import CalderaLinear, HadamardCalderaLinear
    if coded_factors not in ("refuse", "freeze"):
        raise ValueError(f"prepare_factor_finetuning: coded_factors {coded_factors!r} not in ('refuse', 'freeze')")
    inner = {id(mod.inner) for mod in model.modules() if isinstance(mod, HadamardCalderaLinear)}
    bad, layers = [], []
    for name, mod in model.named_modules():
        if isinstance(mod, HadamardCalderaLinear):
            lin, what = mod.inner, "Hadamard basis"
            if not hadamard:
                bad.append(f"{name or '<model>'} (Hadamard basis)")
                continue
        elif isinstance(mod, CalderaLinear) and id(mod) not in inner:
            lin, what = mod, ""
        else:
            continue
        if lin.L_codes is not None or lin.R_codes is not None:
            if coded_factors == "refuse":
                bad.append(f"{name or '<model>'} ({what + ', ' if what else ''}coded factors)")
        elif lin.rank > 0:
            layers.append(lin)
    if bad:
        raise ValueError("prepare_factor_finetuning: packed layers without a backward: " + ", ".join(bad))
    params = []
    for mod in layers:
        params += mod.enable_factor_training(master_dtype)
    return params


def finish_factor_finetuning(model: torch.nn.Module) -> torch.nn.Module:
    """Round every trained factor back to its fp16 buffer (`CalderaLinear.freeze_factors`; the
    inner layer of a `linear.HadamardCalderaLinear` is one of `model.modules()`): the packed
    layers are inference layers again."""
    from .linear import CalderaLinear
    for mod in model.modules():
        if isinstance(mod, CalderaLinear):
            mod.freeze_factors()
    return model


def _packed_layers(model: torch.nn.Module) -> list:
    """[(name, module)] of every packed layer of `model`: each `linear.HadamardCalderaLinear` and each
    `linear.CalderaLinear` that is not the inner layer of one."""
    from .linear import CalderaLinear, HadamardCalderaLinear
    inner = {id(mod.inner) for mod in model.modules() if isinstance(mod, HadamardCalderaLinear)}
    return [(name, mod) for name, mod in model.named_modules()
            if isinstance(mod, HadamardCalderaLinear) or (isinstance(mod, CalderaLinear) and id(mod) not in inner)]


def set_dense_prefill(model: torch.nn.Module, tokens) -> list:
    """Set (`tokens`: an int above `_lib.LINEAR_DECODE_MAX_TOKENS`) or clear (None) the token count from
    which every packed layer materialises its fp16 weight into the shared scratch buffer and runs the
    dense GEMM (`CalderaLinear.dense_prefill_tokens`; a Hadamard layer's threshold is its inner
    layer's).  Returns the layers' names.  ValueError before any layer is changed."""
    from .linear import check_dense_prefill_tokens
    tokens = check_dense_prefill_tokens(tokens)
    layers = _packed_layers(model)
    for _, mod in layers:
        mod.dense_prefill_tokens = tokens
    return [name for name, _ in layers]


def unpack_packed_layers(model: torch.nn.Module, dtype=torch.float16) -> list:
    """Replace every `linear.CalderaLinear` / `linear.HadamardCalderaLinear` by an `nn.Linear` whose
    weight is the layer's `materialize(dtype)` (cq_linear_dequant: fp16, bf16 or fp32) and whose bias
    is the layer's, cast to dtype: the model as plain dense layers, e.g. for export.  Returns the
    replaced names.  ValueError, before anything is changed, for layers whose factors are trainable:
    call `finish_factor_finetuning` first.  A `linear.CalderaLinearGroup` of a replaced layer is dissolved."""
    layers = _packed_layers(model)
    bad = [name or "<model>" for name, mod in layers if mod.factors_trainable]
    if bad:
        raise ValueError("unpack_packed_layers: trainable factors (call finish_factor_finetuning first): "
                         + ", ".join(bad))
    for name, mod in layers:
        if not name:
            raise ValueError("unpack_packed_layers: the model itself is a packed layer (nothing to replace it in)")
    for name, mod in layers:
        W = mod.materialize(dtype)
        lin = torch.nn.Linear(mod.in_features, mod.out_features, bias=mod.bias is not None, device=W.device,
                              dtype=dtype)
        with torch.no_grad():
            lin.weight.copy_(W)
            if mod.bias is not None:
                lin.bias.copy_(mod.bias)
        _dissolve_group_of(mod)  # a group of layers that are no longer all in the model
        _set_module(model, name, lin)
    return [name for name, _ in layers]


SHARED_INPUT_SETS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"))


def group_shared_input_layers(model: torch.nn.Module, sets=SHARED_INPUT_SETS, hadamard=False):
    """Make a `linear.CalderaLinearGroup` of every set of sibling packed layers that read the same
    activation: for each module of `model` and each tuple of child names in `sets`, the children of
    those names, when all of them are `linear.CalderaLinear` layers that can form a group.  The
    model's code stays as it is: `self.q_proj(h)`, `self.k_proj(h)`, `self.v_proj(h)` then run as one
    launch pair (see `CalderaLinearGroup`), with the bits of the ungrouped layers.

    Returns (grouped, skipped): the dotted names of each group made, as tuples, and for every set of
    which a module has at least one child but which was not grouped, (names, reason) -- a child is
    missing, dense, a Hadamard-basis layer, already grouped, or the layers do not fit one group.
    Nothing raises for them.

    hadamard=True: a set whose children are all `linear.HadamardCalderaLinear` layers becomes a
    `linear.HadamardLinearGroup` (one input transform, one inner launch pair, one grouped output
    transform per padded width).  A set that mixes plain and Hadamard-basis layers stays skipped.  With
    the default, Hadamard-basis sets are skipped as before."""
    from .linear import CalderaLinear, CalderaLinearGroup, HadamardCalderaLinear, HadamardLinearGroup
    grouped, skipped = [], []
    for prefix, mod in list(model.named_modules()):
        for names in sets:
            children = [mod._modules.get(name) for name in names]
            if all(child is None for child in children):
                continue
            full = tuple(f"{prefix}.{name}" if prefix else name for name in names)
            reason = None
            basis = hadamard and all(isinstance(child, HadamardCalderaLinear) for child in children)
            for name, child in zip(names, children):
                if child is None:
                    reason = f"{name} is missing"
                elif basis:
                    if child.group is not None:
                        reason = f"{name} is already grouped"
                elif isinstance(child, HadamardCalderaLinear):
                    reason = f"{name} is a HadamardCalderaLinear"
                elif not isinstance(child, CalderaLinear):
                    reason = f"{name} is dense ({type(child).__name__})"
                elif child.group is not None:
                    reason = f"{name} is already grouped"
                if reason:
                    break
            if reason is None:
                try:
                    (HadamardLinearGroup if basis else CalderaLinearGroup)(children)
                except ValueError as e:
                    reason = f"incompatible: {e}"
            if reason is None:
                grouped.append(full)
            else:
                skipped.append((full, reason))
    return grouped, skipped


def ungroup_shared_input_layers(model: torch.nn.Module) -> list:
    """Dissolve every `linear.CalderaLinearGroup` and `linear.HadamardLinearGroup` that a layer of `model`
    belongs to; returns the dotted names of each dissolved group's members found in the model, as tuples."""
    from .linear import CalderaLinear, HadamardCalderaLinear
    names = {id(mod): name for name, mod in model.named_modules()}
    done = []
    for mod in list(model.modules()):
        group = mod.group if isinstance(mod, (CalderaLinear, HadamardCalderaLinear)) else None
        if group is not None:
            done.append(tuple(names[id(lin)] for lin in group.members if id(lin) in names))
            group.dissolve()
    return done


def _dissolve_group_of(mod):
    group = mod.__dict__.get("_group")
    if group is not None:
        group.dissolve()


GATED_MLP_NAMES = ("gate_proj", "up_proj", "down_proj", "act_fn")


def _recognise_activation(fn):
    """"silu" for an `nn.SiLU` instance or `torch.nn.functional.silu`, else None."""
    if isinstance(fn, torch.nn.SiLU) or fn is torch.nn.functional.silu:
        return "silu"
    return None


def fuse_gated_mlps(model: torch.nn.Module, names=GATED_MLP_NAMES, act=None, hadamard=False):
    """Replace every gated MLP block of `model` by a `linear.CalderaGatedMLP`, whose gate / up pair runs
    as one launch pair with the activation and the product in its epilogue (cq_linear_glu_forward).

    A block is a module with the three children names[0:3] (gate, up, down) and a recognisable
    activation: its attribute names[3] is an `nn.SiLU` instance or `torch.nn.functional.silu`, or `act`
    ("silu" | "identity") is passed explicitly and overrides it.  THE ASSUMPTION: the block's forward
    computes the standard formula `down(act(gate(x)) * up(x))` and nothing else; this function cannot see
    the forward's code, so do not fuse a block that does more (dropout, a residual, a different product).
    A block with further children, parameters or buffers of its own is left alone for that reason.

    The new module holds the three layers under the names gate_proj / up_proj / down_proj (with the
    default `names` the state dict keys are unchanged, and a state dict saved before loads after and the
    other way round) and keeps the original block in its `__dict__` (not a submodule) for
    `unfuse_gated_mlps`.

    Returns (fused, skipped): the dotted names of the replaced blocks, and (name, reason) for every
    module that has the three children but was left alone -- a dense child, a Hadamard-basis layer, an
    unknown activation, layers that do not fit the entry, extra state, the model itself, already fused.
    Nothing raises for them.  `unpack_packed_layers`, `set_dense_prefill`, `prepare_factor_finetuning`
    and `group_shared_input_layers` work on a fused model: they find the layers by type, and the fused
    module takes its unfused formula wherever the fused launch is not the layers' own.

    hadamard=True: a block whose gate and up are both `linear.HadamardCalderaLinear` layers becomes a
    `linear.HadamardGatedMLP` (the activation and the product in the output transform's epilogue,
    cq_hadamard_glu_rows).  A block that mixes a plain and a Hadamard-basis layer stays skipped.  With the
    default, Hadamard-basis blocks are skipped as before."""
    from .linear import (ACTIVATIONS, CalderaGatedMLP, CalderaLinear, HadamardCalderaLinear, HadamardGatedMLP, glu_fit,
                         hadamard_glu_fit)
    if len(names) != 4:
        raise ValueError(f"fuse_gated_mlps: names {names!r} is not (gate, up, down, activation)")
    if act is not None and act not in ACTIVATIONS:
        raise ValueError(f"fuse_gated_mlps: act {act!r} not in {tuple(ACTIVATIONS)}")
    gate_n, up_n, down_n, act_n = names
    fused, skipped = [], []
    for name, mod in list(model.named_modules()):
        children = [mod._modules.get(n) for n in (gate_n, up_n, down_n)]
        if any(child is None for child in children):
            continue
        label = name or "<model>"
        if isinstance(mod, (CalderaGatedMLP, HadamardGatedMLP)):
            skipped.append((label, "already fused"))
            continue
        gate, up, down = children
        how = act if act is not None else _recognise_activation(getattr(mod, act_n, None))
        extra = [n for n in mod._modules if n not in names] + list(mod._parameters) + list(mod._buffers)
        reason = None
        basis = hadamard and isinstance(gate, HadamardCalderaLinear) and isinstance(up, HadamardCalderaLinear)
        for n, child in ((gate_n, gate), (up_n, up)):
            if basis:
                break
            if isinstance(child, HadamardCalderaLinear):
                reason = f"{n} is a HadamardCalderaLinear"
            elif not isinstance(child, CalderaLinear):
                reason = f"{n} is dense ({type(child).__name__})"
            if reason:
                break
        if reason is None:
            why = hadamard_glu_fit(gate, up) if basis else glu_fit(gate, up)
            if why is not None:
                reason = f"incompatible: {why}"
            elif how is None:
                reason = f"unknown activation {act_n} = {getattr(mod, act_n, None)!r} (pass act=)"
            elif extra:
                reason = f"the block has more than the three layers and the activation: {', '.join(extra)}"
            elif not name:
                reason = "the model itself is the block (nothing to replace it in)"
        if reason is not None:
            skipped.append((label, reason))
            continue
        new = (HadamardGatedMLP if basis else CalderaGatedMLP)(gate, up, down, act=how)
        new.__dict__["_original"] = (mod, (gate_n, up_n, down_n))
        new.train(mod.training)
        _set_module(model, name, new)
        fused.append(name)
    return fused, skipped


def unfuse_gated_mlps(model: torch.nn.Module) -> list:
    """Put back the original block of every `linear.CalderaGatedMLP` and `linear.HadamardGatedMLP` that
    `fuse_gated_mlps` made, with the three layers the fused module holds now (they may have been replaced
    or unpacked since); returns the dotted names.  A fused module built by hand has no original and stays."""
    from .linear import CalderaGatedMLP, HadamardGatedMLP
    done = []
    for name, mod in list(model.named_modules()):
        if (not isinstance(mod, (CalderaGatedMLP, HadamardGatedMLP)) or "_original" not in mod.__dict__
                or not name):
            continue
        orig, names = mod.__dict__["_original"]
        for n, layer in zip(names, (mod.gate_proj, mod.up_proj, mod.down_proj)):
            setattr(orig, n, layer)
        _set_module(model, name, orig)
        done.append(name)
    return done
