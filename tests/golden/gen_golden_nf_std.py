"""Generate tests/golden/nf_std_kat.npz from the REFERENCE's standardised NF quantiser.

Test infrastructure only.  This script imports the unmodified reference (its
src/caldera/utils/quantization_stable_nf4.py and src/caldera/decomposition/alg.py) from the
directory given on the command line and records, on the CPU with one torch thread (the fp32 mean
of a large block depends on the thread count):

  quantiser cases   for every in_* input of quant_kat.npz (read from there), nf4 and nf2, block 64
                    and whole matrix: idx, mean, std and the dequantised values, keys
                    {method}_bs{64|all}_{input}_{idx|mean|std|deq}
  end-to-end cases  one fp16 W (128 x 256, seed 11, stored as W) through caldera() with H = I,
                    rank 8, iters 2, update_order ["Q", "LR"], sigma_reg 1e-8:
                      a  standardised nf4 Q at 4 bits, fp16 factors
                      b  standardised nf2 Q at 2 bits, fp16 factors
                      c  uniform 2-bit Q, 4-bit standardised-nf4 factors, lplr_iters 3
                    keys {a|b|c}_errors_Q, _errors_LR, _global_scale, _QLR (Q + L R, fp32)

Usage:  python tests/golden/gen_golden_nf_std.py <reference checkout>
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from src.caldera.decomposition import alg
    from src.caldera.utils import quantization_stable_nf4 as qs
    from src.caldera.utils.dataclasses import CalderaParams

    torch.set_num_threads(1)
    kat = np.load(os.path.join(OUT, "quant_kat.npz"), allow_pickle=False)
    o = {}
    for k in kat.files:
        if not k.startswith("in_"):
            continue
        x = kat[k]
        for method, bits in (("nf4", 4), ("nf2", 2)):
            for bs in (64, x.size):
                qz = qs.LowMemoryQuantizer(num_bits=bits, method=method, block_size=bs)
                idx, (mean, std), shape = qz.quantize_block(torch.from_numpy(x.copy()))
                deq = qz.dequantize_block(idx, (mean, std), shape)
                key = f"{method}_bs{'all' if bs == x.size else bs}_{k[3:]}"
                assert idx.dtype == torch.uint8 and mean.dtype == std.dtype == deq.dtype == torch.float32
                o[key + "_idx"] = idx.numpy()
                o[key + "_mean"] = mean.numpy()
                o[key + "_std"] = std.numpy()
                o[key + "_deq"] = deq.numpy()

    torch.manual_seed(11)
    W = (torch.randn(128, 256) * 0.02).to(torch.float16)
    o["W"] = W.numpy()
    base = dict(rank=8, iters=2, update_order=["Q", "LR"], sigma_reg=1e-8)
    cfgs = {"a": dict(Q_bits=4, L_bits=16, R_bits=16, quant_factory_Q=qs.QuantizerFactory(method="nf4")),
            "b": dict(Q_bits=2, L_bits=16, R_bits=16, quant_factory_Q=qs.QuantizerFactory(method="nf2")),
            "c": dict(Q_bits=2, L_bits=4, R_bits=4, lplr_iters=3, quant_factory_Q=qs.QuantizerFactory(method="uniform"),
                      quant_factory_LR=qs.QuantizerFactory(method="nf4"))}
    for tag, kw in cfgs.items():
        d = alg.caldera(CalderaParams(**base, **kw), W.clone(), None, device="cpu", use_tqdm=False)
        if tag != "c":
            assert isinstance(d.Q_scale, tuple) and d.Q_idxs.dtype == torch.uint8
        o[tag + "_errors_Q"] = np.array(d.errors["Q"], dtype=np.float64)
        o[tag + "_errors_LR"] = np.array(d.errors["LR"], dtype=np.float64)
        o[tag + "_global_scale"] = np.float64(d.global_scale)
        o[tag + "_QLR"] = (d.Q.float() + d.L.float() @ d.R.float()).numpy()
        print(tag, d.errors)
    path = os.path.join(OUT, "nf_std_kat.npz")
    np.savez_compressed(path, **o)
    print(path, len(o), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
