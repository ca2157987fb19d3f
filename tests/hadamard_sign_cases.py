"""Shared pieces of the randomised-Hadamard tests (test_hadamard_signs_host.py, test_gpu_hadamard_signs.py,
test_gpu_hadamard_sign_layers.py): the pinned sign vector, sign-byte vectors for the kernel entries and the
kernel cases.

The kernels flip an element iff its sign byte is negative, so `sign_bytes` draws its negative entries from
-128 .. -1 and the others from 0 .. 127, not from +-1 alone: a kernel that tested `== -1`, bit 0 or `!= 1`
would show.  `as_pm1` gives the +-1 vector such bytes stand for.

Kernel cases (P, rows, n_in, n_out), the smallest that reach every kernel form of csrc/cq_hadamard.hip with
the sign path both ways:
    P = 4, 64, 2048   the one-wave teams (one chunk per row; 16 lanes per row; a whole wave with 8 chunks)
    P = 4096          one row per workgroup (the LDS exchange)
    P = 8192          the block kernel (two sub-rows and stage B)
with rows in {1, 3, 17}, whole rows (every chunk takes the 4-byte sign load when the vector is aligned) and
ragged n_in / n_out that are no multiple of four (the last chunk takes the scalar path, and the chunks
beyond read no sign byte at all)."""
import numpy as np

# linear.hadamard_sign_vector(7, 32), and the sum of its first 4096 entries
SEED7_FIRST32 = [-1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1, -1, 1, 1, -1,
                 -1, 1, -1, -1, -1, -1, 1, -1, -1, -1, 1, -1, 1, -1, 1, -1]
SEED7_SUM4096 = -54

KERNEL_CASES = [
    (4, 3, 4, 4), (4, 1, 3, 2),
    (64, 17, 50, 37), (64, 3, 64, 64),
    (2048, 3, 2048, 2043), (2048, 1, 1029, 2048),
    (4096, 1, 4096, 4096), (4096, 3, 2050, 4091),
    (8192, 3, 8187, 8192), (8192, 1, 8192, 4097),
]
# P at which the exact cases of hadamard_cases.py hold (c a power of two); the others take its random bar
EXACT_PS = (4, 64, 4096)
DTYPE_PAIR_P = 64      # every (x dtype, y dtype) pair runs at this P


def case_id(c):
    return "P{}r{}i{}o{}".format(*c)


def sign_bytes(n, seed):
    """n int8 sign bytes: about half negative (-128 .. -1), the others in 0 .. 127."""
    rng = np.random.default_rng(977 * seed + n)
    neg = rng.integers(0, 2, n).astype(bool)
    return np.where(neg, rng.integers(-128, 0, n), rng.integers(0, 128, n)).astype(np.int8)


def as_pm1(b):
    """The +-1 fp32 vector the sign bytes b stand for."""
    return np.where(b < 0, -1.0, 1.0).astype(np.float32)
