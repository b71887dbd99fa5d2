"""numpy restatement of the dropout draw of csrc/pn2_train.hip (mix_u32 / dropout_kernel), used by the tests only.

The draw of element i is the low 32 bits of a 64-bit mix of (seed, step, i); the element is kept when the draw is below
uint32(float64(float32(keep)) * 2**32), and unconditionally when keep >= 1.  The mix is a bijection of its 64-bit input (odd
multipliers, xor-shifts by 32), so `seed_for_output` can construct the seed that makes a chosen element draw a chosen value."""
import numpy as np

M64 = (1 << 64) - 1
STEP_MUL = 0x9E3779B97F4A7C15
INDEX_MUL = 0xD1B54A32D192ED03
ROUND_MUL = 0xD6E8FEB86659FD93
ROUND_MUL_INV = pow(ROUND_MUL, -1, 1 << 64)


def _u64(v):
    """a Python int of either sign -> the 64-bit pattern the kernel sees after its signed-to-unsigned cast"""
    return int(v) & M64


def mix64_int(seed, step, i):
    """the whole 64-bit mix in plain Python integers"""
    x = _u64(seed) ^ (_u64(step) * STEP_MUL & M64) ^ (_u64(i) * INDEX_MUL & M64)
    x ^= x >> 32
    x = x * ROUND_MUL & M64
    x ^= x >> 32
    x = x * ROUND_MUL & M64
    x ^= x >> 32
    return x


def draw_int(seed, step, i):
    return mix64_int(seed, step, i) & 0xFFFFFFFF


def draws(seed, step, n, start=0):
    """uint32 draws of elements start .. start + n - 1, vectorised in numpy uint64 (wrapping arithmetic)"""
    i = np.arange(start, start + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = i * np.uint64(INDEX_MUL)
        x ^= np.uint64(_u64(seed) ^ (_u64(step) * STEP_MUL & M64))
        x ^= x >> np.uint64(32)
        x *= np.uint64(ROUND_MUL)
        x ^= x >> np.uint64(32)
        x *= np.uint64(ROUND_MUL)
        x ^= x >> np.uint64(32)
    return x.astype(np.uint32)  # keeps the low word


def threshold(keep):
    """uint32(float64(float32(keep)) * 2**32) for keep < 1"""
    return int(np.float64(np.float32(keep)) * 4294967296.0)


def keep_bits(seed, step, n, keep, start=0):
    """bool (n,): which elements are kept.  keep >= 1 keeps every element whatever it draws."""
    if np.float32(keep) >= np.float32(1):
        return np.ones(n, bool)
    return draws(seed, step, n, start) < np.uint32(threshold(keep))


def apply(x, kept, keep):
    """where(kept, x * float32(1 / keep), 0) in float32: what pn2_dropout writes to y and pn2_dropout_grad to dx"""
    inv = np.float32(1.0) / np.float32(keep)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.where(kept, np.asarray(x, np.float32) * inv, np.float32(0)).astype(np.float32)


def seed_for_output(out64, step=0, i=0):
    """the seed (as the signed int64 the state tensor holds) for which mix64(seed, step, i) == out64"""
    x = _u64(out64)
    x ^= x >> 32
    x = x * ROUND_MUL_INV & M64
    x ^= x >> 32
    x = x * ROUND_MUL_INV & M64
    x ^= x >> 32
    x ^= (_u64(step) * STEP_MUL & M64) ^ (_u64(i) * INDEX_MUL & M64)
    return x - (1 << 64) if x >> 63 else x


# mix64(KEEP_ONE_SEED, 0, 0) = 0x12345678FFFFFFFF: element 0 of step 0 draws 0xFFFFFFFF, the one draw a `draw < 0xFFFFFFFF` rule drops
KEEP_ONE_OUTPUT = 0x12345678FFFFFFFF
KEEP_ONE_SEED = seed_for_output(KEEP_ONE_OUTPUT)
