"""Reference for the load-time LoRA merge, written from its specification in float64 -- not from
llama_p2p_amd.gguf.lora_merge_bf16, which the tests compare against it.

    acc[n][k] = sum_j B[n][j] A[j][k]            w'[n][k] = bf16_rne(w[n][k] + scale * acc[n][k])

w: bf16 bits [n_out][n_in]; A [r][n_in]; B [n_out][r].  The device evaluates the sum and the update in f32 with no
promised order; a float64 evaluation of f32 inputs is exact for the dyadic cases below and within 2^-52 relative of
exact otherwise, far below the f32 error the interval rule allows for."""
import numpy as np

# (rows, cols, r) of the kernel tests: one chunk of r (16 per chunk) and several, a ragged r, rows and columns that
# are not whole tiles (64 x 256)
KERNEL_SHAPES = [(128, 256, 1), (512, 256, 16), (256, 512, 64), (96, 160, 3), (33, 40, 5)]
DYADIC_SCALE = 2.0 ** -12
WEIGHT_STD = 0.02  # the synthetic weights' magnitude (llama_p2p_amd/synth.py)


def bf16_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def f64_to_bf16_rne(x):
    """Exact round-to-nearest-even of float64 values to bf16 bits (finite inputs).  bf16 keeps 8 significant bits
    with f32's exponent range: for |x| = m 2^e, m in [0.5, 1), the spacing is 2^(e - 8), never below 2^-133 (the
    subnormals).  x / spacing and the product back are exact in float64 (powers of two), np.rint rounds ties to
    even, and the result is a bf16 value, so its f32 form is exact (2^128 becomes inf, as RNE gives)."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e - 8, -133))
    y = np.rint(x / q) * q
    with np.errstate(over="ignore"):
        f = y.astype(np.float32)
    u = f.view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any()
    return (u >> np.uint32(16)).astype(np.uint16)


def merge_f64(w_bits, A, B, scale):
    """(x, bits): the float64 value w + scale * B A and its exact bf16 rounding."""
    x = bf16_to_f64(w_bits) + float(np.float32(scale)) * (np.asarray(B, np.float64) @ np.asarray(A, np.float64))
    return x, f64_to_bf16_rne(x)


def merge_interval(w_bits, A, B, scale, r):
    """The bf16 values an f32 evaluation may return: [RNE(x - d), RNE(x + d)] with the first-order f32 error bound
    d = (r + 2) 2^-24 (|w| + |scale| sum_j |B| |A|): r - 1 additions and r products of the sum, bounded together by
    r u times the sum of the absolute products (u = 2^-24), the product with scale and the final addition, one u
    each.  Returns (lo bits, hi bits, x)."""
    x, _ = merge_f64(w_bits, A, B, scale)
    mag = np.abs(bf16_to_f64(w_bits)) + abs(float(np.float32(scale))) * (np.abs(np.asarray(B, np.float64)) @
                                                                         np.abs(np.asarray(A, np.float64)))
    d = (r + 2) * 2.0 ** -24 * mag
    return f64_to_bf16_rne(x - d), f64_to_bf16_rne(x + d), x


def random_weights(rng, rows, cols):
    """bf16 bits of N(0, WEIGHT_STD) values."""
    return f64_to_bf16_rne(rng.standard_normal((rows, cols)) * WEIGHT_STD)


def dyadic_case(rows, cols, r, seed):
    """w random bf16, A and B integers in [-8, 8], scale 2^-12: every product and partial sum is an integer of at
    most 64 r <= 4096 in magnitude, exact in f32 in any order, with or without FMA, and scale * acc is exact."""
    rng = np.random.default_rng(seed)
    w = random_weights(rng, rows, cols)
    A = rng.integers(-8, 9, (r, cols)).astype(np.float32)
    B = rng.integers(-8, 9, (rows, r)).astype(np.float32)
    return w, A, B, DYADIC_SCALE


def real_case(rows, cols, r, seed):
    """A, B ~ 0.02 N(0, 1); scale 2 for the small ranks (the update stays above the weights' bf16 spacing) and 0.25
    for r >= 16."""
    rng = np.random.default_rng(seed)
    w = random_weights(rng, rows, cols)
    A = (0.02 * rng.standard_normal((r, cols))).astype(np.float32)
    B = (0.02 * rng.standard_normal((rows, r))).astype(np.float32)
    return w, A, B, (2.0 if r < 16 else 0.25)
