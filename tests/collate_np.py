"""The collation rule of snf_collate_padded (include/shennong_amd.h) as a plain numpy loop, with its two
roundings written out: the checker of tests/test_device_out.py and tests/test_device_out_gpu.py."""

import numpy as np


def num_out(frames, subsample, offset):
    """Frames offset, offset + subsample, ... below `frames`"""
    return 0 if frames <= offset else (frames - offset + subsample - 1) // subsample


def round_bf16(x):
    """float32 -> bfloat16 bit patterns (uint16): to nearest, ties to even; a NaN stays a NaN (quiet, sign kept);
    subnormals are rounded like every other value"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (bits >> 16) | 0x40, rounded).astype(np.uint16)


def round_f16(x):
    """float32 -> IEEE binary16 bit patterns (uint16): numpy's conversion is to nearest even with overflow to
    infinity"""
    with np.errstate(over='ignore'):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


CASTS = {'float32': lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.uint32),
         'float16': round_f16, 'bfloat16': round_bf16}


def collate(rows, foff, dtype, left, right, subsample, offset, pad_value, t_max):
    """`rows` float32 [foff[-1], dim] -> (bit patterns [B, t_max, dim (left + 1 + right)], lengths int32 [B])"""
    rows = np.asarray(rows, dtype=np.float32)
    dim = rows.shape[1]
    cast = CASTS[dtype]
    n = len(foff) - 1
    width = left + 1 + right
    out = np.empty((n, t_max, width * dim), dtype=cast(np.zeros(1, np.float32)).dtype)
    out[...] = cast(np.array([pad_value], dtype=np.float32))[0]
    lengths = np.zeros(n, dtype=np.int32)
    for u in range(n):
        frames = int(foff[u + 1] - foff[u])
        lengths[u] = num_out(frames, subsample, offset)
        for j in range(lengths[u]):
            for k in range(-left, right + 1):
                t = min(max(offset + j * subsample + k, 0), frames - 1)
                out[u, j, (k + left) * dim:(k + left + 1) * dim] = cast(rows[foff[u] + t])
    return out, lengths


def same_bits(got, want, dtype):
    """Equal bit patterns, except that a NaN only has to be a NaN (its payload is the converter's)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    exponent, mantissa = {'float32': (0x7F800000, 0x007FFFFF), 'float16': (0x7C00, 0x03FF),
                          'bfloat16': (0x7F80, 0x007F)}[dtype]

    def is_nan(bits):
        return ((bits & exponent) == exponent) & ((bits & mantissa) != 0)
    nan_got, nan_want = is_nan(got), is_nan(want)
    return bool(np.array_equal(nan_got, nan_want) and np.array_equal(got[~nan_got], want[~nan_want]))


def special_rows(rows):
    """`rows` with the values a rounding can get wrong written over its first entries (as many as fit)"""
    specials = np.array([
        1.00390625, 1.01171875, -1.00390625,       # bfloat16 ties: to even down, to even up, negative
        1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,    # float16 ties
        65519.9, 65520.0, -70000.0,                # float16: the largest that stays finite, overflow both ways
        1e-6, 6e-8, 2.9e-8, 1e-40, -1e-40,         # float16 subnormals and underflow, float32 subnormals
        3.3895314e38,                              # bfloat16: rounds up to infinity
        np.inf, -np.inf, np.nan, -0.0, 0.0], dtype=np.float32)
    flat = rows.reshape(-1)
    count = min(flat.size, specials.size)
    flat[:count] = specials[:count]
    return rows
