"""The shares of the workgroups of fbank512b_kernel (kernels_fbank512b.hip, DEAL): workgroup b of `blocks` deals the
frame sets [lo, hi) to its waves.  A host function of three numbers (fbank512b_share through the test aid
snf_debug_fbank512b_share): no device, no audio.

The shares tile [0, n_sets) exactly, in order, with no set missing or twice, and differ by at most one set.
"""
import ctypes

import pytest

N_SETS = [0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 739249, 2 ** 28 - 1]


def _share(n_sets, blocks, block):
    from shennong_amd import _backend
    lo, hi = ctypes.c_int64(-1), ctypes.c_int64(-1)
    launched = _backend.lib().snf_debug_fbank512b_share(n_sets, blocks, block, ctypes.byref(lo), ctypes.byref(hi))
    assert launched >= 0, launched
    return lo.value, hi.value, launched


@pytest.mark.parametrize('n_sets', N_SETS)
def test_shares_tile_the_sets_in_order(n_sets):
    blocks = min(256, -(-n_sets // 16))
    sizes, end = [], 0
    for b in range(blocks):
        lo, hi, launched = _share(n_sets, blocks, b)
        assert launched == blocks          # the launcher starts as many workgroups as the test assumes
        assert lo == end and hi >= lo      # in order: no set missing, none twice
        sizes.append(hi - lo)
        end = hi
    assert end == n_sets
    if blocks:
        assert max(sizes) - min(sizes) <= 1
        assert min(sizes) >= 1             # no workgroup without a set
        # fewer than 256 workgroups: no share above the 16 waves' first sets
        assert blocks == 256 or max(sizes) <= 16
    else:
        assert n_sets == 0 and _share(0, 0, 0)[:2] == (0, 0)


def test_an_uneven_count_gives_shares_of_two_sizes_the_larger_ones_first():
    n_sets = 739249  # = 256 * 2887 + 177
    sizes = [hi - lo for lo, hi, _ in (_share(n_sets, 256, b) for b in range(256))]
    assert sizes == [2888] * 177 + [2887] * 79 and sum(sizes) == n_sets


def test_a_workgroup_outside_the_launch_is_refused():
    from shennong_amd import _backend
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    lib = _backend.lib()
    assert lib.snf_debug_fbank512b_share(100, 7, 8, ctypes.byref(lo), ctypes.byref(hi)) < 0
    assert lib.snf_debug_fbank512b_share(-1, 7, 0, ctypes.byref(lo), ctypes.byref(hi)) < 0
    assert lib.snf_debug_fbank512b_share(100, 7, 0, None, ctypes.byref(hi)) < 0
