#!/usr/bin/env python
"""Measured worst errors of the DTW distances on the GPU against the float64 statement (tests/dtw_f64.py), on the
cases of tests/test_dtw_gpu.py: the 100 ordered pairs of the seam lengths, per D.

    python tools/dtw_errors.py > profiles/dtw_errors.txt

Cosine, standard-normal rows: the worst error of the normalised distance, the largest fraction of the derived
bound (tests/dtw_cases.py cosine_bound) that any pair uses, and whether every path length is equal.  Integer
rows, sqeuclidean: bit-equality.  Float rows, sqeuclidean, D = 39: the worst error of the cost and the largest
fraction of its bound."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import dtw_cases
    from shennong_amd import _backend, dtw_distances
    shapes = dtw_cases.pair_shapes()
    print('# DTW distances on', _backend.device_name(0).strip(), 'against tests/dtw_f64.py; lengths',
          list(dtw_cases.LENGTHS), '(100 ordered pairs per D)')
    print('# cosine, standard-normal rows: normalised distance')
    print('# D  min_margin  max_|cos|  lengths_equal  worst_error  worst_error/bound  smallest_bound')
    for dim in dtw_cases.COSINE_DIMS:
        xs, ys, (cost, length, margin, cosine) = dtw_cases.cosine_case(dim)
        feats, pairs = dtw_cases.two_set_collection(xs, ys)
        got, got_length = dtw_distances(feats, pairs, return_lengths=True)
        error = np.abs(got.astype(np.float64) - cost / length)
        bound = dtw_cases.cosine_bound(dim, shapes[:, 0], shapes[:, 1])
        print('%3d  %.3g  %.4f  %s  %.3g  %.3g  %.3g' % (
            dim, margin.min(), cosine.max(), bool(np.array_equal(got_length, length)), error.max(),
            (error / bound).max(), bound.min()))
    print('# sqeuclidean, integer rows in [-2, 2]: cost and length bit for bit')
    print('# D  pairs_with_a_margin-0_tie  cost_equal  lengths_equal')
    for dim in dtw_cases.EXACT_DIMS:
        xs, ys, (cost, length, margin, _) = dtw_cases.exact_case(dim)
        feats, pairs = dtw_cases.two_set_collection(xs, ys)
        got, got_length = dtw_distances(feats, pairs, metric='sqeuclidean', normalized=False, return_lengths=True)
        print('%3d  %d  %s  %s' % (dim, int((margin == 0).sum()), bool(np.array_equal(got, cost.astype(np.float32))),
                                   bool(np.array_equal(got_length, length))))
    print('# sqeuclidean, standard-normal rows, D = 39: cost')
    xs, ys = dtw_cases.item_sets('normal', 39, seed=4)
    cost, length, _, _ = dtw_cases.statement(xs, ys, 'sqeuclidean', margins=False)
    feats, pairs = dtw_cases.two_set_collection(xs, ys)
    got, got_length = dtw_distances(feats, pairs, metric='sqeuclidean', normalized=False, return_lengths=True)
    square = lambda m: (m.astype(np.float64) ** 2).sum(axis=1).max()   # noqa: E731
    scale = np.array([square(x) + square(y) for x in xs for y in ys])
    bound = dtw_cases.sqeuclidean_bound(39, shapes[:, 0], shapes[:, 1], scale, cost)
    error = np.abs(got.astype(np.float64) - cost)
    print('worst_error %.3g  worst_relative_error %.3g  worst_error/bound %.3g  lengths_equal %s' % (
        error.max(), (error / cost).max(), (error / bound).max(), bool(np.array_equal(got_length, length))))


if __name__ == '__main__':
    main()
