#!/usr/bin/env python
"""Measured worst errors of the symkl DTW costs on the GPU against the float64 statement (tests/symkl_f64.py), on the
cases of tests/test_symkl_gpu.py: the 100 ordered pairs of the seam lengths, per D and kind of rows.

    python tools/symkl_errors.py > profiles/symkl_errors.txt

Per case: the number of pairs whose path margin is at least twice the derived bound (tests/symkl_cases.py), whether
the path lengths of those pairs are equal, the worst error of the cost, the worst relative error, and the largest
fraction of the bound that any pair uses.  And the dense posteriors (snf_gmm_posteriors) against the float64 softmax
of the downloaded log-likelihoods."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import dtw_cases
    import gmm_f64
    import symkl_cases
    from shennong_amd import _backend, dtw_distances
    from shennong_amd import gmm as G
    from test_ubm_gpu import mixture
    print('# symkl DTW costs on', _backend.device_name(0).strip(), 'against tests/symkl_f64.py; lengths',
          list(dtw_cases.LENGTHS), '(100 ordered pairs per case)')
    print('# D  kind  qualifying  lengths_equal_there  worst_error  worst_relative_error  worst_error/bound')
    for dim in symkl_cases.COST_ONLY_DIMS + symkl_cases.DIMS:
        for kind in symkl_cases.KINDS:
            xs, ys, (cost, length, margin, max_a, bound), q = symkl_cases.case(kind, dim)
            feats, pairs = dtw_cases.two_set_collection(xs, ys)
            got, got_length = dtw_distances(feats, pairs, metric='symkl', normalized=False, return_lengths=True)
            error = np.abs(got.astype(np.float64) - cost)
            print('%3d  %-7s  %3d  %s  %.3g  %.3g  %.3g' % (
                dim, kind, int(q.sum()), bool(np.array_equal(got_length[q], length[q])), error.max(),
                (error / cost).max(), (error / bound).max()))
    print('# dense posteriors against exp(L - logsumexp(L)) in float64 on the downloaded L (mixture model of '
          'tests/test_ubm_gpu.py)')
    print('# F  C  D  worst_error  worst_|row_sum - 1|')
    for F, C, D in ((130, 130, 39), (1000, 64, 39), (1000, 1024, 39), (1000, 2048, 13)):
        x, gmm = mixture(F + C + D, F, D, C)
        block, dg = G.FrameBlock([x]), G.DeviceGmm(gmm)
        L = block.loglikes(dg).astype(np.float64)
        want = np.exp(L - gmm_f64.logsumexp(L, axis=1)[:, None])
        post = block.posteriors(dg)
        print('%5d  %4d  %2d  %.3g  %.3g' % (F, C, D, np.abs(post - want).max(),
                                             np.abs(post.astype(np.float64).sum(axis=1) - 1).max()))


if __name__ == '__main__':
    main()
