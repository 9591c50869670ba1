#!/usr/bin/env python
"""Measured worst errors of the subsequence DTW search on the GPU against the float64 statement
(tests/dtw_search_f64.py), on the cases of tests/test_dtw_search_gpu.py: every query against every target of the
seam lengths, all 6 200 ends of the 100 pairs, per D.

    python tools/dtw_search_errors.py > profiles/dtw_search_errors.txt

Cosine, standard-normal rows: the worst error of the normalised score C / L over all ends, the largest fraction of
the derived bound (tests/dtw_cases.py cosine_bound) that any end uses, the ends whose margin is at least MIN_MARGIN and
whether L and B are equal there, the ends where they differ at all, the pairs whose best end leads by twice the bound
and whether (start, end, length) are equal there.  symkl, rows of probabilities: the same for the unnormalised cost
and the bound of tests/symkl_cases.py, an end qualifying when its margin is at least twice its bound.  Integer rows,
sqeuclidean: bit-equality of every end and of the best, for both rankings."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def measure(found, answers, bound_of, qualifies, normalized):
    import dtw_search_f64
    worst = ratio = 0.0
    ends = qualifying = equal_qualifying = different = decided = equal_decided = 0
    for p, a in enumerate(answers):
        cost, length, start = found.curve(p)
        bound = np.broadcast_to(bound_of(a), a.cost.shape)
        truth = dtw_search_f64.scores(a.cost, a.length, normalized)
        got = cost.astype(np.float64) / length if normalized else cost.astype(np.float64)
        error = np.abs(got - truth)
        worst, ratio = max(worst, error.max()), max(ratio, (error / bound).max())
        mask = qualifies(a, bound)
        same = (length == a.length) & (start == a.start)
        ends += mask.size
        qualifying += int(mask.sum())
        equal_qualifying += int((mask & same).sum())
        different += int((~same).sum())
        ranked = np.sort(truth)
        if truth.size >= 2 and ranked[1] - ranked[0] >= 2 * bound.max():
            decided += 1
            best = (int(found.length[p]), int(found.start_frame[p]), int(found.end_frame[p]))
            equal_decided += best == a.best(normalized)[2:]
    return '%.3g  %.3g  %d  %d  %d  %d  %d  %d' % (worst, ratio, ends, qualifying, equal_qualifying, different,
                                                  decided, equal_decided)


def main():
    import dtw_cases
    import dtw_search_cases
    from shennong_amd import _backend, dtw_search
    print('# subsequence DTW search on', _backend.device_name(0).strip(), 'against tests/dtw_search_f64.py; lengths',
          list(dtw_cases.LENGTHS), '(100 query x target pairs, 6200 ends per D)')
    columns = ('worst_error  worst_error/bound  ends  qualifying_ends  of_them_L_and_B_equal  '
               'ends_with_L_or_B_different  decided_pairs  of_them_best_equal')
    print('# cosine, standard-normal rows: normalised score at every end')
    print('# D ', columns)
    for dim in dtw_search_cases.COSINE_DIMS:
        xs, ys, answers = dtw_search_cases.cosine_case(dim)
        feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
        found = dtw_search(feats, queries, targets, return_curves=True)
        print('%3d ' % dim, measure(found, answers, lambda a: dtw_cases.cosine_bound(dim, *a.shape),
                                    lambda a, b: a.margin >= dtw_cases.MIN_MARGIN, True))
    print('# symkl, rows of probabilities: unnormalised cost at every end')
    print('# kind D ', columns)
    for kind, dim in dtw_search_cases.SYMKL_CASES:
        xs, ys, answers = dtw_search_cases.symkl_case(kind, dim)
        feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
        found = dtw_search(feats, queries, targets, metric='symkl', normalized=False, return_curves=True)
        print('%s %3d ' % (kind, dim), measure(found, answers, lambda a: dtw_search_cases.symkl_bound(a, dim),
                                                lambda a, b: a.margin >= 2 * b, False))
    print('# sqeuclidean, integer rows in [-2, 2]: (C, L, B) of every end and the best of every pair, bit for bit')
    print('# D  normalized  pairs_whose_best_end_depends_on_the_ranking  curves_equal  best_equal')
    for dim in dtw_search_cases.EXACT_DIMS:
        xs, ys, answers = dtw_search_cases.exact_case(dim)
        feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
        depends = sum(a.best(True, np.float32)[4] != a.best(False, np.float32)[4] for a in answers)
        for normalized in (False, True):
            found = dtw_search(feats, queries, targets, metric='sqeuclidean', normalized=normalized,
                               return_curves=True)
            curves = best = True
            for p, a in enumerate(answers):
                cost, length, start = found.curve(p)
                curves &= bool(np.array_equal(cost, a.cost.astype(np.float32)) and np.array_equal(length, a.length)
                               and np.array_equal(start, a.start))
                want = a.best(normalized, np.float32)
                best &= (float(found.score[p]), float(found.cost[p]), int(found.length[p]),
                         int(found.start_frame[p]), int(found.end_frame[p])) == tuple(float(v) if k < 2 else v
                                                                                      for k, v in enumerate(want))
            print('%3d  %s  %d  %s  %s' % (dim, normalized, depends, curves, best))


if __name__ == '__main__':
    main()
