#!/usr/bin/env python
"""Measured worst errors of the long-frame kernels on the multi-trip batches of tests/long_frame_cases.py, per
trip of the grid-stride walk, against the CPU oracle.

    python tools/long_frames_errors.py > profiles/long_frames_seams_errors.txt

Per kernel, kind, snip_edges and trip: the rows that trip wrote, the worst absolute error, and the worst error
as a fraction of the bound of conftest.assert_close at rtol 1e-4 (the family's absolute term + 1e-4 |want|; a
spectrogram bin more than 60 dB under its frame's peak against the linear bound 1e-4 P + 1e-9 P_peak).  A record,
not a bound: a later trip that sat visibly above trip 0 would be a finding."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def fraction_of_bound(got, want, family, rtol=1e-4):
    """[rows]: the largest error / bound of each row"""
    import conftest
    g, w = got.astype(np.float64), want.astype(np.float64)
    err = np.abs(g - w)
    frac = err / (conftest.FAMILY_ATOL[family] + rtol * np.abs(w))
    if family == 'spectrogram':
        peak = w.max(axis=1, keepdims=True)
        null = w < peak - conftest.NULL_DB / 10.0 * np.log(10.0)
        pg, pw = np.exp(g - peak), np.exp(w - peak)
        frac = np.where(null, np.abs(pg - pw) / (1e-4 * pw + 1e-9), frac)
    return frac.max(axis=1), err.max(axis=1)


def main():
    import conftest
    import long_frame_cases as lf
    import test_long_frames_seams_gpu as seams
    from shennong_amd import _backend
    print('# long-frame kernels on', _backend.device_name(0).strip(), 'against the CPU oracle: batches of',
          'tests/long_frame_cases.py multi_trip_batch (8192 < pairs or frames < 12288, stride 4096)')
    print('# kernel  rate  kind  snip_edges  trip  rows  worst_abs_error  worst_error/bound')
    cases = seams.VALUE_CASES + [(seams.PAIRED, 32000, 'plp')]
    for kernel, rate, kind in cases:
        for snip_edges in (True, False):
            waves, warps = lf.multi_trip_batch(rate, snip_edges)
            proc = seams._proc(kind, rate, snip_edges)
            wants = seams._wants(kind, rate, snip_edges)
            if kind == 'plp':   # (NaN cepstra on digital silence, in the oracle too: those rows are left out)
                gots = _backend.get_plan(proc._build_options()).run(waves, warps, check_finite=False)
                gots, wants = seams.plp_without_silent_frames(gots, wants)
            else:
                gots = seams._run(proc, waves, warps, rate)
            assert seams._kernel(proc) == kernel
            family = conftest.family_of(proc.name)
            frac, err = fraction_of_bound(np.concatenate(gots), np.concatenate(wants), family)
            trips = lf.row_trips(waves, rate, snip_edges)
            for trip in (0, 1, 2, -1):
                rows = trips == trip
                if rows.any():
                    print('%s  %d  %s  %s  %s  %d  %.3g  %.3g' % (
                        kernel, rate, kind, snip_edges, trip if trip >= 0 else 'generic', int(rows.sum()),
                        err[rows].max(), frac[rows].max()))


if __name__ == '__main__':
    main()
