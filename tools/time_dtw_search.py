#!/usr/bin/env python
"""Times the subsequence DTW search (snf_dtw_search, shennong_amd.dtw.dtw_search) on one MI355X, one JSON line per
workload.

    python tools/time_dtw_search.py [a b c] [--repeat 7] [--metric cosine] [--out profiles/dtw_search_timing.jsonl]

Workloads (everything seeded; standard-normal float32 rows, D = 39; for symkl rows of probabilities as in
tools/time_dtw.py); every query against every target:
  a  1 000 queries of 30 to 100 frames x 1 000 targets of 298 frames (words in 3-second utterances)
  b  100 queries of 30 to 100 frames x 1 000 targets of 3 000 frames (words in 30-second utterances)
  c  the same as b, with the curves (C, L, B of every end of every pair: 3 x 300 000 000 elements)

Per workload, after one warm-up call, the median of `--repeat` runs, the protocol of tools/time_dtw.py:
  event_ms        between two events on the call's stream, the first recorded before ``snf_dtw_search`` is called
                  and the second behind its kernels: host table work + kernels, the whole C call on rows in HBM;
  call_ms         the wall clock of the same call, which returns once the kernels are enqueued: the host table work;
  pairs_event_ms  event_ms of ``snf_dtw_pairs`` on the same pair table - the same lattices, end to end instead of
                  free ends - for comparison: `search_over_pairs` is the ratio of the two medians;
  wall_ms         ``dtw_search`` host to host on the device collection (selection, the call, the downloads, the
                  times of the matches).
pairs/s and cells/s (cells = sum of N M over the pairs) are given for event_ms and for wall_ms.  For scale only: the
float64 statement (tests/dtw_search_f64.py, numpy on one core) on 20 pairs.  `--out` appends the lines."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WORKLOADS = {
    'a': dict(queries=1000, query_frames=(30, 100), targets=1000, target_frames=298, dim=39, curves=False),
    'b': dict(queries=100, query_frames=(30, 100), targets=1000, target_frames=3000, dim=39, curves=False),
    'c': dict(queries=100, query_frames=(30, 100), targets=1000, target_frames=3000, dim=39, curves=True),
}


def make(spec, seed, metric='cosine'):
    """(host collection of one utterance per item, query names, target names, frames of every item)"""
    import dtw_cases
    rng = np.random.default_rng(seed)
    lo, hi = spec['query_frames']
    frames = np.concatenate([rng.integers(lo, hi + 1, size=spec['queries']),
                             np.full(spec['targets'], spec['target_frames'])])
    block = rng.standard_normal((int(frames.sum()), spec['dim']), dtype=np.float32)
    if metric == 'symkl':
        block = np.exp(2 * block - 2 * block.max(axis=1, keepdims=True))
        block /= block.sum(axis=1, keepdims=True)
    starts = np.concatenate([[0], np.cumsum(frames)[:-1]])
    feats = dtw_cases.collection([block[a:a + n] for a, n in zip(starts.tolist(), frames.tolist())])
    names = list(feats)
    return feats, names[:spec['queries']], names[spec['queries']:], frames


def median(values):
    return float(np.median(values))


def timed(L, backend, stream, ev, call, repeat):
    """(event_ms, call_ms) of `repeat` runs of `call` after one warm-up"""
    call()
    backend.check(L.snf_stream_synchronize(stream))
    event_ms, call_ms = [], []
    for _ in range(repeat):
        backend.check(L.snf_event_record(ev[0], stream))
        t0 = time.perf_counter()
        call()
        call_ms.append(1e3 * (time.perf_counter() - t0))
        backend.check(L.snf_event_record(ev[1], stream))
        backend.check(L.snf_event_synchronize(ev[1]))
        ms = C.c_float()
        backend.check(L.snf_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        event_ms.append(ms.value)
    return event_ms, call_ms


def run(name, args, metric):
    from shennong_amd import _backend, dtw
    from shennong_amd.device import DeviceFeaturesCollection
    import dtw_search_f64
    spec = WORKLOADS[name]
    feats, queries, targets, frames = make(spec, seed=ord(name if name != 'c' else 'b'), metric=metric)
    resident = DeviceFeaturesCollection.from_host(feats)
    first, count, pairs, n_queries, _, dim, block = dtw._select_search(resident, queries, targets, None)
    index_pairs = pairs + np.array([0, n_queries], dtype=np.int32)
    n = pairs.shape[0]
    cells = int((count[index_pairs[:, 0]].astype(np.int64) * count[index_pairs[:, 1]]).sum())
    columns = count[index_pairs[:, 1]].astype(np.int64)
    curve_first = np.concatenate([[0], np.cumsum(columns)])
    L = _backend.lib()
    stream = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _backend.check(L.snf_event_create(C.byref(e)))
    outputs = [_backend.DeviceBuffer(4 * n) for _ in range(4)]
    curves = {}
    if spec['curves']:
        curves = dict(curve_first=curve_first[:-1])
        for key in ('d_curve_cost', 'd_curve_len', 'd_curve_start'):
            outputs.append(_backend.DeviceBuffer(4 * int(curve_first[-1])))
            curves[key] = outputs[-1].ptr

    def search():
        _backend.dtw_search(block.buffer.ptr, dim, first, count, index_pairs, metric, True,
                            *[b.ptr for b in outputs[:4]], stream=stream.value, **curves)

    def whole_pairs():
        _backend.dtw_pairs(block.buffer.ptr, dim, first, count, index_pairs, metric, outputs[0].ptr, outputs[1].ptr,
                           stream=stream.value)

    event_ms, call_ms = timed(L, _backend, stream, ev, search, args.repeat)
    pairs_event_ms, _ = timed(L, _backend, stream, ev, whole_pairs, args.repeat)
    for b in outputs:
        b.free()
    dtw.dtw_search(resident, queries, targets, metric=metric, return_curves=spec['curves'])
    wall_ms = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        found = dtw.dtw_search(resident, queries, targets, metric=metric, return_curves=spec['curves'])
        wall_ms.append(1e3 * (time.perf_counter() - t0))
    assert np.isfinite(found.score).all()
    line = {
        'workload': name, 'metric': metric, 'device': _backend.device_name(0), 'pairs': n, 'cells': cells,
        'queries': spec['queries'], 'query_frames': list(spec['query_frames']), 'targets': spec['targets'],
        'target_frames': spec['target_frames'], 'dim': spec['dim'], 'curves': spec['curves'],
        'curve_elements': int(curve_first[-1]) if spec['curves'] else 0, 'repeat': args.repeat,
        'event_ms': sorted(event_ms), 'call_ms': sorted(call_ms), 'pairs_event_ms': sorted(pairs_event_ms),
        'wall_ms': sorted(wall_ms),
        'event_median_ms': median(event_ms), 'call_median_ms': median(call_ms),
        'pairs_event_median_ms': median(pairs_event_ms), 'wall_median_ms': median(wall_ms),
        'search_over_pairs': median(event_ms) / median(pairs_event_ms),
        'event_pairs_per_s': n / (1e-3 * median(event_ms)), 'event_cells_per_s': cells / (1e-3 * median(event_ms)),
        'wall_pairs_per_s': n / (1e-3 * median(wall_ms)), 'wall_cells_per_s': cells / (1e-3 * median(wall_ms)),
    }
    # for scale only: the float64 statement on 20 of these pairs, and agreement with it
    t0 = time.perf_counter()
    want = [dtw_search_f64.search(feats[queries[q]].data, feats[targets[t]].data, metric)
            for q, t in pairs[:20].tolist()]
    line['statement_f64_ms_per_pair'] = 1e3 * (time.perf_counter() - t0) / 20
    line['statement_max_abs_score_difference_20_pairs'] = float(
        np.abs(found.score[:20] - np.array([w[0] for w in want])).max())
    line['statement_equal_ends_20_pairs'] = int(sum(
        (int(found.start_frame[k]), int(found.end_frame[k])) == w[3:] for k, w in enumerate(want)))
    for e in ev:
        L.snf_event_destroy(e)
    resident.release()
    return line


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('workloads', nargs='*', help='a, b, c (default: all)')
    parser.add_argument('--repeat', type=int, default=7)
    parser.add_argument('--metric', nargs='+', default=['cosine'])
    parser.add_argument('--out')
    args = parser.parse_args()
    if set(args.workloads) - set(WORKLOADS):
        parser.error('workloads are ' + ', '.join(sorted(WORKLOADS)))
    for name in args.workloads or sorted(WORKLOADS):
        for metric in args.metric:
            line = json.dumps(run(name, args, metric))
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as fh:
                    fh.write(line + '\n')


if __name__ == '__main__':
    main()
