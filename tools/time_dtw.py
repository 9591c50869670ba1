#!/usr/bin/env python
"""Times the DTW distances (snf_dtw_pairs, shennong_amd.dtw.dtw_distances) on one MI355X, one JSON line per
workload.

    python tools/time_dtw.py [a b c] [--repeat 7] [--metric cosine [symkl ...]] [--out profiles/dtw_timing.jsonl]

Several metrics are timed one after the other in one process, a line each.  Workloads (everything seeded;
standard-normal float32 rows; for symkl rows of probabilities, the float32 softmax of twice such rows):
  a  1 000 000 pairs among 20 000 items of 5 to 30 frames, D = 39 (word-sized ABX items, a task file's worth)
  b  100 000 pairs among 5 000 items of 30 to 100 frames, D = 39
  c  10 000 pairs among 400 items of 298 frames, D = 40 (whole 3-second utterances)

Per workload, after one warm-up call, the median of `--repeat` runs of:
  event_ms  between two events on the call's stream, the first recorded before ``snf_dtw_pairs`` is called and the
            second behind its kernels.  The call checks, sorts and uploads its tables before it enqueues anything,
            so this is host table work + kernels: the whole C call on rows that are in HBM;
  call_ms   the wall clock of the same call, which returns once the kernels are enqueued: the host table work.
            (event_ms - call_ms is NOT the kernels' time: for workload (a) it came out at a third of what
            ``rocprofv3 --kernel-trace --stats`` reports.  The kernels alone: this command under rocprofv3, one
            workload per run);
  wall_ms   ``dtw_distances`` host to host on the device collection (item selection, the call, two downloads,
            the division).
pairs/s and cells/s (cells = sum of N M over the pairs) are given for event_ms and for wall_ms.  For scale only:
the float64 statement (tests/dtw_f64.py, numpy on one core) on 20 pairs of (c).  `--out` appends the lines."""
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
    'a': dict(items=20000, frames=(5, 30), pairs=1000000, dim=39),
    'b': dict(items=5000, frames=(30, 100), pairs=100000, dim=39),
    'c': dict(items=400, frames=(298, 298), pairs=10000, dim=40),
}


def make(spec, seed, metric='cosine'):
    """(host collection of one utterance per item, items, pairs)"""
    import dtw_cases
    rng = np.random.default_rng(seed)
    lo, hi = spec['frames']
    frames = rng.integers(lo, hi + 1, size=spec['items'])
    block = rng.standard_normal((int(frames.sum()), spec['dim']), dtype=np.float32)
    if metric == 'symkl':
        block = np.exp(2 * block - 2 * block.max(axis=1, keepdims=True))
        block /= block.sum(axis=1, keepdims=True)
    starts = np.concatenate([[0], np.cumsum(frames)[:-1]])
    feats = dtw_cases.collection([block[a:a + n] for a, n in zip(starts.tolist(), frames.tolist())])
    items = [('item%d' % k, 0.0, 1e9) for k in range(spec['items'])]
    pairs = rng.integers(0, spec['items'], size=(spec['pairs'], 2)).astype(np.int32)
    return feats, items, pairs, frames


def median(values):
    return float(np.median(values))


def run(name, args, metric):
    from shennong_amd import _backend, dtw
    from shennong_amd.device import DeviceFeaturesCollection
    import dtw_f64
    import symkl_f64
    spec = WORKLOADS[name]
    feats, items, pairs, frames = make(spec, seed=ord(name), metric=metric)
    cells = int((frames[pairs[:, 0]].astype(np.int64) * frames[pairs[:, 1]]).sum())
    resident = DeviceFeaturesCollection.from_host(feats)
    first, count, pairs32, dim, block = dtw._select(resident, pairs, items)
    n = pairs32.shape[0]
    L = _backend.lib()
    stream = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _backend.check(L.snf_event_create(C.byref(e)))
    d_cost, d_len = _backend.DeviceBuffer(4 * n), _backend.DeviceBuffer(4 * n)

    def call():
        _backend.dtw_pairs(block.buffer.ptr, dim, first, count, pairs32, metric, d_cost.ptr, d_len.ptr,
                           stream=stream.value)

    call()
    _backend.check(L.snf_stream_synchronize(stream))
    event_ms, call_ms = [], []
    for _ in range(args.repeat):
        _backend.check(L.snf_event_record(ev[0], stream))
        t0 = time.perf_counter()
        call()
        call_ms.append(1e3 * (time.perf_counter() - t0))
        _backend.check(L.snf_event_record(ev[1], stream))
        _backend.check(L.snf_event_synchronize(ev[1]))
        ms = C.c_float()
        _backend.check(L.snf_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        event_ms.append(ms.value)
    dtw.dtw_distances(resident, pairs, items=items, metric=metric)
    wall_ms = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        got = dtw.dtw_distances(resident, pairs, items=items, metric=metric)
        wall_ms.append(1e3 * (time.perf_counter() - t0))
    assert np.isfinite(got).all()
    line = {
        'workload': name, 'metric': metric, 'device': _backend.device_name(0), 'pairs': n, 'cells': cells,
        'items': spec['items'], 'frames': list(spec['frames']), 'dim': spec['dim'], 'repeat': args.repeat,
        'event_ms': sorted(event_ms), 'call_ms': sorted(call_ms), 'wall_ms': sorted(wall_ms),
        'event_median_ms': median(event_ms), 'call_median_ms': median(call_ms), 'wall_median_ms': median(wall_ms),
        'event_pairs_per_s': n / (1e-3 * median(event_ms)), 'event_cells_per_s': cells / (1e-3 * median(event_ms)),
        'wall_pairs_per_s': n / (1e-3 * median(wall_ms)), 'wall_cells_per_s': cells / (1e-3 * median(wall_ms)),
    }
    if name == 'c':   # for scale only: the float64 statement on 20 of these pairs, and agreement with it
        t0 = time.perf_counter()
        want = []
        for a, b in pairs[:20].tolist():
            x, y = feats['item%d' % a].data, feats['item%d' % b].data
            want.append(symkl_f64.dtw(x, y)[0] if metric == 'symkl' else dtw_f64.dtw(x, y, metric)[0])
        line['statement_f64_ms_per_pair'] = 1e3 * (time.perf_counter() - t0) / 20
        line['statement_max_abs_difference_20_pairs'] = float(np.abs(got[:20] - np.array(want)).max())
    for e in ev:
        L.snf_event_destroy(e)
    d_cost.free()
    d_len.free()
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
