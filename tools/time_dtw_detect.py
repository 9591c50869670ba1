#!/usr/bin/env python
"""Times the detections and the top-k of the search (snf_dtw_detect, snf_dtw_topk, shennong_amd.dtw.dtw_detect)
against snf_dtw_search on one MI355X, one JSON line per workload.

    python tools/time_dtw_detect.py [a b] [--repeat 7] [--k 4] [--out profiles/dtw_detect_timing.jsonl]
    python tools/time_dtw_detect.py a b --search-only        # snf_dtw_search alone: for A/B runs of two builds of
                                                             # the library (SHENNONG_AMD_LIB), alternated by the caller

Workloads: (a) and (b) of tools/time_dtw_search.py (everything seeded; cosine, D = 39; every query against every
target).  Per workload, after one warm-up call, the median of `--repeat` runs, the protocol of that tool - the whole
C call between two events on the call's stream, host table work included - in one process on one box:
  detect_event_ms   ``snf_dtw_detect`` with K = `--k` detections per pair, no threshold, no curves;
  search_event_ms   ``snf_dtw_search`` on the same pair table: `detect_over_search` is the ratio of the two medians;
  topk_event_ms     ``snf_dtw_topk`` with T = `--top-k` over the arrays that the detection left on the device.
For (b) also three host-to-host figures on the device collection (selection, the calls, the downloads, the times):
  detect_wall_ms        ``dtw_detect(max_detections=K)``;
  detect_topk_wall_ms   ``dtw_detect(max_detections=K, top_k=T)``;
  curves_greedy_wall_ms ``dtw_search(return_curves=True)`` and then the greedy of the statement
                        (tests/dtw_detect_f64.py ``detections``, numpy, float32) on every curve on the host: what a
                        user did before; `--host-repeat` runs, it takes seconds.
The detections of the last run are compared with that host greedy (`equal_to_host_greedy`).  `--out` appends."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import time_dtw_search  # noqa: E402

WORKLOADS = {name: time_dtw_search.WORKLOADS[name] for name in ('a', 'b')}
median = time_dtw_search.median


def run(name, args):
    from shennong_amd import _backend, dtw
    from shennong_amd.device import DeviceFeaturesCollection
    import dtw_detect_f64
    spec = WORKLOADS[name]
    feats, queries, targets, frames = time_dtw_search.make(spec, seed=ord(name))
    resident = DeviceFeaturesCollection.from_host(feats)
    first, count, pairs, n_queries, _, dim, block = dtw._select_search(resident, queries, targets, None)
    index_pairs = pairs + np.array([0, n_queries], dtype=np.int32)
    n, k, t = pairs.shape[0], args.k, args.top_k
    cells = int((count[index_pairs[:, 0]].astype(np.int64) * count[index_pairs[:, 1]]).sum())
    L = _backend.lib()
    stream = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _backend.check(L.snf_event_create(C.byref(e)))
    line = {
        'workload': name, 'metric': 'cosine', 'device': _backend.device_name(0), 'pairs': n, 'cells': cells,
        'queries': spec['queries'], 'query_frames': list(spec['query_frames']), 'targets': spec['targets'],
        'target_frames': spec['target_frames'], 'dim': spec['dim'], 'repeat': args.repeat,
        'library': os.environ.get('SHENNONG_AMD_LIB', ''),
    }
    found = [_backend.DeviceBuffer(4 * n) for _ in range(4)]

    def search():
        _backend.dtw_search(block.buffer.ptr, dim, first, count, index_pairs, 'cosine', True,
                            *[b.ptr for b in found], stream=stream.value)

    event_ms, call_ms = time_dtw_search.timed(L, _backend, stream, ev, search, args.repeat)
    line.update(search_event_ms=sorted(event_ms), search_event_median_ms=median(event_ms),
                search_call_median_ms=median(call_ms))
    for b in found:
        b.free()
    if not args.search_only:
        line.update(max_detections=k, top_k=t)
        slots = [_backend.DeviceBuffer(4 * n)] + [_backend.DeviceBuffer(4 * n * k) for _ in range(4)]
        best = [_backend.DeviceBuffer(4 * n_queries)] + [_backend.DeviceBuffer(4 * n_queries * t) for _ in range(6)]
        order = np.argsort(pairs[:, 0], kind='stable').astype(np.int32)
        bounds = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=n_queries))])

        def detect():
            _backend.dtw_detect(block.buffer.ptr, dim, first, count, index_pairs, 'cosine', True, k, None,
                                *[b.ptr for b in slots], stream=stream.value)

        def topk():
            _backend.dtw_topk(*[b.ptr for b in slots], n, k, True, order, bounds, t, *[b.ptr for b in best],
                              stream=stream.value)

        event_ms, call_ms = time_dtw_search.timed(L, _backend, stream, ev, detect, args.repeat)
        line.update(detect_event_ms=sorted(event_ms), detect_event_median_ms=median(event_ms),
                    detect_call_median_ms=median(call_ms),
                    detect_over_search=median(event_ms) / line['search_event_median_ms'],
                    detect_cells_per_s=cells / (1e-3 * median(event_ms)))
        event_ms, call_ms = time_dtw_search.timed(L, _backend, stream, ev, topk, args.repeat)
        line.update(topk_event_ms=sorted(event_ms), topk_event_median_ms=median(event_ms))
        counts = slots[0].download(np.zeros(n, dtype=np.int32))
        line['detections'] = int(counts.sum())
        for b in slots + best:
            b.free()
    if not args.search_only and name == 'b':
        for key, kwargs in (('detect_wall_ms', {}), ('detect_topk_wall_ms', dict(top_k=t))):
            dtw.dtw_detect(resident, queries, targets, max_detections=k, **kwargs)
            wall_ms = []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                hits = dtw.dtw_detect(resident, queries, targets, max_detections=k, **kwargs)
                wall_ms.append(1e3 * (time.perf_counter() - t0))
            line[key] = sorted(wall_ms)
            line[key.replace('_ms', '_median_ms')] = median(wall_ms)
            line[key.replace('_wall_ms', '_rows')] = len(hits)
        hits = dtw.dtw_detect(resident, queries, targets, max_detections=k)
        wall_ms, greedy_ms = [], []
        for _ in range(args.host_repeat):
            t0 = time.perf_counter()
            searched = dtw.dtw_search(resident, queries, targets, return_curves=True)
            t1 = time.perf_counter()
            rows = [dtw_detect_f64.detections(*searched.curve(p), k, True, None, np.float32) for p in range(n)]
            wall_ms.append(1e3 * (time.perf_counter() - t0))
            greedy_ms.append(1e3 * (time.perf_counter() - t1))
        line.update(curves_greedy_wall_ms=sorted(wall_ms), curves_greedy_wall_median_ms=median(wall_ms),
                    host_greedy_median_ms=median(greedy_ms), host_repeat=args.host_repeat)
        flat = [found for per_pair in rows for found in per_pair]
        line['equal_to_host_greedy'] = bool(
            len(flat) == len(hits) and hits.counts.tolist() == [len(per_pair) for per_pair in rows] and
            np.array_equal(hits.end_frame, [f[4] for f in flat]) and
            np.array_equal(hits.start_frame, [f[3] for f in flat]) and
            hits.score.tobytes() == np.array([f[0] for f in flat], dtype=np.float32).tobytes())
        line['wall_curves_greedy_over_detect'] = line['curves_greedy_wall_median_ms'] / line['detect_wall_median_ms']
        line['wall_curves_greedy_over_detect_topk'] = \
            line['curves_greedy_wall_median_ms'] / line['detect_topk_wall_median_ms']
    for e in ev:
        L.snf_event_destroy(e)
    resident.release()
    return line


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('workloads', nargs='*', help='a, b (default: both)')
    parser.add_argument('--repeat', type=int, default=7)
    parser.add_argument('--host-repeat', type=int, default=3)
    parser.add_argument('--k', type=int, default=4)
    parser.add_argument('--top-k', type=int, default=10)
    parser.add_argument('--search-only', action='store_true')
    parser.add_argument('--out')
    args = parser.parse_args()
    if set(args.workloads) - set(WORKLOADS):
        parser.error('workloads are ' + ', '.join(sorted(WORKLOADS)))
    for name in args.workloads or sorted(WORKLOADS):
        line = json.dumps(run(name, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
