#!/usr/bin/env python
"""Times the warping paths (snf_dtw_align) against the sibling call that returns the summary alone, on the same pair
tables in one process on one MI355X, one JSON line per workload.

    python tools/time_dtw_align.py [pa pc sb] [--repeat 7] [--k 4] [--out profiles/dtw_align_timing.jsonl]
    python tools/time_dtw_align.py pc --only align        # the alignment alone: for a run under rocprofv3
    python tools/time_dtw_align.py pa pc --only sibling   # the sibling alone: for A/B runs of two builds of the
                                                          # library (SHENNONG_AMD_LIB), alternated by the caller

Workloads (everything seeded; cosine):
  pa  workload (a) of tools/time_dtw.py: 1 000 000 pairs among 20 000 items of 5 to 30 frames, D = 39   global
  pc  workload (c) of tools/time_dtw.py: 10 000 pairs among 400 items of 298 frames, D = 40               global
  sb  workload (b) of tools/time_dtw_search.py: 100 queries of 30 to 100 frames against 1000 targets of 3000
      frames, D = 39                                                                                     subsequence
Per workload, after one warm-up call, the median of `--repeat` runs of the whole C call between two events on the
call's stream (host table work included: the protocol of tools/time_dtw.py):
  global       ``snf_dtw_pairs`` and ``snf_dtw_align`` (SNF_DTW_ALIGN_GLOBAL): `align_over_pairs`;
  subsequence  ``snf_dtw_search`` and ``snf_dtw_align`` with one slot: `align_over_search`; ``snf_dtw_detect`` and
               ``snf_dtw_align`` with K = `--k` slots: `align_over_detect`.
The results of the last runs are compared bit for bit (`equal_to_sibling`), and `record_bytes`, `runs` say what the
decisions took of the scratch (`--scratch-bytes`, 0: the default of 1 GiB).  The lattice and the traceback kernels
apart: this command with `--only align` under ``rocprofv3 --kernel-trace --stats``.  `--out` appends the lines."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import time_dtw  # noqa: E402
import time_dtw_search  # noqa: E402

WORKLOADS = {'pa': ('global', time_dtw.WORKLOADS['a'], 'a'), 'pc': ('global', time_dtw.WORKLOADS['c'], 'c'),
             'sb': ('subsequence', time_dtw_search.WORKLOADS['b'], 'b')}
median = time_dtw_search.median


def run(name, args):
    from shennong_amd import _backend, dtw
    from shennong_amd.device import DeviceFeaturesCollection
    mode, spec, seed = WORKLOADS[name]
    if mode == 'global':
        feats, items, pairs, _ = time_dtw.make(spec, seed=ord(seed))
        resident = DeviceFeaturesCollection.from_host(feats)
        first, count, index_pairs, dim, block = dtw._select(resident, pairs, items)
    else:
        feats, queries, targets, _ = time_dtw_search.make(spec, seed=ord(seed))
        resident = DeviceFeaturesCollection.from_host(feats)
        first, count, pairs, n_queries, _, dim, block = dtw._select_search(resident, queries, targets, None)
        index_pairs = pairs + np.array([0, n_queries], dtype=np.int32)
    n = index_pairs.shape[0]
    rows, columns = count[index_pairs[:, 0]].astype(np.int64), count[index_pairs[:, 1]].astype(np.int64)
    L = _backend.lib()
    stream = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _backend.check(L.snf_event_create(C.byref(e)))
    record_bytes = _backend.dtw_record_bytes(rows, columns)
    scratch = args.scratch_bytes or 2 ** 30
    line = {'workload': name, 'mode': mode, 'metric': 'cosine', 'device': _backend.device_name(0), 'pairs': n,
            'cells': int((rows * columns).sum()), 'dim': int(dim), 'repeat': args.repeat,
            'library': os.environ.get('SHENNONG_AMD_LIB', ''), 'record_bytes': int(record_bytes.sum()),
            'scratch_bytes': int(scratch), 'runs_at_least': int(-(-int(record_bytes.sum()) // scratch))}
    rows_ptr = block.buffer.ptr

    def timed(call):
        event_ms, _ = time_dtw_search.timed(L, _backend, stream, ev, call, args.repeat)
        return sorted(event_ms), median(event_ms)

    def results(buffers, dtypes):
        return [b.download(np.zeros(b.nbytes // 4, dtype=t)).tobytes() for b, t in zip(buffers, dtypes)]

    def with_slots(k, sibling, key):
        """`sibling(out)` against the alignment with k slots a pair, on buffers of their own"""
        kinds = (np.int32, np.float32, np.int32, np.int32, np.int32)
        sizes = (n, n * k, n * k, n * k, n * k)
        theirs = [_backend.DeviceBuffer(4 * s) for s in sizes]
        if args.only != 'align':
            line[key + '_event_ms'], line[key + '_event_median_ms'] = timed(lambda: sibling(theirs))
        if args.only != 'sibling':
            mine = [_backend.DeviceBuffer(4 * s) for s in sizes]
            room = (rows + columns - 1).repeat(k)
            path_first = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64)
            paths = [_backend.DeviceBuffer(4 * int(room.sum())) for _ in range(2)]
            tag = 'align' if mode == 'global' else 'align_k%d' % k

            def align():
                _backend.dtw_align(rows_ptr, dim, first, count, index_pairs, 'cosine', mode, mine[1].ptr, mine[2].ptr,
                                   path_first, paths[0].ptr, paths[1].ptr, normalized=True, max_detections=k,
                                   d_count=mine[0].ptr, d_start=mine[3].ptr, d_end=mine[4].ptr,
                                   scratch_bytes=args.scratch_bytes, stream=stream.value)

            line[tag + '_event_ms'], line[tag + '_event_median_ms'] = timed(align)
            line[tag + '_path_room_cells'] = int(room.sum())
            if args.only is None:
                line['align_over_' + key] = line[tag + '_event_median_ms'] / line[key + '_event_median_ms']
                used = slice(1, 3) if mode == 'global' else slice(0 if key == 'detect' else 1, 5)
                line['equal_to_' + key] = results(mine[used], kinds[used]) == results(theirs[used], kinds[used])
            length = mine[2].download(np.zeros(n * k, dtype=np.int32))
            line[tag + '_path_cells'] = int(length.sum())
            for b in mine + paths:
                b.free()
        for b in theirs:
            b.free()

    if mode == 'global':
        with_slots(1, lambda out: _backend.dtw_pairs(rows_ptr, dim, first, count, index_pairs, 'cosine', out[1].ptr,
                                                     out[2].ptr, stream=stream.value), 'pairs')
    else:
        with_slots(1, lambda out: _backend.dtw_search(rows_ptr, dim, first, count, index_pairs, 'cosine', True,
                                                      *[b.ptr for b in out[1:]], stream=stream.value), 'search')
        with_slots(args.k, lambda out: _backend.dtw_detect(rows_ptr, dim, first, count, index_pairs, 'cosine', True,
                                                           args.k, None, *[b.ptr for b in out],
                                                           stream=stream.value), 'detect')
    for e in ev:
        L.snf_event_destroy(e)
    resident.release()
    return line


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('workloads', nargs='*', help='pa, pc, sb (default: all)')
    parser.add_argument('--repeat', type=int, default=7)
    parser.add_argument('--k', type=int, default=4)
    parser.add_argument('--scratch-bytes', type=int, default=0)
    parser.add_argument('--only', choices=['align', 'sibling'])
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
