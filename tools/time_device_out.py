#!/usr/bin/env python
"""Times the device-resident results on one MI355X, one case per process, one JSON line per case.

    python tools/time_device_out.py collate [--utts 10000] [--seconds 3] [--repeat 7] [--out FILE]
    python tools/time_device_out.py process_all [--utts 10000] [--seconds 3] [--rounds 5] [--out FILE]
    python tools/time_device_out.py pipeline [--utts 1000] [--seconds 3] [--rounds 5] [--out FILE]

`collate`: ``snf_collate_padded`` on a float32 block of `--utts` x (frames of `--seconds`) x 40 that is in HBM -
the fbank-40 block of the benchmark's corpus by shape; the kernel moves bits, their values do not matter - for
float32 and bfloat16 and (left, right, subsample) = (0, 0, 1) and (1, 1, 3): eight calls back to back between two
events on their stream, per call (the kernel; the copy of a call's table of 16 bytes per utterance goes on another
stream beside the kernel before it), after three warm-up calls.  The kernel alone: the same command under
``rocprofv3 --kernel-trace --stats``, in a run of its own.  The bytes are the ones the rule needs: every input row
the output names, once, and every output byte.  Beside it, in the same process on the same block: ``delta_kernel`` (order 2, window 2: 160 bytes in,
480 out per row of 40), the project's HBM-bound yardstick, from the plan's own event pair after the call that
builds its tile table.  Fractions are of the 8 TB/s of the data sheet.

`process_all`: ``FilterbankProcessor(num_bins=40, dither=0)`` on `--utts` utterances pinned into one page-locked
block: ``process_all`` (unchanged by the device entry point: it is the parent's call) and ``process_all_device``
alternated `--rounds` times after a warm-up of each, wall clock around calls that end complete; the resident
result is released inside the timed window (it waits for the device).

`pipeline`: ``extract_features`` and ``extract_features_device`` with MFCC + Kaldi pitch + CMVN by speaker + delta
on `--utts` in-memory utterances of 100 speakers, alternated the same way.

`--out` appends the line to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes per second, data sheet
INNER = 8   # calls between one pair of events


def event_timed(fn, stream, repeat):
    """Milliseconds per call of `fn` (which enqueues on `stream`): INNER calls back to back between two events, so
    that the host part of a call - the upload of its table - runs beside the kernel of the one before"""
    from shennong_amd import _backend
    L = _backend.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _backend.check(L.snf_event_create(C.byref(e)))
    device = []
    for _ in range(repeat):
        _backend.check(L.snf_event_record(ev[0], stream))
        for _ in range(INNER):
            fn()
        _backend.check(L.snf_event_record(ev[1], stream))
        _backend.check(L.snf_event_synchronize(ev[1]))
        ms = C.c_float()
        _backend.check(L.snf_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        device.append(ms.value / INNER)
    for e in ev:
        L.snf_event_destroy(e)
    return device


def rows_read(frames, left, right, subsample):
    """Distinct input rows of one utterance that the output names"""
    kept = np.arange(0, frames, subsample)
    named = np.clip(kept[:, None] + np.arange(-left, right + 1)[None, :], 0, frames - 1)
    return int(np.unique(named).size)


def collate_case(args):
    from shennong_amd import _abi, _backend
    from shennong_amd.postprocessor import DeltaPostProcessor
    n, dim = args.utts, 40
    fo = _abi.default_frame_options()
    frames = _backend.num_frames(fo, int(args.seconds * 16000))
    rows = n * frames
    rng = np.random.default_rng(11)
    block = _backend.DeviceBuffer(4 * rows * dim)
    host = rng.standard_normal((frames * 100, dim), dtype=np.float32)   # (uploaded in 100-utterance stretches)
    L = _backend.lib()
    for a in range(0, n, 100):
        count = min(100, n - a) * frames * dim * 4
        _backend.check(L.snf_memcpy_h2d(block.ptr + 4 * a * frames * dim, host.ctypes.data, count))
    foff = np.arange(n + 1, dtype=np.int64) * frames
    stream = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(stream)))
    results = []
    for dtype in ('float32', 'bfloat16'):
        for left, right, subsample in ((0, 0, 1), (1, 1, 3)):
            t_max = _backend.collate_num_out(frames, subsample, 0)
            width = dim * (left + 1 + right)
            itemsize = 4 if dtype == 'float32' else 2
            out = _backend.DeviceBuffer(n * t_max * width * itemsize)
            lengths = _backend.DeviceBuffer(4 * n)

            def call():
                _backend.collate_padded(block.ptr, dim, foff, dtype, left, right, subsample, 0, 0.0, t_max, out.ptr,
                                        lengths.ptr, stream=stream.value)
            for _ in range(3):
                call()
            _backend.check(L.snf_stream_synchronize(stream))
            ms = event_timed(call, stream, args.repeat)
            moved = 4.0 * dim * n * rows_read(frames, left, right, subsample) + float(n) * t_max * width * itemsize
            median = float(np.median(ms))
            results.append({'dtype': dtype, 'left': left, 'right': right, 'subsample': subsample,
                            'shape': [n, t_max, width], 'event_ms': sorted(ms), 'ms': median, 'bytes': moved,
                            'bytes_per_s': moved / (1e-3 * median), 'fraction_of_8TBps': moved / (1e-3 * median) / HBM_PEAK})
            out.free()
            lengths.free()
    # the yardstick on the same block: the first call builds the tile table, the following ones are the kernel
    plan = _backend.get_plan(DeltaPostProcessor()._build_options())
    d_delta = _backend.DeviceBuffer(4 * rows * dim * 3)
    delta = []
    for k in range(3 + args.repeat):
        plan.run_post_device(block.ptr, dim, foff, d_delta.ptr)
        if k >= 3:
            delta.append(plan.last_kernel_ms(0))
    delta_bytes = 4.0 * rows * dim * 4
    delta_ms = float(np.median(delta))
    return {'case': 'collate', 'utts': n, 'frames_each': frames, 'dim': dim, 'device': _backend.device_name(),
            'collate': results,
            'delta_kernel': {'name': plan.kernel_name(1), 'event_ms': sorted(delta), 'ms': delta_ms,
                             'bytes': delta_bytes, 'bytes_per_s': delta_bytes / (1e-3 * delta_ms),
                             'fraction_of_8TBps': delta_bytes / (1e-3 * delta_ms) / HBM_PEAK}}


def alternated(calls, rounds):
    """Wall milliseconds of every callable of `calls` (name -> function), alternated `rounds` times after one
    warm-up of each"""
    for fn in calls.values():
        fn()
    walls = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            walls[name].append(1e3 * (time.perf_counter() - t0))
    return walls


def corpus(args, speakers=None):
    from shennong_amd import Audio, Utterances
    rng = np.random.default_rng(5)
    waves = rng.integers(-20000, 20000, size=(args.utts, int(args.seconds * 16000)), dtype=np.int16)
    return Utterances([('u%05d' % i, Audio(w, 16000, validate=False)) + (('s%03d' % (i % speakers),) if speakers else ())
                       for i, w in enumerate(waves)])


def process_all_case(args):
    from shennong_amd import _backend
    from shennong_amd.processor import FilterbankProcessor
    pinned = corpus(args).pin()
    fbank = FilterbankProcessor(num_bins=40, dither=0)
    walls = alternated({'process_all': lambda: fbank.process_all(pinned),
                        'process_all_device': lambda: fbank.process_all_device(pinned).release()}, args.rounds)
    host, resident = (float(np.median(walls[k])) for k in ('process_all', 'process_all_device'))
    return {'case': 'process_all', 'utts': args.utts, 'seconds_each': args.seconds, 'device': _backend.device_name(),
            'audio': 'Utterances.pin(): one page-locked int16 block', 'wall_ms': walls,
            'process_all_median_ms': host, 'process_all_device_median_ms': resident, 'ratio': resident / host,
            'upload_bytes': 2 * args.utts * int(args.seconds * 16000)}


def pipeline_case(args):
    import logging
    from shennong_amd import _backend, pipeline
    utts = corpus(args, speakers=100)
    config = pipeline.get_default_config('mfcc', with_pitch='kaldi', with_cmvn=True, with_delta=True)
    quiet = logging.getLogger('time_device_out')
    quiet.setLevel(logging.ERROR)
    walls = alternated({
        'extract_features': lambda: pipeline.extract_features(config, utts, log=quiet),
        'extract_features_device': lambda: pipeline.extract_features_device(config, utts, log=quiet).release()},
        args.rounds)
    host, resident = (float(np.median(walls[k])) for k in ('extract_features', 'extract_features_device'))
    return {'case': 'pipeline', 'utts': args.utts, 'seconds_each': args.seconds, 'device': _backend.device_name(),
            'configuration': 'mfcc + kaldi pitch + cmvn by speaker (100 speakers) + delta', 'wall_ms': walls,
            'extract_features_median_ms': host, 'extract_features_device_median_ms': resident,
            'ratio': resident / host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('case', choices=['collate', 'process_all', 'pipeline'])
    ap.add_argument('--utts', type=int, default=None)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.utts is None:
        args.utts = 1000 if args.case == 'pipeline' else 10000
    from shennong_amd import _backend
    if _backend.device_count() < 1:
        raise SystemExit('time_device_out needs an MI355X: no HIP device visible')
    line = json.dumps({'collate': collate_case, 'process_all': process_all_case, 'pipeline': pipeline_case}[args.case](args))
    print(line, flush=True)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
