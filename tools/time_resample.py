#!/usr/bin/env python
"""Times the device resampler on one MI355X, one case per process, one JSON line per case.

    python tools/time_resample.py kernel --rates 16000 8000 [--utts 10000] [--seconds 3] [--repeat 7] [--out FILE]
    python tools/time_resample.py bottleneck [--utts 1000] [--seconds 3] [--hidden 1500] [--rounds 3] [--out FILE]

`kernel`: ``snf_linear_resample`` (int16) on `--utts` utterances of `--seconds` that are on the device, per call
between two events on the call's stream (the kernel and the copy of its table of 32 bytes per utterance), and
host to host; the share of that time that the bytes moved - 2 in and 2 out per sample - would take at the
6.29 TB/s a copy kernel reaches on this chip; beside it the pitch tracker's ``pitch_resample_kernel`` on the same
block in the same process, at the same rates, cutoff and width: a pitch plan stopped after its first two
launches (SNF_PITCH_TRACE=1), so its figure holds the upload of the tracker's tables and ``pitch_stats_kernel``
too.  The two kernels alone: the same command under ``rocprofv3 --kernel-trace --stats``, in a run of its own.

`bottleneck`: ``BottleneckProcessor.process_all`` on `--utts` utterances of 16 kHz audio (shennong_amd.synth,
synthetic weights of tests/bottleneck_f64.py), `resample` 'scipy' and 'kaldi' alternated `--rounds` times in one
process after a warm-up of each; the medians, and the resampler's own call on the same audio.

`--out` appends the line to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

COPY_RATE = 6.29e12   # bytes per second of a float4 copy kernel on an MI355X (8 TB/s by the data sheet)


def taps_per_output(rate_in, rate_out):
    """Average filter length over the phases (the table of host_tables.cpp make_linear_resample)"""
    base = np.gcd(rate_in, rate_out)
    half = 6 / (2.0 * float(np.float32(0.99 * 0.5 * min(rate_in, rate_out))))
    taps = []
    for i in range(rate_out // base):
        t = i / float(rate_out)
        taps.append(int(np.floor((t + half) * rate_in)) - int(np.ceil((t - half) * rate_in)) + 1)
    return float(np.mean(taps))


def event_timed(fn, stream, repeat):
    """Milliseconds between two events around every call of `fn` (which waits for `stream`), and host to host"""
    from shennong_amd import _backend
    L = _backend.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _backend.check(L.snf_event_create(C.byref(e)))
    device, host = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        _backend.check(L.snf_event_record(ev[0], stream))
        fn()
        _backend.check(L.snf_event_record(ev[1], stream))
        _backend.check(L.snf_event_synchronize(ev[1]))
        host.append(1e3 * (time.perf_counter() - t0))
        ms = C.c_float()
        _backend.check(L.snf_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        device.append(ms.value)
    for e in ev:
        L.snf_event_destroy(e)
    return device, host


def tracker_resampler(args, block, soff, length):
    """Milliseconds of a pitch plan stopped after ``pitch_resample_kernel`` and ``pitch_stats_kernel`` on the
    same block: the same rates, cutoff and width"""
    from shennong_amd import _abi, _backend
    rate_in, rate_out = args.rates
    n = args.utts
    po = _abi.default_pitch_options()
    po.samp_freq, po.resample_freq = float(rate_in), float(rate_out)
    po.lowpass_cutoff = float(np.float32(0.99 * 0.5 * min(rate_in, rate_out)))
    po.lowpass_filter_width = 6
    opts = _abi.default_options(_abi.KIND_PITCH)
    opts.pitch = po
    plan = _backend.Plan(opts)
    frames = plan.num_frames(length)
    foff = np.arange(n + 1, dtype=np.int64) * frames
    out = _backend.DeviceBuffer(max(16, 4 * n * frames * plan.ndims))
    stderr = os.dup(2)   # (the trace knob prints a line per call)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 2)
    pitch = []
    try:
        for k in range(3 + args.repeat):
            plan.run_device(block.ptr, soff, foff, out.ptr)
            if k >= 3:
                pitch.append(plan.last_kernel_ms(0))
    finally:
        os.dup2(stderr, 2)
        os.close(null)
        os.close(stderr)
    return pitch


def kernel_case(args):
    os.environ['SNF_PITCH_TRACE'] = '1'   # (read once, when the tracker first runs: stop after resample + stats)
    from shennong_amd import _backend
    rate_in, rate_out = args.rates
    n, length = args.utts, int(args.seconds * rate_in)
    rng = np.random.default_rng(7)
    waves = rng.integers(-20000, 20000, size=(n, length), dtype=np.int16)
    block = _backend.DeviceBuffer(waves.nbytes)
    block.upload(waves)
    soff = np.arange(n + 1, dtype=np.int64) * length
    n_out = _backend.resample_num_out(rate_in, rate_out, length)
    dst = _backend.DeviceBuffer(2 * n * n_out)
    starts = np.arange(n, dtype=np.int64) * n_out
    L = _backend.lib()
    handle = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(handle)))
    pi64 = C.POINTER(C.c_int64)

    def ours():
        _backend.check(L.snf_linear_resample(
            _backend.get_device(), rate_in, rate_out, 0, C.c_void_p(block.ptr), soff.ctypes.data_as(pi64), n,
            C.c_void_p(dst.ptr), starts.ctypes.data_as(pi64), handle))

    for _ in range(3):
        ours()
    device, host = event_timed(ours, handle, args.repeat)
    check = dst.download(np.empty(n * n_out, dtype=np.int16))

    pitch, pitch_error = [], None
    try:
        pitch = tracker_resampler(args, block, soff, length)
    except (RuntimeError, ValueError) as err:   # (a rate pair the tracker's plan refuses: reported, not hidden)
        pitch_error = str(err)
    taps = taps_per_output(rate_in, rate_out)
    work = n * n_out * taps
    moved = 2.0 * n * (length + n_out)
    ms = float(np.median(device))
    return {
        'case': 'kernel', 'rate_in': rate_in, 'rate_out': rate_out, 'utts': n, 'seconds_each': args.seconds,
        'device': _backend.device_name(), 'samples_in': n * length, 'samples_out': n * n_out,
        'taps_per_output': taps, 'linear_resample_event_ms': sorted(device), 'linear_resample_ms': ms,
        'linear_resample_host_ms': float(np.median(host)), 'bytes_moved': moved,
        'copy_time_ms_at_6.29TBps': 1e3 * moved / COPY_RATE, 'fraction_of_copy_time': 1e3 * moved / COPY_RATE / ms,
        'linear_resample_ps_per_output_tap': 1e9 * ms / work,
        'pitch_resample_and_stats_ms': sorted(pitch),
        'pitch_resample_and_stats_median_ms': float(np.median(pitch)) if pitch else None,
        'pitch_ps_per_output_tap_upper_bound': 1e9 * float(np.median(pitch)) / work if pitch else None,
        'pitch_plan_error': pitch_error,
        'checksum': int(check.astype(np.int64).sum())}


def bottleneck_case(args):
    import bottleneck_f64 as f64
    from shennong_amd import Audio, Utterances, _backend, synth
    from shennong_amd.processor import bottleneck
    tmp = tempfile.mkdtemp(prefix='bottleneck_weights_')
    os.environ[bottleneck.ENV_DIR] = tmp
    np.savez(os.path.join(tmp, bottleneck._FILES['BabelMulti'] + '.npz'), **f64.make_weights(1, args.hidden, 5))
    proc = bottleneck.BottleneckProcessor(dither=0.0)
    length = int(args.seconds * 16000)
    waves = synth.utterances(0, args.utts, length)
    utts = Utterances([('u%05d' % i, Audio(w, 16000, validate=False)) for i, w in enumerate(waves)])
    times = {'scipy': [], 'kaldi': []}
    for name in times:   # warm-up: code objects, tables, pools
        proc.resample = name
        proc.process_all(utts)
    for _ in range(args.rounds):
        for name in times:
            proc.resample = name
            t0 = time.perf_counter()
            proc.process_all(utts)
            times[name].append(1e3 * (time.perf_counter() - t0))
    # the resampler's share: its call alone on the batch, on the device
    block = _backend.upload_rows(list(waves), np.int16)
    soff = np.arange(args.utts + 1, dtype=np.int64) * length
    alone = []
    for k in range(2 + args.rounds):
        t0 = time.perf_counter()
        _backend.resample_device(block, soff, 16000, 8000, 0)
        if k >= 2:
            alone.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    for w in waves[:50]:
        Audio(w, 16000, validate=False).resample(8000)
    host_loop = 1e3 * (time.perf_counter() - t0) / 50 * args.utts
    scipy_ms, kaldi_ms = float(np.median(times['scipy'])), float(np.median(times['kaldi']))
    return {
        'case': 'bottleneck', 'utts': args.utts, 'seconds_each': args.seconds, 'hidden': args.hidden,
        'device': _backend.device_name(), 'process_all_scipy_ms': times['scipy'], 'process_all_kaldi_ms': times['kaldi'],
        'process_all_scipy_median_ms': scipy_ms, 'process_all_kaldi_median_ms': kaldi_ms,
        'speedup': scipy_ms / kaldi_ms, 'resample_device_call_ms': alone,
        'resampler_share_of_kaldi_call': float(np.median(alone)) / kaldi_ms,
        'host_resample_loop_ms_extrapolated_from_50': host_loop}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('case', choices=['kernel', 'bottleneck'])
    ap.add_argument('--rates', type=int, nargs=2, default=[16000, 8000])
    ap.add_argument('--utts', type=int, default=None)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--hidden', type=int, default=1500)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.utts is None:
        args.utts = 10000 if args.case == 'kernel' else 1000
    line = json.dumps(kernel_case(args) if args.case == 'kernel' else bottleneck_case(args))
    print(line, flush=True)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
