#!/usr/bin/env python
"""Times the bottleneck extractor on one MI355X: per-stage device times (events around each C ABI call on
device-resident audio), the whole ``process_all`` host to host, the achieved TFLOP/s of the square layer
(``snf_dense_layer`` / ``snf_dense_layer_bf16`` alone, best of `--repeat`) and of the whole forward pass
against the matrix peak of the precision (157.3 TF FP32, 2516.6 TF BF16), and the ratio to the float64 numpy
statement (tests/bottleneck_f64.py) on the host's CPUs.

    python tools/time_bottleneck.py --utts 1000 --hidden 500 1500 [--precision float32 bfloat16] [--seconds 3]
                                    [--out FILE] [--pipeline]

Prints one JSON line per configuration and precision; the precisions of one configuration are timed in one
process on the same inputs (random operands), each after its own warm-up.  Synthetic weights
(tests/bottleneck_f64.py make_weights).

`--pipeline` replaces all of that by the pipeline leg: ``pipeline.extract_features`` with the bare bottleneck entry
(one ``snf_bottleneck_extract`` call, dither 0) on the corpus at 8 kHz and again at 16 kHz (resampled on the device),
and ``BottleneckProcessor.process_all`` on the same input in the same process (at 16 kHz with ``resample =
'kaldi'``, the pipeline's resampler), each after its own warm-up, best and spread of `--repeat`; beside each the
HBM the process holds at its peak (total minus the least free memory a sampling thread saw every millisecond; the
device pool is emptied before each leg, the pipeline leg runs first)."""
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
import bottleneck_f64 as f64  # noqa: E402

PEAK_TF = {'float32': 157.3, 'bfloat16': 2516.6}   # 256 CUs x 4 SIMDs x 2.4 GHz x 64 (FP32) or 1024 (BF16) FLOP/clk


def corpus(n, seconds, seed=0, rate=8000):
    rng = np.random.RandomState(seed)
    length = int(rate * seconds)
    t = np.arange(length) / float(rate)
    base = [np.clip(np.round((np.sin(2 * np.pi * (1.5 + 0.2 * k) * t + k) > -0.3)
                             * (5000 * np.sin(2 * np.pi * (180 + 20 * k) * t) + 700 * rng.randn(length))
                             + 15 * rng.randn(length)), -32768, 32767).astype(np.int16) for k in range(16)]
    return [base[i % 16] for i in range(n)]


def timed(fn, repeat):
    best = float('inf')
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def timed_all(fn, repeat):
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return times


def peak_hbm(fn, backend):
    """HBM in use (total - free, the whole process) at the peak of one call of `fn`"""
    import threading
    backend.DEVICE_POOL.clear()
    free, total = backend.mem_info()
    least, stop = [free], threading.Event()

    def watch():
        while not stop.is_set():
            least[0] = min(least[0], backend.mem_info()[0])
            time.sleep(0.001)
    thread = threading.Thread(target=watch)
    thread.start()
    try:
        fn()
    finally:
        stop.set()
        thread.join()
    return int(total - least[0])


def pipeline_leg(args):
    from shennong_amd import Audio, Utterances, _backend, pipeline
    from shennong_amd.logger import get_logger
    from shennong_amd.processor import bottleneck
    quiet = get_logger('time', 'error')
    lines = []
    for hidden in args.hidden:
        tmp = tempfile.mkdtemp(prefix='bottleneck_weights_')
        os.environ[bottleneck.ENV_DIR] = tmp
        np.savez(os.path.join(tmp, bottleneck._FILES['BabelMulti'] + '.npz'), **f64.make_weights(1, hidden, 5))
        config = {'bottleneck': pipeline.get_bottleneck_config()}
        config['bottleneck']['dither'] = 0.0
        for n in args.utts:
            for rate in (8000, 16000):
                waves = corpus(n, args.seconds, rate=rate)
                utts = Utterances([('u%05d' % i, Audio(w, rate, validate=False)) for i, w in enumerate(waves)])
                proc = bottleneck.BottleneckProcessor(dither=0.0)
                if rate != 8000:
                    proc.resample = 'kaldi'
                legs = (('pipeline', lambda: pipeline.extract_features(config, utts, log=quiet)),
                        ('process_all', lambda: proc.process_all(utts)))
                line = {'hidden': hidden, 'utts': n, 'seconds_each': args.seconds, 'sample_rate': rate,
                        'device': _backend.device_name(), 'repeat': args.repeat}
                for name, fn in legs:
                    line[name + '_peak_hbm_bytes'] = peak_hbm(fn, _backend)   # (also the warm-up)
                    times = timed_all(fn, args.repeat)
                    line[name + '_ms'] = 1e3 * min(times)
                    line[name + '_ms_all'] = [1e3 * t for t in times]
                lines.append(line)
                print(json.dumps(line), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, nargs='+', default=[1000])
    ap.add_argument('--hidden', type=int, nargs='+', default=[500, 1500])
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--precision', nargs='+', default=['float32'], choices=['float32', 'bfloat16'])
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--cpu-utts', type=int, default=8)
    ap.add_argument('--out', default=None)
    ap.add_argument('--pipeline', action='store_true')
    args = ap.parse_args()
    if args.pipeline:
        lines = pipeline_leg(args)
        if args.out:
            with open(args.out, 'w') as fh:
                for line in lines:
                    fh.write(json.dumps(line) + '\n')
        return
    from shennong_amd import Audio, Utterances, _backend
    from shennong_amd.processor import bottleneck
    lines = []
    for hidden in args.hidden:
        weights = f64.make_weights(1, hidden, 5)
        tmp = tempfile.mkdtemp(prefix='bottleneck_weights_')   # (looked up again by every call: kept)
        os.environ[bottleneck.ENV_DIR] = tmp
        np.savez(os.path.join(tmp, bottleneck._FILES['BabelMulti'] + '.npz'), **weights)
        proc = bottleneck.BottleneckProcessor(dither=0.0)
        dnet = proc._device_network(_backend.get_device())
        # the square layer alone: 65 536 rows (calls wait for their stream: host to host = device time + launch)
        rng = np.random.RandomState(2)
        m = 65536
        x = _backend.DeviceBuffer(4 * m * hidden)
        y = _backend.DeviceBuffer(4 * m * hidden)
        x.upload(rng.uniform(0, 1, (m, hidden)).astype(np.float32))
        L = _backend.lib()

        packed = bottleneck.pack_weights(dnet.buffers[2], hidden, hidden, _backend.get_device())

        def square(precision):
            if precision == 'bfloat16':
                _backend.check(L.snf_dense_layer_bf16(_backend.get_device(), C.c_void_p(x.ptr), m, hidden,
                                                      C.c_void_p(packed.ptr), C.c_void_p(dnet.buffers[3].ptr),
                                                      hidden, 1, C.c_void_p(y.ptr), None))
            else:
                _backend.check(L.snf_dense_layer(_backend.get_device(), C.c_void_p(x.ptr), m, hidden,
                                                 C.c_void_p(dnet.buffers[2].ptr), C.c_void_p(dnet.buffers[3].ptr),
                                                 hidden, 1, C.c_void_p(y.ptr), None))
        sq = {}
        for precision in args.precision:
            square(precision)
            sq[precision] = timed(lambda: square(precision), args.repeat)
        for n in args.utts:
            waves = corpus(n, args.seconds)
            batch = bottleneck.BottleneckBatch(waves)
            batch.vad(); batch.fbank(0.0)   # warm-up (scratch, tables)
            t_vad = timed(batch.vad, args.repeat)
            t_fb = timed(lambda: batch.fbank(0.0), args.repeat)
            utts = Utterances([('u%05d' % i, Audio(w, 8000, validate=False)) for i, w in enumerate(waves)])
            k = min(args.cpu_utts, n)
            t0 = time.perf_counter()
            for w in waves[:k]:
                f64.extract(w, weights)
            t_cpu = (time.perf_counter() - t0) / k * n
            for precision in args.precision:
                batch.forward(dnet, precision)
                t_fw = timed(lambda: batch.forward(dnet, precision), args.repeat)
                r0, r1 = int(batch.roff[-1]), int(batch.ooff[-1])
                flop = 2.0 * (r0 * (144 * hidden + hidden * hidden + hidden * 80)
                              + r1 * (400 * hidden + hidden * hidden + hidden * 80))
                proc.precision = precision
                proc.process_all(utts)
                t_all = timed(lambda: proc.process_all(utts), args.repeat)
                tf = 2.0 * m * hidden * hidden / sq[precision] / 1e12
                lines.append({
                    'precision': precision, 'hidden': hidden, 'utts': n, 'seconds_each': args.seconds,
                    'device': _backend.device_name(), 'vad_ms': 1e3 * t_vad, 'fbank_ms': 1e3 * t_fb,
                    'nn_input_forward_download_ms': 1e3 * t_fw, 'process_all_ms': 1e3 * t_all,
                    'forward_flop': flop, 'forward_tflops_incl_input_and_download': flop / t_fw / 1e12,
                    'square_layer_rows': m, 'square_layer_ms': 1e3 * sq[precision],
                    'square_layer_tflops': tf, 'square_layer_fraction_of_peak': tf / PEAK_TF[precision],
                    'numpy_f64_ms_extrapolated_from': k, 'numpy_f64_ms': 1e3 * t_cpu,
                    'speedup_vs_numpy_f64': t_cpu / t_all})
                print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
