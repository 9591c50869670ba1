#!/usr/bin/env python
"""Times CrepePitchProcessor on the device: 100 utterances of 3 s at 16 kHz, capacities tiny and full, seeded
synthetic weights (tests/crepe_f64.py).  Host to host, best of 3, every call waits for its stream: the network
alone (snf_crepe_forward, with the achieved TFLOP/s from the layers' arithmetic), the decoders alone
(snf_crepe_decode), and process_all.  The float64 numpy statement is timed on the host's CPUs for a few
utterances and scaled to the batch (--host-utts 0 leaves it out).  One JSON line per capacity and precision
(profiles/crepe_timing.jsonl; profiles/crepe_bf16_timing.jsonl for --precision float32 bfloat16: both in one
process on the same inputs, each after its own warm-up, the later lines with their gain over float32).

    python tools/time_crepe.py [--utts 100] [--seconds 3] [--capacities tiny,full] [--host-utts 1]
                               [--precision float32 [bfloat16]]
"""

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def macs_per_frame(filters):
    """Multiply-adds of one frame: six convolutions (positions x taps x C_in x C_out) and the classifier"""
    total, c_in, positions = 0, 1, 256
    for c, width in zip(filters, (512, 64, 64, 64, 64, 64)):
        total += positions * width * c_in * c
        c_in, positions = c, positions // 2
    return total + 4 * c_in * 360


def best_of(n, call):
    best = float('inf')
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=100)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--capacities', default='tiny,full')
    ap.add_argument('--host-utts', type=int, default=1)
    ap.add_argument('--precision', nargs='+', default=['float32'], choices=['float32', 'bfloat16'])
    args = ap.parse_args()

    import crepe_f64 as f64
    from shennong_amd import Audio, Utterances, _backend
    from shennong_amd.processor import CrepePitchProcessor, pitch_crepe

    if _backend.device_count() < 1:
        raise RuntimeError('tools/time_crepe.py needs an MI355X: no HIP device visible')
    waves = [f64.synthetic_signal(seed=100 + i, seconds=args.seconds, f0=90.0 + 2.0 * i) for i in range(args.utts)]
    utterances = Utterances([('utt%03d' % i, Audio(w, 16000)) for i, w in enumerate(waves)])
    with tempfile.TemporaryDirectory() as directory:
        os.environ[pitch_crepe.ENV_DIR] = directory
        for capacity in args.capacities.split(','):
            weights = f64.make_weights(capacity, 40)
            np.savez(os.path.join(directory, 'model-%s.npz' % capacity),
                     **{k: v.astype(np.float32) for k, v in weights.items()})
            proc = CrepePitchProcessor(model_capacity=capacity)
            model = pitch_crepe.device_model(capacity, _backend.get_device())
            batch = pitch_crepe.CrepeBatch(waves, 160, True)
            flop = 2.0 * macs_per_frame(pitch_crepe.filters(capacity)) * batch.total_frames
            host = None
            if args.host_utts > 0:
                rounded = {k: v.astype(np.float32).astype(np.float64) for k, v in weights.items()}
                t0 = time.perf_counter()
                for w in waves[:args.host_utts]:
                    f64.process(w, rounded)
                host = (time.perf_counter() - t0) * args.utts / args.host_utts
            plain = None
            for precision in args.precision:
                proc.precision = precision
                batch.forward(model, precision)     # warm-up: code objects, scratch, the packed images
                batch.decode(True)
                proc.process_all(utterances)
                forward = best_of(3, lambda: batch.forward(model, precision))
                decode_viterbi = best_of(3, lambda: batch.decode(True))
                decode_plain = best_of(3, lambda: batch.decode(False))
                whole = best_of(3, lambda: proc.process_all(utterances))
                line = {
                    'what': 'crepe', 'capacity': capacity, 'precision': precision, 'device': _backend.device_name(),
                    'utts': args.utts, 'seconds_each': args.seconds, 'frames': batch.total_frames,
                    'gmac_per_frame': round(macs_per_frame(pitch_crepe.filters(capacity)) / 1e9, 4),
                    'forward_s': round(forward, 5), 'forward_tflops': round(flop / forward / 1e12, 2),
                    'decode_viterbi_s': round(decode_viterbi, 5), 'decode_argmax_s': round(decode_plain, 5),
                    'process_all_s': round(whole, 5)}
                if precision == 'float32':
                    plain = (forward, whole)
                elif plain is not None:
                    line['forward_gain_over_float32'] = round(plain[0] / forward, 3)
                    line['process_all_gain_over_float32'] = round(plain[1] / whole, 3)
                if host is not None:
                    line.update({'host_f64_numpy_s_scaled': round(host, 2), 'host_utts_timed': args.host_utts,
                                 'host_cpus': len(os.sched_getaffinity(0)),
                                 'ratio_host_over_process_all': round(host / whole, 1)})
                print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
