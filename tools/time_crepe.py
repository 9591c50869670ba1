#!/usr/bin/env python
"""Times CrepePitchProcessor on the device: 100 utterances of 3 s at 16 kHz, capacities tiny and full, seeded
synthetic weights (tests/crepe_f64.py).  Host to host, best of 3, every call waits for its stream: the network
alone (snf_crepe_forward, with the achieved TFLOP/s from the layers' arithmetic), the decoders alone
(snf_crepe_decode), and process_all.  The float64 numpy statement is timed on the host's CPUs for a few
utterances and scaled to the batch (--host-utts 0 leaves it out).  One JSON line per capacity and precision
(profiles/crepe_timing.jsonl; profiles/crepe_bf16_timing.jsonl for --precision float32 bfloat16: both in one
process on the same inputs, each after its own warm-up, the later lines with their gain over float32).

With --tail, one line instead (profiles/crepe_tail_timing.jsonl; 1 000 utterances of 3 s there): from the
activation to the post-processed pitch on the host, the host tail (decoder, download, scipy.signal.resample,
predict_voicing, np.interp, pov_to_nccf per utterance, then the Kaldi post-processing kernel: what
CrepePitchProcessor and CrepePitchPostProcessor do) against the device tail (decoder, snf_crepe_rows,
snf_crepe_voicing_convert, the same post-processing kernel, one download), best of 3 in the same process, and
extract_features with the CREPE pitch entry on the same corpus, host to host.

    python tools/time_crepe.py [--utts 100] [--seconds 3] [--capacities tiny,full] [--host-utts 1]
                               [--precision float32 [bfloat16]]
    python tools/time_crepe.py --tail --utts 1000 --capacities tiny
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


def tail_line(args, waves, utterances, capacity):
    """The tail alone, host against device, and the pipeline with the CREPE entry"""
    import scipy.signal
    from shennong_amd import Features, _backend, pipeline
    from shennong_amd.processor import CrepePitchPostProcessor, CrepePitchProcessor, pitch_crepe
    proc = CrepePitchProcessor(model_capacity=capacity)
    post = CrepePitchPostProcessor(delta_pitch_noise_stddev=0)
    model = pitch_crepe.device_model(capacity, _backend.get_device())
    batch = pitch_crepe.CrepeBatch(waves, 160, True)
    batch.forward(model)
    counts = np.asarray([proc._output_rows(len(w)) for w in waves], dtype=np.int64)
    roff = np.concatenate([[0], np.cumsum(counts)])
    qplan = _backend.get_plan(post._build_options())
    pdim = qplan.post_ndims(2)

    def host_tail():
        raw = batch.decode(True)
        feats, properties = [], proc.get_properties()
        for a, b, m in zip(batch.foff[:-1], batch.foff[1:], counts):
            data = scipy.signal.resample(raw[a:b], m)
            data[data[:, 0] < 1e-2, 0] = 0
            data[data[:, 0] > 1, 0] = 1
            feats.append(Features(data, proc.times(m), properties=properties))
        return np.concatenate([f.data for f in post._process_batch(feats)])

    def device_tail():
        batch.decode(True, resident=True)
        batch.rows(counts)
        batch.convert()
        d_pitch = _backend.DeviceBuffer(int(roff[-1]) * pdim * 4)
        qplan.run_post_device(batch.nccf_pitch.ptr, 2, roff, d_pitch.ptr, noise_call=1)
        out = d_pitch.download(np.empty((int(roff[-1]), pdim), dtype=np.float32))
        for block in (d_pitch, batch.resampled, batch.nccf_pitch):
            block.free(synced=True)
        return out

    want, got = host_tail(), device_tail()   # (warm-up, and the two results side by side)
    host = best_of(3, host_tail)
    device = best_of(3, device_tail)
    config = pipeline.get_default_config('mfcc', with_delta=True)
    config['mfcc']['dither'] = 0
    config['pitch'] = pipeline.get_crepe_pitch_config()
    config['pitch']['model_capacity'] = capacity
    config['pitch']['postprocessing']['delta_pitch_noise_stddev'] = 0
    pipeline.extract_features(config, utterances)
    whole = best_of(3, lambda: pipeline.extract_features(config, utterances))
    return {
        'what': 'crepe tail', 'capacity': capacity, 'device': _backend.device_name(), 'utts': args.utts,
        'seconds_each': args.seconds, 'frames': batch.total_frames, 'rows': int(roff[-1]),
        'host_tail_s': round(host, 5), 'device_tail_s': round(device, 5), 'ratio_host_over_device': round(host / device, 1),
        'max_abs_difference': float(np.abs(want.astype(np.float64) - got).max()),
        'extract_features_crepe_s': round(whole, 5), 'host_cpus': len(os.sched_getaffinity(0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=100)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--capacities', default='tiny,full')
    ap.add_argument('--host-utts', type=int, default=1)
    ap.add_argument('--precision', nargs='+', default=['float32'], choices=['float32', 'bfloat16'])
    ap.add_argument('--tail', action='store_true')
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
            if args.tail:
                print(json.dumps(tail_line(args, waves, utterances, capacity)), flush=True)
                continue
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
