#!/usr/bin/env python
"""Times the framed one-hot labels of a corpus: 10 000 synthetic alignments of 3 s, about 30 tokens each over an
inventory of 40, at the defaults (16 kHz, 25 ms frames every 10 ms: 298 frames each).

Appends one line to profiles/onehot_timing.jsonl: the device time of the three kernels (events around them,
``snf_framed_onehot``), ``FramedOneHotProcessor.process_all`` from host to host (tables up, rows down, the
Features built), and the numpy statement of the rule (tests/onehot_np.py) on 20 of the alignments,
extrapolated to the batch, as the CPU counterpart.

    python tools/time_onehot.py [--alignments 10000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))

import onehot_np  # noqa
from shennong_amd import _backend, window  # noqa
from shennong_amd.alignment import Alignment  # noqa
from shennong_amd.processor import FramedOneHotProcessor  # noqa


def corpus(count, seconds=3.0, tokens=30, inventory=40, seed=0):
    rng = np.random.default_rng(seed)
    names = np.array([f'p{i:02d}' for i in range(inventory)])
    out = {}
    for i in range(count):
        cuts = np.sort(rng.uniform(0.0, seconds, tokens - 1))
        edges = rng.uniform(0.0, 0.5) + np.concatenate(([0.0], cuts, [seconds]))
        edges = np.unique(edges)
        times = np.stack((edges[:-1], edges[1:]), axis=1)
        out[f'utt{i:05d}'] = Alignment(times, names[rng.integers(0, inventory, times.shape[0])], validate=False)
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--alignments', type=int, default=10000)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'onehot_timing.jsonl'))
    args = parser.parse_args()
    if _backend.device_count() < 1:
        raise RuntimeError('tools/time_onehot.py needs an MI355X: no HIP device visible')
    alignments = corpus(args.alignments)
    names = sorted({p for a in alignments.values() for p in a.tokens})
    processor = FramedOneHotProcessor(tokens=names)
    batch = list(alignments.values())
    kernel, whole = [], []
    for _ in range(args.repeats + 1):   # (the first pass allocates the scratch and page-locks the result block)
        record = {}
        processor._process_batch(batch, timing=record)
        kernel.append(record['kernel_ms'])
        start = time.perf_counter()
        feats = processor.process_all(alignments)
        whole.append((time.perf_counter() - start) * 1e3)
    frames = sum(f.nframes for f in feats.values())
    # the CPU counterpart: the numpy statement on 20 alignments
    table = window.window(processor.frame.samples_per_frame)
    index = {p: i for i, p in enumerate(names)}
    sample = batch[::max(1, len(batch) // 20)][:20]
    start = time.perf_counter()
    for ali in sample:
        onehot_np.framed_onehot(float(ali.onsets[0]), ali.offsets, [index[p] for p in ali.tokens], len(names),
                                processor.sample_rate, 400, 160, table)
    numpy_ms = (time.perf_counter() - start) * 1e3 / len(sample) * len(batch)
    line = {
        'tool': 'tools/time_onehot.py', 'device': _backend.device_name(), 'alignments': len(batch),
        'tokens_per_alignment': 30, 'inventory': len(names), 'frames': int(frames), 'repeats': args.repeats,
        'kernel_ms_median': float(np.median(kernel[1:])), 'kernel_ms_min': float(np.min(kernel[1:])),
        'process_all_ms_median': float(np.median(whole[1:])), 'process_all_ms_min': float(np.min(whole[1:])),
        'numpy_statement_ms_extrapolated_from_20': float(numpy_ms),
        'dense_bytes': int(frames) * len(names)}
    print(json.dumps(line))
    with open(args.output, 'a') as stream:
        stream.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
