"""Timing of the linear-VTLN kernels and of VtlnProcessor.process; prints ONE JSON line.

    python tools/time_vtln.py [--frames 500000] [--minutes 60] [--reps 5]

- fMLLR statistics (snf_fmllr_accumulate, batched as VtlnProcessor batches them) per `--frames` frames at
  D = 39, n = 15, for 200 and for 20 000 segments: host time around the synchronising calls (median of
  `--reps` after one warm-up), FLOP 2 F (D(D+1) + D + 1)(D + 1) and the share of an FP64 matrix peak of
  78.6 TF (the spec-sheet figure);
- class search (snf_lvtln_select) for 1 000 segments x 41 classes, offset norm;
- the 41 mapping-transform Grams (snf_vtln_gram) over `--frames` / 5 frames;
- VtlnProcessor().process at its defaults on about `--minutes` minutes of synthetic audio, stage split;
- a numpy float64 CPU STAND-IN for the reference's per-frame statistics loop (no pykaldi here), timed on
  2 000 frames and scaled.

Run under `timeout -k 10 <s>`; profile in a separate run (rocprofv3 --kernel-trace --stats -- python ...).
"""

import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

from shennong_amd import _backend, gmm as G, lvtln as LV, synth  # noqa: E402

PEAK64 = 78.6e12


def timed(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=500000)
    ap.add_argument('--minutes', type=float, default=60.0)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    out = {'device': _backend.device_name(0)}
    rng = np.random.RandomState(0)
    D, n, Cg, F = 39, 15, 64, args.frames
    gmm = G.DiagGmm(Cg, D)
    gmm.weights_[:] = 1.0 / Cg
    gmm.inv_vars_ = rng.uniform(0.5, 2, (Cg, D)).astype(np.float32)
    gmm.means_invvars_ = (rng.randn(Cg, D) * gmm.inv_vars_).astype(np.float32)
    gmm.compute_gconsts()
    x = rng.randn(F, D).astype(np.float32)
    sel = np.stack([rng.permutation(Cg)[:n] for _ in range(1000)])[rng.randint(0, 1000, F)].astype(np.int32)
    post = rng.dirichlet(np.ones(n), size=1000).astype(np.float32)[rng.randint(0, 1000, F)]
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    dsel = block.upload_selection(sel)
    dpost = _backend.upload_rows([post], np.float32)
    flop = 2.0 * F * (D * (D + 1) + D + 1) * (D + 1)
    per = LV.segments_per_call(D)
    for S in (200, 20000):
        offsets = np.linspace(0, F, S + 1).astype(np.int64)

        def run():
            for first in range(0, S, per):
                LV.fmllr_accumulate(block, dg, dsel, dpost, n, offsets, first, min(S, first + per))
        ms = timed(run, args.reps)
        out[f'fmllr_stats_ms_{S}_segments'] = round(ms, 3)
        out[f'fmllr_stats_fp64_peak_share_{S}_segments'] = round(flop / (ms * 1e-3) / PEAK64, 4)
    out['fmllr_stats_gflop'] = round(flop / 1e9, 2)
    out['fmllr_stats_frames'] = F
    # class search: 1 000 segments x 41 classes
    lv = LV.LinearVtln(D, 41, 15)
    for c in range(41):
        lv.set_transform(c, np.eye(D) + 0.01 * rng.randn(D, D))
    dl = LV.DeviceLvtln(lv)
    offsets = np.linspace(0, F, 1001).astype(np.int64)
    stats = LV.fmllr_accumulate(block, dg, dsel, dpost, n, offsets, 0, 1000)
    out['class_search_ms_1000x41'] = round(timed(lambda: dl.select(stats, 1000, 'offset', 0.0), args.reps), 3)
    # mapping transforms: 41 Grams over F / 5 frames
    Fm = F // 5
    dx = _backend.upload_rows([x[:Fm]], np.float32)
    dy = _backend.upload_rows([x[Fm:2 * Fm]], np.float32)
    out['mapping_grams_ms_41'] = round(timed(lambda: [LV.vtln_gram(dx, dy, Fm, D) for _ in range(41)], 2), 3)
    # CPU stand-in: float64 numpy per-frame loop of the reference (scaled from 2 000 frames)
    import lvtln_f64 as R
    t0 = time.perf_counter()
    R.fmllr_stats_loop(x[:2000].astype(np.float64), sel[:2000], post[:2000], gmm.means_invvars_, gmm.inv_vars_)
    out['cpu_standin_stats_loop_ms_scaled'] = round(1e3 * (time.perf_counter() - t0) * F / 2000, 1)
    # VtlnProcessor().process on synthetic audio
    if args.minutes > 0:
        import scipy.io.wavfile
        import tempfile
        from shennong_amd import Utterances
        from shennong_amd.processor.vtln import VtlnProcessor
        tmp = tempfile.mkdtemp()
        nutt = max(4, int(args.minutes * 60 / 4))
        waves = synth.ragged_utterances(0, nutt, min_s=2.0, max_s=6.0)
        rows = []
        for i, w in enumerate(waves):
            path = os.path.join(tmp, f'u{i}.wav')
            scipy.io.wavfile.write(path, 16000, w)
            rows.append((f'u{i}', path, f'spk{i % max(1, nutt // 10)}'))
        utts = Utterances(rows)
        stages = {}
        proc = VtlnProcessor()
        for name in ('_estimate_device', '_mapping_from_device'):
            orig = getattr(proc, name)

            def wrap(*a, _orig=orig, _name=name, **k):
                t = time.perf_counter()
                r = _orig(*a, **k)
                stages[_name] = stages.get(_name, 0.0) + time.perf_counter() - t
                return r
            setattr(proc, name, wrap)
        t0 = time.perf_counter()
        proc.process(utts)
        total = time.perf_counter() - t0
        out['process_audio_hours'] = round(sum(len(w) for w in waves) / 16000 / 3600, 3)
        out['process_s'] = round(total, 2)
        out['process_stage_s'] = {k: round(v, 2) for k, v in stages.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
