"""Timing of the linear-VTLN kernels and of VtlnProcessor.process; prints ONE JSON line.

    python tools/time_vtln.py [--frames 500000] [--minutes 60] [--reps 5]

- fMLLR statistics (snf_fmllr_accumulate, batched as VtlnProcessor batches them) per `--frames` frames at
  D = 39, n = 15, for 200 and for 20 000 segments: host time around the synchronising calls (median of
  `--reps` after one warm-up), FLOP 2 F (D(D+1) + D + 1)(D + 1) and the share of an FP64 matrix peak of
  78.6 TF (the spec-sheet figure);
- class search (snf_lvtln_select) for 1 000 segments x 41 classes, offset norm;
- the 41 mapping-transform Grams (snf_vtln_gram) over `--frames` / 5 frames;
- VtlnProcessor().process at its defaults on about `--minutes` minutes of synthetic audio, stage split (UBM
  training, unwarped passes, mapping transforms, estimate loop), for the per-class host round trip and for the
  device-resident sweep (`--paths host,device`), with the sweep's RunStats;
- extract_features with a 'vtln' entry (VtlnProcessor defaults, MFCC + CMVN + delta) on the same corpus:
  train / extract split (`--pipeline`);
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
    ap.add_argument('--paths', default='host,device', help='process() runs: host and/or device mapping path')
    ap.add_argument('--pipeline', type=int, default=1, help='also time extract_features with a vtln entry')
    ap.add_argument('--skip-kernels', type=int, default=0)
    args = ap.parse_args()
    out = {'device': _backend.device_name(0)}
    if not args.skip_kernels:
        kernels(args, out)
    if args.minutes > 0:
        process(args, out)
    print(json.dumps(out))


def kernels(args, out):
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
    # the same Grams from a (block, row) list over two blocks
    pick = np.sort(rng.choice(2 * Fm, Fm, replace=False))
    dblock, drow = LV.upload_row_list((pick >= Fm).astype(np.int32), pick % Fm)
    out['mapping_grams_rows_ms_41'] = round(timed(
        lambda: [LV.vtln_gram_rows([dx, dy], [dy, dx], dblock, drow, Fm, D) for _ in range(41)], 2), 3)
    # CPU stand-in: float64 numpy per-frame loop of the reference (scaled from 2 000 frames)
    import lvtln_f64 as R
    t0 = time.perf_counter()
    R.fmllr_stats_loop(x[:2000].astype(np.float64), sel[:2000], post[:2000], gmm.means_invvars_, gmm.inv_vars_)
    out['cpu_standin_stats_loop_ms_scaled'] = round(1e3 * (time.perf_counter() - t0) * F / 2000, 1)


def corpus(minutes):
    import scipy.io.wavfile
    import tempfile
    from shennong_amd import Utterances
    tmp = tempfile.mkdtemp()
    nutt = max(4, int(minutes * 60 / 4))
    waves = synth.ragged_utterances(0, nutt, min_s=2.0, max_s=6.0)
    rows = []
    for i, w in enumerate(waves):
        path = os.path.join(tmp, f'u{i}.wav')
        scipy.io.wavfile.write(path, 16000, w)
        rows.append((f'u{i}', path, f'spk{i % max(1, nutt // 10)}'))
    return Utterances(rows), round(sum(len(w) for w in waves) / 16000 / 3600, 3)


def process(args, out):
    """VtlnProcessor().process on synthetic audio, per mapping path; then extract_features with a vtln entry"""
    from shennong_amd import pipeline
    from shennong_amd.processor import ubm as ubm_module, vtln as vtln_module
    from shennong_amd.processor.vtln import VtlnProcessor
    utts, hours = corpus(args.minutes)
    out['process_audio_hours'] = hours
    out['process_utterances'] = len(utts)
    wrapped = [(ubm_module.DiagUbmProcessor, 'process', 'ubm_training'),
               (VtlnProcessor, '_base_transforms', 'base_transforms'),
               (VtlnProcessor, '_mapping_host', 'mapping'),
               (VtlnProcessor, '_mapping_sweep', 'mapping')]
    stages = {}
    saved = [(owner, name, getattr(owner, name)) for owner, name, _ in wrapped]
    for owner, name, tag in wrapped:
        def wrap(*a, _orig=getattr(owner, name), _tag=tag, **k):
            t = time.perf_counter()
            try:
                return _orig(*a, **k)
            finally:
                stages[_tag] = stages.get(_tag, 0.0) + time.perf_counter() - t
        setattr(owner, name, wrap)
    sweep = vtln_module._sweep_on_device
    try:
        results = {}
        for path in args.paths.split(','):
            vtln_module._sweep_on_device = (lambda u: path == 'device')
            stages.clear()
            proc = VtlnProcessor()
            stats = pipeline.RunStats()
            if path == 'device':   # (the sweep's link bytes: _base_transforms gets the RunStats)
                base = VtlnProcessor._base_transforms
                VtlnProcessor._base_transforms = lambda self, *a, **k: base(self, *a, stats=stats, **k)
            t0 = time.perf_counter()
            try:
                warps = proc.process(utts)
            finally:
                if path == 'device':
                    VtlnProcessor._base_transforms = base
            total = time.perf_counter() - t0
            results[path] = (warps, proc.lvtln)
            split = {
                'ubm_training': stages.get('ubm_training', 0.0),
                'unwarped_passes': stages.get('base_transforms', 0.0) - stages.get('mapping', 0.0),
                'mapping_transforms': stages.get('mapping', 0.0),
                'estimate_loop': total - stages.get('ubm_training', 0.0) - stages.get('base_transforms', 0.0)}
            out[f'process_{path}_s'] = round(total, 2)
            out[f'process_{path}_stage_s'] = {k: round(v, 3) for k, v in split.items()}
            if path == 'device':
                out['process_device_sweep_runstats'] = {k: (round(v, 4) if isinstance(v, float) else v)
                                                        for k, v in stats.as_dict().items()}
        if len(results) == 2:
            (wa, la), (wb, lb) = results['host'], results['device']
            out['process_paths_bit_identical'] = bool(
                wa == wb and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(la.A, lb.A)))
    finally:
        vtln_module._sweep_on_device = sweep
        for owner, name, orig in saved:
            setattr(owner, name, orig)
    if args.pipeline:
        config = pipeline.get_default_config('mfcc', with_cmvn=True, with_delta=True)
        config['vtln'] = VtlnProcessor().get_params()
        train = pipeline._train_vtln
        split = {}

        def timed_train(*a, **k):
            t = time.perf_counter()
            r = train(*a, **k)
            split['train'] = time.perf_counter() - t
            return r
        pipeline._train_vtln = timed_train
        try:
            t0 = time.perf_counter()
            pipeline.extract_features(config, utts)
            total = time.perf_counter() - t0
        finally:
            pipeline._train_vtln = train
        out['extract_features_vtln_s'] = round(total, 2)
        out['extract_features_vtln_split_s'] = {'train': round(split['train'], 2),
                                                'extract': round(total - split['train'], 2)}


if __name__ == '__main__':
    main()
