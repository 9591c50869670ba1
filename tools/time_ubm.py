"""Timing of the diagonal-GMM kernels and of DiagUbmProcessor.process; prints ONE JSON line.

    python tools/time_ubm.py [--frames 500000] [--hours 10] [--reps 20]

- E-step (snf_gmm_accumulate) per `--frames` frames at D = 39, C in {64, 512, 2048}: device-event time of
  the three launches (after 3 warm-up calls, median of `--reps`), FLOP/s from 2 F C 2D + 2 F C (2D + 1)
  (the useful work: the kernel recomputes L once more in its statistics pass) and the share of the
  155 TF FP32 matrix peak;
- gselect (snf_gmm_gselect) at C = 2048, n = 15;
- DiagUbmProcessor(64).process on a synthetic corpus of about `--hours` hours (synth.ragged_utterances),
  defaults, with a stage breakdown;
- a CPU STAND-IN for the reference's per-frame Kaldi E-step (no Kaldi / pykaldi here): the same E-step
  as float32 numpy on 16 threads, at the same sizes (one call, `--cpu-frames` frames, scaled).

Run under `timeout -k 10 <s>`; profile in a separate run (rocprofv3 --kernel-trace --stats -- python ...).
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from shennong_amd import _backend, gmm as G, synth  # noqa: E402

PEAK = 155e12


def event_ms(fn, stream, reps):
    L = _backend.lib()
    a, b = C.c_void_p(), C.c_void_p()
    _backend.check(L.snf_event_create(C.byref(a)))
    _backend.check(L.snf_event_create(C.byref(b)))
    times = []
    for _ in range(reps):
        _backend.check(L.snf_event_record(a, stream))
        fn()
        _backend.check(L.snf_event_record(b, stream))
        _backend.check(L.snf_event_synchronize(b))
        ms = C.c_float()
        _backend.check(L.snf_event_elapsed_ms(a, b, C.byref(ms)))
        times.append(ms.value)
    L.snf_event_destroy(a)
    L.snf_event_destroy(b)
    return float(np.median(times))


def model(C_, D, rng):
    gmm = G.DiagGmm(C_, D)
    gmm.weights_[:] = 1.0 / C_
    gmm.inv_vars_ = rng.uniform(0.5, 2, (C_, D)).astype(np.float32)
    gmm.means_invvars_ = (rng.randn(C_, D) * gmm.inv_vars_).astype(np.float32)
    gmm.compute_gconsts()
    return gmm


def estep_numpy(x, gc, mi, iv):
    L = gc[None, :] + x @ mi.T - 0.5 * (x * x) @ iv.T
    m = L.max(axis=1, keepdims=True)
    P = np.exp(L - m)
    s = P.sum(axis=1, keepdims=True)
    P /= s
    return P.sum(axis=0), P.T @ x, P.T @ (x * x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=500000)
    ap.add_argument('--hours', type=float, default=10.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cpu-frames', type=int, default=50000)
    ap.add_argument('--skip-process', action='store_true')
    args = ap.parse_args()
    D, F = 39, args.frames
    rng = np.random.RandomState(0)
    x = rng.randn(F, D).astype(np.float32)
    block = G.FrameBlock([x])
    L = _backend.lib()
    stream = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(stream)))
    out = {'tool': 'time_ubm', 'device': _backend.device_name(0), 'frames': F, 'dim': D, 'estep': {}}
    stats = _backend.DeviceBuffer(8 * (2048 * (2 * D + 1) + 1))
    for C_ in (64, 512, 2048):
        dg = G.DeviceGmm(model(C_, D, rng))
        n = C_ * (2 * D + 1)

        def call():
            _backend.check(L.snf_gmm_accumulate(0, C.c_void_p(block.frames.ptr), F, D, None, *dg.args(),
                                                C.c_void_p(stats.ptr), C.c_void_p(stats.ptr + 8 * n), None,
                                                stream))
        for _ in range(3):
            call()
        ms = event_ms(call, stream, args.reps)
        flop = 2.0 * F * C_ * 2 * D + 2.0 * F * C_ * (2 * D + 1)
        cpu_x = x[:args.cpu_frames]
        g = dg
        gm = model(C_, D, np.random.RandomState(1))
        t0 = time.perf_counter()
        estep_numpy(cpu_x, gm.gconsts_, gm.means_invvars_, gm.inv_vars_)
        cpu_s = (time.perf_counter() - t0) * F / cpu_x.shape[0]
        out['estep'][str(C_)] = {'ms': round(ms, 4), 'tflops': round(flop / ms / 1e9, 2),
                                 'share_of_155tf': round(flop / ms / 1e9 / (PEAK / 1e12), 4),
                                 'cpu_standin_numpy_f32_16thr_ms': round(cpu_s * 1e3, 1)}
        del g
    dg = G.DeviceGmm(model(2048, D, rng))
    idx = _backend.DeviceBuffer(4 * F * 15)

    def gsel():
        _backend.check(L.snf_gmm_gselect(0, C.c_void_p(block.frames.ptr), F, D, *dg.args(), 15,
                                         C.c_void_p(idx.ptr), None, stream))
    gsel()
    out['gselect_2048_n15_ms'] = round(event_ms(gsel, stream, max(3, args.reps // 4)), 3)

    if not args.skip_process:
        from shennong_amd import Audio, Utterances
        from shennong_amd.processor.ubm import DiagUbmProcessor
        count = int(args.hours * 3600 / 3.5)
        waves = synth.ragged_utterances(0, count, min_s=1.0, max_s=6.0)
        utts = Utterances([(f'u{i}', Audio(w, 16000)) for i, w in enumerate(waves)])
        ubm = DiagUbmProcessor(64)
        stages = {}
        t = time.perf_counter()
        feats = ubm._prepare(utts, 1)
        stages['extract_vad_cmvn_trim_s'] = time.perf_counter() - t
        t = time.perf_counter()
        ubm.initialize_gmm(feats)
        stages['init_s (frame selection + upload + init iterations)'] = time.perf_counter() - t
        from shennong_amd.features import FeaturesCollection
        sub = FeaturesCollection({u: f.copy(subsample=ubm.subsample) for u, f in feats.items()})
        t = time.perf_counter()
        block2 = G.FrameBlock([f.data for f in sub.values()])
        stages['upload_main_s'] = time.perf_counter() - t
        t = time.perf_counter()
        for _ in range(ubm.num_iters):
            accs, _ = ubm._em_step(block2)
            ubm.estimate(accs)
        stages['main_iterations_s'] = time.perf_counter() - t
        out['process_64'] = {'hours': round(sum(len(w) for w in waves) / 16000 / 3600, 2),
                             'frames_after_vad': int(sum(f.nframes for f in feats.values())),
                             **{k: round(v, 3) for k, v in stages.items()}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
