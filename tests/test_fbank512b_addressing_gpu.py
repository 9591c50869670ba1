"""The set addressing of fbank512b_kernel: sample offsets relative to the first frame of a frame set.

The 25 ms forms of fbank512b_kernel (kernels_fbank512b.hip, REL) read the first-sample table and the noise keys
of the four frames of a set through a buffer over the rows of that set (scalar base, lane constant 8 q; the
buffer's bound stands in for the clamp of the frame index) and the samples through a buffer that starts at the
first sample of the set's row 0: one 32-bit byte offset per lane and set.  Frame and set indices are 32-bit there.
No product or sum changes, so every output keeps the bits fbank512_kernel gives, and stays inside the suite's
tolerances of the CPU oracle.

The smallest batches at which such addressing can go wrong:

    ragged0 .. ragged3   utterances of 1, 2, 3, 5 and 7 frames mixed with utterances shorter than a window (no
                         frame): sets straddle utterances, a frameless utterance sits inside a set (rows 0 and 1
                         of set 0), and the total is 36 + k frames, k = 0 .. 3: the last set has 4, 1, 2, 3 rows
                         that are frames (the rows behind them lie outside the table buffer)
    one                  a batch of one frame
    sets16, sets16p1     16 * 4 and 16 * 4 + 1 frames: a workgroup has 16 waves, so every wave runs one set and no
                         look-ahead finds a frame / wave 0 runs a second set of one row

over fbank-40, fbank-23 with the energy column, MFCC-13 (default and htk_compat), PLP-13, without and with dither,
for the 25 ms window (NJ = 13: the new addressing) and the 20 ms window (NJ = 16: 64-bit addresses per lane, as
before).  The same frame counts come out for both windows (400 + 160 (n - 1) samples hold n frames of either).

Each kernel runs in a child process of its own, where the launcher's knob SNF_FBANK512_OLD=1 selects
fbank512_kernel; LDS and the pooled device buffers start full of NaN bit patterns; every element of every row is
compared on its raw bits.

The route's decision between the two addressings is a host function of the offset tables
(fbank512b_rel32_ok through the test aid snf_debug_fbank512b_rel32); its tests need no device and no audio.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    'fbank40': ('fbank', dict(num_bins=40)),
    'fbank23_energy': ('fbank', dict(num_bins=23, use_energy=True)),
    'mfcc13': ('mfcc', dict()),
    'mfcc13_htk': ('mfcc', dict(htk_compat=True)),
    'plp13': ('plp', dict()),
}
DITHERS = (0.0, 1.0)
WINDOWS = {'25ms': 0.025, '20ms': 0.02}
NOISE_CALL = 13  # the same call id on both kernels: the same dither stream

RAGGED = [1, 0, 2, 3, 5, 0, 7, 2, 0, 1, 3, 5, 7]  # frames per utterance: 36 in all
BATCHES = {
    'ragged0': RAGGED,
    'ragged1': RAGGED + [1],
    'ragged2': RAGGED + [2],
    'ragged3': RAGGED + [0, 3],
    'one': [1],
    'sets16': [64],
    'sets16p1': [65],
}


def _samples(frames):
    return 400 + 160 * (frames - 1) if frames > 0 else 300


def _waves(batch):
    from shennong_amd import synth
    frames = BATCHES[batch]
    seed = 7000 + 100 * sorted(BATCHES).index(batch)
    return [np.ascontiguousarray(synth.utterances(seed + i, 1, nsamples=_samples(n))[0]) for i, n in enumerate(frames)]


def _processor(config, dither, window):
    from shennong_amd.processor import FilterbankProcessor, MfccProcessor, PlpProcessor
    kind, opts = CONFIGS[config]
    cls = {'fbank': FilterbankProcessor, 'mfcc': MfccProcessor, 'plp': PlpProcessor}[kind]
    return cls(dither=dither, frame_length=WINDOWS[window], **opts)


def _key(config, dither, window, batch):
    return '%s_d%d_%s_%s' % (config, int(dither), window, batch)


def _child(path):
    """Runs every case on whichever kernel the environment selects and writes the rows to `path`"""
    sys.path.insert(0, ROOT)
    from shennong_amd import _backend
    # (as the suite's `gpu` fixture does: LDS and pooled device buffers start full of NaN bit patterns)
    _backend.check(_backend.lib().snf_debug_fill_lds(0xFFFFFFFF))
    _backend.DEVICE_POOL.poison = True
    result = {}
    for batch in BATCHES:
        waves = _waves(batch)
        soff = np.zeros(len(waves) + 1, dtype=np.int64)
        np.cumsum([w.shape[0] for w in waves], out=soff[1:])
        d_wave = _backend.upload_rows(waves, np.int16)
        for config in CONFIGS:
            for dither in DITHERS:
                for window in WINDOWS:
                    plan = _backend.Plan(_processor(config, dither, window)._build_options())
                    foff = np.zeros(len(waves) + 1, dtype=np.int64)
                    np.cumsum([plan.num_frames(w.shape[0]) for w in waves], out=foff[1:])
                    d_out = _backend.DeviceBuffer(int(foff[-1]) * plan.ndims * 4)
                    plan.run_device(d_wave.ptr, soff, foff, d_out.ptr, noise_call=NOISE_CALL)
                    out = np.empty((int(foff[-1]), plan.ndims), dtype=np.float32)
                    d_out.download(out)
                    names = [plan.kernel_name(i) for i in range(1, 9)]
                    key = _key(config, dither, window, batch)
                    result[key] = out
                    result[key + '_kernels'] = np.array(','.join(n for n in names if n))
                    result[key + '_foff'] = foff
    np.savez(path, **result)


@pytest.fixture(scope='module')
def both(_gpu_backend, tmp_path_factory):
    """{'new': rows of fbank512b_kernel, 'old': rows of fbank512_kernel}, one child process each"""
    where = tmp_path_factory.mktemp('fbank512b_addressing')
    got = {}
    for label, knob in (('new', None), ('old', '1')):
        env = dict(os.environ)
        env.pop('SNF_FBANK512_OLD', None)
        env.pop('SNF_FBANK512B_ADDR64', None)
        if knob is not None:
            env['SNF_FBANK512_OLD'] = knob
        path = str(where / (label + '.npz'))
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path], env=env, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert done.returncode == 0, done.stdout.decode(errors='replace')[-2000:]
        with np.load(path) as z:
            got[label] = {k: z[k] for k in z.files}
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('window', list(WINDOWS))
@pytest.mark.parametrize('dither', DITHERS)
@pytest.mark.parametrize('config', list(CONFIGS))
def test_fbank512b_addressing_matches_fbank512_bit_for_bit(gpu, both, config, dither, window):
    from conftest import assert_close
    from oracle import oracle as orc
    kind = CONFIGS[config][0]
    for batch, frames in BATCHES.items():
        key = _key(config, dither, window, batch)
        new, old = both['new'][key], both['old'][key]
        assert 'fbank512b_kernel' in str(both['new'][key + '_kernels']).split(','), both['new'][key + '_kernels']
        kernels_old = str(both['old'][key + '_kernels']).split(',')
        assert 'fbank512_kernel' in kernels_old and 'fbank512b_kernel' not in kernels_old, kernels_old
        foff = both['new'][key + '_foff']
        # the batch holds what it is meant to hold
        assert np.diff(foff).tolist() == frames and new.shape[0] == sum(frames)
        assert new.shape == old.shape and new.dtype == old.dtype == np.float32
        # every element, on the bits
        diff = new.view(np.uint32) != old.view(np.uint32)
        rows = np.flatnonzero(diff.any(axis=1))
        print('%s: %d of %d values differ bitwise' % (key, int(diff.sum()), diff.size))
        assert not diff.any(), ('%s: %d values differ, first rows %s: %s vs %s' %
                                (key, int(diff.sum()), rows[:4], new[rows[:1]], old[rows[:1]]))
        assert np.isfinite(new).all()
        if dither == 0.0:
            # ... and against the CPU oracle, utterance by utterance, at the suite's tolerances
            options = _processor(config, dither, window)._build_options()
            for u, wave in enumerate(_waves(batch)):
                if frames[u] > 0:
                    assert_close(new[foff[u]:foff[u + 1]], orc.compute(options, wave), rtol=1e-4,
                                 what='%s utterance %d' % (key, u), family=kind)


def test_last_set_row_counts_are_covered():
    totals = {name: sum(frames) for name, frames in BATCHES.items()}
    assert sorted(totals[name] % 4 for name in ('ragged0', 'ragged1', 'ragged2', 'ragged3')) == [0, 1, 2, 3]
    assert totals['one'] == 1 and totals['sets16'] == 16 * 4 and totals['sets16p1'] == 16 * 4 + 1
    for name in ('ragged0', 'ragged1', 'ragged2', 'ragged3'):
        assert set(BATCHES[name]) >= {0, 1, 2, 3, 5, 7}
    assert RAGGED[:3] == [1, 0, 2]  # a frameless utterance between rows 0 and 1 of set 0


# ---- the route guard, on the CPU: offset tables only ----------------------------------------------------------
def _rel32(samples, frames=None):
    """the route's decision for utterances of `samples` samples (frames: 25 ms windows unless given)"""
    from shennong_amd import _backend
    soff = np.zeros(len(samples) + 1, dtype=np.int64)
    np.cumsum(samples, out=soff[1:])
    if frames is None:
        frames = [1 + (n - 400) // 160 if n >= 400 else 0 for n in samples]
    foff = np.zeros(len(samples) + 1, dtype=np.int64)
    np.cumsum(frames, out=foff[1:])
    p64 = ctypes.POINTER(ctypes.c_int64)
    rc = _backend.lib().snf_debug_fbank512b_rel32(soff.ctypes.data_as(p64), foff.ctypes.data_as(p64), len(samples))
    assert rc in (0, 1), rc
    return rc


def test_route_guard_takes_the_new_form_below_2_30_samples_across_three_utterances(monkeypatch):
    monkeypatch.delenv('SNF_FBANK512B_ADDR64', raising=False)
    third = (1 << 30) // 3
    # three utterances that span 2^30 - 1 samples: every frame of a set lies below 2^30 samples from its row 0
    assert _rel32([third, third, (1 << 30) - 1 - 2 * third]) == 1
    # ... and 2^30 samples: the 64-bit form
    assert _rel32([third, third, (1 << 30) - 2 * third]) == 0
    # the same three behind and in front of short utterances
    assert _rel32([16000, third, third, (1 << 30) - 1 - 2 * third, 16000]) == 1
    assert _rel32([16000, third, third, (1 << 30) - 2 * third, 16000]) == 0
    assert _rel32([16000] * 5) == 1 and _rel32([400]) == 1 and _rel32([300]) == 1 and _rel32([]) == 1


def test_route_guard_counts_frameless_utterances_into_the_span(monkeypatch):
    monkeypatch.delenv('SNF_FBANK512B_ADDR64', raising=False)
    third = (1 << 30) // 3
    last = (1 << 30) - 2 * third
    # a frameless utterance between them: the fourth frame of a set lies behind it
    assert _rel32([third, third, 300, last - 301, 16000]) == 1
    assert _rel32([third, third, 300, last - 300, 16000]) == 0
    # frameless utterances alone span nothing: only utterances with frames open and close a span
    assert _rel32([third, third, last - 1] + [300] * 4 + [16000]) == 0
    assert _rel32([third, third, last - 1 - 1200] + [300] * 4 + [16000]) == 1


def test_route_guard_is_about_neighbours_not_about_the_batch(monkeypatch):
    monkeypatch.delenv('SNF_FBANK512B_ADDR64', raising=False)
    # 2^31 samples in utterances of 2^28: any three span 3/4 of 2^30
    assert _rel32([1 << 28] * 8) == 1
    # ... of 2^29: three span 3/2 of 2^30
    assert _rel32([1 << 29] * 4) == 0
    # frame and set indices are 32-bit in the new form: 2^30 frames keep the 64-bit form (tables only)
    assert _rel32([16000, 16000], frames=[(1 << 30) - 2, 1]) == 1
    assert _rel32([16000, 16000], frames=[(1 << 30) - 1, 1]) == 0


def test_route_guard_knob_keeps_the_64_bit_form(monkeypatch):
    monkeypatch.setenv('SNF_FBANK512B_ADDR64', '1')
    assert _rel32([16000] * 5) == 0
    monkeypatch.setenv('SNF_FBANK512B_ADDR64', '0')
    assert _rel32([16000] * 5) == 1


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        _child(sys.argv[2])
