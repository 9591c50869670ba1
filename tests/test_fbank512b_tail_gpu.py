"""fbank512b_kernel against fbank512_kernel, bit for bit, over every path of its mel phase and MFCC tail.

The set loop of fbank512b_kernel reads the operands of the mel chain ahead of the chain (the weights in front of the
power-tile writes, the tile operands in one batch behind them) where the bank plan is a template parameter of the
launch, and the DCT rows of the MFCC tail ahead of the log-mel write (kernels_fbank512b.hip: launch_plan, MMQ / LV).
No product or sum changes: every output must keep the bits fbank512_kernel gives.

The bank plan of a configuration - chain length in quads, most blocks per split group, DCT groups - comes from the host
table builder (fast512_build), printed on the CPU for 16 kHz, 25 ms (the 30 ms window gives the same plans):

    case               bins  low-high Hz  mm_quads  mm_levels  dd_groups  launch (MMQ, LV)
    fbank40             40    20-8000        7         3          -        7, 3   the benchmark's form
    fbank23             23    20-8000        6         4          -        6, 4   rows stored element-wise
    fbank24             24    20-8000        7         4          -        7, 4
    fbank48             48    20-8000        8         2          -        0, 0   even generic chain
    fbank45             45    20-8000        9         2          -        0, 0   odd generic chain
    fbank16             16    20-8000        9         4          -        0, 0   odd chain, four blocks
    fbank64_2k          64    20-2000        4         1          -        0, 0   no group is split
    fbank57_4k          57    20-4000        6         2          -        0, 0   six quads tested per set
    fbank40_lin         40    20-8000        7         3          -        7, 3   use_log_fbank=False
    fbank40_energy      40    20-8000        7         3          -        7, 3   energy column, element-wise rows
    mfcc23              23    20-8000        6         4          6        6, 4   the benchmark's MFCC-13 (use_energy)
    mfcc23_noenergy     23    20-8000        6         4          6        6, 4
    mfcc23_htk          23    20-8000        6         4          6        6, 4   htk_compat, energy last
    mfcc23_htk_c0       23    20-8000        6         4          6        6, 4   htk_compat, C0 scaled by sqrt 2
    mfcc23_ceps8 / 16   23    20-8000        6         4          6        6, 4   num_ceps 8 / 16
    mfcc40              40    20-8000        7         3         10        7, 3   DCT loop
    mfcc24              24    20-8000        7         4          6        7, 4   (0, 0 with dither: no registers)
    mfcc13              13    20-8000        9         4          4        0, 0   DCT loop
    fbank40_30ms        40    20-8000        7         3          -        0, 0   NJ = 16 keeps the per-set tests
    mfcc23_30ms         23    20-8000        6         4          6        0, 0   NJ = 16

Every case runs without dither and with the reference's default dither.  The dither forms are instantiations of
their own; those with element-wise row stores (fbank23, fbank40_energy) and mfcc24 launch (0, 0) with dither, for
want of registers.  The batch is the kind
test_fbank512b_pruned_gpu.py uses: ragged speech-like utterances whose sets straddle utterance boundaries, a
one-frame and a two-frame utterance (sets with idle rows), a constant signal and digital silence (exact zeros: the
floors of the logarithms), a total frame count that is no multiple of 4.

Each kernel runs in a child process of its own, where the launcher's knob SNF_FBANK512_OLD=1 selects
fbank512_kernel; LDS and the pooled device buffers start full of NaN bit patterns; every element of every row is
compared on its raw bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    'fbank40': ('fbank', dict(num_bins=40)),
    'fbank23': ('fbank', dict(num_bins=23)),
    'fbank24': ('fbank', dict(num_bins=24)),
    'fbank48': ('fbank', dict(num_bins=48)),
    'fbank45': ('fbank', dict(num_bins=45)),
    'fbank16': ('fbank', dict(num_bins=16)),
    'fbank64_2k': ('fbank', dict(num_bins=64, high_freq=2000)),
    'fbank57_4k': ('fbank', dict(num_bins=57, high_freq=4000)),
    'fbank40_lin': ('fbank', dict(num_bins=40, use_log_fbank=False)),
    'fbank40_energy': ('fbank', dict(num_bins=40, use_energy=True)),
    'mfcc23': ('mfcc', dict(num_bins=23, use_energy=True)),
    'mfcc23_noenergy': ('mfcc', dict(num_bins=23, use_energy=False)),
    'mfcc23_htk': ('mfcc', dict(num_bins=23, use_energy=True, htk_compat=True)),
    'mfcc23_htk_c0': ('mfcc', dict(num_bins=23, use_energy=False, htk_compat=True)),
    'mfcc23_ceps8': ('mfcc', dict(num_bins=23, num_ceps=8)),
    'mfcc23_ceps16': ('mfcc', dict(num_bins=23, num_ceps=16)),
    'mfcc40': ('mfcc', dict(num_bins=40)),
    'mfcc24': ('mfcc', dict(num_bins=24)),
    'mfcc13': ('mfcc', dict(num_bins=13)),
    'fbank40_30ms': ('fbank', dict(num_bins=40, frame_length=0.03)),
    'mfcc23_30ms': ('mfcc', dict(num_bins=23, frame_length=0.03)),
}
DITHERS = (0.0, 1.0)
NOISE_CALL = 11  # the same call id on both kernels: the same dither stream


def _batch():
    from shennong_amd import synth
    waves = [np.ascontiguousarray(w) for w in synth.ragged_utterances(4099, 10, min_s=0.05, max_s=0.4)]
    speech = synth.utterances(91, 1, nsamples=1200)[0]
    waves.insert(1, np.ascontiguousarray(speech[:400]))   # one frame of 25 ms (none of 30 ms)
    waves.insert(3, np.ascontiguousarray(speech[:560]))   # two frames of 25 ms
    waves.insert(4, np.full(2000, 1234, dtype=np.int16))  # constant: exact zeros behind the DC removal
    waves.insert(6, np.zeros(1777, dtype=np.int16))       # digital silence
    waves.insert(8, np.ascontiguousarray(speech[:720]))   # three / two frames: the total is no multiple of 4
    waves.append(np.ascontiguousarray(speech[:480]))      # one frame of either window
    waves.append(np.ascontiguousarray(speech[:640]))      # two frames of either window
    return waves


def _child(path):
    """Runs every case on whichever kernel the environment selects and writes the rows to `path`"""
    sys.path.insert(0, ROOT)
    from shennong_amd import _backend
    from shennong_amd.processor import FilterbankProcessor, MfccProcessor
    # (as the suite's `gpu` fixture does: LDS and pooled device buffers start full of NaN bit patterns)
    _backend.check(_backend.lib().snf_debug_fill_lds(0xFFFFFFFF))
    _backend.DEVICE_POOL.poison = True
    waves = _batch()
    soff = np.zeros(len(waves) + 1, dtype=np.int64)
    np.cumsum([w.shape[0] for w in waves], out=soff[1:])
    d_wave = _backend.upload_rows(waves, np.int16)
    result = {}
    for name, (kind, opts) in CASES.items():
        for dither in DITHERS:
            cls = FilterbankProcessor if kind == 'fbank' else MfccProcessor
            plan = _backend.Plan(cls(dither=dither, **opts)._build_options())
            foff = np.zeros(len(waves) + 1, dtype=np.int64)
            np.cumsum([plan.num_frames(w.shape[0]) for w in waves], out=foff[1:])
            d_out = _backend.DeviceBuffer(int(foff[-1]) * plan.ndims * 4)
            plan.run_device(d_wave.ptr, soff, foff, d_out.ptr, noise_call=NOISE_CALL)
            out = np.empty((int(foff[-1]), plan.ndims), dtype=np.float32)
            d_out.download(out)
            key = '%s_d%d' % (name, int(dither))
            result[key] = out
            result[key + '_kernel'] = np.array(plan.kernel_name(1))
            result[key + '_foff'] = foff
    np.savez(path, **result)


@pytest.fixture(scope='module')
def both(_gpu_backend, tmp_path_factory):
    """{'new': rows of fbank512b_kernel, 'old': rows of fbank512_kernel}, one child process each"""
    where = tmp_path_factory.mktemp('fbank512b_tail')
    got = {}
    for label, knob in (('new', None), ('old', '1')):
        env = dict(os.environ)
        env.pop('SNF_FBANK512_OLD', None)
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
@pytest.mark.parametrize('dither', DITHERS)
@pytest.mark.parametrize('name', list(CASES))
def test_fbank512b_tail_matches_fbank512_bit_for_bit(gpu, both, name, dither):
    key = '%s_d%d' % (name, int(dither))
    new, old = both['new'][key], both['old'][key]
    assert str(both['new'][key + '_kernel']) == 'fbank512b_kernel'
    assert str(both['old'][key + '_kernel']) == 'fbank512_kernel'
    frames = np.diff(both['new'][key + '_foff'])
    # the batch holds what it is meant to hold: utterances of one and two frames, sets with idle rows at the end
    assert (frames == 1).any() and (frames == 2).any() and frames[-1] == 2
    assert frames.sum() == new.shape[0] > 40 and new.shape[0] % 4 != 0
    if 'frame_length' not in CASES[name][1]:
        assert frames[[1, 3]].tolist() == [1, 2]
    opts = CASES[name][1]
    if CASES[name][0] == 'mfcc':
        assert new.shape[1] == opts.get('num_ceps', 13)
    else:
        assert new.shape[1] == opts['num_bins'] + (1 if opts.get('use_energy') else 0)
    assert new.shape == old.shape and new.dtype == old.dtype == np.float32
    # every element, on the bits
    diff = new.view(np.uint32) != old.view(np.uint32)
    rows = np.flatnonzero(diff.any(axis=1))
    print('%s: %d of %d values differ bitwise' % (key, int(diff.sum()), diff.size))
    assert not diff.any(), ('%s: %d values differ, first rows %s: %s vs %s' %
                            (key, int(diff.sum()), rows[:4], new[rows[:1]], old[rows[:1]]))
    assert np.isfinite(new).all()


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        _child(sys.argv[2])
