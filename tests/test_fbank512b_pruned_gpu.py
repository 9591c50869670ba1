"""fbank512b_kernel against fbank512_kernel, bit for bit, after the trimming pass of the set loop
(kernels_fbank512b.hip, device_fft.h: the select-free left neighbour of phase A, row_head_carry13, and the
mel-phase table reads hoisted out of the loop).

A pruned first FFT pass was part of the same work and is NOT in the tree because it failed exactly this
comparison (tools/experiments/fbank512b_prune_pass1.diff): forwarding an operand where the full transform adds
an exact zero may turn a -0 into +0 and, as it turned out, lets the compiler contract other multiply / add pairs.
The batch holds what could show either: a constant signal (exact zeros behind the DC removal), digital
silence, utterances of one and two frames (sets with idle rows), and ragged speech-like utterances whose sets
straddle utterance boundaries.

Each kernel runs in a child process of its own, which is where the launcher's knob SNF_FBANK512_OLD=1 (every
batch on fbank512_kernel) is set - the way tools/ab_fbank512.cpp selects the kernel.  Every element of every
row is compared; the comparison is on the raw bits, so a NaN or a signed zero cannot hide.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (processor, options).  25 ms windows run the NJ = 13 instantiations, the 30 ms one NJ = 16 (which keeps
# the full transform and the per-element window test).
CASES = {
    'fbank40': ('fbank', dict(num_bins=40)),
    'fbank23_energy': ('fbank', dict(num_bins=23, use_energy=True)),
    'mfcc13': ('mfcc', dict()),
    'fbank40_30ms': ('fbank', dict(num_bins=40, frame_length=0.03)),
}
DITHERS = (0.0, 1.0)
NOISE_CALL = 7  # the same call id on both kernels: the same dither stream


def _batch():
    from shennong_amd import synth
    waves = [np.ascontiguousarray(w) for w in synth.ragged_utterances(5120, 9, min_s=0.05, max_s=0.4)]
    speech = synth.utterances(77, 1, nsamples=1200)[0]
    waves.insert(1, np.ascontiguousarray(speech[:400]))            # one frame of 25 ms (none of 30 ms)
    waves.insert(3, np.ascontiguousarray(speech[:560]))            # two frames
    waves.insert(4, np.full(2000, 1234, dtype=np.int16))           # constant: exact zeros after DC removal
    waves.insert(6, np.zeros(1777, dtype=np.int16))                # digital silence
    waves.append(np.full(481, -32768, dtype=np.int16))             # constant at the rail, one frame
    waves.append(np.ascontiguousarray(speech[:480]))               # one frame of 30 ms
    waves.append(np.ascontiguousarray(speech[:640]))               # two frames of either
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
    where = tmp_path_factory.mktemp('fbank512b_pruned')
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
def test_fbank512b_matches_fbank512_bit_for_bit(gpu, both, name, dither):
    key = '%s_d%d' % (name, int(dither))
    new, old = both['new'][key], both['old'][key]
    assert str(both['new'][key + '_kernel']) == 'fbank512b_kernel'
    assert str(both['old'][key + '_kernel']) == 'fbank512_kernel'
    foff = both['new'][key + '_foff']
    frames = np.diff(foff)
    # the batch holds what it is meant to hold (25 ms: utterances of one and two frames; 30 ms: one frame)
    assert (frames == 1).any() and frames.sum() == new.shape[0] > 40
    assert (frames == 2).any() and frames[-1] == 2
    if 'frame_length' not in CASES[name][1]:
        assert frames[[1, 3]].tolist() == [1, 2]
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
