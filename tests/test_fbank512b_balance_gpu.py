"""The set dealing of fbank512b_kernel: frame sets handed to the waves of a workgroup as they finish.

Every workgroup of fbank512b_kernel (kernels_fbank512b.hip, DEAL) owns a contiguous share of the frame sets and its
16 waves take them from a ticket counter in LDS: the first set of wave w is lo + w, every later one a ticket.  Which
wave transforms a set does not enter the set's arithmetic, so every output keeps the bits fbank512_kernel gives.

The set counts are the seams of the dealing:

    sets1                          one set of 3 frames
    sets15, sets16, sets17         fewer waves than a workgroup / exactly one workgroup / a second workgroup with one
                                   set (the launcher starts ceil(17 / 16) = 2 workgroups: shares of 9 and 8 sets)
    sets4095, sets4096, sets4097   256 workgroups; every wave has one set (one wave has none) / exactly one / the
                                   first workgroup draws one ticket that is a set; frame counts no multiple of 4
    sets12293                      3 x 4096 + 5 sets: every wave draws several tickets and the shares are unequal

The batches are ragged: utterances of 1 to 40 frames with utterances shorter than a window (no frame) between them
and at both ends, so that every row of a set belongs to another mix of utterances than its neighbours.

Forms: fbank-40, fbank-23, MFCC-13 with its raw-energy column, fbank-40 with dither = 1.0 (the key table is read per
set), fbank-40 on a 20 ms window (NJ = 16: the fixed walk stays) and fbank-40 with SNF_FBANK512B_ADDR64=1 (the 64-bit
addressing with the dealing).

Each kernel runs in a child process of its own, where the launcher's knob SNF_FBANK512_OLD=1 selects
fbank512_kernel; LDS and the pooled device buffers start full of NaN bit patterns; every element of every row is
compared on its raw bits, and a canary region behind the output has to stay as it was.  The largest batch also runs
three times on one plan and on two plans on two streams enqueued together: the same bits every time.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# config -> (processor, options, window in seconds, dither)
CONFIGS = {
    'fbank40': ('fbank', dict(num_bins=40), 0.025, 0.0),
    'fbank23': ('fbank', dict(num_bins=23), 0.025, 0.0),
    'mfcc13': ('mfcc', dict(), 0.025, 0.0),
    'fbank40_dither': ('fbank', dict(num_bins=40), 0.025, 1.0),
    'fbank40_20ms': ('fbank', dict(num_bins=40), 0.02, 0.0),
}
ADDR64_CONFIG = 'fbank40'   # the third child (SNF_FBANK512B_ADDR64=1) runs this one
NOISE_CALL = 17             # the same call id on both kernels: the same dither stream
CANARY_WORDS = 1024
CANARY = 0xC0FFEE11

# batch -> frames; sets = ceil(frames / 4)
BATCHES = {
    'sets1': 3,
    'sets15': 58,
    'sets16': 64,
    'sets17': 65,
    'sets4095': 4 * 4095 - 1,
    'sets4096': 4 * 4096 - 2,
    'sets4097': 4 * 4096 + 1,
    'sets12293': 4 * (3 * 4096 + 5) - 3,
}
LARGEST = 'sets12293'


def _utterance_frames(batch):
    """frames per utterance: ragged, 1 .. 40 frames, frameless utterances between them and at both ends"""
    total = BATCHES[batch]
    rng = np.random.RandomState(1000 + sorted(BATCHES).index(batch))
    frames, left = [0], total
    while left > 0:
        n = int(min(left, rng.randint(1, 41)))
        frames.append(n)
        left -= n
        if rng.randint(0, 3) == 0:
            frames.append(0)
    if frames[-1] != 0:
        frames.append(0)
    return frames


def _samples(frames, window):
    win = int(round(window * 16000))
    return win + 160 * (frames - 1) if frames > 0 else 300   # (300 samples: shorter than either window)


def _waves(batch, window):
    frames = _utterance_frames(batch)
    lengths = [_samples(n, window) for n in frames]
    rng = np.random.RandomState(77 + sorted(BATCHES).index(batch))
    total = int(sum(lengths))
    t = np.arange(total, dtype=np.float64)
    signal = 6000.0 * np.sin(2 * np.pi * 190.0 * t / 16000.0) + 2500.0 * np.sin(2 * np.pi * 1370.0 * t / 16000.0)
    wave = np.clip(np.rint(signal + rng.normal(0.0, 1500.0, total)), -32767, 32767).astype(np.int16)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    return [np.ascontiguousarray(wave[bounds[i]:bounds[i + 1]]) for i in range(len(lengths))]


def _processor(config):
    from shennong_amd.processor import FilterbankProcessor, MfccProcessor
    kind, opts, window, dither = CONFIGS[config]
    cls = {'fbank': FilterbankProcessor, 'mfcc': MfccProcessor}[kind]
    return cls(dither=dither, frame_length=window, **opts)


def _key(config, batch):
    return '%s_%s' % (config, batch)


class _Case:
    """one batch on the device: the samples, the offset tables and an output buffer with a canary behind it"""

    def __init__(self, backend, plan, waves):
        self.backend, self.plan = backend, plan
        self.soff = np.zeros(len(waves) + 1, dtype=np.int64)
        np.cumsum([w.shape[0] for w in waves], out=self.soff[1:])
        self.foff = np.zeros(len(waves) + 1, dtype=np.int64)
        np.cumsum([plan.num_frames(w.shape[0]) for w in waves], out=self.foff[1:])
        self.rows, self.cols = int(self.foff[-1]), plan.ndims

    def buffer(self):
        words = self.rows * self.cols
        d_out = self.backend.DeviceBuffer((words + CANARY_WORDS) * 4)
        fill = np.full(words + CANARY_WORDS, 0xFFFFFFFF, dtype=np.uint32)
        fill[words:] = CANARY
        d_out.upload(fill)
        return d_out

    def read(self, d_out):
        words = self.rows * self.cols
        got = np.empty(words + CANARY_WORDS, dtype=np.uint32)
        d_out.download(got)
        assert (got[words:] == CANARY).all(), 'the canary behind the output was written'
        return got[:words].view(np.float32).reshape(self.rows, self.cols).copy()


def _child(path, configs, repeats):
    """Runs every case on whichever kernel the environment selects and writes the rows to `path`"""
    sys.path.insert(0, ROOT)
    from shennong_amd import _backend
    # (as the suite's `gpu` fixture does: LDS and pooled device buffers start full of NaN bit patterns)
    _backend.check(_backend.lib().snf_debug_fill_lds(0xFFFFFFFF))
    _backend.DEVICE_POOL.poison = True
    result, uploaded = {}, {}
    for config in configs:
        window = CONFIGS[config][2]
        options = _processor(config)._build_options()
        plan = _backend.Plan(options)
        for batch in BATCHES:
            if (batch, window) not in uploaded:   # (one audio per batch and window, shared by the configs)
                waves = _waves(batch, window)
                uploaded[batch, window] = waves, _backend.upload_rows(waves, np.int16)
            waves, d_wave = uploaded[batch, window]
            case = _Case(_backend, plan, waves)
            d_out = case.buffer()
            plan.run_device(d_wave.ptr, case.soff, case.foff, d_out.ptr, noise_call=NOISE_CALL)
            key = _key(config, batch)
            result[key] = case.read(d_out)
            names = [plan.kernel_name(i) for i in range(1, 9)]
            result[key + '_kernels'] = np.array(','.join(n for n in names if n))
            result[key + '_foff'] = case.foff
            if repeats and batch == LARGEST:
                # three more times on the same plan, into fresh buffers
                for r in range(3):
                    d_again = case.buffer()
                    plan.run_device(d_wave.ptr, case.soff, case.foff, d_again.ptr, noise_call=NOISE_CALL)
                    result['%s_again%d' % (key, r)] = case.read(d_again)
                # two plans on two streams, enqueued together
                lib = _backend.lib()
                plans = [_backend.Plan(options), _backend.Plan(options)]
                streams, outs = [], []
                for _ in plans:
                    handle = ctypes.c_void_p()
                    _backend.check(lib.snf_stream_create(ctypes.byref(handle)))
                    streams.append(handle.value)
                    outs.append(case.buffer())
                for k in (0, 1, 0, 1):   # (twice each: the second launch of a plan queues behind its first)
                    plans[k].run_device(d_wave.ptr, case.soff, case.foff, outs[k].ptr, stream=streams[k],
                                        noise_call=NOISE_CALL)
                for k, stream in enumerate(streams):
                    _backend.check(lib.snf_stream_synchronize(ctypes.c_void_p(stream)))
                    result['%s_stream%d' % (key, k)] = case.read(outs[k])
                    lib.snf_stream_destroy(ctypes.c_void_p(stream))
    np.savez(path, **result)


@pytest.fixture(scope='module')
def runs(_gpu_backend, tmp_path_factory):
    """{'new': rows of fbank512b_kernel, 'old': rows of fbank512_kernel, 'addr64': fbank512b_kernel with 64-bit
    addresses}, one child process each"""
    where = tmp_path_factory.mktemp('fbank512b_balance')
    got = {}
    for label, knobs, configs in (('new', {}, ','.join(CONFIGS)),
                                  ('old', {'SNF_FBANK512_OLD': '1'}, ','.join(CONFIGS)),
                                  ('addr64', {'SNF_FBANK512B_ADDR64': '1'}, ADDR64_CONFIG)):
        env = dict(os.environ)
        for name in ('SNF_FBANK512_OLD', 'SNF_FBANK512B_ADDR64', 'SNF_FBANK512B_FIXED'):
            env.pop(name, None)
        env.update(knobs)
        path = str(where / (label + '.npz'))
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path, configs,
                               '1' if label == 'new' else '0'], env=env, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert done.returncode == 0, done.stdout.decode(errors='replace')[-2000:]
        with np.load(path) as z:
            got[label] = {k: z[k] for k in z.files}
    return got


def _same_bits(what, new, old):
    assert new.shape == old.shape and new.dtype == old.dtype == np.float32, (what, new.shape, old.shape)
    diff = new.view(np.uint32) != old.view(np.uint32)
    rows = np.flatnonzero(diff.any(axis=1))
    print('%s: %d of %d values differ bitwise' % (what, int(diff.sum()), diff.size))
    assert not diff.any(), ('%s: %d values differ, first rows %s: %s vs %s' %
                            (what, int(diff.sum()), rows[:4], new[rows[:1]], old[rows[:1]]))


def _check(runs, label, config):
    for batch, frames in BATCHES.items():
        key = _key(config, batch)
        new, old = runs[label][key], runs['old'][key]
        assert 'fbank512b_kernel' in str(runs[label][key + '_kernels']).split(','), runs[label][key + '_kernels']
        kernels_old = str(runs['old'][key + '_kernels']).split(',')
        assert 'fbank512_kernel' in kernels_old and 'fbank512b_kernel' not in kernels_old, kernels_old
        # the batch holds what it is meant to hold
        assert np.diff(runs[label][key + '_foff']).tolist() == _utterance_frames(batch) and new.shape[0] == frames
        _same_bits('%s %s' % (label, key), new, old)
        assert np.isfinite(new).all()


@pytest.mark.gpu
@pytest.mark.parametrize('config', list(CONFIGS))
def test_fbank512b_dealt_sets_match_fbank512_bit_for_bit(gpu, runs, config):
    _check(runs, 'new', config)


@pytest.mark.gpu
def test_fbank512b_dealt_sets_with_64_bit_addresses_match_fbank512_bit_for_bit(gpu, runs):
    _check(runs, 'addr64', ADDR64_CONFIG)


@pytest.mark.gpu
@pytest.mark.parametrize('config', list(CONFIGS))
def test_fbank512b_dealt_sets_repeat_on_one_plan_and_on_two_streams(gpu, runs, config):
    key = _key(config, LARGEST)
    old = runs['old'][key]
    for tag in ('again0', 'again1', 'again2', 'stream0', 'stream1'):
        _same_bits('%s %s' % (key, tag), runs['new']['%s_%s' % (key, tag)], old)


def test_batches_sit_on_the_seams_of_the_dealing():
    sets = {name: (frames + 3) // 4 for name, frames in BATCHES.items()}
    assert sets == {'sets1': 1, 'sets15': 15, 'sets16': 16, 'sets17': 17, 'sets4095': 4095, 'sets4096': 4096,
                    'sets4097': 4097, 'sets12293': 3 * 4096 + 5}
    assert BATCHES['sets1'] == 3
    for name in ('sets4095', 'sets4096', 'sets4097', 'sets12293'):
        assert BATCHES[name] % 4 != 0
    for name in BATCHES:
        frames = _utterance_frames(name)
        assert sum(frames) == BATCHES[name] and max(frames) <= 40
        assert frames[0] == 0 and frames[-1] == 0   # frameless utterances at both ends
        if BATCHES[name] > 100:
            assert 0 in frames[1:-1] and min(n for n in frames if n) == 1
    for _, _, window, _ in CONFIGS.values():
        assert _samples(0, window) < int(round(window * 16000))


if __name__ == '__main__':
    if len(sys.argv) == 5 and sys.argv[1] == '--child':
        _child(sys.argv[2], sys.argv[3].split(','), sys.argv[4] == '1')
