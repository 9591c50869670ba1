"""Independent numpy statement of the CREPE pitch processor (reference processor/pitch_crepe.py: network
:109-183, decoders :186-243, voicing model :256-291, framing and glue :392-489), written from the algorithm's
description.  A plain helper module of the test suite: it shares no code with shennong_amd.processor.pitch_crepe.
Every stage of the network takes a `dtype` (float64 or float32); the decoders are float64 always.
"""

import numpy as np
import scipy.signal

FRAME, BINS, EPSILON = 1024, 360, 1e-3
MULTIPLIER = {'tiny': 4, 'small': 8, 'medium': 16, 'large': 24, 'full': 32}
WIDTHS = [512, 64, 64, 64, 64, 64]
STRIDES = [4, 1, 1, 1, 1, 1]
CENTS = np.linspace(0, 7180, BINS) + 1997.3794084376191


def filters(capacity):
    return [n * MULTIPLIER[capacity] for n in [32, 4, 4, 4, 8, 16]]


def make_weights(capacity, seed):
    """Synthetic weights under the Keras layer names: kernels with variance 2 / fan_in (so that the activations
    keep their scale through the ReLUs), small biases, batch-normalisation scales of BOTH signs, moving
    variances in [0.5, 1.5], and a classifier wide enough for peaked sigmoids"""
    rng = np.random.RandomState(seed)
    w, c_in = {}, 1
    for l, (c, width) in enumerate(zip(filters(capacity), WIDTHS), 1):
        fan_in = width * c_in
        w['conv%d/kernel' % l] = rng.uniform(-1.0, 1.0, (width, 1, c_in, c)) * np.sqrt(6.0 / fan_in)
        w['conv%d/bias' % l] = rng.uniform(-0.1, 0.1, c)
        w['conv%d-BN/gamma' % l] = rng.uniform(0.5, 1.5, c) * np.where(rng.uniform(size=c) < 0.3, -1.0, 1.0)
        w['conv%d-BN/beta' % l] = rng.uniform(-0.2, 0.2, c)
        w['conv%d-BN/moving_mean' % l] = rng.uniform(0.2, 0.6, c)
        w['conv%d-BN/moving_variance' % l] = rng.uniform(0.5, 1.5, c)
        c_in = c
    w['classifier/kernel'] = rng.uniform(-1.0, 1.0, (4 * c_in, BINS)) * 3.0 * np.sqrt(3.0 / (4 * c_in))
    w['classifier/bias'] = rng.uniform(-0.5, 0.5, BINS) - 2.0
    return w


def synthetic_signal(seed=3, seconds=0.8, f0=180.0):
    """16 kHz int16: a gliding harmonic tone with a pause in the middle, over faint noise"""
    rng = np.random.RandomState(seed)
    n = int(16000 * seconds)
    t = np.arange(n) / 16000.0
    phase = 2 * np.pi * np.cumsum(f0 * (1.0 + 0.3 * np.sin(2 * np.pi * 1.5 * t))) / 16000.0
    voice = 5000.0 * np.sin(phase) + 2000.0 * np.sin(2 * phase + 0.3) + 900.0 * np.sin(3 * phase + 1.1)
    gate = (t < 0.35 * seconds) | (t > 0.5 * seconds)
    x = np.where(gate, voice, 0.0) + 40.0 * rng.randn(n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


# ---- framing ------------------------------------------------------------------------------------------------
def num_frames(nsamples, hop, center=True):
    padded = nsamples + (FRAME if center else 0)
    return 1 + (padded - FRAME) // hop if padded >= FRAME else 0


def frames_of(samples, hop, center=True, dtype=np.float64):
    """[frames, 1024]: every frame minus its mean, over its deviation (floored at 1e-8)"""
    x = np.asarray(samples).astype(dtype)
    if center:
        x = np.concatenate([np.zeros(FRAME // 2, dtype), x, np.zeros(FRAME // 2, dtype)])
    n = num_frames(len(samples), hop, center)
    frames = x[hop * np.arange(n)[:, None] + np.arange(FRAME)[None, :]].copy()
    frames -= frames.mean(axis=1, dtype=dtype)[:, None]
    deviation = np.sqrt((frames * frames).mean(axis=1, dtype=dtype))
    return (frames / np.maximum(deviation, dtype(1e-8))[:, None]).astype(dtype)


# ---- network ------------------------------------------------------------------------------------------------
def same_padding(length, width, stride):
    """(positions, zeros before, zeros after) of a 'same' convolution"""
    positions = -(-length // stride)
    total = max((positions - 1) * stride + width - length, 0)
    return positions, total // 2, total - total // 2


def conv(x, kernel, stride, dtype=np.float64):
    """'same' correlation along axis 1 of x [frames, length, C_in] with kernel [width, C_in, C_out], no bias"""
    x, kernel = x.astype(dtype), kernel.astype(dtype)
    frames, length, c_in = x.shape
    width, _, c_out = kernel.shape
    positions, before, after = same_padding(length, width, stride)
    xp = np.concatenate([np.zeros((frames, before, c_in), dtype), x, np.zeros((frames, after, c_in), dtype)], axis=1)
    if c_in == 1:
        taps = xp[:, stride * np.arange(positions)[:, None] + np.arange(width)[None, :], 0]
        return taps @ kernel[:, 0, :]
    out = np.zeros((frames, positions, c_out), dtype)
    span = (positions - 1) * stride + 1
    for j in range(width):
        out += xp[:, j:j + span:stride, :] @ kernel[j]
    return out


def pool(x):
    frames, length, c = x.shape
    return x.reshape(frames, length // 2, 2, c).max(axis=2)


def block(x, weights, l, dtype=np.float64):
    """Convolution block `l` (1..6): convolution + bias, ReLU, batch normalisation (inference), max-pool 2"""
    k = weights['conv%d/kernel' % l]
    y = conv(x, k.reshape(k.shape[0], k.shape[2], k.shape[3]), STRIDES[l - 1], dtype)
    y = np.maximum(y + weights['conv%d/bias' % l].astype(dtype), dtype(0))
    name = 'conv%d-BN/' % l
    g, b, m, v = (weights[name + n].astype(dtype) for n in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
    y = (y - m) / np.sqrt(v + dtype(EPSILON)) * g + b
    return pool(y.astype(dtype))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def activation_of_frames(frames, weights, dtype=np.float64):
    x = frames.astype(dtype)[:, :, None]
    for l in range(1, 7):
        x = block(x, weights, l, dtype)
    flat = x.reshape(x.shape[0], -1)        # time-major, channels innermost
    z = flat @ weights['classifier/kernel'].astype(dtype) + weights['classifier/bias'].astype(dtype)
    return sigmoid(z).astype(dtype)


def activation(samples, weights, hop=160, center=True, dtype=np.float64):
    return activation_of_frames(frames_of(samples, hop, center, dtype), weights, dtype)


# ---- decoders -----------------------------------------------------------------------------------------------
def local_average_cents(salience, centre):
    """Weighted average of the bins' cents over [centre - 4, centre + 5) clipped to the 360 bins"""
    lo, hi = max(0, centre - 4), min(BINS, centre + 5)
    s = np.asarray(salience[lo:hi], dtype=np.float64)
    return float(np.sum(s * CENTS[lo:hi]) / np.sum(s))


def hmm_tables():
    """(log start [360], log transition [360, 360] from -> to, log emission [360 states, 360 symbols])"""
    i = np.arange(BINS)
    transition = np.maximum(12 - np.abs(i[:, None] - i[None, :]), 0).astype(np.float64)
    transition /= transition.sum(axis=1)[:, None]
    emission = np.eye(BINS) * 0.1 + np.ones((BINS, BINS)) * (0.9 / BINS)
    with np.errstate(divide='ignore'):
        return np.log(np.ones(BINS) / BINS), np.log(transition), np.log(emission)


def viterbi_path(observations):
    """Most likely state sequence for the symbols `observations`, first index on ties"""
    start, transition, emission = hmm_tables()
    obs = np.asarray(observations, dtype=int)
    n = len(obs)
    lattice = np.empty((n, BINS))
    back = np.zeros((n, BINS), dtype=int)
    lattice[0] = start + emission[:, obs[0]]
    for t in range(1, n):
        scores = lattice[t - 1][:, None] + transition
        back[t] = np.argmax(scores, axis=0)
        lattice[t] = scores[back[t], np.arange(BINS)] + emission[:, obs[t]]
    path = np.empty(n, dtype=int)
    path[-1] = int(np.argmax(lattice[-1]))
    for t in range(n - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path


def decode(act, viterbi=True):
    """(confidence [n], cents [n], first argmax [n], chosen bin [n]) of an activation [n, 360]"""
    act = np.asarray(act)
    first = np.argmax(act, axis=1)
    chosen = viterbi_path(first) if viterbi else first
    cents = np.array([local_average_cents(act[t], int(chosen[t])) for t in range(len(act))])
    return act.max(axis=1).astype(np.float64), cents, first, chosen


def hertz(cents):
    f = 10.0 * 2.0 ** (np.asarray(cents, dtype=np.float64) / 1200.0)
    f[np.isnan(f)] = 0
    return f


def raw_rows(act, viterbi=True):
    """[n, 2] (confidence, Hertz) per network frame"""
    confidence, cents, _, _ = decode(act, viterbi)
    return np.stack([confidence, hertz(cents)], axis=1)


def output_rows(nsamples, frame_shift=0.01, frame_length=0.025):
    return 1 + int((nsamples - frame_length * 16000) / int(np.round(16000 * frame_shift)))


def finish(rows, nsamples, frame_shift=0.01, frame_length=0.025):
    """The network's rows brought to the output's row count by the Fourier method, the confidence clamped"""
    data = scipy.signal.resample(rows, output_rows(nsamples, frame_shift, frame_length))
    data[data[:, 0] < 1e-2, 0] = 0
    data[data[:, 0] > 1, 0] = 1
    return data


def process(samples, weights, viterbi=True, center=True, frame_shift=0.01, frame_length=0.025, dtype=np.float64):
    """The whole processor on 16 kHz samples: [rows, 2] float64 (POV, Hertz)"""
    act = activation(samples, weights, int(16000 * frame_shift), center, dtype)
    return finish(raw_rows(act, viterbi), len(samples), frame_shift, frame_length)


def times(nframes, frame_shift=0.01, frame_length=0.025):
    start = np.arange(nframes) * frame_shift
    return np.vstack((start, start + frame_length)).T


# ---- voicing model ------------------------------------------------------------------------------------------
def voicing(confidence):
    """Voiced (1) / unvoiced (0) per frame: two states with Gaussian emissions N(0, 0.25) and N(1, 0.25), self
    transition 0.99, uniform start; Viterbi in the log domain, first index on ties"""
    c = np.asarray(confidence, dtype=np.float64)
    n = len(c)
    emission = np.stack([-0.5 * np.log(2 * np.pi * 0.25) - (c - m) ** 2 / (2 * 0.25) for m in (0.0, 1.0)], axis=1)
    transition = np.log(np.array([[0.99, 0.01], [0.01, 0.99]]))
    lattice = np.empty((n, 2))
    back = np.zeros((n, 2), dtype=int)
    lattice[0] = np.log(0.5) + emission[0]
    for t in range(1, n):
        for j in range(2):
            scores = lattice[t - 1] + transition[:, j]
            back[t, j] = int(np.argmax(scores))
            lattice[t, j] = scores[back[t, j]] + emission[t, j]
    path = np.empty(n, dtype=int)
    path[-1] = int(np.argmax(lattice[-1]))
    for t in range(n - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path
