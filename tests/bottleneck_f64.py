"""Independent numpy statement of the BUT/Phonexia bottleneck extractor (reference processor/bottleneck.py:
VAD :403-453, HTK filterbank :135-217, context projection :465-474, networks :477-501, glue :699-764),
written from the algorithm's description.  A plain helper module of the test suite: it shares no code with
shennong_amd.processor.bottleneck.  Every stage takes a `dtype` (float64 or float32); the VAD is float64 always.
"""

import numpy as np

WIN, SHIFT, NFFT, NMEL, NBASES, EDGE, NOUT = 200, 80, 256, 24, 6, 15, 80
KEYS = ['bn_std', 'input_mean', 'b2', 'b5', 'input_std', 'W5', 'W7', 'W6', 'b6', 'b7', 'W3', 'W2', 'context',
        'b3', 'bn_mean', 'W1', 'b1']


def make_weights(seed, hidden, context):
    """Synthetic weights in the format of the published files (17 arrays): uniform +-1/sqrt(fan_in) matrices,
    small biases, means ~0.1 and scales in [0.5, 1.5], so that every layer stays in the sigmoid's active range"""
    rng = np.random.RandomState(seed)

    def mat(k, n):
        return rng.uniform(-1.0, 1.0, (k, n)) / np.sqrt(k)

    def vec(n):
        return rng.uniform(-0.1, 0.1, n)

    nin, nstack = NMEL * NBASES, 5 * NOUT
    w = {'context': np.array(context, dtype=np.int64)}
    w['input_mean'], w['input_std'] = vec(nin), rng.uniform(0.5, 1.5, nin)
    w['W1'], w['b1'] = mat(nin, hidden), vec(hidden)
    w['W2'], w['b2'] = mat(hidden, hidden), vec(hidden)
    w['W3'], w['b3'] = mat(hidden, NOUT), vec(NOUT)
    w['bn_mean'], w['bn_std'] = vec(nstack), rng.uniform(0.5, 1.5, nstack)
    w['W5'], w['b5'] = mat(nstack, hidden), vec(hidden)
    w['W6'], w['b6'] = mat(hidden, hidden), vec(hidden)
    w['W7'], w['b7'] = mat(hidden, NOUT), vec(NOUT)
    assert sorted(w) == sorted(KEYS)
    return w


def synthetic_signal(seed=7, seconds=0.6):
    """8 kHz int16: two bursts of a noisy two-tone signal with faint noise before, between and after"""
    rng = np.random.RandomState(seed)
    n = int(8000 * seconds)
    t = np.arange(n) / 8000.0
    gate = ((t > 0.10) & (t < 0.27)) | ((t > 0.38) & (t < 0.52))
    voice = 6000.0 * np.sin(2 * np.pi * 310.0 * t) + 2500.0 * np.sin(2 * np.pi * 1270.0 * t + 0.4)
    x = np.where(gate, voice + 600.0 * rng.randn(n), 0.0) + 12.0 * rng.randn(n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def num_frames(nsamples):
    return int((nsamples - WIN) / SHIFT + 1) if nsamples >= WIN else 0


def _frames(x, width, shift):
    n = int((x.shape[0] - width) / shift + 1)
    idx = shift * np.arange(n)[:, None] + np.arange(width)[None, :]
    return x[idx]


def frame_energy(samples):
    """Per-frame sums of the squares as int16 arithmetic leaves them (they wrap), exact integers"""
    s = np.asarray(samples, dtype=np.int16).astype(np.int64)
    sq = ((s * s + 32768) % 65536) - 32768      # two's-complement wrap to 16 bits
    return _frames(sq, WIN, SHIFT).sum(axis=1)


def vad_posterior(samples, passes=5):
    """Posterior of component 0 per frame, or None where the reference falls back to 'all unvoiced'"""
    e = frame_energy(samples).astype(np.float64)
    if e.size == 0:
        return None
    e = e - e.mean()
    sd = e.std()
    if not (sd > 0 and np.isfinite(sd)):
        return None
    e = e / sd
    w, m, c = np.array([0.33, 0.33, 0.33]), np.array([-1.0, 0.0, 1.0]), np.ones(3)

    def post(w, m, c):
        ll = (np.log(w) - 0.5 * (np.log(c) + m * m / c + np.log(2 * np.pi)))[None, :] \
            + e[:, None] * (m / c)[None, :] - 0.5 * (e * e)[:, None] / c[None, :]
        mx = ll.max(axis=1, keepdims=True)
        ll = ll - (mx + np.log(np.exp(ll - mx).sum(axis=1, keepdims=True)))
        return np.exp(ll)

    with np.errstate(all='ignore'):
        for _ in range(passes):
            p = post(w, m, c)
            n = p.sum(axis=0)
            if not np.all(n > 0):
                return None
            w, m = n / n.sum(), (p * e[:, None]).sum(axis=0) / n
            c = (p * (e * e)[:, None]).sum(axis=0) / n - m * m
            if not (np.all(c > 0) and np.all(w > 0) and np.all(np.isfinite(c)) and np.all(np.isfinite(m))):
                return None
        return post(w, m, c)[:, 0]


def vad(samples):
    p = vad_posterior(samples)
    if p is None:
        return np.zeros(num_frames(len(samples)), dtype=bool)
    return p < 0.3


def mel_scale(hz):
    return 1127.0 * np.log(1.0 + np.asarray(hz, dtype=np.float64) / 700.0)


def mel_matrix(fs=8000, nfft=NFFT, nchan=NMEL, lo=64.0, hi=3800.0):
    """[nfft / 2 + 1, nchan] triangles on the HTK mel scale; bin edges at floor(f / fs * nfft) + 1"""
    bins = mel_scale(np.arange(nfft // 2 + 1) * fs / nfft)
    centres = np.linspace(mel_scale(lo), mel_scale(hi), nchan + 2)
    edge_hz = (np.exp(centres / 1127.0) - 1.0) * 700.0
    edge = np.floor(edge_hz / fs * nfft).astype(int) + 1
    out = np.zeros((nfft // 2 + 1, nchan))
    for i in range(nchan):
        a, b, c = edge[i], edge[i + 1], edge[i + 2]
        out[a:b, i] = (centres[i] - bins[a:b]) / (centres[i] - centres[i + 1])
        out[b:c, i] = (centres[i + 2] - bins[b:c]) / (centres[i + 2] - centres[i + 1])
    if lo > 0.0 and lo / fs * nfft + 0.5 > edge[0]:
        out[edge[0], :] = 0.0
    return out


def logmel(samples, dtype=np.float64):
    dtype = np.dtype(dtype)
    x = _frames(np.asarray(samples).astype(dtype), WIN, SHIFT) * np.hamming(WIN).astype(dtype)
    spec = np.fft.rfft(x, NFFT)
    re, im = spec.real.astype(dtype), spec.imag.astype(dtype)
    power = re * re + im * im
    return np.log(np.maximum(dtype.type(1.0), power @ mel_matrix().astype(dtype)))


def context_basis(context):
    """[(2 context + 1), 6]: orthonormal DCT-II rows 0..5 (row 0 set to sqrt(2 / L)) times a Hamming window"""
    L = 2 * int(context) + 1
    t = np.arange(L)
    rows = np.sqrt(2.0 / L) * np.cos(np.pi * np.arange(NBASES)[:, None] * (2 * t[None, :] + 1) / (2.0 * L))
    rows[0] = np.sqrt(2.0 / L)
    return (rows * np.hamming(L)[None, :]).T


def nn_input(fea, mask, context, dtype=np.float64):
    dtype = np.dtype(dtype)
    fea = np.asarray(fea, dtype=dtype)
    fea = fea - fea[mask].mean(axis=0)
    fea = np.concatenate([np.repeat(fea[:1], EDGE, axis=0), fea, np.repeat(fea[-1:], EDGE, axis=0)])
    L = 2 * int(context) + 1
    rows = fea.shape[0] - L + 1
    win = fea[np.arange(rows)[:, None] + np.arange(L)[None, :]]           # [rows, L, band]
    out = np.einsum('rtb,tj->rbj', win, context_basis(context).astype(dtype))
    return np.ascontiguousarray(out.reshape(rows, NMEL * NBASES).astype(dtype))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(x, weights, dtype=np.float64):
    """(final [rows - 20, 80], first stage [rows, 80])"""
    dtype = np.dtype(dtype)
    w = {k: np.asarray(v).astype(dtype) for k, v in weights.items() if k != 'context'}
    y = (np.asarray(x, dtype=dtype) + w['input_mean']) * w['input_std']
    y = _sigmoid(y @ w['W1'] + w['b1'])
    y = _sigmoid(y @ w['W2'] + w['b2'])
    bn = y @ w['W3'] + w['b3']
    n = bn.shape[0] - 20
    z = np.concatenate([bn[5 * j:5 * j + n] for j in range(5)], axis=1)
    z = (z + w['bn_mean']) * w['bn_std']
    z = _sigmoid(z @ w['W5'] + w['b5'])
    z = _sigmoid(z @ w['W6'] + w['b6'])
    return z @ w['W7'] + w['b7'], bn


def extract(samples, weights, dtype=np.float64):
    """Every recorded stage for one utterance (8 kHz int16, no dither)"""
    context = int(weights['context'])
    mask = vad(samples)
    fea = logmel(samples, dtype)
    out, bn = forward(nn_input(fea, mask, context, dtype), weights, dtype)
    return {'vad': mask, 'logmel': fea, 'bn': bn, 'out': out}


def times(nrows):
    start = np.arange(nrows) * SHIFT
    return (1.0 / 8000) * np.vstack((start, start + WIN)).T
