"""GPU checks of the diagonal-GMM kernels (kernels_gmm.hip) and of DiagUbmProcessor against the float64
statement of tests/gmm_f64.py and scikit-learn"""

import os
import sys

import numpy as np
import pytest
import scipy.io.wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_f64 as R  # noqa: E402

from shennong_amd import gmm as G  # noqa: E402

pytestmark = pytest.mark.gpu


def mixture(seed, F, D, C, sep=6.0):
    """Separated synthetic mixture with clearly unequal proportions and a model near it"""
    rng = np.random.RandomState(seed)
    centers = rng.randn(C, D) * sep
    props = np.linspace(1.0, 3.0, C)
    props /= props.sum()
    labels = rng.choice(C, size=F, p=props)
    x = (centers[labels] + rng.randn(F, D)).astype(np.float32)
    gmm = G.DiagGmm(C, D)
    gmm.weights_ = props.astype(np.float32)
    gmm.inv_vars_ = (1.0 / rng.uniform(0.5, 2.0, (C, D))).astype(np.float32)
    gmm.means_invvars_ = ((centers + 0.3 * rng.randn(C, D)) * gmm.inv_vars_).astype(np.float32)
    gmm.compute_gconsts()
    return x, gmm


def model64(gmm):
    return (gmm.gconsts_.astype(np.float64), gmm.means_invvars_.astype(np.float64),
            gmm.inv_vars_.astype(np.float64))


SHAPES = [(1, 2, 1), (31, 5, 2), (33, 37, 13), (1000, 64, 39), (1000, 129, 40), (200, 2048, 39),
          (33, 5, 100), (1000, 2, 1)]


@pytest.mark.parametrize('F,C,D', SHAPES)
def test_loglikes_and_fused_agree(gpu, F, C, D):
    x, gmm = mixture(F + C + D, F, D, C)
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    L = block.loglikes(dg)
    want = R.loglikes(x, *model64(gmm))
    bound = R.loglike_bound(x, *model64(gmm))
    ratio = np.max(np.abs(L - want) / bound)
    assert ratio <= 1e-5, ratio
    # gselect (n = C): exactly the order of the downloaded L under the tie rule
    idx, gl = block.gselect(dg, C)
    np.testing.assert_array_equal(idx, R.gselect(L, C))
    lse = R.logsumexp(L, axis=1)
    np.testing.assert_allclose(gl, lse, rtol=1e-6, atol=1e-6)
    stats, tot, alse = block.accumulate(dg, with_lse=True)
    np.testing.assert_allclose(alse, lse, rtol=1e-6, atol=1e-6)
    # the gathered path (preselection = all Gaussians, reversed) sees the same bits of L
    pre = np.tile(np.arange(C)[::-1], (F, 1)).astype(np.int32)
    idx2, _ = block.gselect(dg, C, preselect=pre)
    np.testing.assert_array_equal(idx2, idx)
    post, like = block.selection_posteriors(dg, idx)
    np.testing.assert_allclose(like, lse, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('F,C,D', SHAPES + [(200000, 64, 39)])
@pytest.mark.parametrize('weighted', [False, True])
def test_accumulate_against_f64_fed_with_hip_L(gpu, F, C, D, weighted):
    x, gmm = mixture(3 * F + C, F, D, C)
    w = np.random.RandomState(F).uniform(0, 2, F).astype(np.float32) if weighted else None
    block = G.FrameBlock([x], None if w is None else [w])
    dg = G.DeviceGmm(gmm)
    L = block.loglikes(dg)
    stats, tot, _ = block.accumulate(dg)
    occ, m1, m2, tl = R.accumulate(x, L, w)
    want = np.concatenate([occ[:, None], m1, m2], axis=1)
    scale = np.max(np.abs(want), axis=1, keepdims=True) + 1e-30
    assert np.max(np.abs(stats - want) / scale) <= 1e-5
    assert abs(tot - tl) <= 1e-5 * np.sum(np.abs(R.logsumexp(L, axis=1)) * (1 if w is None else w))
    # deterministic
    stats2, tot2, _ = block.accumulate(dg)
    assert np.array_equal(stats, stats2) and tot == tot2


def test_gselect_against_f64_and_preselect_ties(gpu):
    x, gmm = mixture(7, 1000, 39, 129)
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    idx, _ = block.gselect(dg, 15)
    want_L = R.loglikes(x, *model64(gmm))
    want = R.gselect(want_L, 15)
    bound = R.loglike_bound(x, *model64(gmm))
    srt = np.sort(want_L, axis=1)[:, ::-1]
    for f in np.nonzero(np.any(idx != want, axis=1))[0]:
        assert srt[f, 14] - srt[f, 15] <= 2e-5 * np.max(bound[f])
    # preselect: the top 7 of the top 15
    idx7, l7 = block.gselect(dg, 7, preselect=idx)
    L = block.loglikes(dg)
    np.testing.assert_array_equal(idx7, R.gselect(L, 7, preselect=idx))
    # constructed ties: two identical Gaussians -> the higher index ranks first
    g2 = G.DiagGmm(4, 3)
    g2.weights_[:] = 0.25
    g2.inv_vars_[:] = 1
    g2.means_invvars_[:] = np.array([[0, 0, 0], [1, 1, 1], [0, 0, 0], [5, 5, 5]], np.float32)
    g2.compute_gconsts()
    xb = G.FrameBlock([np.zeros((3, 3), np.float32)])
    d2 = G.DeviceGmm(g2)
    i2, _ = xb.gselect(d2, 2)
    np.testing.assert_array_equal(i2, [[2, 0]] * 3)
    i3, _ = xb.gselect(d2, 2, preselect=np.array([[0, 2, 3]] * 3, np.int32))
    np.testing.assert_array_equal(i3, [[2, 0]] * 3)


def test_selection_posteriors_and_sequential_pruning(gpu):
    x, gmm = mixture(11, 500, 13, 37)
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    idx, _ = block.gselect(dg, 15)
    L = block.loglikes(dg)
    Lsel = np.take_along_axis(L, idx, axis=1)
    for min_post in (None, 0.01, 0.2):
        post, like = block.selection_posteriors(dg, idx, min_post)
        want, wlike = R.selection_posteriors(Lsel, min_post)
        np.testing.assert_allclose(post, want, atol=2e-6)
        np.testing.assert_allclose(like, wlike, rtol=1e-6)
    # a frame where sequential pruning differs from a one-shot renormalisation: posteriors
    # (0.3, 0.25, 0.25, 0.2), min_post 0.26: sequentially 0.25 -> 0.333 survives, one-shot prunes it
    p = np.array([0.3, 0.25, 0.25, 0.2])
    g3 = G.DiagGmm(4, 1)
    g3.weights_ = p.astype(np.float32)
    g3.inv_vars_[:] = 1e-6
    g3.means_invvars_[:] = 0
    g3.compute_gconsts()
    b3 = G.FrameBlock([np.zeros((1, 1), np.float32)])
    post, _ = b3.selection_posteriors(G.DeviceGmm(g3), np.array([[0, 1, 2, 3]], np.int32), 0.26)
    seq, _ = R.selection_posteriors(np.log(p)[None, :], 0.26)
    oneshot = np.where(p >= 0.26, p, 0) / np.where(p >= 0.26, p, 0).sum()
    assert not np.allclose(seq, oneshot)
    np.testing.assert_allclose(post, seq, atol=1e-6)


def test_em_step_against_sklearn(gpu):
    from sklearn.mixture import GaussianMixture
    x, gmm = mixture(5, 20000, 13, 5)
    means, var, w = gmm.get_means().astype(np.float64), gmm.get_vars().astype(np.float64), gmm.weights_
    w = w.astype(np.float64)
    w /= w.sum()
    gmm.weights_ = w.astype(np.float32)
    gmm.compute_gconsts()
    block = G.FrameBlock([x])
    stats, _, _ = block.accumulate(G.DeviceGmm(gmm))
    G.mle_diag_gmm_update(G.AccumDiagGmm.from_stats(stats), gmm, G.MleDiagGmmOptions(min_variance=0))
    sk = GaussianMixture(5, covariance_type='diag', reg_covar=0, max_iter=1, weights_init=w,
                         means_init=means, precisions_init=1 / var).fit(x.astype(np.float64))
    for got, want in ((gmm.weights_[None, :], sk.weights_[None, :]), (gmm.get_means(), sk.means_),
                      (gmm.get_vars(), sk.covariances_)):
        scale = np.max(np.abs(want), axis=1, keepdims=True)
        assert np.max(np.abs(got - want) / scale) <= 1e-4


def _synthetic_features(seed, F, D=13):
    rng = np.random.RandomState(seed)
    C = 6
    centers = rng.randn(C, D) * 4
    props = np.array([0.35, 0.25, 0.15, 0.12, 0.08, 0.05])
    labels = rng.choice(C, size=F, p=props)
    return (centers[labels] + rng.randn(F, D) * rng.uniform(0.5, 1.5, D)).astype(np.float32)


@pytest.mark.parametrize('num_gauss', [8, 64])
def test_training_against_f64_loop(gpu, num_gauss):
    from shennong_amd.features import Features, FeaturesCollection
    from shennong_amd.processor.ubm import DiagUbmProcessor
    x = _synthetic_features(num_gauss, 6000)
    parts = np.split(x, [1000, 3500])
    coll = FeaturesCollection({f'u{i}': Features(p, np.arange(p.shape[0], dtype=np.float64) * 0.01)
                               for i, p in enumerate(parts)})
    models = []
    for _ in range(2):
        ubm = DiagUbmProcessor(num_gauss, num_iters_init=6, num_frames=5000, seed=3)
        ubm.initialize_gmm(coll)
        sub = FeaturesCollection({u: f.copy(subsample=ubm.subsample) for u, f in coll.items()})
        ubm.remove_low_count_gaussians = False
        for _ in range(2):
            ubm.estimate(ubm.accumulate(sub))
        models.append(ubm)
    a, b = models
    for getter in ('weights', 'get_means', 'get_vars'):
        assert np.array_equal(getattr(a.gmm, getter)(), getattr(b.gmm, getter)())
    log = []
    sub = np.concatenate([p[::a.subsample] for p in parts])
    w, mu, var = R.train(x, num_gauss, 6, 2, seed=3, num_frames=5000, subsample_feats=sub, log=log)
    assert [h for kind, h in log if kind == 'split'] == a.split_history
    assert a.gmm.num_gauss() == w.shape[0]
    for got, want in ((a.gmm.weights(), w), (a.gmm.get_means(), mu), (a.gmm.get_vars(), var)):
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * np.max(np.abs(want)))


@pytest.mark.parametrize('features', ['default', 'plain'])
def test_process_reference_configs(gpu, tmp_path, wav_file, features):
    """The reference's test_process: 16 kHz, float32 and 8 kHz audio with segments, num_frames=100"""
    from shennong_amd import Utterances, pipeline
    from shennong_amd.processor.ubm import DiagUbmProcessor
    rate, data = scipy.io.wavfile.read(wav_file)
    f32 = str(tmp_path / 'test.f32.wav')
    scipy.io.wavfile.write(f32, rate, (data / 2 ** 15).astype(np.float32))
    wav8 = os.path.join(os.path.dirname(wav_file), 'test.8k.wav')
    utts = Utterances([('utt1', wav_file, 'spk1', 0, 1.2), ('utt2', f32, 'spk1', 0.1, 1.4),
                       ('utt3', wav8, 'spk2', 0, 1.3)])
    config = None if features == 'default' else pipeline.get_default_config('mfcc', with_cmvn=False)
    ubm = DiagUbmProcessor(2, num_iters_init=1, num_iters=1, num_frames=100, vad={'energy_threshold': 0},
                           features=config)
    ubm.process(utts)
    assert ubm.gmm.num_gauss() == 2
    assert ubm.gmm.get_means().shape[1] == (39 if features == 'default' else 13)


def test_doc_example(gpu, wav_file):
    from shennong_amd import Utterances
    from shennong_amd.processor import DiagUbmProcessor
    utterances = Utterances([('utt1', wav_file, 'spk1', 0, 1), ('utt2', wav_file, 'spk1', 1, 1.4)])
    ubm = DiagUbmProcessor(4, num_iters_init=10)
    ubm.num_iters = 3
    ubm.process(utterances)
    means = ubm.gmm.get_means()
    assert means.shape[0] == 4 and means.shape[1] == 39


def test_selection_api_and_real_features(gpu, audio):
    from shennong_amd.features import FeaturesCollection
    from shennong_amd.postprocessor import DeltaPostProcessor
    from shennong_amd.processor import DiagUbmProcessor, MfccProcessor
    feats = DeltaPostProcessor().process(MfccProcessor().process(audio))
    coll = FeaturesCollection(utt=feats)
    ubm = DiagUbmProcessor(4, num_gselect=6)
    ubm.initialize_gmm(coll)
    L = G.FrameBlock([feats.data]).loglikes(G.DeviceGmm(ubm.gmm))
    gc, mi, iv = model64(ubm.gmm)
    assert np.max(np.abs(L - R.loglikes(feats.data, gc, mi, iv)) / R.loglike_bound(feats.data, gc, mi, iv)) <= 1e-5
    ubm.gaussian_selection(coll)                      # warns and clamps to 4
    assert ubm.num_gselect == 4 and ubm.selection['utt'].shape == (140, 4)
    ubm.selection = {'utt': ubm.selection['utt'].tolist()}   # lists are accepted, as the reference tests assign
    ubm.gaussian_selection(coll)                      # with a preselection
    post = ubm.gaussian_selection_to_post(coll, min_post=0.1)
    assert len(post['utt']) == 140
    assert all(abs(sum(p for _, p in frame) - 1) < 1e-5 for frame in post['utt'])
