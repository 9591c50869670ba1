"""CPU checks of DiagUbmProcessor (reference test/processor/test_ubm.py re-stated on our types), of the
host-side GMM (Kaldi binary form, M-step, split) against tests/gmm_f64.py and scikit-learn, and of the
argument checks of the snf_gmm_* entry points"""

import ctypes as C
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_f64 as R  # noqa: E402

from shennong_amd import _backend  # noqa: E402
from shennong_amd import gmm as G  # noqa: E402
from shennong_amd.features import Features, FeaturesCollection  # noqa: E402
from shennong_amd.processor.ubm import DiagUbmProcessor  # noqa: E402


def random_gmm(seed, C=4, D=3):
    rng = np.random.RandomState(seed)
    gmm = G.DiagGmm(C, D)
    gmm.weights_ = (rng.dirichlet(np.ones(C))).astype(np.float32)
    gmm.inv_vars_ = (1 / rng.uniform(0.5, 2, (C, D))).astype(np.float32)
    gmm.means_invvars_ = (rng.randn(C, D) * gmm.inv_vars_).astype(np.float32)
    gmm.compute_gconsts()
    return gmm


def test_params():
    assert len(DiagUbmProcessor(2).get_params()) == 12
    params = {'num_gauss': 16, 'num_iters': 3, 'num_gselect': 5, 'initial_gauss_proportion': 0.7,
              'num_iters_init': 13, 'num_frames': 100, 'subsample': 3, 'min_gaussian_weight': 1e-3,
              'remove_low_count_gaussians': True, 'seed': 1,
              'vad': {'energy_threshold': 4.0}, 'features': {'mfcc': {}}}
    ubm = DiagUbmProcessor(**params)
    got = ubm.get_params()
    assert got['min_gaussian_weight'] == np.float32(1e-3)
    for k, v in params.items():
        if k != 'min_gaussian_weight':
            assert got[k] == v, k
    other = DiagUbmProcessor(2)
    other.set_params(**params)
    assert other.get_params() == got
    assert ubm.name == 'ubm'


def test_defaults():
    ubm = DiagUbmProcessor(2)
    assert ubm.vad['energy_threshold'] == 5.5
    assert ubm.features['sliding_window_cmvn']['cmn_window'] == 300
    assert ubm.features['delta']['window'] == 3
    assert 'mfcc' in ubm.features
    assert ubm.min_gaussian_weight == np.float32(1e-4)
    assert ubm.remove_low_count_gaussians is False


def test_validation():
    with pytest.raises(ValueError, match='Number of gaussians must be at least 2'):
        DiagUbmProcessor(1)
    with pytest.raises(TypeError, match='Features configuration must be a dict'):
        DiagUbmProcessor(2, features='mfcc')
    with pytest.raises(ValueError, match='Need mfcc features to train UBM-GMM'):
        DiagUbmProcessor(2, features={'plp': {}})
    with pytest.raises(TypeError, match='VAD configuration must be a dict'):
        DiagUbmProcessor(2, vad=1)
    with pytest.raises(ValueError, match='Unknown parameters given for VAD config'):
        DiagUbmProcessor(2, vad={'bad': 1})


def collection(*shapes, seed=0):
    rng = np.random.RandomState(seed)
    return FeaturesCollection({f'u{i}': Features(rng.randn(*s).astype(np.float32),
                                                 np.arange(s[0], dtype=np.float64))
                               for i, s in enumerate(shapes)})


def test_initialize_errors():
    ubm = DiagUbmProcessor(10)
    with pytest.raises(ValueError, match='Features have unconsistent dims'):
        ubm.initialize_gmm(collection((20, 3), (20, 4)))
    with pytest.raises(ValueError, match='Too few frames to train on'):
        ubm.initialize_gmm(collection((20, 3)))
    zero = FeaturesCollection(u=Features(np.ones((200, 3), np.float32), np.arange(200, dtype=np.float64)))
    with pytest.raises(ValueError, match='Features do not have positive variance'):
        ubm.initialize_gmm(zero)


def test_selection_and_accumulate_errors():
    ubm = DiagUbmProcessor(4)
    feats = collection((10, 3))
    with pytest.raises(TypeError, match='GMM not initialized'):
        ubm.gaussian_selection(feats)
    with pytest.raises(TypeError, match='GMM not initialized'):
        ubm.accumulate(feats)
    with pytest.raises(TypeError, match='GMM not initialized'):
        ubm.estimate(None)
    with pytest.raises(ValueError, match='Gaussian selection has not been done'):
        ubm.gaussian_selection_to_post(feats)
    ubm.gmm = random_gmm(0, 4, 3)
    ubm.selection = {}
    with pytest.raises(ValueError, match='No gselect information for utterance'):
        ubm.gaussian_selection(feats)
    with pytest.raises(ValueError, match='No gselect information for utterance'):
        ubm.gaussian_selection_to_post(feats)
    ubm.selection = {'u0': [[0, 1]] * 3}
    with pytest.raises(ValueError, match='has wrong size'):
        ubm.gaussian_selection(feats)
    with pytest.raises(ValueError, match='has wrong size'):
        ubm.gaussian_selection_to_post(feats)
    with pytest.raises(ValueError, match='wrong dims'):
        ubm.accumulate(collection((10, 4)))
    with pytest.raises(ValueError, match='Keys differ between weights and features'):
        ubm.accumulate(feats, {'other': np.ones(10)})
    with pytest.raises(ValueError, match='Wrong size for weights'):
        ubm.accumulate(feats, {'u0': np.ones(9)})
    with pytest.raises(ValueError, match='Mixup parameter must be greater than the number of gaussians'):
        ubm.estimate(G.AccumDiagGmm(4, 3), mixup=4)


def test_kaldi_binary_round_trip(tmp_path):
    gmm = random_gmm(1, 5, 7)
    blob = gmm.to_bytes()
    # token sequence, byte-wise
    expect = io.BytesIO()
    expect.write(b'\0B<DiagGMM> <GCONSTS> FV \x04' + struct.pack('<i', 5) + gmm.gconsts_.tobytes())
    expect.write(b'<WEIGHTS> FV \x04' + struct.pack('<i', 5) + gmm.weights_.tobytes())
    expect.write(b'<MEANS_INVVARS> FM \x04' + struct.pack('<i', 5) + b'\x04' + struct.pack('<i', 7)
                 + gmm.means_invvars_.tobytes())
    expect.write(b'<INV_VARS> FM \x04' + struct.pack('<i', 5) + b'\x04' + struct.pack('<i', 7)
                 + gmm.inv_vars_.tobytes())
    expect.write(b'</DiagGMM> ')
    assert blob == expect.getvalue()
    ubm = DiagUbmProcessor(5)
    ubm.gmm = gmm
    path = str(tmp_path / 'ubm.dubm')
    ubm.save(path)
    with pytest.raises(OSError, match='file already exists'):
        ubm.save(path)
    with pytest.raises(OSError, match='file not found'):
        DiagUbmProcessor.load(str(tmp_path / 'missing'))
    other = DiagUbmProcessor.load(path)
    assert other.num_gauss == 5
    for getter in ('weights', 'gconsts', 'get_means', 'get_vars'):
        np.testing.assert_allclose(getattr(other.gmm, getter)(), getattr(gmm, getter)(), rtol=1e-6)
    empty = DiagUbmProcessor(2)
    with pytest.raises(TypeError, match='GMM not initialized'):
        empty.save(str(tmp_path / 'other'))


def test_gconsts_against_f64():
    gmm = random_gmm(2, 6, 5)
    np.testing.assert_allclose(gmm.gconsts(), R.gconsts(gmm.weights_, gmm.get_means(), gmm.get_vars()),
                               rtol=1e-5)


def test_split():
    gmm = random_gmm(3, 3, 4)
    w0, mu0, var0 = gmm.weights().astype(np.float64), gmm.get_means().astype(np.float64), \
        gmm.get_vars().astype(np.float64)
    hist = gmm.split(6, 0.1, np.random.RandomState(5))
    w, mu, var, want_hist = R.split(w0, mu0, var0, 6, 0.1, np.random.RandomState(5))
    assert hist == want_hist
    assert hist[0] == int(np.argmax(w0))
    np.testing.assert_allclose(gmm.weights(), w, rtol=1e-6)
    np.testing.assert_allclose(gmm.get_means(), mu, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gmm.get_vars(), var, rtol=1e-6)
    np.testing.assert_allclose(gmm.gconsts(), R.gconsts(w, mu, var), rtol=1e-5)
    with pytest.raises(ValueError):
        gmm.split(2, 0.1, np.random.RandomState(0))


def _stats(x, gmm, weights=None):
    L = R.loglikes(x, gmm.gconsts_, gmm.means_invvars_, gmm.inv_vars_)
    occ, m1, m2, _ = R.accumulate(x, L, weights)
    acc = G.AccumDiagGmm(gmm.num_gauss(), gmm.dim())
    acc.add_stats(np.concatenate([occ[:, None], m1, m2], axis=1))
    return acc


def test_em_step_equals_sklearn():
    from sklearn.mixture import GaussianMixture
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.randn(300, 2) + [5, 0], rng.randn(500, 2) * 0.5 - [5, 0],
                        rng.randn(200, 2) * 2 + [0, 8]])
    w = np.array([0.3, 0.4, 0.3])
    means = np.array([[4.5, 0.2], [-4.8, 0.1], [0.3, 7.5]])
    var = np.array([[1.2, 0.8], [0.3, 0.4], [3.0, 5.0]])
    gc, mi, iv = R.natural(w, means, var)
    L = R.loglikes(x, gc, mi, iv)
    occ, m1, m2, _ = R.accumulate(x, L)
    w1, mu1, var1, removed = R.mle_update(w, means, var, occ, m1, m2, min_variance=0)
    sk = GaussianMixture(3, covariance_type='diag', reg_covar=0, max_iter=1, weights_init=w, means_init=means,
                         precisions_init=1 / var).fit(x)
    assert not removed
    np.testing.assert_allclose(w1, sk.weights_, rtol=1e-12)
    np.testing.assert_allclose(mu1, sk.means_, rtol=1e-12)
    np.testing.assert_allclose(var1, sk.covariances_, rtol=1e-12)
    # per-frame log-likelihood = score_samples
    ref = GaussianMixture(3, covariance_type='diag', reg_covar=0, max_iter=1, weights_init=w, means_init=means,
                          precisions_init=1 / var)
    ref._initialize_parameters(x, np.random.RandomState(0))
    np.testing.assert_allclose(R.logsumexp(L, axis=1), ref.score_samples(x), rtol=1e-12)
    # integer frame weights = duplicated rows
    k = rng.randint(0, 3, x.shape[0])
    occ_w, m1_w, m2_w, _ = R.accumulate(x, L, k)
    xd = np.repeat(x, k, axis=0)
    occ_d, m1_d, m2_d, _ = R.accumulate(xd, R.loglikes(xd, gc, mi, iv))
    np.testing.assert_allclose(occ_w, occ_d, rtol=1e-12)
    np.testing.assert_allclose(m1_w, m1_d, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(m2_w, m2_d, rtol=1e-12)


@pytest.mark.parametrize('remove', [False, True])
def test_mle_update_corner_cases(remove):
    rng = np.random.RandomState(4)
    gmm = random_gmm(4, 4, 3)
    x = rng.randn(1000, 3).astype(np.float32)
    acc = _stats(x, gmm)
    acc.occupancy[:] = [600.0, 392.0, 5.0, 3.0]     # 2: below the occupancy bound
    acc.mean_accumulator[2:] = 0
    acc.variance_accumulator[0] = acc.occupancy[0] * (acc.mean_accumulator[0] / acc.occupancy[0]) ** 2  # var 0
    acc.occupancy[3] = 11.0                                 # 3: above occupancy, weight 11/1008 > 1e-4
    opts = G.MleDiagGmmOptions(min_gaussian_weight=0.02, remove_low_count_gaussians=remove)
    w0, mu0, var0 = gmm.weights().astype(np.float64), gmm.get_means().astype(np.float64), \
        gmm.get_vars().astype(np.float64)
    _, count, floored, _, removed = G.mle_diag_gmm_update(acc, gmm, opts)
    w, mu, var, want_removed = R.mle_update(w0, mu0, var0, acc.occupancy, acc.mean_accumulator,
                                            acc.variance_accumulator, 0.02, 10.0, 1e-3, remove)
    assert count == acc.occupancy.sum()
    assert floored == 3
    assert removed == len(want_removed) == (2 if remove else 0)
    np.testing.assert_allclose(gmm.weights(), w, rtol=1e-6)
    np.testing.assert_allclose(gmm.get_means(), mu, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gmm.get_vars(), var, rtol=1e-5)
    if not remove:
        # below a bound: mean and variance kept, weight max(prob, min_gaussian_weight)
        np.testing.assert_allclose(gmm.get_means()[2], mu0[2], rtol=1e-6)
        assert gmm.weights()[2] == np.float32(0.02)
        np.testing.assert_allclose(gmm.get_vars()[0], 1e-3, rtol=1e-6)


def test_last_component_never_removed():
    gmm = random_gmm(5, 2, 2)
    acc = G.AccumDiagGmm(2, 2)
    acc.occupancy[:] = [1.0, 2.0]
    _, _, _, _, removed = G.mle_diag_gmm_update(acc, gmm, G.MleDiagGmmOptions())
    assert removed == 1 and gmm.num_gauss() == 1
    assert gmm.weights()[0] == np.float32(1.0)


def _call(name, *args):
    rc = getattr(_backend.lib(), name)(*args)
    return rc, _backend.lib().snf_last_error().decode()


def test_capi_refuses_bad_arguments():
    vp = C.c_void_p
    one = vp(16)  # never dereferenced: every check below fails before any device work
    rc, msg = _call('snf_gmm_loglikes', 0, one, 10, 3, None, one, one, 4, one, None)
    assert rc == -1 and 'null model buffer' in msg
    rc, msg = _call('snf_gmm_loglikes', 0, one, 10, 0, one, one, one, 4, one, None)
    assert rc == -1 and 'dimension' in msg
    rc, msg = _call('snf_gmm_loglikes', 0, None, 10, 3, one, one, one, 4, one, None)
    assert rc == -1 and 'null frames buffer' in msg
    rc, msg = _call('snf_gmm_accumulate', 0, one, 10, 3, None, one, one, one, 0, one, one, None, None)
    assert rc == -1 and 'Gaussians' in msg
    rc, msg = _call('snf_gmm_accumulate', 0, one, 10, 3, None, one, one, one, 4, None, one, None, None)
    assert rc == -1 and 'null statistics buffer' in msg
    rc, msg = _call('snf_gmm_gselect', 0, one, 10, 3, one, one, one, 4, 5, one, None, None)
    assert rc == -1 and 'num_gselect' in msg
    rc, msg = _call('snf_gmm_gselect_preselect', 0, one, 10, 3, one, one, one, 4, one, 3, 4, one, None, None)
    assert rc == -1 and 'num_gselect' in msg
    rc, msg = _call('snf_gmm_gselect_preselect', 0, one, 10, 3, one, one, one, 4, None, 3, 2, one, None, None)
    assert rc == -1 and 'null selection buffer' in msg
    rc, msg = _call('snf_gmm_selection_posteriors', 0, one, 10, 3, one, one, one, 4, one, 0, C.c_float(-1),
                    one, one, None)
    assert rc == -1 and 'num_gselect' in msg
    rc, msg = _call('snf_gmm_selection_posteriors', 0, one, -1, 3, one, one, one, 4, one, 2, C.c_float(-1),
                    one, one, None)
    assert rc == -1 and 'frames' in msg
