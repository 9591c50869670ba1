"""CPU checks of linear VTLN: the float64 statement of tests/lvtln_f64.py pinned independently, the
reference's VtlnProcessor parameter and file tests restated, the LinearVtln bytes, and the argument checks
of the snf_* VTLN entry points"""

import ctypes as C
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lvtln_f64 as R  # noqa: E402

from shennong_amd import _abi, _backend  # noqa: E402
from shennong_amd import lvtln as LV  # noqa: E402
from shennong_amd.features import Features, FeaturesCollection  # noqa: E402
from shennong_amd.processor.vtln import VtlnProcessor, mapping_from_gram  # noqa: E402


def problem(seed, F=60, D=3, C=4, n=3):
    rng = np.random.RandomState(seed)
    x = rng.randn(F, D)
    mu = rng.randn(C, D)
    iv = 1.0 / rng.uniform(0.5, 2.0, (C, D))
    sel = np.stack([rng.choice(C, n, replace=False) for _ in range(F)])
    post = rng.dirichlet(np.ones(n), size=F)
    return x, mu, iv, sel, post


def log_normal(z, mu, iv):
    return 0.5 * np.sum(np.log(iv)) - 0.5 * z.shape[-1] * np.log(2 * np.pi) - 0.5 * np.sum((z - mu) ** 2 * iv)


def test_aux_is_the_log_likelihood():
    x, mu, iv, sel, post = problem(0)
    D = x.shape[1]
    stats = R.fmllr_stats(x, sel, post, mu * iv, iv)
    rng = np.random.RandomState(1)
    W = np.concatenate([np.eye(D) + 0.2 * rng.randn(D, D), 0.3 * rng.randn(D, 1)], axis=1)
    direct = 0.0
    for f in range(len(x)):
        y = W[:, :D] @ x[f] + W[:, D]
        for g, p in zip(sel[f], post[f]):
            direct += p * (log_normal(y, mu[g], iv[g]) - log_normal(x[f], mu[g], iv[g]))
    direct += stats[0] * np.linalg.slogdet(W[:, :D])[1]
    got = R.aux(W, stats) - R.aux(np.eye(D, D + 1), stats)
    assert got == pytest.approx(direct, rel=1e-10, abs=1e-10)


def test_vectorised_stats_equal_frame_loop():
    x, mu, iv, sel, post = problem(2, D=4)
    a, b = R.fmllr_stats(x, sel, post, mu * iv, iv), R.fmllr_stats_loop(x, sel, post, mu * iv, iv)
    assert a[0] == pytest.approx(b[0])
    np.testing.assert_allclose(a[1], b[1], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('solve', ['offset', 'diag'])
def test_solves_are_stationary_and_optimal(solve):
    x, mu, iv, sel, post = problem(3)
    D = x.shape[1]
    stats = R.fmllr_stats(x, sel, post, mu * iv, iv)
    W = R.solve_offset(stats) if solve == 'offset' else R.solve_diag(stats)
    free = [(i, D) for i in range(D)] + ([(i, i) for i in range(D)] if solve == 'diag' else [])
    base = R.aux(W, stats)
    for (i, j) in free:
        h = 1e-6
        Wp, Wm = W.copy(), W.copy()
        Wp[i, j] += h
        Wm[i, j] -= h
        assert abs((R.aux(Wp, stats) - R.aux(Wm, stats)) / (2 * h)) < 1e-5 * max(1.0, abs(base))
    rng = np.random.RandomState(4)
    for _ in range(20):
        Wr = W.copy()
        for (i, j) in free:
            Wr[i, j] += 0.05 * rng.randn()
        assert R.aux(Wr, stats) <= base


def test_mapping_transform_is_scaled_least_squares():
    rng = np.random.RandomState(5)
    x = rng.randn(500, 3)
    y = x @ (np.eye(3) + 0.3 * rng.randn(3, 3)).T + 1.0 + 0.1 * rng.randn(500, 3)
    w = rng.rand(500)
    A = R.mapping_transform(x, y, w)
    xp = np.concatenate([x, np.ones((500, 1))], axis=1)
    sw = np.sqrt(w)[:, None]
    lst = np.linalg.lstsq(xp * sw, y * sw, rcond=None)[0].T
    scale = A[:, 0] / lst[:, 0]
    np.testing.assert_allclose(A, lst[:, :3] * scale[:, None], rtol=1e-9)
    # scaled rows: the variance of the mapped x equals the variance of x, per dimension
    mapped = x @ A.T
    mean = lambda v: (w @ v) / w.sum()  # noqa: E731
    np.testing.assert_allclose(mean(mapped ** 2) - mean(mapped) ** 2 - 0, mean(x ** 2) - mean(x) ** 2, rtol=1e-9)
    # the processor's Gram route
    z = np.concatenate([x, np.ones((500, 1)), y], axis=1)
    got, _ = mapping_from_gram((z * w[:, None]).T @ z, 3)
    np.testing.assert_allclose(got, A, rtol=1e-5, atol=1e-6)


def test_params():
    assert len(VtlnProcessor().get_params()) == 10
    p = {'num_iters': 3, 'min_warp': 1, 'max_warp': 1.1, 'warp_step': 0.02, 'logdet_scale': 0.5,
         'norm_type': 'diag', 'subsample': 3, 'by_speaker': False}
    proc = VtlnProcessor(**p)
    got = proc.get_params()
    for k, v in p.items():
        assert got[k] == v
    with pytest.raises(ValueError, match='Invalid norm type'):
        proc.norm_type = 'wrong'
    with pytest.raises(TypeError):
        proc.features = 'a'
    with pytest.raises(ValueError, match='Need mfcc'):
        proc.features = {'plp': {}}
    with pytest.raises(TypeError):
        proc.ubm = 'a'
    with pytest.raises(ValueError, match='Unknown parameters'):
        proc.ubm = {'wrong': 1}


def test_load_save_model(tmp_path):
    proc = VtlnProcessor()
    with pytest.raises(TypeError, match='VTLN not initialized'):
        proc.save(str(tmp_path / 'm'))
    proc.lvtln = LV.LinearVtln(5, 3, 1)
    proc.lvtln.set_transform(2, np.arange(25, dtype=np.float32).reshape(5, 5) + np.eye(5, dtype=np.float32))
    proc.lvtln.set_warp(2, 1.1)
    path = str(tmp_path / 'lvtln.ark')
    proc.save(path)
    with pytest.raises(OSError, match='already exists'):
        proc.save(path)
    with pytest.raises(OSError, match='not found'):
        VtlnProcessor.load(str(tmp_path / 'none'))
    got = VtlnProcessor.load(path).lvtln
    assert got.num_classes() == 3 and got.dim() == 5 and got.default_class == 1
    np.testing.assert_array_equal(got.get_transform(2), proc.lvtln.get_transform(2))
    assert got.get_warp(2) == pytest.approx(1.1) and got.logdets == proc.lvtln.logdets


def test_load_save_warps(tmp_path):
    proc = VtlnProcessor()
    with pytest.raises(TypeError, match='Warps not computed'):
        proc.save_warps(str(tmp_path / 'w'))
    proc.warps = {'a': 1.0, 'b': 0.95}
    path = str(tmp_path / 'w.yml')
    proc.save_warps(path)
    assert VtlnProcessor.load_warps(path) == proc.warps
    with pytest.raises(OSError):
        proc.save_warps(path)
    with pytest.raises(OSError):
        VtlnProcessor.load_warps(str(tmp_path / 'none'))


def test_lvtln_bytes_layout():
    lv = LV.LinearVtln(2, 2, 1)
    lv.set_transform(0, [[1, 2], [3, 4]])
    lv.set_warp(0, 0.9)
    want = b'\0B<LinearVtln> \4' + struct.pack('<i', 2)
    for A, w in ((np.array([[1, 2], [3, 4]], '<f4'), 0.9), (np.eye(2, dtype='<f4'), 1.0)):
        want += (b'<Transform> FM \4' + struct.pack('<i', 2) + b'\4' + struct.pack('<i', 2) + A.tobytes()
                 + b'<Warp> \4' + struct.pack('<f', w))
    want += b'<DefaultClass> \4' + struct.pack('<i', 1) + b'</LinearVtln> '
    assert lv.to_bytes() == want
    back = LV.LinearVtln.from_bytes(want)
    assert back.default_class == 1 and back.logdets[0] == pytest.approx(np.log(2.0))
    legacy = want[:want.index(b'<DefaultClass>')] + b'</LinearVtln> '
    assert LV.LinearVtln.from_bytes(legacy).default_class == 1   # (2 + 1) // 2
    assert LV.LinearVtln(3, 5, 2).logdets == [0.0] * 5


def test_compute_mapping_transform_and_estimate_errors():
    proc = VtlnProcessor()
    feats = FeaturesCollection(u=Features(np.zeros((4, 3), np.float32), np.arange(4.0)))
    with pytest.raises(TypeError, match='VTLN not initialized'):
        proc.compute_mapping_transform(feats, feats, 0, 1.0)
    with pytest.raises(TypeError, match='VTLN not initialized'):
        proc.estimate(None, feats, {})
    proc.lvtln = LV.LinearVtln(3, 2, 1)
    with pytest.raises(ValueError, match='No transformed features'):
        proc.compute_mapping_transform(feats, FeaturesCollection(), 0, 1.0)
    other = FeaturesCollection(u=Features(np.zeros((5, 3), np.float32), np.arange(5.0)))
    with pytest.raises(ValueError, match='Number of rows'):
        proc.compute_mapping_transform(feats, other, 0, 1.0)
    with pytest.raises(ValueError, match='No weights'):
        proc.compute_mapping_transform(feats, feats, 0, 1.0, weights={})
    with pytest.raises(ValueError, match='No posterior'):
        proc.estimate(None, feats, {})
    with pytest.raises(ValueError, match='Posterior has wrong size'):
        proc.estimate(None, feats, {'u': [[(0, 1.0)]]})


def test_snf_vtln_argument_checks():
    L = _backend.lib()
    E = _abi.SNF_E_INVALID
    off = np.array([0, 4], np.int64)
    offp = off.ctypes.data_as(C.c_void_p)
    p = C.c_void_p(16)
    assert L.snf_fmllr_accumulate(0, p, 4, 0, p, p, 2, p, p, 4, offp, 1, p, None) == E
    assert L.snf_fmllr_accumulate(0, p, 4, 65, p, p, 2, p, p, 4, offp, 1, p, None) == E
    assert L.snf_fmllr_accumulate(0, p, 4, 3, p, p, 0, p, p, 4, offp, 1, p, None) == E
    assert L.snf_fmllr_accumulate(0, p, 4, 3, p, p, 2, None, p, 4, offp, 1, p, None) == E
    bad = np.array([0, 3], np.int64)
    assert L.snf_fmllr_accumulate(0, p, 4, 3, p, p, 2, p, p, 4, bad.ctypes.data_as(C.c_void_p), 1, p, None) == E
    dec = np.array([0, 3, 2, 4], np.int64)
    assert L.snf_fmllr_accumulate(0, p, 4, 3, p, p, 2, p, p, 4, dec.ctypes.data_as(C.c_void_p), 3, p, None) == E
    assert L.snf_fmllr_accumulate(0, p, 4, 3, p, p, 2, p, p, 4, None, 1, p, None) == E
    assert L.snf_vtln_gram(0, p, p, None, -1, 3, p, None) == E
    assert L.snf_vtln_gram(0, p, p, None, 4, 3, None, None) == E
    assert L.snf_vtln_gram(0, None, p, None, 4, 3, p, None) == E
    assert L.snf_lvtln_select(0, p, 1, 3, p, p, 2, 3, 0.0, 0, p, p, p, p, p, None) == E
    assert L.snf_lvtln_select(0, p, 1, 3, p, p, 2, 1, 0.0, 2, p, p, p, p, p, None) == E
    assert L.snf_lvtln_select(0, p, 1, 3, p, p, 0, 1, 0.0, 0, p, p, p, p, p, None) == E
    assert L.snf_lvtln_select(0, p, 1, 3, p, p, 2, 1, float('nan'), 0, p, p, p, p, p, None) == E
    assert L.snf_lvtln_select(0, p, 1, 3, None, p, 2, 1, 0.0, 0, p, p, p, p, p, None) == E
    assert L.snf_affine_apply_segments(0, p, 4, 3, bad.ctypes.data_as(C.c_void_p), 1, p, p, None) == E
    assert L.snf_affine_apply_segments(0, p, 4, 0, offp, 1, p, p, None) == E
    assert L.snf_affine_apply_segments(0, None, 4, 3, offp, 1, p, p, None) == E
