"""GPU checks of the linear-VTLN kernels (kernels_vtln.hip) and of VtlnProcessor against the float64
statement of tests/lvtln_f64.py"""

import os
import sys

import numpy as np
import pytest
import scipy.io.wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lvtln_f64 as R  # noqa: E402

from shennong_amd import _backend  # noqa: E402
from shennong_amd import gmm as G  # noqa: E402
from shennong_amd import lvtln as LV  # noqa: E402

pytestmark = pytest.mark.gpu


def model(seed, C, D):
    rng = np.random.RandomState(seed)
    gmm = G.DiagGmm(C, D)
    gmm.weights_ = rng.dirichlet(np.ones(C)).astype(np.float32)
    gmm.inv_vars_ = (1.0 / rng.uniform(0.5, 2.0, (C, D))).astype(np.float32)
    gmm.means_invvars_ = (rng.randn(C, D) * gmm.inv_vars_).astype(np.float32)
    gmm.compute_gconsts()
    return gmm


def selection(seed, F, n, C):
    rng = np.random.RandomState(seed)
    sel = np.stack([rng.choice(C, n, replace=False) for _ in range(F)]) if F else np.zeros((0, n), int)
    post = rng.dirichlet(np.ones(n), size=F).astype(np.float32) if F else np.zeros((0, n), np.float32)
    if F and n > 1:
        post[rng.rand(F, n) < 0.2] = 0.0      # pruned entries
    return sel.astype(np.int32), post


def device_stats(x, sel, post, gmm, offsets):
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    dsel = block.upload_selection(sel) if len(x) else _backend.DeviceBuffer(16)
    dpost = _backend.upload_rows([post], np.float32) if len(x) else _backend.DeviceBuffer(16)
    buf = LV.fmllr_accumulate(block, dg, dsel, dpost, sel.shape[1], offsets)
    return LV.download_stats(buf, len(offsets) - 1, x.shape[1])


def check_stats(got, x, sel, post, gmm, offsets):
    D = x.shape[1]
    for s in range(len(offsets) - 1):
        a, b = offsets[s], offsets[s + 1]
        beta, K, Gm = R.fmllr_stats(x[a:b], sel[a:b], post[a:b], gmm.means_invvars_, gmm.inv_vars_)
        st = LV.FmllrStats.from_device_layout(got[s])
        # scale of every term: the same sums over absolute values
        _, Ks, Gs = R.fmllr_stats(np.abs(x[a:b]), sel[a:b], post[a:b], np.abs(gmm.means_invvars_), gmm.inv_vars_)
        assert abs(st.beta - beta) <= 1e-11 * max(1.0, beta)
        assert np.all(np.abs(st.K - K) <= 1e-11 * (Ks + 1e-300)), s
        assert np.all(np.abs(st.G - Gm) <= 1e-11 * (Gs + 1e-300)), s
        assert st.G.shape == (D, D + 1, D + 1)


@pytest.mark.parametrize('D', [1, 2, 13, 39, 40, 60])
@pytest.mark.parametrize('n,C', [(1, 2), (2, 64), (15, 2048)])
def test_fmllr_stats(gpu, D, n, C):
    if n > C:
        pytest.skip('n > C')
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 0, 3000] if D in (13, 39) else [0, 1, 17, 64, 65, 0]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    F = int(offsets[-1])
    rng = np.random.RandomState(D * 100 + n)
    x = (rng.randn(F, D) * 3 + 1).astype(np.float32)
    gmm = model(D + n + C, C, D)
    sel, post = selection(D + C, F, n, C)
    got = device_stats(x, sel, post, gmm, offsets)
    check_stats(got, x, sel, post, gmm, offsets)
    again = device_stats(x, sel, post, gmm, offsets)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


def test_fmllr_stats_long_and_many_segments(gpu):
    D, n, C = 39, 15, 64
    lens = [10000] + [int(v) for v in np.random.RandomState(1).randint(0, 40, 3000)]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    F = int(offsets[-1])
    x = np.random.RandomState(2).randn(F, D).astype(np.float32)
    gmm = model(3, C, D)
    sel, post = selection(4, F, n, C)
    got = device_stats(x, sel, post, gmm, offsets)
    pick = [0, 1, 2, 500, 1777, 3000]
    for s in pick:
        o = offsets[s:s + 2]
        check_stats(got[s:s + 1], x[o[0]:o[1]], sel[o[0]:o[1]], post[o[0]:o[1]], gmm, o - o[0])


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('D', [1, 13, 39, 60])
def test_gram_and_mapping_transform(gpu, D, weighted):
    from shennong_amd.features import Features, FeaturesCollection
    from shennong_amd.processor.vtln import VtlnProcessor
    rng = np.random.RandomState(D)
    lens = [50, 3000, 7]
    xs = [rng.randn(m, D).astype(np.float32) for m in lens]
    M = rng.randn(D, D) * 0.2 + np.eye(D)
    ys = [(x @ M.T + 0.5 + 0.1 * rng.randn(*x.shape)).astype(np.float32) for x in xs]
    ws = [rng.rand(m).astype(np.float32) for m in lens] if weighted else None
    dx, dy = _backend.upload_rows(xs, np.float32), _backend.upload_rows(ys, np.float32)
    dw = _backend.upload_rows(ws, np.float32) if weighted else None
    gram = LV.vtln_gram(dx, dy, sum(lens), D, dw)
    x, y = np.concatenate(xs).astype(np.float64), np.concatenate(ys).astype(np.float64)
    w = np.concatenate(ws).astype(np.float64) if weighted else np.ones(len(x))
    z = np.concatenate([x, np.ones((len(x), 1)), y], axis=1)
    want = (z * w[:, None]).T @ z
    scale = (np.abs(z) * w[:, None]).T @ np.abs(z)
    assert np.all(np.abs(gram - want) <= 1e-12 * scale)
    vt = VtlnProcessor()
    vt.lvtln = LV.LinearVtln(D, 3, 1)
    fx = FeaturesCollection({f'u{i}': Features(a, np.arange(len(a)) * 0.01, validate=False) for i, a in enumerate(xs)})
    fy = FeaturesCollection({f'u{i}': Features(a, np.arange(len(a)) * 0.01, validate=False) for i, a in enumerate(ys)})
    weights = {f'u{i}': a for i, a in enumerate(ws)} if weighted else None
    vt.compute_mapping_transform(fx, fy, 2, 1.07, weights=weights)
    np.testing.assert_allclose(vt.lvtln.get_transform(2), R.mapping_transform(x, y, w), rtol=1e-5, atol=1e-5)
    assert vt.lvtln.get_warp(2) == pytest.approx(1.07)


def class_setup(D, C, S, seed):
    rng = np.random.RandomState(seed)
    As = [(np.eye(D) + 0.05 * rng.randn(D, D)).astype(np.float32) for _ in range(C)]
    lvtln = LV.LinearVtln(D, C, C // 2)
    for c, A in enumerate(As):
        lvtln.set_transform(c, A)
    gmm = model(seed, 32, D)
    lens = [0] + [int(v) for v in rng.randint(20, 400, S - 1)]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    F = int(offsets[-1])
    x = (rng.randn(F, D) * 1.5).astype(np.float32)
    sel, post = selection(seed + 1, F, 5, 32)
    return lvtln, gmm, x, sel, post, offsets


@pytest.mark.parametrize('norm_type', ['none', 'offset', 'diag'])
@pytest.mark.parametrize('logdet_scale', [0.0, 0.5, 1.0])
def test_class_search(gpu, norm_type, logdet_scale):
    D, C, S = 13, 9, 12
    lvtln, gmm, x, sel, post, offsets = class_setup(D, C, S, 7)
    block = G.FrameBlock([x])
    dsel = block.upload_selection(sel)
    dpost = _backend.upload_rows([post], np.float32)
    stats = LV.fmllr_accumulate(block, G.DeviceGmm(gmm), dsel, dpost, 5, offsets)
    dl = LV.DeviceLvtln(lvtln)
    objf, cls, impr, count, dtrans = dl.select(stats, S, norm_type, logdet_scale)
    trans = dtrans.download(np.empty((S, D, D + 1), np.float32))
    host = LV.download_stats(stats, S, D)
    for s in range(S):
        st = LV.FmllrStats.from_device_layout(host[s])
        objs, best, imp, cnt, W = R.compute_transform(lvtln.A, lvtln.logdets, (st.beta, st.K, st.G), norm_type,
                                                      logdet_scale, lvtln.default_class)
        if st.beta == 0:
            assert cls[s] == lvtln.default_class and impr[s] == 0 and count[s] == 0
            np.testing.assert_array_equal(trans[s][:, :D], lvtln.A[lvtln.default_class])
            assert np.all(trans[s][:, D] == 0)
            continue
        np.testing.assert_allclose(objf[s], objs, rtol=1e-10)
        assert cls[s] == int(np.argmax(objf[s]))
        assert count[s] == pytest.approx(st.beta, rel=1e-12)
        W = R.compute_transform([lvtln.A[cls[s]]], [lvtln.logdets[cls[s]]], (st.beta, st.K, st.G), norm_type,
                                logdet_scale, 0)[4]
        np.testing.assert_allclose(trans[s], W, atol=1e-6, rtol=1e-6)
        np.testing.assert_allclose(impr[s], objf[s][cls[s]] - R.aux(np.eye(D, D + 1), (st.beta, st.K, st.G)),
                                   rtol=1e-9, atol=1e-9 * abs(objf[s][cls[s]]))


def test_affine_apply(gpu):
    D = 39
    rng = np.random.RandomState(5)
    offsets = np.array([0, 10, 10, 333, 400], np.int64)
    x = rng.randn(400, D).astype(np.float32)
    W = rng.randn(4, D, D + 1).astype(np.float32)
    block = G.FrameBlock([x])
    dW = _backend.DeviceBuffer(W.nbytes)
    dW.upload(W)
    y = LV.affine_apply_segments(block, offsets, dW).download(np.empty((400, D), np.float32))
    for s in range(4):
        a, b = offsets[s], offsets[s + 1]
        want = x[a:b] @ W[s][:, :D].T + W[s][:, D]
        np.testing.assert_allclose(y[a:b], want, rtol=1e-5, atol=1e-4)


def test_estimate_forms_and_keys(gpu):
    from shennong_amd.features import Features, FeaturesCollection
    from shennong_amd.processor.ubm import DiagUbmProcessor
    from shennong_amd.processor.vtln import VtlnProcessor
    D, C = 13, 5
    lvtln, gmm, _, _, _, _ = class_setup(D, C, 4, 11)
    lens = [100, 0, 250, 80]
    offs = np.concatenate([[0], np.cumsum(lens)])
    x = np.random.RandomState(12).randn(offs[-1], D).astype(np.float32)
    sel, post = selection(13, offs[-1], 5, 32)
    utts = [f'u{i}' for i in range(4)]
    coll = FeaturesCollection({u: Features(x[offs[i]:offs[i + 1]], np.arange(lens[i]) * 0.01, validate=False)
                               for i, u in enumerate(utts)})
    arrays = {u: (sel[offs[i]:offs[i + 1]], post[offs[i]:offs[i + 1]]) for i, u in enumerate(utts)}
    lists = {u: [[(int(g), float(p)) for g, p in zip(sr, pr) if p != 0] for sr, pr in zip(*arrays[u])]
             for u in utts}
    ubm = DiagUbmProcessor(32)
    ubm.gmm = gmm
    vt = VtlnProcessor()
    vt.lvtln = lvtln
    t1, w1 = vt.estimate(ubm, coll, lists)
    t2, w2 = vt.estimate(ubm, coll, arrays)
    assert list(t1) == utts and w1 == w2
    for u in utts:
        np.testing.assert_array_equal(t1[u], t2[u])
    assert w1['u1'] == lvtln.get_warp(lvtln.default_class)
    t3, w3 = vt.estimate(ubm, coll, lists, utt2speak={'u0': 'a', 'u1': 'b', 'u2': 'a', 'u3': 'c'})
    assert sorted(t3) == ['a', 'b', 'c'] and t3['a'].shape == (D, D + 1)


def wavs(tmp_path, wav_file):
    rate, data = scipy.io.wavfile.read(wav_file)
    f32 = str(tmp_path / 'test.f32.wav')
    scipy.io.wavfile.write(f32, rate, (data / 2 ** 15).astype(np.float32))
    return f32, os.path.join(os.path.dirname(wav_file), 'test.8k.wav')


@pytest.mark.parametrize('by_speaker', [True, False])
def test_process_reference(gpu, tmp_path, wav_file, by_speaker):
    """The reference's test_process / test_process_no_speaker: mixed 16 kHz, float32 and 8 kHz audio"""
    from shennong_amd import Utterances
    from shennong_amd.processor.vtln import VtlnProcessor
    f32, wav8 = wavs(tmp_path, wav_file)
    utts = Utterances([('utt1', wav_file, 'spk1', 0, 1.2), ('utt2', f32, 'spk1', 0.1, 1.4),
                       ('utt3', wav8, 'spk2', 0, 1.3)] if by_speaker else
                      [('utt1', wav_file, 0, 1.2), ('utt2', f32, 0.1, 1.4), ('utt3', wav8, 0, 1.3)])
    proc = VtlnProcessor(min_warp=0.95, max_warp=1.05, num_iters=1, by_speaker=by_speaker)
    proc.ubm = {'num_gauss': 4, 'num_iters_init': 1, 'num_iters': 1, 'num_frames': 100,
                'vad': {'energy_threshold': 0}}
    warps = proc.process(utts)
    assert sorted(warps) == ['utt1', 'utt2', 'utt3']
    assert all(0.95 - 1e-6 <= w <= 1.05 + 1e-6 for w in warps.values())
    if by_speaker:
        assert warps['utt1'] == warps['utt2']
        spk = proc.process(utts, group_by='speaker')
        assert sorted(spk) == ['spk1', 'spk2']
        path = str(tmp_path / 'warps.yml')
        proc.save_warps(path)
        assert VtlnProcessor.load_warps(path) == proc.warps
        model = str(tmp_path / 'lvtln.ark')
        proc.save(model)
        assert VtlnProcessor.load(model).lvtln.num_classes() == 11
    else:
        with pytest.raises(ValueError, match='group warps by speaker'):
            proc.process(utts, group_by='speaker')


def synth_corpus(tmp_path, speakers=4, per=3):
    from shennong_amd import Utterances, synth
    rows = []
    for s in range(speakers):
        waves = synth.utterances(100 * s, per, nsamples=24000)
        for u, w in enumerate(waves):
            path = str(tmp_path / f's{s}_{u}.wav')
            scipy.io.wavfile.write(path, 16000, w)
            rows.append((f's{s}_u{u}', path, f'spk{s}'))
    return Utterances(rows)


def test_end_to_end_against_replay(gpu, tmp_path):
    """process() with a given UBM against the fp64 replay of its loop from the same frames, selection
    and UBM (the replay's E-step / posteriors are the device ones, so only the VTLN part is restated)"""
    from shennong_amd.processor.ubm import DiagUbmProcessor
    from shennong_amd.processor.vtln import VtlnProcessor
    utts = synth_corpus(tmp_path)
    ubm = DiagUbmProcessor(8, num_iters_init=4, num_iters=2, vad={'energy_threshold': 0})
    ubm.process(utts)
    gmm0 = ubm.gmm.copy()
    proc = VtlnProcessor(min_warp=0.9, max_warp=1.1, warp_step=0.02, num_iters=2)
    captured = {}
    orig_estimate = proc._estimate_device

    def spy(ubm_, block, dsel, dpost, width, offsets, keys, what='speaker'):
        if 'x' not in captured:
            captured['x'] = block.frames.download(np.empty((block.nframes, block.dim), np.float32))
            captured['sel'] = dsel.download(np.empty((block.nframes, width), np.int32))
            captured['offsets'] = np.asarray(offsets).copy()
        return orig_estimate(ubm_, block, dsel, dpost, width, offsets, keys, what)

    proc._estimate_device = spy
    proc.process(utts, ubm=ubm, group_by='speaker')
    x, sel, off = captured['x'], captured['sel'], captured['offsets']
    segs = [slice(off[s], off[s + 1]) for s in range(len(off) - 1)]

    def posteriors(gmm, frames, s):
        b = G.FrameBlock([np.asarray(frames, np.float32)])
        return b.selection_posteriors(G.DeviceGmm(gmm), s)[0]

    def em_step(gmm, frames):
        stats, _, _ = G.FrameBlock([frames]).accumulate(G.DeviceGmm(gmm))
        G.mle_diag_gmm_update(G.AccumDiagGmm.from_stats(stats), gmm, ubm._options)

    res = R.replay([x[s] for s in segs], [sel[s] for s in segs], gmm0, proc.lvtln.A, proc.lvtln.warps,
                   'offset', 0.0, proc.lvtln.default_class, 2, em_step, posteriors)
    spks = sorted({u.speaker for u in utts})
    for s, (objs, best, _, _, W) in enumerate(res):
        top = np.sort(objs)[-2:]
        assert top[1] - top[0] > 1e-6 * abs(top[1])
        spk = spks[s]
        utt = [u.name for u in utts if u.speaker == spk][0]
        assert proc.warps[utt] == proc.lvtln.get_warp(best)
        np.testing.assert_allclose(proc.transforms[utt], W, atol=1e-4, rtol=1e-4)


def test_hand_off_to_extract_features(gpu, tmp_path):
    from shennong_amd import pipeline
    from shennong_amd.processor.vtln import VtlnProcessor
    utts = synth_corpus(tmp_path, speakers=2, per=2)
    proc = VtlnProcessor(min_warp=0.95, max_warp=1.05, num_iters=1)
    proc.ubm = {'num_gauss': 4, 'num_iters_init': 2, 'num_iters': 1, 'vad': {'energy_threshold': 0}}
    warps = proc.process(utts, group_by='speaker')
    config = pipeline.get_default_config('mfcc', with_cmvn=False)
    config['mfcc']['dither'] = 0
    got = pipeline.extract_features(config, utts, warps=warps)
    per_utt = {u.name: warps[u.speaker] for u in utts}
    want = pipeline.extract_features(config, utts, warps=per_utt)
    for u in utts:
        np.testing.assert_array_equal(got[u.name].data, want[u.name].data)
