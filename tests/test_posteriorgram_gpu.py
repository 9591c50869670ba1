"""Dense GMM posteriors on the GPU (snf_gmm_posteriors through FrameBlock.posteriors and
DiagUbmProcessor.posteriorgrams): every tile seam of frames and Gaussians against the float64 softmax of the
downloaded log-likelihoods, the log-sum-exp against the E-step's bit for bit, every output element written; and end
to end from a wav file to symkl DTW distances between posteriorgrams that never leave the device."""

import numpy as np
import pytest

import gmm_f64 as R
import symkl_cases
from shennong_amd import Utterances, dtw_distances
from shennong_amd import dtw as dtw_module
from shennong_amd import gmm as G
from shennong_amd.device import DeviceFeaturesCollection
from shennong_amd.features import FeaturesCollection
from shennong_amd.postprocessor import DeltaPostProcessor
from shennong_amd.postprocessor.cmvn import SlidingWindowCmvnPostProcessor
from shennong_amd.processor import DiagUbmProcessor, MfccProcessor
from shennong_amd.utils import dict_equal
from test_ubm_gpu import mixture

pytestmark = pytest.mark.gpu

FRAMES = (1, 15, 16, 17, 63, 64, 65, 130)        # around the 16 frames of a wave and the 64 of a tile, 3 tiles
GAUSSIANS = (1, 3, 16, 17, 64, 65, 130)          # around the 16 of an MFMA tile and the block of 64; C % 4 != 0 too
ATOL = 2e-6                                      # the project's figure for selection posteriors (test_ubm_gpu.py)


def _bits(a):
    return np.asarray(a).view(np.uint32)


# ---- 1. shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 13, 39])
def test_posteriors_at_every_seam(gpu, D):
    worst = 0.0
    for F in FRAMES:
        for C in GAUSSIANS:
            x, gmm = mixture(F + 7 * C + D, F, D, C)
            block = G.FrameBlock([x])
            dg = G.DeviceGmm(gmm)
            L = block.loglikes(dg).astype(np.float64)
            want = np.exp(L - R.logsumexp(L, axis=1)[:, None])
            # a poisoned output block: every element must be written
            nbytes = 4 * F * C
            gpu.DeviceBuffer(nbytes).free()
            out = gpu.DeviceBuffer(nbytes)   # (out of the pool: full of NaN bit patterns, the `gpu` fixture)
            assert (out.download(np.zeros(F * C, dtype=np.uint32)) == 0xFFFFFFFF).all()
            same, lse = block.posteriors(dg, out=out, with_lse=True)
            assert same is out
            post = out.download(np.zeros((F, C), dtype=np.float32))
            out.free()
            what = (F, C, D)
            assert not (_bits(post) == 0xFFFFFFFF).any() and np.isfinite(post).all(), what
            worst = max(worst, float(np.abs(post - want).max()))
            assert np.abs(post - want).max() <= ATOL, what
            assert np.abs(post.astype(np.float64).sum(axis=1) - 1).max() <= C * ATOL, what
            assert (post >= 0).all() and (post <= 1).all(), what
            # the log-sum-exp is the E-step's, bit for bit
            _, _, acc_lse = block.accumulate(dg, with_lse=True)
            assert np.array_equal(_bits(lse), _bits(acc_lse)), what
            # ... and the host form returns the same bits
            assert np.array_equal(_bits(block.posteriors(dg)), _bits(post)), what
            if C == 1:
                assert (post == 1).all(), what
    print('D', D, 'worst |posterior - float64 softmax of the device L| %.3g' % worst)


def test_a_mismatched_dimension_and_a_short_output_are_refused(gpu):
    x, gmm = mixture(3, 20, 5, 4)
    block = G.FrameBlock([x[:, :4]])
    with pytest.raises(ValueError, match='Features have dimension 4, the GMM 5'):
        block.posteriors(G.DeviceGmm(gmm))
    block = G.FrameBlock([x])
    with pytest.raises(ValueError, match='bytes'):
        block.posteriors(G.DeviceGmm(gmm), out=gpu.DeviceBuffer(4 * 20 * 4 - 4))


# ---- 2. end to end ------------------------------------------------------------------------------------------------
def test_from_a_wav_file_to_symkl_distances(gpu, wav_file, audio):
    utterances = Utterances([('utt1', wav_file, 'spk1', 0, 1), ('utt2', wav_file, 'spk1', 1, 1.4)])
    ubm = DiagUbmProcessor(8, num_iters_init=10)
    ubm.num_iters = 3
    with pytest.raises(TypeError, match='GMM not initialized'):
        ubm.posteriorgrams(FeaturesCollection())
    ubm.process(utterances)
    assert ubm.gmm.num_gauss() == 8 and ubm.gmm.dim() == 39
    # the features the model was trained on, of the whole file: MFCC + deltas, sliding CMVN
    config = ubm.features
    feats = MfccProcessor(**config['mfcc']).process(audio)
    feats = DeltaPostProcessor(**config['delta']).process(feats)
    feats = SlidingWindowCmvnPostProcessor(**config['sliding_window_cmvn']).process(feats)
    mfcc = FeaturesCollection(utt=feats)
    assert feats.shape == (140, 39)

    host = ubm.posteriorgrams(mfcc)
    assert isinstance(host, FeaturesCollection) and list(host) == ['utt']
    post = host['utt']
    assert post.shape == (140, 8) and post.dtype == np.float32
    assert np.array_equal(post.times, feats.times)
    assert post.properties['posteriorgram'] == {'num_gauss': 8, 'ndims': 39}
    assert dict_equal({k: v for k, v in post.properties.items() if k != 'posteriorgram'}, feats.properties)
    assert 'posteriorgram' not in feats.properties
    # the values are FrameBlock.posteriors' (checked against float64 above).  A model of 8 Gaussians trained on a
    # second of speech puts |lse| near 100, and the float32 lse carries |lse| 2^-24 into every posterior of a frame:
    # measured 7.1e-6 here against the float64 softmax, so only a loose figure is asked of the row sums
    direct = G.FrameBlock([feats.data]).posteriors(G.DeviceGmm(ubm.gmm))
    assert np.array_equal(_bits(post.data), _bits(direct))
    assert np.abs(post.data.astype(np.float64).sum(axis=1) - 1).max() <= 1e-4 and (post.data >= 0).all()

    resident = ubm.posteriorgrams(mfcc, device=True)
    assert isinstance(resident, DeviceFeaturesCollection) and resident['utt'].shape == (140, 8)
    assert np.array_equal(resident['utt'].times, feats.times)
    assert np.array_equal(_bits(resident.to_host()['utt'].data), _bits(post.data))
    source = DeviceFeaturesCollection.from_host(mfcc)
    from_device = ubm.posteriorgrams(source, device=True)
    source.release()
    back = from_device.to_host()
    assert np.array_equal(_bits(back['utt'].data), _bits(post.data))
    assert np.array_equal(back['utt'].times, feats.times) and dict_equal(back['utt'].properties, post.properties)
    from_device.release()
    with pytest.raises(ValueError, match='Features have dimension 13, the GMM 39'):
        ubm.posteriorgrams(FeaturesCollection(utt=MfccProcessor().process(audio)))

    # the two halves of the utterance against each other, on the rows where the kernel wrote them
    items = [('utt', 0.0, 0.7), ('utt', 0.7, 2.0)]
    pairs = np.array([(0, 1), (1, 0)])
    got, got_length = dtw_distances(resident, pairs, items=items, metric='symkl', normalized=False,
                                    return_lengths=True)
    centre = dtw_module._centres(feats.times)
    first, second = post.data[centre <= 0.7], post.data[centre >= 0.7]
    assert first.shape[0] + second.shape[0] == 140 and min(first.shape[0], second.shape[0]) > 32
    for k, (x, y) in enumerate(((first, second), (second, first))):
        cost, length, margin, _, limit = symkl_cases.pair_statement(x, y)
        print('halves', k, 'cost %.6g error %.3g bound %.3g margin %.3g' %
              (cost, abs(float(got[k]) - cost), limit, margin))
        assert abs(float(got[k]) - cost) <= limit
        if margin >= 2 * limit:
            assert got_length[k] == length
    batch = resident.padded()
    assert batch.shape == (1, 140, 8)
    resident.release()
