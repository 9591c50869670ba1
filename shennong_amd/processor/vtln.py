"""Extraction of VTLN warp factors from utterances.

Linear Vocal Tract Length Normalization after Kaldi's LinearVtln, as the reference's processor/vtln.py
trains it, with the same parameters, defaults, checks and messages.  Where the reference loops over
frames with pykaldi objects, this one runs HIP kernels (``kernels_vtln.hip``): the weighted Gram of the
mapping transforms, the fMLLR statistics of every speaker (or utterance), the search over the warp
classes and the per-speaker affine transform of the frames.  The UBM's E-step, selection and posteriors
are those of :class:`~shennong_amd.processor.ubm.DiagUbmProcessor`.

Examples
--------

>>> from shennong_amd import Utterances
>>> from shennong_amd.processor.vtln import VtlnProcessor
>>> wav = './tests/golden/test.wav'
>>> utterances = Utterances(
...     [('utt1', wav, 'spk1', 0, 1), ('utt2', wav, 'spk1', 1, 1.4)])
>>> vtln = VtlnProcessor(min_warp=0.95, max_warp=1.05, ubm={'num_gauss': 4})
>>> vtln.num_iters = 10
>>> warps = vtln.process(utterances)                          # doctest: +SKIP

The warps go to ``extract_features(config, utterances, warps=warps)`` or to a processor's ``process(...,
vtln_warp=...)``.  A ``vtln`` entry in the pipeline configuration (``config['vtln'] = VtlnProcessor().get_params()``)
has ``extract_features`` train them with this class and extract with them.

The mapping transforms take one warped extraction per class.  When the corpus fits one device batch, they run
as a device-resident sweep (:meth:`VtlnProcessor._mapping_sweep`): the audio goes up once, every class's
features stay in HBM and the Grams gather their rows there.  The results are bit for bit those of the host
round trip, which larger corpora keep.

Divergences from the reference
------------------------------
- A speaker (or utterance) with no voiced frames gets the default class, the default warp and the
  transform ``[A_default | 0]``; the reference's debug line divides by its zero count and raises
  ZeroDivisionError.
- fMLLR statistics: every frame is counted, and the per-frame sums ``a_f``, ``b_f`` are float64 where
  Kaldi keeps them in float (see ``kernels_vtln.hip``).  The class objectives are float64 on the float64
  composed transform; the logdet_scale reading is stated in :mod:`shennong_amd.lvtln`.
- Within one speaker the frames are taken utterance after utterance in the order of ``utt2speak``.
"""

import copy
import os

import numpy as np
import yaml

from shennong_amd import _backend
from shennong_amd import gmm as _gmm
from shennong_amd import lvtln as _lvtln
from shennong_amd import pipeline
from shennong_amd.base import BaseProcessor
from shennong_amd.features import FeaturesCollection
from shennong_amd.logger import null_logger
from shennong_amd.postprocessor.cmvn import SlidingWindowCmvnPostProcessor
from shennong_amd.postprocessor.vad import VadPostProcessor
from shennong_amd.processor.ubm import DiagUbmProcessor
from shennong_amd.utils import get_njobs


def mapping_from_gram(M, dim):
    """The variance-normalised least-squares map of reference vtln.py:344-376 from the Gram
    ``M = sum_f w_f z_f z_f^T``, z = [x | 1 | y] (float64): A [dim, dim] float32.  Also returns, per
    dimension, (error, sqdiff, scatter) for the debug line."""
    D = dim
    Q = M[:D + 1, :D + 1]
    l = M[D + 1:, :D + 1]
    c = np.diag(M)[D + 1:]
    beta = M[D, D]
    sum_xplus = M[D, :D + 1]
    sumsq_x = np.diag(M)[:D]
    sumsq_diff = np.diag(M)[:D] + c - 2.0 * np.diag(M[:D, D + 1:])
    Qinv = np.linalg.inv(Q)
    W = l @ Qinv.T                      # rows w_i = Qinv l_i
    QW = W @ Q                          # rows Q w_i (Q symmetric)
    wQw = np.sum(QW * W, axis=1)
    error = (wQw - 2.0 * np.sum(W * l, axis=1) + c) / beta
    x_var = sumsq_x / beta - (sum_xplus[:D] / beta) ** 2
    y_var = wQw / beta - (W @ sum_xplus / beta) ** 2
    scale = np.sqrt(x_var / y_var)
    A = (W[:, :D] * scale[:, None]).astype(np.float32)
    return A, (error, sumsq_diff / beta, sumsq_x / beta)


def _sweep_on_device(utterances):
    """True when the mapping transforms take the device-resident sweep (the audio, every class's features and
    the row list stay in HBM); False - a corpus that does not fit one device batch - keeps the per-class host
    round trip (extract_features_warp, trim, subsample, upload)"""
    return not pipeline._too_large_for_one_batch(utterances)


def sweep_rows(names, vad, subsample, layout):
    """The records of the mapping Gram as (block [F] int32, row [F] int64): per utterance of `names` in order,
    ``np.flatnonzero(vad[u])[::subsample]`` - the rows ``FeaturesCollection.trim(vad)`` then ``[::subsample]``
    keeps - offset to where the frames of u start in its block, ``layout[u] = (block, first row)``"""
    blocks, rows = [], []
    for name in names:
        block, first = layout[name]
        keep = np.flatnonzero(vad[name])[::subsample]
        rows.append(keep + first)
        blocks.append(np.full(keep.size, block, dtype=np.int32))
    if not rows:
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    return np.concatenate(blocks).astype(np.int32), np.concatenate(rows).astype(np.int64)


class VtlnProcessor(BaseProcessor):
    """VTLN model"""
    name = 'vtln'

    def __init__(self, num_iters=15, min_warp=0.85,
                 max_warp=1.25, warp_step=0.01,
                 logdet_scale=0.0, norm_type='offset',
                 subsample=5, features=None,
                 ubm=None, by_speaker=True):
        super().__init__()
        self.num_iters = num_iters
        self.min_warp = min_warp
        self.max_warp = max_warp
        self.warp_step = warp_step
        self.logdet_scale = logdet_scale
        self.norm_type = norm_type
        self.subsample = subsample
        self.by_speaker = by_speaker

        if features in (None, 'default'):
            config = pipeline.get_default_config('mfcc', with_delta=True)
            config['sliding_window_cmvn'] = SlidingWindowCmvnPostProcessor().get_params()
            config['sliding_window_cmvn']['cmn_window'] = 300
            config['delta']['window'] = 3
            self.features = config
        else:
            self.features = features

        if ubm is None:
            default_num_gauss = 64
            self.ubm = DiagUbmProcessor(default_num_gauss).get_params()
        else:
            self.ubm = ubm

        self.lvtln = None
        self.transforms = None
        self.warps = None

    # ---- parameters (reference vtln.py:104-207)
    @property
    def num_iters(self):
        """Number of iterations of training"""
        return self._num_iters

    @num_iters.setter
    def num_iters(self, value):
        self._num_iters = int(value)

    @property
    def min_warp(self):
        """Minimum warp considered"""
        return self._min_warp

    @min_warp.setter
    def min_warp(self, value):
        self._min_warp = float(value)

    @property
    def max_warp(self):
        """Maximum warp considered"""
        return self._max_warp

    @max_warp.setter
    def max_warp(self, value):
        self._max_warp = float(value)

    @property
    def warp_step(self):
        """Warp step"""
        return self._warp_step

    @warp_step.setter
    def warp_step(self, value):
        self._warp_step = float(value)

    @property
    def logdet_scale(self):
        """Scale on log-determinant term in auxiliary function"""
        return self._logdet_scale

    @logdet_scale.setter
    def logdet_scale(self, value):
        self._logdet_scale = float(value)

    @property
    def norm_type(self):
        """Type of fMLLR applied (``offset``, ``none`` or ``diag``)"""
        return self._norm_type

    @norm_type.setter
    def norm_type(self, value):
        if value not in ['offset', 'none', 'diag']:
            raise ValueError('Invalid norm type {}'.format(value))
        self._norm_type = value

    @property
    def subsample(self):
        """When computing base LVTLN transforms, use every n frames
         (a speedup)"""
        return self._subsample

    @subsample.setter
    def subsample(self, value):
        self._subsample = int(value)

    @property
    def by_speaker(self):
        """Compute the warps for each speaker, or each utterance"""
        return self._by_speaker

    @by_speaker.setter
    def by_speaker(self, value):
        self._by_speaker = bool(value)

    @property
    def features(self):
        """Features extraction configuration"""
        return self._features

    @features.setter
    def features(self, value):
        if not isinstance(value, dict):
            raise TypeError('Features extraction configuration must be a dict')
        if 'mfcc' not in value:
            raise ValueError('Need mfcc features to train VTLN model')
        self._features = copy.deepcopy(value)

    @property
    def ubm(self):
        "Diagonal UBM-GMM configuration"
        return self._ubm

    @ubm.setter
    def ubm(self, value):
        if not isinstance(value, dict):
            raise TypeError('UBM configuration must be a dict')
        ubm_keys = DiagUbmProcessor(2).get_params().keys()
        if not value.keys() <= ubm_keys:
            raise ValueError('Unknown parameters given for UBM config')
        self._ubm = copy.deepcopy(value)

    # ---- files (reference vtln.py:209-260)
    @classmethod
    def load(cls, path):
        """Load the LVTLN from a binary file"""
        if not os.path.isfile(path):
            raise OSError('{}: file not found'.format(path))
        vtln = VtlnProcessor()
        with open(path, 'rb') as stream:
            vtln.lvtln = _lvtln.LinearVtln.from_bytes(stream.read())
        return vtln

    @classmethod
    def load_warps(cls, path):
        """Load precomputed warps"""
        if not os.path.isfile(path):
            raise OSError('{}: file not found'.format(path))
        try:
            with open(path, 'r') as stream:
                warps = yaml.load(stream, Loader=yaml.FullLoader)
        except yaml.YAMLError as err:  # pragma: nocover
            raise ValueError('Error in VTLN warps file when loading: {}'.format(err))
        return warps

    def save(self, path):
        """Save the LVTLN to a binary file"""
        if os.path.isfile(path):
            raise OSError('{}: file already exists'.format(path))
        if not isinstance(self.lvtln, _lvtln.LinearVtln):
            raise TypeError('VTLN not initialized')
        with open(path, 'wb') as stream:
            stream.write(self.lvtln.to_bytes())

    def save_warps(self, path):
        """Save the computed warps"""
        if os.path.isfile(path):
            raise OSError('{}: file already exists'.format(path))
        if not isinstance(self.warps, dict):
            raise TypeError('Warps not computed')
        try:
            with open(path, 'w') as stream:
                yaml.dump(self.warps, stream)
        except yaml.YAMLError as err:  # pragma: nocover
            raise ValueError('Error in VTLN warps file when saving: {}'.format(err))

    def _check_lvtln(self):
        if not isinstance(self.lvtln, _lvtln.LinearVtln):
            raise TypeError('VTLN not initialized')

    # ---- mapping transforms (reference vtln.py:262-376)
    def compute_mapping_transform(self, feats_untransformed, feats_transformed, class_idx, warp, weights=None):
        """Set one of the transforms in lvtln to the minimum-squared-error solution to mapping
        feats_untransformed to feats_transformed; weights may optionally be used to downweight/remove
        silence (Kaldi gmm-train-lvtln-special).  The sums are one weighted Gram on the GPU.

        Raises
        ------
        ValueError
            If the features have unconsistent dimensions, or a key has no transformed features or
            no weights.
        """
        self._check_lvtln()
        dim = self.lvtln.dim()
        xs, ys, ws = [], [], []
        for utt in feats_untransformed:
            if utt not in feats_transformed:
                raise ValueError(f'No transformed features for key {utt}')
            x = feats_untransformed[utt].data
            y = feats_transformed[utt].data
            if x.shape[0] != y.shape[0] or x.shape[1] != y.shape[1] or x.shape[1] != dim:
                raise ValueError('Number of rows and/or columns differs: '
                                 f'{x.shape[0]} vs {y.shape[0]} '
                                 f'rows, {x.shape[1]} vs '
                                 f'{y.shape[1]} columns, {dim} dim')
            if weights is not None:
                if utt not in weights:
                    raise ValueError(f'No weights for utterance {utt}')
                ws.append(np.asarray(weights[utt], dtype=np.float32).reshape(-1))
            xs.append(x)
            ys.append(y)
        dx = _backend.upload_rows(xs, np.float32) if xs else None
        dy = _backend.upload_rows(ys, np.float32) if ys else None
        dw = _backend.upload_rows(ws, np.float32) if weights is not None and ws else None
        nframes = sum(x.shape[0] for x in xs)
        self._mapping_from_device(dx, dy, dw, nframes, class_idx, warp)

    def _mapping_from_device(self, dx, dy, dw, nframes, class_idx, warp):
        self._mapping_from_gram(_lvtln.vtln_gram(dx, dy, nframes, self.lvtln.dim(), dw), class_idx, warp)

    def _mapping_from_gram(self, M, class_idx, warp):
        dim = self.lvtln.dim()
        A, (error, sqdiff, scatter) = mapping_from_gram(M, dim)
        for i in range(dim):
            self.log.debug(
                'For dimension %s sum-squared error in linear approximation '
                'is %s, versus feature-difference %s, orig-sumsq is %s',
                i, error[i], sqdiff[i], scatter[i])
        self.lvtln.set_transform(class_idx, A)
        self.lvtln.set_warp(class_idx, warp)

    # ---- transforms (reference vtln.py:378-509)
    @staticmethod
    def _posterior_arrays(utt, post, nrows):
        """(selection [F, n] int32, posteriors [F, n] float32) of the reference's list form or of an array
        pair; pruned or missing entries have posterior 0"""
        if isinstance(post, tuple) and len(post) == 2 and isinstance(post[0], np.ndarray):
            sel, p = post
            if sel.shape[0] != nrows:
                raise ValueError(f'Posterior has wrong size {sel.shape[0]} vs {nrows}')
            sel, p = np.asarray(sel, np.int32), np.asarray(p, np.float32)
            width = sel.shape[1] if sel.ndim == 2 else max(1, sel.size // max(1, nrows))
            return sel.reshape(nrows, width), p.reshape(nrows, width)
        if len(post) != nrows:
            raise ValueError(f'Posterior has wrong size {len(post)} vs {nrows}')
        width = max([len(row) for row in post] + [1])
        sel = np.zeros((nrows, width), np.int32)
        p = np.zeros((nrows, width), np.float32)
        for i, row in enumerate(post):
            for j, (g, v) in enumerate(row):
                sel[i, j] = g
                p[i, j] = v
        return sel, p

    def estimate(self, ubm, feats_collection, posteriors, utt2speak=None):
        """Estimate linear-VTLN transforms, either per utterance or for the supplied set of speakers
        (``utt2speak``), from posteriors over the UBM's Gaussians (Kaldi gmm-global-est-lvtln-trans).

        Parameters
        ----------
        ubm : DiagUbmProcessor
        feats_collection : FeaturesCollection
            The untransformed features.
        posteriors : dict[str, list[list[tuple[int, float]]]]
            For every utterance and frame, (Gaussian, posterior) pairs.  An utterance may instead map to
            an array pair ``(selection [F, n] int32, posteriors [F, n] float32)``: the same result.
        utt2speak : dict[str, str], optional

        Returns
        -------
        transforms : dict[str, ndarray]  float32 [D, D+1] per speaker (or utterance)
        warps : dict[str, float]
        """
        self._check_lvtln()
        if utt2speak is not None:
            groups = {spk: list(part.keys()) for spk, part in feats_collection.partition(utt2speak).items()}
        else:
            groups = {utt: [utt] for utt in feats_collection}
        keys, mats, sels, posts, offsets = [], [], [], [], [0]
        for key, utts in groups.items():
            for utt in utts:
                if utt not in posteriors:
                    raise ValueError(f'No posterior for utterance {utt}')
                data = feats_collection[utt].data
                sel, p = self._posterior_arrays(utt, posteriors[utt], data.shape[0])
                mats.append(data)
                sels.append(sel)
                posts.append(p)
            keys.append(key)
            offsets.append(offsets[-1] + sum(feats_collection[u].nframes for u in utts))
        width = max([s.shape[1] for s in sels] + [1])
        pad = [(np.pad(s, ((0, 0), (0, width - s.shape[1]))), np.pad(p, ((0, 0), (0, width - p.shape[1]))))
               for s, p in zip(sels, posts)]
        dim = self.lvtln.dim()
        if not mats:
            return {}, {}
        block = _gmm.FrameBlock([np.asarray(m, np.float32).reshape(-1, dim) for m in mats])
        if block.nframes:
            dsel = block.upload_selection(np.concatenate([s for s, _ in pad], axis=0))
            dpost = _backend.upload_rows([p for _, p in pad], np.float32, block.device)
        else:
            dsel = dpost = _backend.DeviceBuffer(16, block.device)
        transforms, warps, _ = self._estimate_device(ubm, block, dsel, dpost, width, np.asarray(offsets), keys)
        return transforms, warps

    def _estimate_device(self, ubm, block, dsel, dpost, width, offsets, keys, what='speaker'):
        """Statistics, class search and transforms of every segment (frames offsets[s] .. offsets[s+1]
        of `block`); the statistics go through HBM in batches of at most lvtln.STATS_BYTES_BOUND bytes.
        Returns (transforms, warps, transforms [S, D, D+1] float32)."""
        dgmm = _gmm.DeviceGmm(ubm.gmm, block.device)
        dl = _lvtln.DeviceLvtln(self.lvtln, block.device)
        dim = self.lvtln.dim()
        S = len(keys)
        per = _lvtln.segments_per_call(dim)
        all_cls = np.zeros(S, np.int32)
        all_impr = np.zeros(S, np.float64)
        all_count = np.zeros(S, np.float64)
        all_trans = np.zeros((S, dim, dim + 1), np.float32)
        for first in range(0, S, per):
            last = min(S, first + per)
            stats = _lvtln.fmllr_accumulate(block, dgmm, dsel, dpost, width, offsets, first, last)
            _, cls, impr, count, dtrans = dl.select(stats, last - first, self.norm_type, self.logdet_scale)
            all_cls[first:last], all_impr[first:last], all_count[first:last] = cls, impr, count
            all_trans[first:last] = dtrans.download(np.empty((last - first, dim, dim + 1), np.float32))
        transforms, warps = {}, {}
        class_counts = np.zeros(self.lvtln.num_classes())
        for s, key in enumerate(keys):
            c = int(all_cls[s])
            class_counts[c] += 1
            transforms[key] = all_trans[s].copy()
            warps[key] = self.lvtln.get_warp(c)
            self.log.debug('%s %s: auxf-impr from LVTLN is %s, over %s frames', what, key,
                           all_impr[s] / all_count[s] if all_count[s] else 0.0, all_count[s])
        tot_t = float(all_count.sum())
        message = 'Distribution of classes is'
        for count in class_counts:
            message += ' ' + str(count)
        message += (f', overall LVTLN auxfimpr per frame is '
                    f'{float(all_impr.sum()) / tot_t if tot_t else 0.0}  over {tot_t} frames')
        self.log.debug(message)
        return transforms, warps, all_trans

    # ---- base transforms (reference vtln.py:553-610)
    def _base_transforms(self, utterances, ubm, num_classes, njobs=1, stats=None):
        """Features with the sliding CMVN popped, VAD on the raw features, CMVN, trim and subsample: returns the
        original frames.  Sets the mapping transform of every class on the way: one warped extraction per
        class, on the device (:meth:`_mapping_sweep`) unless the corpus does not fit one device batch.
        `stats` (a pipeline.RunStats) counts the link bytes and kernel time of the device sweep."""
        cmvn_config = self.features.pop('sliding_window_cmvn', None)
        waves = None
        try:
            if _sweep_on_device(utterances):
                # the unwarped pass keeps its audio in HBM for the warped ones
                get_njobs(njobs, log=null_logger())
                config = pipeline._init_config(self.features, log=null_logger())
                waves = pipeline._SweepWaves()
                raw_mfcc = pipeline._extract_features(config, pipeline._view_of(utterances), None, null_logger(),
                                                      resident=waves, stats=stats)
            else:
                raw_mfcc = pipeline.extract_features(self.features, utterances, njobs=njobs, log=null_logger())
            self.log.debug('... computing VAD decision')
            utts = list(raw_mfcc.keys())
            decisions = VadPostProcessor(**ubm.vad)._process_batch([raw_mfcc[u] for u in utts])
            vad = {u: d.data.reshape((d.shape[0],)).astype(bool) for u, d in zip(utts, decisions)}
            if cmvn_config is not None:
                normed = SlidingWindowCmvnPostProcessor(**cmvn_config)._process_batch([raw_mfcc[u] for u in utts])
                orig_features = FeaturesCollection(zip(utts, normed))
            else:
                orig_features = raw_mfcc
            orig_features = orig_features.trim(vad)
            orig_features = FeaturesCollection(
                {utt: feats.copy(subsample=self.subsample) for utt, feats in orig_features.items()})

            if waves is not None:
                self._mapping_sweep(config, utterances, raw_mfcc, vad, num_classes, waves, stats)
            else:
                self._mapping_host(utterances, utts, vad, num_classes, njobs)
        finally:
            if waves is not None:
                waves.clear()
            if cmvn_config is not None:
                self.features['sliding_window_cmvn'] = cmvn_config
        return orig_features

    def _mapping_host(self, utterances, utts, vad, num_classes, njobs):
        """The base transforms with a host round trip per class: the unwarped frames uploaded once, one warped
        extraction per class downloaded, trimmed, subsampled and uploaded"""
        dim = self.lvtln.dim()
        featsub_unwarped = pipeline.extract_features(
            self.features, utterances, njobs=njobs, log=null_logger()).trim(vad)
        xs = [featsub_unwarped[u].data[::self.subsample] for u in utts]
        nframes = sum(x.shape[0] for x in xs)
        dx = _backend.upload_rows(xs, np.float32)
        del featsub_unwarped
        for c in range(num_classes):
            this_warp = self.min_warp + c * self.warp_step
            self.log.info('Computing base transform (warp=%s) %s/%s', this_warp, c + 1, num_classes)
            warped = pipeline.extract_features_warp(
                self.features, utterances, this_warp, null_logger(), njobs=njobs).trim(vad)
            ys = [warped[u].data[::self.subsample] for u in utts]
            for x, y in zip(xs, ys):
                if x.shape != y.shape:
                    raise ValueError('Number of rows and/or columns differs: '
                                     f'{x.shape[0]} vs {y.shape[0]} rows, {x.shape[1]} vs '
                                     f'{y.shape[1]} columns, {dim} dim')
            dy = _backend.upload_rows(ys, np.float32)
            self._mapping_from_device(dx, dy, None, nframes, c, this_warp)

    def _mapping_sweep(self, config, utterances, raw_mfcc, vad, num_classes, waves, stats=None):
        """The base transforms from data that stay in HBM: every warped pass borrows the audio the unwarped one
        left in `waves` and leaves its features in HBM (one block per sample rate); the unwarped rows go up once,
        in the same layout, and the Gram of every class gathers its records from both by one (block, row) list -
        the rows the host path trims and subsamples, in the same order: the same Gram, bit for bit."""
        dim = self.lvtln.dim()
        view = pipeline._view_of(utterances)
        names = list(raw_mfcc.keys())
        xdim = raw_mfcc[names[0]].ndims if names else dim
        x_blocks, row_list, layout, counts = [], None, None, None
        try:
            for c in range(num_classes):
                this_warp = self.min_warp + c * self.warp_step
                self.log.info('Computing base transform (warp=%s) %s/%s', this_warp, c + 1, num_classes)
                out = []
                try:
                    offsets = pipeline._extract_features(
                        config, view, {u.name: float(this_warp) for u in view}, null_logger(), stages=('delta',),
                        utterance_properties=False, device_out=out, resident=waves, stats=stats, bare=True)
                    if layout is None:
                        # frame counts do not depend on the warp: the layout, the row list and the unwarped
                        # blocks are made once
                        layout, counts = {}, {}
                        for b, ((_, block_names, _), off) in enumerate(zip(out, offsets)):
                            for i, name in enumerate(block_names):
                                layout[name] = (b, int(off[i]))
                                counts[name] = int(off[i + 1] - off[i])
                        for name in names:
                            nx, ny = raw_mfcc[name].nframes, counts[name]
                            if nx != ny or xdim != dim:
                                raise ValueError('Number of rows and/or columns differs: '
                                                 f'{nx} vs {ny} rows, {xdim} vs {out[layout[name][0]][2]} '
                                                 f'columns, {dim} dim')
                        x_blocks = [_backend.upload_rows([raw_mfcc[n].data for n in block_names], np.float32)
                                    for _, block_names, _ in out]
                        blocks_of, rows = sweep_rows(names, vad, self.subsample, layout)
                        nframes = rows.size
                        row_list = _lvtln.upload_row_list(blocks_of, rows)
                    elif any(not np.array_equal(np.diff(off), [counts[n] for n in block_names])
                             for (_, block_names, _), off in zip(out, offsets)):
                        raise ValueError('Number of rows and/or columns differs between warps')
                    if any(ydim != xdim for _, _, ydim in out):
                        raise ValueError('Number of rows and/or columns differs: '
                                         f'{xdim} vs {out[0][2]} columns, {dim} dim')
                    M = _lvtln.vtln_gram_rows(x_blocks, [block for block, _, _ in out], row_list[0], row_list[1],
                                              nframes, dim)
                finally:
                    for block, _, _ in out:
                        block.free()
                self._mapping_from_gram(M, c, this_warp)
        finally:
            for block in x_blocks + list(row_list or ()):
                block.free()

    # ---- training (reference vtln.py:511-680)
    def process(self, utterances, ubm=None, group_by='utterance', njobs=1):
        """Compute the VTLN warp factors for the given utterances.

        Follows the reference step for step: features with the sliding CMVN popped, VAD on the raw
        features, CMVN, trim and subsample; one warped extraction per class and its mapping transform;
        Gaussian selection on the original frames and their posteriors; ``estimate``; then `num_iters`
        rounds of: transform the frames (on the device), UBM E-step and M-step on them, posteriors of the
        transformed frames with the original selection, ``estimate`` on the original frames.  The original
        frames, the selection and the posteriors stay in HBM for the whole loop.

        Returns
        -------
        warps : dict[str, float]
            Per utterance, or per speaker with ``group_by='speaker'``.
        """
        if group_by not in ('utterance', 'speaker'):
            raise ValueError(f'group_by must be "utterance" or "speaker", it is: {group_by}')
        if group_by == 'speaker' and not self.by_speaker:
            raise ValueError(
                'Asking to group warps by speaker but they are computed '
                'per utterance, please set VtlnProcessor.by_speaker to True')
        if self.by_speaker and not utterances.has_speakers():
            raise ValueError('Requested speaker based VTLN, but speaker information is missing')

        utt2speak = None
        if self.by_speaker:
            utt2speak = {utt.name: utt.speaker for utt in utterances}

        if self.min_warp > self.max_warp:
            raise ValueError(f'Min warp > max warp: {self.min_warp} > {self.max_warp}')

        if ubm is None:
            ubm = DiagUbmProcessor(**self.ubm)
            ubm.log.setLevel(self.log.getEffectiveLevel())
            ubm.process(utterances, njobs=njobs)
        else:
            if ubm.gmm is None:
                raise ValueError('Given UBM-GMM has not been trained')
            self.ubm = ubm.get_params()

        self.log.info('Initializing base LVTLN transforms')
        dim = ubm.gmm.dim()
        num_classes = int(1.5 + (self.max_warp - self.min_warp) / self.warp_step)
        default_class = int(0.5 + (1 - self.min_warp) / self.warp_step)
        self.lvtln = _lvtln.LinearVtln(dim, num_classes, default_class)

        orig_features = self._base_transforms(utterances, ubm, num_classes, njobs)

        self.log.debug('Computing Gaussian selection info')
        ubm.gaussian_selection(orig_features)

        # segments: one per speaker (its utterances in utt2speak order) or one per utterance
        if utt2speak is not None:
            groups = {spk: list(part.keys()) for spk, part in orig_features.partition(utt2speak).items()}
        else:
            groups = {utt: [utt] for utt in orig_features}
        keys = list(groups)
        order = [u for k in keys for u in groups[k]]
        offsets = np.zeros(len(keys) + 1, np.int64)
        np.cumsum([sum(orig_features[u].nframes for u in groups[k]) for k in keys], out=offsets[1:])
        width = max([ubm.selection[u].shape[1] for u in order if ubm.selection[u].ndim == 2] + [1])
        block = _gmm.FrameBlock([orig_features[u].data for u in order])
        sel = np.concatenate([ubm.selection[u].reshape(-1, width) for u in order], axis=0)
        dsel = block.upload_selection(sel) if block.nframes else _backend.DeviceBuffer(16, block.device)
        what = 'speaker' if utt2speak is not None else 'utterance'

        self.log.info('Computing LVTLN transforms (%s iterations)', self.num_iters)
        dpost = (block.selection_posteriors_device(_gmm.DeviceGmm(ubm.gmm, block.device), dsel, width)
                 if block.nframes else dsel)
        self.transforms, self.warps, trans = self._estimate_device(ubm, block, dsel, dpost, width, offsets, keys,
                                                                   what)
        dtrans = _backend.DeviceBuffer(max(16, trans.nbytes), block.device)
        ybuf = _backend.DeviceBuffer(4 * max(1, block.nframes * dim), block.device)
        for i in range(self.num_iters):
            self.log.debug('Updating model on pass %s/%s', i + 1, self.num_iters)
            dtrans.upload(trans)
            _lvtln.affine_apply_segments(block, offsets, dtrans, ybuf)
            yblock = _gmm.FrameBlock.from_device(ybuf, block.offsets, dim)
            if block.nframes:
                stats, _, _ = yblock.accumulate(_gmm.DeviceGmm(ubm.gmm, block.device))
                gmm_accs = _gmm.AccumDiagGmm.from_stats(stats)
            else:
                gmm_accs = _gmm.AccumDiagGmm(ubm.gmm.num_gauss(), dim)
            ubm.estimate(gmm_accs)
            if block.nframes:
                dpost = yblock.selection_posteriors_device(_gmm.DeviceGmm(ubm.gmm, block.device), dsel, width)
            self.transforms, self.warps, trans = self._estimate_device(
                ubm, block, dsel, dpost, width, offsets, keys, what)

        if self.by_speaker:
            self.transforms = {utt: self.transforms[spk] for utt, spk in utt2speak.items()}
            self.warps = {utt: self.warps[spk] for utt, spk in utt2speak.items()}

        self.log.info('Done training LVTLN model')
        if group_by == 'utterance':
            return self.warps
        return {spk: self.warps[utts[0].name] for spk, utts in utterances.by_speaker().items()}
