"""Provides the DiagUbmProcessor class to train a Universal Background Model

- Gaussian Mixture Model (UBM-GMM) with diagonal covariances.
- Same parameters, defaults, checks and messages as the reference's processor/ubm.py (which runs
  Kaldi's DiagGmm per frame); here the E-step, the Gaussian selection and the posteriors are HIP kernels
  (``kernels_gmm.hip``) over frames uploaded once, and the M-step is float64 numpy
  (:func:`shennong_amd.gmm.mle_diag_gmm_update`).

Examples
--------

>>> from shennong_amd import Utterances
>>> from shennong_amd.processor.ubm import DiagUbmProcessor
>>> wav = './tests/golden/test.wav'
>>> utterances = Utterances(
...     [('utt1', wav, 'spk1', 0, 1), ('utt2', wav, 'spk1', 1, 1.4)])
>>> num_gauss = 4
>>> ubm = DiagUbmProcessor(num_gauss, num_iters_init=10)
>>> ubm.num_iters = 3
>>> ubm.process(utterances)                                   # doctest: +SKIP
>>> means = ubm.gmm.get_means()                               # doctest: +SKIP
>>> means.shape[0] == num_gauss, means.shape[1]               # doctest: +SKIP
(True, 39)

Randomness
----------
``self._rng = np.random.RandomState(seed)`` (reset by the `seed` setter) is drawn from as follows:

- corpus of at most `num_frames` frames: no draw before the reference's
  ``_rng.choice(num_frames, num_gauss_init, replace=False)`` (ubm.py:416), so the initial model is the
  reference's;
- larger corpus: the reference keeps `num_frames` frames by a per-frame reservoir (ubm.py:310-322, with
  its FIXME bias against the last slot).  That loop is replaced by ONE uniform draw without replacement,
  ``_rng.choice(num_read, num_frames, replace=False)`` (kept in corpus order) - a documented divergence;
- :meth:`DiagGmm.split` draws ``_rng.randn(dim)`` per new component, in creation order, where Kaldi's
  ``Split`` calls its non-reproducible RandGauss().
"""

import copy
import os

import numpy as np

from shennong_amd import _backend
from shennong_amd import gmm as _gmm
from shennong_amd import pipeline
from shennong_amd.base import BaseProcessor
from shennong_amd.device import DeviceFeaturesCollection
from shennong_amd.features import Features, FeaturesCollection
from shennong_amd.logger import null_logger
from shennong_amd.postprocessor.cmvn import SlidingWindowCmvnPostProcessor
from shennong_amd.postprocessor.vad import VadPostProcessor


class DiagUbmProcessor(BaseProcessor):
    """Universal Background Model with Diagonal GMM"""
    name = 'ubm'

    def __init__(self, num_gauss,
                 num_iters=4, num_gselect=15, initial_gauss_proportion=0.5,
                 num_iters_init=20, num_frames=500000,
                 subsample=5, min_gaussian_weight=1e-4,
                 remove_low_count_gaussians=False, seed=0,
                 features=None, vad=None):
        super().__init__()
        self._options = _gmm.MleDiagGmmOptions()
        self._options.min_gaussian_weight = float(min_gaussian_weight)
        self._options.remove_low_count_gaussians = bool(remove_low_count_gaussians)

        self.num_gauss = num_gauss
        self.num_iters = num_iters
        self.num_iters_init = num_iters_init
        self.num_gselect = num_gselect
        self.initial_gauss_proportion = initial_gauss_proportion
        self.num_frames = num_frames
        self.subsample = subsample
        self.seed = seed

        if vad is None:
            config = VadPostProcessor().get_params()
            config['energy_threshold'] = 5.5
            self.vad = config
        else:
            self.vad = vad

        if features in (None, 'default'):
            config = pipeline.get_default_config('mfcc', with_delta=True)
            config['sliding_window_cmvn'] = SlidingWindowCmvnPostProcessor().get_params()
            config['sliding_window_cmvn']['cmn_window'] = 300
            config['delta']['window'] = 3
            self.features = config
        else:
            self.features = features

        self.gmm = None
        self.selection = None

    # ---- parameters (reference ubm.py:104-233)
    @property
    def num_gauss(self):
        """Number of Gaussians in the model"""
        return self._num_gauss

    @num_gauss.setter
    def num_gauss(self, value):
        if int(value) < 2:
            raise ValueError('Number of gaussians must be at least 2, not {}'.format(value))
        self._num_gauss = int(value)

    @property
    def num_iters(self):
        """Number of iterations of training."""
        return self._num_iters

    @num_iters.setter
    def num_iters(self, value):
        self._num_iters = int(value)

    @property
    def num_iters_init(self):
        """ Number of E-M iterations for model initialization."""
        return self._num_iters_init

    @num_iters_init.setter
    def num_iters_init(self, value):
        self._num_iters_init = int(value)

    @property
    def num_gselect(self):
        """Number of Gaussians per frame to limit computation to, for speed."""
        return self._num_gselect

    @num_gselect.setter
    def num_gselect(self, value):
        self._num_gselect = int(value)

    @property
    def initial_gauss_proportion(self):
        """Proportion of Gaussians to start with in initialization phase (then split)"""
        return self._initial_gauss_proportion

    @initial_gauss_proportion.setter
    def initial_gauss_proportion(self, value):
        self._initial_gauss_proportion = float(value)

    @property
    def num_frames(self):
        """Maximum num-frames to keep in memory for model initialization."""
        return self._num_frames

    @num_frames.setter
    def num_frames(self, value):
        self._num_frames = int(value)

    @property
    def subsample(self):
        """In main E-M phase, use every n frames (a speedup)"""
        return self._subsample

    @subsample.setter
    def subsample(self, value):
        self._subsample = int(value)

    @property
    def min_gaussian_weight(self):
        """Minimum weight below which a Gaussian is not updated"""
        return np.float32(self._options.min_gaussian_weight)

    @min_gaussian_weight.setter
    def min_gaussian_weight(self, value):
        self._options.min_gaussian_weight = float(value)

    @property
    def remove_low_count_gaussians(self):
        """Remove Gaussians with a weight below `min_gaussian_weight`"""
        return self._options.remove_low_count_gaussians

    @remove_low_count_gaussians.setter
    def remove_low_count_gaussians(self, value):
        self._options.remove_low_count_gaussians = bool(value)

    @property
    def features(self):
        """Features extraction configuration"""
        return self._features

    @features.setter
    def features(self, value):
        if not isinstance(value, dict):
            raise TypeError('Features configuration must be a dict')
        if 'mfcc' not in value:
            raise ValueError('Need mfcc features to train UBM-GMM')
        self._features = copy.deepcopy(value)

    @property
    def vad(self):
        """VAD configuration for the UBM-GMM"""
        return self._vad

    @vad.setter
    def vad(self, value):
        if not isinstance(value, dict):
            raise TypeError('VAD configuration must be a dict')
        vad_keys = VadPostProcessor().get_params().keys()
        if not value.keys() <= vad_keys:
            raise ValueError('Unknown parameters given for VAD config')
        self._vad = copy.deepcopy(value)

    @property
    def seed(self):
        """Random seed for initialization from random frames"""
        return self._seed

    @seed.setter
    def seed(self, value):
        self._seed = int(value)
        self._rng = np.random.RandomState(seed=self._seed)

    # ---- model files (reference ubm.py:241-266)
    @classmethod
    def load(cls, path):
        """Load the GMM from a binary Kaldi file"""
        if not os.path.isfile(path):
            raise OSError('{}: file not found'.format(path))
        with open(path, 'rb') as stream:
            gmm = _gmm.DiagGmm.from_bytes(stream.read())
        ubm = DiagUbmProcessor(gmm.num_gauss())
        ubm.gmm = gmm
        return ubm

    def save(self, path):
        """Save the GMM to a binary Kaldi file"""
        if os.path.isfile(path):
            raise OSError('{}: file already exists'.format(path))
        if not isinstance(self.gmm, _gmm.DiagGmm):
            raise TypeError('GMM not initialized')
        if not self.gmm.valid_gconsts:
            self.log.debug('Computing gconsts before saving GMM')
            self.gmm.compute_gconsts()
        with open(path, 'wb') as stream:
            stream.write(self.gmm.to_bytes())

    # ---- helpers
    @staticmethod
    def _matrices(feats_collection):
        return [np.asarray(feats_collection[utt].data, dtype=np.float32) for utt in feats_collection.keys()]

    def _check_gmm(self):
        if not isinstance(self.gmm, _gmm.DiagGmm):
            raise TypeError('GMM not initialized')

    def _em_step(self, block, dgmm=None):
        """One E-step on the device: (AccumDiagGmm, tot_like)"""
        stats, tot_like, _ = block.accumulate(dgmm or _gmm.DeviceGmm(self.gmm, block.device))
        return _gmm.AccumDiagGmm.from_stats(stats), tot_like

    # ---- training (reference ubm.py:268-429)
    def _select_init_frames(self, feats_collection):
        """The frames the initialisation trains on, float32 [N, D] (see the module's Randomness note)"""
        dim = 0
        for utt in feats_collection.keys():
            this = feats_collection[utt].data
            if dim == 0:
                dim = this.shape[1]
            elif this.shape[1] != dim:
                raise ValueError(
                    'Features have unconsistent dims '
                    f'{this.shape[1]} vs {dim}'
                    f'(current utt is {utt})')
        mats = self._matrices(feats_collection)
        feats = np.concatenate(mats, axis=0) if mats else np.zeros((0, dim), np.float32)
        num_read = feats.shape[0]
        if num_read <= self.num_frames:
            if num_read < self.num_frames:
                self.log.debug('Number of frames read %s was less than target number %s, using all we read',
                               num_read, self.num_frames)
            return feats
        keep = np.sort(self._rng.choice(num_read, self.num_frames, replace=False))
        self.log.debug('Kept %s out of %s input frames = %s %%',
                       self.num_frames, num_read, 100 * self.num_frames / num_read)
        return feats[keep]

    def initialize_gmm(self, feats_collection, njobs=1):
        """Initializes a single diagonal GMM and does the initial iterations of training (reference
        ubm.py:268-364, Kaldi gmm-global-init-from-feats).  `njobs` is accepted for compatibility.

        Raises
        ------
        ValueError
            If the features have unconsistent dimensions, too few frames or no positive variance.
        """
        num_gauss_init = int(self.initial_gauss_proportion * self.num_gauss)
        self.log.info('Initializing model')
        feats = self._select_init_frames(feats_collection)
        self.gmm = _gmm.DiagGmm(num_gauss_init, feats.shape[1])
        self._init_from_random_frames(feats)

        cur_num_gauss = num_gauss_init
        gauss_inc = int((self.num_gauss - num_gauss_init) / (self.num_iters_init / 2))
        if gauss_inc == 0:
            self.log.warning('Number of gaussians %s is too low', self.num_gauss)
            gauss_inc = 1

        block = _gmm.FrameBlock([feats])
        self.split_history = []
        for i in range(self.num_iters_init):
            self.log.debug('Iteration %s', i)
            accs, tot_like = self._em_step(block)
            self.log.debug('Likelihood per frame: %s over %s frames', tot_like / feats.shape[0], feats.shape[0])
            obj_change, count, _, _, _ = _gmm.mle_diag_gmm_update(accs, self.gmm, self._options)
            self.log.debug('Objective-function change: %s over %s frames', obj_change / count, count)
            next_num_gauss = min(self.num_gauss, cur_num_gauss + gauss_inc)
            if next_num_gauss > self.gmm.num_gauss():
                self.log.debug('Splitting to %s Gaussians', next_num_gauss)
                self.split_history.append(self.gmm.split(next_num_gauss, 0.1, self._rng))
                cur_num_gauss = next_num_gauss

    def _init_from_random_frames(self, feats):
        """Variances to the global variance of the features, means to distinct random frames (reference
        ubm.py:366-429)"""
        num_gauss = self.gmm.num_gauss()
        num_frames, dim = feats.shape
        if num_frames < 10 * num_gauss:
            raise ValueError(f'Too few frames to train on ({num_frames} frames)')
        x = feats.astype(np.float64)
        mean = x.mean(axis=0)
        var = (x * x).mean(axis=0) - mean * mean
        if var.max() <= 0:
            raise ValueError(f'Features do not have positive variance {var.astype(np.float32)}')
        inv_var = (1.0 / var).astype(np.float32)
        random_frames = self._rng.choice(num_frames, num_gauss, replace=False)
        self.gmm.weights_ = np.full(num_gauss, np.float32(1.0 / num_gauss), dtype=np.float32)
        self.gmm.inv_vars_ = np.tile(inv_var, (num_gauss, 1))
        self.gmm.means_invvars_ = (feats[random_frames] * inv_var).astype(np.float32)
        self.gmm.compute_gconsts()

    def _selection_arrays(self, feats_collection, what='Input gselect'):
        out = {}
        for utt in feats_collection.keys():
            if utt not in self.selection:
                raise ValueError(f'No gselect information for utterance {utt}')
            sel = self.selection[utt]
            nframes = feats_collection[utt].nframes
            if len(sel) != nframes:
                raise ValueError(f'{what} utterance {utt} has wrong size {len(sel)} vs {nframes}')
            arr = np.asarray(sel, dtype=np.int32)
            if nframes and arr.ndim != 2:
                raise ValueError(f'{what} utterance {utt} has rows of different lengths')
            out[utt] = arr.reshape(nframes, -1)
        return out

    def gaussian_selection(self, feats_collection):
        """Precompute Gaussian indices for pruning: for each frame the `num_gselect` best Gaussians,
        best first (reference ubm.py:431-504, Kaldi gmm-gselect).  With a selection already present it is
        used as the preselection.  ``selection[utt]`` is an int32 array [frames, num_gselect]."""
        self._check_gmm()
        already_selection = self.selection is not None
        if self.num_gselect > self.gmm.num_gauss():
            self.log.warning(
                'You asked for %s Gaussians but GMM only has %s,'
                ' returning this many. Note: this means the'
                ' Gaussian selection is pointless',
                self.num_gselect, self.gmm.num_gauss())
            self.num_gselect = self.gmm.num_gauss()
        utts = list(feats_collection.keys())
        if not utts:
            if not already_selection:
                self.selection = {}
            return
        preselect = self._selection_arrays(feats_collection) if already_selection else None
        block = _gmm.FrameBlock(self._matrices(feats_collection))
        dgmm = _gmm.DeviceGmm(self.gmm, block.device)
        if preselect is None:
            idx, like = block.gselect(dgmm, self.num_gselect)
            self.selection = {}
        else:
            widths = {p.shape[1] for p in preselect.values() if p.shape[0]}
            if len(widths) > 1:
                raise ValueError('Input gselect utterances have different numbers of Gaussians per frame')
            width = widths.pop() if widths else self.num_gselect
            n = min(self.num_gselect, width)
            idx, like = block.gselect(dgmm, n, np.concatenate([preselect[u] for u in utts], axis=0)
                                      if block.nframes else np.zeros((0, width), np.int32))
        for utt, rows in zip(utts, block.split(idx)):
            self.selection[utt] = rows.copy()
        tot_t = block.nframes
        if tot_t:
            self.log.debug('Done %s utterances, mean UBM log-likelihood is %s over %s frames',
                           len(utts), float(like.astype(np.float64).sum()) / tot_t, tot_t)

    def _selection_posteriors(self, feats_collection, min_post=None):
        """Array form of :meth:`gaussian_selection_to_post`: utt -> (selection [F, n] int32,
        posteriors [F, n] float32 with pruned entries at 0)"""
        if not isinstance(self.selection, dict):
            raise ValueError('Gaussian selection has not been done')
        self._check_gmm()
        selection = self._selection_arrays(feats_collection, what='Input gselect')
        utts = [u for u in feats_collection.keys() if selection[u].shape[0]]
        out = {u: (selection[u], np.zeros(selection[u].shape, np.float32)) for u in feats_collection.keys()}
        by_width = {}
        for utt in utts:
            by_width.setdefault(selection[utt].shape[1], []).append(utt)
        for group in by_width.values():
            block = _gmm.FrameBlock([feats_collection[u].data for u in group])
            post, like = block.selection_posteriors(
                _gmm.DeviceGmm(self.gmm, block.device),
                np.concatenate([selection[u] for u in group], axis=0), min_post)
            for utt, p, l in zip(group, block.split(post), block.split(like)):
                out[utt] = (selection[utt], p)
                self.log.debug('Likelihood per frame for utt %s was %s per frame over %s frames',
                               utt, float(l.astype(np.float64).mean()), l.shape[0])
        return out

    def gaussian_selection_to_post(self, feats_collection, min_post=None):
        """Per-frame posteriors of the selected Gaussians (reference ubm.py:506-583, Kaldi
        gmm-global-gselect-to-post), pruned below `min_post` by the reference's sequential loop.

        Returns
        -------
        posteriors : dict[str, list[list[tuple[int, float]]]]
            For each utterance and frame, (Gaussian, posterior) of the non-zero posteriors."""
        out = {}
        for utt, (sel, post) in self._selection_posteriors(feats_collection, min_post).items():
            keep = post != 0
            counts = keep.sum(axis=1)
            pairs = list(zip(sel[keep].tolist(), post[keep].tolist()))
            cuts = np.cumsum(counts)[:-1].tolist() if counts.size else []
            bounds = zip([0] + cuts, cuts + [len(pairs)])
            out[utt] = [pairs[a:b] for a, b in bounds] if counts.size else []
        return out

    def posteriorgrams(self, feats_collection, device=False):
        """The posteriorgram of every utterance under the trained model: one probability per frame and Gaussian,
        ``exp(L[f, c] - logsumexp_c L[f, :])``, float32 [nframes, num_gauss], with the input's times (an extension:
        the reference hands out the pruned posteriors of a selection only, :meth:`gaussian_selection_to_post`).
        No pruning, no smoothing.  Computed on the device over all the frames at once (snf_gmm_posteriors).

        Parameters
        ----------
        feats_collection : FeaturesCollection or DeviceFeaturesCollection
            The features the model was trained on (same dimension).  A device collection is read where it lies
            and must lie in one block.
        device : bool
            True: a :class:`~shennong_amd.device.DeviceFeaturesCollection` over the block the kernel wrote,
            for :func:`~shennong_amd.dtw_distances` or :func:`~shennong_amd.abx_scores` with
            ``metric='symkl'`` or for ``padded()``.  False: its ``to_host()``.

        The properties are the input's plus ``'posteriorgram': {'num_gauss': ..., 'ndims': ...}`` (`ndims` of
        the source features).

        Raises
        ------
        TypeError
            If the model is not trained.
        ValueError
            If the features do not have the model's dimension, or lie in several device blocks.
        """
        self._check_gmm()
        owned = None
        if isinstance(feats_collection, DeviceFeaturesCollection):
            source = feats_collection
            source._alive()
            if len(source._blocks) > 1:
                raise ValueError('the utterances lie in {} device blocks (one per sample rate): posteriorgrams '
                                 'are made of one block'.format(len(source._blocks)))
        else:
            source = owned = DeviceFeaturesCollection.from_host(feats_collection)
        try:
            names = list(source)
            num_gauss, ndims = self.gmm.num_gauss(), self.gmm.dim()
            extra = {'posteriorgram': {'num_gauss': num_gauss, 'ndims': ndims}}
            template = FeaturesCollection()
            for name in names:
                feats = source[name]
                shape = (feats.nframes, num_gauss)
                placeholder = np.broadcast_to(np.float32(0), shape) if shape[0] else np.zeros(shape, np.float32)
                # (the result copies times and properties when they are first read: the input's are not touched)
                template[name] = Features._of_batch(placeholder, feats.times, feats.properties, extra)
            if source._blocks:
                in_block = source._blocks[0]
                block = _gmm.FrameBlock.from_device(in_block.alive(), in_block.foff, in_block.dim)
                order = in_block.names
            else:
                block, order = None, names
            nframes = block.nframes if block is not None else 0
            device_id = block.device if block is not None else None
            out = _backend.DeviceBuffer(max(16, 4 * nframes * num_gauss), device_id)
            try:
                if nframes:
                    block.posteriors(_gmm.DeviceGmm(self.gmm, block.device), out=out)
                result = DeviceFeaturesCollection._build(template, [(out, order, num_gauss)])
            except BaseException:
                out.free()
                raise
        finally:
            if owned is not None:
                owned.release()
        if device:
            return result
        try:
            return result.to_host()
        finally:
            result.release()

    def accumulate(self, feats_collection, weights_collection=None, njobs=1):
        """Statistics for training a diagonal GMM (reference ubm.py:585-664, Kaldi gmm-global-acc-stats).
        `njobs` is accepted for compatibility.

        Returns
        -------
        gmm_accs : :class:`shennong_amd.gmm.AccumDiagGmm`
        """
        self._check_gmm()
        dim = self.gmm.dim()
        for utt, feats in feats_collection.items():
            if feats.ndims != dim:
                raise ValueError(f'Features from utterance {utt} have wrong dims {feats.ndims}, instead of {dim}')
        if weights_collection is not None:
            if weights_collection.keys() != feats_collection.keys():
                raise ValueError('Keys differ between weights and features collections')
            for utt, weights in weights_collection.items():
                if np.asarray(weights).shape[0] != feats_collection[utt].nframes:
                    raise ValueError(f'Wrong size for weights on utterance {utt}')
        utts = list(feats_collection.keys())
        if not utts:
            return _gmm.AccumDiagGmm(self.gmm.num_gauss(), dim)
        weights = None if weights_collection is None else [weights_collection[u] for u in utts]
        block = _gmm.FrameBlock(self._matrices(feats_collection), weights)
        accs, tot_like = self._em_step(block)
        tot_weight = block.nframes if weights is None else float(
            sum(np.asarray(w, dtype=np.float64).sum() for w in weights))
        if tot_weight:
            self.log.debug('Overall likelihood per frame = %s over %s weighted frames',
                           tot_like / tot_weight, tot_weight)
        return accs

    def estimate(self, gmm_accs, mixup=None, perturb_factor=0.01):
        """M-step from the accumulated statistics (reference ubm.py:666-712, Kaldi gmm-global-est), then
        optionally split up to `mixup` components"""
        self._check_gmm()
        if mixup is not None and mixup <= self.num_gauss:
            raise ValueError('Mixup parameter must be greater than the number of gaussians')
        objf_impr, count, _, _, _ = _gmm.mle_diag_gmm_update(gmm_accs, self.gmm, self._options)
        if count:
            self.log.debug('Overall objective function improvement is %s per frame over %s frames',
                           objf_impr / count, count)
        if mixup is not None:
            self.gmm.split(int(mixup), perturb_factor, self._rng)

    def _prepare(self, utterances, njobs):
        """Steps 1-4 of :meth:`process`: features, VAD on the raw features, sliding CMVN, trim"""
        cmvn = self.features.pop('sliding_window_cmvn', None)
        try:
            raw = pipeline.extract_features(self.features, utterances, njobs=njobs, log=null_logger())
        finally:
            if cmvn is not None:
                self.features['sliding_window_cmvn'] = cmvn
        utts = list(raw.keys())
        decisions = VadPostProcessor(**self.vad)._process_batch([raw[u] for u in utts])
        vad = {u: d.data.reshape((d.shape[0],)).astype(bool) for u, d in zip(utts, decisions)}
        if cmvn is not None:
            normed = SlidingWindowCmvnPostProcessor(**cmvn)._process_batch([raw[u] for u in utts])
            features = FeaturesCollection(zip(utts, normed))
        else:
            features = raw
        return features.trim(vad)

    def process(self, utterances, njobs=1):
        """Initialize the GMM from random frames, then train it (reference ubm.py:714-772): features
        (with the sliding CMVN popped), VAD on the raw features, sliding CMVN, trim, initialisation,
        subsampling and `num_iters` EM iterations.  The subsampled frames are uploaded once for all the
        iterations.  `remove_low_count_gaussians` applies to the last iteration only."""
        self.log.info('Training UBM using %s jobs', njobs)
        features = self._prepare(utterances, njobs)
        self.initialize_gmm(features, njobs=njobs)
        self.log.info('Training for %s iterations', self.num_iters)
        features = FeaturesCollection(
            {utt: feats.copy(subsample=self.subsample) for utt, feats in features.items()})
        remove_low_count_gaussians = self.remove_low_count_gaussians
        self.remove_low_count_gaussians = False
        try:
            block = _gmm.FrameBlock(self._matrices(features))
            for i in range(self.num_iters):
                self.log.debug('Training pass %s', i + 1)
                accs, _ = self._em_step(block)
                if i == self.num_iters - 1:
                    self.remove_low_count_gaussians = remove_low_count_gaussians
                self.estimate(accs)
        finally:
            self.remove_low_count_gaussians = remove_low_count_gaussians
        self.log.info('Done training UBM.')

