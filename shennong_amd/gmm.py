"""Diagonal-covariance GMM: the model, its statistics, the M-step and the HIP E-step.

Host-side stand-ins for the pykaldi objects the reference's UBM trainer uses (processor/ubm.py):

- :class:`DiagGmm` for ``kaldi.gmm.DiagGmm`` (float32 natural parameters, like Kaldi),
- :class:`AccumDiagGmm` for ``kaldi.gmm.AccumDiagGmm`` (float64 statistics, like Kaldi),
- :func:`mle_diag_gmm_update` for ``kaldi.gmm.mle_diag_gmm_update`` (fp64, C x D work on the host).

The per-frame work (log-likelihoods, E-step statistics, Gaussian selection, posteriors) runs on the GPU
over a :class:`FrameBlock`, a device-resident block of frames uploaded once (``kernels_gmm.hip``).
"""

import ctypes as C
import io
import math

import numpy as np

from shennong_amd import _backend
from shennong_amd.serializers import KaldiBinaryReader, write_kaldi_object, write_kaldi_token


_LOG_2PI = math.log(2.0 * math.pi)


class DiagGmm:
    """Diagonal GMM in Kaldi's natural form ([KALDI-UPSTREAM] gmm/diag-gmm.h): ``gconsts[C]``,
    ``weights[C]``, ``means_invvars[C, D]`` (mean / variance) and ``inv_vars[C, D]``, float32.

    The getters return numpy arrays (copies) where pykaldi returns Kaldi vectors and matrices:
    ``get_means().shape[0]`` stands for ``get_means().num_rows``."""

    def __init__(self, num_gauss=0, dim=0):
        self.weights_ = np.zeros(num_gauss, dtype=np.float32)
        self.means_invvars_ = np.zeros((num_gauss, dim), dtype=np.float32)
        self.inv_vars_ = np.ones((num_gauss, dim), dtype=np.float32)
        self.gconsts_ = np.zeros(num_gauss, dtype=np.float32)
        self.valid_gconsts = False

    def num_gauss(self):
        return self.weights_.shape[0]

    def dim(self):
        return self.means_invvars_.shape[1]

    def copy(self):
        other = DiagGmm()
        other.weights_, other.gconsts_ = self.weights_.copy(), self.gconsts_.copy()
        other.means_invvars_, other.inv_vars_ = self.means_invvars_.copy(), self.inv_vars_.copy()
        other.valid_gconsts = self.valid_gconsts
        return other

    # ---- getters (Kaldi DiagGmm::GetMeans / GetVars / weights / gconsts)
    def get_means(self):
        return (self.means_invvars_.astype(np.float64) / self.inv_vars_).astype(np.float32)

    def get_vars(self):
        return (1.0 / self.inv_vars_.astype(np.float64)).astype(np.float32)

    def weights(self):
        return self.weights_.copy()

    def gconsts(self):
        """Kaldi raises when the gconsts are not valid (after a setter); so does this"""
        if not self.valid_gconsts:
            raise RuntimeError('Must call ComputeGconsts() before using gconsts')
        return self.gconsts_.copy()

    def means_invvars(self):
        return self.means_invvars_.copy()

    def inv_vars(self):
        return self.inv_vars_.copy()

    # ---- setters (Kaldi DiagGmm::SetMeans / SetInvVars / SetWeights, SetComponent*)
    def set_means(self, means):
        means = np.asarray(means, dtype=np.float64)
        self.means_invvars_ = (means * self.inv_vars_).astype(np.float32)
        self.valid_gconsts = False

    def set_inv_vars(self, inv_vars):
        """Keeps the means (Kaldi SetInvVars rescales means_invvars)"""
        means = self.means_invvars_.astype(np.float64) / self.inv_vars_
        self.inv_vars_ = np.asarray(inv_vars, dtype=np.float32).reshape(self.inv_vars_.shape).copy()
        self.means_invvars_ = (means * self.inv_vars_).astype(np.float32)
        self.valid_gconsts = False

    def set_weights(self, weights):
        self.weights_ = np.asarray(weights, dtype=np.float32).reshape(self.weights_.shape).copy()
        self.valid_gconsts = False

    def compute_gconsts(self):
        """[KALDI-UPSTREAM] diag-gmm.cc DiagGmm::ComputeGconsts:
        gconst = log w - D/2 log 2pi + sum_d (1/2 log iv_d - mi_d^2 / (2 iv_d)), -inf for a zero weight.
        Returns the number of NaN gconsts (Kaldi's num_bad)."""
        iv = self.inv_vars_.astype(np.float64)
        mi = self.means_invvars_.astype(np.float64)
        with np.errstate(divide='ignore'):
            gc = (np.log(self.weights_.astype(np.float64)) - 0.5 * _LOG_2PI * self.dim()
                  + np.sum(0.5 * np.log(iv) - 0.5 * mi * mi / iv, axis=1))
        bad = np.isnan(gc)
        gc[bad & (self.weights_ == 0)] = -np.inf
        if np.any(bad & (self.weights_ != 0)):
            raise ValueError('Not a number in gconst computation')
        self.gconsts_ = gc.astype(np.float32)
        self.valid_gconsts = True
        return int(bad.sum())

    def split(self, target_components, perturb_factor, rng):
        """[KALDI-UPSTREAM] diag-gmm.cc DiagGmm::Split: while fewer than `target_components`, the heaviest
        component (first one on a tie, new ones included) is halved into a copy, and the two means move by
        -/+ perturb_factor * sigma * z.  Kaldi draws z with RandGauss(); here z = ``rng.randn(dim)`` is
        drawn once per new component, in creation order, so a test can replay it.  Returns the split
        components' indices."""
        cur = self.num_gauss()
        if target_components < cur or cur == 0:
            raise ValueError(f'Cannot split from {cur} to {target_components} components')
        history = []
        if target_components == cur:
            return history
        extra = target_components - cur
        self.weights_ = np.concatenate([self.weights_, np.zeros(extra, np.float32)])
        self.means_invvars_ = np.concatenate([self.means_invvars_, np.zeros((extra, self.dim()), np.float32)])
        self.inv_vars_ = np.concatenate([self.inv_vars_, np.ones((extra, self.dim()), np.float32)])
        for i in range(cur, target_components):
            j = int(np.argmax(self.weights_[:i]))
            history.append(j)
            self.weights_[j] /= np.float32(2)
            self.weights_[i] = self.weights_[j]
            rand = (rng.randn(self.dim()).astype(np.float32) * np.sqrt(self.inv_vars_[j])).astype(np.float32)
            self.inv_vars_[i] = self.inv_vars_[j]
            self.means_invvars_[i] = self.means_invvars_[j] + np.float32(perturb_factor) * rand
            self.means_invvars_[j] = self.means_invvars_[j] - np.float32(perturb_factor) * rand
        self.compute_gconsts()
        return history

    def remove_components(self, gauss, renorm_weights=True):
        """[KALDI-UPSTREAM] diag-gmm.cc DiagGmm::RemoveComponents"""
        keep = np.setdiff1d(np.arange(self.num_gauss()), np.asarray(gauss, dtype=np.int64))
        if keep.size == 0:
            raise ValueError('Cannot remove all the components of a GMM')
        self.weights_ = self.weights_[keep].copy()
        self.means_invvars_ = self.means_invvars_[keep].copy()
        self.inv_vars_ = self.inv_vars_[keep].copy()
        if renorm_weights:
            self.weights_ = (self.weights_ / np.float32(self.weights_.sum(dtype=np.float64))).astype(np.float32)
        self.compute_gconsts()

    # ---- Kaldi binary form ([KALDI-UPSTREAM] diag-gmm.cc DiagGmm::Write / Read)
    def write(self, stream):
        if not self.valid_gconsts:
            raise RuntimeError('Must call ComputeGconsts() before writing the model.')
        write_kaldi_token(stream, '<DiagGMM>')
        write_kaldi_token(stream, '<GCONSTS>')
        write_kaldi_object(stream, self.gconsts_)
        write_kaldi_token(stream, '<WEIGHTS>')
        write_kaldi_object(stream, self.weights_)
        write_kaldi_token(stream, '<MEANS_INVVARS>')
        write_kaldi_object(stream, self.means_invvars_)
        write_kaldi_token(stream, '<INV_VARS>')
        write_kaldi_object(stream, self.inv_vars_)
        write_kaldi_token(stream, '</DiagGMM>')

    def to_bytes(self):
        """The model as a binary Kaldi file (``\\0B`` marker first), readable by gmm-global-* tools"""
        stream = io.BytesIO()
        stream.write(b'\0B')
        self.write(stream)
        return stream.getvalue()

    @classmethod
    def from_bytes(cls, blob):
        if blob[:2] != b'\0B':
            raise ValueError('not a binary Kaldi file')
        reader = KaldiBinaryReader(blob, 2)
        gmm = cls()
        reader.expect('<DiagGMM>')
        tok = reader.token()
        if tok == '<GCONSTS>':
            gmm.gconsts_ = reader.object()
            tok = reader.token()
        if tok != '<WEIGHTS>':
            raise ValueError(f'expected token <WEIGHTS>, got {tok}')
        gmm.weights_ = reader.object()
        reader.expect('<MEANS_INVVARS>')
        gmm.means_invvars_ = reader.object()
        reader.expect('<INV_VARS>')
        gmm.inv_vars_ = reader.object()
        reader.expect('</DiagGMM>')
        gmm.compute_gconsts()  # (Kaldi's Read recomputes them too)
        return gmm


class AccumDiagGmm:
    """[KALDI-UPSTREAM] gmm/mle-diag-gmm.h AccumDiagGmm (all update flags): float64 ``occupancy [C]``,
    ``mean_accumulator [C, D]`` (sum P x), ``variance_accumulator [C, D]`` (sum P x^2)"""

    def __init__(self, num_gauss, dim):
        self.occupancy = np.zeros(num_gauss, dtype=np.float64)
        self.mean_accumulator = np.zeros((num_gauss, dim), dtype=np.float64)
        self.variance_accumulator = np.zeros((num_gauss, dim), dtype=np.float64)

    @classmethod
    def from_stats(cls, stats):
        """From the device layout [C, 2D + 1] = [occupancy | sum P x | sum P x^2]"""
        stats = np.asarray(stats, dtype=np.float64)
        dim = (stats.shape[1] - 1) // 2
        acc = cls(stats.shape[0], dim)
        acc.add_stats(stats)
        return acc

    def add_stats(self, stats):
        dim = self.mean_accumulator.shape[1]
        self.occupancy += stats[:, 0]
        self.mean_accumulator += stats[:, 1:dim + 1]
        self.variance_accumulator += stats[:, dim + 1:]

    def num_gauss(self):
        return self.occupancy.shape[0]

    def dim(self):
        return self.mean_accumulator.shape[1]


class MleDiagGmmOptions:
    """[KALDI-UPSTREAM] mle-diag-gmm.h MleDiagGmmOptions, with Kaldi's defaults"""

    def __init__(self, min_gaussian_weight=1e-5, min_gaussian_occupancy=10.0, min_variance=0.001,
                 remove_low_count_gaussians=True):
        self.min_gaussian_weight = float(min_gaussian_weight)
        self.min_gaussian_occupancy = float(min_gaussian_occupancy)
        self.min_variance = float(min_variance)
        self.remove_low_count_gaussians = bool(remove_low_count_gaussians)


def ml_objective(gmm, accs):
    """[KALDI-UPSTREAM] mle-diag-gmm.cc MlObjective (in float64 here)"""
    return float(accs.occupancy @ gmm.gconsts_.astype(np.float64)
                 + np.sum(accs.mean_accumulator * gmm.means_invvars_)
                 - 0.5 * np.sum(accs.variance_accumulator * gmm.inv_vars_))


def mle_diag_gmm_update(accs, gmm, opts):
    """M-step in place on `gmm`: [KALDI-UPSTREAM] mle-diag-gmm.cc MleDiagGmmUpdate (means, variances and
    weights), in float64.  Returns ``(objective change, count, floored elements, floored Gaussians,
    removed Gaussians)`` like pykaldi's ``mle_diag_gmm_update``.

    Per Gaussian with occupancy `occ` and `prob = occ / sum(occ)`:

    - ``occ > min_gaussian_occupancy and prob > min_gaussian_weight``: weight = prob, mean = m1 / occ,
      variance = m2 / occ - mean^2 floored at `min_variance`;
    - otherwise, with `remove_low_count_gaussians` and while fewer than C - 1 are marked, the component
      is removed (the last one never is); else it keeps its mean and variance and its weight becomes
      ``max(prob, min_gaussian_weight)`` (the ``ngmm.weights_(i) = std::max(prob, ...)`` line of the
      upstream branch that does not remove).

    Weights are not renormalised afterwards unless components were removed (RemoveComponents with
    renormalisation)."""
    ngauss = gmm.num_gauss()
    occ = accs.occupancy
    occ_sum = float(occ.sum())
    gmm.compute_gconsts()
    obj_old = ml_objective(gmm, accs)
    weights = gmm.weights_.astype(np.float64)
    inv_vars = gmm.inv_vars_.astype(np.float64)
    means = gmm.means_invvars_.astype(np.float64) / inv_vars
    variances = 1.0 / inv_vars
    to_remove = []
    floored_elements = floored_gauss = 0
    for i in range(ngauss):
        prob = occ[i] / occ_sum if occ_sum > 0.0 else 1.0 / ngauss
        if occ[i] > opts.min_gaussian_occupancy and prob > opts.min_gaussian_weight:
            weights[i] = prob
            means[i] = accs.mean_accumulator[i] / occ[i]
            var = accs.variance_accumulator[i] / occ[i] - means[i] ** 2
            floored = int(np.sum(var < opts.min_variance))
            var = np.maximum(var, opts.min_variance)
            if floored:
                floored_elements += floored
                floored_gauss += 1
            variances[i] = var
        elif opts.remove_low_count_gaussians and len(to_remove) < ngauss - 1:
            to_remove.append(i)
        else:
            weights[i] = max(prob, opts.min_gaussian_weight)
    # DiagGmmNormal::CopyToDiagGmm: natural parameters in float32
    gmm.weights_ = weights.astype(np.float32)
    gmm.inv_vars_ = (1.0 / variances).astype(np.float32)
    gmm.means_invvars_ = (means / variances).astype(np.float32)
    gmm.compute_gconsts()
    obj_new = ml_objective(gmm, accs)
    if to_remove:
        gmm.remove_components(to_remove, True)
    return obj_new - obj_old, occ_sum, floored_elements, floored_gauss, len(to_remove)


# ---- device side --------------------------------------------------------------------------------------------
def _p(buf):
    return C.c_void_p(buf.ptr) if buf is not None else None


class DeviceGmm:
    """The float32 natural parameters of a :class:`DiagGmm` in HBM (re-uploaded after every M-step:
    C x (2D + 1) floats)"""

    def __init__(self, gmm, device=None):
        if not gmm.valid_gconsts:
            gmm.compute_gconsts()
        self.num_gauss, self.dim = gmm.num_gauss(), gmm.dim()
        self.gconsts = _backend.DeviceBuffer(4 * self.num_gauss, device)
        self.means_invvars = _backend.DeviceBuffer(4 * self.num_gauss * self.dim, device)
        self.inv_vars = _backend.DeviceBuffer(4 * self.num_gauss * self.dim, device)
        self.gconsts.upload(gmm.gconsts_)
        self.means_invvars.upload(gmm.means_invvars_)
        self.inv_vars.upload(gmm.inv_vars_)

    def args(self):
        return (C.c_void_p(self.gconsts.ptr), C.c_void_p(self.means_invvars.ptr), C.c_void_p(self.inv_vars.ptr),
                self.num_gauss)


class FrameBlock:
    """Frames of one or more utterances, float32 [F, D] in HBM, uploaded once, with the utterance offsets
    (``offsets[u] .. offsets[u + 1]`` are the rows of utterance u) and optional per-frame weights"""

    def __init__(self, mats, weights=None, device=None):
        mats = [np.asarray(m, dtype=np.float32) for m in mats]
        if not mats:
            raise ValueError('FrameBlock needs at least one matrix')
        self.dim = int(mats[0].shape[1])
        self.offsets = np.zeros(len(mats) + 1, dtype=np.int64)
        np.cumsum([m.shape[0] for m in mats], out=self.offsets[1:])
        self.nframes = int(self.offsets[-1])
        self.device = _backend.get_device() if device is None else int(device)
        self.frames = _backend.upload_rows(mats, np.float32, self.device)
        self.weights = None
        if weights is not None:
            w = np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in weights])
            if w.shape[0] != self.nframes:
                raise ValueError('Wrong size for weights')
            self.weights = _backend.DeviceBuffer(4 * max(1, self.nframes), self.device)
            self.weights.upload(w)

    @classmethod
    def from_device(cls, frames, offsets, dim, device=None):
        """A block over an existing device buffer of float32 [F, D] frames (no copy): e.g. the output of
        :func:`shennong_amd.lvtln.affine_apply_segments`"""
        block = cls.__new__(cls)
        block.dim = int(dim)
        block.offsets = np.asarray(offsets, dtype=np.int64).copy()
        block.nframes = int(block.offsets[-1])
        block.device = frames.device if device is None else int(device)
        block.frames = frames
        block.weights = None
        return block

    def upload_selection(self, selection):
        """A selection [F, n] int32 in HBM, uploaded once for several :meth:`selection_posteriors_device`"""
        sel = np.ascontiguousarray(selection, dtype=np.int32)
        if sel.ndim != 2 or sel.shape[0] != self.nframes:
            raise ValueError('selection must be [frames, n]')
        dsel = _backend.DeviceBuffer(max(16, sel.nbytes), self.device)
        dsel.upload(sel)
        return dsel

    def selection_posteriors_device(self, dgmm, dsel, num_gselect, min_post=None):
        """:meth:`selection_posteriors` of a selection already in HBM (`dsel`, [F, num_gselect] int32); the
        posteriors stay on the device: a DeviceBuffer [F, num_gselect] float32"""
        self._check(dgmm)
        F, n = self.nframes, int(num_gselect)
        post = _backend.DeviceBuffer(4 * max(1, F * n), self.device)
        like = _backend.DeviceBuffer(4 * max(1, F), self.device)
        _backend.check(_backend.lib().snf_gmm_selection_posteriors(
            self.device, C.c_void_p(self.frames.ptr), F, self.dim, *dgmm.args(), C.c_void_p(dsel.ptr), n,
            -1.0 if min_post is None else float(min_post), C.c_void_p(post.ptr), C.c_void_p(like.ptr), None))
        return post

    def split(self, values):
        """Rows of a per-frame host array, per utterance"""
        return [values[a:b] for a, b in zip(self.offsets[:-1], self.offsets[1:])]

    def _check(self, dgmm):
        if dgmm.dim != self.dim:
            raise ValueError(f'Features have dimension {self.dim}, the GMM {dgmm.dim}')

    def loglikes(self, dgmm):
        """L [F, C] float32 (small blocks; tests)"""
        self._check(dgmm)
        out = _backend.DeviceBuffer(4 * max(1, self.nframes * dgmm.num_gauss), self.device)
        _backend.check(_backend.lib().snf_gmm_loglikes(
            self.device, C.c_void_p(self.frames.ptr), self.nframes, self.dim, *dgmm.args(), C.c_void_p(out.ptr),
            None))
        return out.download(np.empty((self.nframes, dgmm.num_gauss), dtype=np.float32))

    def posteriors(self, dgmm, out=None, with_lse=False):
        """Dense posteriors ``exp(L - lse)`` [F, C] float32 (snf_gmm_posteriors).  `out` None: a host array.
        `out` a DeviceBuffer of at least 4 F C bytes on the block's device: written there and returned, the
        posteriors stay in HBM.  `with_lse`: ``(posteriors, lse [F] float32 on the host)``, the per-frame
        log-sum-exp of :meth:`accumulate`, bit for bit."""
        self._check(dgmm)
        F, n = self.nframes, dgmm.num_gauss
        post = _backend.DeviceBuffer(4 * max(1, F * n), self.device) if out is None else out
        if post.nbytes < 4 * F * n:
            raise ValueError(f'out holds {post.nbytes} bytes, the posteriors need {4 * F * n}')
        lse = _backend.DeviceBuffer(4 * max(1, F), self.device) if with_lse else None
        _backend.check(_backend.lib().snf_gmm_posteriors(
            self.device, C.c_void_p(self.frames.ptr), F, self.dim, *dgmm.args(), C.c_void_p(post.ptr), _p(lse), None))
        result = post.download(np.empty((F, n), dtype=np.float32)) if out is None else post
        return (result, lse.download(np.empty(F, dtype=np.float32))) if with_lse else result

    def accumulate(self, dgmm, with_lse=False):
        """E-step: (stats [C, 2D + 1] float64, tot_like, lse [F] float32 or None)"""
        self._check(dgmm)
        n = dgmm.num_gauss * (2 * self.dim + 1)
        stats = _backend.DeviceBuffer(8 * n + 8, self.device)
        lse = _backend.DeviceBuffer(4 * max(1, self.nframes), self.device) if with_lse else None
        _backend.check(_backend.lib().snf_gmm_accumulate(
            self.device, C.c_void_p(self.frames.ptr), self.nframes, self.dim, _p(self.weights), *dgmm.args(),
            C.c_void_p(stats.ptr), C.c_void_p(stats.ptr + 8 * n), _p(lse), None))
        host = stats.download(np.empty(n + 1, dtype=np.float64))
        out_lse = lse.download(np.empty(self.nframes, dtype=np.float32)) if with_lse else None
        return host[:n].reshape(dgmm.num_gauss, -1), float(host[n]), out_lse

    def gselect(self, dgmm, num_gselect, preselect=None):
        """(indices [F, n] int32 best first, per-frame log-sum-exp of the selected L [F] float32)"""
        self._check(dgmm)
        F = self.nframes
        idx = _backend.DeviceBuffer(4 * max(1, F * num_gselect), self.device)
        lse = _backend.DeviceBuffer(4 * max(1, F), self.device)
        if preselect is None:
            _backend.check(_backend.lib().snf_gmm_gselect(
                self.device, C.c_void_p(self.frames.ptr), F, self.dim, *dgmm.args(), int(num_gselect),
                C.c_void_p(idx.ptr), C.c_void_p(lse.ptr), None))
        else:
            pre = np.ascontiguousarray(preselect, dtype=np.int32)
            if pre.ndim != 2 or pre.shape[0] != F:
                raise ValueError('preselection must be [frames, n]')
            dpre = _backend.DeviceBuffer(max(16, pre.nbytes), self.device)
            dpre.upload(pre)
            _backend.check(_backend.lib().snf_gmm_gselect_preselect(
                self.device, C.c_void_p(self.frames.ptr), F, self.dim, *dgmm.args(), C.c_void_p(dpre.ptr),
                int(pre.shape[1]), int(num_gselect), C.c_void_p(idx.ptr), C.c_void_p(lse.ptr), None))
        return (idx.download(np.empty((F, num_gselect), dtype=np.int32)),
                lse.download(np.empty(F, dtype=np.float32)))

    def selection_posteriors(self, dgmm, selection, min_post=None):
        """(posteriors [F, n] float32 aligned with `selection`, pruned entries 0; loglike [F] float32)"""
        self._check(dgmm)
        sel = np.ascontiguousarray(selection, dtype=np.int32)
        F = self.nframes
        if sel.ndim != 2 or sel.shape[0] != F:
            raise ValueError('selection must be [frames, n]')
        n = sel.shape[1]
        dsel = _backend.DeviceBuffer(max(16, sel.nbytes), self.device)
        dsel.upload(sel)
        post = _backend.DeviceBuffer(4 * max(1, F * n), self.device)
        like = _backend.DeviceBuffer(4 * max(1, F), self.device)
        _backend.check(_backend.lib().snf_gmm_selection_posteriors(
            self.device, C.c_void_p(self.frames.ptr), F, self.dim, *dgmm.args(), C.c_void_p(dsel.ptr), n,
            -1.0 if min_post is None else float(min_post), C.c_void_p(post.ptr), C.c_void_p(like.ptr), None))
        return (post.download(np.empty((F, n), dtype=np.float32)),
                like.download(np.empty(F, dtype=np.float32)))
