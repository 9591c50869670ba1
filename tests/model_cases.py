"""Case builders shared by tests/test_gmm_seams_gpu.py, tests/test_vtln_seams_gpu.py and their CPU half
tests/test_model_cases.py: the shapes around every tile, chunk, item and pass boundary of kernels_gmm.hip and
kernels_vtln.hip, the derived error scales, and Python restatements of the host scheduling the shapes were chosen
against (csrc/capi_models.hip).  Host code only: numpy, the float64 references and the host-side model classes;
nothing here touches the device."""

import numpy as np

import gmm_f64 as RG
import lvtln_f64 as RV
from test_ubm_gpu import mixture, model64  # noqa: F401  (model64 is re-exported)
from test_vtln_gpu import class_setup, model, selection  # noqa: F401

from shennong_amd import lvtln as LV

POISON = 0xFFFFFFFF   # what a buffer out of the poisoned pool holds in every 32-bit word

# ---- GMM ----------------------------------------------------------------------------------------------------------
# k-chunk of dense_block (Kp = round_up(2D, 4), 64 per LDS stage): 31, 32, 33; column block of gmm_stats_kernel
# (J = 2D + 1, 128 per workgroup): 63, 64
GMM_DIMS = (1, 31, 32, 33, 63, 64)
SEAM_FRAMES = (1, 63, 64, 65, 129)                   # the 64-frame tile; three tiles
SEAM_GAUSSIANS = (1, 15, 16, 17, 63, 64, 65, 129)    # the 16-Gaussian MFMA tile, the 64-Gaussian block; three blocks
ESTEP_FRAMES = (63, 64, 65, 129)
CHUNKED = (4129, 2048, 64)                           # (F, C, D): 65 tiles in 22 chunks of 3, the last holding 2
SCRATCH = (16384 + 65, 2048, 2)                      # (F, C, D): the second scratch block holds 64 + 1 frames
SCRATCH_TAIL = 16382                                 # first frame of the block compared across the scratch seam
ZERO_WEIGHT = (4, 11)                                # Gaussians of weight 0 in zero_weight_case


SOFT_FRAMES = (65, 129)                              # the overlapping mixtures: soft posteriors at every D
SOFT_GAUSSIANS = (17, 65, 129)


def seam_mixture(F, C, D, soft=False):
    """`soft`: centres 2 / sqrt(D) apart per dimension instead of 6, so that neighbouring Gaussians are a few
    nats apart whatever D is (at 6 the posteriors are one-hot from D = 31 on: every log-sum-exp is the maximum)"""
    return mixture(F + 7 * C + D, F, D, C, sep=2.0 / np.sqrt(D)) if soft else mixture(F + 7 * C + D, F, D, C)


def seam_shapes(frames):
    """(F, C, soft) of the seam tests: the grid on the separated mixture, then a few shapes on the soft one"""
    return ([(F, C, False) for F in frames for C in SEAM_GAUSSIANS]
            + [(F, C, True) for F in SOFT_FRAMES for C in SOFT_GAUSSIANS])


def estep_weights(F):
    """Frame weights uniform in (0, 2), the first and the last frame's exactly 0"""
    w = np.random.RandomState(F).uniform(0, 2, F).astype(np.float32)
    w[0] = w[-1] = 0.0
    return w


def posteriors64(L):
    """(P [F, C], lse [F]) in float64 of log-likelihoods L"""
    L = np.asarray(L, np.float64)
    lse = RG.logsumexp(L, axis=1)
    with np.errstate(under='ignore'):
        return np.exp(L - lse[:, None]), lse


def estep_scale(x, L, w=None):
    """The derived error bound of the E-step statistics, element by element: (T, floor), both [C, 2D + 1].

    T[c, j] = sum_f P_fc w_f |y_fj| e_f with y = [1 | x | x^2] and e_f = 2^-23 (|lse_f| + 128): 2^-24 |lse_f| for
    the float32 lse, 2^-24 * 128 for the 64-term float32 tile sum, the rounding of L - lse for every P above 1e-30
    (|L - lse| < 70), expf and the weight product; the whole doubled.

    floor[c, j] = 1e-30 sum_f w_f |y_fj| covers what the derivation of T leaves out: a posterior below 1e-30
    carries a relative error below 2^-23 (|L - lse| + 128) < 1 as long as float32 can hold it and is flushed to
    zero below 1.2e-38, so its absolute error is below 1e-30 either way.  It matters only for a Gaussian none of
    whose frames has a posterior above ~1e-25, where T itself is of the order of the float32 underflow.  Measured
    (profiles/gmm_vtln_seams_errors.txt): without the floor such elements reach 8e5 T (the kernel holds 0 where
    float64 holds 1e-60); with it the worst element of every shape is 0.15 of the bound, the same figure as over
    the elements that have occupancy."""
    x = np.asarray(x, np.float64)
    F = x.shape[0]
    w = np.ones(F) if w is None else np.asarray(w, np.float64)
    P, lse = posteriors64(L)
    e = 2.0 ** -23 * (np.abs(lse) + 128.0)
    y = np.abs(np.concatenate([np.ones((F, 1)), x, x * x], axis=1))
    T = (P * (w * e)[:, None]).T @ y
    floor = 1e-30 * np.tile((w[:, None] * y).sum(axis=0), (P.shape[1], 1))
    return T, floor


def stats_chunks(F, C, D):
    """(chunks, tiles per chunk, tiles of the last chunk).  Mirrors gmm_stats_chunks() and the `per` of
    launch_gmm_accumulate() in csrc/kernels_gmm.hip: 64-frame tiles, 64-Gaussian blocks, 128-column blocks of
    J = 2D + 1, chunks so that the grid reaches 2048 workgroups."""
    ntiles = (F + 63) // 64
    grid = ((C + 63) // 64) * ((2 * D + 1 + 127) // 128)
    chunks = max(1, (2048 + grid - 1) // grid)
    chunks = min(chunks, max(ntiles, 1))
    per = (ntiles + chunks - 1) // chunks
    chunks = max(1, (ntiles + per - 1) // per)
    return chunks, per, ntiles - (chunks - 1) * per


def gselect_rows(F, C):
    """Frames per scratch block of L.  Mirrors `rows` of snf_gmm_gselect() in csrc/capi_models.hip."""
    rows = max(64, ((32 << 20) // C) & ~63)
    return min(rows, (F + 63) & ~63)


def zero_weight_case():
    """(x [65, 3], gmm of 17 Gaussians, the Gaussians ZERO_WEIGHT with weight 0, hence gconst -inf)"""
    x, gmm = mixture(5, 65, 3, 17)
    weights = gmm.weights_.copy()
    weights[list(ZERO_WEIGHT)] = 0.0
    gmm.weights_ = weights
    gmm.compute_gconsts()
    return x, gmm


# ---- VTLN ---------------------------------------------------------------------------------------------------------
# D = 64: the only dimension with two column groups of the fMLLR product (V = 65) and three of the Gram (V = 129)
VTLN_DIMS = (1, 7, 8, 15, 16, 31, 32, 63, 64)
SHORT_LENS = (0, 1, 3, 4, 5, 31, 32, 33, 0, 0, 65, 0)     # the 4 frames of an MFMA step, the 32 of an LDS stage
LONG_LENS = (2047, 2048, 2049, 4096, 4097)                # the 2048 frames of an item
LONG_DIMS = (13, 64)
MIXED_LENS = (0, 5, 17, 2049, 33, 0, 64, 1, 31, 100, 3, 0)   # empty at 0, at 5 and last; one split segment
GRAM_FRAMES = (1, 3, 4, 5, 31, 32, 33)
GRAM_LONG_FRAMES = (2047, 2048, 2049, 4097)
SELECT_CASES = ((1, 1), (13, 31), (13, 32), (13, 33), (13, 41), (13, 65), (39, 41), (64, 33))   # (D, classes)
APPLY_OFFSETS = (0, 0, 0, 5, 5, 9, 300, 300)
DEFAULT_CLASSES, DEFAULT_CLASS = 41, 15                   # VtlnProcessor(): warps 0.85 .. 1.25 by 0.01


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def item_count(length):
    """Items of one segment.  Mirrors vtln_items() in csrc/capi_models.hip with vtln_item_frames() = 2048 of
    csrc/kernels_vtln.hip: none for an empty segment, else runs of at most 2048 frames."""
    return (length + 2047) // 2048


def fmllr_case(D, n, C, lens):
    """(x, gmm, selection, posteriors, offsets), drawn as test_vtln_gpu.test_fmllr_stats draws them"""
    offsets = offsets_of(lens)
    F = int(offsets[-1])
    rng = np.random.RandomState(D * 100 + n)
    x = (rng.randn(F, D) * 3 + 1).astype(np.float32)
    gmm = model(D + n + C, C, D)
    sel, post = selection(D + C, F, n, C)
    return x, gmm, sel, post, offsets


def select_segments(D):
    return 4 if D <= 39 else 2


def objective_abs(W, stats, extra):
    """Sum of the absolute values of the terms of the class objective aux(W) + extra:
    |beta log|det W_A|| + |extra| + sum |W K| + 1/2 sum_d |W_d| |G_d| |W_d|^T"""
    beta, K, Gm = stats
    D = K.shape[0]
    W = np.asarray(W, np.float64)
    ld = np.linalg.slogdet(W[:, :D])[1]
    return (abs(beta * ld) + abs(extra) + np.sum(np.abs(W * K))
            + 0.5 * np.einsum('dk,dkl,dl->', np.abs(W), np.abs(Gm), np.abs(W)))


def class_reference(As, logdets, stats, norm_type, logdet_scale):
    """(objectives [C], scales [C]): lvtln_f64.compute_transform class by class (a class's objective does not
    depend on the others) and objective_abs of its transform.  The two-matmul form above D = 13."""
    fast = stats[1].shape[0] > 13
    objs, scales = [], []
    for A, ld in zip(As, logdets):
        o, _, _, _, W = RV.compute_transform([A], [ld], stats, norm_type, logdet_scale, 0, fast=fast)
        objs.append(o[0])
        scales.append(objective_abs(W, stats, (logdet_scale - 1.0) * stats[0] * ld))
    return np.asarray(objs), np.asarray(scales)


def tied_lvtln(D, C, default_class, same, seed):
    """C classes A_c = I + 0.05 randn; the classes listed in `same` all hold the matrix of the first of them
    (`same` = 'all': one matrix everywhere)"""
    rng = np.random.RandomState(seed)
    lvtln = LV.LinearVtln(D, C, default_class)
    As = [(np.eye(D) + 0.05 * rng.randn(D, D)).astype(np.float32) for _ in range(C)]
    same = range(C) if same == 'all' else same
    for c in same:
        As[c] = As[same[0]]
    for c, A in enumerate(As):
        lvtln.set_transform(c, A)
    return lvtln


def default_config_case():
    """The class search as VtlnProcessor() configures it (41 classes, default class 15, 'offset', logdet_scale 0)
    at D = 39 on three segments: dict(lvtln, gmm, x, sel, post, offsets)"""
    D, seed = 39, 42   # (chosen so that the three winners are 2, 35, 2: both passes of 32 classes hold one)
    lvtln = tied_lvtln(D, DEFAULT_CLASSES, DEFAULT_CLASS, (), seed)
    gmm = model(seed, 32, D)
    offsets = offsets_of((150, 90, 220))
    F = int(offsets[-1])
    x = (np.random.RandomState(seed + 1).randn(F, D) * 1.5).astype(np.float32)
    sel, post = selection(seed + 2, F, 5, 32)
    return dict(lvtln=lvtln, gmm=gmm, x=x, sel=sel, post=post, offsets=offsets)


def default_config_reference(case):
    """Per segment (objectives [41], class, W) of lvtln_f64 from the frames themselves"""
    lvtln, gmm, off = case['lvtln'], case['gmm'], case['offsets']
    out = []
    for s in range(len(off) - 1):
        a, b = off[s], off[s + 1]
        st = RV.fmllr_stats(case['x'][a:b], case['sel'][a:b], case['post'][a:b], gmm.means_invvars_, gmm.inv_vars_)
        objs, best, _, _, W = RV.compute_transform(lvtln.A, [RV.logdet(A) for A in lvtln.A], st, 'offset', 0.0,
                                                   lvtln.default_class, fast=True)
        out.append((objs, best, W))
    return out


def top_two_margin(objs):
    """Relative distance between the two largest objectives"""
    top = np.sort(np.asarray(objs))[-2:]
    return (top[1] - top[0]) / abs(top[1])


def apply_case(D, offsets, seed=5):
    """(x [F, D], W [S, D, D + 1]) float32 for the per-segment affine apply"""
    rng = np.random.RandomState(seed + D)
    F, S = int(offsets[-1]), len(offsets) - 1
    return rng.randn(F, D).astype(np.float32), rng.randn(S, D, D + 1).astype(np.float32)


def apply_reference(x, W, offsets):
    """(y [F, D] float64, tolerance [F, D]): 2^-23 (D + 1) (sum_c |W_c x_c| + |W_D|), a float32 FMA chain of D
    terms and one add, doubled"""
    x64, W64 = np.asarray(x, np.float64), np.asarray(W, np.float64)
    D = x.shape[1]
    y, tol = np.zeros(x.shape), np.zeros(x.shape)
    for s in range(len(offsets) - 1):
        a, b = offsets[s], offsets[s + 1]
        y[a:b] = x64[a:b] @ W64[s][:, :D].T + W64[s][:, D]
        tol[a:b] = 2.0 ** -23 * (D + 1) * (np.abs(x64[a:b]) @ np.abs(W64[s][:, :D]).T + np.abs(W64[s][:, D]))
    return y, tol


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])

