"""Independent float64 numpy statement of linear-VTLN training ([KALDI-UPSTREAM] transform/fmllr-diag-gmm.cc,
transform-common.cc, lvtln.cc; reference processor/vtln.py).  A plain helper module of the test suite: it
shares no code with shennong_amd.lvtln."""

import numpy as np


def frame_terms(sel, post, means_invvars, inv_vars):
    """a [F, D], b [F, D], count [F]: sum_j p_fj means_invvars[g_fj] (inv_vars), sum_j p_fj"""
    p = np.asarray(post, np.float64)
    mi = np.asarray(means_invvars, np.float64)[sel]
    iv = np.asarray(inv_vars, np.float64)[sel]
    return (p[..., None] * mi).sum(axis=1), (p[..., None] * iv).sum(axis=1), p.sum(axis=1)


def fmllr_stats(x, sel, post, means_invvars, inv_vars, fast=False):
    """(beta, K [D, D+1], G [D, D+1, D+1]) of one segment.  `fast`: G as one matrix product of b^T with the
    frames' outer products x+ x+^T (the same float64 sums over the frames, for long segments at large D)"""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    if x.shape[0] == 0:
        return 0.0, np.zeros((D, D + 1)), np.zeros((D, D + 1, D + 1))
    a, b, count = frame_terms(sel, post, means_invvars, inv_vars)
    xp = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)
    K = a.T @ xp
    if fast:
        outer = (xp[:, :, None] * xp[:, None, :]).reshape(x.shape[0], -1)
        return float(count.sum()), K, (b.T @ outer).reshape(D, D + 1, D + 1)
    G = np.einsum('fd,fk,fl->dkl', b, xp, xp)
    return float(count.sum()), K, G


def fmllr_stats_loop(x, sel, post, means_invvars, inv_vars):
    """The same, frame by frame as the reference's accumulate_from_posteriors_preselect loop"""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    beta, K, G = 0.0, np.zeros((D, D + 1)), np.zeros((D, D + 1, D + 1))
    for f in range(x.shape[0]):
        a, b, c = np.zeros(D), np.zeros(D), 0.0
        for g, p in zip(sel[f], post[f]):
            a += float(p) * np.asarray(means_invvars[g], np.float64)
            b += float(p) * np.asarray(inv_vars[g], np.float64)
            c += float(p)
        xp = np.append(x[f], 1.0)
        beta += c
        K += np.outer(a, xp)
        for d in range(D):
            G[d] += b[d] * np.outer(xp, xp)
    return beta, K, G


def apply_transform_to_stats(A, stats, fast=False):
    """ApplyFeatureTransformToStats with A [D, D] (or [D, D+1]).  `fast`: G'_d = (Ahat G_d) Ahat^T as two
    matrix products per row instead of the five-index sum (the same sums in another association: large D)"""
    beta, K, G = stats
    D = K.shape[0]
    Ah = np.eye(D + 1)
    Ah[:D, :A.shape[1]] = A
    if fast:
        return beta, K @ Ah.T, np.matmul(np.matmul(Ah, G), Ah.T)
    return beta, K @ Ah.T, np.einsum('ik,dkl,jl->dij', Ah, G, Ah)


def aux(W, stats):
    """FmllrAuxFuncDiagGmm: beta log|det W_A| + tr(W K^T) - 1/2 sum_d W_d G_d W_d^T"""
    beta, K, G = stats
    W = np.asarray(W, np.float64)
    D = K.shape[0]
    _, ld = np.linalg.slogdet(W[:, :D])
    return beta * ld + np.sum(W * K) - 0.5 * np.einsum('dk,dkl,dl->', W, G, W)


def solve_offset(stats):
    beta, K, G = stats
    D = K.shape[0]
    W = np.concatenate([np.eye(D), np.zeros((D, 1))], axis=1)
    for i in range(D):
        W[i, D] = (K[i, D] - G[i][D, i]) / G[i][D, D]
    return W


def solve_diag(stats):
    beta, K, G = stats
    D = K.shape[0]
    W = np.concatenate([np.eye(D), np.zeros((D, 1))], axis=1)
    for i in range(D):
        gdd, gdD, gDD = G[i][i, i], G[i][i, D], G[i][D, D]
        aq = gdd - gdD * gdD / gDD
        bq = K[i, i] - K[i, D] * gdD / gDD
        s = (bq + np.sqrt(bq * bq + 4 * aq * beta)) / (2 * aq)
        W[i, i] = s
        W[i, D] = (K[i, D] - s * gdD) / gDD
    return W


def compose(T, A):
    """ComposeTransforms(T affine [D, D+1], A linear [D, D]) = [T_A A | t]"""
    D = A.shape[0]
    return np.concatenate([T[:, :D] @ A, T[:, D:]], axis=1)


def compute_transform(As, logdets, stats, norm_type, logdet_scale, default_class, fast=False):
    """LinearVtln::ComputeTransform: (objectives [C], class, impr, count, W [D, D+1]).  `fast`: see
    apply_transform_to_stats"""
    beta, K, G = stats
    D = K.shape[0]
    if beta == 0.0:
        W = np.concatenate([np.asarray(As[default_class], np.float64), np.zeros((D, 1))], axis=1)
        return np.zeros(len(As)), default_class, 0.0, 0.0, W
    ident = np.concatenate([np.eye(D), np.zeros((D, 1))], axis=1)
    old = aux(ident, stats)
    objs, Ws = [], []
    for c, A in enumerate(As):
        A = np.asarray(A, np.float64)
        st = apply_transform_to_stats(A, stats, fast)
        if norm_type == 'none':
            T = ident
        elif norm_type == 'offset':
            T = solve_offset(st)
        else:
            T = solve_diag(st)
        W = compose(T, A)
        objs.append(aux(W, stats) + (logdet_scale - 1.0) * beta * logdets[c])
        Ws.append(W)
    objs = np.asarray(objs)
    best = int(np.argmax(objs))
    return objs, best, objs[best] - old, beta, Ws[best]


def mapping_transform(x, y, w=None):
    """compute_mapping_transform (reference vtln.py:299-376): A [D, D]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    F, D = x.shape
    w = np.ones(F) if w is None else np.asarray(w, np.float64)
    xp = np.concatenate([x, np.ones((F, 1))], axis=1)
    Q = (xp * w[:, None]).T @ xp
    l = (y * w[:, None]).T @ xp
    beta = w.sum()
    sum_xplus = w @ xp
    sumsq_x = w @ (x * x)
    A = np.zeros((D, D))
    Qinv = np.linalg.inv(Q)
    for i in range(D):
        wi = Qinv @ l[i]
        x_var = sumsq_x[i] / beta - (sum_xplus[i] / beta) ** 2
        y_var = wi @ Q @ wi / beta - (wi @ sum_xplus / beta) ** 2
        A[i] = wi[:D] * np.sqrt(x_var / y_var)
    return A


def logdet(A):
    return float(np.linalg.slogdet(np.asarray(A, np.float64))[1])


def replay(x_segments, sel_segments, ubm_gmm, As, warps, norm_type, logdet_scale, default_class, num_iters,
           em_step, posteriors):
    """process()'s loop from the original frames, the selection and a UBM: `em_step(gmm, frames)` updates
    the model in place, `posteriors(gmm, frames, sel)` returns the selection posteriors.  Returns the
    per-segment (classes, transforms, objectives) of the last estimate."""
    lds = [logdet(A) for A in As]

    def estimate(posts):
        out = []
        for x, sel, p in zip(x_segments, sel_segments, posts):
            st = fmllr_stats(x, sel, p, ubm_gmm.means_invvars_, ubm_gmm.inv_vars_)
            out.append(compute_transform(As, lds, st, norm_type, logdet_scale, default_class))
        return out

    res = estimate([posteriors(ubm_gmm, x, s) for x, s in zip(x_segments, sel_segments)])
    for _ in range(num_iters):
        ys = [(np.asarray(x, np.float32) @ r[4][:, :-1].astype(np.float32).T + r[4][:, -1].astype(np.float32))
              for x, r in zip(x_segments, res)]
        em_step(ubm_gmm, np.concatenate(ys, axis=0))
        res = estimate([posteriors(ubm_gmm, y, s) for y, s in zip(ys, sel_segments)])
    return res
