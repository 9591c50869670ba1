"""The float64 statement of the subsequence DTW search that snf_dtw_search computes (shennong_amd/dtw.py
``dtw_search``)

For a query x [N, D] and a target y [M, D] (float32 rows, N, M >= 1), with d[i, j] the frame distance of
tests/dtw_f64.py (`cosine`, `sqeuclidean`) or tests/symkl_f64.py (`symkl`), in float64 on the float32 values:

    C[0, j] = d[0, j],  L[0, j] = 1,  B[0, j] = j          for every j   (free start)
    i >= 1: C[i, j] = d[i, j] + C[p], L[i, j] = L[p] + 1, B[i, j] = B[p]
            p = the predecessor of smallest C among (i-1, j-1), (i-1, j), (i, j-1) that exist, ties to the first of
            that order
    score[j] = C[N-1, j] / L[N-1, j] if normalized else C[N-1, j]          (free end)
    end = the smallest j of minimal score;  start = B[N-1, end];  cost = C[N-1, end];  length = L[N-1, end]

As in tests/dtw_f64.py the dynamic programme minimises C: the normalisation only ranks the ends, it does not look
for the path of smallest mean.  `tables_loop` is the plain double loop, `tables` the same recursion one
anti-diagonal at a time (equal bit for bit: the same float64 additions and comparisons).  `end_margins` says, for
every end, how close its path comes to a decision that would change its length or its start."""

import numpy as np

import dtw_f64
import symkl_f64

METRICS = ('cosine', 'sqeuclidean', 'symkl')


def frame_distances(x, y, metric='cosine'):
    """d [N, M] in float64"""
    if metric == 'symkl':
        return symkl_f64.frame_distances(x, y)
    return dtw_f64.frame_distances(x, y, metric)


def tables_loop(d):
    """(C, L, B) by the plain double loop"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    C = np.zeros((n, m), dtype=np.float64)
    L = np.zeros((n, m), dtype=np.int64)
    B = np.zeros((n, m), dtype=np.int64)
    for j in range(m):
        C[0, j], L[0, j], B[0, j] = d[0, j], 1, j
    for i in range(1, n):
        for j in range(m):
            best = None
            for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if b >= 0 and (best is None or C[a, b] < C[best]):
                    best = (a, b)
            C[i, j] = d[i, j] + C[best]
            L[i, j] = L[best] + 1
            B[i, j] = B[best]
    return C, L, B


def tables(d):
    """(C, L, B) one anti-diagonal at a time: every cell of i + j = t, i >= 1, depends on the diagonals t - 1 and
    t - 2 only"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    # (a border of +inf stands for the predecessors that do not exist: cell (i, j) is at [i, j + 1])
    C = np.full((n, m + 1), np.inf)
    L = np.zeros((n, m + 1), dtype=np.int64)
    B = np.zeros((n, m + 1), dtype=np.int64)
    C[0, 1:], L[0, 1:], B[0, 1:] = d[0], 1, np.arange(m)
    for t in range(1, n + m - 1):
        i = np.arange(max(1, t - m + 1), min(n - 1, t) + 1)
        j = t - i
        bc, bl, bb = C[i - 1, j], L[i - 1, j], B[i - 1, j]                  # (i - 1, j - 1)
        uc, ul, ub = C[i - 1, j + 1], L[i - 1, j + 1], B[i - 1, j + 1]      # (i - 1, j)
        take = uc < bc
        bc, bl, bb = np.where(take, uc, bc), np.where(take, ul, bl), np.where(take, ub, bb)
        lc, ll, lb = C[i, j], L[i, j], B[i, j]                              # (i, j - 1)
        take = lc < bc
        bc, bl, bb = np.where(take, lc, bc), np.where(take, ll, bl), np.where(take, lb, bb)
        C[i, j + 1] = d[i, j] + bc
        L[i, j + 1] = bl + 1
        B[i, j + 1] = bb
    return C[:, 1:], L[:, 1:], B[:, 1:]


def scores(cost, length, normalized=True, dtype=np.float64):
    """score [M] of every end from the last rows of C and L, the division in `dtype` (np.float32: the device's)"""
    cost = np.asarray(cost).astype(dtype)
    return cost / np.asarray(length).astype(dtype) if normalized else cost


def best_end(cost, length, start, normalized=True, dtype=np.float64):
    """(score, cost, length, start, end) of the smallest end of minimal score: a strict < over ascending j"""
    score = scores(cost, length, normalized, dtype)
    end = int(np.argmin(score))   # (the first of the minimal ones)
    return score[end], cost[end], int(length[end]), int(start[end]), end


def search(x, y, metric='cosine', normalized=True, loop=False):
    """(score, cost, length, start, end) of the query x in the target y, float64 and ints"""
    C, L, B = (tables_loop if loop else tables)(frame_distances(x, y, metric))
    return best_end(C[-1], L[-1], B[-1], normalized)


def end_margins_loop(C, L, B):
    """margin [M]: for every end j, follows the path back from (N-1, j) to row 0.  At each of its cells: the gap
    between the chosen predecessor's C and any other predecessor whose (L, B) differs from the chosen one's.  The
    smallest gap along the path (inf when no cell has such a predecessor): below it, a perturbation of C cannot
    change L or B of that end."""
    n, m = C.shape
    margins = np.full(m, np.inf)
    for end in range(m):
        i, j = n - 1, end
        while i > 0:
            preds = [(a, b) for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if b >= 0]
            best = preds[0]
            for p in preds[1:]:
                if C[p] < C[best]:
                    best = p
            for p in preds:
                if p != best and (L[p], B[p]) != (L[best], B[best]):
                    margins[end] = min(margins[end], float(C[p] - C[best]))
            i, j = best
    return margins


def end_margins(C, L, B):
    """`end_margins_loop` for all the ends at once: the margin of a cell is the smaller of its own gap and the
    margin of its chosen predecessor, which is the minimum along the path that a walk back from the cell follows.
    One anti-diagonal at a time, as `tables`."""
    n, m = C.shape
    pad = lambda a, fill: np.concatenate([np.full((n, 1), fill, dtype=a.dtype), a], axis=1)   # noqa: E731
    C, L, B = pad(np.asarray(C, dtype=np.float64), np.inf), pad(np.asarray(L), -1), pad(np.asarray(B), -1)
    G = np.full((n, m + 1), np.inf)
    for t in range(1, n + m - 1):
        i = np.arange(max(1, t - m + 1), min(n - 1, t) + 1)
        j = t - i
        cand = [(C[a, b], L[a, b], B[a, b], G[a, b]) for a, b in ((i - 1, j), (i - 1, j + 1), (i, j))]
        bc, bl, bb, bg = cand[0]
        for c, l, b, g in cand[1:]:
            take = c < bc
            bc, bl, bb, bg = np.where(take, c, bc), np.where(take, l, bl), np.where(take, b, bb), np.where(take, g, bg)
        gap = np.full(i.shape, np.inf)
        for c, l, b, _ in cand:
            # (the chosen one differs from itself in nothing; a predecessor that does not exist has C = inf)
            differs = (l != bl) | (b != bb)
            gap = np.where(differs, np.minimum(gap, c - bc), gap)
        G[i, j + 1] = np.minimum(bg, gap)
    return G[-1, 1:]
