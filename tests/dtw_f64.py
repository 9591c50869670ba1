"""The float64 statement of the DTW distance that snf_dtw_pairs computes (shennong_amd/dtw.py)

For the items x [N, D] and y [M, D] (float32 rows, N, M >= 1), in float64 on the float32 values:

    cosine       d[i, j] = arccos(clip(x_i.y_j / (|x_i| |y_j|), -1, 1)) / pi
                 d = 1 when exactly one of the two rows has zero norm, 0 when both have
    sqeuclidean  d[i, j] = sum_k (x_ik - y_jk)^2

    C[0, 0] = d[0, 0], L[0, 0] = 1
    C[i, j] = d[i, j] + C[p], L[i, j] = L[p] + 1, p the predecessor of smallest C among (i-1, j-1), (i-1, j),
    (i, j-1) where they exist, ties to the first of that order

    cost = C[N-1, M-1], length = L[N-1, M-1], distance = cost / length if normalized else cost

`tables_loop` is the plain double loop, `tables` the same recursion one anti-diagonal at a time (equal bit for
bit: the same float64 additions and comparisons), `path_margin` how close the optimal path comes to a decision
that would change its length."""

import numpy as np

METRICS = ('cosine', 'sqeuclidean')


def frame_distances(x, y, metric='cosine'):
    """d [N, M] in float64"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    if metric == 'sqeuclidean':
        # (256 rows of x at a time: the differences of a 4096-frame item would not fit at once)
        return np.concatenate([((x[a:a + 256, None, :] - y[None, :, :]) ** 2).sum(axis=2)
                               for a in range(0, x.shape[0], 256)], axis=0)
    if metric != 'cosine':
        raise ValueError(metric)
    nx, ny = np.sqrt((x * x).sum(axis=1)), np.sqrt((y * y).sum(axis=1))
    zx, zy = nx == 0, ny == 0
    scale = np.where(zx, 1.0, nx)[:, None] * np.where(zy, 1.0, ny)[None, :]
    d = np.arccos(np.clip((x @ y.T) / scale, -1.0, 1.0)) / np.pi
    one = zx[:, None] ^ zy[None, :]
    both = zx[:, None] & zy[None, :]
    return np.where(both, 0.0, np.where(one, 1.0, d))


def tables_loop(d):
    """(C, L) by the plain double loop"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    C = np.zeros((n, m), dtype=np.float64)
    L = np.zeros((n, m), dtype=np.int64)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                C[0, 0], L[0, 0] = d[0, 0], 1
                continue
            best = None
            for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if a >= 0 and b >= 0 and (best is None or C[a, b] < C[best]):
                    best = (a, b)
            C[i, j] = d[i, j] + C[best]
            L[i, j] = L[best] + 1
    return C, L


def tables(d):
    """(C, L) one anti-diagonal at a time: every cell of i + j = t depends on the diagonals t - 1 and t - 2 only"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    # (a border of +inf stands for the predecessors that do not exist: cell (i, j) is at [i + 1, j + 1])
    C = np.full((n + 1, m + 1), np.inf)
    L = np.zeros((n + 1, m + 1), dtype=np.int64)
    C[1, 1], L[1, 1] = d[0, 0], 1
    for t in range(1, n + m - 1):
        i = np.arange(max(0, t - m + 1), min(n - 1, t) + 1)
        j = t - i
        bc, bl = C[i, j], L[i, j]                       # (i - 1, j - 1)
        uc, ul = C[i, j + 1], L[i, j + 1]               # (i - 1, j)
        take = uc < bc
        bc, bl = np.where(take, uc, bc), np.where(take, ul, bl)
        lc, ll = C[i + 1, j], L[i + 1, j]               # (i, j - 1)
        take = lc < bc
        bc, bl = np.where(take, lc, bc), np.where(take, ll, bl)
        C[i + 1, j + 1] = d[i, j] + bc
        L[i + 1, j + 1] = bl + 1
    return C[1:, 1:], L[1:, 1:]


def dtw(x, y, metric='cosine', normalized=True, loop=False):
    """(distance, length) of the pair, float64 and int"""
    C, L = (tables_loop if loop else tables)(frame_distances(x, y, metric))
    cost, length = float(C[-1, -1]), int(L[-1, -1])
    return (cost / length if normalized else cost), length


def path_margin(d, made=None):
    """Follows the optimal path back from (N-1, M-1).  At each of its cells: the gap between the chosen
    predecessor's C and the nearest other predecessor whose L differs from the chosen one's.  Returns the
    smallest gap along the path (inf when no cell has such a predecessor): below it, a perturbation of C
    cannot change the length of the path.  `made`: the (C, L) of `d` where the caller has them."""
    C, L = tables(d) if made is None else made
    i, j = C.shape[0] - 1, C.shape[1] - 1
    margin = np.inf
    while i > 0 or j > 0:
        preds = [(a, b) for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if a >= 0 and b >= 0]
        best = preds[0]
        for p in preds[1:]:
            if C[p] < C[best]:
                best = p
        for p in preds:
            if p != best and L[p] != L[best]:
                margin = min(margin, float(C[p] - C[best]))
        i, j = best
    return margin
