"""The statement of the ABX scores that ``shennong_amd.abx.abx_scores`` and snf_abx_cells compute,
with plain loops straight from the item labels: nothing here reuses the product's cell construction.

    a triplet (A, B, X): three distinct items, equal on every `by` column, on(A) == on(X) != on(B) and, with
    `across`, ac(A) == ac(B) != ac(X)
    its cell: (by values, on(A), on(B)[, ac(A), ac(X)])
    per cell: n triplets, less = #{d(A, X) < d(B, X)}, equal = #{d(A, X) == d(B, X)}, bad = #{one of the two is
    not finite} (a bad triplet is in neither other count), score = (less + 0.5 equal) / n in float64

`triplets` enumerates them, `table_rows` counts them per cell through a distance lookup d(Y, X), `cell_counts`
counts one cell of snf_abx_cells from its two sub-matrices by sorting (for cells too large to enumerate) and
`cell_counts_loop` by the plain triple loop, `expand` lists the triplets that cell records address."""

import numpy as np


def triplets(labels, on, across=None, by=()):
    """{cell key: [(A, B, X), ...]} over the items 0 .. n - 1; key = (by values ..., on(A), on(B)[, ac(A), ac(X)])"""
    n = len(labels[on])
    cells = {}
    for a in range(n):
        for b in range(n):
            for x in range(n):
                if a == b or a == x or b == x:
                    continue
                if any(not (labels[c][a] == labels[c][b] == labels[c][x]) for c in by):
                    continue
                if not (labels[on][a] == labels[on][x] and labels[on][a] != labels[on][b]):
                    continue
                key = tuple(labels[c][a] for c in by) + (labels[on][a], labels[on][b])
                if across is not None:
                    if not (labels[across][a] == labels[across][b] and labels[across][a] != labels[across][x]):
                        continue
                    key += (labels[across][a], labels[across][x])
                cells.setdefault(key, []).append((a, b, x))
    return cells


def table_rows(labels, on, across, by, distance):
    """[(key, score, n, less, equal, bad)] sorted by key; `distance(y, x)` = d(item y, item x)"""
    rows = []
    for key, members in sorted(triplets(labels, on, across, by).items()):
        less = equal = bad = 0
        for a, b, x in members:
            dax, dbx = distance(a, x), distance(b, x)
            if not (np.isfinite(dax) and np.isfinite(dbx)):
                bad += 1
            elif dax < dbx:
                less += 1
            elif dax == dbx:
                equal += 1
        n = len(members)
        rows.append((key, (np.float64(less) + 0.5 * np.float64(equal)) / np.float64(n), n, less, equal, bad))
    return rows


def cell_counts_loop(values, record):
    """(less, equal, bad) of the record {offA, offB, stride, nA, nB, nX, same, 0} over the float32 `values`"""
    off_a, off_b, stride, n_a, n_b, n_x, same = [int(v) for v in record[:7]]
    less = equal = bad = 0
    for x in range(n_x):
        for a in range(n_a):
            if same and a == x:
                continue
            dax = values[off_a + x * stride + a]
            for b in range(n_b):
                dbx = values[off_b + x * stride + b]
                if not (np.isfinite(dax) and np.isfinite(dbx)):
                    bad += 1
                elif dax < dbx:
                    less += 1
                elif dax == dbx:
                    equal += 1
    return less, equal, bad


def cell_counts(values, record):
    """The same counts by sorting: per x, the A-row is looked up in the sorted finite part of the B-row"""
    off_a, off_b, stride, n_a, n_b, n_x, same = [int(v) for v in record[:7]]
    less = equal = bad = 0
    for x in range(n_x):
        row_a = values[off_a + x * stride:off_a + x * stride + n_a]
        row_b = values[off_b + x * stride:off_b + x * stride + n_b]
        if same:
            row_a = np.delete(row_a, x)
        fine_a = row_a[np.isfinite(row_a)]
        fine_b = np.sort(row_b[np.isfinite(row_b)])
        lo = np.searchsorted(fine_b, fine_a, side='left')
        hi = np.searchsorted(fine_b, fine_a, side='right')
        less += int((fine_b.shape[0] - hi).sum())
        equal += int((hi - lo).sum())
        bad += row_a.shape[0] * n_b - fine_a.shape[0] * fine_b.shape[0]
    return less, equal, bad


def expand(pairs, records):
    """[(A, B, X)] item triplets that the records address in the pair list `pairs` [P, 2] = (Y, X); asserts that
    the two distances of a triplet share their X"""
    out = []
    for record in np.asarray(records).tolist():
        off_a, off_b, stride, n_a, n_b, n_x, same, zero = record
        assert zero == 0
        found = []
        for x in range(n_x):
            for a in range(n_a):
                if same and a == x:
                    continue
                ya, xa = pairs[off_a + x * stride + a]
                for b in range(n_b):
                    yb, xb = pairs[off_b + x * stride + b]
                    assert xa == xb
                    found.append((int(ya), int(yb), int(xa)))
        out.append(found)
    return out
