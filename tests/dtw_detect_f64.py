"""The float64/int statement of the detections that snf_dtw_detect picks and of the selection that snf_dtw_topk makes
(shennong_amd/dtw.py ``dtw_detect``), on top of tests/dtw_search_f64.py

The inputs are the last rows (cost [M], length [M], start [M]) of the lattice of a (query, target) pair (`tables` of
tests/dtw_search_f64.py).  With the score of the search,

    score[j] = cost[j] / length[j] in `dtype` if normalized else cost[j]

the detections are a greedy non-maximum suppression over the ends.  Every end is alive at first; then, until k
detections are made or no end is alive:

    1. e = the smallest alive j of minimal score (a strict < over ascending j, as `best_end`)
    2. if max_score is given and not score[e] <= max_score (compared in `dtype`): stop
    3. (score[e], cost[e], length[e], start[e], e) is the detection of the next rank
    4. every end j' whose path interval [start[j'], j'] shares a frame with [start[e], e] dies:
       start[j'] <= e and j' >= start[e] (e itself among them)

The detections of a pair come in ascending score, their intervals are pairwise disjoint, and rank 0 is the match of
the search.  The definition is this project's own; agreement with any outside toolkit is not pinned.
`detections_loop` is the plain loop, `detections` the same steps on whole arrays.

`top_k`: for every query the first t of the detections of its pairs in the order (score ascending in float32, then
the pair's index in the caller's order, then the rank): a plain stable sort."""

import numpy as np

import dtw_search_f64


def detections_loop(cost, length, start, k, normalized=True, max_score=None, dtype=np.float64):
    """[(score, cost, length, start, end)] by the plain loops"""
    score = dtw_search_f64.scores(cost, length, normalized, dtype)
    m = score.shape[0]
    alive = [True] * m
    found = []
    while len(found) < k:
        e = None
        for j in range(m):
            if alive[j] and (e is None or score[j] < score[e]):
                e = j
        if e is None:
            break
        if max_score is not None and not score[e] <= dtype(max_score):
            break
        found.append((score[e], cost[e], int(length[e]), int(start[e]), e))
        for j in range(m):
            if start[j] <= e and j >= start[e]:
                alive[j] = False
    return found


def detections(cost, length, start, k, normalized=True, max_score=None, dtype=np.float64):
    """[(score, cost, length, start, end)], every step on whole arrays"""
    score = dtw_search_f64.scores(cost, length, normalized, dtype)
    start = np.asarray(start)
    ends = np.arange(score.shape[0])
    alive = np.ones(score.shape[0], dtype=bool)
    found = []
    while len(found) < k and alive.any():
        live = ends[alive]
        e = int(live[np.argmin(score[live])])   # (the first of the minimal ones)
        if max_score is not None and not score[e] <= dtype(max_score):
            break
        found.append((score[e], cost[e], int(length[e]), int(start[e]), e))
        alive &= ~((start <= e) & (ends >= start[e]))
    return found


def top_k(detections_of_pairs, query_of_pair, t):
    """{query: [(pair, rank)] of its t best detections}: `detections_of_pairs[p]` are the detections of pair p in the
    caller's order, `query_of_pair[p]` its query"""
    best = {}
    for q in sorted(set(int(q) for q in query_of_pair)):
        mine = [(np.float32(found[0]), p, r) for p, q_of_p in enumerate(query_of_pair) if int(q_of_p) == q
                for r, found in enumerate(detections_of_pairs[p])]
        mine.sort(key=lambda key: (float(key[0]), key[1], key[2]))
        best[q] = [(p, r) for _, p, r in mine[:t]]
    return best
