"""Data shared by the detection tests (tests/test_dtw_detect.py, tests/test_dtw_detect_gpu.py) and by
tools/time_dtw_detect.py, on top of tests/dtw_search_cases.py: a target with three planted copies of a query, and the
statement (tests/dtw_detect_f64.py) of a whole case as the arrays that snf_dtw_detect writes."""

import numpy as np

import dtw_detect_f64
import dtw_search_cases

PLANTED_GAPS = ((5, 7, 40, 3), (0, 1, 1, 0), (40, 30, 64, 70))   # rows of 9s before, between and behind the copies
PLANTED_FRAMES = 20


def planted_three(gaps, seed, dim=3, frames=PLANTED_FRAMES):
    """(query [frames, dim], target, first rows of the three copies): integer rows; the target is rows of 9s, the
    query, 9s, the query, 9s, the query, 9s, the four stretches of 9s `gaps` rows long"""
    query, _ = dtw_search_cases.planted(frames, 0, 0, dim, seed)
    nines = lambda k: np.full((k, dim), 9, dtype=np.float32)   # noqa: E731
    parts, firsts, row = [], [], 0
    for k, gap in enumerate(gaps):
        parts.append(nines(gap))
        row += gap
        if k < 3:
            parts.append(query)
            firsts.append(row)
            row += frames
    return query, np.concatenate(parts, axis=0), firsts


def slots(answer, k, normalized, max_score=None, dtype=np.float32):
    """(count, cost [k], length [k], start [k], end [k]) of a pair as snf_dtw_detect writes them, sentinels
    included, from the statement's last rows (a dtw_search_cases.Answer or anything with cost, length, start)"""
    found = dtw_detect_f64.detections(answer.cost, answer.length, answer.start, k, normalized, max_score, dtype)
    cost = np.full(k, np.inf, dtype=np.float32)
    length = np.zeros(k, dtype=np.int32)
    start, end = np.full(k, -1, dtype=np.int32), np.full(k, -1, dtype=np.int32)
    for r, (_, c, n, b, e) in enumerate(found):
        cost[r], length[r], start[r], end[r] = c, n, b, e
    return len(found), cost, length, start, end
