"""tests/pitch_state_cases.py is what it claims, on the CPU: every state count comes out of the oracle's lag ladder,
every run takes the route the table expects (the ladder as tests/test_pitch_route.py states it), every utterance has
its frames, the glide reaches both ends of the state space, the refusal sits where the LDS ends, and the first
frame of an utterance at the largest state counts fills the long-window queue of refine_levels to its last entry."""
import numpy as np
import pytest

import pitch_state_cases as pc
from oracle import oracle as orc
from test_pitch_route import BY_STATE, FLAT, LDS_LIMIT, TEAM, _route, _state_lds


def test_every_entry_has_its_state_count():
    for S, delta in pc.DELTA_PITCH.items():
        assert float(np.float32(delta)) == delta, S        # a float32, as the option record holds it
        lags, first_lag, last_lag = orc.pitch_lags(pc.oracle_options(S))
        assert lags.shape[0] == S
        assert (first_lag, last_lag) == (8, 82)            # the NCCF of the default options
        assert pc.options_kwargs(S) == dict(min_f0=50.0, max_f0=400.0, delta_pitch=delta)
    assert set(pc.DELTA_PITCH) == set(pc.ALL_S) | {pc.REFUSED_S}


@pytest.mark.parametrize('S', [2, 129, 448, 1460])
def test_the_helper_finds_a_state_count(S):
    delta = pc.find_delta_pitch(S)
    assert pc.num_states(delta) == S
    # ... away from both ends of the interval of delta_pitch that gives S
    assert pc.num_states(float(np.float32(delta * (1 + 1e-5)))) == S == pc.num_states(float(np.float32(delta * (1 - 1e-5))))
    assert delta == pc.DELTA_PITCH[S]


def test_the_table_has_the_counts_the_seams_need():
    assert {2, 33, 64, 65, 127, 128, 129, 256, 257, 384, 385, 447, 448} <= set(pc.STATE_7)
    assert {449, 511, 512} <= set(pc.STATE_8) and {513, 641, 1460} <= set(pc.STATE_0)
    assert set(pc.TEAM_S) == {128, 129, 256, 257, 384, 385, 448, 449, 511, 512}
    assert {129, 130, 131, 132, 160, 161, 256, 257, 385} | set(range(441, 449)) <= set(pc.FLAT_S)
    assert max(pc.STATE_7) == 448 < min(pc.STATE_8) and max(pc.STATE_8) == 512 < min(pc.STATE_0)
    for S in pc.ALL_S:
        runs = pc.forms_at(S)
        assert 'state' in runs, S
        assert ('team2' in runs) == ('team4' in runs) == (S in pc.TEAM_S)
        assert ('flat' in runs) == (S in pc.FLAT_S)
        assert ('team2_ignored' in runs) == (S in pc.TEAM_IGNORED_S)
        assert ('flat_ignored' in runs) == (S in pc.FLAT_IGNORED_S)


def test_every_run_takes_the_route_it_expects():
    seen = set()
    for S, name in pc.GPU_CASES:
        team, flat, form, waves, nk = pc.forms_at(S)[name]
        for n_utts in pc.UTT_COUNTS:
            got = _route(S, n_utts, team, flat)
            assert got[:3] == (form, waves, nk) and not got[4], (S, name, n_utts)
            assert got[3] <= LDS_LIMIT
        seen.add((form, waves, nk))
        # a knob the route ignores: the run is the by-state form, the one the `state` run of that count takes
        if name.endswith('_ignored'):
            assert form == BY_STATE == pc.forms_at(S)['state'][2]
    assert seen == {(TEAM, 2, -1), (TEAM, 4, -1), (FLAT, 8, -1), (BY_STATE, 8, 7), (BY_STATE, 8, 8), (BY_STATE, 8, 0)}
    assert (pc.BY_STATE, pc.TEAM, pc.FLAT) == (BY_STATE, TEAM, FLAT)


def test_refusal_sits_where_the_lds_ends():
    """(nothing to compare at the refused count: only where it lies)"""
    s4 = lambda S: (S + 3) & ~3
    assert _state_lds(s4(pc.LDS_LIMIT_S)) <= LDS_LIMIT < _state_lds(s4(pc.REFUSED_S))
    assert pc.REFUSED_S == pc.LDS_LIMIT_S + 1 == max(pc.ALL_S) + 1
    assert _route(pc.REFUSED_S, 17, '1', '0')[4] and not _route(pc.LDS_LIMIT_S, 17, '1', '0')[4]
    # (a forced team does not rescue it: above 512 states the route runs by state)
    assert _route(pc.REFUSED_S, 17, '4', None)[4]


def test_utterances_have_their_frames():
    for S in (2, 448, 1460):
        po = pc.oracle_options(S)
        for frames, samples in pc.FRAMES_TO_SAMPLES.items():
            assert orc.pitch_num_frames(po, samples) == frames
            if frames:   # the shortest utterance with that many
                assert orc.pitch_num_frames(po, samples - 1) == frames - 1
        for i, (kind, frames) in enumerate(pc.MASTER):
            assert orc.pitch_num_frames(po, pc.utterance(i).shape[0]) == frames, (S, i)
        for i in pc.HOLES:
            assert orc.pitch_num_frames(po, pc.too_short(i).shape[0]) == 0
    assert {frames for _, frames in pc.MASTER} == {1, 2, 63, 64, 65, 128, 129, pc.CLICK_FRAMES}
    assert all(w.dtype == np.int16 and w.shape[0] <= 1.31 * pc.SAMPLE_RATE for i, w in
               enumerate(map(pc.utterance, range(len(pc.MASTER)))) if pc.MASTER[i][0] != 'click')
    assert {kind for kind, _ in pc.MASTER} == set(pc.SIGNALS)


def test_click_is_the_recompute_corner():
    from test_oracle_pins import _click_utterance
    wave = pc.utterance([kind for kind, _ in pc.MASTER].index('click'))
    assert np.array_equal(wave, _click_utterance(pc.CLICK_SAMPLES))
    assert 500 <= pc.CLICK_FRAMES <= 502     # tests/test_oracle_pins.py test_pitch_recompute_backtraces_corner


def test_batches():
    assert [len(pc.batch(name)) for name in pc.BATCHES] == [1, 7, 8, 9, 17, 17]
    holes = pc.batch('holes')
    assert [i for i, u in enumerate(holes) if u < 0] == [3, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    assert all(u == i for i, u in enumerate(holes) if u >= 0)
    # longest first, as the tracker deals the utterances out: the seven that work fill slots 0 .. 6
    frames = [pc.MASTER[u][1] if u >= 0 else 0 for u in holes]
    order = sorted(range(17), key=lambda u: -frames[u])
    assert [frames[u] > 0 for u in order] == [True] * 7 + [False] * 10
    assert all(pc.wanted(2, u).shape == ((0, 0) if u < 0 else (pc.MASTER[u][1], 2)) for u in holes)


@pytest.mark.parametrize('S', [33, 1460])
def test_glide_reaches_both_ends(S):
    """the smallest count at which a path can move (pitch_state_cases.glide) and the largest"""
    for index, (kind, _) in enumerate(pc.MASTER):
        if kind == 'glide':
            states = orc.pitch_debug(pc.oracle_options(S), pc.utterance(index))[4]
            assert states.min() == 0 and states.max() == S - 1, (index, states.min(), states.max())


def test_glide_rests_with_two_states():
    states = orc.pitch_debug(pc.oracle_options(2), pc.utterance(8))[4]
    assert np.unique(states).shape[0] == 1


def test_tie_cases():
    """penalty_factor = 0 on digital silence: every candidate ties, and the oracle's path is state 0 throughout"""
    assert set(pc.TIE_S) <= set(pc.ALL_S) and pc.TIE_PENALTY == 0.0
    assert {name for _, name in pc.TIE_CASES} == {'state', 'team2', 'team4', 'flat'}
    assert len(pc.TIE_FRAMES) == 17 and set(pc.TIE_FRAMES) == set(pc.FRAMES_TO_SAMPLES)
    assert not any(w.any() for w in pc.tie_waves())
    for S in pc.TIE_S:
        po = pc.oracle_options(S, penalty_factor=pc.TIE_PENALTY)
        lags = orc.pitch_lags(po)[0]
        for frames, wave, want in zip(pc.TIE_FRAMES, pc.tie_waves(), pc.tie_wanted(S)):
            assert orc.pitch_num_frames(po, wave.shape[0]) == frames
            if frames:
                assert not orc.pitch_debug(po, wave)[4].any()
                assert want.shape == (frames, 2) and np.all(want[:, 1] == np.float32(1.0) / lags[0])
            else:
                assert want.size == 0


def _kaldi_search(prev, factor):
    """PitchFrameInfo::ComputeBacktraces as oracle/kaldi_oracle.c compute_backtraces states it (backpointers only)"""
    S = len(prev)
    cost = lambda i, j: (j - i) ** 2 * factor + prev[j]
    bp, fw, lo, hi, last = [0] * S, [0.0] * S, [0] * S, [S - 1] * S, 0
    for i in range(S):
        best_j = last
        for j in range(last + 1, S):
            if cost(i, j) < cost(i, best_j):
                best_j = j
            else:
                break
        bp[i], fw[i], lo[i], last = best_j, cost(i, best_j), best_j, best_j
    for sweep in range(S):
        changed = False
        down = sweep % 2 == 0
        last = S - 1 if down else 0
        for i in (range(S - 1, -1, -1) if down else range(S)):
            lower, upper = (lo[i], min(last, hi[i])) if down else (max(last, lo[i]), hi[i])
            best_j = bp[i]
            if upper == lower or best_j == (upper if down else lower):
                last = lower if upper == lower else best_j
                continue
            for j in (range(upper, lower + 1, -1) if down else range(lower, upper - 1)):
                if cost(i, j) < fw[i]:
                    fw[i], best_j = cost(i, j), j
                elif (best_j > j) if down else (best_j < j):
                    break
            if down:
                hi[i] = best_j
            else:
                lo[i] = best_j
            changed |= best_j != bp[i]
            bp[i] = last = best_j
        if not changed:
            break
    return bp


def test_kaldi_search_on_partial_ties():
    """why the tie batch is silence only: with no transition cost and forward costs that tie in part, Kaldi's search
    does not return the first minimum - its backward sweep walks down from the last state and keeps the higher of
    two tied minima.  With the default penalty, and on all-equal costs, it is the first minimum."""
    prev = [3.0, 2.0, 2.0, 5.0, 1.0, 1.0, 4.0, 0.0, 0.0, 3.0] + [3.0] * 22
    assert prev.index(min(prev)) == 7 and _kaldi_search(prev, 0.0) == [8] * 32
    assert _kaldi_search([1.0] * 32, 0.0) == [0] * 32
    factor = float(np.float32(0.1) * np.float32(np.log(1.005)) ** 2)
    exact = [min(range(32), key=lambda j: ((j - i) ** 2 * factor + prev[j], j)) for i in range(32)]
    assert _kaldi_search(prev, factor) == exact


# ---- the long-window queue -----------------------------------------------------------------------------------------
NOISE_128, GLIDE_129, SILENCE_2 = 11, 8, 5


def test_signals_of_the_queue_cases():
    assert [pc.MASTER[i] for i in (NOISE_128, GLIDE_129, SILENCE_2)] == [('noise', 128), ('glide', 129), ('silence', 2)]


@pytest.mark.parametrize('S, index, penalty', [(512, NOISE_128, 0.1), (512, GLIDE_129, 0.1), (512, NOISE_128, 0.01),
                                               (512, NOISE_128, 0.001), (1460, NOISE_128, 0.1),
                                               (1460, GLIDE_129, 0.1), (1460, NOISE_128, 0.01),
                                               (1460, GLIDE_129, 0.001)])
def test_long_windows_of_levels_4_and_5_stay_under_a_pass(S, index, penalty):
    """noise and the glide, the default penalty and small ones: levels 4 and 5 never queue more than 64 windows in a
    frame (the largest seen: 51, level 5, 1460 states), so only level 3 can make a wave work its queue off early"""
    _, worst, queued, mid_level = pc.long_windows(pc.oracle_options(S, penalty_factor=penalty), pc.utterance(index))
    print(S, pc.MASTER[index], penalty, 'long windows per frame', worst, 'queue', queued, 'mid-level', mid_level)
    assert max(worst[4], worst[5]) <= 64 and mid_level[4] == mid_level[5] == 0
    # level 3 of the first frame: bp[i] = i, every window between two known states is exactly kLongRange3 long
    assert len(pc.level_states(3, S)[0]) == ((S + 7) >> 3) - ((S + 31) >> 5)
    assert worst[3] == len(pc.first_frame_long(S)) >= len(pc.level_states(3, S)[0]) - 3
    assert (mid_level[3] > 0) == (S == 1460)


@pytest.mark.parametrize('S, flushes_early', [(1025, False), (1368, False), (1369, True), (1460, True)])
def test_first_frame_fills_the_queue(S, flushes_early):
    """the case that reaches the flush in the middle of a level: ANY utterance from 1369 states on, in its first
    frame, and digital silence in every frame (here: two frames of silence)"""
    frames, worst, queued, mid_level = pc.long_windows(pc.oracle_options(S), pc.utterance(SILENCE_2))
    count, n_long = len(pc.level_states(3, S)[0]), len(pc.first_frame_long(S))
    assert frames == 2 and worst[3] == n_long and worst[4] == worst[5] == 0
    # (the queue is looked at after every pass of 64 states: never more than kQueueEntries in it)
    assert queued[3] == min(n_long, pc.QUEUE_ENTRIES)
    assert mid_level[3] == (frames if flushes_early else 0)
    assert (count > pc.QUEUE_ENTRIES) == flushes_early and n_long > pc.QUEUE_ENTRIES - 64
