"""State counts, batches and signals at the seams of the pitch tracker's Viterbi stage (shennong_amd/csrc/
pitch_route.h, kernels_pitch_viterbi.hip, kernels_pitch_flat.hip), shared by tests/test_pitch_state_cases.py (CPU:
every entry is what it claims), tests/test_pitch_seams_gpu.py and tools/pitch_seams_errors.py.

The stage has three forms - a lane per state (`state`: viterbi_forward<7 | 8 | 0>), a team of 2 or 4 waves per
utterance (`team2`, `team4`) and a lane per candidate (`flat`) - and two numbers a caller chooses freely decide
what each of them does: the number of states S (one per log-spaced lag between 1 / max_f0 and 1 / min_f0, a factor
1 + delta_pitch apart) and the number of utterances of the call.  The five-level search of every form counts its
states with formulas in S modulo 4, 8, 32 and 128; the route changes form at 127 | 128, 128 | 129, 448 | 449 and
512 | 513 states and refuses from 1461 on.  Plain Python: nothing here needs a GPU."""

import functools

import numpy as np

from oracle import oracle as orc
from shennong_amd import _abi, synth

SAMPLE_RATE = 16000
MIN_F0, MAX_F0 = 50.0, 400.0      # the defaults: first / last lag of the NCCF (8, 82) stay the default run's


def pitch_options(**fields):
    """the oracle's option record: the defaults with `fields` (names of snf_pitch_options) set"""
    po = _abi.default_pitch_options()
    for name, value in fields.items():
        assert hasattr(po, name), name
        setattr(po, name, value)
    return po


def num_states(delta_pitch, min_f0=MIN_F0, max_f0=MAX_F0):
    return orc.pitch_lags(pitch_options(min_f0=min_f0, max_f0=max_f0, delta_pitch=delta_pitch))[0].shape[0]


def find_delta_pitch(target, min_f0=MIN_F0, max_f0=MAX_F0):
    """A float32 delta_pitch whose lag ladder has exactly `target` entries, by bisection against the oracle (the
    ladder is accumulated in float32, shennong_amd/csrc/host_tables.cpp make_pitch_tables: a closed formula is off
    by one near the bounds).  The ladder shortens as delta_pitch grows; the bisection aims at the middle of the
    interval of delta_pitch that gives `target`, so that the value found sits away from both of its ends."""
    ratio = np.log(max_f0 / min_f0)

    def edge(count):
        """(about) the largest delta_pitch that still gives `count` states"""
        lo, hi = 1e-5, 100.0
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if num_states(float(np.float32(mid)), min_f0, max_f0) >= count:
                lo = mid
            else:
                hi = mid
        return lo
    assert target >= 1 and np.exp(ratio / max(target, 2)) > 1.0
    upper, lower = edge(target), edge(target + 1)
    delta = float(np.float32(0.5 * (upper + lower)))
    assert num_states(delta, min_f0, max_f0) == target, (target, delta)
    return delta


# ---- state counts -> delta_pitch, found by find_delta_pitch(S) with the default min_f0 and max_f0 and recorded here
# (tests/test_pitch_state_cases.py: every entry gives the S it claims, and the helper finds four of them again) ---
DELTA_PITCH = {
    2: 4.41421365737915, 33: 0.06609074026346207, 64: 0.03329133242368698,
    65: 0.032766759395599365, 127: 0.01657438836991787, 128: 0.016443327069282532, 129: 0.016314318403601646,
    130: 0.01618732139468193, 131: 0.016062287613749504, 132: 0.015939168632030487, 160: 0.013122736476361752,
    161: 0.013040443882346153, 256: 0.008171956054866314, 257: 0.008139966987073421, 384: 0.005437010433524847,
    385: 0.005422831512987614, 441: 0.004731804598122835, 442: 0.004721063654869795, 443: 0.004710369743406773,
    444: 0.004699723795056343, 445: 0.004689124412834644, 446: 0.004678572993725538, 447: 0.004668071400374174,
    448: 0.004657614976167679, 449: 0.004647204652428627, 511: 0.004081652499735355, 512: 0.004073658958077431,
    513: 0.004065695218741894, 641: 0.0032518687658011913, 1025: 0.002031775191426277, 1368: 0.001521772239357233,
    1369: 0.0015206579118967056, 1460: 0.00142577919177711, 1461: 0.0014248015359044075,
}


def options_kwargs(S, **more):
    """keyword arguments of KaldiPitchProcessor for `S` states"""
    return dict(min_f0=MIN_F0, max_f0=MAX_F0, delta_pitch=DELTA_PITCH[S], **more)


def oracle_options(S, **fields):
    return pitch_options(min_f0=MIN_F0, max_f0=MAX_F0, delta_pitch=DELTA_PITCH[S], **fields)


# ---- which form runs at which state count -------------------------------------------------------------------
# (name of the form: SNF_PITCH_TEAM, SNF_PITCH_FLAT as the test sets them; None: unset)
KNOBS = {'state': ('1', '0'), 'team2': ('2', None), 'team4': ('4', None), 'flat': ('1', '1')}
BY_STATE, TEAM, FLAT = 0, 1, 2     # PitchForm of pitch_route.h, as tests/test_pitch_route.py numbers them

LDS_LIMIT_S, REFUSED_S = 1460, 1461      # 100 S4 + 17 536 bytes against 160 KiB: S4 <= 1460
# viterbi_forward<7>: one super-state (and below 33 states no level-2 state, below 9 no level-3 state), every
# multiple of 32, 64 and 128 with its neighbour, both ends of the register form
STATE_7 = (2, 33, 64, 65, 127, 128, 129, 256, 257, 384, 385, 447, 448)
STATE_8 = (449, 511, 512)
# viterbi_forward<0>: 513 and 641 (a second trip of the level-1 loop, 5 and 6 super-states; 17 level-2 states: a
# second trip of that loop too), 1025 (a third trip of level 1 that holds one super-state alone, a third of level
# 2), the last count whose LDS fits.  1368 | 1369: 128 | 129 states of level 3, two | three passes of 64.  In the
# first frame of every utterance (forward costs all zero: bp[i] = i, every level-3 window between two known states
# is exactly kLongRange3 long) and in every frame of digital silence all of them but those of the last, partial gap
# go to the long-window queue of refine_levels: with 128 the queue is worked off where the level ends, holding 126;
# with 129 the second pass fills it to its kQueueEntries and it is worked off in the middle of the level.
STATE_0 = (513, 641, 1025, 1368, 1369, LDS_LIMIT_S)
TEAM_S = (128, 129, 256, 257, 384, 385, 448, 449, 511, 512)
TEAM_IGNORED_S = (127, 513)              # the knob is set, the route runs the by-state form: the same bytes
FLAT_S = (129, 130, 131, 132, 160, 161, 256, 257, 385) + tuple(range(441, 449))
FLAT_IGNORED_S = (128, 449)              # SNF_PITCH_FLAT=1 outside 129 .. 448: by state


def forms_at(S):
    """{name of a run: (SNF_PITCH_TEAM, SNF_PITCH_FLAT, expected form, expected waves, expected nk)} at S states.
    `state` always runs; the runs whose knob the route ignores are named `team2_ignored`, ... and expect the
    by-state form."""
    nk = 7 if S <= 448 else 8 if S <= 512 else 0
    runs = {}
    if S in STATE_7 + STATE_8 + STATE_0 or S in TEAM_IGNORED_S + FLAT_IGNORED_S:
        runs['state'] = KNOBS['state'] + (BY_STATE, 8, nk)
    if S in TEAM_S:
        runs['state'] = KNOBS['state'] + (BY_STATE, 8, nk)
        runs['team2'] = KNOBS['team2'] + (TEAM, 2, -1)
        runs['team4'] = KNOBS['team4'] + (TEAM, 4, -1)
    if S in TEAM_IGNORED_S:
        # (below 128 and above 512 states the flat form does not run either: FLAT unset is by state)
        runs['team2_ignored'] = ('2', '0', BY_STATE, 8, nk)
        runs['team4_ignored'] = ('4', '0', BY_STATE, 8, nk)
    if S in FLAT_S:
        runs['state'] = KNOBS['state'] + (BY_STATE, 8, nk)
        runs['flat'] = KNOBS['flat'] + (FLAT, 8, -1)
    if S in FLAT_IGNORED_S:
        runs['flat_ignored'] = KNOBS['flat'] + (BY_STATE, 8, nk)
    return runs


# ---- ties.  With the default penalty no two candidates of a state tie for its minimum, not even on digital silence
# (cost = (j - i)^2 factor + fwd[j]: j = i wins alone).  With penalty_factor = 0 a step costs nothing, the cost of
# (i, j) is fwd[j], and on digital silence, where all forward costs are equal, EVERY candidate of every state ties:
# the lowest index must win in each scan, each combine of partial results, each atomic minimum and in the
# traceback, and the path is state 0 throughout (Kaldi's search starts every state at index 0 and only moves for a
# strictly lower cost).  The batch is digital silence only.  On other signals a zero penalty is outside what the
# tracker promises: the transition cost is no longer convex, Kaldi's bounded search is then a local search, and
# where forward costs tie in part its backward sweep keeps the HIGHER of two tied minima (tests/
# test_pitch_state_cases.py test_kaldi_search_on_partial_ties) while the kernels return the first one.
# One count per shape of the level-1 combine: a last super-state alone (129), the largest flat one (448), four full
# super-states (512), a second trip of the level-1 loop (641).
TIE_PENALTY = 0.0
TIE_S = (129, 448, 512, 641)
TIE_FRAMES = (129, 64, 65, 0, 128, 1, 2, 63, 0, 129, 64, 65, 0, 128, 1, 2, 63)     # 17 utterances of silence


def tie_waves():
    return [silence(FRAMES_TO_SAMPLES[frames]) for frames in TIE_FRAMES]


@functools.lru_cache(maxsize=None)
def tie_wanted(S):
    po = oracle_options(S, penalty_factor=TIE_PENALTY)
    wanted_by_frames = {frames: orc.pitch(po, silence(FRAMES_TO_SAMPLES[frames])) for frames in set(TIE_FRAMES)}
    return [wanted_by_frames[frames] for frames in TIE_FRAMES]


ALL_S = tuple(sorted(set(STATE_7 + STATE_8 + STATE_0 + TEAM_S + TEAM_IGNORED_S + FLAT_S + FLAT_IGNORED_S)))
GPU_CASES = tuple((S, name) for S in ALL_S for name in forms_at(S))
TIE_CASES = tuple((S, name) for S in TIE_S for name in forms_at(S))


# ---- utterance lengths --------------------------------------------------------------------------------------
# samples of a 16 kHz utterance -> pitch frames (oracle.pitch_num_frames; the count does not depend on the lags):
# the resampler gives a 4 kHz signal, a frame is 100 of its samples, 40 apart
FRAMES_TO_SAMPLES = {0: 396, 1: 397, 2: 557, 63: 10317, 64: 10477, 65: 10637, 128: 20717, 129: 20877}
CLICK_SAMPLES, CLICK_FRAMES = 80400, 501     # tests/test_oracle_pins.py _click_utterance: T1 < 500 <= T
TOO_SHORT = (396, 1, 37, 200)                 # samples of the zero-frame utterances, dealt in turn


# ---- signals: seeded, nothing read from disk ------------------------------------------------------------------
def voiced(n, ident):
    return synth.utterances(ident, 1, n)[0]


def silence(n, ident=0):
    """digital silence: every cost ties, the lowest index wins at every level and in the traceback"""
    return np.zeros(n, dtype=np.int16)


def noise(n, ident):
    """Gaussian noise at amplitude 200: many jumps of the backpointer function, hence long windows"""
    return np.rint(np.random.default_rng(7000 + ident).normal(0.0, 200.0, n)).astype(np.int16)


GLIDE_SWEEP_S, GLIDE_HOLD_S = 0.5, 0.1
GLIDE_LOW = MIN_F0 / 1.1        # a little below min_f0: the path rests on the last state while f0 turns


def glide(n, ident=0):
    """a harmonic tone that holds max_f0 for 0.1 s, falls to a little below min_f0 in 0.5 s (exponentially: a
    constant number of states per frame), rises again in the next 0.5 s, and so on: the chosen state visits state
    0 and state S - 1, where the traceback's column clamp works.  (From 33 states on.  With two states a step
    costs penalty_factor log(1 + delta_pitch)^2 = 0.29 while the ballasted NCCF moves a local cost by about 0.01
    a frame: the path of such a ladder never leaves its state, whatever the signal.)"""
    t = np.arange(n, dtype=np.float64) / SAMPLE_RATE
    phase = np.maximum((t % (GLIDE_HOLD_S + 2.0 * GLIDE_SWEEP_S)) - GLIDE_HOLD_S, 0.0) / GLIDE_SWEEP_S
    tri = np.where(phase < 1.0, phase, 2.0 - phase)                     # 0 (held) -> 1 -> 0
    f0 = MAX_F0 * (GLIDE_LOW / MAX_F0) ** tri
    cycles = np.cumsum(f0) / SAMPLE_RATE
    x = sum(np.sin(2 * np.pi * h * cycles) / h for h in range(1, 6)) * 6000.0
    x += np.random.default_rng(9000 + ident).normal(0.0, 20.0, n)
    return np.clip(np.rint(x), -32767, 32767).astype(np.int16)


def click(n, ident=0):
    """tests/test_oracle_pins.py _click_utterance, restated (its seed, whatever `ident`): quiet, and the last 24
    samples are a loud click"""
    rng = np.random.default_rng(3)
    t = np.arange(n)
    w = (rng.normal(0, 12, n) + 40 * np.sin(2 * np.pi * 140 * t / 16000)).astype(np.int16)
    w[-24:] = (20000 * np.sin(2 * np.pi * 300 * np.arange(24) / 16000 + 0.5)).astype(np.int16)
    return w


SIGNALS = {'voiced': voiced, 'silence': silence, 'noise': noise, 'glide': glide, 'click': click}

# ---- the 17 utterances: (signal, frames).  The four signals in turn; every length of the list (1, 2, 63, 64, 65,
# 128 and 129 frames: one, and one more or less than one and two 64-frame chunks of the traceback) falls on at
# least two signals, the glide has the two long ones. ----------------------------------------------------------
MASTER = (
    ('voiced', 129), ('silence', 64), ('noise', 65), ('glide', 128),
    ('voiced', 1), ('silence', 2), ('noise', 63), ('click', CLICK_FRAMES),
    ('glide', 129), ('voiced', 64), ('silence', 65), ('noise', 128),
    ('glide', 63), ('voiced', 2), ('silence', 1), ('noise', 64), ('glide', 65),
)
UTT_COUNTS = (1, 7, 8, 9, 17)      # one wave; one short of, exactly, one more than a workgroup of 8; two and one
HOLES = (3,) + tuple(range(8, 16)) + (16,)


@functools.lru_cache(maxsize=None)
def utterance(index):
    kind, frames = MASTER[index]
    n = CLICK_SAMPLES if kind == 'click' else FRAMES_TO_SAMPLES[frames]
    wave = SIGNALS[kind](n, index)
    wave.setflags(write=False)
    return wave


@functools.lru_cache(maxsize=None)
def too_short(index):
    """the zero-frame utterance that stands at `index` of the batch with holes: not one pitch frame"""
    n = TOO_SHORT[index % len(TOO_SHORT)]
    wave = noise(n, 100 + index)
    wave.setflags(write=False)
    return wave


def batch(name):
    """[(index into MASTER, or -1 - index for a zero-frame utterance)] of a batch: 'n1', 'n7', 'n8', 'n9', 'n17',
    and 'holes': the 17 utterances with zero-frame ones at index 3, at 8 .. 15 and at the last index.

    The tracker hands a ragged batch out LONGEST FIRST (run_pitch_device sorts the utterances by frame count,
    ties in batch order), so the seven utterances that are left fill slots 0 .. 6: the first workgroup of the
    by-state and the flat kernel ends in one wave that leaves at `T <= 0` beside seven that work, the second
    holds eight such waves, the third one and seven waves behind the batch (`slot >= n_utts`); of the team
    kernel's seventeen workgroups ten leave whole."""
    if name == 'holes':
        return tuple(-1 - i if i in HOLES else i for i in range(len(MASTER)))
    count = int(name[1:])
    assert name == 'n%d' % count and count in UTT_COUNTS
    return tuple(range(count))


BATCHES = tuple('n%d' % n for n in UTT_COUNTS) + ('holes',)


def waves_of(name):
    return [utterance(i) if i >= 0 else too_short(-1 - i) for i in batch(name)]


@functools.lru_cache(maxsize=None)
def wanted(S, index):
    """the oracle's rows of utterance `index` of MASTER at S states ((0, 0) for a zero-frame one); computed once
    per process and left unchanged"""
    out = orc.pitch(oracle_options(S), utterance(index) if index >= 0 else too_short(-1 - index))
    out.setflags(write=False)
    return out


def wanted_of(S, name):
    return [wanted(S, i) for i in batch(name)]


# ---- the long-window queue of refine_levels ----------------------------------------------------------------------
LONG_RANGE = {3: 32, 4: 12, 5: 12}           # kLongRange3, kLongRange4 (kernels_pitch_viterbi.hip)
QUEUE_ENTRIES = 128                          # kQueueEntries: a pass flushes mid-level above 128 - 64 entries


def first_frame_long(S):
    """level-3 states whose window is long when bp[i] = i: all but those of a last gap that ends before 32 states"""
    return [i for i in level_states(3, S)[0] if (i & ~31) + 32 < S or S - 1 - (i & ~31) >= LONG_RANGE[3]]


def level_states(level, S):
    """(states of a level of refine_levels, distance of their known neighbours)"""
    if level == 3:
        return [i for i in range(8, S, 8) if i % 32], 32
    if level == 4:
        return list(range(4, S, 8)), 8
    return [i for i in range(S) if i % 4], 4


def long_windows(po, wave):
    """Replay of the search on the oracle's resampled NCCF (tools/pitch_search_replay.py, for any option set): the
    exact backpointer function of every frame in float32, then per level the number of states whose window
    bp[below] .. bp[above] is long, the largest number a single wave has queued when it looks at its queue, and how
    often it works the queue off before the level ends -> (frames, {level: largest count in one frame}, {level:
    largest queue length of one wave}, {level: flushes in the middle of a level})."""
    f32 = np.float32
    _, _, res, _, _ = orc.pitch_debug(po, wave)
    lags = orc.pitch_lags(po)[0]
    S = lags.shape[0]
    factor = f32(f32(np.log(f32(1.0 + float(po.delta_pitch)))) ** 2 * f32(po.penalty_factor))
    jj = np.arange(S)
    trans = (((jj[None, :] - jj[:, None]) ** 2).astype(f32) * factor).astype(f32)
    soft = (f32(po.soft_min_f0) * lags).astype(f32)
    levels = {level: level_states(level, S) for level in (3, 4, 5)}
    below = {level: np.array([i & ~(gap - 1) for i in st], dtype=np.int64) for level, (st, gap) in levels.items()}
    worst = {3: 0, 4: 0, 5: 0}
    queued = {3: 0, 4: 0, 5: 0}
    mid_level = {3: 0, 4: 0, 5: 0}
    fwd = np.zeros(S, f32)
    for t in range(res.shape[0]):
        cost = trans + fwd[None, :]
        bp = cost.argmin(axis=1)
        for level, (st, gap) in levels.items():
            if not st:
                continue
            above = below[level] + gap
            hi = np.where(above < S, bp[np.minimum(above, S - 1)], S - 1)
            longs = hi - bp[below[level]] >= LONG_RANGE[level]
            worst[level] = max(worst[level], int(longs.sum()))
            # one wave (W == 1): 64 states of the level per pass, the queue is worked off once it holds more than
            # QUEUE_ENTRIES - 64 entries or the level ends
            n_queued = 0
            for p0 in range(0, len(st), 64):
                n_queued += int(longs[p0:p0 + 64].sum())
                queued[level] = max(queued[level], n_queued)
                if n_queued > QUEUE_ENTRIES - 64:
                    mid_level[level] += p0 + 64 < len(st)
                    n_queued = 0
        v = res[t]
        local = (f32(1.0) - v).astype(f32)
        local = (local + (soft * v).astype(f32)).astype(f32)
        nf = (cost[jj, bp] + local).astype(f32)
        fwd = (nf + f32(-nf.min())).astype(f32)
    return res.shape[0], worst, queued, mid_level
