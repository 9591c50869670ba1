#!/usr/bin/env python
"""What the Viterbi forms of the pitch tracker return at the state counts and on the batches of
tests/pitch_state_cases.py, against the CPU oracle and against each other.

    python tools/pitch_seams_errors.py > profiles/pitch_seams_errors.txt

Per state count and run (tests/pitch_state_cases.py forms_at: the by-state kernel, a team of two or four waves, the
lane-per-candidate kernel, and the runs whose knob the route ignores), over the six batches: the frames compared,
the frames in which a bit of the row (POV NCCF, pitch) differs from the oracle's, and the bytes that differ from the
by-state run of the same state count; then the same for the silent batch with penalty_factor = 0 (`ties`).  The
contract is zero everywhere; the file is the record of it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import pitch_state_cases as pc
    import test_pitch_seams_gpu as seams
    from shennong_amd import _backend
    _backend.check(_backend.lib().snf_debug_fill_lds(0xFFFFFFFF))
    _backend.DEVICE_POOL.poison = True
    setenv, delenv = os.environ.__setitem__, lambda name: os.environ.pop(name, None)
    print('# Viterbi forms of the pitch tracker on', _backend.device_name(0).strip(), 'against the CPU oracle: batches',
          ', '.join(pc.BATCHES), 'of tests/pitch_state_cases.py')
    print('# states  run  kernel  utterances  frames  frames_differing_from_oracle  bytes_differing_from_by_state_run')
    kernels = {pc.BY_STATE: 'viterbi_forward<%d>', pc.TEAM: 'viterbi_forward_team<%d>', pc.FLAT: 'viterbi_forward_flat'}
    total = 0
    cases = [(S, run, pc.BATCHES) for S, run in pc.GPU_CASES] + [(S, run, ('ties',)) for S, run in pc.TIE_CASES]
    for S, run, batches in cases:
        _, _, form, waves, nk = pc.forms_at(S)[run]
        kernel = kernels[form] % (nk if form == pc.BY_STATE else waves) if form != pc.FLAT else kernels[form]
        utts = frames = differ = other = 0
        for batch in batches:
            gots = seams.outputs(S, run, batch, setenv, delenv)
            refs = seams.outputs(S, 'state', batch, setenv, delenv)
            wants = pc.tie_wanted(S) if batch == 'ties' else pc.wanted_of(S, batch)
            for got, want, ref in zip(gots, wants, refs):
                n, bad = seams.compare(got, want)
                utts, frames, differ = utts + 1, frames + n, differ + bad
                assert got.shape == ref.shape
                other += int((np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(ref.tobytes(), np.uint8)).sum())
        total += differ + other
        print('%d  %s  %s  %d  %d  %d  %d' % (S, run if batches != ('ties',) else run + '/ties', kernel, utts, frames,
                                              differ, other))
    return 1 if total else 0


if __name__ == '__main__':
    sys.exit(main())
