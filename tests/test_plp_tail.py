"""CPU half of the tests of the PLP tail and RASTA kernels: factoring the tail out of the oracle and out of the
float64 statement changed neither, and the cases of plp_tail_cases.py reach what they claim - on the very rows
test_plp_tail_gpu.py gives the HIP kernels."""

import numpy as np
import pytest

import plp_tail_cases as pc
from oracle import oracle as orc
from oracle import spec_f64
from shennong_amd.processor import FilterbankProcessor, PlpProcessor


@pytest.mark.parametrize('opts', [dict(), dict(htk_compat=True), dict(cepstral_lifter=0, cepstral_scale=0.9),
                                  dict(lpc_order=8, num_ceps=9), dict(compress_factor=0.5)],
                         ids=lambda o: '-'.join(f'{k}={v}' for k, v in o.items()) or 'default')
def test_oracle_tail_is_the_tail_of_compute(wave, opts):
    """oracle.plp_tail on the oracle's own linear mel rows of test.wav gives the bits of orc.compute of the PLP
    options: the factoring changed nothing"""
    plp = PlpProcessor(dither=0, use_energy=False, **opts)
    bank = FilterbankProcessor(dither=0, num_bins=plp.num_bins, use_log_fbank=False)
    mel = orc.compute(bank._build_options(), wave)
    assert mel.shape == (140, plp.num_bins)
    got = orc.plp_tail(plp._build_options(), mel, np.zeros(mel.shape[0]))
    assert np.array_equal(got, orc.compute(plp._build_options(), wave))


def test_oracle_tail_energy_column(wave):
    """with use_energy the tail takes the double logarithm of the linear frame energy, floored at float64 eps and at
    the energy floor: the raw energies of test.wav give the energy column of orc.compute to its last bits"""
    plp = PlpProcessor(dither=0, use_energy=True)
    want = orc.compute(plp._build_options(), wave)
    bank = FilterbankProcessor(dither=0, use_log_fbank=False)
    mel = orc.compute(bank._build_options(), wave)
    energy = np.exp(want[:, 0].astype(np.float64))
    got = orc.plp_tail(plp._build_options(), mel, energy)
    assert np.array_equal(got[:, 1:], want[:, 1:])
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= np.spacing(want[:, 0]))
    floored = PlpProcessor(dither=0, use_energy=True, energy_floor=pc.ENERGY_FLOOR)
    got = orc.plp_tail(floored._build_options(), mel, np.array([0.0, 1e-20, pc.EPS64] + [1e9] * 137))
    assert np.all(got[:3, 0] == np.float32(np.log(pc.ENERGY_FLOOR))) and np.all(got[3:, 0] == np.float32(np.log(1e9)))
    got = orc.plp_tail(plp._build_options(), mel, np.array([0.0, 1e-20, pc.EPS64] + [1e9] * 137))
    assert np.all(got[:3, 0] == np.float32(np.log(pc.EPS64)))


@pytest.mark.parametrize('opts', [dict(), dict(use_energy=False, htk_compat=True), dict(use_rasta=True),
                                  dict(num_bins=40, lpc_order=20, num_ceps=21, raw_energy=False)],
                         ids=lambda o: '-'.join(f'{k}={v}' for k, v in o.items()) or 'default')
def test_statement_tail_is_the_tail_of_plp(wave, opts):
    """spec_f64.plp_tail behind the statement's own mel rows is spec_f64.plp"""
    x = wave.astype(np.float64)
    want = spec_f64.plp(x, **opts)
    shift, length, padded = spec_f64.frame_geometry(16000, 0.01, 0.025)
    frames = spec_f64.extract_frames(x, shift, length)
    frames = frames - frames.mean(axis=1, keepdims=True)
    raw = np.log(np.maximum((frames * frames).sum(axis=1), pc.EPS64))
    pre = frames.copy()
    pre[:, 1:] = frames[:, 1:] - 0.97 * frames[:, :-1]
    pre[:, 0] = frames[:, 0] - 0.97 * frames[:, 0]
    pre = pre * spec_f64.window_function(length)[None, :]
    post = np.log(np.maximum((pre * pre).sum(axis=1), pc.EPS64))
    spec = np.fft.rfft(pre, n=padded, axis=1)
    power = (spec.real ** 2 + spec.imag ** 2)[:, :padded // 2]
    bins = opts.get('num_bins', 23)
    w, centers = spec_f64.mel_banks_vtln(bins, 16000, padded)
    mel = power @ w.T
    if opts.get('use_rasta'):
        mel = spec_f64.rasta(mel, eps=pc.EPS32)
    got = spec_f64.plp_tail(
        mel, centers, raw if opts.get('raw_energy', True) else post, lpc_order=opts.get('lpc_order', 12),
        num_ceps=opts.get('num_ceps', 13), use_energy=opts.get('use_energy', True),
        htk_compat=opts.get('htk_compat', False))
    assert np.array_equal(got, want)


def test_statement_rasta_eps():
    """the statement's filter adds what it is told to: on a bin of 1e-9 float32 eps (the reference's, on its float32
    frames) and float64 eps are different functions, and the C oracle follows the former"""
    rows, off, want, oracle, _ = pc.rasta_reference(23)
    u, b = pc.RASTA_QUIET
    quiet = rows[off[u]:off[u + 1]]
    other = spec_f64.rasta(quiet)
    assert np.array_equal(other, spec_f64.rasta(quiet, eps=pc.EPS64))
    keep = [k for k in range(23) if k != b]
    assert np.abs(other[:, keep] / want[u][:, keep] - 1).max() < 1e-6      # loud bins: the choice does not show
    # (the quiet bin is constant: what is added to it before the logarithm cancels in a filter whose numerator
    # sums to zero - the two statements differ where a quiet bin VARIES)
    varying = quiet.copy()
    varying[:, b] = np.float32(1e-9) * (1 + np.arange(quiet.shape[0]) % 3)
    a32, a64 = spec_f64.rasta(varying, eps=pc.EPS32), spec_f64.rasta(varying, eps=pc.EPS64)
    assert np.abs(a64[4:, b] / a32[4:, b] - 1).max() > 0.05
    assert np.abs(orc.rasta(varying)[4:, b] / a32[4:, b] - 1).max() < 1e-5


@pytest.mark.parametrize('case', pc.SHAPE_CASES, ids=lambda c: c[0])
def test_regular_rows_stay_off_the_durbin_floor(case):
    """no regular row reaches Durbin's 1 - k^2 < 1e-5 floor, in the statement's arithmetic or in float32 (zero rows
    left out): at the floor the recursion is discontinuous and no bound on the round-off holds"""
    _, shape, opts, _ = case
    proc = pc.processor(shape, **opts)
    rows, energy = pc.regular_rows(shape)
    assert rows.shape == (max(pc.frames_of(shape)), shape[0]) and rows.dtype == np.float32
    assert np.all(rows > 0) and np.all((energy >= 1e2) & (energy <= 1e12))
    assert pc.floor_hits(proc, rows).size == 0
    # ... and the bound the device is held to is a float32 round-off, not a licence: the oracle errs by less than
    # 1e-3 of a cepstrum on these rows (1e-2 under square-root compression: the compressed spectrum then spans nine
    # decades instead of six, and the recursion amplifies accordingly)
    _, _, want, oracle, bound = pc.reference(shape, pc._key(opts))
    assert want.shape == oracle.shape == (rows.shape[0], shape[2])
    assert np.all(bound > 0) and bound.max() < (4e-2 if 'compress_factor' in opts else 4e-3)


def test_option_cases_stay_off_the_floor_too():
    for opts in pc.OPTION_CASES:
        _, _, want, oracle, bound = pc.reference(pc.EXACT_SHAPE, pc._key(opts))
        assert np.all(np.isfinite(want)) and np.all(bound > 0) and bound.max() < 4e-3, opts


def test_cases_reach_every_route_and_bound():
    routes = {pc.route_of(shape, env) for _, shape, _, env in pc.SHAPE_CASES}
    assert routes == {'plp_tail_exact_kernel', 'plp_tail_small_kernel', 'plp_tail_kernel'}
    shapes = [shape for _, shape, _, _ in pc.SHAPE_CASES]
    assert (pc.SMALL_BINS, pc.SMALL_LPC, pc.SMALL_LPC + 1) in shapes       # the small kernel's bound
    assert (pc.MAX_BINS, pc.MAX_LPC, pc.MAX_LPC + 1) in shapes             # the generic kernel's bound
    assert (pc.SMALL_BINS + 1, 12, 13) in shapes and (23, pc.SMALL_LPC + 1, 13) in shapes   # one past either bound
    for shape in pc.BOTH_SHAPES:
        assert pc.route_of(shape, ('SNF_PLP_SMALL_TAIL',)) == 'plp_tail_small_kernel'
        assert pc.route_of(shape, ('SNF_PLP_GENERIC_TAIL',)) == 'plp_tail_kernel'
    for env in pc.DEFAULT_ROUTES:
        assert pc.route_of(pc.EXACT_SHAPE, env) in routes
    assert len({pc.route_of(pc.EXACT_SHAPE, env) for env in pc.DEFAULT_ROUTES}) == 3


def test_frame_counts_reach_every_seam():
    pc.check_frames(pc.FRAMES, pc.EXACT_ROWS)
    pc.check_frames(pc.FRAMES, pc.SMALL_ROWS)
    assert 1 in pc.FRAMES and 515 == 2 * pc.EXACT_ROWS + 3 == 8 * pc.SMALL_ROWS + 3
    with pytest.raises(ValueError, match='odd_partial_last_block'):
        pc.check_frames((1, 64, 65, 256, 257, 514), pc.EXACT_ROWS)
    with pytest.raises(ValueError, match='one_past_a_block'):
        pc.check_frames((1, 64, 256, 515), pc.SMALL_ROWS)
    # the widest shape runs one frame past a block of either height
    assert pc.BIG_FRAMES == (pc.SMALL_ROWS + 1, pc.EXACT_ROWS + 1)


def test_edge_rows_reach_what_they_claim():
    rows, energy = pc.check_edge_rows()
    assert rows.shape == (pc.EDGE['rows'], 23)
    proc = pc.processor(pc.EXACT_SHAPE)
    assert pc.floor_hits(proc, rows).size == 0
    # the oracle and the statement floor c0 of the quiet rows at float64 eps, exactly
    _, _, want, oracle, _ = pc.reference(pc.EXACT_SHAPE, (), 'edge')
    for k in pc.EDGE['below_one'] + pc.EDGE['tiny']:
        assert want[k, 0] == pc.EPS64 and oracle[k, 0] == np.float32(pc.EPS64)
    assert np.all(np.isfinite(oracle)) and np.all(np.isfinite(want))
    # ... and the energies at or below eps give log(eps), those under the floor log(floor)
    key = pc._key({'use_energy': True})
    _, _, want, oracle, _ = pc.reference(pc.EXACT_SHAPE, key, 'edge')
    for name in ('energy_zero', 'energy_1e-20', 'energy_eps'):
        assert oracle[pc.EDGE[name], 0] == np.float32(np.log(pc.EPS64)) == np.float32(want[pc.EDGE[name], 0])
    key = pc._key({'use_energy': True, 'energy_floor': pc.ENERGY_FLOOR})
    _, _, want, oracle, _ = pc.reference(pc.EXACT_SHAPE, key, 'edge')
    low = energy < pc.ENERGY_FLOOR
    assert np.all(oracle[low, 0] == np.float32(np.log(pc.ENERGY_FLOOR)))
    assert np.all(oracle[~low, 0] == np.log(energy[~low]).astype(np.float32))


@pytest.mark.parametrize('bins', pc.RASTA_BINS)
def test_rasta_layout_and_first_frames(bins):
    """the layout reaches utterances of 0 to 6 frames, an empty one between others and a partial last block; the
    oracle's filter emits exactly 1.0 for the first four frames of every utterance"""
    rows, off, want, oracle, bound = pc.rasta_reference(bins)
    assert list(np.diff(off)) == pc.RASTA_LENGTHS and rows.shape == (sum(pc.RASTA_LENGTHS), bins)
    if bins == 23:
        assert len(pc.RASTA_LENGTHS) * bins == 230     # three full blocks of 64 threads and one of 38
    with pytest.raises(ValueError, match='length_5'):
        pc.check_rasta_layout([n for n in pc.RASTA_LENGTHS if n != 5], bins)
    for o, w in zip(oracle, want):
        assert np.all(o[:4] == np.float32(1.0)) and np.all(w[:4] == 1.0)
    (u, b), (v, c) = pc.RASTA_ZERO, pc.RASTA_QUIET
    if b < bins and c < bins:
        assert np.all(rows[off[u]:off[u + 1], b] == 0) and np.all(rows[off[v]:off[v + 1], c] == np.float32(1e-9))
        assert np.all(np.isfinite(oracle[u])) and np.all(np.isfinite(oracle[v]))
    assert np.all(bound > 0) and bound.shape == (bins,)
