"""The three routes of launch_plp_tail and rasta_kernel (kernels_plp_tail.hip) alone, on chosen mel rows through
Plan.debug_plp_tail (snf_debug_plp_tail runs launch_rasta and launch_plp_tail as the product path does, without the
mel front end), against the float64 statement of the tail (oracle/spec_f64.py plp_tail) on the same float32 rows.
test_plp_tail.py shows on the CPU that the cases of plp_tail_cases.py reach what they claim.

The rule is the project's rule for kernels with powf / logf / expf (test_post_routes_gpu.py, test_bottleneck_gpu.py):
per output column the device may err 4 times as far from the statement as the float32 C oracle does over the same
batch.  One stated exception: plp_tail_exact_kernel takes a float logf "good to an ulp" for c0 and for the energy,
where the oracle's double logarithm is correctly rounded; those columns get 2 ulp of |want| on top.  Every test
asserts its route through Plan.kernel_name and prints its worst error over bound (run with -s; the committed lines
are profiles/plp_tail_errors.txt)."""

import numpy as np
import pytest

import plp_tail_cases as pc
from conftest import assert_close
from oracle import oracle as orc
from shennong_amd import _backend

pytestmark = pytest.mark.gpu


def _tail_name(plan):
    """the last kernel the plan recorded (slot 1 is rasta_kernel on a RASTA plan)"""
    names = [plan.kernel_name(k) for k in range(1, 7)]
    return [n for n in names if n][-1]


def _plan(monkeypatch, shape, opts=(), env=()):
    """a fresh plan made under the switches of `env` (SNF_PLP_EXACT_POW is read when the plan is made, the two
    routing switches at every launch)"""
    for name in ('SNF_PLP_GENERIC_TAIL', 'SNF_PLP_SMALL_TAIL', 'SNF_PLP_EXACT_POW'):
        monkeypatch.delenv(name, raising=False)
    for name in env:
        monkeypatch.setenv(name, '1')
    proc = pc.processor(shape, **dict(opts))
    return proc, _backend.Plan(proc._build_options(), quiet=True)


def _run(plan, route, rows, energy, frames=None):
    frames = rows.shape[0] if frames is None else frames
    got = plan.debug_plp_tail(rows[:frames], energy[:frames])
    assert _tail_name(plan) == route and plan.kernel_name(2) is None
    assert got.shape == (frames, plan.ndims) and got.dtype == np.float32
    return got


def _check(tag, proc, route, got, want, oracle, bound, family=True):
    """the 4 x rule per column (bound: over the case's longest run), then the family tolerance against the oracle
    (`family` False: test_routes_against_the_oracle_at_the_family_tolerance asserts it for the case)"""
    n = got.shape[0]
    err = np.abs(got.astype(np.float64) - want[:n])
    allow = pc.allowance(proc, want[:n], bound, route)
    ratio = np.max(err / allow, axis=0)
    print(f'plp_tail {tag} {route} {n} frames: worst error / bound per column', ' '.join(f'{r:.3f}' for r in ratio))
    assert np.all(np.isfinite(got)), tag
    assert np.all(err <= allow), (tag, n, float(ratio.max()), int(np.argmax(ratio)))
    if family:
        assert_close(got, oracle[:n], rtol=1e-4, what=tag, family='plp')
    return float(ratio.max())


@pytest.mark.parametrize('case', pc.SHAPE_CASES, ids=lambda c: c[0])
def test_routes_against_the_statement(gpu, monkeypatch, case):
    """every route at its shapes, every total frame count; a shorter run reads a prefix of the longest run's rows, and
    the output of a batch does not depend on what follows it: the first 256 (64) rows of the longer runs are the
    256-frame (64-frame) run bit for bit, row 0 of every run is the one-frame run"""
    tag, shape, opts, env = case
    route = pc.route_of(shape, env)
    rows, energy, want, oracle, bound = pc.reference(shape, pc._key(opts))
    proc, plan = _plan(monkeypatch, shape, pc._key(opts), env)
    runs = {n: _run(plan, route, rows, energy, n) for n in pc.frames_of(shape)}
    for n, got in runs.items():
        _check(tag, proc, route, got, want, oracle, bound, family=False)
    for n, got in runs.items():
        for m, longer in runs.items():
            if m > n:
                assert np.array_equal(longer[:n], got), (tag, n, m)


@pytest.mark.parametrize('case', pc.SHAPE_CASES, ids=lambda c: c[0])
def test_routes_against_the_oracle_at_the_family_tolerance(gpu, monkeypatch, case):
    """the same runs against the float32 C oracle at the parity suite's tolerance for PLP, 1e-4 relative + 1.2e-5.

    On these rows, six decades wide, the Durbin recursion amplifies float32 round-off until the oracle itself is
    further from the float64 statement than the tolerance is wide (up to 3.0e-3 under square-root compression): two
    float32 implementations agree that closely only if they round alike.  plp_tail_kernel, plp_tail_small_kernel
    and the form of plp_tail_exact_kernel for exponents other than 1/3 therefore take the reference's arithmetic
    operation by operation (the double power rounded once, no fused products) and need no absolute term at all;
    with the device's powf and fused products, square-root compression needed 3.2e-4 and 23 / 12 / 12 1.27e-5.
    The cube-root form of plp_tail_exact_kernel keeps its own arithmetic and needs 3.5e-6 (7.0e-6 with powf)."""
    tag, shape, opts, env = case
    route = pc.route_of(shape, env)
    rows, energy, _, oracle, _ = pc.reference(shape, pc._key(opts))
    _, plan = _plan(monkeypatch, shape, pc._key(opts), env)
    runs = {n: _run(plan, route, rows, energy, n) for n in pc.frames_of(shape)}
    for n, got in runs.items():
        excess = np.abs(got.astype(np.float64) - oracle[:n]) - 1e-4 * np.abs(oracle[:n].astype(np.float64))
        print(f'plp_tail {tag} {route} {n} frames: needs {max(float(excess.max()), 0.0):.3g} absolute at 1e-4 relative '
              f'against the oracle (family: 1.2e-05), {int((excess > 1.2e-5).sum())} of {got.size} values outside')
    for n, got in runs.items():
        assert_close(got, oracle[:n], rtol=1e-4, what=tag, family='plp')


@pytest.mark.parametrize('env', pc.DEFAULT_ROUTES, ids=lambda e: pc.route_of(pc.EXACT_SHAPE, e))
@pytest.mark.parametrize('opts', pc.OPTION_CASES, ids=lambda o: '-'.join(f'{k}={v}' for k, v in o.items()))
def test_options_on_the_default_shape(gpu, monkeypatch, opts, env):
    """use_energy, htk_compat, the lifter and the scale on each route of 23 / 12 / 13, at 257 frames (one frame
    past a block of either height); htk_compat is a pure rotation of the columns of the plain output"""
    route = pc.route_of(pc.EXACT_SHAPE, env)
    key = pc._key(opts)
    rows, energy, want, oracle, bound = pc.reference(pc.EXACT_SHAPE, key)
    proc, plan = _plan(monkeypatch, pc.EXACT_SHAPE, key, env)
    got = _run(plan, route, rows, energy, 257)
    _check('-'.join(f'{k}={v}' for k, v in opts.items()), proc, route, got, want, oracle, bound)
    if opts.get('htk_compat'):
        plain = dict(opts, htk_compat=False)
        _, plain_plan = _plan(monkeypatch, pc.EXACT_SHAPE, pc._key(plain), env)
        flat = _run(plain_plan, route, rows, energy, 257)
        assert np.array_equal(got, np.concatenate([flat[:, 1:], flat[:, :1]], axis=1))


@pytest.mark.parametrize('shape', pc.BOTH_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_small_and_generic_kernels_agree_bit_for_bit(gpu, monkeypatch, shape):
    """plp_tail_small_kernel is "the same arithmetic, same order" as plp_tail_kernel: the same bits on every shape both
    accept, on the regular rows (c0 column) and, for the default shape, on the edge batch with the energy column"""
    rows, energy = pc.regular_rows(shape)
    outs = {}
    for env in (('SNF_PLP_SMALL_TAIL',), ('SNF_PLP_GENERIC_TAIL',)):
        route = pc.route_of(shape, env)
        _, plan = _plan(monkeypatch, shape, (), env)
        outs[route] = [_run(plan, route, rows, energy)]
        if shape == pc.EXACT_SHAPE:
            _, plan = _plan(monkeypatch, shape, pc._key({'use_energy': True}), env)
            outs[route].append(_run(plan, route, *pc.edge_rows()))
    assert sorted(outs) == ['plp_tail_kernel', 'plp_tail_small_kernel']
    for a, b in zip(outs['plp_tail_small_kernel'], outs['plp_tail_kernel']):
        differ = np.argwhere(a != b)
        print(f'plp_tail small against generic {shape}: {len(differ)} of {a.size} values differ')
        assert len(differ) == 0, (shape, differ[:5].tolist())


@pytest.mark.parametrize('env', pc.DEFAULT_ROUTES + [('SNF_PLP_EXACT_POW',)],
                         ids=lambda e: pc.route_of(pc.EXACT_SHAPE, e) + ('-exactpow' if 'SNF_PLP_EXACT_POW' in e else ''))
def test_edge_rows(gpu, monkeypatch, env):
    """exact values where the recipe floors: c0 = float32(float64 eps) where the residual energy is below 1, the
    energy column float32(log(float64 eps)) for energies at or below eps and float32(log floor) under an energy
    floor; the rows below pow_third's 1e-30 line come out finite and inside the bound"""
    route = pc.route_of(pc.EXACT_SHAPE, env)
    rows, energy, want, oracle, bound = pc.reference(pc.EXACT_SHAPE, (), 'edge')
    proc, plan = _plan(monkeypatch, pc.EXACT_SHAPE, (), env)
    got = _run(plan, route, rows, energy)
    _check('edge rows', proc, route, got, want, oracle, bound)
    for k in pc.EDGE['below_one'] + pc.EDGE['tiny']:
        assert got[k, 0] == np.float32(pc.EPS64), (k, got[k, 0])
    if route == 'plp_tail_exact_kernel' and not env:
        # pow_third scales the tiny rows in and out: their cepstra agree with those of the correctly rounded powf
        _, exact = _plan(monkeypatch, pc.EXACT_SHAPE, (), ('SNF_PLP_EXACT_POW',))
        other = _run(exact, route, rows, energy)
        tiny = list(pc.EDGE['tiny'])
        diff = np.abs(got[tiny].astype(np.float64) - other[tiny])
        print('plp_tail tiny rows, pow_third against powf: worst difference / bound per column',
              ' '.join(f'{r:.3f}' for r in (diff / bound).max(axis=0)))
        assert np.all(np.isfinite(got[tiny])) and np.all(np.isfinite(other[tiny]))
        assert np.all(diff[:, 1:] <= bound[1:])
    # the energy column
    key = pc._key({'use_energy': True})
    _, _, want, oracle, bound = pc.reference(pc.EXACT_SHAPE, key, 'edge')
    proc, plan = _plan(monkeypatch, pc.EXACT_SHAPE, key, env)
    got = _run(plan, route, rows, energy)
    _check('edge rows use_energy', proc, route, got, want, oracle, bound)
    for name in ('energy_zero', 'energy_1e-20', 'energy_eps'):
        assert got[pc.EDGE[name], 0] == np.float32(np.log(pc.EPS64)), (name, got[pc.EDGE[name], 0])
    assert got[pc.EDGE['energy_above_eps'], 0] == np.float32(np.log(pc.EPS64))    # (one double above: the same float)
    key = pc._key({'use_energy': True, 'energy_floor': pc.ENERGY_FLOOR})
    _, _, want, oracle, bound = pc.reference(pc.EXACT_SHAPE, key, 'edge')
    proc, plan = _plan(monkeypatch, pc.EXACT_SHAPE, key, env)
    got = _run(plan, route, rows, energy)
    _check('edge rows energy_floor', proc, route, got, want, oracle, bound)
    low = energy < pc.ENERGY_FLOOR
    assert low.sum() >= 5 and np.all(got[low, 0] == np.float32(np.log(pc.ENERGY_FLOOR)))
    assert np.array_equal(got[:, 1:], _run(_plan(monkeypatch, pc.EXACT_SHAPE, pc._key({'use_energy': True}), env)[1],
                                           route, rows, energy)[:, 1:])


@pytest.mark.parametrize('shape', [(127, 12, 13), (126, 64, 13), (127, 64, 65)], ids=lambda s: '-'.join(map(str, s)))
def test_shapes_past_the_bounds_are_refused(gpu, monkeypatch, shape):
    """126 bins and order 63 are the bounds of plp_tail_kernel's arrays (the 126 / 63 / 64 case runs them); one more of
    either is refused by launch_plp_tail before anything is launched"""
    proc, plan = _plan(monkeypatch, shape)
    rows = np.ones((3, shape[0]), np.float32)
    with pytest.raises(RuntimeError, match=pc.REFUSAL):
        plan.debug_plp_tail(rows, np.ones(3))
    assert plan.kernel_name(1) is None


def test_the_entry_refuses_other_plans(gpu, monkeypatch):
    from shennong_amd.processor import MfccProcessor
    plan = _backend.Plan(MfccProcessor(dither=0)._build_options(), quiet=True)
    with pytest.raises(ValueError, match='not a PLP plan'):
        plan.debug_plp_tail(np.ones((3, 23), np.float32), np.ones(3))
    _, plp = _plan(monkeypatch, pc.EXACT_SHAPE)
    with pytest.raises(ValueError):
        plp.debug_plp_tail(np.ones((3, 22), np.float32), np.ones(3))       # (rows of another width)
    assert plp.debug_plp_tail(np.ones((0, 23), np.float32), np.ones(0)).shape == (0, 13)


# ---- RASTA --------------------------------------------------------------------------------------------------------
def _rasta_plan(monkeypatch, bins):
    shape = (bins, 2, 3) if bins == 3 else pc.EXACT_SHAPE
    return _plan(monkeypatch, shape, pc._key({'rasta': True}))


@pytest.mark.parametrize('bins', pc.RASTA_BINS)
def test_rasta_kernel(gpu, monkeypatch, bins):
    """rasta_kernel through the entry's `mel_out` (the rows the tail read: the filter works in place) on utterances
    of 0 to 6, 9 and 50 frames: 4 times the oracle's error against the float64 statement with float32 eps per bin
    over the utterances of more than 4 frames; frames 0-3 of every utterance exactly 1.0; the batch equals each
    utterance filtered alone bit for bit (so an utterance of 0 to 4 frames leaves its neighbours' rows alone); the
    tail behind it reads the filtered rows"""
    rows, off, want, oracle, bound = pc.rasta_reference(bins)
    proc, plan = _rasta_plan(monkeypatch, bins)
    energy = np.ones(rows.shape[0])
    out, filtered = plan.debug_plp_tail(rows, energy, frame_offsets=off, mel_out=True)
    route = pc.route_of((bins, 2, 3) if bins == 3 else pc.EXACT_SHAPE)
    assert plan.kernel_name(1) == 'rasta_kernel' and plan.kernel_name(2) == route and plan.kernel_name(3) is None
    assert filtered.shape == rows.shape and np.all(np.isfinite(filtered))
    worst = np.zeros(bins)
    for u, (a, b) in enumerate(zip(off[:-1], off[1:])):
        got = filtered[a:b]
        assert np.all(got[:4] == np.float32(1.0)), u
        if b - a > 4:
            err = np.abs(got.astype(np.float64) - want[u]).max(axis=0)
            worst = np.maximum(worst, err)
            assert np.all(err <= bound), (u, float((err / bound).max()))
            assert_close(got, oracle[u], rtol=1e-4, atol=0.0, what=f'rasta utterance {u}')
        if b > a:
            alone_out, alone = plan.debug_plp_tail(rows[a:b], energy[a:b], mel_out=True)
            assert np.array_equal(alone, got), u
            assert np.array_equal(alone_out, out[a:b]), u
    print(f'rasta_kernel {bins} bins: worst error / bound per bin', ' '.join(f'{r:.3f}' for r in worst / bound))
    # the tail read the filtered rows: a plan without the filter gives the same bits on them
    _, plain = _plan(monkeypatch, (bins, 2, 3) if bins == 3 else pc.EXACT_SHAPE)
    again, unfiltered = plain.debug_plp_tail(filtered, energy, frame_offsets=off, mel_out=True)
    assert plain.kernel_name(1) == route and plain.kernel_name(2) is None
    assert np.array_equal(again, out) and np.array_equal(unfiltered, filtered)
