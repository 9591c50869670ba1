#!/usr/bin/env python
"""Times the ABX scores (shennong_amd.abx.abx_scores: snf_dtw_pairs + snf_abx_cells) on one MI355X, one JSON line
per task, and sweeps the two thresholds of snf_abx_cells.

    python tools/time_abx.py [within across] [--items 100000] [--repeat 7] [--out profiles/abx_timing.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/time_abx.py --sweep [--repeat 7] --plan DIR/plan.json
    python tools/time_abx.py --trace DIR/.../*_kernel_trace.csv --plan DIR/plan.json [--out profiles/abx_timing.jsonl]

The corpus is synthetic and seeded: `--items` items of 5 to 30 frames at D = 39 (standard-normal float32 rows), one
utterance each, with labels drawn uniformly from 40 phones, 20 talkers and 200 contexts.  The two tasks are those of
the reference's run.sh: within (on phone, by talker and context) and across (on phone, across talker, by context).
Per task, after one warm-up pass, the median of `--repeat` passes of the host's wall clock for every step of
``abx_scores``, each on its own:
  build_ms        host task construction (``build_task``, the runs, the pair and record tables of every run)
  dtw_call_ms     the ``snf_dtw_pairs`` calls, which return once their kernels are enqueued: the check, sort and
                  upload of the pair table
  dtw_wait_ms     from their return to the end of the stream.  NOT the kernels' time: the kernels start while the
                  call is still returning (it frees its tables behind the launch), as tools/time_dtw.py found
  abx_call_ms, abx_wait_ms   the same two for ``snf_abx_cells``
  table_ms        download of the counts and the table
and the sizes: items, blocks, cells, triplets, pairs computed, the share of them that no triplet reads.  For scale
only: the numpy statement (tests/abx_np.py ``cell_counts``) on a 1 % sample of the cells, from distances brought to
the host for that purpose, and whether it agrees with the device's counts there.  The kernels' own times: this
command under ``rocprofv3 --kernel-trace --stats``, one task per run (its kernel_stats.csv; `--repeat` + 1 calls).

`--sweep` runs snf_abx_cells alone on synthetic distances (small integers), `--repeat` + 1 calls per setting, with
the thresholds set through SNF_ABX_SMALL_WORK and SNF_ABX_SPLIT_WORK:
  small  200 000 cells of k x k x k for k = 1 .. 10, every cell by one lane against every cell by one wave
  split  one cell of 2048 x 2048 x 1100 and 64 cells of 256 x 256 x 256, cut into stretches of 2^16 .. 2^26 compares
         and not cut at all
and writes to `--plan` which kernel every setting dispatches, in order.  It takes no kernel time itself: run it
under rocprofv3 as above, then `--trace` reads the kernels' durations from the dispatch trace of that run, in the
order of the plan, and gives per setting the median of the `--repeat` dispatches behind the warm-up (one dispatch
per call: the zeroing of the counts ahead of a cut cell is a fill of the runtime's, not counted).
`--out` appends the lines."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

TASKS = {'within': dict(on='phone', across=None, by=['talker', 'context']),
         'across': dict(on='phone', across='talker', by=['context'])}
PHONES, TALKERS, CONTEXTS, DIM, FRAMES = 40, 20, 200, 39, (5, 30)


def median(values):
    return float(np.median(values))


def make(n_items, seed):
    """(host collection of one utterance per item, AbxItems)"""
    import dtw_cases
    from shennong_amd.abx import AbxItems
    rng = np.random.default_rng(seed)
    frames = rng.integers(FRAMES[0], FRAMES[1] + 1, size=n_items)
    block = rng.standard_normal((int(frames.sum()), DIM), dtype=np.float32)
    starts = np.concatenate([[0], np.cumsum(frames)[:-1]])
    feats = dtw_cases.collection([block[a:a + n] for a, n in zip(starts.tolist(), frames.tolist())])
    labels = {'phone': np.array(['p%02d' % k for k in rng.integers(0, PHONES, n_items)]),
              'talker': np.array(['t%02d' % k for k in rng.integers(0, TALKERS, n_items)]),
              'context': np.array(['c%03d' % k for k in rng.integers(0, CONTEXTS, n_items)])}
    items = AbxItems(['item%d' % k for k in range(n_items)], np.zeros(n_items), np.full(n_items, 1e9), labels)
    return feats, items


def unread_share(records, n_pairs):
    """Share of the `n_pairs` distances that no record reads"""
    marks = np.zeros(n_pairs + 1, dtype=np.int64)
    for off, count in ((0, 3), (1, 4)):
        rep = np.repeat(np.arange(records.shape[0]), records[:, 5])
        x = np.arange(rep.shape[0]) - np.repeat(np.cumsum(records[:, 5]) - records[:, 5], records[:, 5])
        lo = records[rep, off] + x * records[rep, 2]
        marks += np.bincount(lo, minlength=n_pairs + 1)
        marks -= np.bincount(lo + records[rep, count], minlength=n_pairs + 1)
    return float((np.cumsum(marks[:-1]) == 0).mean())


def run_task(name, args):
    import abx_np
    from shennong_amd import _backend, abx
    from shennong_amd.device import DeviceFeaturesCollection
    kind = TASKS[name]
    feats, items = make(args.items, seed=len(name))
    resident = DeviceFeaturesCollection.from_host(feats)
    first, count, dim, block = abx._resolve(resident, items)
    buffer = block.alive()
    L = _backend.lib()
    stream = C.c_void_p()
    _backend.check(L.snf_stream_create(C.byref(stream)))
    sync = lambda: _backend.check(L.snf_stream_synchronize(stream))   # noqa: E731
    steps = {key: [] for key in ('build_ms', 'dtw_call_ms', 'dtw_wait_ms', 'abx_call_ms', 'abx_wait_ms',
                                 'table_ms')}
    sizes, sample = {}, {}
    for turn in range(args.repeat + 1):   # (turn 0: the warm-up)
        spent = dict.fromkeys(steps, 0.0)
        t0 = time.perf_counter()
        task = abx.build_task(items.labels, **kind)
        runs = task.runs(args.max_pairs)
        tables = [task.tables(blocks) for blocks in runs]
        spent['build_ms'] += 1e3 * (time.perf_counter() - t0)
        counts = np.zeros((task.n.shape[0], 3), dtype=np.uint64)
        for pairs, records, cells in tables:
            n_pairs = pairs.shape[0]
            d_cost, d_len = _backend.DeviceBuffer(4 * n_pairs), _backend.DeviceBuffer(4 * n_pairs)
            d_counts = _backend.DeviceBuffer(24 * cells.shape[0])
            sync()
            t0 = time.perf_counter()
            _backend.dtw_pairs(buffer.ptr, dim, first, count, pairs, args.metric, d_cost.ptr, d_len.ptr,
                               stream=stream.value)
            t1 = time.perf_counter()
            sync()
            t2 = time.perf_counter()
            _backend.abx_cells(d_cost.ptr, d_len.ptr, n_pairs, records, d_counts.ptr, stream=stream.value)
            t3 = time.perf_counter()
            sync()
            t4 = time.perf_counter()
            got = d_counts.download(np.zeros((cells.shape[0], 3), dtype=np.uint64))
            counts[cells] = got
            t5 = time.perf_counter()
            for key, value in (('dtw_call_ms', t1 - t0), ('dtw_wait_ms', t2 - t1), ('abx_call_ms', t3 - t2),
                               ('abx_wait_ms', t4 - t3), ('table_ms', t5 - t4)):
                spent[key] += 1e3 * value
            if turn == 0 and not sizes.get('sampled'):   # the first run of the warm-up: sizes, and the statement
                sizes['sampled'] = True
                sizes['unread_share_first_run'] = unread_share(records, n_pairs)
                cost = d_cost.download(np.zeros(n_pairs, dtype=np.float32))
                length = d_len.download(np.zeros(n_pairs, dtype=np.int32))
                values = cost / length.astype(np.float32)
                pick = np.random.default_rng(1).choice(cells.shape[0], size=max(cells.shape[0] // 100, 1),
                                                       replace=False)
                t0 = time.perf_counter()
                want = np.array([abx_np.cell_counts(values, records[c]) for c in pick], dtype=np.uint64)
                sample = {'statement_cells': int(pick.shape[0]),
                          'statement_ms_per_cell': 1e3 * (time.perf_counter() - t0) / pick.shape[0],
                          'statement_agrees': bool(np.array_equal(want, got[pick]))}
                del cost, length, values
            for one in (d_cost, d_len, d_counts):
                one.free()
        t0 = time.perf_counter()
        table = abx._table(task, counts)
        spent['table_ms'] += 1e3 * (time.perf_counter() - t0)
        print(name, 'pass', turn, {key: round(value, 1) for key, value in spent.items()}, file=sys.stderr, flush=True)
        if turn:
            for key in steps:
                steps[key].append(spent[key])
    sizes.pop('sampled', None)
    levels = [['context', 'phone_1', 'phone_2'], ['phone_1', 'phone_2']]
    line = {'task': name, 'metric': args.metric, 'device': _backend.device_name(0), 'items': args.items,
            'phones': PHONES, 'talkers': TALKERS, 'contexts': CONTEXTS, 'frames': list(FRAMES), 'dim': DIM,
            'repeat': args.repeat, 'max_pairs': args.max_pairs, 'runs': len(runs),
            'blocks': int(np.unique(task.cell_block).shape[0]), 'cells': int(task.n.shape[0]),
            'triplets': int(task.n.sum()), 'pairs': int(sum(t[0].shape[0] for t in tables)),
            'cells_of_one_triplet': int((task.n == 1).sum()), 'largest_cell': int(task.n.max()),
            'error_rate': table.error_rate(levels)}
    line.update(sizes)
    line.update(sample)
    for key, values in steps.items():
        line[key] = sorted(values)
        line[key.replace('_ms', '_median_ms')] = median(values)
    line['total_median_ms'] = sum(median(values) for values in steps.values())
    L.snf_stream_destroy(stream)
    resident.release()
    return line


def call_cells(values, records, repeat):
    """`repeat` + 1 calls of snf_abx_cells: (median wall clock of the call, ms; the counts)"""
    from shennong_amd import _backend
    d_values, d_counts = _backend.DeviceBuffer(values.nbytes), _backend.DeviceBuffer(24 * len(records))
    d_values.upload(values)
    host = []
    for turn in range(repeat + 1):
        t0 = time.perf_counter()
        _backend.abx_cells(d_values.ptr, None, values.shape[0], records, d_counts.ptr)   # (waits for its stream)
        if turn:
            host.append(1e3 * (time.perf_counter() - t0))
    counts = d_counts.download(np.zeros((len(records), 3), dtype=np.uint64))
    d_values.free()
    d_counts.free()
    return median(host), counts


def sweep(args):
    """The plan: one entry per setting, in the order run, with the kernel that each of its calls dispatches once"""
    from shennong_amd import _backend
    rng = np.random.default_rng(5)
    plan = []
    n_cells = 200000
    values = rng.integers(0, 8, size=1 << 22).astype(np.float32)
    for k in range(1, 11):
        records = np.zeros((n_cells, 8), dtype=np.int64)
        stride = 2 * k + 3
        records[:, 0] = rng.integers(0, values.shape[0] - k * stride - 2 * k - 8, size=n_cells)
        records[:, 1] = records[:, 0] + k + 1
        records[:, 2] = stride
        records[:, 3:6] = k
        sums = set()
        for label, small, kernel in (('lane', 1 << 40, 'abx_small_kernel'), ('wave', 0, 'abx_wave_kernel')):
            os.environ['SNF_ABX_SMALL_WORK'] = str(small)
            call_ms, counts = call_cells(values, records, args.repeat)
            plan.append({'sweep': 'small', 'cells': n_cells, 'shape': [k, k, k], 'work': k ** 3, 'path': label,
                         'kernel': kernel, 'call_wall_ms': call_ms})
            sums.add(int(counts.sum()))
        assert len(sums) == 1
    os.environ.pop('SNF_ABX_SMALL_WORK', None)
    cases = {'one cell of 2048 x 2048 x 1100': [(2048, 2048, 1100)], '64 cells of 256 x 256 x 256': [(256,) * 3] * 64}
    for what, shapes in cases.items():
        records, base = [], 0
        for n_a, n_b, n_x in shapes:
            records.append([base, base + n_a, n_a + n_b, n_a, n_b, n_x, 0, 0])
            base += n_x * (n_a + n_b)
        records = np.array(records, dtype=np.int64)
        values = rng.integers(0, 8, size=base).astype(np.float32)
        sums = set()
        for log2 in (16, 18, 20, 22, 24, 26, 62):
            os.environ['SNF_ABX_SPLIT_WORK'] = str(1 << log2)
            call_ms, counts = call_cells(values, records, args.repeat)
            plan.append({'sweep': 'split', 'cells': what, 'split_work_log2': log2, 'kernel': 'abx_wave_kernel',
                         'work': int((records[:, 3] * records[:, 4] * records[:, 5]).sum()),
                         'call_wall_ms': call_ms})
            sums.add(int(counts.sum()))
        assert len(sums) == 1
    os.environ.pop('SNF_ABX_SPLIT_WORK', None)
    for row in plan:
        row['device'], row['repeat'] = _backend.device_name(0), args.repeat
    return plan


def from_trace(plan, path):
    """The plan's lines with `kernel_ms`, the median duration of every setting's dispatches behind its warm-up,
    read from rocprofv3's kernel_trace.csv of the run that wrote the plan"""
    import csv
    found = {}
    with open(path, newline='') as stream:
        reader = csv.DictReader(stream)
        column = {key.lower(): key for key in reader.fieldnames}
        name, start, end = column['kernel_name'], column['start_timestamp'], column['end_timestamp']
        for row in reader:
            for kernel in ('abx_small_kernel', 'abx_wave_kernel'):
                if kernel in row[name]:
                    found.setdefault(kernel, []).append((int(row[start]), int(row[end])))
    for spans in found.values():
        spans.sort()
    taken = dict.fromkeys(found, 0)
    for row in plan:
        calls, kernel = row['repeat'] + 1, row['kernel']
        spans = found[kernel][taken[kernel]:taken[kernel] + calls]
        taken[kernel] += calls
        assert len(spans) == calls, (row, len(spans))
        durations = [1e-6 * (end - start) for start, end in spans[1:]]
        row['kernel_ms'], row['kernel_ms_all'] = median(durations), sorted(durations)
        row['source'] = 'rocprofv3 --kernel-trace, one dispatch per call'
    assert all(taken[kernel] == len(found[kernel]) for kernel in found), (taken, {k: len(v) for k, v in found.items()})
    return plan


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('tasks', nargs='*', help='within, across (default: both)')
    parser.add_argument('--items', type=int, default=100000)
    parser.add_argument('--repeat', type=int, default=7)
    parser.add_argument('--metric', default='cosine')
    parser.add_argument('--max-pairs', type=int, default=1 << 26)
    parser.add_argument('--sweep', action='store_true')
    parser.add_argument('--plan', help='with --sweep: where the plan goes; with --trace: where it is')
    parser.add_argument('--trace', help="rocprofv3's kernel_trace.csv of the --sweep run")
    parser.add_argument('--out')
    args = parser.parse_args()
    if set(args.tasks) - set(TASKS):
        parser.error('tasks are ' + ', '.join(sorted(TASKS)))
    if args.sweep:
        if not args.plan:
            parser.error('--sweep needs --plan')
        with open(args.plan, 'w') as fh:
            json.dump(sweep(args), fh)
        return
    if args.trace:
        with open(args.plan) as fh:
            lines = from_trace(json.load(fh), args.trace)
    else:
        lines = (run_task(name, args) for name in args.tasks or sorted(TASKS, reverse=True))
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(text + '\n')


if __name__ == '__main__':
    main()
