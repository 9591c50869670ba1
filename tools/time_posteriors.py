#!/usr/bin/env python
"""Times the dense GMM posteriors (snf_gmm_posteriors) beside the E-step (snf_gmm_accumulate) on the same block of
frames on one MI355X, one JSON line.

    python tools/time_posteriors.py [--frames 500000] [--gauss 1024] [--dim 39] [--repeat 7] [--out FILE]

After one warm-up call each, the median of `--repeat` runs of the wall clock of the C call on frames and a model that
lie in HBM (the call waits for its stream before it returns).  The kernels alone: this command under
``rocprofv3 --kernel-trace --stats``.  `--out` appends the line."""
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


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--frames', type=int, default=500000)
    parser.add_argument('--gauss', type=int, default=1024)
    parser.add_argument('--dim', type=int, default=39)
    parser.add_argument('--repeat', type=int, default=7)
    parser.add_argument('--out')
    args = parser.parse_args()
    from shennong_amd import _backend
    from shennong_amd import gmm as G
    from test_ubm_gpu import mixture
    F, n, D = args.frames, args.gauss, args.dim
    x, gmm = mixture(1, F, D, n)
    block, dg = G.FrameBlock([x]), G.DeviceGmm(gmm)
    L = _backend.lib()
    post = _backend.DeviceBuffer(4 * F * n)
    stats = _backend.DeviceBuffer(8 * n * (2 * D + 1) + 8)
    frames = C.c_void_p(block.frames.ptr)

    def posteriors():
        _backend.check(L.snf_gmm_posteriors(0, frames, F, D, *dg.args(), C.c_void_p(post.ptr), None, None))

    def accumulate():
        _backend.check(L.snf_gmm_accumulate(0, frames, F, D, None, *dg.args(), C.c_void_p(stats.ptr),
                                            C.c_void_p(stats.ptr + 8 * n * (2 * D + 1)), None, None))

    line = {'device': _backend.device_name(0), 'frames': F, 'num_gauss': n, 'dim': D, 'repeat': args.repeat,
            'posterior_bytes': 4 * F * n}
    for name, call in (('posteriors', posteriors), ('accumulate', accumulate)):
        call()
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            call()
            ms.append(1e3 * (time.perf_counter() - t0))
        line[name + '_ms'] = sorted(ms)
        line[name + '_median_ms'] = float(np.median(ms))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
