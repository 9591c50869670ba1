#!/usr/bin/env python
"""Turns a pretrained CREPE Keras weights file ``model-<capacity>.h5`` (the files the CREPE package publishes,
https://github.com/marl/crepe) into the ``model-<capacity>.npz`` that
shennong_amd.processor.CrepePitchProcessor looks up under SHENNONG_AMD_CREPE_DIR.

    python tools/convert_crepe_h5.py model-tiny.h5 [output directory]

The .npz holds one float32 array per weight under the Keras layer names: conv{1..6}/kernel, conv{1..6}/bias,
conv{l}-BN/{gamma,beta,moving_mean,moving_variance}, classifier/{kernel,bias}.  Every shape is checked against
the capacity named in the file name before anything is written.

h5py is imported when the tool runs.  It was not importable where this tool was written, so the tool has never
been run against a published file: the layout it expects - one HDF5 group per layer holding datasets named
``<layer>/<weight>:0`` at any depth - is the one Keras 2 writes with ``save_weights``.
"""

import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_h5(path):
    """name -> array for every dataset of the file, keyed by '<layer>/<weight>'"""
    import h5py
    arrays = {}

    def visit(name, node):
        if isinstance(node, h5py.Dataset):
            parts = name.split('/')
            weight = parts[-1].split(':')[0]
            arrays['%s/%s' % (parts[-2], weight)] = np.asarray(node)

    with h5py.File(path, 'r') as handle:
        root = handle['model_weights'] if 'model_weights' in handle else handle
        root.visititems(visit)
    return arrays


def main(argv):
    if len(argv) not in (2, 3):
        sys.exit(__doc__)
    source = argv[1]
    match = re.search(r'model-(tiny|small|medium|large|full)\.h5$', os.path.basename(source))
    if not match:
        sys.exit('the file name must be model-<capacity>.h5, it is %s' % os.path.basename(source))
    capacity = match.group(1)
    from shennong_amd.processor import pitch_crepe
    arrays = read_h5(source)
    pitch_crepe._validate(arrays, capacity, os.path.basename(source))
    shapes = pitch_crepe.expected_shapes(capacity)
    target = os.path.join(argv[2] if len(argv) == 3 else os.path.dirname(os.path.abspath(source)),
                          'model-%s.npz' % capacity)
    np.savez(target, **{name: np.asarray(arrays[name], dtype=np.float32) for name in shapes})
    print('wrote %s (%d arrays)' % (target, len(shapes)))


if __name__ == '__main__':
    main(sys.argv)
