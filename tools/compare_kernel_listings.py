#!/usr/bin/env python3
"""Are the kernels of two sets of assembly listings the same code?  For a change that moves kernels between
translation units without editing them.

  hipcc $(CXXFLAGS) -S --cuda-device-only -o before.s kernels_x.hip      (at the parent commit)
  hipcc $(CXXFLAGS) -S --cuda-device-only -o after_1.s kernels_x.hip     (the candidate's files)
  hipcc $(CXXFLAGS) -S --cuda-device-only -o after_2.s kernels_y.hip
  tools/compare_kernel_listings.py --before before.s --after after_1.s after_2.s

Compares, per kernel symbol, the function's listing (from its label to its end label) and its kernel descriptor
(.amdhsa_kernel ... .end_amdhsa_kernel: registers, LDS, scratch) as text, after folding what moves with the
translation unit alone: the function's number in local labels (BB<n>_, .Lfunc_end<n>) and the comment column.
Prints the symbol counts and the symbols that differ; the exit status is the number of them (0: same code).
"""
import argparse
import re
import sys

_LABEL_NUMBER = re.compile(r'(\.LBB|\.Lfunc_begin|\.Lfunc_end)\d+')


def _normalise(line):
    line = line.split(';', 1)[0].rstrip()
    return _LABEL_NUMBER.sub(r'\1', line)


def kernels(path):
    """{symbol: normalised lines of its body and its descriptor} of every kernel of one listing"""
    with open(path) as f:
        lines = f.read().split('\n')
    names = [l.split()[1] for l in lines if l.strip().startswith('.amdhsa_kernel ')]
    out = {name: [] for name in names}
    current, closing = None, None
    for line in lines:
        stripped = line.strip()
        if current is None:
            label = stripped.split(':', 1)[0] if ':' in stripped else None
            if label in out and stripped.startswith(label + ':'):
                current, closing = label, re.compile(r'^\.Lfunc_end\d+:')
            elif stripped.startswith('.amdhsa_kernel ') and stripped.split()[1] in out:
                current, closing = stripped.split()[1], re.compile(r'^\.end_amdhsa_kernel')
            else:
                continue
        text = _normalise(line)
        if text:
            out[current].append(text)
        if closing.match(stripped):
            current = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--before', nargs='+', required=True)
    ap.add_argument('--after', nargs='+', required=True)
    args = ap.parse_args()
    sides = []
    for paths in (args.before, args.after):
        merged = {}
        for path in paths:
            found = kernels(path)
            dup = set(found) & set(merged)
            if dup:
                sys.exit('%s: kernel defined twice: %s' % (path, sorted(dup)[0]))
            merged.update(found)
            print('%-40s %4d kernels, %8d lines' % (path, len(found), sum(len(v) for v in found.values())))
        sides.append(merged)
    before, after = sides
    only_before, only_after = sorted(set(before) - set(after)), sorted(set(after) - set(before))
    differing = [name for name in sorted(set(before) & set(after)) if before[name] != after[name]]
    print('kernels before: %d  after: %d  only before: %d  only after: %d  differing: %d'
          % (len(before), len(after), len(only_before), len(only_after), len(differing)))
    for tag, names in (('only before', only_before), ('only after', only_after), ('differs', differing)):
        for name in names:
            print('  %s: %s' % (tag, name))
    return len(only_before) + len(only_after) + len(differing)


if __name__ == '__main__':
    sys.exit(min(main(), 255))
