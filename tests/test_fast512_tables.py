"""The tables of the 512-point fast path (shennong_amd/csrc/fast512_tables.cpp), built on the CPU.

tools/fast512_tables_digest.cpp is compiled against fast512_tables.cpp and host_tables.cpp - host code only, no
device and no library - and its output compared with profiles/fast512_tables_digest.txt: for every configuration of
its list (all kinds, 13- and 16-row windows, 256- and 128-sample frames, both forms of the 256-sample tables, both
DCT forms, VTLN-warped banks, the two shapes the builder refuses) the return code, every scalar of Fast512Params,
the length of the blob and a hash of its bytes.  This pins table BYTES: a change that means to alter the tables
records the file again (run the program, commit its output)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'shennong_amd', 'csrc')


def _compiler():
    for candidate in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


def test_fast512_tables_match_recorded_digest(tmp_path):
    hipcc = _compiler()
    if hipcc is None:
        pytest.skip('no hipcc to compile tools/fast512_tables_digest.cpp with')
    program = str(tmp_path / 'fast512_tables_digest')
    subprocess.run([hipcc, '-O1', '-std=c++17', '-o', program,
                    os.path.join(ROOT, 'tools', 'fast512_tables_digest.cpp'),
                    os.path.join(CSRC, 'fast512_tables.cpp'), os.path.join(CSRC, 'host_tables.cpp')],
                   check=True, cwd=str(tmp_path))
    got = subprocess.run([program], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
    with open(os.path.join(ROOT, 'profiles', 'fast512_tables_digest.txt')) as f:
        want = f.read().splitlines()
    assert [line.split()[:2] for line in got] == [line.split()[:2] for line in want], 'another list of configurations'
    for g, w in zip(got, want):
        assert g == w, 'tables of %s changed' % ' '.join(w.split()[:2])
    # the list reaches the builder's refusals and both table forms
    assert sum(' rc=1 ' in line for line in got) == 2
    assert any(' dual=1 ' in line for line in got) and any(' dct_mfma=1 ' in line for line in got)
