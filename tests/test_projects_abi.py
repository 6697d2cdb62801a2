"""The project entry points of the C-ABI (no GPU needed): exported, listed, argument-checked, and
the project kernel's resources from the compiler's remarks.

Project#license (projects/project.rb:24-32) is a segmented reduction over the resident per-file
results (csrc/dice_project.hip): a lane per small project with its licenses in registers (static
indices only), a wave per large one with an LDS bitset -- it must compile without scratch."""
import ctypes
import os
import sys

import pytest

from licensee_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HIPCC = '/opt/rocm/bin/hipcc'
NAMES = ('dice_batch_projects', 'dice_batch_download_projects', 'dice_batch_download_project_match')


def test_symbols_exported_and_listed():
    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'licensee_dice.h')).read()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert f'int {name}(dice_batch *batch' in hdr, name
    assert '#define DICE_PROJECT_K_MAX 8' in hdr and _native.DICE_PROJECT_K_MAX == 8
    assert 'project.rb' in hdr


def test_null_batch_and_argument_errors():
    lib = _native.load_library()
    off = (ctypes.c_int64 * 1)(0)
    fl = (ctypes.c_uint8 * 1)(0)
    args = (ctypes.cast(off, ctypes.c_void_p), ctypes.cast(fl, ctypes.c_void_p), ctypes.cast(fl, ctypes.c_void_p))
    assert lib.dice_batch_projects(None, 0, *args, 1, 4, None) == -1
    assert b'NULL batch' in lib.dice_last_error()
    assert lib.dice_batch_projects(None, -1, *args, 1, 4, None) == -1
    assert b'n_projects' in lib.dice_last_error()
    for k in (-1, 9):
        assert lib.dice_batch_projects(None, 0, *args, 1, k, None) == -1
        assert b'k_licenses' in lib.dice_last_error()
    assert lib.dice_batch_download_projects(None, None, None, None, None, None) == -1
    assert b'NULL batch' in lib.dice_last_error()
    assert lib.dice_create(None, 0, None) == -1          # another message in between
    assert lib.dice_batch_download_project_match(None, None, None, None, None) == -1
    assert b'NULL batch' in lib.dice_last_error()


def test_project_detection_has_slots():
    from licensee_amd.batch import ProjectDetection
    assert ProjectDetection.__slots__ == ('license', 'matched_file', 'matcher', 'confidence', 'licenses', 'n_licenses',
                                          'n_files', 'content_hash')
    d = ProjectDetection(None, None, None, None, [], 0, 0)
    assert d.content_hash is None and not hasattr(d, '__dict__')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
def test_project_kernel_has_no_scratch():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'licensee_amd', 'csrc', 'dice_project.hip'))
    assert rows, 'no resource remarks (did the compile fail?)'
    r = next(v for v in rows if v['name'].endswith('dice::dice_project_kernel'))
    assert r['ScratchSize [bytes/lane]'] == '0' and r['VGPRs Spill'] == '0' and r['SGPRs Spill'] == '0', r
    assert r['Dynamic Stack'] == 'False', r
    assert int(r['Occupancy [waves/SIMD]']) >= 4, r
