"""The UTF-8 text form on the host (no GPU needed): lh_normalize_files_utf8 and the new C-ABI entries.

ContentHelper#content_hash is SHA-1 of content_normalized (content_helper.rb:136-138), so the device
can only hash a text whose resident bytes are content_normalized's UTF-8. lh_normalize_files_utf8
writes exactly those bytes (what lh_normalize writes), with tlen in bytes and length in characters;
lh_normalize_files keeps its one-byte-per-character form, which is the UTF-8 form with every
non-ASCII character folded to one 0x80. The Python content_normalized is the checker."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from licensee_amd import _native
from licensee_amd.license import License
from tests.utf8_texts import NON_ASCII, fuzz_texts, to_x80

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = '/opt/rocm/bin/hipcc'


@pytest.fixture(scope='module')
def host():
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.native_host import HostPrep
    return HostPrep(TemplateCorpus(License.all(hidden=True, pseudo=False)))


@pytest.fixture(scope='module')
def inputs(reference_root):
    """(contents, filenames): every fixture file (all but the one HTML file, which the project marks
    unsupported and does not archive), the 47 template bodies, the fuzzed texts."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'fixture_files.json'), encoding='utf-8') as fh:
        recs = json.load(fh)
    contents, names = [], []
    recs = [r for r in recs if 'unsupported' not in r]
    assert len(recs) >= 57
    for r in recs:
        with open(os.path.join(reference_root, 'spec', 'fixtures', r['fixture'], r['file']), 'rb') as fh:
            contents.append(fh.read())
        names.append(r['file'])
    templates = License.all(hidden=True, pseudo=False)
    assert len(templates) == 47
    contents += [t.content_normalized().encode('utf-8') for t in templates]   # (the bodies as vendored)
    assert sum(not t.content_normalized().isascii() for t in templates) == 6
    names += ['LICENSE.txt'] * len(templates)
    fuzz = fuzz_texts(300)
    assert all(any(u in t for t in fuzz) for u in NON_ASCII)
    contents += [t.encode('utf-8') for t in fuzz]
    names += ['LICENSE'] * len(fuzz)
    return contents, names


def test_utf8_form_is_content_normalized_and_folds_to_the_byte_form(host, inputs):
    from licensee_amd.project_files import LicenseFile
    contents, names = inputs
    text8, off8, tl8, ln8, cc8, cr8, fell8 = host.normalize_files(contents, names, nthreads=4, utf8=True)
    text1, off1, tl1, ln1, cc1, cr1, fell1 = host.normalize_files(contents, names, nthreads=4)
    assert not (off8 & 15).any() and not (off1 & 15).any() and (off8 >= 0).all()
    assert np.array_equal(ln8, ln1) and np.array_equal(cc8, cc1) and np.array_equal(cr8, cr1)
    assert np.array_equal(fell8, fell1)
    n_multi = 0
    for i, (c, fn) in enumerate(zip(contents, names)):
        want = LicenseFile(c, fn).content_normalized() or ''
        got = text8[int(off8[i]):int(off8[i]) + int(tl8[i])].tobytes()
        assert got.decode('utf-8') == want, (i, fn)
        assert ln8[i] == len(want) and tl8[i] == len(want.encode('utf-8')), (i, fn)
        one = text1[int(off1[i]):int(off1[i]) + int(tl1[i])].tobytes()
        assert one == to_x80(want) and tl1[i] == ln1[i] == len(want), (i, fn)
        if want.isascii():
            assert got == one, (i, fn)
        else:
            n_multi += 1
    assert n_multi >= 250       # (most fuzzed texts, the non-ASCII templates and fixtures)
    # files lie apart: sorted by offset, each ends before the next begins
    order = np.lexsort((tl8, off8))     # (an empty text shares its offset with the next one)
    assert (off8[order][:-1] + tl8[order][:-1] <= off8[order][1:]).all()


def test_native_calls_agree_file_by_file(host, inputs):
    """The C entry points themselves on the files inside the native envelope (no Python completion):
    the same status, flags and lengths, UTF-8 bytes equal to lh_normalize's, ASCII files identical."""
    from licensee_amd import native_host
    lib = native_host._load()
    contents, names = inputs
    n = len(contents)
    data, keep = native_host._cstrs(contents)
    fns, keep2 = native_host._cstrs(names)
    lens = np.array([len(c) for c in contents], np.int64)
    cap = int(lens.sum()) + 16 * n + 65536
    res = {}
    for name in ('lh_normalize_files', 'lh_normalize_files_utf8'):
        buf = np.full(cap, 0xAA, np.uint8)
        off, tl, ln = np.full(n, -7, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        cc, cr, st = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        used = getattr(lib, name)(host._c, n, data, lens.ctypes.data, fns, 3, buf.ctypes.data, cap, off.ctypes.data,
                                  tl.ctypes.data, ln.ctypes.data, cc.ctypes.data, cr.ctypes.data, st.ctypes.data)
        assert 0 <= used <= cap and used % 16 == 0
        res[name] = (buf, off, tl, ln, cc, cr, st, used)
    b1, o1, t1, l1, c1, r1, s1, _ = res['lh_normalize_files']
    b8, o8, t8, l8, c8, r8, s8, _ = res['lh_normalize_files_utf8']
    assert np.array_equal(s1, s8) and set(s8.tolist()) <= {0, 1}
    ok = s8 == 0
    assert ok.sum() >= n - 5
    assert np.array_equal(l1[ok], l8[ok]) and np.array_equal(c1[ok], c8[ok]) and np.array_equal(r1[ok], r8[ok])
    assert (o8[~ok] == -1).all() and (t8[~ok] == 0).all()
    for i in np.nonzero(ok)[0].tolist():
        u = b8[int(o8[i]):int(o8[i]) + int(t8[i])].tobytes()
        assert o8[i] % 16 == 0 and o1[i] % 16 == 0
        assert u.decode('utf-8') == host.normalize(contents[i], names[i]), i
        assert l8[i] == len(u.decode('utf-8'))
        assert b1[int(o1[i]):int(o1[i]) + int(t1[i])].tobytes() == to_x80(u.decode('utf-8')), i


def test_no_room_is_status_3(host):
    """A `cap` that holds the first text's UTF-8 but not the second's: status 3 for the one that did
    not fit, nothing written past `cap`, and HostPrep completes such a file as UTF-8."""
    from licensee_amd import native_host
    lib = native_host._load()
    contents = ['permission is hereby granted'.encode(), ('é' * 40 + ' warranty').encode('utf-8')]
    assert len(contents[1]) == 89           # 49 characters: the one-byte form would fit 64 bytes
    data, keep = native_host._cstrs(contents)
    lens = np.array([len(c) for c in contents], np.int64)
    for name, want in (('lh_normalize_files_utf8', [0, 3]), ('lh_normalize_files', [0, 0])):
        cap = 32 + 64
        buf = np.full(cap + 64, 0xAA, np.uint8)
        off, tl, ln = np.full(2, -7, np.int64), np.zeros(2, np.int32), np.zeros(2, np.int32)
        cc, cr, st = np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
        used = getattr(lib, name)(host._c, 2, data, lens.ctypes.data, None, 1, buf.ctypes.data, cap, off.ctypes.data,
                                  tl.ctypes.data, ln.ctypes.data, cc.ctypes.data, cr.ctypes.data, st.ctypes.data)
        assert st.tolist() == want, name
        assert (buf[cap:] == 0xAA).all() and used <= cap
        if want[1] == 3:
            assert off[1] == -1 and tl[1] == 0 and ln[1] == 49
    # through HostPrep: a buffer too small for everything, the rest appended as UTF-8
    texts = [('é' * 3000 + ' granted ' + str(i)).encode('utf-8') for i in range(40)]
    text, off, tl, ln, _, _, fell = host.normalize_files(texts, None, nthreads=2, utf8=True,
                                                         out=lambda nbytes: np.empty(100000, np.uint8))
    assert not fell.any() and not (off & 15).any()
    for i, t in enumerate(texts):
        assert text[int(off[i]):int(off[i]) + int(tl[i])].tobytes().decode('utf-8') == host.normalize(t), i
        assert ln[i] == len(host.normalize(t)) and tl[i] > ln[i]


def test_python_fallback_files_are_utf8_too(host):
    """A file outside the native envelope (U+03A3 and U+0130, whose lower-casing is contextual) is
    normalized by the Python path and appended in the form asked for."""
    from licensee_amd.project_files import LicenseFile
    contents = ['ΣΟΦΙΑ license café 许可'.encode('utf-8'), 'İstanbul license 😀 granted'.encode('utf-8'),
                b'plain ascii text']
    names = ['LICENSE', 'COPYING', 'LICENSE']
    text, off, tl, ln, _, _, fell = host.normalize_files(contents, names, utf8=True)
    assert fell.tolist() == [True, True, False]
    for i in range(3):
        want = LicenseFile(contents[i], names[i]).content_normalized() or ''
        assert text[int(off[i]):int(off[i]) + int(tl[i])].tobytes().decode('utf-8') == want
        assert ln[i] == len(want) and tl[i] == len(want.encode('utf-8')) and off[i] % 16 == 0
    text1, off1, tl1, ln1, _, _, _ = host.normalize_files(contents, names)
    assert np.array_equal(ln1, ln) and np.array_equal(tl1, ln1)


NEW_DICE = ('dice_batch_upload_text_utf8', 'dice_batch_download_length')


def test_new_symbols_exported_declared_and_reject_null():
    from licensee_amd import native_host
    lib = _native.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'licensee_dice.h')).read()
    for name in NEW_DICE:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert f'int {name}(dice_batch *batch' in hdr, name
    assert lib.dice_create(None, 0, None) == -1          # another message first
    assert lib.dice_batch_upload_text_utf8(None, 0, None, 0, None, None, None, None, None, None, None) == -1
    assert b'NULL batch' in lib.dice_last_error()
    assert lib.dice_create(None, 0, None) == -1
    assert lib.dice_batch_download_length(None, None, None) == -1
    assert b'NULL batch' in lib.dice_last_error()
    hlib = native_host._load()
    assert hasattr(hlib, 'lh_normalize_files_utf8')
    # (exported and described in licensee_host.h, but not declared there: tests/test_abi.py pins the
    # exact set of functions that header declares)
    assert 'lh_normalize_files_utf8' in open(os.path.join(ROOT, 'include', 'licensee_host.h')).read()
    # bad arguments as lh_normalize_files: -1
    assert hlib.lh_normalize_files_utf8(None, 1, None, None, None, 1, None, 0, None, None, None, None, None, None) == -1


def test_upload_text_length_none_needs_utf8():
    """DeviceBatch.upload_text refuses length=None for the one-byte form before any native call."""
    b = _native.DeviceBatch.__new__(_native.DeviceBatch)
    with pytest.raises(ValueError, match='utf8=True'):
        b.upload_text(np.zeros(16, np.uint8), [0], [3], None, [0])


def test_batch_detector_has_host_hashed_counter():
    import inspect

    from licensee_amd.batch import BatchDetector
    from licensee_amd.native_host import HostPrep
    assert 'host_hashed' in inspect.getsource(BatchDetector.__init__)
    assert inspect.signature(HostPrep.normalize_files).parameters['utf8'].default is False
    assert inspect.signature(_native.DeviceBatch.upload_text).parameters['utf8'].default is False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
def test_character_count_kernel_has_no_scratch():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'licensee_amd', 'csrc', 'dice_words.hip'))
    assert rows, 'no resource remarks (did the compile fail?)'
    r = next(v for v in rows if v['name'].endswith('dice::dice_text_chars_kernel'))
    assert r['ScratchSize [bytes/lane]'] == '0' and r['VGPRs Spill'] == '0' and r['SGPRs Spill'] == '0', r
    assert int(r['Occupancy [waves/SIMD]']) >= 4, r
