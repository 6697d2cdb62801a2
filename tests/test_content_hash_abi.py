"""The content-hash entry points of the C-ABI (no GPU needed): exported, listed, argument-checked,
and the SHA-1 kernel's register budget from the compiler's resource remarks.

ContentHelper#content_hash (content_helper.rb:136-138) runs one lane per file over the resident
texts (csrc/dice_hash.hip): the 16-word schedule, the prefetched block and the state stay in
VGPRs, so the kernel must compile without scratch or spills and fit at least 4 waves per SIMD."""
import os
import sys

import pytest

from licensee_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HIPCC = '/opt/rocm/bin/hipcc'
NAMES = ('dice_batch_content_hash', 'dice_batch_download_content_hash')


def test_symbols_exported_and_listed():
    lib = _native.load_library()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, 'include', 'licensee_dice.h')).read()
    for name in NAMES:
        assert f'int {name}(dice_batch *batch' in hdr, name


def test_null_batch_is_rejected():
    lib = _native.load_library()
    assert lib.dice_batch_content_hash(None, None) == -1
    assert b'NULL batch' in lib.dice_last_error()
    assert lib.dice_create(None, 0, None) == -1          # another message in between
    assert lib.dice_batch_download_content_hash(None, None, None, None) == -1
    assert b'NULL batch' in lib.dice_last_error()


def test_detection_field_is_last_and_defaulted():
    import dataclasses

    from licensee_amd.batch import Detection
    fields = dataclasses.fields(Detection)
    assert [f.name for f in fields] == ['license', 'matcher', 'confidence', 'content_hash']
    assert fields[-1].default is None
    assert Detection('l', 'dice', 99.0) == Detection('l', 'dice', 99.0, None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
def test_sha1_kernel_has_no_scratch_and_fits_4_waves():
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'licensee_amd', 'csrc', 'dice_hash.hip'))
    assert rows, 'no resource remarks (did the compile fail?)'
    r = next(v for v in rows if v['name'].endswith('dice::dice_sha1_kernel'))
    assert r['ScratchSize [bytes/lane]'] == '0' and r['VGPRs Spill'] == '0', r
    assert int(r['Occupancy [waves/SIMD]']) >= 4, r


def test_host_completion_hashes_equal_hashlib_of_normalize():
    """HostPrep.content_hashes (the completion of the files the device flags) is
    hashlib.sha1(content_normalized's UTF-8), for ASCII and non-ASCII texts, whatever buffer the
    previous file left behind."""
    import hashlib

    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from licensee_amd.native_host import HostPrep
    from licensee_amd.project_files import LicenseFile
    templates = License.all(hidden=True, pseudo=False)
    hp = HostPrep(TemplateCorpus(templates))
    texts = ['', 'MIT License\n\nCopyright (c) 2020 Zoë Ünïcode\n\nPermission is hereby granted…', 'x ' * 35000 + ' café',
             'short'] + [t.content_normalized() for t in templates if t.key in ('mit', 'eupl-1.2', 'cecill-2.1', 'mulanpsl-2.0')]
    names = ['LICENSE', 'LICENSE.md', None, 'COPYING'] + ['LICENSE.txt'] * (len(texts) - 4)
    assert len(texts) == 8
    got = hp.content_hashes(texts, names)
    for t, fn, h in zip(texts, names, got):
        want = hp.normalize(t, fn)
        assert want is not None and h == hashlib.sha1(want.encode('utf-8')).hexdigest(), fn
        if len(t) < 2000:    # (the per-file Python object, where it is quick)
            assert h == LicenseFile(t, fn or 'LICENSE').content_hash()
    assert got == hp.content_hashes([t.encode('utf-8') for t in texts], names)
