import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the reference's raw data files the tests read (fixture license files, detect.json,
# license-hashes.json, the 47 choosealicense.com templates and their SPDX XMLs), archived at their paths
# in a reference checkout by tests/golden/make_golden.py; LICENSEE_REFERENCE names a whole checkout to
# read instead
REFERENCE_ARCHIVE = os.path.join(ROOT, 'tests', 'golden', 'reference.tar.xz')


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a gfx950 GPU (run on the MI355X box)')


def pytest_sessionstart(session):
    """GPU sessions: initialize torch's HIP runtime up front. The library shares it either way
    (licensee_amd._native maps torch's runtime before liblicensee_dice.so; tests/test_runtime.py
    checks the library-first order), so this only moves torch's device start-up out of the first
    test's time limit."""
    markexpr = getattr(session.config.option, 'markexpr', '') or ''
    if 'gpu' in markexpr and 'not gpu' not in markexpr:
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass


@pytest.fixture(scope='session')
def reference_root(tmp_path_factory):
    ref = os.environ.get('LICENSEE_REFERENCE')
    if ref:
        return ref
    import tarfile
    dst = tmp_path_factory.mktemp('reference')
    with tarfile.open(REFERENCE_ARCHIVE) as tar:
        tar.extractall(dst, **({'filter': 'data'} if hasattr(tarfile, 'data_filter') else {}))
    return str(dst)
