"""dice_words_kernel and dice_vocab_setup at their edges, against the regex reference of
tests/words_cases.py (no code shared with the host scan, oracle/ or test_gpu_words.py).

Every case goes through Scorer.vocab_setup, DeviceBatch.upload_text and download_rows; rows, |W_F|,
field masks and status are compared for every file of the batch, flagged files included (their
outputs are zero). Every case runs with the bytes outside the files (gaps, the buffer's tail) filled
with 0x00 and with "s's's...": bytes past a file's end must never reach the scan.
"""
import ctypes

import numpy as np
import pytest

from tests import words_cases as W

pytestmark = pytest.mark.gpu

CASES = W.all_cases()


def _scorer(vocab):
    from licensee_amd._native import Scorer
    return Scorer(*vocab.corpus_arrays(), device=0)


def _upload(b, files, fill, gaps=None, tail=0, utf8=False):
    text, off, tl = W.build_buffer(files, fill, gaps, tail)
    st = b.upload_text(text, off, tl, tl.copy(), np.zeros(len(files), np.uint8), utf8=utf8)
    return (*b.download_rows(), st)


def _assert_equal(vocab, files, got, what, ref=None):
    rows, wf, fm, st = ref or W.reference(vocab, files)
    assert all(a.shape[0] == len(files) for a in got)      # the comparison set is the whole batch
    for name, a, e in zip(('status', 'rows', '|W_F|', 'field mask'), (got[3], got[0], got[1], got[2]), (st, rows, wf, fm)):
        bad = np.nonzero((a != e).reshape(len(files), -1).any(axis=1))[0]
        assert np.array_equal(a, e), (what, name, [(int(i), files[i][:60], a[i].tolist(), e[i].tolist()) for i in bad[:3]])


@pytest.fixture(scope='module')
def scorers():
    cache = {}

    def get(vocab):
        key = (tuple(vocab.words), tuple(vocab.extra))
        if key not in cache:
            sc = _scorer(vocab)
            sc.vocab_setup(vocab.words, vocab.extra)
            cache[key] = sc
        return cache[key]
    yield get
    for sc in cache.values():
        sc.close()


@pytest.mark.parametrize('fill', sorted(W.FILLS))
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_equals_the_regex_reference(scorers, case, fill):
    sc = scorers(case.vocab)
    b = sc.batch(max(len(case.files), 1))
    ref = W.reference(case.vocab, case.files)
    for gaps, tail in ((case.gaps, case.tail), ([i % 3 for i in range(len(case.files))], 37)):
        got = _upload(b, case.files, W.FILLS[fill], gaps, tail)
        _assert_equal(case.vocab, case.files, got, (case.name, fill, tail), ref)
    b.close()


@pytest.mark.parametrize('fill', sorted(W.FILLS))
def test_overflow_count_equals_the_status_sum(scorers, fill):
    """S1 through the C call itself: n_overflow == sum(status) == the reference's flagged files."""
    from licensee_amd._native import _check, _ptr, load_library
    case = W.s1_capacity()[0]
    sc = scorers(case.vocab)
    n = len(case.files)
    b = sc.batch(n)
    text, off, tl = W.build_buffer(case.files, W.FILLS[fill])
    st, nov, cc = np.zeros(n, np.uint8), ctypes.c_int64(-1), np.zeros(n, np.uint8)
    _check(load_library().dice_batch_upload_text(b._b, n, _ptr(text), int(text.size), _ptr(off), _ptr(tl), _ptr(tl),
                                                 _ptr(cc), _ptr(st), ctypes.byref(nov), None))
    ref = W.reference(case.vocab, case.files)[3]
    assert ref.sum() > 0 and np.array_equal(st, ref) and nov.value == int(ref.sum())
    b.close()


@pytest.mark.parametrize('fill', sorted(W.FILLS))
def test_scheduling(scorers, fill):
    """n = 0, 1, 3, 4, 5 and 16 n_cu + 1 files (every wave of the grid takes a file, one takes two);
    upload_text and upload_text(utf8=True) on one batch, re-uploaded in both orders."""
    import torch
    sc = scorers(W.N_VOCAB)
    many = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    b = sc.batch(many)
    for n in W.N_SIZES + (many,):
        files = W.n_files(n)
        if n == 0:
            st = b.upload_text(np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32),
                               np.zeros(0, np.uint8))
            assert st.size == 0 and all(a.shape[0] == 0 for a in b.download_rows())
            continue
        ref = W.reference(W.N_VOCAB, files)
        for utf8 in (False, True, True, False):
            _assert_equal(W.N_VOCAB, files, _upload(b, files, W.FILLS[fill], utf8=utf8), (n, fill, utf8), ref)
    b.close()


def test_largest_vocabulary():
    """w64 = 3,936 (V = 251,904: the scan's workgroup declares 160 KiB of LDS) is accepted and scans
    equal to the reference; w64 = 3,937 is refused by dice_vocab_setup (DICE_E_ARG)."""
    from licensee_amd._native import DiceError
    case = W.l_largest()
    sc = _scorer(case.vocab)
    sc.vocab_setup(case.vocab.words)
    b = sc.batch(len(case.files))
    for fill in W.FILLS.values():
        _assert_equal(case.vocab, case.files, _upload(b, case.files, fill), ('L', fill))
    b.close()
    sc.close()
    over = W.l_vocab(W.L_W64 + 1)
    sc = _scorer(over)
    with pytest.raises(DiceError, match='dice error -1') as e:
        sc.vocab_setup(over.words)
    assert 'too large' in str(e.value)
    sc.close()
