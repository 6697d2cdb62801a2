"""GPU parity of the top-k-only path: Scorer.topk / DeviceBatch.topk / topk_sharded /
DiceEngine.closest_files (dice_topk, dice_batch_topk, dice_topk_sharded; include/licensee_dice.h).

The path answers `licensee detect`'s "closest licenses" (detect.rb:96-106 over dice.rb:34-41): per
file its k best potential matches, ranked exactly as dice_batch_matrix(k) ranks them, without the
N x T matrix. Every comparison is bit-exact (np.array_equal; scores with ==) against the C oracle's
ranking -- the lexsort over OracleScorer.matrix with the CC mask, as tests/test_gpu_corpus_sizes.py
builds it -- and against the matrix call's own top-k, on every kernel family a context can select:
the sparse program (both tile layouts; under DICE_PROG_MATCH=valu and =mfma, which moves match mode
to the matrix cores and must leave this call on the VALU program with the same results), the postings
kernels, the LDS-record kernel and the dense kernel.
"""
import functools

import numpy as np
import pytest

from tests.helpers import ArrayCorpus, NormFile, make_files, outside_fast_envelope, widen_lanes
from tests.test_gpu_corpus_sizes import KIND, corpus_of, select_kernel
from tests.test_topk_abi import DICE_E_ARG, DICE_E_STATE, assert_topk, expected_topk, tie_rate

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 5, 16)
SMALL_N = (1, 63, 64, 65, 700)
# T <= 64: the sparse program under both settings of the match stage's switch, and the dense kernel;
# the full-bitset tile layout once, on the vendored 47
SMALL_CASES = [(t, v) for t in (1, 2, 5, 33, 47, 64) for v in ('valu', 'mfma', 'dense')] + [(47, 'bits')]
LARGE_CASES = [(t, v) for t in (65, 130, 700) for v in ('post', 'lds', 'dense')]


def _head(fb, n):
    from licensee_amd._native import FileBatch
    return FileBatch(fb.bits[:n], fb.wordset_size[:n], fb.length[:n], fb.cc_false_positive[:n])


def _scorer(c, monkeypatch, variant):
    """A Scorer on the kernel family `variant` names (select_kernel of test_gpu_corpus_sizes)."""
    from licensee_amd._native import Scorer
    monkeypatch.delenv('DICE_PROG_MATCH', raising=False)
    monkeypatch.delenv('DICE_PROG_LAYOUT', raising=False)
    if variant in ('valu', 'mfma'):
        monkeypatch.setenv('DICE_PROG_MATCH', variant)
    if variant == 'bits':
        monkeypatch.setenv('DICE_PROG_LAYOUT', 'bits')
    kernel = variant if variant in KIND else 'program'
    select_kernel(monkeypatch, kernel)
    sc = Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab, device=0)
    assert sc.info()[2] == KIND[kernel], (variant, sc.info())
    if variant == 'valu':
        assert sc.program_stage() == 0
    return sc


@functools.lru_cache(maxsize=None)
def _data(n_templates):
    """Corpus, files (every 7th CC-flagged) and the oracle's top-16, computed once per corpus size;
    the ranking for a smaller k or a head of the files is a slice of it."""
    from licensee_amd._native import FileBatch
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.synth import SyntheticCorpus
    c = TemplateCorpus(corpus_of(n_templates))
    fb = SyntheticCorpus(c).generate(0, 700 if n_templates <= 64 else 2000, seed=n_templates, nthreads=8)
    cc = fb.cc_false_positive.copy()
    cc[::7] = 1
    fb = FileBatch(fb.bits, fb.wordset_size, fb.length, cc)
    return c, fb, expected_topk(c, fb, 16)


def _exp(exp16, n, k):
    return exp16[0][:n, :k], exp16[1][:n, :k]


def _check_all(sc, fb, exp16, sizes, where):
    for n in sizes:
        part = _head(fb, n)
        for k in KS:
            got = sc.topk(part, k)
            assert got[0].shape == got[1].shape == (n, k)
            assert_topk(got, _exp(exp16, n, k), (where, n, k))
    # the matrix call's own top-k, on the whole batch
    for k in (3, 16):
        assert_topk(sc.topk(fb, k), sc.matrix(fb, k)[2:], (where, 'matrix', k))
    empty = sc.topk(_head(fb, 0), 3)
    assert empty[0].shape == empty[1].shape == (0, 3)


@pytest.mark.parametrize('n_templates,variant', SMALL_CASES)
def test_small_corpora(n_templates, variant, monkeypatch):
    c, fb, exp16 = _data(n_templates)
    if n_templates == 2:   # the two cc-by texts: a flagged file ranks nothing
        assert (exp16[0][::7] == -1).all() and (exp16[1][::7] == -1.0).all()
    if n_templates < 16:   # k > T: padding
        assert (exp16[0][:, n_templates:] == -1).all()
    sc = _scorer(c, monkeypatch, variant)
    try:
        _check_all(sc, fb, exp16, SMALL_N, (n_templates, variant))
    finally:
        sc.close()


@pytest.mark.parametrize('n_templates,variant', LARGE_CASES)
def test_large_corpora(n_templates, variant, monkeypatch):
    c, fb, exp16 = _data(n_templates)
    sc = _scorer(c, monkeypatch, variant)
    try:
        _check_all(sc, fb, exp16, (fb.n,), (n_templates, variant))
    finally:
        sc.close()


# ---- ties -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tie_data(large):
    """Corpora in which templates repeat under later indices, so every file's top k holds exact
    ties. Small: six vendored texts and their clones (12 templates). Large: 100 synthetic templates,
    then the first 40 again (140 templates)."""
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from licensee_amd.synth import SyntheticCorpus
    from licensee_amd.synth_templates import synthetic_templates
    if not large:
        from tests.test_topk_abi import _tie_corpus
        c = _tie_corpus()
        base = [License.find(k) for k in ('apache-2.0', 'bsd-2-clause', 'cc-by-4.0', 'isc', 'mit', 'unlicense')]
        fb = c.intern_files(make_files(base, 699, 5, cc_rate=0.2) + [NormFile('')])
    else:
        c100 = TemplateCorpus(synthetic_templates(License.all(hidden=True, pseudo=False), 100, seed=100))
        b = ArrayCorpus.of(c100)
        sel = np.r_[np.arange(100), np.arange(40)]
        c = ArrayCorpus(b.lf_bits[sel], b.lf_size[sel], b.fields_set_size[sel], b.length_slack[sel], b.length[sel],
                        b.is_cc[sel], b.n_vocab)
        fb = SyntheticCorpus(c100).generate(0, 2000, seed=5, nthreads=8)
    exp16 = expected_topk(c, fb, 16)
    tied = (exp16[0][:, 1] >= 0) & (exp16[1][:, 0] == exp16[1][:, 1])
    assert tie_rate(exp16) > (0.3 if large else 0.7)
    assert (exp16[0][tied, 0] > exp16[0][tied, 1]).all()      # the later template first
    return c, fb, exp16


@pytest.mark.parametrize('variant', ['valu', 'mfma', 'dense', 'post', 'lds', 'dense-large'])
def test_exact_ties_put_the_later_template_first(variant, monkeypatch):
    large = variant in ('post', 'lds', 'dense-large')
    c, fb, exp16 = _tie_data(large)
    sc = _scorer(c, monkeypatch, 'dense' if variant == 'dense-large' else variant)
    try:
        for k in KS:
            assert_topk(sc.topk(fb, k), _exp(exp16, fb.n, k), (variant, k))
    finally:
        sc.close()


# ---- IEEE-double branch -------------------------------------------------------------------------

@pytest.mark.parametrize('n_templates,variant', [(47, 'valu'), (47, 'mfma'), (47, 'dense'), (130, 'post'), (130, 'lds')])
def test_slow_lanes_mixed_into_fast_waves(n_templates, variant, monkeypatch):
    c, fb, _ = _data(n_templates)
    wide, idx = widen_lanes(fb, seed=11)
    assert idx.size > 50
    exp16 = expected_topk(c, wide, 16)
    sc = _scorer(c, monkeypatch, variant)
    try:
        for k in (3, 5):
            assert_topk(sc.topk(wide, k), _exp(exp16, wide.n, k), (variant, k))
    finally:
        sc.close()


@pytest.mark.parametrize('n_templates,variant', [(47, 'valu'), (47, 'mfma'), (130, 'post')])
def test_corpus_outside_the_fast_envelope(n_templates, variant, monkeypatch):
    c, fb, _ = _data(n_templates)
    slow = outside_fast_envelope(c)
    exp16 = expected_topk(slow, fb, 16)
    assert (exp16[1] > 100.0).any()
    sc = _scorer(slow, monkeypatch, variant)
    try:
        for k in (4, 16):
            assert_topk(sc.topk(fb, k), _exp(exp16, fb.n, k), (variant, k))
    finally:
        sc.close()


# ---- state and memory ---------------------------------------------------------------------------

def _code(exc):
    return exc.value.code


@pytest.mark.parametrize('n_templates,variant', [(47, 'valu'), (130, 'post'), (130, 'lds')])
def test_state_and_memory(n_templates, variant, monkeypatch):
    from licensee_amd._native import DiceError
    c, fb, exp16 = _data(n_templates)
    fb = _head(fb, 300)
    sc = _scorer(c, monkeypatch, variant)
    b = sc.batch(512)      # capacity above n: the matrix buffers are sized by it
    try:
        b.upload(fb)
        with pytest.raises(DiceError) as e:      # no ranking since creation
            b.download_topk(3)
        assert _code(e) == DICE_E_STATE
        for bad in (0, -1, 17):
            with pytest.raises(DiceError) as e:
                b.topk(bad)
            assert _code(e) == DICE_E_ARG
            with pytest.raises(DiceError) as e:
                b.download_topk(bad)
            assert _code(e) == DICE_E_ARG
        b.match(98.0)
        match = b.download_match()
        assert b.matrix_bytes() == 0
        b.topk(3)
        first = b.download_topk(3)
        assert_topk(first, _exp(exp16, fb.n, 3))
        assert b.matrix_bytes() == 0             # nothing N x T was allocated
        for got, ref in zip(b.download_match(), match):   # the match results are untouched
            assert np.array_equal(got, ref)
        b.topk(3)
        assert_topk(b.download_topk(3), first)   # twice: the same
        with pytest.raises(DiceError) as e:
            b.download_topk(4)
        assert _code(e) == DICE_E_ARG
        with pytest.raises(DiceError) as e:      # overlap / score after topk: no matrix on the device
            b.download_matrix(3)
        assert _code(e) == DICE_E_STATE
        # ... its top-k outputs still work
        from licensee_amd._native import _check, _ptr, load_library
        tki = np.empty((fb.n, 3), np.int32)
        tks = np.empty((fb.n, 3), np.float64)
        _check(load_library().dice_batch_download_matrix(b._b, None, None, 3, _ptr(tki), _ptr(tks), None))
        assert_topk((tki, tks), first)
        ov = np.empty((fb.n, n_templates), np.uint32)
        assert load_library().dice_batch_download_matrix(b._b, _ptr(ov), None, 3, None, None, None) == DICE_E_STATE
        # the matrix call allocates capacity x ld x (4 + 8) bytes and serves download_topk too
        b.matrix(5)
        ld = n_templates if variant != 'post' else (n_templates + 31) // 32 * 32
        assert b.matrix_bytes() == 512 * ld * 12
        mov, msc, mki, mks = b.download_matrix(5)
        assert_topk((mki, mks), _exp(exp16, fb.n, 5))
        assert_topk(b.download_topk(5), (mki, mks))
        assert np.array_equal(np.take_along_axis(msc, np.maximum(mki, 0), 1)[mki >= 0], mks[mki >= 0])
        # topk again, with a larger k than the buffers held: the matrix stays allocated but stale
        b.topk(16)
        assert_topk(b.download_topk(16), _exp(exp16, fb.n, 16))
        assert b.matrix_bytes() == 512 * ld * 12
        with pytest.raises(DiceError) as e:
            b.download_matrix(16)
        assert _code(e) == DICE_E_STATE
        for got, ref in zip(b.download_match(), match):
            assert np.array_equal(got, ref)
    finally:
        b.close()
        sc.close()


# ---- sharded ------------------------------------------------------------------------------------

@pytest.mark.parametrize('gather', [0, 1])
def test_topk_sharded_equals_single(gather, monkeypatch):
    from licensee_amd._native import Scorer, topk_sharded
    c, fb, exp16 = _data(47)
    monkeypatch.delenv('DICE_FORCE_DENSE', raising=False)
    scs = [Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab, device=0)
           for _ in range(3)]
    try:
        for k in (3, 16):
            ref = scs[0].topk(fb, k)
            assert_topk(ref, _exp(exp16, fb.n, k))
            for n_ctx in (1, 2, 3):
                assert_topk(topk_sharded(scs[:n_ctx], fb, k, gather), ref, (n_ctx, gather, k))
        tiny = _head(fb, 2)                      # more shards than files: empty shards
        assert_topk(topk_sharded(scs, tiny, 3, gather), _exp(exp16, 2, 3))
    finally:
        for s in scs:
            s.close()


# ---- DiceEngine.closest_files -------------------------------------------------------------------

def test_closest_files_on_the_fixture_files():
    """detect.rb:93-98 ranks every template, CC filter off: the fixture files of
    tests/golden/dice_spec.json and perturbed templates against the oracle's ranking."""
    from licensee_amd.dice import default_engine
    from oracle import dice_oracle as O
    from tests.helpers import oracle_templates
    from tests.test_gpu_golden import GoldenLicenseFile, golden
    eng = default_engine()
    templates = eng.templates
    otpl = oracle_templates(templates)
    cases = golden('dice_spec.json')['cases']
    files = [GoldenLicenseFile(v['file']) for v in cases.values() if isinstance(v, dict) and 'file' in v]
    assert len(files) >= 3
    files += make_files(templates, 80, 34, cc_rate=0.3)
    for k in (1, 3, 5):
        got = eng.closest_files(files, k)
        assert len(got) == len(files)
        for i, f in enumerate(files):
            of = f.oracle if hasattr(f, 'oracle') else O.OracleFile(f.content_normalized())
            ranked = O.matches_by_similarity(otpl, of, cc_fp=False)[:k]
            assert [(l.key, s) for l, s in got[i]] == [(templates[t].key, s) for t, s in ranked], (k, i)
    assert eng.closest_files(files, 0) == [[] for _ in files]
