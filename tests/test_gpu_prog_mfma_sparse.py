"""The matrix-core match kernel with its templates in assigned rows and only the live (K-step, block)
fragments multiplied (csrc/dice_program_gen.cpp: assign_rows, group_bits, emit_mfma_prologue), on the
device. DICE_PROG_MATCH=mfma forces the stage; results must equal the C oracle and the same scorer
built with DICE_PROG_MATCH=valu, exactly: over partial tiles and partial 32-file halves, a batch just
above one tile per CU, a block of one template (every fold form with a padded row), two full blocks,
a corpus where some K-steps are live in block 1 only, and one where no fragment is dead."""
import numpy as np
import pytest

from tests.helpers import ArrayCorpus
from tests.test_gpu_compact_layout import _same
from tests.test_gpu_corpus_sizes import corpus_of
from tests.test_gpu_prog_mfma import N, _array_files, _check, _head, _oracle, _results, _scorer, _tables_dims
from tests.test_gpu_prog_mfma import vendored, vendored_scorers  # noqa: F401  (module-scoped fixtures)
from tests.test_program_mfma_sparse import mfma_rows

pytestmark = pytest.mark.gpu

BIG = 16384 + 37        # just above one tile per CU (256 CUs), a partial tile with a partial 32-file half


def _live(c):
    n, dims = _tables_dims(c)
    assert n > 0
    rows, live, n_live = mfma_rows(c, dims)
    return rows, live, n_live, dims


def test_vendored_stage_is_sparse(vendored):   # noqa: F811
    rows, live, n_live, dims = _live(vendored[0])
    print('vendored corpus: live fragments', n_live, 'of', live.size)
    assert dims[1] == 2 and 0 < n_live < live.size
    assert (rows[:32] >= 0).all() and (rows[32:] >= 0).sum() == 15


@pytest.mark.parametrize('n', [1, 33, 64, 65])
def test_vendored_sizes(vendored, vendored_scorers, n):   # noqa: F811
    c, fb, orc = vendored
    mf, va = vendored_scorers
    part = _head(fb, n)
    _check(c, part, orc, _results(mf, part), _results(va, part), n)


def test_vendored_one_tile_per_cu(vendored, vendored_scorers):   # noqa: F811
    """16,384 + 37 files: the head of the fixture (empty file, all-words file, edge files, slow-path
    files), then generated ones. Match results against the VALU leg and the oracle, every file."""
    from licensee_amd.synth import SyntheticCorpus
    from tests.test_program_compact_codegen import concat
    c, fb, orc = vendored
    mf, va = vendored_scorers
    big = concat(fb, SyntheticCorpus(c).generate(0, BIG - fb.n, seed=5, nthreads=8))
    assert big.n == BIG
    got = mf.match(big, 98.0)
    _same(got, va.match(big, 98.0), 'valu')
    _same(got, orc.match(big.bits, big.wordset_size, big.length, big.cc_false_positive, 98.0, nthreads=8), 'oracle')


@pytest.mark.parametrize('n_templates', [33, 64])
def test_synthetic_corpora(n_templates, monkeypatch):
    """33 templates: one block holds a single template, so its fold pairs have a pad on one side or on
    both; 64: no pads at all."""
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.synth import SyntheticCorpus
    from tests.test_program_compact_codegen import concat, edge_files, word_classes
    c = TemplateCorpus(corpus_of(n_templates))
    fb = concat(concat(c.intern_files([_norm('')]), edge_files(c, word_classes(c)[1])),
                SyntheticCorpus(c).generate(0, N, seed=11, nthreads=8))
    rows = _live(c)[0]
    assert sorted([(rows[:32] >= 0).sum(), (rows[32:] >= 0).sum()]) == ([1, 32] if n_templates == 33 else [32, 32])
    _both_legs(c, fb, monkeypatch, n_templates)


def _norm(text):
    from tests.helpers import NormFile
    return NormFile(text)


def _member_corpus(member, is_cc=None):
    """ArrayCorpus of a [T][V] 0/1 membership matrix."""
    T, V = member.shape
    pad = np.zeros((T, (V + 63) // 64 * 64), np.uint8)
    pad[:, :V] = member
    size = member.sum(1).astype(np.uint32)
    return ArrayCorpus(np.packbits(pad, axis=1, bitorder='little').view(np.uint64), size, np.ones(T, np.uint32),
                       np.full(T, 5, np.int32), (size * 6).astype(np.int32),
                       np.zeros(T, np.uint8) if is_cc is None else is_cc, V)


def _both_legs(c, fb, monkeypatch, where):
    mf = _scorer(c, monkeypatch, 'mfma')
    try:
        assert mf.program_stage() == 2
        got = _results(mf, fb)
    finally:
        mf.close()
    va = _scorer(c, monkeypatch, 'valu')
    try:
        ref = _results(va, fb)
    finally:
        va.close()
    _check(c, fb, _oracle(c), got, ref, where)


def test_ksteps_live_in_block_1_only(monkeypatch):
    """36 templates: 300 words in random sets of templates 0-31, 120 words exclusive to templates
    32-35 (15 sets of 8 words: small classes, kept as bits), 30 words shared by the two groups. The
    120 exclusive words fill more than one K-step that no other template touches."""
    rng = np.random.default_rng(7)
    T, V = 36, 450
    member = np.zeros((T, V), np.uint8)
    member[:32, :300] = rng.random((32, 300)) < 0.3
    member[rng.integers(0, 32, 300), np.arange(300)] = 1
    for w in range(120):
        member[32:, 300 + w] = [(w // 8 + 1) >> k & 1 for k in range(4)]
    member[:, 420:] = rng.random((T, 30)) < 0.5
    member[0, 420:] = member[33, 420:] = 1
    cc = np.zeros(T, np.uint8)
    cc[[2, 34]] = 1
    c = _member_corpus(member, cc)
    rows, live, n_live, dims = _live(c)
    only = [(live[:, 1 - j] == 0) & (live[:, j] == 1) for j in range(2)]
    print('live by block', live.sum(0), 'K-steps live in one block only', only[0].sum(), only[1].sum())
    assert only[1].any() and only[0].any()
    _both_legs(c, _array_files(c, 3, N), monkeypatch, 'block-1-only')


def test_dense_membership_nothing_dead(monkeypatch):
    """40 templates, every word in about half of them: each word touches both blocks however the rows
    are assigned, so every fragment is live."""
    rng = np.random.default_rng(9)
    T, V = 40, 255
    member = (rng.random((T, V)) < 0.5).astype(np.uint8)
    c = _member_corpus(member)
    rows, live, n_live, dims = _live(c)
    assert n_live == live.size == dims[0] * 2
    _both_legs(c, _array_files(c, 4, N), monkeypatch, 'dense')
