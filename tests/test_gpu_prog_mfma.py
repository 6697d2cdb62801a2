"""The sparse program's matrix-core accumulate stage (DICE_PROG_MATCH, csrc/dice_program.cpp) on
the device (match mode; matrix mode keeps the VALU kernels of the same module): match,
match(confidence=True) and matrix(k=3) must equal the C oracle's hash mode and
the same scorer built with DICE_PROG_MATCH=valu, exactly, over partial tiles and partial 32-file
sub-tiles, template-tile padding, bit regions that do not fill their last K-steps, corpora without
count fields or without a bit region, every upload path, and a wave on the IEEE-double path."""
import numpy as np
import pytest

from tests.helpers import ArrayCorpus, NormFile, make_files
from tests.test_gpu_compact_layout import _expect, _same, _topk
from tests.test_gpu_corpus_sizes import corpus_of
from tests.test_program_compact_codegen import concat, edge_files, files_from_words, word_classes

pytestmark = pytest.mark.gpu

N = 3 * 64 + 5
SIZES = [1, 15, 16, 17, 63, 64, 65, N]


def _scorer(c, monkeypatch, stage):
    from licensee_amd._native import Scorer
    if stage is None:
        monkeypatch.delenv('DICE_PROG_MATCH', raising=False)
    else:
        monkeypatch.setenv('DICE_PROG_MATCH', stage)
    return Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab, device=0)


def _oracle(c):
    from oracle.native import OracleScorer
    return OracleScorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab)


def _tables_dims(c):
    import ctypes
    from licensee_amd import _native
    from tests.test_program_codegen import _templates_struct
    keep, t = _templates_struct(c)
    dims = (ctypes.c_int32 * 4)()
    n = _native.load_library().dice_program_mfma_tables(ctypes.byref(t), ctypes.addressof(dims), None, 0, None, 0)
    return n, list(dims)


def _head(fb, n):
    from licensee_amd._native import FileBatch
    return FileBatch(fb.bits[:n], fb.wordset_size[:n], fb.length[:n], fb.cc_false_positive[:n])


def _results(sc, fb):
    """(match, confidence, (mov, msc), (tki, tks)) of one resident batch."""
    b = sc.batch(fb.n)
    try:
        b.upload(fb)
        b.match(98.0)
        m = b.download_match()
        b.match(98.0, confidence=True)
        conf = b.download_match()
        b.matrix(3)
        gov, gsc, tki, tks = b.download_matrix()
        return m, conf, (gov, gsc), (tki, tks)
    finally:
        b.close()


def _check(c, fb, orc, got, ref, where):
    m, conf, mat = _expect(orc, fb)
    _same(got[0], m, (where, 'match'))
    _same(got[1], conf, (where, 'confidence'))
    _same(got[2], mat, (where, 'matrix'))
    k = got[3][0].shape[1]
    for i, ranked in enumerate(_topk(c, fb, mat[1], k)):
        assert got[3][0][i].tolist() == ranked + [-1] * (k - len(ranked)), (where, i)
        assert got[3][1][i, :len(ranked)].tolist() == [mat[1][i, t] for t in ranked], (where, i)
    for g, r, name in zip(got, ref, ('match', 'confidence', 'matrix', 'topk')):
        _same(g, r, (where, 'valu', name))


@pytest.fixture(scope='module')
def vendored():
    """The 47 vendored templates and N files whose head holds the edge files, the empty file, a
    CC-flagged file and one file outside the fast envelope (so every size above 2 has a wave on the
    IEEE-double path), then generated files."""
    from licensee_amd._native import FileBatch
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    templates = License.all(hidden=True, pseudo=False)
    c = TemplateCorpus(templates)
    edges = edge_files(c, word_classes(c)[1])
    cc_text = License.find('cc-by-4.0').content_normalized()
    special = c.intern_files([NormFile(''), NormFile(cc_text, cc=True), NormFile(License.find('mit').content_normalized())])
    fb = concat(concat(special, edges), c.intern_files(make_files(templates, N - edges.n - 3, 21)))
    assert fb.n == N
    wf, ln = fb.wordset_size.copy(), fb.length.copy()
    wf[2] = (1 << 20) + 77          # the MIT text with a huge out-of-vocabulary wordset: slow lane
    wf[70], ln[70] = (1 << 20) + 5, (1 << 21) + 9
    fb = FileBatch(fb.bits, wf, ln, fb.cc_false_positive)
    return c, fb, _oracle(c)


@pytest.fixture(scope='module')
def vendored_scorers(vendored):
    mp = pytest.MonkeyPatch()
    c = vendored[0]
    try:
        mf, va = _scorer(c, mp, 'mfma'), _scorer(c, mp, 'valu')
    finally:
        mp.undo()
    yield mf, va
    mf.close()
    va.close()


def test_vendored_stage_selection(vendored, vendored_scorers, monkeypatch):
    c = vendored[0]
    mf, va = vendored_scorers
    n, dims = _tables_dims(c)
    assert n == dims[0] * dims[1] * 256 > 0 and dims[1] == 2
    assert dims[2] % 8 != 0                   # the bit region ends inside a K-step pair group
    assert mf.match_kernel() == va.match_kernel() == 1
    assert mf.program_stage() == 2 and va.program_stage() == 0
    sc = _scorer(c, monkeypatch, None)
    try:
        assert sc.program_stage() == dims[3]  # the cost rule
    finally:
        sc.close()


@pytest.mark.parametrize('n', SIZES)
def test_vendored_sizes(vendored, vendored_scorers, n):
    c, fb, orc = vendored
    mf, va = vendored_scorers
    part = _head(fb, n)
    _check(c, part, orc, _results(mf, part), _results(va, part), n)


def test_upload_paths(vendored, vendored_scorers):
    from licensee_amd import _native
    c, fb, orc = vendored
    mf, _ = vendored_scorers
    m = _expect(orc, fb)[0]
    b = mf.batch(fb.n)
    try:
        offs, ids = _native.bits_to_ids(fb.bits, c.n_vocab)
        b.upload_ids(offs, ids, fb.wordset_size, fb.length, fb.cc_false_positive)
        b.match(98.0)
        _same(b.download_match(), m, 'upload_ids')
        idx = np.array([3, N - 2])                  # one row of the partial last tile
        src = np.array([N - 1, 7])
        b.set_rows(idx, fb.bits[src], fb.wordset_size[src])
        bits, wf = fb.bits.copy(), fb.wordset_size.copy()
        bits[idx], wf[idx] = fb.bits[src], fb.wordset_size[src]
        fb2 = _native.FileBatch(bits, wf, fb.length, fb.cc_false_positive)
        b.match(98.0)
        _same(b.download_match(), _expect(orc, fb2)[0], 'set_rows')
    finally:
        b.close()
    for i in (3, 40):                               # dice_match with n = 1: the all-words file, a generated one
        one = _native.FileBatch(fb.bits[i:i + 1], fb.wordset_size[i:i + 1], fb.length[i:i + 1],
                                fb.cc_false_positive[i:i + 1])
        _same(mf.match(one, 98.0), [x[i:i + 1] for x in m], ('dice_match', i))


def _distinct_column_corpus():
    """8 templates over 255 words, every word in its own membership class: no count fields."""
    T, V = 8, 255
    member = ((np.arange(1, V + 1)[None, :] >> np.arange(T)[:, None]) & 1).astype(np.uint8)   # [T][V]
    pad = np.zeros((T, 256), np.uint8)
    pad[:, :V] = member
    bits = np.packbits(pad, axis=1, bitorder='little').view(np.uint64)
    size = member.sum(1).astype(np.uint32)
    return ArrayCorpus(bits, size, np.ones(T, np.uint32), np.full(T, 5, np.int32), (size * 6).astype(np.int32),
                       np.array([0, 0, 1, 0, 0, 0, 0, 1], np.uint8), V)


def _array_files(c, seed, n):
    rng = np.random.default_rng(seed)
    lists = [list(range(c.n_vocab)), []]
    while len(lists) < n:
        lists.append(np.flatnonzero(rng.random(c.n_vocab) < rng.random()).tolist())
    fb = files_from_words(c, lists)
    cc = np.zeros(n, np.uint8)
    cc[5::7] = 1
    from licensee_amd._native import FileBatch
    return FileBatch(fb.bits, fb.wordset_size, fb.length, cc)


@pytest.mark.parametrize('name', ['T1', 'T16', 'T17', 'T33', 'T64', 'nocount'])
def test_other_corpora(name, monkeypatch):
    """Template-tile padding (1, 16, 17 and 33 templates in 32-template tiles, 64 filling two), a
    corpus of one template (every word in one count class: no bit region, the VALU program runs)
    and one without count fields."""
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.synth import SyntheticCorpus
    if name == 'nocount':
        c = _distinct_column_corpus()
        fb = _array_files(c, 5, N)
    else:
        c = TemplateCorpus(corpus_of(int(name[1:])))
        fb = SyntheticCorpus(c).generate(0, N, seed=11, nthreads=8)
    n, dims = _tables_dims(c)
    mf = _scorer(c, monkeypatch, 'mfma')
    try:
        if name == 'T1':
            assert n == 0 and dims[2] == 0 and mf.program_stage() == 0
        else:                                   # every other corpus runs the matrix-core kernel
            assert n > 0 and mf.program_stage() == 2, dims
        if name == 'nocount':
            assert dims[2] == 8
        got = _results(mf, fb)
    finally:
        mf.close()
    va = _scorer(c, monkeypatch, 'valu')
    try:
        ref = _results(va, fb)
    finally:
        va.close()
    _check(c, fb, _oracle(c), got, ref, name)


def test_default_rule_on_a_batch_of_one_tile_per_cu(vendored, monkeypatch):
    """The default (cost rule) takes the matrix-core kernels from one tile per CU on; the batch ends
    in a partial tile and the workgroups' tile shares differ by one. Every file against the VALU
    leg, every 61st (and the last tile) against the oracle."""
    import torch
    from licensee_amd._native import FileBatch
    from licensee_amd.synth import SyntheticCorpus
    c, _, orc = vendored
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (cus + 37) * 64 + 5
    fb = SyntheticCorpus(c).generate(0, n, seed=3, nthreads=8)
    got = {}
    for stage in (None, 'valu'):
        sc = _scorer(c, monkeypatch, stage)
        try:
            got[stage] = sc.match(fb, 98.0), sc.program_stage()
        finally:
            sc.close()
    assert got[None][1] == _tables_dims(c)[1][3] and got['valu'][1] == 0
    _same(got[None][0], got['valu'][0], 'valu')
    pick = np.unique(np.concatenate([np.arange(0, n, 61), np.arange(n - 69, n)]))
    sub = FileBatch(fb.bits[pick], fb.wordset_size[pick], fb.length[pick], fb.cc_false_positive[pick])
    exp = orc.match(sub.bits, sub.wordset_size, sub.length, sub.cc_false_positive, 98.0, nthreads=8)
    _same([x[pick] for x in got[None][0]], exp, 'oracle')
