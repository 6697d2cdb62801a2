"""The match kernels' running best with the template index in the denominator's top byte
(csrc/dice_program_gen.cpp, MATCH_FILE), the fold that writes the accumulators, the count entries as
one v_dot4_u32_u8 each and the tile loop's scalar addresses: best, overlap and score of match and
match(confidence=True) with DICE_PROG_MATCH=mfma must equal the C oracle and the DICE_PROG_MATCH=valu
leg bit for bit.

Corpora: the 47 vendored templates; 33 and 64 templates (index 63 lies next to the 0xFF of "none
yet"); a corpus with byte-identical clones under later keys (a later template takes a tie); one built
so that a count dword holds four fields of 255 words (every byte 255 in the all-words file).

Files, in every batch: every vocabulary word (each bit-region word, each count byte at its
capacity), the empty file, CC-flagged files in every tile, a file outside the fast envelope in the
second tile and one in the last, so that those waves take the IEEE-double body, which keeps the index
beside a whole 32-bit denominator -- one of them with a denominator above 2^24, where an index byte
inside it would be overwritten. Sizes 1, 64, 65 and 64 * 13 + 5 leave padding lanes beyond n.

The launch gives every compute unit one workgroup and a wave its second tile only from 12 tiles per
compute unit on, so at those four sizes every tile is a wave's first. The fifth size,
64 (12 C + 1) + 5 with C compute units, makes the partial last tile the second tile of a wave: its
requests go to the next tile through the scalar base, and behind it to tile 0."""
import numpy as np
import pytest

from tests.helpers import ArrayCorpus
from tests.test_gpu_compact_layout import _same
from tests.test_gpu_corpus_sizes import corpus_of
from tests.test_gpu_prog_mfma import _oracle, _scorer
from tests.test_program_compact_codegen import concat, edge_files, files_from_words, word_classes, word_matrix

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65, 64 * 13 + 5]
N = SIZES[-1]
ORACLE_FILES = 2000


def _count255_corpus():
    """6 templates. Words 0-1019: four membership classes of exactly 255 words, four count fields
    that fill one count dword. Words 1020-1059: one class each (the bit region). Template 4 is a
    CC template, template 5 lives in the bit region alone."""
    T, V = 6, 4 * 255 + 40
    cols = [0b000011] * 255 + [0b000110] * 255 + [0b001100] * 255 + [0b011001] * 255
    cols += [m for m in range(1, 64) if m not in (0b000011, 0b000110, 0b001100, 0b011001)][:40]
    member = ((np.array(cols)[None, :] >> np.arange(T)[:, None]) & 1).astype(np.uint8)   # [T][V]
    pad = np.zeros((T, (V + 63) // 64 * 64), np.uint8)
    pad[:, :V] = member
    bits = np.packbits(pad, axis=1, bitorder='little').view(np.uint64)
    size = member.sum(1).astype(np.uint32)
    return ArrayCorpus(bits, size, np.ones(T, np.uint32), np.full(T, 5, np.int32), (size * 6).astype(np.int32),
                       np.array([0, 0, 0, 0, 1, 0], np.uint8), V)


def _clone_corpus():
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    base = [License.find(k) for k in ('apache-2.0', 'bsd-2-clause', 'isc', 'mit', 'mpl-2.0', 'unlicense')]
    clones = [License('zz-' + l.key, {'title': l.title}, content_normalized=l.content_normalized(),
                      alt_segments=l.spdx_alt_segments()) for l in base]
    return TemplateCorpus(sorted(base + clones, key=lambda l: l.key))


def _corpus(name):
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    if name == 'vendored':
        return TemplateCorpus(License.all(hidden=True, pseudo=False))
    if name == 'clones':
        return _clone_corpus()
    if name == 'count255':
        return _count255_corpus()
    return TemplateCorpus(corpus_of(int(name[1:])))


def _files(c, n, seed):
    """n files: the edge files (the all-words file first), the empty file and every template's own
    word set at its own length (the last index and the clones are matched for certain) at the head,
    then generated ones; CC flags in every tile; slow-envelope files in the second and the last tile."""
    from licensee_amd._native import FileBatch
    own = files_from_words(c, [np.flatnonzero(row).tolist() for row in word_matrix(c.lf_bits, c.n_vocab)])
    own = FileBatch(own.bits, own.wordset_size, np.asarray(c.length, np.int32).copy(), own.cc_false_positive)
    head = concat(concat(edge_files(c, word_classes(c)[1]), files_from_words(c, [[]])), own)
    if isinstance(c, ArrayCorpus):
        rng = np.random.default_rng(seed)
        rest = files_from_words(c, [np.flatnonzero(rng.random(c.n_vocab) < rng.random()).tolist()
                                    for _ in range(n - head.n)])
    else:
        from licensee_amd.synth import SyntheticCorpus
        rest = SyntheticCorpus(c).generate(0, n - head.n, seed=seed, nthreads=8)
    fb = concat(head, rest)
    wf, ln, cc = fb.wordset_size.copy(), fb.length.copy(), fb.cc_false_positive.copy()
    cc[5::7] = 1
    wf[70], ln[70] = (1 << 20) + 5, (1 << 21) + 9          # denominator a little above 2^20
    wf[n - 2], ln[n - 2] = (1 << 26) + 3, (1 << 30) + 1    # denominator above 2^24
    return FileBatch(fb.bits, wf, ln, cc)


def _head(fb, n):
    from licensee_amd._native import FileBatch
    return FileBatch(fb.bits[:n], fb.wordset_size[:n], fb.length[:n], fb.cc_false_positive[:n])


def _both(sc, fb):
    b = sc.batch(fb.n)
    try:
        b.upload(fb)
        b.match(98.0)
        m = b.download_match()
        b.match(98.0, confidence=True)
        return m, b.download_match()
    finally:
        b.close()


def _check(c, fb, mf, va, orc, where):
    from licensee_amd._native import FileBatch
    got, ref = _both(mf, fb), _both(va, fb)
    _same(got[0], ref[0], (where, 'valu', 'match'))
    _same(got[1], ref[1], (where, 'valu', 'confidence'))
    n = fb.n
    pick = np.unique(np.concatenate([np.arange(min(n, ORACLE_FILES)), np.arange(max(0, n - ORACLE_FILES), n)]))
    sub = FileBatch(fb.bits[pick], fb.wordset_size[pick], fb.length[pick], fb.cc_false_positive[pick])
    m = orc.match(sub.bits, sub.wordset_size, sub.length, sub.cc_false_positive, 98.0, nthreads=8)
    conf = (m[0], np.where(m[0] >= 0, m[1], 0).astype(np.uint32), np.where(m[0] >= 0, m[2], 0.0))
    _same([x[pick] for x in got[0]], m, (where, 'oracle', 'match'))
    _same([x[pick] for x in got[1]], conf, (where, 'oracle', 'confidence'))
    return got


@pytest.fixture(scope='module', params=['vendored', 'T33', 'T64', 'clones', 'count255'])
def setup(request):
    """A corpus, its two scorers, the oracle and the batch of 64 * 13 + 5 files (the smaller sizes
    are heads of it)."""
    c = _corpus(request.param)
    mp = pytest.MonkeyPatch()
    try:
        mf, va = _scorer(c, mp, 'mfma'), _scorer(c, mp, 'valu')
    finally:
        mp.undo()
    assert mf.program_stage() == 2 and va.program_stage() == 0
    yield request.param, c, _files(c, N, 17), mf, va, _oracle(c)
    mf.close()
    va.close()


@pytest.mark.parametrize('n', SIZES)
def test_sizes(setup, n):
    from licensee_amd._native import FileBatch
    name, c, fb, mf, va, orc = setup
    part = _head(fb, n)
    if 1 < n < N:                                          # a slow-envelope file in this size's last tile too
        wf, ln = part.wordset_size.copy(), part.length.copy()
        wf[n - 2], ln[n - 2] = (1 << 26) + 3, (1 << 30) + 1
        part = FileBatch(part.bits, wf, ln, part.cc_false_positive)
    got = _check(c, part, mf, va, orc, (name, n))
    if name == 'clones' and n == N:
        matched = got[0][0][got[0][0] >= 0]                # sorted keys: the six originals, then their zz- clones
        assert len(matched) >= 6 and (matched >= 6).all()


def test_count_dword_of_four_full_bytes():
    """The layout the count255 corpus was built for: four count fields, all in one dword."""
    from tests.test_program_compact_codegen import compact_layout
    c = _count255_corpus()
    dest = compact_layout(c)[0]
    fields = -2 - dest[dest <= -2]
    assert sorted(set(fields.tolist())) == [0, 1, 2, 3]
    assert all((fields == f).sum() == 255 for f in range(4))


@pytest.mark.parametrize('name', ['vendored', 'T64'])
def test_second_tile_of_a_wave(name):
    """64 (12 C + 1) + 5 files: the last workgroup's share is 13 tiles, and the partial last tile,
    which holds a slow-envelope file and a CC-flagged one, is its wave 0's second."""
    import torch
    C = torch.cuda.get_device_properties(0).multi_processor_count
    c = _corpus(name)
    fb = _files(c, 64 * (12 * C + 1) + 5, 23)
    mp = pytest.MonkeyPatch()
    try:
        mf, va = _scorer(c, mp, 'mfma'), _scorer(c, mp, 'valu')
    finally:
        mp.undo()
    try:
        assert mf.program_stage() == 2 and va.program_stage() == 0
        _check(c, fb, mf, va, _oracle(c), (name, 'second tile'))
    finally:
        mf.close()
        va.close()
