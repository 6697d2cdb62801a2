"""The sparse program over the compact (class-count) tile on the device: every upload path
lands on the compact tile (dice_pack_compact) and scores exactly as the oracle and as the
full-bitset tile (DICE_PROG_LAYOUT=bits)."""
import numpy as np
import pytest

from tests.helpers import NormFile, make_files
from tests.test_program_compact_codegen import compact_layout, concat, edge_files, word_classes

pytestmark = pytest.mark.gpu

N = 3 * 64 + 5


def _scorer(c):
    from licensee_amd._native import Scorer
    return Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab, device=0)


@pytest.fixture(scope='module')
def case():
    """Corpus, the N files (generated ones, the empty file, the edge files) and the oracle's
    results: match at 98, Dice#confidence outputs, matrix."""
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from oracle.native import OracleScorer
    templates = License.all(hidden=True, pseudo=False)
    c = TemplateCorpus(templates)
    edges = edge_files(c, word_classes(c)[1])
    fb = concat(c.intern_files(make_files(templates, N - edges.n - 1, 21) + [NormFile('')]), edges)
    assert fb.n == N
    orc = OracleScorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab)
    return c, fb, orc


def _expect(orc, fb):
    m = orc.match(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive, 98.0, mode=0)
    conf = (m[0], np.where(m[0] >= 0, m[1], 0).astype(np.uint32), np.where(m[0] >= 0, m[2], 0.0))
    mov, msc = orc.matrix(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive)
    return m, conf, (mov, msc)


def _same(got, exp, where):
    for i, (g, e) in enumerate(zip(got, exp)):
        assert np.array_equal(g, e), (where, i, np.nonzero(np.asarray(g) != np.asarray(e))[0][:10])


def _topk(c, fb, msc, k):
    T = msc.shape[1]
    out = []
    for i in range(fb.n):
        cand = [t for t in range(T) if not (c.is_cc[t] and fb.cc_false_positive[i])]
        out.append(sorted(cand, key=lambda t: (msc[i, t], t), reverse=True)[:k])
    return out


def _run_batch(sc, c, fb, exp, where):
    """upload -> match, match(confidence) and matrix(k=3) against the oracle; the tile bytes."""
    m, conf, (mov, msc) = exp
    b = sc.batch(fb.n)
    try:
        b.upload(fb)
        b.match(98.0)
        _same(b.download_match(), m, (where, 'match'))
        b.match(98.0, confidence=True)
        _same(b.download_match(), conf, (where, 'confidence'))
        b.matrix(3)
        gov, gsc, tki, tks = b.download_matrix()
        _same((gov, gsc), (mov, msc), (where, 'matrix'))
        for i, ranked in enumerate(_topk(c, fb, msc, 3)):
            assert tki[i].tolist() == ranked + [-1] * (3 - len(ranked)), (where, i)
            assert tks[i, :len(ranked)].tolist() == [msc[i, t] for t in ranked], (where, i)
        return b.bytes_per_file()
    finally:
        b.close()


def test_compact_equals_oracle_and_bits_layout(case, monkeypatch):
    c, fb, orc = case
    exp = _expect(orc, fb)
    quads = compact_layout(c)[3]
    sc = _scorer(c)
    try:
        assert sc.match_kernel() == 1
        compact_bytes = _run_batch(sc, c, fb, exp, 'compact')
    finally:
        sc.close()
    monkeypatch.setenv('DICE_PROG_LAYOUT', 'bits')
    sc = _scorer(c)
    try:
        assert sc.match_kernel() == 1
        bits_bytes = _run_batch(sc, c, fb, exp, 'bits')
    finally:
        sc.close()
    assert compact_bytes == 16 * quads < bits_bytes == 16 * ((c.w64 + 1) // 2)


def test_other_upload_paths_land_on_the_compact_tile(case):
    from licensee_amd import _native
    c, fb, orc = case
    m = _expect(orc, fb)[0]
    sc = _scorer(c)
    try:
        b = sc.batch(fb.n)
        try:
            offs, ids = _native.bits_to_ids(fb.bits, c.n_vocab)
            b.upload_ids(offs, ids, fb.wordset_size, fb.length, fb.cc_false_positive)
            b.match(98.0)
            _same(b.download_match(), m, 'upload_ids')
            # two rows replaced (one in the partial last tile): rows and |W_F| change, lengths stay
            idx = np.array([3, N - 2])
            src = np.array([N - 1, 7])
            b.set_rows(idx, fb.bits[src], fb.wordset_size[src])
            bits, wf = fb.bits.copy(), fb.wordset_size.copy()
            bits[idx], wf[idx] = fb.bits[src], fb.wordset_size[src]
            fb2 = _native.FileBatch(bits, wf, fb.length, fb.cc_false_positive)
            b.match(98.0)
            _same(b.download_match(), _expect(orc, fb2)[0], 'set_rows')
        finally:
            b.close()
        # n = 1 through dice_match (the small-call path): the all-words edge file, a generated one
        for i in (N - 11, 5):
            one = _native.FileBatch(fb.bits[i:i + 1], fb.wordset_size[i:i + 1], fb.length[i:i + 1],
                                    fb.cc_false_positive[i:i + 1])
            _same(sc.match(one, 98.0), [x[i:i + 1] for x in m], ('dice_match', i))
    finally:
        sc.close()
