"""The envelope-edge cases of tests/envelope_cases.py on the device, through the C-ABI. Every
comparison is np.array_equal against the plain Python reference: bit-exact, no tolerance.

T <= 64 (sparse program), each corpus under DICE_PROG_MATCH=valu, DICE_PROG_MATCH=mfma and
DICE_PROG_LAYOUT=bits: match at thresholds 0 and 98, match(confidence=True), matrix(k=4), topk(k=4)
on the whole grid and on its first 65 files, and dice_match with n = 1 on five edge files.
  lf2047 / lf2048          NARROW_MUL 1 / 0 (the 64-bit products of ge<true>), products above 2^31
  lf2047_base200, _len20   CORPUS_FAST 0 by equality in 200 |Lf| < 1024 base, by length = 2^20
  base18_in / base18_out   base 2^18 - 1 / 2^18; w64 = 4101, rows packed from global memory. The
                           full-bitset layout of this corpus takes 23 s to compile, so only the
                           compact legs run here; both layouts' sources are checked on the CPU.
  pack8128 / pack8129      w64 = 127 / 128, the last LDS-staged and the first global-row size of
                           dice_pack_compact: 65 files, download_rows round trip, compact = bits leg
  ties                     200 near-ties (cross-difference 1) and 50 ties of unequal terms
T = 65: the same grids on the postings kernels (DICE_POST_PRUNE=0), the bound-pruned kernel (the
default), the LDS record kernel and the dense kernel, with the kernel kind asserted, the pruned
kernel's deferral at |W_F| = 2^28 and not at 2^28 - 1, and the corpora at post_feasible's limits.
"""
import numpy as np
import pytest

from tests import envelope_cases as E
from tests.test_envelope_edges import CASES, files_of, same

pytestmark = pytest.mark.gpu

ENV = ('DICE_PROG_MATCH', 'DICE_PROG_LAYOUT', 'DICE_LARGE_KERNEL', 'DICE_FORCE_DENSE', 'DICE_POST_PRUNE',
       'DICE_POST_DENSE', 'DICE_PRUNE_MAX_EVALS', 'DICE_PRUNE_ROUTE', 'DICE_PRUNE_ROUTE_AT', 'DICE_PRUNE_LONG_ROUTE')
LEGS = {'valu': {'DICE_PROG_MATCH': 'valu'}, 'mfma': {'DICE_PROG_MATCH': 'mfma'}, 'bits': {'DICE_PROG_LAYOUT': 'bits'}}
KINDS = {   # environment, dice_ctx_info kind, dice_ctx_match_kernel
    'post': ({'DICE_POST_PRUNE': '0'}, 3, 3),
    # dice_match sends a batch in which a quarter of the files have more words than the largest
    # template to the postings kernels whole, and most of the grid's files do: 'routed' is that
    # default, 'prune' has the pruned kernel answer every call
    'routed': ({}, 3, 4),
    'prune': ({'DICE_PRUNE_LONG_ROUTE': '0'}, 3, 4),
    'lds': ({'DICE_LARGE_KERNEL': 'lds'}, 2, 2),
    'dense': ({'DICE_FORCE_DENSE': '1'}, 0, 0),
}


def _scorer(c, env):
    from licensee_amd._native import Scorer
    mp = pytest.MonkeyPatch()
    try:
        for k in ENV:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        return Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab, device=0)
    finally:
        mp.undo()


class Expected:
    """The reference's outputs for one batch, computed once; a head of the batch is a slice."""

    def __init__(self, corpus, fb, k=4):
        ref = E.Reference(corpus, fb)
        self.out = {'match0': ref.match(0.0), 'match98': ref.match(98.0), 'conf': ref.match(98.0, confidence=True),
                    'matrix': ref.matrix(), 'topk': ref.topk(k)}
        self.k = k

    def get(self, what, n=None, idx=None):
        if idx is not None:
            return [a[idx] for a in self.out[what]]
        return [a[:n] for a in self.out[what]]


@pytest.fixture(scope='module')
def data():
    """name -> (case, files, Expected), built on first use and shared by the module's tests."""
    made = {}

    def get(name, k=4):
        if (name, k) not in made:
            case = CASES[name]()
            fb = files_of(name, case)
            made[name, k] = (case, fb, Expected(case.corpus, fb, k))
        return made[name, k]
    return get


def check_entry_points(sc, fb, exp, n, where, matrix=True):
    part = E.head(fb, n)
    same(sc.match(part, 0.0), exp.get('match0', n), (where, n, 'match 0'))
    same(sc.match(part, 98.0), exp.get('match98', n), (where, n, 'match 98'))
    same(sc.match(part, 98.0, confidence=True), exp.get('conf', n), (where, n, 'confidence'))
    if matrix:
        mov, msc, tki, tks = sc.matrix(part, exp.k)
        same((mov, msc), exp.get('matrix', n), (where, n, 'matrix'))
        same((tki, tks), exp.get('topk', n), (where, n, 'matrix top-k'))
        same(sc.topk(part, exp.k), exp.get('topk', n), (where, n, 'topk'))


def edge_files(fb):
    """Five files for the n = 1 call: |W_F| = 2^20 - 1 with len_F = 2^21 - 1 (the last fast file),
    |W_F| = 2^20, len_F = 2^21, len_F = 2^31 - 1 and |W_F| = 2^28."""
    wf, ln = fb.wordset_size.astype(np.int64), fb.length.astype(np.int64)
    picks = [np.flatnonzero((wf == E.P20 - 1) & (ln == E.P21 - 1)), np.flatnonzero((wf == E.P20) & (ln < E.P21)),
             np.flatnonzero((ln == E.P21) & (wf < E.P20)), np.flatnonzero(ln == (1 << 31) - 1), np.flatnonzero(wf == E.P28)]
    assert all(p.size for p in picks)
    return [int(p[0]) for p in picks]


def _tables(c):
    from tests.test_gpu_prog_mfma import _tables_dims
    return _tables_dims(c)[0]


# ---- T <= 64 -----------------------------------------------------------------------------------

SMALL = ['lf2047', 'lf2048', 'lf2047_base200', 'lf2047_len20', 'pack8128', 'pack8129', 'base18_in', 'base18_out']


# every leg of every corpus, except the full-bitset layout of the 2^18-word corpora (23 s to compile)
SMALL_LEGS = [(name, leg) for name in SMALL for leg in LEGS if not (name.startswith('base18') and leg == 'bits')]


@pytest.mark.parametrize('name,leg', SMALL_LEGS)
def test_sparse_program_grid(data, name, leg):
    case, fb, exp = data(name)
    sc = _scorer(case.corpus, LEGS[leg])
    try:
        assert sc.info()[2] == 1
        if leg == 'valu':
            assert sc.program_stage() == 0
        if leg == 'mfma':                       # the matrix-core stage needs a bit region in the compact tile
            assert sc.program_stage() == (2 if _tables(case.corpus) > 0 else 0)
        for n in (fb.n, 65):
            check_entry_points(sc, fb, exp, n, (name, leg))
        for i in edge_files(fb):
            one = E.take(fb, [i])
            same(sc.match(one, 98.0), exp.get('match98', idx=[i]), (name, leg, 'dice_match n=1', i))
            same(sc.match(one, 0.0), exp.get('match0', idx=[i]), (name, leg, 'dice_match n=1', i))
    finally:
        sc.close()


@pytest.mark.parametrize('leg', list(LEGS))
@pytest.mark.parametrize('name', ['lf2047', 'lf2048'])
def test_one_lane_past_each_cut(data, name, leg):
    """Waves whose only lane outside the envelope has |W_F| = 2^20, or len_F = 2^21."""
    case, grid, _ = data(name)
    fb, _ = E.cut_waves(grid)
    exp = Expected(case.corpus, fb)
    sc = _scorer(case.corpus, LEGS[leg])
    try:
        check_entry_points(sc, fb, exp, fb.n, (name, leg, 'cut waves'))
    finally:
        sc.close()


def test_stage_two_runs_on_the_twins():
    """The 2,047 / 2,048-word twins have a bit region, so DICE_PROG_MATCH=mfma is the matrix-core
    kernel on both sides of NARROW_MUL."""
    for name in ('lf2047', 'lf2048'):
        assert _tables(CASES[name]().corpus) > 0


def _download_rows(b):
    """dice_batch_download_rows without field masks (the batch was uploaded as bitsets)."""
    from licensee_amd import _native
    rows = np.empty((b.n, _native.words64(b.scorer.n_vocab)), np.uint64)
    wf = np.empty(b.n, np.uint32)
    _native._check(_native.load_library().dice_batch_download_rows(b._b, rows.ctypes.data, wf.ctypes.data, None, None))
    return rows, wf


@pytest.mark.parametrize('V', [8128, 8129])
def test_pack_edges(data, V):
    """w64 = 127 (65,280 bytes of LDS rows) and w64 = 128 (rows read from global memory): a full tile
    and a partial one, the all-words file and the last-word file among them."""
    case, fb, exp = data(f'pack{V}')
    c, n = case.corpus, 65
    part = E.head(fb, n)
    words = E.unpack(part.bits, V)
    assert words.all(1).any() and ((words.sum(1) == 1) & (words[:, V - 1] == 1)).any()
    assert c.w64 == (127 if V == 8128 else 128)
    got = {}
    for leg in ('valu', 'bits'):
        sc = _scorer(c, LEGS[leg])
        b = sc.batch(n)
        try:
            b.upload(part)
            b.match(98.0)
            m = b.download_match()
            b.matrix(4)
            mat = b.download_matrix()
            rows, wf = _download_rows(b)
            assert np.array_equal(rows, part.bits) and np.array_equal(wf, part.wordset_size), (V, leg, 'download_rows')
            same(m, exp.get('match98', n), (V, leg, 'match'))
            same(mat[:2], exp.get('matrix', n), (V, leg, 'matrix'))
            same(mat[2:], exp.get('topk', n), (V, leg, 'topk'))
            got[leg] = m + mat
        finally:
            b.close()
            sc.close()
    same(got['valu'], got['bits'], (V, 'compact against bits'))


# ---- near-ties and ties of unequal terms ---------------------------------------------------------

def check_ties(sc, fb, exp, where):
    same(sc.match(fb, 0.0), exp.get('match0'), (where, 'match 0'))
    same(sc.match(fb, 98.0, confidence=True), exp.get('conf'), (where, 'confidence'))
    mov, msc, tki, tks = sc.matrix(fb, 2)
    same((mov, msc), exp.get('matrix'), (where, 'matrix'))
    same((tki, tks), exp.get('topk'), (where, 'matrix top-2'))
    same(sc.topk(fb, 2), exp.get('topk'), (where, 'topk 2'))


@pytest.mark.parametrize('leg', list(LEGS))
def test_ties_sparse_program(data, leg):
    case, fb, exp = data('ties', 2)
    assert fb.n == 250
    sc = _scorer(case.corpus, LEGS[leg])
    try:
        assert sc.info()[2] == 1
        check_ties(sc, fb, exp, ('ties', leg))
    finally:
        sc.close()


@pytest.mark.parametrize('kind', list(KINDS))
def test_ties_large_corpus(data, kind):
    case, fb, exp = data('ties_T65', 2)
    env, info_kind, match_kernel = KINDS[kind]
    sc = _scorer(case.corpus, env)
    try:
        assert sc.info()[2] == info_kind and sc.match_kernel() == match_kernel
        check_ties(sc, fb, exp, ('ties_T65', kind))
    finally:
        sc.close()


# ---- T = 65 ------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('name', ['lf2047_T65', 'lf2048_T65'])
def test_large_corpus_grid(data, name, kind):
    case, fb, exp = data(name)
    env, info_kind, match_kernel = KINDS[kind]
    sc = _scorer(case.corpus, env)
    try:
        assert sc.info()[2] == info_kind and sc.match_kernel() == match_kernel
        for n in (fb.n, 65):
            check_entry_points(sc, fb, exp, n, (name, kind))
    finally:
        sc.close()


@pytest.mark.parametrize('name', ['lf2047_T65', 'lf2048_T65'])
def test_pruned_kernel_defers_at_2_28(data, name):
    """|W_F| = 2^28 goes to the postings kernels, 2^28 - 1 is answered by the pruned kernel itself.
    Files without a vocabulary word take the pruned kernel's shortest path (no bound, no route), so
    among them the count of deferred files is exactly the count at or above 2^28."""
    from licensee_amd._native import FileBatch
    case, fb, exp = data(name)
    sc = _scorer(case.corpus, KINDS['prune'][0])
    try:
        assert sc.match_kernel() == 4
        b = sc.batch(fb.n)
        try:
            b.upload(fb)
            for conf, what in ((False, 'match98'), (True, 'conf')):
                b.match(98.0, confidence=conf)
                same(b.download_match(), exp.get(what), (name, what))
                assert b.deferred() >= int((fb.wordset_size >= E.P28).sum()) > 0
            empty = np.flatnonzero(~fb.bits.any(1))
            below = empty[fb.wordset_size[empty] == E.P28 - 1]
            at = empty[fb.wordset_size[empty] == E.P28]
            assert below.size >= 5 and at.size >= 5
            for idx, expect in ((below, 0), (at, at.size), (np.concatenate([below, at]), at.size)):
                part = E.take(fb, idx)
                b.upload(part)
                b.match(98.0)
                same(b.download_match(), exp.get('match98', idx=idx), (name, 'empty files', expect))
                assert b.deferred() == expect
            # the same rows one step apart: only |W_F| moves across the cut
            wf = fb.wordset_size[below].copy()
            for step, expect in ((0, 0), (1, below.size)):
                part = FileBatch(fb.bits[below], wf + step, fb.length[below], fb.cc_false_positive[below])
                b.upload(part)
                b.match(98.0)
                same(b.download_match(), E.Reference(case.corpus, part).match(98.0), (name, 'step', step))
                assert b.deferred() == expect
        finally:
            b.close()
    finally:
        sc.close()


# ---- post_feasible's limits --------------------------------------------------------------------

@pytest.mark.parametrize('name', ['post_in', 'post_lf', 'post_slack', 'post_base65535', 'post_base65536'])
def test_postings_limits(data, name):
    """The default choice for T = 65: postings kernels (kind 3) on the feasible side of each limit,
    LDS records (kind 2) on the other; results equal the reference on both. A base of 65,535 needs
    |Lf| >= 65,535, which is infeasible by itself, so both base corpora are kind 2 and the largest
    feasible base is post_in's 65,534."""
    case, fb, exp = data(name)
    sc = _scorer(case.corpus, {})
    try:
        assert sc.info()[2] == case.expect['kernel_kind']
        # (the pruned kernel's tables take at most 512 u64 words per row; this corpus has 1,027)
        assert sc.match_kernel() == case.expect['kernel_kind']
        check_entry_points(sc, fb, exp, fb.n, name)
        check_entry_points(sc, fb, exp, 65, name, matrix=False)
    finally:
        sc.close()
    if name == 'post_in':
        full = np.flatnonzero(E.unpack(fb.bits, case.corpus.n_vocab).all(1))
        assert full.size and (exp.out['matrix'][0][full, 40] == 65534).all()
