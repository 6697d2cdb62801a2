"""The device memory of dice_ctx and dice_batch across growth and back: every allocation path of the
host layer is walked from a small size to a larger one and to the small one again on one batch or one
context, and every result is compared bit for bit (np.array_equal) with the same call on a freshly
created batch or context, or with the host's own encoding of the files.

Two corpora from tests/exact_cases.py: `chunks` (T = 12, V = 8,320: the sparse program, template-major
matrix, transposed downloads) and `chunks65` (T = 65: the postings kernels, row-major matrix, the dense
partials of post_reserve). n <= 300. No assertion reads free device memory: the device is shared.
"""
import ctypes

import numpy as np
import pytest

from tests import exact_cases as X
from tests.envelope_cases import head

pytestmark = pytest.mark.gpu

KIND = {'chunks': 1, 'chunks65': 3}
MAKE = {'chunks': X.chunks, 'chunks65': lambda: X.padded(X.chunks())}
ENV = ('DICE_PROG_MATCH', 'DICE_PROG_LAYOUT', 'DICE_LARGE_KERNEL', 'DICE_FORCE_DENSE', 'DICE_POST_PRUNE',
       'DICE_POST_DENSE', 'DICE_PRUNE_MAX_EVALS', 'DICE_PRUNE_ROUTE', 'DICE_PRUNE_ROUTE_AT', 'DICE_PRUNE_LONG_ROUTE',
       'DICE_NO_SMALL_CALL')
N = 300
NAMES = ['chunks', 'chunks65']


def new_scorer(corpus):
    from licensee_amd._native import Scorer
    mp = pytest.MonkeyPatch()
    try:
        for k in ENV:
            mp.delenv(k, raising=False)
        return Scorer(*corpus.arrays(), corpus.n_vocab, device=0)
    finally:
        mp.undo()


class Leg:
    """A corpus, a context with the Exact and wordset tables set, N files as sets, as bitsets with
    their field masks and as texts, and the set reference's Exact answers."""

    def __init__(self, name):
        self.c = MAKE[name]()
        self.corpus, self.ws, self.fbits, self.need = self.c.encoded()
        self.sc = new_scorer(self.corpus)
        self.sc.exact_setup(self.ws, self.fbits, self.need)
        self.sc.vocab_setup(*X.vocabulary(self.c.V))
        self.files = X.sized(self.c, N)
        self.fb, self.fm = X.encode_files(self.c.V, self.files)
        self.exp = X.reference(self.c.templates, self.files)

    def fresh(self, fn, capacity=N):
        """fn on a batch nothing else has touched."""
        b = self.sc.batch(capacity)
        try:
            return fn(b)
        finally:
            b.close()


@pytest.fixture(scope='module')
def legs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Leg(name)
            assert made[name].sc.info()[2] == KIND[name]
        return made[name]
    yield get
    for leg in made.values():
        leg.sc.close()


def rows_of(b, masks):
    """dice_batch_download_rows; without masks the batch need not hold any."""
    from licensee_amd._native import _check, _ptr, load_library, words64
    bits = np.empty((b.n, words64(b.scorer.n_vocab)), np.uint64)
    wf = np.empty(b.n, np.uint32)
    fm = np.empty(b.n, np.uint64) if masks else None
    _check(load_library().dice_batch_download_rows(b._b, _ptr(bits), _ptr(wf), _ptr(fm), None))
    return bits, wf, fm


def same(got, want, where):
    assert len(got) == len(want), where
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (where, j)


def matched(b):
    b.match(98.0)
    return b.download_match()


# ---- uploads -----------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_id_list_upload_grows_and_shrinks(legs, name):
    """The id staging of dice_batch_upload_ids: 4 files, 300, 4 again on one batch."""
    from licensee_amd._native import bits_to_ids
    leg = legs(name)
    b = leg.sc.batch(N)
    sizes = []
    for n in (4, N, 4):
        part = head(leg.fb, n)
        off, ids = bits_to_ids(part.bits, leg.c.V)
        sizes.append(int(off[-1]))
        b.upload_ids(off, ids, part.wordset_size, part.length, part.cc_false_positive)
        bits, wf, _ = rows_of(b, False)
        assert np.array_equal(bits, part.bits) and np.array_equal(wf, part.wordset_size), n

        def by_bitsets(f):
            f.upload(part)
            return rows_of(f, False)[:2] + matched(f)
        same((bits, wf) + matched(b), leg.fresh(by_bitsets), ('ids', n))
    assert sizes[1] > 8 * sizes[0] > 0
    b.close()


@pytest.mark.parametrize('utf8_middle', [False, True])
@pytest.mark.parametrize('name', NAMES)
def test_text_upload_grows_and_shrinks(legs, name, utf8_middle):
    """The text buffer of dice_batch_upload_text: a small text, one more than ten times larger, the
    small one again; the middle upload once more in the UTF-8 form (the texts are ASCII: the same
    bytes). Rows, |W_F| and field masks equal the host's each time."""
    leg = legs(name)
    b = leg.sc.batch(N)
    nbytes = []
    for step, n in enumerate((6, N, 6)):
        part = head(leg.fb, n)
        text, off, tl = X.texts_of(leg.files[:n])
        nbytes.append(text.shape[0])
        utf8 = utf8_middle and step == 1
        st = b.upload_text(text, off, tl, part.length, part.cc_false_positive, utf8=utf8)
        assert not st.any()
        bits, wf, fm = rows_of(b, True)
        assert np.array_equal(bits, part.bits) and np.array_equal(wf, part.wordset_size), (step, n)
        assert np.array_equal(fm, leg.fm[:n]), (step, n)
        assert np.array_equal(b.download_length(), part.length)

        def by_bitsets(f):
            f.upload(part)
            return matched(f)
        same(matched(b), leg.fresh(by_bitsets), ('text', step))
        b.exact(None)
        assert np.array_equal(b.download_exact(), leg.exp[:n]), (step, n)
    assert nbytes[1] > 10 * nbytes[0]
    b.close()


@pytest.mark.parametrize('name', NAMES)
def test_field_masks_first_allocated_by_each_caller(legs, name):
    """The mask buffer is allocated by whichever of dice_batch_exact, a text upload and
    dice_batch_set_rows comes first on a batch: one fresh batch each, the same Exact answers."""
    leg = legs(name)
    fb, fm = leg.fb, leg.fm
    text, off, tl = X.texts_of(leg.files)
    idx = np.array([0, 63, 64, 130, 255, N - 1], np.int64)

    def by_exact(b):
        b.upload(fb)
        b.exact(fm)
        return b.download_exact()

    def by_text(b):
        assert not b.upload_text(text, off, tl, fb.length, fb.cc_false_positive).any()
        b.exact(None)
        return b.download_exact()

    def by_set_rows(b):
        b.upload(fb)
        b.set_rows(idx, fb.bits[idx], fb.wordset_size[idx], fm[idx])
        b.exact(fm)
        return b.download_exact()

    for fn in (by_exact, by_text, by_set_rows):
        assert np.array_equal(leg.fresh(fn), leg.exp), fn.__name__
    assert (leg.exp >= 0).sum() >= 10 and (leg.exp < 0).sum() >= 10     # the reference gives both answers


# ---- rankings ----------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_topk_sizes_then_matrix(legs, name):
    """dice_batch_topk with k = 3, 16, 3, then dice_batch_matrix(3), on one batch: the [n][k] buffers
    grow, the N x T buffers come last (at T = 65 the first ranking also makes the dense partials)."""
    leg = legs(name)
    b = leg.sc.batch(N)
    b.upload(leg.fb)
    assert b.matrix_bytes() == 0
    for k in (3, 16, 3):
        b.topk(k)

        def ranked(f):
            f.upload(leg.fb)
            f.topk(k)
            return f.download_topk()
        same(b.download_topk(), leg.fresh(ranked), ('topk', k))
        assert b.matrix_bytes() == 0, k

    def full(f):
        f.upload(leg.fb)
        f.matrix(3)
        return f.download_matrix() + (np.array([f.matrix_bytes()]),)
    b.matrix(3)
    want = leg.fresh(full)
    same(b.download_matrix() + (np.array([b.matrix_bytes()]),), want, 'matrix')
    assert int(want[-1][0]) >= N * len(leg.c.templates) * 12
    same(matched(b), leg.fresh(lambda f: (f.upload(leg.fb), matched(f))[1]), 'match after the rankings')
    b.close()


def test_transposed_downloads_grow_the_stage(legs):
    """The sparse program's template-major results come back through the batch's transposing stage:
    n = 1, then n = capacity, then n = 1."""
    leg = legs('chunks')
    b = leg.sc.batch(N)
    for n in (1, N, 1):
        part = head(leg.fb, n)

        def full(f):
            f.upload(part)
            f.matrix(3)
            return f.download_matrix()
        same(full(b), leg.fresh(full), ('stage', n))
    b.close()


# ---- projects ----------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_project_counts_grow_and_shrink(legs, name):
    """dice_batch_projects with P = 1, 65, 200, 1 over the same files: the record buffers grow
    64 -> 128 -> 256 and are then reused."""
    leg = legs(name)
    T = len(leg.c.templates)
    rng = np.random.default_rng(12)
    fflags = rng.integers(0, 8, N).astype(np.uint8) * (rng.random(N) < 0.2)
    tflags = rng.integers(0, 4, T).astype(np.uint8)

    def ready(b):
        b.upload(leg.fb)
        b.match(90.0)
        b.exact(leg.fm)

    def resolve(b, P):
        off = np.floor(np.linspace(0, N, P + 1)).astype(np.int64)
        b.projects(off, fflags, tflags, use_exact=True, k=4)
        return b.download_projects() + b.download_project_match()[:2]

    b = leg.sc.batch(N)
    ready(b)
    for P in (1, 65, 200, 1):
        got = resolve(b, P)
        assert got[0].shape == (P,)
        same(got, leg.fresh(lambda f: (ready(f), resolve(f, P))[1]), ('projects', P))
    b.close()


# ---- the host-buffer calls and the contexts' own batches ---------------------------------------

def batch_api(leg, part):
    """dice_match, dice_similarity_matrix(3) and dice_topk(3) of `part` through a fresh batch."""
    def run(b):
        b.upload(part)
        m = matched(b)
        b.matrix(3)
        mx = b.download_matrix()
        b.topk(3)
        return m + mx + b.download_topk()
    return leg.fresh(run)


@pytest.mark.parametrize('name', NAMES)
def test_host_buffer_calls_on_one_context(legs, name):
    """n = 5 (the small-call batch), 65, 300 (the scratch batch destroyed and re-created), 65, 5 on one
    context; then the context is destroyed with both internal batches live."""
    leg = legs(name)
    sc = new_scorer(leg.corpus)
    try:
        for n in (5, 65, N, 65, 5):
            part = head(leg.fb, n)
            got = sc.match(part, 98.0) + sc.matrix(part, 3) + sc.topk(part, 3)
            same(got, batch_api(leg, part), ('host', n))
    finally:
        sc.close()


@pytest.mark.parametrize('name', NAMES)
def test_context_and_batch_cycles(legs, name):
    """Twenty create -> upload -> match -> destroy cycles: the batch is destroyed before its context,
    the context's small-call and scratch batches by destroying the context alone."""
    leg = legs(name)
    small = head(leg.fb, 5)
    want = None
    for cycle in range(20):
        sc = new_scorer(leg.corpus)
        try:
            b = sc.batch(N)
            b.upload(leg.fb)
            got = matched(b)
            b.close()
            got += sc.match(small, 98.0) + sc.match(leg.fb, 98.0)
        finally:
            sc.close()
        if want is None:
            want = got
            same(got[:3], got[6:], 'batch and host-buffer call')
        same(got, want, cycle)
