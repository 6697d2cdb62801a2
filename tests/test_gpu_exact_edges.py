"""dice_exact_kernel and dice_exact_setup at their edges, through the C-ABI wrappers of _native.py,
against the set reference of tests/exact_cases.py. Every comparison is np.array_equal.

  chunks     w64 = 130: templates of 0, 1, 63, 64, 65, 128, 129 and 130 records, near misses in records
             0, 62, 63, 64, 65, 127, 128 and the last (the record loop's second and third pass and its
             partial last pass), bits 0, 31, 32 and 63, records from field_bits alone, |W_F| = 0 and
             2^32 - 1. Two legs: as built (T = 12, sparse program, the compact repack beside the rows)
             and padded to T = 65 (postings kernels, row-major batch alone).
  runs       T = 300 > 256: a size run of 70, a run that ends the sorted table, duplicates, templates
             that differ in need alone (bits 0, 31, 32, 63, all 64), with and without field masks.
  placement  the pending file on lane 0 only, lane 63 only, on every lane, on the last lane of a
             partial last wave, in the last wave of a 256-thread block; n = 1 ... 700.
  state      Exact before and after match / matrix / topk on one batch, re-uploads, id-list upload,
             a second dice_exact_setup, n = 0, and where dice_batch_exact(NULL) takes its masks from.
"""
import numpy as np
import pytest

from tests import exact_cases as X

pytestmark = pytest.mark.gpu

KIND = {'chunks': 1, 'chunks65': 3, 'runs': 3}
MAKE = {'chunks': X.chunks, 'chunks65': lambda: X.padded(X.chunks()), 'runs': X.runs}
ENV = ('DICE_PROG_MATCH', 'DICE_PROG_LAYOUT', 'DICE_LARGE_KERNEL', 'DICE_FORCE_DENSE', 'DICE_POST_PRUNE',
       'DICE_POST_DENSE', 'DICE_PRUNE_MAX_EVALS', 'DICE_PRUNE_ROUTE', 'DICE_PRUNE_ROUTE_AT', 'DICE_PRUNE_LONG_ROUTE')
CAPACITY = 512


class Leg:
    """A corpus, its context with the Exact tables set, its files encoded, the reference's answers
    with the files' field masks (exp) and without (exp0), computed once."""

    def __init__(self, name):
        from licensee_amd._native import Scorer
        self.c = MAKE[name]()
        self.corpus, self.ws, self.fbits, self.need = self.c.encoded()
        mp = pytest.MonkeyPatch()
        try:
            for k in ENV:
                mp.delenv(k, raising=False)
            self.sc = Scorer(*self.corpus.arrays(), self.corpus.n_vocab, device=0)
        finally:
            mp.undo()
        self.sc.exact_setup(self.ws, self.fbits, self.need)
        self.fb, self.fm = X.encode_files(self.c.V, self.c.files)
        self.exp = X.reference(self.c.templates, self.c.files)
        self.exp0 = X.reference(self.c.templates, X.strip_fields(self.c.files))

    def check(self, files, where, batch=None):
        """The one-shot call and, given a batch, upload / exact / download_exact, with and without masks."""
        fb, fm = X.encode_files(self.c.V, files)
        exp = X.reference(self.c.templates, files)
        exp0 = X.reference(self.c.templates, X.strip_fields(files))
        assert np.array_equal(self.sc.exact(fb, fm), exp), (where, 'dice_exact')
        assert np.array_equal(self.sc.exact(fb, None), exp0), (where, 'dice_exact, no masks')
        if batch is not None:
            batch.upload(fb)
            batch.exact(fm)
            assert np.array_equal(batch.download_exact(), exp), (where, 'batch')
            batch.exact(None)
            assert np.array_equal(batch.download_exact(), exp0), (where, 'batch, no masks')
        return exp


@pytest.fixture(scope='module')
def legs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Leg(name)
        return made[name]
    yield get
    for leg in made.values():
        leg.sc.close()


# ---- the corpora -------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['chunks', 'chunks65', 'runs'])
def test_corpus_one_shot_and_batch(legs, name):
    leg = legs(name)
    assert leg.sc.info()[2] == KIND[name] and leg.sc.info()[0] == len(leg.c.templates)
    assert (leg.exp >= 0).sum() >= len(leg.c.templates) - 2 and (leg.exp < 0).sum() >= 20
    assert np.array_equal(leg.sc.exact(leg.fb, leg.fm), leg.exp)
    assert np.array_equal(leg.sc.exact(leg.fb, None), leg.exp0)
    b = leg.sc.batch(leg.fb.n)
    b.upload(leg.fb)
    b.exact(leg.fm)
    assert np.array_equal(b.download_exact(), leg.exp)
    b.exact(None)
    assert np.array_equal(b.download_exact(), leg.exp0)
    b.close()
    if leg.c.special:      # |W_F| = 2^32 - 1 beside ordinary files (outside the Dice input domain: Exact only)
        exp = leg.check(leg.c.special, (name, 'special'))
        assert exp[0] == -1 and (exp >= 0).any()


@pytest.mark.parametrize('where', ['lane0', 'lane63', 'all64', 'partial_last_wave', 'block_last_wave', 'mixed_depths'])
def test_placements(legs, where):
    leg = legs('runs')
    files = X.placements(leg.c)[where]
    b = leg.sc.batch(len(files))
    exp = leg.check(files, where, b)
    b.close()
    assert (exp >= 0).any()


@pytest.mark.parametrize('n', X.BATCH_SIZES)
@pytest.mark.parametrize('name', ['chunks', 'runs'])
def test_batch_sizes(legs, name, n):
    leg = legs(name)
    b = leg.sc.batch(n)
    leg.check(X.sized(leg.c, n), (name, n), b)
    b.close()


# ---- batch state -------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['chunks', 'chunks65'])
def test_exact_before_and_after_dice_on_one_batch(legs, name):
    """The T <= 64 leg keeps the compact repack beside the row-major rows Exact reads; the T = 65 leg
    scores from those rows. Neither match, matrix nor topk may change them or the resident result."""
    leg = legs(name)
    assert leg.fb.n <= CAPACITY
    b = leg.sc.batch(CAPACITY)
    b.upload(leg.fb)
    b.exact(leg.fm)
    assert np.array_equal(b.download_exact(), leg.exp)
    b.match(98.0)
    m = b.download_match()
    assert np.array_equal(b.download_exact(), leg.exp)          # the resident result outlives the match
    b.matrix(3)
    b.download_matrix()
    b.topk(3)
    b.download_topk()
    b.exact(leg.fm)
    assert np.array_equal(b.download_exact(), leg.exp)
    for got, want in zip(m, leg.sc.match(leg.fb, 98.0)):        # and Dice on the batch is Dice
        assert np.array_equal(got, want)
    b.close()


@pytest.mark.parametrize('name', ['chunks', 'chunks65'])
def test_reupload_id_upload_and_empty_batch(legs, name):
    from licensee_amd._native import bits_to_ids
    from tests.envelope_cases import head
    leg = legs(name)
    b = leg.sc.batch(CAPACITY)
    for n in (100, 37, leg.fb.n):                               # smaller, then larger
        b.upload(head(leg.fb, n))
        b.exact(leg.fm[:n])
        assert np.array_equal(b.download_exact(), leg.exp[:n]), n
    off, ids = bits_to_ids(leg.fb.bits, leg.c.V)
    b.upload(head(leg.fb, 5))
    b.upload_ids(off, ids, leg.fb.wordset_size, leg.fb.length, leg.fb.cc_false_positive)
    b.exact(leg.fm)
    assert np.array_equal(b.download_exact(), leg.exp)
    empty, no_masks = X.encode_files(leg.c.V, [])
    b.upload(empty)
    b.exact(None)
    assert b.download_exact().shape == (0,)
    b.exact(no_masks)
    assert b.download_exact().shape == (0,)
    b.upload(leg.fb)
    b.exact(leg.fm)
    assert np.array_equal(b.download_exact(), leg.exp)
    b.close()


@pytest.mark.parametrize('name', ['chunks', 'chunks65'])
def test_second_setup_replaces_the_tables(legs, name):
    leg = legs(name)
    r = X.retabled(leg.c)
    _, ws2, fbits2, need2 = r.encoded()
    fb, fm = X.encode_files(r.V, r.files)
    old, new = X.reference(leg.c.templates, r.files), X.reference(r.templates, r.files)
    assert (old != new).sum() >= 2 * len(r.templates) - 2
    b = leg.sc.batch(CAPACITY)
    b.upload(fb)
    b.exact(fm)
    assert np.array_equal(b.download_exact(), old)
    try:
        leg.sc.exact_setup(ws2, fbits2, need2)
        b.exact(fm)                                             # the resident batch, the new tables
        assert np.array_equal(b.download_exact(), new)
        assert np.array_equal(leg.sc.exact(fb, fm), new)
    finally:
        leg.sc.exact_setup(leg.ws, leg.fbits, leg.need)
    b.exact(fm)
    assert np.array_equal(b.download_exact(), old)
    b.close()


# ---- where dice_batch_exact(NULL) takes its masks from -----------------------------------------

def test_mask_provenance(legs):
    """include/licensee_dice.h, dice_batch_exact: NULL masks mean the device's own masks after a text
    upload -- dice_batch_set_rows patches included -- and all-zero masks after every other upload,
    whatever an earlier call left in the mask buffer and whatever dice_batch_set_rows writes there."""
    leg = legs('runs')
    c, fb, fm = leg.c, leg.fb, leg.fm
    assert fb.n <= CAPACITY and (fm >> np.uint64(63)).any()
    leg.sc.vocab_setup(*X.vocabulary(c.V))
    text, off, tl = X.texts_of(c.files)
    b = leg.sc.batch(CAPACITY)

    def upload_text():
        st = b.upload_text(text, off, tl, fb.length, fb.cc_false_positive)
        assert not st.any()

    upload_text()
    b.exact(None)
    assert np.array_equal(b.download_exact(), leg.exp)
    bits, wf, dm = b.download_rows()
    assert np.array_equal(bits, fb.bits) and np.array_equal(wf, fb.wordset_size) and np.array_equal(dm, fm)
    b.exact(fm)
    assert np.array_equal(b.download_exact(), leg.exp)
    # bitsets into the same batch: the masks of the text upload are still in the buffer, and stale
    b.upload(fb)
    b.exact(None)
    assert np.array_equal(b.download_exact(), leg.exp0)
    assert (leg.need[leg.exp[leg.exp >= 0]] != 0).sum() >= 40 and (leg.exp0 != leg.exp).sum() >= 40
    # patches: six files become six others, masks included
    src = [c.pick(kind='need', of='g40_63')[0], c.pick(kind='need', of='g50_0')[0], c.pick(kind='own', of='g40_all')[0],
           c.pick(kind='fm_lacks', s=40, bit=63)[0], c.pick(kind='own', of='long3')[0], c.pick(kind='x_for_field', s=50)[0]]
    idx = np.array([0, 63, 64, 130, 255, 299], np.int64)
    patched = list(c.files)
    for i, s in zip(idx, src):
        patched[i] = c.files[s]
    exp_p = X.reference(c.templates, patched)
    assert (exp_p[idx] != leg.exp[idx]).all() and (exp_p[idx] >= 0).sum() == 4
    upload_text()
    b.set_rows(idx, fb.bits[src], fb.wordset_size[src], fm[src])
    b.exact(None)
    assert np.array_equal(b.download_exact(), exp_p)
    # ... and without masks (NULL: zero) the patched files have none, the others keep the device's
    upload_text()
    b.set_rows(idx, fb.bits[src], fb.wordset_size[src], None)
    b.exact(None)
    half = list(c.files)
    for i, W in zip(idx, X.strip_fields([c.files[s] for s in src])):
        half[i] = W
    assert np.array_equal(b.download_exact(), X.reference(c.templates, half))
    # after a bitset upload the patches' masks do not count either: no file has a device mask
    b.upload(fb)
    b.set_rows(idx, fb.bits[src], fb.wordset_size[src], fm[src])
    b.exact(None)
    assert np.array_equal(b.download_exact(), X.reference(c.templates, X.strip_fields(patched)))
    b.exact(X.encode_files(c.V, patched)[1])
    assert np.array_equal(b.download_exact(), exp_p)
    b.close()
