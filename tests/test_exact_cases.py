"""The inputs of tests/exact_cases.py, judged from the set reference alone (no GPU): every category a
GPU test relies on is non-empty and says what its name says, so no device test can pass on an empty
or mislabelled case. Conditions, not measurements."""
import os
import re

import numpy as np
import pytest

from tests import exact_cases as X


@pytest.fixture(scope='module')
def chunks():
    c = X.chunks()
    return c, X.reference(c.templates, c.files)


@pytest.fixture(scope='module')
def runs():
    c = X.runs()
    return c, X.reference(c.templates, c.files)


def _sorted_positions(c):
    """Key indices by (|W_t|, key index): the order the device table is specified to have."""
    return sorted(range(len(c.templates)), key=lambda t: (len(c.templates[t].words), t))


def _run_of(c, size):
    return [t for t in range(len(c.templates)) if len(c.templates[t].words) == size]


# ---- the encoder -------------------------------------------------------------------------------

@pytest.mark.parametrize('make', [X.chunks, lambda: X.padded(X.chunks()), lambda: X.retabled(X.chunks()), X.runs],
                         ids=['chunks', 'chunks65', 'chunks_retabled', 'runs'])
def test_decoding_the_encoders_output_reproduces_the_sets(make):
    c = make()
    corpus, ws, fbits, need = c.encoded()
    assert corpus.n_vocab == c.V and corpus.lf_bits.shape == (len(c.templates), (c.V + 63) // 64)
    for tp, (lf, fields, size) in zip(c.templates, X.decode_templates(c.V, corpus, ws, fbits, need)):
        assert (lf, fields, size) == (tp.lf, tp.fields, len(tp.words)), tp.name
    assert np.array_equal(corpus.lf_size, [len(t.lf) for t in c.templates])
    for files in (c.files, c.special):
        fb, fm = X.encode_files(c.V, files)
        assert fb.n == len(files) == fm.shape[0]
        for W, got in zip(files, X.decode_files(c.V, fb, fm)):
            assert got == X.split_file(W)
    fb, fm = X.encode_files(c.V, [])
    assert fb.n == 0 and fb.bits.shape == (0, (c.V + 63) // 64) and fm.shape == (0,)


def test_dice_input_domain():
    """Every denominator of every (file, template) pair is in (0, 2^31), so match, matrix and topk
    may run on the same batches (envelope_cases.Reference asserts it pair by pair)."""
    for c in (X.chunks(), X.padded(X.chunks())):
        corpus = c.encoded()[0]
        fb, _ = X.encode_files(c.V, c.files)
        base = corpus.lf_size.astype(np.int64) - corpus.fields_set_size.astype(np.int64)
        assert (base >= 0).all()
        d = np.abs(corpus.length.astype(np.int64)[None, :] - fb.length.astype(np.int64)[:, None])
        adj = np.where(corpus.length_slack[None, :] < 0, d, np.maximum(d - corpus.length_slack[None, :], 0))
        den = base[None, :] + fb.wordset_size.astype(np.int64)[:, None] + adj // 4
        assert den.min() > 0 and den.max() < 2 ** 31
    assert X.wsize(X.chunks().special[0]) == 2 ** 32 - 1


# ---- chunks ------------------------------------------------------------------------------------

def test_chunks_templates_are_what_they_are_named(chunks):
    c, _ = chunks
    assert c.V == 8320 and 8 <= len(c.templates) <= 16
    by = {t.name: t for t in c.templates}
    assert [t.name for t in c.templates] != sorted(by)           # shuffled key order
    for k in X.REC_COUNTS:
        assert len(X.records(by[f'r{k}'])) == k
    assert not by['r0'].lf and all(not X.is_vocab(w) for w in by['r0'].fields) and by['r0'].fields
    for name, only in (('r65', {64}), ('r128', {64, 127}), ('r129', {64, 128}), ('r130', {64, 129}), ('r64', set())):
        tp = by[name]
        recs = X.records(tp)
        got = {r for r, p in enumerate(recs) if not any(w // 64 == p for w in tp.lf)}
        assert got == only, name
    # records of several bits, records with bits 0, 31, 32, 63, and records fed by Lf and fields both
    for tp in (by['r129'], by['r130']):
        per = {}
        for w in tp.words:
            if X.is_vocab(w):
                per.setdefault(w // 64, set()).add(w % 64)
        assert any(b == set(X.EDGE_BITS) for b in per.values()) and any(len(b) == 3 for b in per.values())
        assert any(any(w // 64 == p for w in tp.lf) and any(X.is_vocab(w) and w // 64 == p for w in tp.fields) for p in per)
    assert len(X.records(by['r130b'])) == 130 and len(by['r130b'].words) == len(by['r130'].words)
    assert len(by['r130b'].words ^ by['r130'].words) == 2
    a, b, cc = by['A'].words, by['B'].words, by['C'].words
    assert a < b < cc and (len(a), len(b), len(cc)) == (10, 11, 12)


def test_chunks_near_misses_reject_and_their_twins_match(chunks):
    c, ref = chunks
    own = {c.meta[i]['of']: i for i in c.pick(kind='own')}
    fb, fm = X.encode_files(c.V, c.files)
    by = {t.name: t for t in c.templates}
    for name in ('r1', 'r63', 'r64', 'r65', 'r128', 'r129', 'r130', 'r130b'):
        k = len(X.records(by[name]))
        assert ref[own[name]] == c.index(name)
        for r in sorted({r for r in X.POSITIONS if r < k} | {k - 1}):
            drops = c.pick(kind='drop', of=name, rec=r)
            assert {c.meta[i]['bit'] for i in drops} == ({0, 31, 32, 62} if (name, r) == ('r130b', 129) else set(X.EDGE_BITS))
            assert len(c.pick(kind='partial', of=name, rec=r)) == 1
            for i in drops + c.pick(kind='partial', of=name, rec=r):
                m = c.meta[i]
                assert ref[i] == -1, (name, r, m)
                # the near miss differs from its twin in the named record alone
                assert X.records(by[name])[r] == m['word']
                diff = fb.bits[i] ^ fb.bits[own[name]]
                assert np.flatnonzero(diff).tolist() == [m['word']], (name, r)
                assert fb.wordset_size[i] == fb.wordset_size[own[name]] and fm[i] == fm[own[name]]
                if m['kind'] == 'drop':
                    assert int(diff[m['word']]) == 1 << m['bit']
                else:
                    assert bin(int(diff[m['word']])).count('1') == 3 and int(fb.bits[i][m['word']])
    # drops made on a field_bits word, at every edge bit, at record 64 and at a last record
    fld = [i for i in c.pick(kind='drop', src='field')]
    assert {c.meta[i]['bit'] for i in fld} >= set(X.EDGE_BITS)
    assert {c.meta[i]['rec'] for i in fld} >= {64, 127, 128, 129}
    for j in X.EDGE_BITS:
        (i,) = c.pick(kind='need_drop', bit=j)
        assert ref[i] == -1 and fm[i] == fm[own['r0']] & ~np.uint64(1 << j) and fb.wordset_size[i] == 4
    assert ref[own['r0']] == c.index('r0') and not fb.bits[own['r0']].any()


def test_chunks_chain_empty_and_huge(chunks):
    c, ref = chunks
    chain = c.pick(kind='chain')
    assert len(chain) >= 9 and all(ref[i] == -1 for i in chain)
    (e,) = c.pick(kind='empty')
    assert c.files[e] == frozenset() and ref[e] == -1          # no empty template here ...
    p = X.padded(c)
    assert len(p.templates) == 65
    refp = X.reference(p.templates, p.files)
    assert refp[e] == p.index('empty')                          # ... and one here
    spec = X.reference(p.templates, p.special)
    assert spec.tolist() == [-1, p.index('A'), p.index('empty'), -1, p.index('r130')]
    fb, _ = X.encode_files(c.V, c.special)
    assert fb.wordset_size[0] == 2 ** 32 - 1 and not fb.bits[0].any()
    # every template of both legs, fillers included, is some file's answer
    assert set(ref.tolist()) - {-1} == set(range(len(c.templates)))
    assert set(refp.tolist()) - {-1} == set(range(65))


def test_retabled_follows_other_tables(chunks):
    c, ref = chunks
    r = X.retabled(c)
    ref2 = X.reference(r.templates, r.files)
    n = len(c.files)
    assert [t.lf for t in r.templates] == [t.lf for t in c.templates]
    assert (ref2[:n] != ref).sum() >= len(c.templates) - 1       # the old answers go ...
    assert set(ref2[n:].tolist()) == set(range(len(r.templates)))   # ... and every new wordset is found
    assert ref2[c.pick(kind='empty')[0]] == r.index('r0')


# ---- runs --------------------------------------------------------------------------------------

def test_runs_layout(runs):
    c, ref = runs
    T = len(c.templates)
    assert c.V == 640 and T == 300 > X.BLOCK
    pos = _sorted_positions(c)
    assert pos != list(range(T))                                   # key order is not size order
    sizes = [len(t.words) for t in c.templates]
    assert len(_run_of(c, min(sizes))) == 1
    long_run = _run_of(c, X.LONG_SIZE)
    assert len(long_run) == X.LONG_RUN > X.WAVE
    assert [c.templates[t].name for t in long_run] == [f'long{i}' for i in range(X.LONG_RUN)]
    last_run = _run_of(c, max(sizes))
    assert pos[-len(last_run):] == last_run and len(last_run) == 6
    for run in (long_run, last_run, _run_of(c, X.DUP_SIZE), _run_of(c, 41), _run_of(c, 51)):
        assert max(run) - min(run) >= 2 * len(run)                 # scattered key indices
    # identical wordsets first, middle and last within a run: only the first is ever an answer
    dup = _run_of(c, X.DUP_SIZE)
    same = [t for t in dup if c.templates[t].words == c.templates[dup[0]].words]
    assert same == [dup[0], dup[3], dup[6]] and len(dup) == 7
    answered = set(ref.tolist()) - {-1}
    assert answered == set(range(T)) - {dup[3], dup[6]}
    # depth targets: the d-th template of the long run in key order answers the depth-d file
    for d in X.DEPTHS:
        (i,) = c.pick(kind='depth', depth=d)
        assert ref[i] == long_run[d - 1]
    # the template on the last sorted position is an answer, reached past five size-equal others
    assert pos[-1] == c.index('last5') and (ref == pos[-1]).any()
    for r in ('long', 'last', 'min'):
        (i,) = c.pick(kind='run_rejects', run=r)
        assert ref[i] == -1
        assert X.wsize(c.files[i]) == {'long': X.LONG_SIZE, 'last': X.LAST_SIZE, 'min': 3}[r]
    # field words that are vocabulary words, and need masks, occur in runs longer than a wave too
    assert sum(1 for t in long_run if any(X.is_vocab(w) for w in c.templates[t].fields)) >= 10
    assert sum(1 for t in long_run if any(not X.is_vocab(w) for w in c.templates[t].fields)) >= 10


def test_runs_need_groups(runs):
    c, ref = runs
    _, ws, _, need = c.encoded()
    for s in X.GROUP_SIZES:
        run = _run_of(c, s + 1)
        names = [c.templates[t].name for t in run]
        assert names == [f'g{s}_H'] + [f'g{s}_{j}' for j in X.NEED_BITS]       # key order within the run
        lf = c.templates[c.index(f'g{s}_none')].lf
        assert all(c.templates[t].lf == lf for t in run[1:])                  # equal records ...
        assert [int(need[t]) for t in run] == [0] + [1 << j for j in X.NEED_BITS]   # ... unequal need
        assert int(need[c.index(f'g{s}_all')]) == 2 ** 64 - 1 and need[c.index(f'g{s}_none')] == 0
        for j in X.NEED_BITS:
            (i,) = c.pick(kind='need', of=f'g{s}_{j}')
            assert ref[i] == c.index(f'g{s}_{j}')
            (i,) = c.pick(kind='fm_lacks', s=s, bit=j)
            assert ref[i] == -1 and X.wsize(c.files[i]) == s + 64
            _, fm = X.encode_files(c.V, [c.files[i]])
            assert int(fm[0]) == (2 ** 64 - 1) ^ (1 << j)
            (i,) = c.pick(kind='fm_superset', s=s, bit=j)
            assert ref[i] == -1 and X.wsize(c.files[i]) == s + 1
        for kind in ('x_for_field', 'other_field'):
            (i,) = c.pick(kind=kind, s=s)
            assert ref[i] == -1 and X.wsize(c.files[i]) == s + 1
        assert (ref == c.index(f'g{s}_all')).any() and (ref == c.index(f'g{s}_none')).any()


def test_runs_without_masks(runs):
    """field_mask=None: a template with need != 0 cannot match, one with need == 0 still does."""
    c, ref = runs
    _, _, _, need = c.encoded()
    ref0 = X.reference(c.templates, X.strip_fields(c.files))
    hit = ref >= 0
    needs = np.zeros(len(ref), bool)
    needs[hit] = need[ref[hit]] != 0
    assert needs.sum() >= 40 and (hit & ~needs).sum() >= 200
    assert (ref0[needs] == -1).all() and np.array_equal(ref0[~needs], ref[~needs])


def test_placements_put_pending_files_where_they_say(runs):
    c, _ = runs
    sizes = {len(t.words) for t in c.templates}
    P = X.placements(c)
    pend = {k: [i for i, W in enumerate(v) if X.wsize(W) in sizes] for k, v in P.items()}
    assert pend['lane0'] == [0] and len(P['lane0']) == 64
    assert pend['lane63'] == [63] and len(P['lane63']) == 64
    assert pend['all64'] == list(range(64))
    assert len(set(X.reference(c.templates, P['all64']).tolist())) >= 62
    assert pend['partial_last_wave'] == [len(P['partial_last_wave']) - 1] and len(P['partial_last_wave']) % 64
    n = len(P['block_last_wave'])
    assert pend['block_last_wave'] == [192, 255, 256, n - 1] and 256 < n < 320
    ref = X.reference(c.templates, P['mixed_depths'])
    long_run = _run_of(c, X.LONG_SIZE)
    depth = [long_run.index(t) + 1 if t >= 0 else 0 for t in ref.tolist()]
    assert sorted(set(depth)) == [0, 1, 2, 3, 35, 70] and depth.count(1) >= 50
    for k, v in P.items():
        assert (X.reference(c.templates, v) >= 0).sum() == len(pend[k]) - (k == 'mixed_depths'), k
    for n in X.BATCH_SIZES:
        for cc in (c, X.chunks()):
            files = X.sized(cc, n)
            assert len(files) == n and len(set(files)) == min(n, len(set(cc.files)))
            assert (X.reference(cc.templates, files) >= 0).any()


def test_texts_spell_the_files(runs):
    c, _ = runs
    text, off, tl = X.texts_of(c.files)
    vocab, extra = X.vocabulary(c.V)
    assert len(set(vocab + extra)) == c.V + 64 and not (off % 16).any()
    for i in (0, 17, len(c.files) - 1):
        words = bytes(text[off[i]:off[i] + tl[i]]).decode('ascii').split(' ')
        known = {int(w[1:]) for w in words if w[0] == 'v'} | {('f', int(w[1:])) for w in words if w[0] == 'f'}
        assert (frozenset(known), sum(w[0] == 'x' for w in words)) == X.split_file(c.files[i])
        assert len(words) == len(set(words)) and sum(w[0] == 'x' for w in words) <= 192


def test_no_case_is_skipped_or_expected_to_fail():
    here = os.path.dirname(os.path.abspath(__file__))
    pat = re.compile(r'mark\.(skip|xfail)|pytest\.(skip|xfail)|import(or)skip')
    for name in ('exact_cases.py', 'test_exact_cases.py', 'test_gpu_exact_edges.py'):
        with open(os.path.join(here, name)) as fh:
            assert not pat.search(fh.read()), name
