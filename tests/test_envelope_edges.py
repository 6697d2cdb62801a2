"""CPU side of the envelope-edge cases (tests/envelope_cases.py): the inputs are valid and the host
forms agree, so a mismatch on the device (tests/test_gpu_envelope_edges.py) is the kernel's.

  * the C oracle's hash mode equals the plain Python reference on every corpus and grid: best,
    overlap, score (thresholds 0 and 98) and the full matrix;
  * the generated program, compiled for the host in both tile layouts, equals the reference on the
    2,047 / 2,048-word twins, the base = 200 corpus and the near-tie corpus: match, matrix, top-4;
  * the generated source carries NARROW_MUL and CORPUS_FAST as the twins prescribe, and post_fast's
    conditions (restated here) flip where they do.
PACK_STRIDE is in the device-only part of the compact source; the GPU test pins it through results.
"""
import shutil

import numpy as np
import pytest

from tests import envelope_cases as E

needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')

CASES = {
    'lf2047': lambda: E.lf_case(2047),
    'lf2048': lambda: E.lf_case(2048),
    'lf2047_base200': lambda: E.lf_case(2047, variant='base200'),
    'lf2047_len20': lambda: E.lf_case(2047, variant='len20'),
    'lf2047_T65': lambda: E.lf_case(2047, 65),
    'lf2048_T65': lambda: E.lf_case(2048, 65),
    'base18_in': lambda: E.base18_case(True),
    'base18_out': lambda: E.base18_case(False),
    'pack8128': lambda: E.pack_case(8128),
    'pack8129': lambda: E.pack_case(8129),
    'post_in': lambda: E.post_case('in'),
    'post_lf': lambda: E.post_case('lf'),
    'post_slack': lambda: E.post_case('slack'),
    'post_base65535': lambda: E.post_case('base65535'),
    'post_base65536': lambda: E.post_case('base65536'),
    'ties': lambda: E.tie_case(4),
    'ties_T65': lambda: E.tie_case(65),
}
LIMIT = {'base18_in': 130, 'base18_out': 130, 'post_in': 130, 'post_lf': 130, 'post_slack': 130,
         'post_base65535': 130, 'post_base65536': 130}


def files_of(name, case):
    if name.startswith('ties'):
        return E.tie_files(case)[0]
    return E.grid(case, limit=LIMIT.get(name))


def _oracle(c):
    from oracle.native import OracleScorer
    return OracleScorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab)


def same(got, exp, where):
    for j, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape and np.array_equal(g, e), (where, j, np.flatnonzero((g != e).reshape(len(g), -1).any(1))[:8])


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_equals_reference(name):
    case = CASES[name]()
    c, fb = case.corpus, files_of(name, case)
    ref, orc = E.Reference(c, fb), _oracle(c)
    for thr in (0.0, 98.0):
        same(orc.match(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive, thr, nthreads=4, mode=0),
             ref.match(thr), (name, thr))
    same(orc.matrix(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive, nthreads=4), ref.matrix(), (name, 'matrix'))


def test_grid_covers_the_cuts():
    fb = E.grid(E.lf_case(2047))
    assert fb.n == 350
    wf, ln = fb.wordset_size.astype(np.int64), fb.length.astype(np.int64)
    for v in E.WF_EDGES:
        assert (wf == v).any()
    for v in E.LEN_EDGES:
        assert (ln == v).any()
    # the fast path's largest product: 2,047 shared words against |W_F| = 2^20 - 1, len_F = 2^21 - 1
    ref = E.Reference(E.lf_case(2047).corpus, fb)
    # in the wave whose 64 files are all inside the envelope
    big = max(ref.ov[i][t] * ref.den[i][u] for i in range(64) for t in range(ref.T) for u in range(ref.T))
    assert 2 ** 31 < big < 2 ** 32


def test_tie_files_are_what_they_claim():
    case = E.tie_case(4)
    fb, meta = E.tie_files(case)
    assert sum(1 for m in meta if m[2] == +1) == sum(1 for m in meta if m[2] == -1) == 100
    assert sum(1 for m in meta if m[2] == 0) == 50
    ref = E.Reference(case.corpus, fb)
    for i, (a, b, s) in enumerate(meta):
        first, second = ref.ranked(i)[:2]
        assert [first, second] == ([a, b] if s > 0 else [b, a]), i
        cross = ref.ov[i][a] * ref.den[i][b] - ref.ov[i][b] * ref.den[i][a]
        assert cross == s and min(ref.den[i][a], ref.den[i][b]) > 1 << 20
        assert (ref.score[i][a] == ref.score[i][b]) == (s == 0)
        assert E.is_fast(int(fb.wordset_size[i]), int(fb.length[i]))
    # the same files on the 65-template corpus rank the same two templates
    case65 = E.tie_case(65)
    fb65, meta65 = E.tie_files(case65)
    ref65 = E.Reference(case65.corpus, fb65)
    pos = case65.corpus.tie_pos
    assert meta65 == meta
    assert all(ref65.ranked(i)[:2] == [pos[t] for t in ref.ranked(i)[:2]] for i in range(fb.n))


def _post_fast(c):
    base = c.lf_size.astype(np.int64) - c.fields_set_size.astype(np.int64)
    return bool(((c.lf_size < 1 << 11) & (base >= 1) & (base < 1 << 18) & (c.length >= 0) & (c.length < 1 << 20) &
                 (200 * c.lf_size.astype(np.int64) < 1024 * base)).all())


@pytest.mark.parametrize('name', ['lf2047', 'lf2048', 'lf2047_base200', 'lf2047_len20', 'base18_in', 'base18_out',
                                  'pack8128', 'pack8129', 'ties'])
def test_generated_source_defines(name):
    from tests.test_program_codegen import generated_source
    from tests.test_program_compact_codegen import compact_source
    case = CASES[name]()
    for src in (generated_source(case.corpus), compact_source(case.corpus)):
        for key in ('NARROW_MUL', 'CORPUS_FAST'):
            lines = [l for l in src.splitlines() if l.startswith(f'#define {key} ')]
            assert lines == [f'#define {key} {case.expect[key.lower()]}'], (name, key, lines)


def test_post_fast_flips_with_the_twins():
    assert _post_fast(E.lf_case(2047, 65).corpus) and not _post_fast(E.lf_case(2048, 65).corpus)
    assert not _post_fast(E.lf_case(2047, 65, 'base200').corpus) and not _post_fast(E.lf_case(2047, 65, 'len20').corpus)
    assert _post_fast(E.tie_case(65).corpus)


@needs_gxx
@pytest.mark.parametrize('layout', ['compact', 'bits'])
@pytest.mark.parametrize('name', ['lf2047', 'lf2048', 'lf2047_base200', 'ties'])
def test_host_program_equals_reference(name, layout, tmp_path):
    from tests import test_program_codegen as bits_form
    from tests import test_program_compact_codegen as compact_form
    case = CASES[name]()
    c, fb = case.corpus, files_of(name, case)
    ref = E.Reference(c, fb)
    if layout == 'compact':
        got = compact_form.run_host(c, fb, 4, tmp_path)
    else:
        got = bits_form.run_host(c, fb, 4, tmp_path, with_votes=True)
    same(got[0:3], ref.match(98.0), (name, layout, 'match'))
    same(got[3:5], ref.matrix(), (name, layout, 'matrix'))
    same(got[5:7], ref.topk(4), (name, layout, 'topk'))
    waves = (fb.n + 63) // 64
    fast = [E.is_fast(int(w), int(l)) for w, l in zip(fb.wordset_size, fb.length)]
    slow_waves = sum(1 for a in range(0, fb.n, 64) if not all(fast[a:a + 64]))
    assert got[7] == (slow_waves if case.expect['corpus_fast'] else waves)
    if name != 'ties':
        assert 0 < slow_waves < waves


@needs_gxx
@pytest.mark.parametrize('layout', ['compact', 'bits'])
def test_wave_vote_one_step_past_each_cut(layout, tmp_path):
    """|W_F| = 2^20 or len_F = 2^21 in one lane: that wave, and no other, leaves the fast body."""
    from tests import test_program_codegen as bits_form
    from tests import test_program_compact_codegen as compact_form
    case = CASES['lf2047']()
    fb, slow_waves = E.cut_waves(files_of('lf2047', case))
    ref = E.Reference(case.corpus, fb)
    if layout == 'compact':
        got = compact_form.run_host(case.corpus, fb, 4, tmp_path)
    else:
        got = bits_form.run_host(case.corpus, fb, 4, tmp_path, with_votes=True)
    assert got[7] == slow_waves
    same(got[0:3], ref.match(98.0), (layout, 'match'))
    same(got[3:5], ref.matrix(), (layout, 'matrix'))
    same(got[5:7], ref.topk(4), (layout, 'topk'))
