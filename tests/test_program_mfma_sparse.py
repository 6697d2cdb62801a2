"""Row assignment, word grouping and fragment liveness of the matrix-core accumulate stage
(dice_program_mfma_rows, csrc/dice_program_gen.cpp: assign_rows, group_bits), checked on the host.

The device keeps the templates in two 32-row blocks chosen so that, with the bit region ordered
[words of block 0 only | of both | of block 1 only] along the K-steps, many (K-step, block) fragments
are all zero; the kernel reads and multiplies only the live ones. Checked here: the row map is a
permutation with pads, a fragment is flagged dead iff it is all zero in the canonical table gathered
through the map, the numpy product over the live fragments alone still gives the oracle's overlaps,
the live count is what the grouping and the padding rule predict, and the generated prologue holds
exactly two matrix instructions per live fragment."""
import ctypes

import numpy as np
import pytest

from tests.helpers import ArrayCorpus
from tests.test_program_codegen import _templates_struct
from tests.test_program_compact_codegen import (compact_layout, compact_pack, compact_source, concat, edge_files,
                                                files_from_words, word_classes, word_matrix)
from tests.test_program_mfma_tables import E2M1, FILE_CODE, _vendored, mfma_tables, template_values


def mfma_rows(corpus, dims):
    """(rows [64] template per device row or -1, live [K][blocks] uint8, live count)."""
    from licensee_amd import _native
    lib = _native.load_library()
    keep, t = _templates_struct(corpus)
    rows = np.full(64, -7, np.int32)
    live = np.full(dims[0] * dims[1], 9, np.uint8)
    n = lib.dice_program_mfma_rows(ctypes.byref(t), rows.ctypes.data, live.ctypes.data, live.size)
    assert lib.dice_program_mfma_rows(ctypes.byref(t), None, None, 0) == n
    if live.size:
        assert lib.dice_program_mfma_rows(ctypes.byref(t), None, live.ctypes.data, live.size - 1) == -1
    return rows, live.reshape(dims[0], dims[1]), n


def kstep_sequence(bit_dwords, ksteps):
    """The bit region's dwords in K-step order and the K-step of each: K-step s multiplies dword
    8 (s // 4) + s % 4 (lane half 0) and that + 4 (half 1), where they exist."""
    seq = [(8 * (s // 4) + 4 * h + s % 4, s) for s in range(ksteps) for h in (0, 1)]
    seq = [(dw, s) for dw, s in seq if dw < bit_dwords]
    return np.array([dw for dw, _ in seq]), np.array([s for _, s in seq])


def predicted_live(a, both, b, bit_dwords, ksteps):
    """Live fragments of [a | pad | both | b] laid along the K-step sequence, by marking: block 0 is
    live where a word of the first two groups sits, block 1 where one of the last two does. The
    padding rule: 0 <= pad <= the bit region's unused bits, the fewest live fragments win."""
    ks_of = kstep_sequence(bit_dwords, ksteps)[1]
    slack = 32 * bit_dwords - (a + both + b)
    best = None
    for pad in range(slack + 1):
        pos = np.concatenate([np.arange(a), a + pad + np.arange(both + b)])
        ks = ks_of[pos // 32]
        n = np.unique(ks[:a + both]).size + np.unique(ks[a:]).size
        best = n if best is None else min(best, n)
    return best


def check_sparse(corpus, fb):
    """Returns (live count, fragments) of the corpus's stage, (0, 0) where it has none."""
    from oracle.native import OracleScorer
    layout = compact_layout(corpus)
    dest, base, qperm, quads = layout
    dims, frag, fmap = mfma_tables(corpus)
    T, V = corpus.lf_bits.shape[0], corpus.n_vocab
    if frag is None:
        rows, live, n_live = mfma_rows(corpus, [0, 0])
        assert n_live == 0
        return 0, 0
    ks, nt = dims[0], dims[1]
    rows, live, n_live = mfma_rows(corpus, dims)
    assert mfma_rows(corpus, dims)[0].tolist() == rows.tolist() and np.array_equal(mfma_rows(corpus, dims)[1], live)
    # the row map: every template once, pads -1, at most 32 per block, nothing past the blocks in use
    assert sorted(rows[rows >= 0].tolist()) == list(range(T)) and (rows[rows < 0] == -1).all()
    assert (rows[32 * nt:] == -1).all()
    if nt == 1:
        assert rows[:T].tolist() == list(range(T))
    # dead iff all zero in the canonical table gathered through the map
    tv = template_values(frag)                                                  # [K][32 nt][64], row = template
    gathered = np.where((rows[:32 * nt] >= 0)[None, :, None], tv[:, np.maximum(rows[:32 * nt], 0), :], 0.0)
    nonzero = gathered.reshape(ks, nt, 32 * 64).any(2)
    assert np.array_equal(nonzero, live.astype(bool)) and n_live == int(live.sum())
    # the product over the live fragments only
    tiles = compact_pack(fb.bits, V, layout)
    trows = tiles.transpose(0, 2, 1, 3).reshape(-1, quads * 4)[:fb.n]
    tb = np.unpackbits(np.ascontiguousarray(trows).view(np.uint8), axis=1, bitorder='little')
    k_of = (np.arange(64) % 32) // 8
    fval = np.where(fmap[None] >= 0, tb[:, np.maximum(fmap, 0)], 1) * E2M1[FILE_CODE[k_of]][None, None, :]
    per_step = np.einsum('nse,sre->nsr', fval, gathered)                        # [n][K][device row]
    per_step *= np.repeat(live, 32, axis=1)[None]                               # a dead fragment is never multiplied
    by_row = per_step.sum(1)
    got = np.zeros((fb.n, T))
    got[:, rows[rows >= 0]] = by_row[:, np.flatnonzero(rows >= 0)]
    W, L = word_matrix(fb.bits, V), word_matrix(corpus.lf_bits, V)
    bit_words, counted = np.flatnonzero(dest >= 0), np.flatnonzero(dest <= -2)
    bit_part = W[:, bit_words].astype(np.int64) @ L[:, bit_words].T.astype(np.int64)
    count_part = W[:, counted].astype(np.int64) @ L[:, counted].T.astype(np.int64)
    assert np.array_equal(got, bit_part)
    orc = OracleScorer(corpus.lf_bits, corpus.lf_size, corpus.fields_set_size, corpus.length_slack, corpus.length,
                       corpus.is_cc, corpus.n_vocab)
    mov, _ = orc.matrix(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive)
    assert np.array_equal(got.astype(np.int64) + count_part, mov.astype(np.int64))
    # grouping and live count
    if nt == 2:
        in0 = L[rows[:32][rows[:32] >= 0]][:, bit_words].any(0)
        in1 = L[rows[32:][rows[32:] >= 0]][:, bit_words].any(0)
        group = np.where(in0 & in1, 1, np.where(in0, 0, 2))
        a, both, b = [int((group == g).sum()) for g in range(3)]
        lower = -(-(a + both) // 64) - (-(both + b) // 64)
        want = predicted_live(a, both, b, dims[2], ks)
        print(f'T={T}: split {int((rows[:32] >= 0).sum())}/{int((rows[32:] >= 0).sum())}, words a={a} both={both} b={b}, '
              f'live {n_live} of {ks * nt} (no padding could give less than {lower})')
        assert lower <= n_live == want
        # a stable partition along the K-step sequence: groups in order, vocabulary order inside each
        seq = kstep_sequence(dims[2], ks)[0]
        at = np.empty(dims[2], np.int64)
        at[seq] = np.arange(seq.size)
        lp = 32 * at[dest[bit_words] >> 5] + (dest[bit_words] & 31)
        order = np.argsort(lp)
        assert (np.diff(group[order]) >= 0).all()
        for g in range(3):
            assert (np.diff(bit_words[order][group[order] == g]) > 0).all()
    else:
        assert (np.diff(dest[bit_words]) > 0).all()                              # one block: the order is untouched
        assert n_live == int((fmap >= 0).any(1).sum())
    return n_live, ks * nt


def check_source(corpus, monkeypatch, n_live):
    """Same text twice; 2 matrix instructions and one fragment read per live fragment in the prologue."""
    monkeypatch.setenv('DICE_PROG_MATCH', 'mfma')
    src = compact_source(corpus)
    assert compact_source(corpus) == src
    if n_live == 0:
        assert 'FILE_PROLOGUE_MFMA' not in src
        return
    pro = src[src.index('#define FILE_PROLOGUE_MFMA'):]
    pro = pro[:pro.index('\n\n')]
    assert pro.count('MFMA44(') == 2 * n_live and pro.count('frag8(tfrag[') == n_live
    assert f'live={n_live} ' in src


def test_vendored_corpus(monkeypatch):
    c, fb = _vendored()
    n_live, n_frag = check_sparse(c, fb)
    print('vendored corpus: live fragments', n_live, 'of', n_frag)
    assert 0 < n_live < n_frag
    check_source(c, monkeypatch, n_live)


@pytest.mark.parametrize('n_templates', [1, 16, 17, 33, 64])
def test_small_corpora(n_templates, monkeypatch):
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.synth import SyntheticCorpus
    from tests.test_gpu_corpus_sizes import corpus_of
    c = TemplateCorpus(corpus_of(n_templates))
    fb = SyntheticCorpus(c).generate(0, 70, seed=11, nthreads=2)
    fb = concat(fb, edge_files(c, word_classes(c)[1]))
    n_live, n_frag = check_sparse(c, fb)
    assert (n_live == 0) == (n_templates == 1)
    check_source(c, monkeypatch, n_live)


def test_corpus_without_count_fields(monkeypatch):
    T, V = 8, 255
    member = ((np.arange(1, V + 1)[None, :] >> np.arange(T)[:, None]) & 1).astype(np.uint8)
    pad = np.zeros((T, 256), np.uint8)
    pad[:, :V] = member
    size = member.sum(1).astype(np.uint32)
    c = ArrayCorpus(np.packbits(pad, axis=1, bitorder='little').view(np.uint64), size, np.ones(T, np.uint32),
                    np.full(T, 5, np.int32), (size * 6).astype(np.int32), np.zeros(T, np.uint8), V)
    rng = np.random.default_rng(2)
    lists = [list(range(V)), []] + [np.flatnonzero(rng.random(V) < rng.random()).tolist() for _ in range(40)]
    n_live, n_frag = check_sparse(c, files_from_words(c, lists))
    assert n_live == n_frag == 4
    check_source(c, monkeypatch, n_live)
