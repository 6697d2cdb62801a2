"""CPU test of the sparse program over the compact (class-count) tile (csrc/dice_program.cpp).

First the layout dice_program_layout reports is checked against the template bitsets in numpy;
then the source dice_program_source_compact generates is compiled for the host under the same
shim and driver as test_program_codegen.py, fed tiles packed here in numpy from the layout, and
its match, matrix and top-k results must equal the C oracle's hash mode bit for bit.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import NormFile, make_files
from tests.test_program_codegen import _check_vs_oracle, _templates_struct

HERE = os.path.dirname(os.path.abspath(__file__))
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')


def compact_source(corpus) -> str:
    from licensee_amd import _native
    lib = _native.load_library()
    keep, t = _templates_struct(corpus)
    n = lib.dice_program_source_compact(ctypes.byref(t), None, 0)
    assert n > 0
    buf = ctypes.create_string_buffer(n + 1)
    assert lib.dice_program_source_compact(ctypes.byref(t), buf, n + 1) == n
    return buf.value.decode()


def compact_layout(corpus):
    """(dest [V], count_base, qperm [quads], quads) of dice_program_layout."""
    from licensee_amd import _native
    lib = _native.load_library()
    keep, t = _templates_struct(corpus)
    quads = lib.dice_program_layout(ctypes.byref(t), None, None, None, 0)
    assert quads >= 1
    dest = np.empty(corpus.n_vocab, np.int32)
    base = ctypes.c_int32(-1)
    qperm = np.empty(quads, np.int32)
    assert lib.dice_program_layout(ctypes.byref(t), dest.ctypes.data, ctypes.addressof(base), qperm.ctypes.data,
                                   quads) == quads
    assert lib.dice_program_layout(ctypes.byref(t), None, None, qperm.ctypes.data, quads - 1) == -1
    return dest, base.value, qperm, quads


def word_matrix(bits: np.ndarray, V: int) -> np.ndarray:
    """[n][w64] uint64 bitsets -> [n][V] bool."""
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder='little')[:, :V].astype(bool)


def compact_pack(bits: np.ndarray, V: int, layout) -> np.ndarray:
    """The compact tile [n_tiles][quads][64] of 4 x uint32 for row-major bitsets, from the layout
    alone: bits moved to their positions, count bytes summed, quads permuted into slot order."""
    dest, base, qperm, quads = layout
    B = word_matrix(bits, V)
    n = B.shape[0]
    tb = np.zeros((n, quads * 128), np.uint8)
    w = np.flatnonzero(dest >= 0)
    tb[:, dest[w]] = B[:, w]
    by = np.packbits(tb, axis=1, bitorder='little')
    n_fields = int((-2 - dest[dest <= -2]).max()) + 1 if (dest <= -2).any() else 0
    for f in range(n_fields):
        cnt = B[:, dest == -2 - f].sum(1)
        assert cnt.max(initial=0) <= 255
        assert not by[:, base + f].any()
        by[:, base + f] = cnt
    nt = (n + 63) // 64
    d32 = np.zeros((nt * 64, quads, 4), np.uint32)
    d32[:n] = by.view(np.uint32).reshape(n, quads, 4)
    t = d32.reshape(nt, 64, quads, 4)[:, :, qperm.astype(np.int64), :]
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3))


def word_classes(corpus):
    """Template-membership column per word ([V][T] bool) and the classes of equal non-zero
    columns (lists of word ids), largest first."""
    cols = word_matrix(corpus.lf_bits, corpus.n_vocab).T
    groups = {}
    for v in range(corpus.n_vocab):
        if cols[v].any():
            groups.setdefault(cols[v].tobytes(), []).append(v)
    return cols, sorted(groups.values(), key=lambda g: (-len(g), g[0]))


def check_layout(corpus, layout):
    dest, base, qperm, quads = layout
    cols, classes = word_classes(corpus)
    placed = cols.any(1)
    # every word of some template is placed, the others stay out of the tile
    assert np.array_equal(dest != -1, placed)
    # bit positions: distinct, inside the tile and below the count bytes
    pos = dest[dest >= 0]
    assert len(set(pos.tolist())) == pos.size
    assert pos.size == 0 or pos.max() < 8 * base
    fields = -2 - dest[dest <= -2]
    n_fields = int(fields.max()) + 1 if fields.size else 0
    assert base % 4 == 0 and base + n_fields <= quads * 16
    for f in range(n_fields):
        ws = np.flatnonzero(dest == -2 - f)
        assert 1 <= ws.size <= 255
        assert (cols[ws] == cols[ws[0]]).all()      # one field, one template set
    assert sorted(qperm.tolist()) == list(range(quads))
    return classes


_built = {}


def run_host(corpus, fb, k, tmp_path, layout=None):
    """(best, ov, score, mov, msc, tki, tks, slow_waves) of the generated compact program run on
    the host over tiles packed from the layout."""
    src = compact_source(corpus)
    layout = layout or compact_layout(corpus)
    quads = layout[3]
    assert f'#define WQ {quads}\n' in src and 'layout=compact' in src
    key = hashlib.sha1(src.encode()).hexdigest()
    d = str(tmp_path)
    exe = _built.get(key)
    if exe is None or not os.path.exists(exe):
        bd = os.path.join(d, 'build')
        os.makedirs(bd)
        with open(os.path.join(bd, 'prog.inc'), 'w') as fh:
            fh.write(src)
        shutil.copy(os.path.join(HERE, 'codegen', 'host_shim.h'), bd)
        exe = os.path.join(bd, 'drv')
        subprocess.run(['g++', '-O1', '-std=c++17', '-w', '-I', bd, '-o', exe,
                        os.path.join(HERE, 'codegen', 'driver.cpp')], check=True)
        _built[key] = exe
    n = fb.n
    npad = ((n + 63) // 64) * 64
    compact_pack(fb.bits, corpus.n_vocab, layout).tofile(os.path.join(d, 'tiles.bin'))
    for name, arr, dt in (('wf', fb.wordset_size, np.uint32), ('len', fb.length, np.int32),
                          ('cc', fb.cc_false_positive, np.uint8)):
        pad = np.zeros(npad, dt)
        pad[:n] = arr
        pad.tofile(os.path.join(d, name + '.bin'))
    out = subprocess.run([exe, d, str(n), str(k)], check=True, capture_output=True, text=True).stdout
    slow_waves = int(out.split('slow_waves ')[1].split()[0])
    T = corpus.lf_bits.shape[0]
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    return (rd('best.out', np.int32), rd('ov.out', np.uint32), rd('score.out', np.float64),
            rd('mov.out', np.uint32).reshape(T, n).T, rd('msc.out', np.float64).reshape(T, n).T,
            rd('tki.out', np.int32).reshape(max(k, 1), n)[:k].T, rd('tks.out', np.float64).reshape(max(k, 1), n)[:k].T,
            slow_waves)


def files_from_words(corpus, word_lists):
    """A FileBatch of files given as vocabulary word-id lists (|W_F| = the word count)."""
    from licensee_amd._native import FileBatch
    B = np.zeros((len(word_lists), corpus.w64 * 64), np.uint8)
    for i, ws in enumerate(word_lists):
        B[i, list(ws)] = 1
    bits = np.packbits(B, axis=1, bitorder='little').view(np.uint64)
    wf = np.array([len(ws) for ws in word_lists], np.uint32)
    return FileBatch(bits, wf, (wf * 6).astype(np.int32), np.zeros(len(word_lists), np.uint8))


def concat(a, b):
    from licensee_amd._native import FileBatch
    return FileBatch(np.concatenate([a.bits, b.bits]), np.concatenate([a.wordset_size, b.wordset_size]),
                     np.concatenate([a.length, b.length]), np.concatenate([a.cc_false_positive, b.cc_false_positive]))


def edge_files(corpus, classes):
    """Every vocabulary bit set (each count field at its capacity); for each of the five largest
    classes the file holding exactly that class and a file holding exactly one of its words."""
    lists = [list(range(corpus.n_vocab))]
    for g in classes[:5]:
        lists += [g, [g[len(g) // 2]]]
    return files_from_words(corpus, lists)


@needs_gxx
def test_vendored_corpus_layout_and_results(tmp_path):
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    templates = License.all(hidden=True, pseudo=False)
    corpus = TemplateCorpus(templates)
    layout = compact_layout(corpus)
    classes = check_layout(corpus, layout)
    # the largest class of the vendored corpus needs more than one count byte
    assert len(classes[0]) > 255
    assert len({int(x) for x in layout[0][classes[0]]}) == (len(classes[0]) + 254) // 255
    assert layout[3] < (corpus.w64 + 1) // 2          # fewer quads than the full bitset
    fb = concat(corpus.intern_files(make_files(templates, 600, 21) + [NormFile(''), NormFile('x' * 10, cc=True)]),
                edge_files(corpus, classes))
    assert fb.n == 602 + 11 and fb.n % 64
    got = run_host(corpus, fb, 5, tmp_path, layout)
    _check_vs_oracle(corpus, fb, got[:-1], 5)
    # the all-words file overlaps every template in all of its words
    assert np.array_equal(got[3][602], corpus.lf_size)


@needs_gxx
def test_tie_clone_corpus(tmp_path):
    """Six templates plus byte-identical clones under later keys: few templates, nearly every
    word in a large class; the clone must still win every tie (dice.rb:39)."""
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    base = [License.find(k) for k in ('apache-2.0', 'bsd-2-clause', 'isc', 'mit', 'mpl-2.0', 'unlicense')]
    clones = [License('zz-' + l.key, {'title': l.title}, content_normalized=l.content_normalized(),
                      alt_segments=l.spdx_alt_segments()) for l in base]
    templates = sorted(base + clones, key=lambda l: l.key)
    corpus = TemplateCorpus(templates)
    layout = compact_layout(corpus)
    classes = check_layout(corpus, layout)
    assert (layout[0] <= -2).sum() > corpus.n_vocab // 2
    fb = concat(corpus.intern_files(make_files(templates, 300, 5) + [NormFile('')]), edge_files(corpus, classes))
    got = run_host(corpus, fb, 3, tmp_path, layout)
    _check_vs_oracle(corpus, fb, got[:-1], 3)
    keys = [t.key for t in templates]
    matched = got[0][got[0] >= 0]
    assert len(matched) > 50 and all(keys[b].startswith('zz-') for b in matched)


@needs_gxx
def test_mixed_fast_slow_waves(tmp_path):
    """Waves mixing fast lanes with lanes outside the fast envelope take the IEEE-double path
    over bit and count dwords alike; the other waves keep the exact rational path."""
    from licensee_amd._native import FileBatch
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from tests.helpers import widen_lanes
    templates = License.all(hidden=True, pseudo=False)
    corpus = TemplateCorpus(templates)
    fb0 = corpus.intern_files(make_files(templates, 1024, 8))
    fb, idx = widen_lanes(fb0, seed=3)
    wf, ln = fb.wordset_size.copy(), fb.length.copy()
    wf[512:], ln[512:] = fb0.wordset_size[512:], fb0.length[512:]
    fb = FileBatch(fb.bits, wf, ln, fb.cc_false_positive)
    got = run_host(corpus, fb, 5, tmp_path)
    assert got[-1] == 8, got[-1]
    _check_vs_oracle(corpus, fb, got[:-1], 5)


@needs_gxx
def test_corpus_outside_fast_envelope(tmp_path):
    """CORPUS_FAST 0: every wave takes the IEEE-double path over the compact tile."""
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from tests.helpers import outside_fast_envelope
    templates = License.all(hidden=True, pseudo=False)
    corpus = outside_fast_envelope(TemplateCorpus(templates))
    assert '#define CORPUS_FAST 0' in compact_source(corpus)
    fb = TemplateCorpus(templates).intern_files(make_files(templates, 300, 12) + [NormFile('')])
    got = run_host(corpus, fb, 4, tmp_path)
    assert got[-1] == (fb.n + 63) // 64
    _check_vs_oracle(corpus, fb, got[:-1], 4)
    assert (got[2] > 100.0).any()
