"""Tables of the sparse program's matrix-core accumulate stage (dice_program_mfma_tables,
csrc/dice_program.cpp), checked on the host.

The stage scores the compact tile's bit region as a binary matrix product on e2m1 operands, K-step
by K-step of 64 elements. It is exact iff every bit of the region sits in exactly one file-side
element, every other element meets zero template elements, and the paired e2m1 values multiply to
1.0 for a shared bit. A numpy restatement of the product -- nibbles decoded, multiplied, summed per
K-step -- over tiles packed with compact_pack must give the bit-region part of the oracle's
overlap matrix bit for bit. The generated device source is also compiled for its resource usage:
no scratch, no spills, 3 waves per SIMD; the code object the runtime compiler makes is checked too."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests.helpers import ArrayCorpus, NormFile, make_files
from tests.test_program_codegen import _templates_struct
from tests.test_program_compact_codegen import (compact_layout, compact_pack, compact_source, concat, edge_files,
                                                files_from_words, word_classes, word_matrix)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
FILE_CODE = np.array([1, 2, 4, 4])          # widen_a: nibble code of a set bit in fragment dword k


def mfma_tables(corpus):
    """(dims [K-steps, template tiles, bit dwords, pays], frag [K][tiles][64][4] u32, map [K][64] i32), or
    (dims, None, None) for a corpus the stage cannot take."""
    from licensee_amd import _native
    lib = _native.load_library()
    keep, t = _templates_struct(corpus)
    dims = (ctypes.c_int32 * 4)()
    n = lib.dice_program_mfma_tables(ctypes.byref(t), ctypes.addressof(dims), None, 0, None, 0)
    assert n >= 0
    if n == 0:
        return list(dims), None, None
    ks, nt = dims[0], dims[1]
    assert n == ks * nt * 256
    frag = np.empty(n, np.uint32)
    fmap = np.empty(ks * 64, np.int32)
    assert lib.dice_program_mfma_tables(ctypes.byref(t), None, frag.ctypes.data, n, fmap.ctypes.data, ks * 64) == n
    assert lib.dice_program_mfma_tables(ctypes.byref(t), None, frag.ctypes.data, n - 1, None, 0) == -1
    assert lib.dice_program_mfma_tables(ctypes.byref(t), None, None, 0, fmap.ctypes.data, ks * 64 - 1) == -1
    return list(dims), frag.reshape(ks, nt, 64, 4), fmap.reshape(ks, 64)


def tile_bit_of(layout):
    """Layout bit position -> bit of the resident tile row (slot order)."""
    dest, base, qperm, quads = layout
    slot_of = np.empty(quads, np.int64)
    slot_of[qperm] = np.arange(quads)
    p = np.arange(quads * 128)
    d = p >> 5
    return 32 * (4 * slot_of[d >> 2] + (d & 3)) + (p & 31)


def template_values(frag):
    """[K][T padded][64 elements] e2m1 values of the template fragments: element 32 h + 8 k + i of
    template 32 j + r is nibble i of dword k of lane 32 h + r."""
    ks, nt = frag.shape[:2]
    nib = (frag[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & 15      # [K][j][lane][k][i]
    val = E2M1[nib].reshape(ks, nt, 2, 32, 32)                                  # [K][j][h][r][e]
    return val.transpose(0, 1, 3, 2, 4).reshape(ks, nt * 32, 64)


def check_corpus(corpus, fb):
    from oracle.native import OracleScorer
    layout = compact_layout(corpus)
    dest, base, qperm, quads = layout
    dims, frag, fmap = mfma_tables(corpus)
    T, V = corpus.lf_bits.shape[0], corpus.n_vocab
    bit_words = np.flatnonzero(dest >= 0)
    if frag is None:
        assert bit_words.size == 0 and dims[2] == 0
        return dims
    ks, nt = dims[0], dims[1]
    assert nt == (T + 31) // 32 and dims[2] == (bit_words.size + 31) // 32 and ks == 4 * ((dims[2] + 7) // 8)
    # every bit-region position in exactly one file-side element
    carried = fmap[fmap >= 0]
    want = tile_bit_of(layout)[dest[bit_words]]
    assert carried.size == want.size and np.array_equal(np.sort(carried), np.sort(want))
    # elements that carry no bit pair with zero template elements; padded templates are zero
    tv = template_values(frag)
    assert not tv[:, T:, :].any()
    assert not tv.transpose(0, 2, 1)[fmap < 0].any()
    assert set(np.unique(tv)) <= {0.0, 0.5, 1.0, 2.0}
    # the product: file-side elements from the packed tiles (an element that carries no bit is given
    # the value of a set bit: only its zero template elements may cancel it)
    tiles = compact_pack(fb.bits, V, layout)                                    # [tiles][quads][64][4]
    rows = tiles.transpose(0, 2, 1, 3).reshape(-1, quads * 4)[:fb.n]
    tb = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder='little')
    k_of = (np.arange(64) % 32) // 8
    fval = np.where(fmap[None] >= 0, tb[:, np.maximum(fmap, 0)], 1) * E2M1[FILE_CODE[k_of]][None, None, :]
    per_step = np.einsum('nse,ste->nst', fval, tv)                              # summed per K-step, in float
    got = per_step.sum(1)[:, :T]
    assert np.array_equal(got, np.rint(got))
    # the oracle's overlap matrix = bit-region part + count-field part
    W, L = word_matrix(fb.bits, V), word_matrix(corpus.lf_bits, V)
    counted = np.flatnonzero(dest <= -2)
    count_part = W[:, counted].astype(np.int64) @ L[:, counted].T.astype(np.int64)
    bit_part = W[:, bit_words].astype(np.int64) @ L[:, bit_words].T.astype(np.int64)
    assert np.array_equal(got.astype(np.int64), bit_part)
    orc = OracleScorer(corpus.lf_bits, corpus.lf_size, corpus.fields_set_size, corpus.length_slack, corpus.length,
                       corpus.is_cc, corpus.n_vocab)
    mov, _ = orc.matrix(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive)
    assert np.array_equal(got.astype(np.int64) + count_part, mov.astype(np.int64))
    return dims


def _vendored():
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    templates = License.all(hidden=True, pseudo=False)
    c = TemplateCorpus(templates)
    fb = concat(c.intern_files(make_files(templates, 150, 21) + [NormFile('')]), edge_files(c, word_classes(c)[1]))
    return c, fb


def test_vendored_corpus_tables():
    c, fb = _vendored()
    dims = check_corpus(c, fb)
    assert dims[1] == 2 and dims[2] % 8 != 0 and dims[3] == 1     # 47 templates pad to 64; the stage pays


@pytest.mark.parametrize('n_templates', [1, 16, 17, 33, 64])
def test_small_corpora_tables(n_templates):
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.synth import SyntheticCorpus
    from tests.test_gpu_corpus_sizes import corpus_of
    c = TemplateCorpus(corpus_of(n_templates))
    fb = SyntheticCorpus(c).generate(0, 70, seed=11, nthreads=2)
    fb = concat(fb, edge_files(c, word_classes(c)[1]))
    dims = check_corpus(c, fb)
    if n_templates == 1:
        assert dims[2] == 0           # one template: one class, all count bytes, no bit region


def test_corpus_without_count_fields():
    T, V = 8, 255
    member = ((np.arange(1, V + 1)[None, :] >> np.arange(T)[:, None]) & 1).astype(np.uint8)
    pad = np.zeros((T, 256), np.uint8)
    pad[:, :V] = member
    size = member.sum(1).astype(np.uint32)
    c = ArrayCorpus(np.packbits(pad, axis=1, bitorder='little').view(np.uint64), size, np.ones(T, np.uint32),
                    np.full(T, 5, np.int32), (size * 6).astype(np.int32), np.zeros(T, np.uint8), V)
    rng = np.random.default_rng(2)
    lists = [list(range(V)), []] + [np.flatnonzero(rng.random(V) < rng.random()).tolist() for _ in range(40)]
    dims = check_corpus(c, files_from_words(c, lists))
    assert dims[:3] == [4, 1, 8]
    assert (compact_layout(c)[0] >= 0).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
def test_generated_matrix_kernel_resources(tmp_path, monkeypatch):
    """Compile-only, offline compiler: dice_prog_match_mfma of the vendored corpus's program uses no
    scratch, spills nothing and fits 3 waves per SIMD (12-wave workgroups). The widening of one wave
    overlaps the matrix work of the SIMD's others."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    monkeypatch.setenv('DICE_PROG_MATCH', 'mfma')
    c, _ = _vendored()
    src = compact_source(c)
    assert 'dice_prog_match_mfma' in src and '#define MWK 12' in src and 'dice_prog_matrix4_mfma' not in src
    path = tmp_path / 'prog.hip'
    path.write_text('#include <hip/hip_runtime.h>\n' + src)
    r = {r['name']: r for r in kernel_resources(str(path))}['dice_prog_match_mfma']
    print('offline: VGPRs', r['VGPRs'], 'occupancy', r['Occupancy [waves/SIMD]'])
    assert r['ScratchSize [bytes/lane]'] == '0' and r['VGPRs Spill'] == '0' and r['SGPRs Spill'] == '0', r
    assert int(r['Occupancy [waves/SIMD]']) >= 3, r
    # the switch's other leg generates no matrix-core code
    monkeypatch.setenv('DICE_PROG_MATCH', 'valu')
    assert '_mfma' not in compact_source(c)


READELF = '/opt/rocm/llvm/bin/llvm-readelf'


@pytest.mark.skipif(not os.path.exists(READELF), reason='llvm-readelf not present')
def test_runtime_compiled_matrix_kernel_resources(tmp_path, monkeypatch):
    """The code object that ships is compiled by hiprtc, whose code differs from the offline
    compiler's for this source (dice_program.cpp, MFMA44). Its metadata for dice_prog_match_mfma:
    no scratch, no VGPR spills, at most 168 VGPRs (3 waves per SIMD), the fragments' 48 KiB of LDS.
    SGPRs written to VGPR lanes (sgpr_spill_count; they cost no scratch) are printed, not bounded."""
    import re
    import subprocess
    from licensee_amd import _native
    monkeypatch.setenv('DICE_PROG_MATCH', 'mfma')
    monkeypatch.setenv('DICE_CACHE_DIR', str(tmp_path))
    c, _ = _vendored()
    keep, t = _templates_struct(c)
    buf = ctypes.create_string_buffer(4096)
    assert _native.load_library().dice_precompile(ctypes.byref(t), buf, 4096) == 0
    notes = subprocess.run([READELF, '--notes', buf.value.decode()], capture_output=True, text=True, check=True).stdout
    kernels = {}
    for block in notes.split('- .agpr_count')[1:]:
        f = dict(re.findall(r'\.(\w+):\s+(\S+)', block))
        kernels[f['name']] = f
    k = kernels['dice_prog_match_mfma']
    print('hiprtc: VGPRs', k['vgpr_count'], 'SGPR spills', k['sgpr_spill_count'])
    assert k['private_segment_fixed_size'] == '0' and k['vgpr_spill_count'] == '0', k
    assert int(k['vgpr_count']) <= 168 and k['max_flat_workgroup_size'] == '768', k
    dims = mfma_tables(c)[0]
    assert int(k['group_segment_fixed_size']) == dims[0] * dims[1] * 1024
