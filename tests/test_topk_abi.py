"""CPU tests of the top-k-only path (dice_topk / dice_batch_topk, include/licensee_dice.h): the
C-ABI's symbols and argument codes, the generated dice_prog_topk4 / dice_prog_topk16 kernels run on
the host against the oracle, and the resources of every top-k kernel against its matrix counterpart.

The path ranks each file's k closest templates (Dice#matches_by_similarity cut to k entries, what
`licensee detect` prints) exactly as the matrix call ranks them, without the N x T matrix.
"""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.test_program_codegen import _templates_struct, generated_source, source_qperm, tile_pack
from tests.test_program_compact_codegen import compact_layout, compact_pack, compact_source

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = '/opt/rocm/bin/hipcc'
READELF = '/opt/rocm/llvm/bin/llvm-readelf'
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')

DICE_E_ARG, DICE_E_STATE = -1, -4
NEW_SYMBOLS = ('dice_topk', 'dice_topk_sharded', 'dice_batch_topk', 'dice_batch_download_topk',
               'dice_batch_matrix_bytes')


def expected_topk(c, fb, k, nthreads=8):
    """The oracle's ranking: per file the k best potential matches (CC templates are none for a
    flagged file, dice.rb:17-25), descending score, the later template first among exact ties
    (dice.rb:39), -1 / -1.0 padding. Returns (index [n][k], score [n][k], full score matrix)."""
    from oracle.native import OracleScorer
    T = c.lf_bits.shape[0]
    orc = OracleScorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab)
    _, emsc = orc.matrix(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive, nthreads=nthreads)
    filt = fb.cc_false_positive.astype(bool)[:, None] & c.is_cc.astype(bool)[None, :]
    key = np.where(filt, -np.inf, emsc)
    order = np.lexsort((-np.arange(T)[None, :].repeat(fb.n, 0), -key), axis=1)[:, :k]
    valid = np.take_along_axis(~filt, order, 1)
    idx = np.full((fb.n, k), -1, np.int32)
    sco = np.full((fb.n, k), -1.0, np.float64)
    idx[:, :order.shape[1]] = np.where(valid, order, -1)
    sco[:, :order.shape[1]] = np.where(valid, np.take_along_axis(emsc, order, 1), -1.0)
    return idx, sco, emsc


def assert_topk(got, exp, where=''):
    tki, tks = got
    assert tki.dtype == np.int32 and tks.dtype == np.float64
    assert np.array_equal(tki, exp[0]), where
    assert np.array_equal(tks, exp[1]), where    # bit-exact: == on doubles


def tie_rate(exp):
    """Share of files whose first two ranked scores are exactly equal."""
    idx, sco = exp[:2]
    return float(((idx[:, 1] >= 0) & (sco[:, 0] == sco[:, 1])).mean()) if idx.shape[1] > 1 else 0.0


def test_new_symbols_exported():
    from licensee_amd import _native
    lib = _native.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'licensee_dice.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\(', hdr), name
    assert 'detect.rb:96-106' in hdr.split('int dice_batch_topk')[0].rsplit('*/', 2)[-2]


@pytest.mark.parametrize('k', [0, -1, 17, 3])
def test_null_and_k_codes(k):
    """NULL batch / context: DICE_E_ARG whatever k is; k outside [1, DICE_TOPK_MAX] is reported
    as such before anything is dereferenced (dice_last_error names the cause)."""
    from licensee_amd import _native
    lib = _native.load_library()
    last = lambda: lib.dice_last_error().decode()
    bad_k = not 1 <= k <= _native.DICE_TOPK_MAX
    idx = np.zeros(16, np.int32)
    sco = np.zeros(16, np.float64)
    files = _native._Files(0, None, None, None, None)
    calls = (
        lambda: lib.dice_batch_topk(None, k, None),
        lambda: lib.dice_batch_download_topk(None, k, idx.ctypes.data, sco.ctypes.data, None),
        lambda: lib.dice_topk(None, ctypes.byref(files), k, idx.ctypes.data, sco.ctypes.data),
        lambda: lib.dice_topk_sharded(None, 1, ctypes.byref(files), 0, k, idx.ctypes.data, sco.ctypes.data),
    )
    for call in calls:
        assert call() == DICE_E_ARG
        assert ('k out of range' in last()) == bad_k, last()
    assert lib.dice_batch_matrix_bytes(None) == -1
    # the matrix download's own NULL check is unchanged
    assert lib.dice_batch_download_matrix(None, None, None, 0, None, None, None) == DICE_E_ARG


def _corpus(n_templates):
    from licensee_amd.corpus import TemplateCorpus
    from tests.test_gpu_corpus_sizes import corpus_of
    return TemplateCorpus(corpus_of(n_templates))


def _tie_corpus():
    """Six templates and their byte-identical clones under later keys: every file ties."""
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    base = [License.find(k) for k in ('apache-2.0', 'bsd-2-clause', 'cc-by-4.0', 'isc', 'mit', 'unlicense')]
    clones = [License('zz-' + l.key, {'title': l.title}, content_normalized=l.content_normalized(),
                      alt_segments=l.spdx_alt_segments()) for l in base]
    return TemplateCorpus(sorted(base + clones, key=lambda l: l.key))


def _files(c, n, seed):
    """n synthetic files, every 7th flagged as a CC false positive."""
    from licensee_amd._native import FileBatch
    from licensee_amd.synth import SyntheticCorpus
    fb = SyntheticCorpus(c).generate(0, n, seed=seed, nthreads=2)
    cc = fb.cc_false_positive.copy()
    cc[::7] = 1
    return FileBatch(fb.bits, fb.wordset_size, fb.length, cc)


def _kernel_text(src, name):
    """The text of one generated kernel after preprocessing (host side of the source)."""
    pre = subprocess.run(['g++', '-E', '-P', '-x', 'c++', '-'], input=src, capture_output=True, text=True,
                         check=True).stdout
    head = 'void ' + name + '('
    assert pre.count(head) == 1, name
    body = pre.split(head)[1]
    return body.split('extern "C"')[0]


@needs_gxx
@pytest.mark.parametrize('layout', ['compact', 'bits'])
def test_sources_hold_topk_kernels_without_row_stores(layout):
    c = _corpus(47)
    src = compact_source(c) if layout == 'compact' else generated_source(c)
    for km in (4, 16):
        top = _kernel_text(src, f'dice_prog_topk{km}')
        mat = _kernel_text(src, f'dice_prog_matrix{km}')
        # the matrix kernel stores through its row pointers once per template; the top-k kernel has
        # neither the pointers, nor their arguments, nor a branch on them
        assert 'orow' in mat and 'srow' in mat
        for word in ('orow', 'srow', 'ov_out', 'score_out'):
            assert word not in top, (km, word)
        assert 'topk_idx' in top and top.count('ge<FASTV>') == mat.count('ge<FASTV>')
        # apart from the rows the two are the same text
        strip = lambda t: re.sub(r'\s+', '', t)
        cut = strip(mat).replace('u32*__restrict__ov_out,double*__restrict__score_out,', '')
        cut = cut.replace('u32*orow=ov_out?ov_out+file:nullptr;double*srow=score_out?score_out+file:nullptr;', '')
        cut, stores = re.subn(r'if\(valid\)\{if\(orow\)\(\*\(orow\+\(i64\)\(\d+\)\*n\)=\(a\)\);'
                              r'if\(srow\)\(\*\(srow\+\(i64\)\(\d+\)\*n\)=\(sc\(a,d\)\)\);\}', '', cut)
        assert stores == 2 * 47     # MATRIX_BODY(true) and MATRIX_BODY(false)
        assert cut == strip(top)


_built = {}


def _run_host_topk(src, tiles, fb, k, tmp_path):
    """dice_prog_topk4 / dice_prog_topk16 of `src` run lane by lane on the host (tests/codegen)."""
    d = str(tmp_path)
    key = hashlib.sha1(src.encode()).hexdigest()
    exe = _built.get(key)
    if exe is None or not os.path.exists(exe):
        bd = os.path.join(d, 'build_' + key[:12])
        os.makedirs(bd)
        with open(os.path.join(bd, 'prog.inc'), 'w') as fh:
            fh.write(src)
        shutil.copy(os.path.join(HERE, 'codegen', 'host_shim.h'), bd)
        exe = os.path.join(bd, 'drv')
        subprocess.run(['g++', '-O1', '-std=c++17', '-w', '-I', bd, '-o', exe,
                        os.path.join(HERE, 'codegen', 'driver_topk.cpp')], check=True)
        _built[key] = exe
    n = fb.n
    npad = ((n + 63) // 64) * 64
    tiles.tofile(os.path.join(d, 'tiles.bin'))
    for name, arr, dt in (('wf', fb.wordset_size, np.uint32), ('len', fb.length, np.int32),
                          ('cc', fb.cc_false_positive, np.uint8)):
        pad = np.zeros(npad, dt)
        pad[:n] = arr
        pad.tofile(os.path.join(d, name + '.bin'))
    subprocess.run([exe, d, str(n), str(k)], check=True, capture_output=True, text=True)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    return (np.ascontiguousarray(rd('tki.out', np.int32).reshape(k, n).T),
            np.ascontiguousarray(rd('tks.out', np.float64).reshape(k, n).T))


def _host_topk(c, fb, k, tmp_path, layout):
    if layout == 'compact':
        src = compact_source(c)
        tiles = compact_pack(fb.bits, c.n_vocab, compact_layout(c))
    else:
        src = generated_source(c)
        wq = (c.w64 + 1) // 2
        tiles = tile_pack(fb.bits, wq, source_qperm(src))
    return _run_host_topk(src, tiles, fb, k, tmp_path)


@needs_gxx
@pytest.mark.parametrize('layout', ['compact', 'bits'])
@pytest.mark.parametrize('n_templates', [5, 33, 47])
def test_generated_topk_kernels_rank_as_the_oracle(n_templates, layout, tmp_path):
    """300 synthetic files, CC flags on every 7th; k = 3 and 4 run dice_prog_topk4, 5 and 16 (more
    slots than the 5-template corpus has templates) dice_prog_topk16."""
    c = _corpus(n_templates)
    fb = _files(c, 300, seed=n_templates)
    for k in (3, 4, 5, 16):
        exp = expected_topk(c, fb, k, nthreads=2)
        assert_topk(_host_topk(c, fb, k, tmp_path, layout), exp, (n_templates, layout, k))
    if n_templates == 5:
        assert (exp[0][:, 5:] == -1).all() and (exp[1][:, 5:] == -1.0).all()


@needs_gxx
@pytest.mark.parametrize('layout', ['compact', 'bits'])
def test_generated_topk_kernels_put_the_later_template_first_on_ties(layout, tmp_path):
    from tests.helpers import NormFile, make_files
    from licensee_amd.license import License
    c = _tie_corpus()
    base = [License.find(k) for k in ('apache-2.0', 'bsd-2-clause', 'cc-by-4.0', 'isc', 'mit', 'unlicense')]
    fb = c.intern_files(make_files(base, 299, 5, cc_rate=0.2) + [NormFile('')])
    for k in (3, 16):
        exp = expected_topk(c, fb, k, nthreads=2)
        assert tie_rate(exp) > 0.7
        # the clone of template t sits at a later index and must come first
        first, second = exp[0][:, 0], exp[0][:, 1]
        tied = (second >= 0) & (exp[1][:, 0] == exp[1][:, 1])
        assert (first[tied] > second[tied]).all()
        assert_topk(_host_topk(c, fb, k, tmp_path, layout), exp, (layout, k))


@needs_gxx
def test_generated_topk_kernels_on_the_ieee_double_branch(tmp_path):
    """Slow lanes mixed into fast waves (the wave-wide vote sends all 64 lanes through
    MATRIX_BODY(false)), and a corpus outside the fast envelope (CORPUS_FAST 0)."""
    from tests.helpers import outside_fast_envelope, widen_lanes
    c = _corpus(47)
    fb, idx = widen_lanes(_files(c, 300, seed=9), seed=3)
    assert idx.size > 10
    assert_topk(_host_topk(c, fb, 5, tmp_path, 'compact'), expected_topk(c, fb, 5, nthreads=2))
    slow = outside_fast_envelope(c)
    assert '#define CORPUS_FAST 0' in compact_source(slow)
    fb = _files(c, 300, seed=10)
    exp = expected_topk(slow, fb, 4, nthreads=2)
    assert (exp[1] > 100.0).any()
    assert_topk(_host_topk(slow, fb, 4, tmp_path, 'compact'), exp)


# ---- kernel resources -------------------------------------------------------------------------

def _occupancy(vgprs, agprs=0):
    """Waves per SIMD the unified register file of a CDNA3/4 SIMD (512 per lane, granule 8) allows."""
    total = (int(vgprs) + 3) // 4 * 4 + int(agprs)
    return min(8, 512 // max(8, (total + 7) // 8 * 8))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
@pytest.mark.parametrize('layout', ['compact', 'bits'])
def test_program_topk_kernel_resources_offline(layout, tmp_path, monkeypatch):
    """Offline compiler, vendored corpus: the top-k kernels use no scratch, spill nothing, need no
    more registers than the matrix kernels they are cut from and run at no lower occupancy."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    c = _corpus(47)
    src = compact_source(c) if layout == 'compact' else generated_source(c)
    path = tmp_path / 'prog.hip'
    path.write_text('#include <hip/hip_runtime.h>\n' + src)
    res = {r['name']: r for r in kernel_resources(str(path))}
    for km in (4, 16):
        top, mat = res[f'dice_prog_topk{km}'], res[f'dice_prog_matrix{km}']
        print(layout, km, 'top-k VGPRs', top['VGPRs'], 'matrix VGPRs', mat['VGPRs'])
        assert top['ScratchSize [bytes/lane]'] == '0' and top['VGPRs Spill'] == '0' and top['SGPRs Spill'] == '0', top
        assert int(top['VGPRs']) <= int(mat['VGPRs']), (top, mat)
        assert int(top['Occupancy [waves/SIMD]']) >= int(mat['Occupancy [waves/SIMD]']), (top, mat)


@pytest.mark.skipif(not os.path.exists(READELF), reason='llvm-readelf not present')
def test_program_topk_kernel_resources_runtime_compiled(tmp_path, monkeypatch):
    """The code objects that ship (hiprtc; dice_precompile caches both tile layouts, each with the
    top-k kernels dice_create will look up): metadata of dice_prog_topk4 / dice_prog_topk16 -- no
    scratch, no VGPR spills, occupancy not below the matrix kernels'."""
    from licensee_amd import _native
    monkeypatch.setenv('DICE_CACHE_DIR', str(tmp_path))
    c = _corpus(47)
    keep, t = _templates_struct(c)
    buf = ctypes.create_string_buffer(4096)
    assert _native.load_library().dice_precompile(ctypes.byref(t), buf, 4096) == 0
    objs = [os.path.join(str(tmp_path), f) for f in os.listdir(str(tmp_path)) if f.endswith('.co')]
    assert len(objs) == 2 and buf.value.decode() in objs
    for obj in objs:
        notes = subprocess.run([READELF, '--notes', obj], capture_output=True, text=True, check=True).stdout
        kernels = {}
        for block in notes.split('- .agpr_count')[1:]:
            f = dict(re.findall(r'\.(\w+):\s+(\S+)', '.agpr_count' + block))
            kernels[f['name']] = f
        for km in (4, 16):
            top, mat = kernels[f'dice_prog_topk{km}'], kernels[f'dice_prog_matrix{km}']
            print(os.path.basename(obj), km, 'top-k VGPRs', top['vgpr_count'], 'matrix VGPRs', mat['vgpr_count'])
            assert top['private_segment_fixed_size'] == '0', top
            assert top['vgpr_spill_count'] == '0', top
            # SGPRs parked in VGPR lanes cost no scratch (tests/test_program_mfma_tables.py prints them
            # too): none in the 4-slot kernel that serves detect's k = 3; the 16-slot kernels of both
            # modes hold their compare masks that way under the runtime compiler
            print('SGPR lane spills', top['sgpr_spill_count'], 'matrix', mat['sgpr_spill_count'])
            if km == 4:
                assert top['sgpr_spill_count'] == '0', top
            assert _occupancy(top['vgpr_count'], top['agpr_count']) >= _occupancy(mat['vgpr_count'], mat['agpr_count'])
            # one pointer pair fewer in the kernel arguments: the rows are gone, not skipped
            assert int(top['kernarg_segment_size']) == int(mat['kernarg_segment_size']) - 16, (top, mat)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not present')
def test_postings_topk_kernel_resources():
    """dice_post_narrow_topk (the matrix kernel without the row stores): no scratch, no VGPR spills,
    no more SGPRs parked in VGPR lanes than the matrix form, and at least its 6 waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    rows = kernel_resources(os.path.join(ROOT, 'licensee_amd', 'csrc', 'dice_post.hip'))
    assert rows, 'no resource remarks (did the compile fail?)'
    res = {r['name']: r for r in rows}
    for tp in (608, 704):
        top = next(v for k, v in res.items() if k.endswith(f'dice::dice_post_narrow_topk<{tp}>'))
        mat = next(v for k, v in res.items() if k.endswith(f'dice::dice_post_narrow_matrix<{tp}>'))
        print(tp, 'top-k VGPRs', top['VGPRs'], 'matrix VGPRs', mat['VGPRs'])
        assert top['ScratchSize [bytes/lane]'] == '0' and top['VGPRs Spill'] == '0', top
        assert int(top['SGPRs Spill']) <= int(mat['SGPRs Spill']), (top, mat)
        assert int(top['VGPRs']) <= int(mat['VGPRs']), (top, mat)
        assert int(top['Occupancy [waves/SIMD]']) >= int(mat['Occupancy [waves/SIMD]']) >= 6, (top, mat)
