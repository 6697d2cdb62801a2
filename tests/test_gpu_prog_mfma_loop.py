"""dice_prog_match_mfma's tile loop carried over several tiles per wave (csrc/dice_program_gen.cpp,
MFMA_TILE). A workgroup of 12 waves walks a contiguous share of the tiles, wave w taking every
12th; each tile's K-steps request the wave's next tile, and after its last tile the requests
collapse onto the tile it holds. The batches of the other tests give a wave one tile, at most two
to one wave of a workgroup, so here the shares are longer: with C compute units,

  64 (12 C + 1) + 5    one wave per workgroup (or none) has two tiles, the last tile is partial
  64 (25 C + 3) + 13   waves of two and three tiles, shares of 25 and 26 tiles, a partial last tile
  64 * 5 + 1           shares shorter than a workgroup: waves leave before their first tile

The vendored corpus with DICE_PROG_MATCH=mfma against DICE_PROG_MATCH=valu, exactly, on every file,
for match and match(confidence=True); the C oracle on the first and last few thousand files. Files
outside the fast envelope sit in tiles that are a wave's second and third, so the IEEE-double branch
runs in a later iteration too."""
import numpy as np
import pytest

from tests.test_gpu_compact_layout import _same
from tests.test_gpu_prog_mfma import _oracle, _scorer

pytestmark = pytest.mark.gpu

ORACLE_FILES = 3000
# block 0 of the second shape holds tiles 0-24: tile 17 is wave 5's second, tile 24 wave 0's third
SLOW_FILES = (64 * 17 + 3, 64 * 24 + 10)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _head(fb, n):
    from licensee_amd._native import FileBatch
    return FileBatch(fb.bits[:n], fb.wordset_size[:n], fb.length[:n], fb.cc_false_positive[:n])


@pytest.fixture(scope='module')
def loop_setup():
    """The corpus, its two scorers, the oracle and the largest batch (the others are heads of it)."""
    from licensee_amd._native import FileBatch
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from licensee_amd.synth import SyntheticCorpus
    c = TemplateCorpus(License.all(hidden=True, pseudo=False))
    n = 64 * (25 * _cus() + 3) + 13
    fb = SyntheticCorpus(c).generate(0, n, seed=5, nthreads=8)
    wf, ln, cc = fb.wordset_size.copy(), fb.length.copy(), fb.cc_false_positive.copy()
    for i in SLOW_FILES + (n - 2,):
        wf[i], ln[i] = (1 << 20) + 5, (1 << 21) + 9
    cc[7::13] = 1                                   # CC-flagged files in every tile
    fb = FileBatch(fb.bits, wf, ln, cc)
    mp = pytest.MonkeyPatch()
    try:
        mf, va = _scorer(c, mp, 'mfma'), _scorer(c, mp, 'valu')
    finally:
        mp.undo()
    assert mf.program_stage() == 2 and va.program_stage() == 0
    yield c, fb, mf, va, _oracle(c)
    mf.close()
    va.close()


def _both(sc, fb):
    b = sc.batch(fb.n)
    try:
        b.upload(fb)
        b.match(98.0)
        m = b.download_match()
        b.match(98.0, confidence=True)
        return m, b.download_match()
    finally:
        b.close()


@pytest.mark.parametrize('shape', ['two_tiles', 'three_tiles', 'short_shares'])
def test_loop_over_several_tiles(loop_setup, shape):
    from licensee_amd._native import FileBatch
    c, big, mf, va, orc = loop_setup
    C = _cus()
    n = {'two_tiles': 64 * (12 * C + 1) + 5, 'three_tiles': 64 * (25 * C + 3) + 13, 'short_shares': 64 * 5 + 1}[shape]
    assert n <= big.n and (shape != 'three_tiles' or n == big.n)
    fb = _head(big, n)
    got, ref = _both(mf, fb), _both(va, fb)
    _same(got[0], ref[0], (shape, 'valu', 'match'))
    _same(got[1], ref[1], (shape, 'valu', 'confidence'))
    pick = np.unique(np.concatenate([np.arange(min(n, ORACLE_FILES)), np.arange(max(0, n - ORACLE_FILES), n)]))
    sub = FileBatch(fb.bits[pick], fb.wordset_size[pick], fb.length[pick], fb.cc_false_positive[pick])
    m = orc.match(sub.bits, sub.wordset_size, sub.length, sub.cc_false_positive, 98.0, nthreads=8)
    conf = (m[0], np.where(m[0] >= 0, m[1], 0).astype(np.uint32), np.where(m[0] >= 0, m[2], 0.0))
    _same([x[pick] for x in got[0]], m, (shape, 'oracle', 'match'))
    _same([x[pick] for x in got[1]], conf, (shape, 'oracle', 'confidence'))
