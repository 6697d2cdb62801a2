"""SPDX license-list-XML ingestion (licensee_amd/spdx.py).

CPU: the vendored data file equals a fresh ingestion of the reference's 47 XMLs (stored in
tests/golden/reference.tar.xz), every alt-segment count equals license.rb:273-283's regex rule
restated in license.py, the XML markup is gone from every text, and each SPDX text is close to
its choosealicense.com template under the oracle's Dice similarity.
GPU (-m gpu): each SPDX text, read as a LICENSE file, is Dice-matched through the product path
(LicenseFile -> Dice on the GPU) to its own choosealicense.com key at the default threshold 98,
except the listed ones, whose best scores are pinned; the GPU results equal the oracle's; and
the 94-real-text config-3 corpus option builds and scores bit-exactly against the oracle.
Parity of the text extraction is unpinned: the reference never builds these texts (it reads
the XML only for the alt-segment count).
"""
import os

import numpy as np
import pytest

from licensee_amd import spdx
from licensee_amd.license import License, spdx_alt_segments_from_xml

# SPDX texts whose Dice match (threshold 98) is not their own choosealicense.com key, with the
# reason (scores asserted in the GPU test)
NOT_DETECTED = {
    # (own template's oracle score, the best template) -- measured with oracle/dice_oracle.py
    'AFL-3.0': 97.59, 'Artistic-2.0': 97.80, 'CC-BY-4.0': 97.87, 'ECL-2.0': 91.56, 'MS-RL': 97.94,
    'MulanPSL-2.0': 88.39, 'NCSA': 97.46, 'OFL-1.1': 96.31, 'OSL-3.0': 97.56, 'PostgreSQL': 92.47,
    # the SPDX text is another document than choosealicense.com's: CECILL-2.1's SPDX text is the
    # French original; LGPL-3.0's is only the additional permissions on top of the GPL
    'CECILL-2.1': None, 'LGPL-3.0': None,
}


def test_data_file_matches_reference_xml(reference_root):
    ref_spdx = os.path.join(reference_root, 'vendor', 'license-list-XML', 'src')
    fresh = spdx.ingest_dir(ref_spdx)
    stored = [{'id': t.spdx_id, 'name': t.title, 'text': t.content, 'alt_segments': t.spdx_alt_segments()}
              for t in spdx.load()]
    assert fresh == stored
    for fn in sorted(os.listdir(ref_spdx)):
        with open(os.path.join(ref_spdx, fn), encoding='utf-8', newline='') as fh:
            raw = fh.read()
        rec = spdx.license_info_from_xml(raw)
        assert rec['alt_segments'] == spdx_alt_segments_from_xml(raw)


def test_texts_have_no_markup_and_cover_the_vendored_set():
    temps = spdx.load()
    assert len(temps) == 47
    ids = {t.spdx_id for t in temps}
    vendored = {l.spdx_id for l in License.all(hidden=True, pseudo=False)}
    assert ids == vendored
    for t in temps:
        assert '<' not in t.content or '&lt;' not in t.content
        for tag in ('<p>', '<alt', '<optional', '<bullet', '<item', '<br'):
            assert tag not in t.content, (t.spdx_id, tag)
        assert len(t.content_normalized()) > 100


def test_alt_segments_feed_the_length_slack():
    from licensee_amd.corpus import TemplateCorpus
    temps = spdx.load()
    c = TemplateCorpus(temps)
    for i, t in enumerate(c.templates):
        assert c.length_slack[i] == 5 * max(len(t.fields_normalized()), t.spdx_alt_segments())


def test_spdx_texts_close_to_their_templates_oracle():
    """Oracle Dice similarity (python restatement) of each SPDX text as a file against its own
    choosealicense.com template: the two are versions of one license text."""
    import oracle.dice_oracle as O
    by_id = {l.spdx_id: l for l in License.all(hidden=True, pseudo=False)}
    low = []
    for t in spdx.load():
        lic = by_id[t.spdx_id]
        s = O.similarity(O.OracleTemplate(lic.key, lic.content_normalized(), lic.spdx_alt_segments()),
                         O.OracleFile(t.content_normalized()))
        if s < 90.0:
            low.append((t.spdx_id, round(s, 2)))
    assert len(low) <= 12, low


@pytest.mark.gpu
def test_spdx_texts_detected_on_gpu():
    import oracle.dice_oracle as O
    from licensee_amd.project_files import LicenseFile
    from tests.helpers import oracle_templates
    temps = License.all(hidden=True, pseudo=False)
    otpl = oracle_templates(temps)
    by_id = {l.spdx_id: l for l in temps}
    misses = {}
    for t in spdx.load():
        lf = LicenseFile(t.content, {'name': 'LICENSE'})
        key, m = lf.license().key, lf.matcher()
        if m is not None and m.name == 'dice':
            # the GPU Dice result equals the oracle's (dice.rb:8-14 over content_helper.rb:128-133)
            i, conf = O.match(otpl, O.OracleFile(lf.content_normalized(), lf.content.strip()), 98)
            assert key == temps[i].key and lf.confidence() == conf, (t.spdx_id, key, conf)
        if key != by_id[t.spdx_id].key:
            misses[t.spdx_id] = (key, m.name if m else None)
    assert set(misses) == set(NOT_DETECTED), misses
    # Dice#matches_by_similarity on the GPU ranks the own template first for every text but the
    # two that are other documents (dice.rb:34-41)
    from licensee_amd.matchers import Dice
    for t in spdx.load():
        ranked = Dice(LicenseFile(t.content, {'name': 'LICENSE'})).matches_by_similarity()
        top, score = ranked[0]
        if NOT_DETECTED.get(t.spdx_id, 0) is None:
            assert top.key != by_id[t.spdx_id].key
        else:
            assert top.key == by_id[t.spdx_id].key, (t.spdx_id, top.key, score)
            if t.spdx_id in NOT_DETECTED:
                assert round(score, 2) == NOT_DETECTED[t.spdx_id], (t.spdx_id, score)


@pytest.mark.gpu
def test_config3_corpus_with_spdx_texts_gpu_vs_oracle():
    from licensee_amd._native import Scorer
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.synth import SyntheticCorpus
    from oracle.native import OracleScorer
    temps = spdx.corpus_with_spdx(License.all(hidden=True, pseudo=False), total=600)
    assert len(temps) == 600 and sum(k.key.startswith('spdx:') for k in temps) == 47
    c = TemplateCorpus(temps)
    fb = SyntheticCorpus(c).generate(0, 20_000, seed=94, nthreads=16)
    sc = Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab, device=0)
    orc = OracleScorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab)
    for thr in (98.0, 0.0):
        got = sc.match(fb, thr)
        exp = orc.match(fb.bits, fb.wordset_size, fb.length, fb.cc_false_positive, thr, nthreads=16, mode=0)
        for a, b in zip(got, exp):
            assert np.array_equal(a, b)
    ov, s, tki, tks = sc.matrix(SyntheticCorpus(c).generate(0, 2000, seed=95, nthreads=16), 3)
    sc.close()
