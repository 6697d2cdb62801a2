"""Resident texts as UTF-8 (dice_batch_upload_text_utf8, csrc/dice_words.hip and dice_hash.hip).

ContentHelper#content_hash is SHA-1 of content_normalized (content_helper.rb:136-138): with the texts
resident as content_normalized's own UTF-8 the device's digest is content_hash for non-ASCII files
too, and no file is left to the host. The wordset scan (content_helper.rb:108-110) is unchanged --
its [\\w/-] is ASCII, every byte >= 0x80 separates tokens -- so rows, |W_F| and field masks equal
those of the one-byte-per-character upload and of the host scan. content_normalized.length is in
characters: with ``length=None`` the device counts them, (b & 0xC0) != 0x80 over each file's bytes.

Checkers: the host scan (lh_prep_files, pinned to the Python restatement by tests/test_native_host.py),
``len(bytes.decode())``, ``hashlib.sha1``, the reference's own license-hashes.json and fixture
expectations. Everything is compared exactly. Gaps between files and the slack behind the last one
are 0xFF, so a read past a file's length that is not masked over-counts characters and breaks digests."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from licensee_amd.license import License
from tests.utf8_texts import fuzz_texts, pack, to_x80

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 65537)
SHA1_EDGES = (55, 56, 63, 64, 65, 119, 120)
STRADDLERS = ('é', '许', '😀')


def golden(name):
    with open(os.path.join(GOLDEN, name), encoding='utf-8') as fh:
        return json.load(fh)


@pytest.fixture(scope='module')
def vendored():
    from licensee_amd._native import Scorer
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.native_host import HostPrep
    corpus = TemplateCorpus(License.all(hidden=True, pseudo=False))
    hp = HostPrep(corpus)
    sc = Scorer(corpus.lf_bits, corpus.lf_size, corpus.fields_set_size, corpus.length_slack, corpus.length,
                corpus.is_cc, corpus.n_vocab, device=0)
    sc.vocab_setup(corpus.vocab, hp.nv_fields)
    yield corpus, hp, sc
    sc.close()


def utf8_of_length(nbytes, seed=0):
    """``nbytes`` bytes of valid UTF-8 with characters of 1 to 4 bytes in which a 2-, 3- or 4-byte
    character (in turn, split at every possible point in turn) straddles every 16-byte boundary, and
    so every 1 KiB boundary, that has room for it."""
    parts, made, tail, i = [], 0, 0, seed
    while made < nbytes + 8:
        ch = STRADDLERS[i % 3]
        size = len(ch.encode('utf-8'))
        head = 1 + (i // 3) % (size - 1)        # its bytes before the boundary
        fill = 16 - tail - head
        inner = 'ü' if fill >= 6 and i % 2 else ''
        parts.append(('lorem ipsum dolor ' * 2)[:fill - 2 * len(inner)] + inner + ch)
        tail = size - head
        made += 16
        i += 1
    b = ''.join(parts).encode('utf-8')[:nbytes].decode('utf-8', 'ignore').encode('utf-8')   # (no cut character)
    return b + b'z' * (nbytes - len(b))


def _rows(b):
    bits, wf, fm = b.download_rows()
    return bits, wf, fm


def _python_scan(corpus, hp, text):
    """Row, |W_F| and field mask of an already normalized text by the wordset regex on the host."""
    from licensee_amd import content_helper as ch
    ws = frozenset(m.group(0) for m in ch.WORDSET_REGEX.finditer(text))
    bits, wf = corpus.intern(ws)
    return bits, wf, sum(1 << k for k, w in enumerate(hp.nv_fields) if w in ws)


def _corner_texts():
    """Already normalized texts (normalization is the identity on them, asserted by the test): a
    2-, 3- and 4-byte character split at every point across the 16-byte lane-group edges and the
    1 KiB chunk edges, a text of non-ASCII characters only, an empty one, a 5,000-byte token
    followed by a two-byte character."""
    filler = 'ab cd ' * 400
    out = []
    for edge in (16, 32, 1024, 2048):
        for ch in STRADDLERS:
            for head in range(1, len(ch.encode('utf-8'))):
                out.append(filler[:edge - head] + ch + ' tail words here')
                out.append(filler[:edge - head] + ch + "s' x's" + ch + 'ab')
    out += ['许可😀é' * 50, '', 'x' * 5000 + 'é']
    return out


def test_scan_parity(vendored):
    """Rows, |W_F| and field masks after the UTF-8 upload == after the 0x80 upload == the host scan."""
    corpus, hp, sc = vendored
    corners = _corner_texts()
    raw = [t.encode('utf-8') for t in fuzz_texts(300) + corners]
    t8, off8, tl8, ln8, cc8, _, fell8 = hp.normalize_files(raw, None, nthreads=8, utf8=True)
    t1, off1, tl1, ln1, cc1, _, fell1 = hp.normalize_files(raw, None, nthreads=8)
    assert not fell8.any() and not fell1.any()
    k = len(raw) - len(corners)
    for i, c in enumerate(corners):     # the straddles are where they were put
        assert t8[int(off8[k + i]):int(off8[k + i]) + int(tl8[k + i])].tobytes() == c.encode('utf-8'), i
    assert (tl8 >= ln8).all() and (tl8 > ln8).sum() >= 250 and np.array_equal(tl1, ln1) and np.array_equal(ln1, ln8)
    fb, _, fm, fell = hp.prep_files(raw, None, nthreads=8, field_masks=True)
    assert not fell.any() and np.array_equal(fb.length, ln8)
    b = sc.batch(len(raw))
    try:
        st8 = b.upload_text(t8, off8, tl8, ln8, cc8, utf8=True)
        bits8, wf8, fm8 = _rows(b)
        len8 = b.download_length()
        st1 = b.upload_text(t1, off1, tl1, ln1, cc1)
        bits1, wf1, fm1 = _rows(b)
    finally:
        b.close()
    assert not st8.any() and not st1.any()          # no overflow
    assert np.array_equal(len8, ln8)
    bad = np.nonzero((bits8 != fb.bits).any(axis=1) | (wf8 != fb.wordset_size) | (fm8 != fm))[0]
    assert bad.size == 0, [(int(i), raw[i][:80], int(wf8[i]), int(fb.wordset_size[i])) for i in bad[:3]]
    assert np.array_equal(bits8, bits1) and np.array_equal(wf8, wf1) and np.array_equal(fm8, fm1)
    assert wf8[-1] == 1 and wf8[-2] == 0 and wf8[-3] == 0      # the token, the empty text, no ASCII at all


def test_character_lengths_counted_on_the_device(vendored):
    """length=None: the device's per-file character counts == len(text.decode()), every edge length
    and 130 files of 0 to 40,000 bytes in one launch, 0xFF between and behind the files, the last
    file ending exactly at text_bytes; and match results equal those with the host's lengths."""
    corpus, _, sc = vendored
    rng = random.Random(20250202)
    texts = [utf8_of_length(rng.randint(0, 40000), seed=j) for j in range(130)]
    texts += [t.content_normalized().encode('utf-8') for t in corpus.templates]     # (files that match)
    texts += [utf8_of_length(n, seed=n) for n in LENGTHS]
    assert len(texts[-1]) == 65537 and [len(t) for t in texts[-len(LENGTHS):]] == list(LENGTHS)
    for t in texts[:130] + texts[-len(LENGTHS):]:       # the construction: a character across every boundary
        edges = range(16, len(t) - 4, 16)
        assert all((t[e] & 0xC0) == 0x80 for e in edges)
    assert {len(c.encode('utf-8')) for t in texts[:5] for c in t.decode('utf-8')} == {1, 2, 3, 4}
    want = np.array([len(t.decode('utf-8')) for t in texts], np.int32)
    buf, off, tl = pack(texts, fill=0xFF, gap=1, exact_end=True)
    assert buf.shape[0] == off[-1] + tl[-1] and buf.shape[0] % 16 == 1
    cc = np.zeros(len(texts), np.uint8)
    b = sc.batch(len(texts))
    try:
        st = b.upload_text(buf, off, tl, None, cc, utf8=True)
        got = b.download_length()
        rows_dev = _rows(b)
        b.match(98.0)
        res_dev = b.download_match()
        st2 = b.upload_text(buf, off, tl, want, cc, utf8=True)
        assert np.array_equal(b.download_length(), want)
        rows_host = _rows(b)
        b.match(98.0)
        res_host = b.download_match()
    finally:
        b.close()
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, [(int(i), int(tl[i]), int(got[i]), int(want[i])) for i in wrong[:8]]
    assert np.array_equal(st, st2)
    for a, h in zip(rows_dev + res_dev, rows_host + res_host):
        assert np.array_equal(a, h)
    assert (res_dev[0][130:177] >= 0).any()         # (the templates' own texts: the lengths took part in a match)


def test_character_lengths_with_several_files_per_wave(vendored):
    """20,001 short files: more files than the device holds waves (8,192 on 256 CUs), so a wave
    counts several consecutive files and the last wave's share is ragged."""
    _, _, sc = vendored
    rng = random.Random(3)
    texts = [utf8_of_length(rng.randint(0, 300), seed=j) for j in range(20001)]
    want = np.array([len(t.decode('utf-8')) for t in texts], np.int32)
    buf, off, tl = pack(texts, fill=0xFF, exact_end=True)
    b = sc.batch(len(texts))
    try:
        st = b.upload_text(buf, off, tl, None, np.zeros(len(texts), np.uint8), utf8=True)
        got = b.download_length()
    finally:
        b.close()
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, [(int(i), int(tl[i]), int(got[i]), int(want[i])) for i in wrong[:8]]
    assert not st.any() and (want < tl).sum() > 15000


@pytest.mark.parametrize('utf8', [False, True], ids=['bytes', 'utf8'])
def test_unpadded_last_file_is_scanned_to_its_end(vendored, utf8):
    """A last file ending exactly at a text_bytes that is no multiple of 16: every byte is scanned.
    (The checker is the wordset regex on the host: lh_prep_files normalizes its input, and
    'mit license' is a title that normalizes to nothing.)"""
    corpus, hp, sc = vendored
    for text in ('x' * 21, 'mit license'):
        raw = text.encode('ascii')
        buf = np.frombuffer(raw, np.uint8).copy()
        assert buf.shape[0] == len(raw) and len(raw) % 16
        b = sc.batch(1)
        try:
            st = b.upload_text(buf, [0], [len(raw)], [len(raw)], [0], utf8=utf8)
            bits, wf, fm = _rows(b)
        finally:
            b.close()
        wbits, wwf, wfm = _python_scan(corpus, hp, text)
        assert not st.any()
        assert np.array_equal(bits[0], wbits) and int(wf[0]) == wwf and int(fm[0]) == wfm, text
    assert wwf == 2 and wbits.any()         # ('license' is a vocabulary word)


def _hashes(b):
    b.content_hash()
    digest, status = b.download_content_hash()
    hx = digest.tobytes().hex()
    return [hx[i:i + 40] for i in range(0, len(hx), 40)], status


def test_template_hashes_all_47(vendored):
    """The 47 vendored templates' content_normalized as UTF-8: every device digest is the reference's
    own hash (license-hashes.json), the 6 non-ASCII templates included, and no file is flagged."""
    corpus, _, sc = vendored
    want = golden('reference_expectations.json')['template_sha1']
    norm = [t.content_normalized() for t in corpus.templates]
    assert len(norm) == 47 and sum(not s.isascii() for s in norm) == 6
    texts = [s.encode('utf-8') for s in norm]
    buf, off, tl = pack(texts)
    b = sc.batch(len(texts))
    try:
        b.upload_text(buf, off, tl, [len(s) for s in norm], np.zeros(len(texts), np.uint8), utf8=True)
        got, status = _hashes(b)
    finally:
        b.close()
    assert not status.any()
    assert got == [want[t.key] for t in corpus.templates]


def test_sha1_padding_edges_and_the_old_status(vendored):
    """Texts whose last character is a 2-, 3- or 4-byte one ending at each SHA-1 padding edge: the
    digests are hashlib's and, after the UTF-8 upload, no status is set; after the one-byte upload
    of the same bytes the status is any(b >= 0x80), as before."""
    _, _, sc = vendored
    rng = random.Random(5)
    texts = []
    for n in SHA1_EDGES:
        for ch in STRADDLERS:
            tail = ch.encode('utf-8')
            texts.append(bytes(rng.choices(range(0x20, 0x7F), k=n - len(tail))) + tail)
        texts.append(bytes(rng.choices(range(0x20, 0x7F), k=n)))
    assert sorted({len(t) for t in texts}) == list(SHA1_EDGES)
    want = [hashlib.sha1(t).hexdigest() for t in texts]
    flags = np.array([any(c >= 0x80 for c in t) for t in texts], np.uint8)
    lens = [len(t.decode('utf-8')) for t in texts]
    buf, off, tl = pack(texts)
    cc = np.zeros(len(texts), np.uint8)
    b = sc.batch(len(texts))
    try:
        b.upload_text(buf, off, tl, lens, cc, utf8=True)
        got8, st8 = _hashes(b)
        b.upload_text(buf, off, tl, tl, cc)
        got1, st1 = _hashes(b)
    finally:
        b.close()
    assert got8 == want and not st8.any()
    assert got1 == want and np.array_equal(st1, flags) and 0 < flags.sum() < len(texts)


def _fixture_records():
    recs = golden('fixture_files.json')
    return [r for r in recs if r['expected'].get('hash') and 'unsupported' not in r and
            sum(x['fixture'] == r['fixture'] for x in recs) == 1]


def _triples(dets):
    return [(d.license.key, d.matcher, d.confidence) for d in dets]


def test_batch_detector_hashes_everything_on_the_device(vendored, reference_root):
    """BatchDetector(content_hash=True): every hash of the fixture files is the reference's `hash:`
    and every hash of 200 non-ASCII texts the per-file Python content_hash, none of them from the
    host; license, matcher and confidence equal a detector without hashes; the stream equals detect."""
    from licensee_amd.batch import BatchDetector
    from licensee_amd.project_files import LicenseFile
    _, hp, _ = vendored
    recs = _fixture_records()
    assert len(recs) >= 40
    contents, names = [], []
    for r in recs:
        with open(os.path.join(reference_root, 'spec', 'fixtures', r['fixture'], r['file']), 'rb') as fh:
            contents.append(fh.read())
        names.append(r['file'])
    fuzz = [t.encode('utf-8') for t in fuzz_texts(260, seed=7) if not t.isascii()][:200]
    assert len(fuzz) == 200
    assert not hp.normalize_files(fuzz, None, utf8=True)[-1].any()        # no Python fallback among them
    fuzz_want = [LicenseFile(t, 'LICENSE').content_hash() for t in fuzz]
    assert len(set(fuzz_want)) > 190
    det = BatchDetector(content_hash=True)
    plain = BatchDetector()
    try:
        out = det.detect(contents, names)
        assert det.host_hashed == 0
        assert not det._batch.download_content_hash()[1].any()
        assert [d.content_hash for d in out] == [r['expected']['hash'] for r in recs]
        assert _triples(out) == _triples(plain.detect(contents, names))
        fout = det.detect(fuzz)
        assert det.host_hashed == 0
        assert [d.content_hash for d in fout] == fuzz_want
        base = plain.detect(fuzz)
        assert plain.host_hashed == 0 and all(d.content_hash is None for d in base)
        assert _triples(fout) == _triples(base)
        both, bn = contents + fuzz, names + ['LICENSE'] * len(fuzz)
        k = len(both) // 3
        parts = [(both[:k], bn[:k]), (both[k:2 * k], bn[k:2 * k]), (both[2 * k:], bn[2 * k:])]
        streamed = [d for batch in det.detect_stream(parts) for d in batch]
        assert det.host_hashed == 0
        assert streamed == out + fout
    finally:
        det.close()
        plain.close()


def test_only_a_utf8_upload_leaves_the_record(vendored):
    """dice_batch_upload, dice_batch_upload_ids and dice_batch_upload_text clear the batch's UTF-8
    record (the same bytes uploaded by the old entry are flagged again); dice_batch_set_rows keeps it."""
    from licensee_amd._native import DiceError, bits_to_ids
    corpus, hp, sc = vendored
    texts = ['café license'.encode('utf-8'), b'plain words', '许可 granted 😀'.encode('utf-8')]
    want = [hashlib.sha1(t).hexdigest() for t in texts]
    lens = [len(t.decode('utf-8')) for t in texts]
    buf, off, tl = pack(texts)
    cc = np.zeros(3, np.uint8)
    fb, _, fm, _ = hp.prep_files([b'permission is hereby granted'] * 3, None, nthreads=1, field_masks=True)
    offsets, ids = bits_to_ids(fb.bits, corpus.n_vocab)
    b = sc.batch(3)
    try:
        for other in ('upload', 'upload_ids', 'upload_text'):
            b.upload_text(buf, off, tl, lens, cc, utf8=True)
            got, status = _hashes(b)
            assert got == want and status.tolist() == [0, 0, 0]
            # set_rows leaves the texts and the record
            b.set_rows([1], fb.bits[:1], fb.wordset_size[:1], fm[:1])
            got, status = _hashes(b)
            assert got == want and status.tolist() == [0, 0, 0]
            if other == 'upload':
                b.upload(fb)
            elif other == 'upload_ids':
                b.upload_ids(offsets, ids, fb.wordset_size, fb.length, fb.cc_false_positive)
            if other != 'upload_text':
                with pytest.raises(DiceError, match='dice error -4'):
                    b.content_hash()
            b.upload_text(buf, off, tl, tl, cc)
            got, status = _hashes(b)
            assert got == want and status.tolist() == [1, 0, 1], other
    finally:
        b.close()
