"""ContentHelper#content_hash on the device (dice_batch_content_hash, csrc/dice_hash.hip).

content_hash is DIGEST.hexdigest content_normalized with SHA-1 (content_helper.rb:136-138). The
device hashes the normalized texts dice_batch_upload_text left resident, one lane per file, and
flags the files whose text holds a non-ASCII character (resident as the byte 0x80), which
BatchDetector(content_hash=True) hashes on the host. ``hashlib.sha1`` is the checker everywhere:
every digest is compared bit for bit, every status exactly.

The packing helper fills every gap between the 16-byte aligned files and the tail of the buffer
with 0xFF, so a read past a file's length that was not masked both breaks the digest and raises
the status."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from licensee_amd.license import License

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')

EDGE_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 121, 127, 128, 129, 191, 192,
                1000, 4095, 4096, 65537)


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


def _ascii_text(rng, n):
    return bytes(rng.choices(range(0x20, 0x7F), k=n))


def _pack(texts, exact_end=False):
    """texts (bytes) at 16-byte aligned offsets, every gap and the tail 0xFF; ``exact_end`` slices
    the buffer at the end of the last text (text_bytes = offsets[-1] + text_len[-1])."""
    tl = np.array([len(t) for t in texts], np.int32)
    step = (tl.astype(np.int64) + 15) // 16 * 16
    off = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64) if len(texts) else np.zeros(0, np.int64)
    total = int(step.sum())
    buf = np.full(total + 48, 0xFF, np.uint8)
    for t, o in zip(texts, off.tolist()):
        buf[o:o + len(t)] = np.frombuffer(t, np.uint8)
    if exact_end:
        buf = buf[:int(off[-1]) + int(tl[-1])]
    return np.ascontiguousarray(buf), off, tl


def _upload(b, texts, exact_end=False):
    buf, off, tl = _pack(texts, exact_end)
    b.upload_text(buf, off, tl, tl, np.zeros(len(texts), np.uint8))


def _device_hashes(sc, texts, exact_end=False, batch=None):
    b = batch if batch is not None else sc.batch(max(len(texts), 1))
    try:
        _upload(b, texts, exact_end)
        b.content_hash()
        digest, status = b.download_content_hash()
    finally:
        if batch is None:
            b.close()
    assert digest.shape == (len(texts), 20) and digest.dtype == np.uint8
    assert status.shape == (len(texts),) and status.dtype == np.uint8
    hx = digest.tobytes().hex()
    return [hx[i:i + 40] for i in range(0, len(hx), 40)], status


def _check(sc, texts, exact_end=False, batch=None):
    got, status = _device_hashes(sc, texts, exact_end, batch)
    want = [hashlib.sha1(t).hexdigest() for t in texts]
    bad = [(i, len(texts[i]), got[i], want[i]) for i in range(len(texts)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:5])
    flags = np.array([any(c >= 0x80 for c in t) for t in texts], np.uint8)
    wrong = np.nonzero(status != flags)[0]
    assert wrong.size == 0, [(int(i), len(texts[i]), int(status[i]), int(flags[i])) for i in wrong[:5]]
    return status


@pytest.fixture(scope='module')
def edge_texts():
    rng = random.Random(20250202)
    return [_ascii_text(rng, n) for n in EDGE_LENGTHS]


def test_padding_edges(vendored, edge_texts):
    """Every length around the padding rule's edges (the 0x80 byte, the 56-byte limit of the
    length words, whole blocks, one text of 1,025 blocks) in one batch."""
    _, _, sc = vendored
    status = _check(sc, edge_texts)
    assert not status.any()


def test_last_file_ends_exactly_at_text_bytes(vendored, edge_texts):
    """The 65,537-byte text last, the buffer sliced at its last byte: no padding follows it."""
    _, _, sc = vendored
    assert len(edge_texts[-1]) == 65537
    buf, off, tl = _pack(edge_texts, exact_end=True)
    assert buf.shape[0] == off[-1] + tl[-1] and buf.shape[0] % 16 == 1
    status = _check(sc, edge_texts, exact_end=True)
    assert not status.any()


def test_many_files_refill_and_ragged_wave(vendored):
    """20,001 short texts: lanes take file after file from the counter, the last wave is ragged."""
    _, _, sc = vendored
    rng = random.Random(7)
    texts = [_ascii_text(rng, rng.randint(0, 300)) for _ in range(20001)]
    status = _check(sc, texts)
    assert not status.any()


def test_divergent_lengths_in_one_wave(vendored):
    _, _, sc = vendored
    rng = random.Random(11)
    texts = [_ascii_text(rng, rng.randint(0, 40000)) for _ in range(130)]
    status = _check(sc, texts)
    assert not status.any()


def test_non_ascii_is_flagged_exactly(vendored):
    """A byte >= 0x80 first, last, in the middle, or nowhere: status == any(b >= 0x80) per file, an
    ASCII file between 0xFF-filled gaps stays 0, and the digest is that of the resident bytes."""
    _, _, sc = vendored
    rng = random.Random(13)
    texts = []
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 100, 1000, 4097):
        t = _ascii_text(rng, n)
        texts.append(t)                                   # none
        texts.append(b'\x80' + t[1:])                     # first
        texts.append(t[:-1] + b'\x80')                    # last
        texts.append(t[:n // 2] + b'\xe9' + t[n // 2 + 1:])   # middle
        texts.append(t)
    texts.append(b'')
    status = _check(sc, texts)
    assert status.sum() == sum(any(c >= 0x80 for c in t) for t in texts) and 0 < status.sum() < len(texts)


def test_template_goldens(vendored):
    """The 47 vendored templates' content_normalized in the resident form: every ASCII one's device
    digest is the reference's own hash (license-hashes.json), the others are flagged."""
    corpus, _, sc = vendored
    want = golden('reference_expectations.json')['template_sha1']
    norm = [t.content_normalized() for t in corpus.templates]
    resident = [bytes(ord(c) if ord(c) < 0x80 else 0x80 for c in s) for s in norm]
    got, status = _device_hashes(sc, resident)
    n_ascii = 0
    for t, s, h, st in zip(corpus.templates, norm, got, status.tolist()):
        assert st == (0 if s.isascii() else 1), t.key
        if st == 0:
            assert h == want[t.key], t.key
            n_ascii += 1
    assert n_ascii >= 40
    assert [h for h in got] == [hashlib.sha1(r).hexdigest() for r in resident]


def _fixture_records():
    recs = golden('fixture_files.json')
    return [r for r in recs if r['expected'].get('hash') and 'unsupported' not in r and
            sum(x['fixture'] == r['fixture'] for x in recs) == 1]


def test_batch_detector_content_hash(reference_root):
    """BatchDetector(content_hash=True) over the raw fixture files: every Detection.content_hash is
    the reference's `hash:` expectation, almost all of them from the device, and license, matcher
    and confidence are those of a detector without hashes."""
    from licensee_amd.batch import BatchDetector
    recs = _fixture_records()
    assert len(recs) >= 40
    contents, names = [], []
    for r in recs:
        with open(os.path.join(reference_root, 'spec', 'fixtures', r['fixture'], r['file']), 'rb') as fh:
            contents.append(fh.read())
        names.append(r['file'])
    det = BatchDetector(content_hash=True)
    plain = BatchDetector()
    try:
        out = det.detect(contents, names)
        _, status = det._batch.download_content_hash()
        assert status.shape == (len(recs),) and status.sum() <= 2
        for r, d in zip(recs, out):
            assert d.content_hash == r['expected']['hash'], r['fixture']
        base = plain.detect(contents, names)
        assert all(d.content_hash is None for d in base)
        assert [(d.license.key, d.matcher, d.confidence) for d in out] == \
               [(d.license.key, d.matcher, d.confidence) for d in base]
        k = len(recs) // 3
        parts = [(contents[:k], names[:k]), (contents[k:2 * k], names[k:2 * k]), (contents[2 * k:], names[2 * k:])]
        streamed = [d for batch in det.detect_stream(parts) for d in batch]
        assert streamed == out
    finally:
        det.close()
        plain.close()


def test_state(vendored):
    from licensee_amd._native import DiceError
    from licensee_amd.batch import BatchDetector
    _, hp, sc = vendored
    rng = random.Random(17)
    b = sc.batch(300)
    try:
        big = [_ascii_text(rng, rng.randint(0, 500)) for _ in range(300)]
        small = [_ascii_text(rng, rng.randint(0, 500)) for _ in range(10)]
        _check(sc, big, batch=b)
        # a new upload: no digest yet, then ten of them
        _upload(b, small)
        with pytest.raises(DiceError, match='dice error -4'):
            b.download_content_hash()
        got, status = _device_hashes(sc, small, batch=b)
        assert len(got) == 10 and got == [hashlib.sha1(t).hexdigest() for t in small] and not status.any()
        # set_rows leaves the texts resident
        fb = hp.prep_files([b'mit license'], None, nthreads=1, field_masks=True)
        b.set_rows([3], fb[0].bits, fb[0].wordset_size, fb[2])
        b.content_hash()
        assert b.download_content_hash()[0].tobytes().hex() == ''.join(got)
        # an upload of bitsets: the texts are no longer the batch's files
        b.upload(fb[0])
        with pytest.raises(DiceError, match='dice error -4'):
            b.content_hash()
        with pytest.raises(DiceError, match='dice error -4'):
            b.download_content_hash()
    finally:
        b.close()
    with pytest.raises(ValueError, match='wordset_on'):
        BatchDetector(wordset_on='host', content_hash=True)
