"""The native host library under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/sanitize/driver.cpp links csrc/rx.cpp, normalize.cpp and vocab_pack.cpp built with
-fsanitize=address,undefined (no recovery), once for baseline x86-64 (the scalar scans) and once
for x86-64-v3 (the AVX2 scans of csrc/scan.h, as the shipped library is built), and drives every entry point of
include/licensee_host.h -- lh_create, lh_set_unicode, lh_set_templates, threaded
lh_prep_files, lh_normalize_files (room for all, then for half), lh_normalize, lh_vocab_pack, lh_destroy -- over the reference fixture texts
(goldens), all 47 template texts, seeded fuzz texts (markup, non-ASCII, contextual
characters) and long mixed files. Host code only: GPU sanitizers are not available.
"""
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _s(b: bytes) -> bytes:
    return struct.pack('<I', len(b)) + b


def _strs(items) -> bytes:
    out = struct.pack('<I', len(items))
    for x in items:
        out += _s(x if isinstance(x, bytes) else x.encode('utf-8'))
    return out


def _arr(a: np.ndarray) -> bytes:
    a = np.ascontiguousarray(a)
    return struct.pack('<I', a.size) + a.tobytes()


def _texts():
    from licensee_amd.license import License
    from tests.test_native_host import CONTEXTUAL, FRAGMENTS
    with open(os.path.join(HERE, 'golden', 'vendored.json'), encoding='utf-8') as fh:
        vend = json.load(fh)
    texts = [c['normalized'] for t in vend['templates'] for c in t['cases'].values()]
    texts += [l.content_normalized() for l in License.all(hidden=True, pseudo=False)]
    rng = random.Random(7)
    for _ in range(300):
        parts = [rng.choice(FRAGMENTS + CONTEXTUAL) for _ in range(rng.randint(1, 15))]
        texts.append(rng.choice(['\n', '\n\n', ' ', '\r\n']).join(parts))
    bodies = [l.content_normalized() for l in License.all(hidden=True, pseudo=False)]
    texts += ['\n\n'.join(rng.sample(bodies, 4)) for _ in range(10)]           # long mixed files
    texts += ['', ' ', '\n', '﻿', 'x' * 5000, '[' * 300 + ']' * 300, '- ' * 2000]
    return [t.encode('utf-8') for t in texts] + [b'\xff\xfe invalid \xc3', b'\xe2\x80']


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
@pytest.mark.parametrize('march', ['x86-64', 'x86-64-v3'])   # scalar scans / the AVX2 scans (scan.h)
def test_host_library_under_asan_ubsan(tmp_path, march):
    from licensee_amd import content_helper as ch
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from licensee_amd.native_host import _FLAG_MASK, host_patterns, unicode_tables
    corpus = TemplateCorpus(License.all(hidden=True, pseudo=False))
    pats = host_patterns()
    fields, off = [], [0]
    for t in corpus.templates:
        fields.extend(sorted(set(t.fields_normalized())))
        off.append(len(fields))
    lf, lt, wl, wh = unicode_tables()
    T = len(corpus.templates)
    sig = np.zeros((corpus.n_vocab, 1), np.uint64)
    bits = np.unpackbits(corpus.lf_bits.view(np.uint8).reshape(T, -1), axis=1, bitorder='little')[:, :corpus.n_vocab]
    for t in range(T):
        sig[:, 0] |= bits[t].astype(np.uint64) << np.uint64(t)
    blob = (_strs(list(pats)) + _strs([p.pattern for p in pats.values()]) +
            _arr(np.array([p.flags & _FLAG_MASK for p in pats.values()], np.int32)) +
            _strs(list(ch.VARIETAL_WORDS)) + _strs(list(ch.VARIETAL_WORDS.values())) + _strs(corpus.vocab) +
            struct.pack('<I', T) + _arr(corpus.lf_bits) +
            _arr(np.array([len(t.wordset()) for t in corpus.templates], np.uint32)) +
            _arr(np.array(off, np.int32)) + _strs(fields) +
            _arr(lf) + _arr(lt) + _arr(wl) + _arr(wh) + _strs(_texts()) + _arr(sig) + struct.pack('<I', 1))
    inp = tmp_path / 'input.bin'
    inp.write_bytes(blob)
    exe = str(tmp_path / 'drv')
    csrc = os.path.join(ROOT, 'licensee_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', f'-march={march}', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-pthread', '-I', os.path.join(ROOT, 'include'), '-I', csrc,
                    '-o', exe, os.path.join(HERE, 'sanitize', 'driver.cpp'), os.path.join(csrc, 'rx.cpp'),
                    os.path.join(csrc, 'normalize.cpp'), os.path.join(csrc, 'vocab_pack.cpp')], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith('ok '), r.stdout
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]


# The sparse program's generator (csrc/dice_program_gen.cpp) under the same sanitizers:
# tests/sanitize/program_driver.cpp plans and emits the program for the full-bitset tile and for the
# compact tile with the VALU and the matrix-core match stage. The corpora are the shapes at which
# its index code can go wrong; every text must be what the shared library returns.

@pytest.fixture(scope='module')
def program_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('progdrv') / 'drv')
    csrc = os.path.join(ROOT, 'licensee_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I', csrc, '-o', exe, os.path.join(HERE, 'sanitize', 'program_driver.cpp'),
                    os.path.join(csrc, 'dice_program_gen.cpp')], check=True)
    return exe


def _program_corpus(name):
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.license import License
    from tests.helpers import ArrayCorpus
    from tests.test_gpu_corpus_sizes import corpus_of
    if name == 'vendored':
        return TemplateCorpus(License.all(hidden=True, pseudo=False))
    if name == 'nofields':   # test_corpus_without_count_fields: no count fields, V no multiple of 64
        T, V = 8, 255
        member = ((np.arange(1, V + 1)[None, :] >> np.arange(T)[:, None]) & 1).astype(np.uint8)
        pad = np.zeros((T, 256), np.uint8)
        pad[:, :V] = member
        size = member.sum(1).astype(np.uint32)
        return ArrayCorpus(np.packbits(pad, axis=1, bitorder='little').view(np.uint64), size, np.ones(T, np.uint32),
                           np.full(T, 5, np.int32), (size * 6).astype(np.int32), np.zeros(T, np.uint8), V)
    # 1: no bit region; 33: two 32-template tiles, the second nearly empty; 64: the most the program serves
    return TemplateCorpus(corpus_of(int(name)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
@pytest.mark.parametrize('name', ['vendored', '1', '33', '64', 'nofields'])
def test_program_generator_under_asan_ubsan(tmp_path, monkeypatch, program_driver, name):
    from tests.test_program_codegen import generated_source
    from tests.test_program_compact_codegen import compact_source
    c = _program_corpus(name)
    T = len(c.lf_size)
    arrays = [(c.lf_bits, np.uint64), (c.lf_size, np.uint32), (c.fields_set_size, np.uint32),
              (c.length_slack, np.int32), (c.length, np.int32), (c.is_cc, np.uint8)]
    inp = tmp_path / 'templates.bin'
    inp.write_bytes(struct.pack('<ii', T, c.n_vocab) +
                    b''.join(np.ascontiguousarray(a, dtype=dt).tobytes() for a, dt in arrays))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([program_driver, str(inp), str(tmp_path / 'prog')], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith('ok '), r.stdout
    assert r.stderr == '', r.stderr[-4000:]
    monkeypatch.delenv('DICE_PROG_DIAG', raising=False)
    monkeypatch.delenv('DICE_PROG_LAYOUT', raising=False)
    assert (tmp_path / 'prog.bits').read_bytes() == generated_source(c).encode()
    for match in ('valu', 'mfma'):
        monkeypatch.setenv('DICE_PROG_MATCH', match)
        assert (tmp_path / f'prog.{match}').read_bytes() == compact_source(c).encode()
