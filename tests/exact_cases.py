"""Matchers::Exact judged by set equality: a reference over Python frozensets, one encoder from sets
to the device's inputs, and two corpora built at the edges of dice_exact_kernel and dice_exact_setup.

Reference (exact.rb:6-12 and nothing more): for each file the first template in key order whose
wordset equals the file's, else -1. A word is
    an int < V        a vocabulary word (a bit of the bitset row);
    ('f', j)          a field word outside the vocabulary, bit j < 64 of the numbering of
                      licensee_host.h lh_template_field_masks;
    ('x', anything)   any other word: it only counts towards |W_F|;
    ('xs', n)         shorthand for n further distinct 'x' words (the file with |W_F| = 2^32 - 1).
A template is (Lf ⊆ V, fields), W_t = Lf ∪ fields; its fields are vocabulary words (field_bits) or
('f', j) words (field_need). The encoder asserts that contract.

Nothing here imports GPU code, oracle/ or another Exact test (envelope_cases supplies the bit packing,
corpus_from_sets and file_batch); the kernel's own vocabulary (records of 64 words, chunks of 64
records, size runs, lanes) appears only in how the inputs are laid out.
"""
from __future__ import annotations

import numpy as np

from tests import envelope_cases as E

WAVE = 64          # lanes per wave = records per pass of the record loop = files per wave
BLOCK = 256        # threads per workgroup of dice_exact_kernel
EDGE_BITS = (0, 31, 32, 63)
POSITIONS = (0, 62, 63, 64, 65, 127, 128)      # and each template's last record
BATCH_SIZES = (1, 63, 64, 65, 255, 256, 257, 700)


# ---- words, sets and the reference -------------------------------------------------------------

def is_vocab(w):
    return isinstance(w, (int, np.integer))


def wsize(W):
    """|W| with ('xs', n) counted as n words."""
    return sum(w[1] if (not is_vocab(w) and w[0] == 'xs') else 1 for w in W)


class Template:
    def __init__(self, name, lf, fields=()):
        self.name, self.lf, self.fields = name, frozenset(int(w) for w in lf), frozenset(fields)
        assert all(is_vocab(w) or (w[0] == 'f' and 0 <= w[1] < 64) for w in self.fields), name
        assert not (self.lf & self.fields), name

    @property
    def words(self):
        return self.lf | self.fields

    def retabled(self, fields):
        return Template(self.name, self.lf, fields)


def reference(templates, files):
    """exact.rb:6-12: potential_matches.find { |m| m.wordset == file.wordset }, as an index."""
    sets = [t.words for t in templates]
    out = np.full(len(files), -1, np.int32)
    for i, W in enumerate(files):
        for t, Wt in enumerate(sets):
            if Wt == W:
                out[i] = t
                break
    return out


def strip_fields(files):
    """The files as a call without field masks describes them: every ('f', j) is just another word."""
    return [frozenset(('x', w) if (not is_vocab(w) and w[0] == 'f') else w for w in W) for W in files]


# ---- the encoder and its inverse ---------------------------------------------------------------

def encode_files(V, files):
    """Sets -> (FileBatch, field_mask [n] uint64). Lengths and CC flags are inside the Dice input
    domain of encode_templates' constants (Exact ignores them)."""
    ids, wf, fm = [], [], []
    for W in files:
        row, m = [], 0
        for w in W:
            if is_vocab(w):
                assert 0 <= w < V
                row.append(int(w))
            elif w[0] == 'f':
                assert 0 <= w[1] < 64
                m |= 1 << w[1]
            else:
                assert w[0] in ('x', 'xs')
        ids.append(sorted(row))
        wf.append(wsize(W))
        fm.append(m)
    n = len(files)
    assert all(0 <= s < 2 ** 32 for s in wf)
    fb = E.file_batch(V, ids, wf, 10 + (np.arange(n) * 7) % 500, np.arange(n) % 11 == 3)
    return fb, np.array(fm, np.uint64)


def decode_files(V, fb, fm):
    """(FileBatch, masks) -> [(frozenset of vocabulary and field words, number of other words)]."""
    U = E.unpack(fb.bits, fb.bits.shape[1] * 64)
    assert not U[:, V:].any()
    out = []
    for i in range(fb.n):
        W = {int(w) for w in np.flatnonzero(U[i])} | {('f', j) for j in range(64) if int(fm[i]) >> j & 1}
        out.append((frozenset(W), int(fb.wordset_size[i]) - len(W)))
    return out


def split_file(W):
    """What decode_files returns for a file encoded from W."""
    known = frozenset(w for w in W if is_vocab(w) or w[0] == 'f')
    return known, wsize(W) - len(known)


def encode_templates(V, templates):
    """Templates -> (ArrayCorpus of the Lf rows, wordset_size [T], field_bits [T][w64], field_need [T]).
    The Dice constants keep every denominator of every file of encode_files in (0, 2^31): template
    lengths from 3,000, file lengths below 510, slack at most 40."""
    T, w64 = len(templates), (V + 63) // 64
    assert all(all(0 <= w < V for w in t.lf) for t in templates)            # the contract: Lf ⊆ V
    fld = [min(len(t.fields), len(t.lf)) for t in templates]
    corpus = E.corpus_from_sets(V, [t.lf for t in templates], fld, [(-1, 0, 5, 40)[t % 4] for t in range(T)],
                                [3000 + 37 * t for t in range(T)], [t % 13 == 5 for t in range(T)])
    B = np.zeros((T, w64 * 64), np.uint8)
    need = np.zeros(T, np.uint64)
    for t, tp in enumerate(templates):
        for w in tp.fields:
            if is_vocab(w):
                assert 0 <= w < V
                B[t, int(w)] = 1
            else:
                need[t] |= np.uint64(1 << w[1])
    ws = np.array([len(t.words) for t in templates], np.uint32)
    return corpus, ws, np.packbits(B, axis=1, bitorder='little').view(np.uint64), need


def decode_templates(V, corpus, ws, fbits, need):
    L, F = E.unpack(corpus.lf_bits, V), E.unpack(fbits, V)
    out = []
    for t in range(L.shape[0]):
        fields = {int(w) for w in np.flatnonzero(F[t])} | {('f', j) for j in range(64) if int(need[t]) >> j & 1}
        out.append((frozenset(int(w) for w in np.flatnonzero(L[t])), frozenset(fields), int(ws[t])))
    return out


def records(tp):
    """The u64 words of the row in which the template has a vocabulary word (Lf or field), ascending:
    record r of the template is the r-th of them."""
    return sorted({w // 64 for w in tp.words if is_vocab(w)})


class Corpus:
    """Templates in key order, files, and per file a dict that says why it is there."""

    def __init__(self, name, V, templates, files, meta, special=()):
        assert len(files) == len(meta)
        self.name, self.V, self.templates, self.files, self.meta = name, V, list(templates), list(files), list(meta)
        self.special = list(special)        # valid for Exact, outside the Dice input domain
        self._enc = None

    def index(self, name):
        return [t.name for t in self.templates].index(name)

    def encoded(self):
        if self._enc is None:
            self._enc = encode_templates(self.V, self.templates)
        return self._enc

    def pick(self, **kv):
        return [i for i, m in enumerate(self.meta) if all(m.get(k) == v for k, v in kv.items())]


# ---- 'chunks': the record loop -----------------------------------------------------------------

CHUNKS_V = 8320
REC_COUNTS = (0, 1, 63, 64, 65, 128, 129, 130)


def _record_template(k, rng):
    """A template with exactly k records over w64 = 130. Records at POSITIONS and the last one carry
    bits 0, 31, 32 and 63; every fifth other record three bits; every other fifth one Lf bit and one
    field bit; the rest one bit. Record 64 (k > 64) and the last record (k >= 65) come from
    field_bits alone."""
    name = f'r{k}'
    if k == 0:
        return Template(name, (), [('f', j) for j in EDGE_BITS])
    ps = sorted(int(p) for p in rng.choice(CHUNKS_V // 64, k, replace=False))
    edge = {r for r in POSITIONS if r < k} | {k - 1}
    field_only = ({64} if k > 64 else set()) | ({k - 1} if k >= 65 else set())
    lf, fields = set(), set()
    for r, p in enumerate(ps):
        if r in edge:
            bits, fbits = EDGE_BITS, ()
        elif r % 5 == 2:
            bits, fbits = tuple((7 * r + d) % 64 for d in (1, 14, 30)), ()
        elif r % 5 == 1:
            bits, fbits = ((11 * r + 5) % 64,), ((11 * r + 25) % 64,)
        else:
            bits, fbits = ((11 * r + 5) % 64,), ()
        if r in field_only:
            bits, fbits = (), bits
        lf |= {64 * p + b for b in bits}
        fields |= {64 * p + b for b in fbits}
    if k == 65:
        fields.add(('f', 63))
    if k == 129:
        fields |= {('f', 0), ('f', 32)}
    return Template(name, lf, fields)


def _near_misses(tp):
    """For every record of tp at POSITIONS or last: one file per word of the record with that word
    replaced by an 'x' word (same size), and, for a record of several words, one file that keeps a
    single word of it."""
    recs = records(tp)
    out = []
    for r in sorted({r for r in POSITIONS if r < len(recs)} | {len(recs) - 1}):
        p = recs[r]
        words = sorted(w for w in tp.words if is_vocab(w) and w // 64 == p)
        src = 'field' if all(w in tp.fields for w in words) else 'lf' if all(w in tp.lf for w in words) else 'both'
        for w in words:
            out.append((tp.words - {w} | {('x', (tp.name, r, w % 64))},
                        dict(kind='drop', of=tp.name, rec=r, word=p, bit=w % 64, src=src, multi=len(words) > 1)))
        if len(words) > 1:
            gone = words[:1] + words[2:]
            out.append((tp.words - set(gone) | {('x', (tp.name, r, 'p', j)) for j in range(len(gone))},
                        dict(kind='partial', of=tp.name, rec=r, word=p, src=src)))
    return out


def chunks() -> Corpus:
    """V = 8,320 (w64 = 130), T = 12 in shuffled key order: templates of 0, 1, 63, 64, 65, 128, 129 and
    130 records, a second 130-record template that differs from the first in its last record alone
    (same size: one size run, both past two full chunks), and the chain A ⊂ B ⊂ C of 10, 11, 12 words."""
    rng = np.random.default_rng(20250611)
    tps = [_record_template(k, rng) for k in REC_COUNTS]
    big = tps[-1]
    last = records(big)[-1]
    tps.append(Template('r130b', big.lf, big.fields - {64 * last + 63} | {64 * last + 62}))
    A = [8000 + 3 * i for i in range(10)]
    tps += [Template('A', A), Template('B', A + [8100]), Template('C', A + [8100], [8200])]
    tps = [tps[j] for j in rng.permutation(len(tps))]
    files, meta = [], []

    def add(W, **m):
        files.append(frozenset(W))
        meta.append(m)

    for tp in tps:
        add(tp.words, kind='own', of=tp.name)
        if tp.name.startswith('r') and tp.name != 'r0':
            for W, m in _near_misses(tp):
                add(W, **m)
    r0 = next(t for t in tps if t.name == 'r0')
    for j in EDGE_BITS:                       # the record-less template: only the need mask decides
        add(r0.words - {('f', j)} | {('x', ('r0', j))}, kind='need_drop', of='r0', bit=j)
    a, b, c = (next(t for t in tps if t.name == n).words for n in 'ABC')
    for n, W in (('A', a), ('B', b), ('C', c)):
        add(W | {('x', n)}, kind='chain', why='superset')
        add(W - {A[0]}, kind='chain', why='subset')
        add(W - {A[0]} | {('x', n)}, kind='chain', why='swap')
    add(a | {8200}, kind='chain', why='A plus the word of C, the size of B')
    add(b - {8100} | {8200}, kind='chain', why='the size of B, holds A')
    add(frozenset(), kind='empty')
    huge = frozenset({('xs', 2 ** 32 - 1)})
    return Corpus('chunks', CHUNKS_V, tps, files, meta, special=[huge, a, frozenset(), huge, big.words])


def padded(c: Corpus, T=65) -> Corpus:
    """c with filler templates up to T, the empty template (W = ∅) among them, in shuffled key
    order, and each filler's own wordset as a file."""
    rng = np.random.default_rng(65)
    fill = [Template(f'fill{j}', {(131 * j + 17 * i) % c.V for i in range(3 + j % 4)}) for j in range(T - len(c.templates) - 1)]
    fill.append(Template('empty', ()))
    tps = c.templates + fill
    assert len({t.words for t in tps}) == len(tps)
    tps = [tps[j] for j in rng.permutation(len(tps))]
    return Corpus(f'{c.name}{T}', c.V, tps, c.files + [t.words for t in fill],
                  c.meta + [dict(kind='own', of=t.name) for t in fill], special=c.special)


def retabled(c: Corpus) -> Corpus:
    """The same Lf rows under other Exact tables (a second dice_exact_setup on one context): a
    template with ('f', j) fields loses them, every other template gains ('f', (3 t + 1) % 64) and
    loses its vocabulary field words. Files: c's, then each new wordset."""
    tps = []
    for t, tp in enumerate(c.templates):
        had = any(not is_vocab(w) for w in tp.fields)
        tps.append(tp.retabled({w for w in tp.fields if is_vocab(w)} if had else {('f', (3 * t + 1) % 64)}))
    return Corpus(c.name + '_retabled', c.V, tps, c.files + [t.words for t in tps],
                  c.meta + [dict(kind='own2', of=t.name) for t in tps], special=c.special)


# ---- 'runs': the size runs and the need masks --------------------------------------------------

RUNS_V, RUNS_T = 640, 300
LONG_SIZE, LONG_RUN = 20, 70
DEPTHS = (1, 2, 3, 35, 70)
NEED_BITS = (0, 31, 32, 63)
GROUP_SIZES = (40, 50)
DUP_SIZE, LAST_SIZE = 30, 120


def runs() -> Corpus:
    """V = 640, T = 300 (more than the 256 threads that fill the sizes in LDS), key order shuffled so
    that a size run's key indices are scattered. Size runs:
      'min'    3 words, one template, the smallest size;
      'long'   20 words, 70 templates; every seventh needs one ('f', j), every fifth has two of its
               vocabulary words as fields;
      'dup'    30 words, 7 templates, the first, fourth and seventh identical;
      'g<s>'   for s = 40, 50: one Lf of s words as Gnone (s words), G1, G31, G32, G63 (s + 1: Lf and
               field 0 / 31 / 32 / 63, after H, another Lf of s + 1 words, in key order) and Gall
               (s + 64: every field);
      'last'   120 words, 6 templates, the largest size: the run that ends the sorted table;
      and runs of 1 to 8 templates at the sizes between."""
    rng = np.random.default_rng(300)
    seen = set()

    def fresh(name, size, need=(), nfield=0):
        while True:
            ids = [int(w) for w in rng.choice(RUNS_V, size - len(need), replace=False)]
            if frozenset(ids) not in seen:
                seen.add(frozenset(ids))
                return Template(name, ids[nfield:], ids[:nfield] + [('f', j) for j in need])

    run_list = [[fresh('min', 3)]]
    run_list.append([fresh(f'long{i}', LONG_SIZE, need=((5 * i) % 64,) if i % 7 == 3 else (), nfield=2 if i % 5 == 4 else 0)
                     for i in range(LONG_RUN)])
    d = fresh('dup0', DUP_SIZE)
    run_list.append([d if i % 3 == 0 else fresh(f'dup{i}', DUP_SIZE) for i in range(7)])
    run_list[-1] = [Template(f'dup{i}', t.lf, t.fields) for i, t in enumerate(run_list[-1])]
    for s in GROUP_SIZES:
        g0 = fresh(f'g{s}_none', s)
        run_list.append([g0])
        run_list.append([fresh(f'g{s}_H', s + 1)] + [Template(f'g{s}_{j}', g0.lf, [('f', j)]) for j in NEED_BITS])
        run_list.append([Template(f'g{s}_all', g0.lf, [('f', j) for j in range(64)])])
    run_list.append([fresh(f'last{i}', LAST_SIZE, need=(63,) if i == 2 else ()) for i in range(6)])
    left = RUNS_T - sum(len(r) for r in run_list)
    taken = {len(r[0].words) for r in run_list}
    sizes = [s for s in list(range(4, 40)) + list(range(52, 104)) if s not in taken]
    j = 0
    while left and j < len(sizes):
        k = min(left, 1 + (5 * j + 2) % 8)
        s = sizes[j]
        run_list.append([fresh(f's{s}_{i}', s, need=((j + i) % 64,) if (i + j) % 6 == 5 else (), nfield=1 if i % 4 == 3 else 0)
                         for i in range(k)])
        left -= k
        j += 1
    assert left == 0, left
    # key order: every run gets a random subset of the key indices, its members in the order given
    keys = [int(x) for x in rng.permutation(RUNS_T)]
    tps = [None] * RUNS_T
    for r in run_list:
        mine, keys = sorted(keys[:len(r)]), keys[len(r):]
        for k, tp in zip(mine, r):
            tps[k] = tp
    c = Corpus('runs', RUNS_V, tps, [], [])

    def add(W, **m):
        c.files.append(frozenset(W))
        c.meta.append(m)

    for tp in tps:
        add(tp.words, kind='own', of=tp.name)
    by = {t.name: t for t in tps}
    for dpt in DEPTHS:
        add(by[f'long{dpt - 1}'].words, kind='depth', depth=dpt)
    w10 = by['long10'].words
    add(w10 - {min(by['long10'].lf)} | {('x', 'long')}, kind='run_rejects', run='long')
    wl = by['last5'].words
    add(wl - {min(by['last5'].lf)} | {('x', 'last')}, kind='run_rejects', run='last')
    wm = by['min'].words
    add(wm - {min(by['min'].lf)} | {('x', 'min')}, kind='run_rejects', run='min')
    for s in GROUP_SIZES:
        lf = by[f'g{s}_none'].lf
        a = min(lf)
        for j in NEED_BITS:
            add(lf | {('f', j)}, kind='need', of=f'g{s}_{j}')
            # the mask holds more than any template of the run needs, the row one word too few
            add(lf - {a} | {('f', j), ('f', (j + 1) % 64)}, kind='fm_superset', s=s, bit=j)
            every = {('f', i) for i in range(64)}
            add(lf | every - {('f', j)} | {('x', j)}, kind='fm_lacks', s=s, bit=j)
        add(lf | {('x', 'nofield')}, kind='x_for_field', s=s)
        add(lf | {('f', 7)}, kind='other_field', s=s)
        add(lf | {('f', 0), ('f', 63)}, kind='fm_superset', s=s, bit=None)
    return c


# ---- placement ---------------------------------------------------------------------------------

def filler(c: Corpus, i):
    """A file whose size matches no template of c (its lane never has a candidate), with a row bit."""
    sizes = {len(t.words) for t in c.templates}
    k = 2
    while k in sizes:
        k += 1
    return frozenset({(7 * i) % c.V} | {('x', ('pad', j)) for j in range(k - 1)})


def place(c: Corpus, n, at):
    """n files: at[i] on index i (lane i % 64 of wave i // 64), fillers everywhere else."""
    assert all(0 <= i < n for i in at)
    return [at[i] if i in at else filler(c, i) for i in range(n)]


def placements(c: Corpus):
    """name -> files, for the `runs` corpus."""
    by = {t.name: t.words for t in c.templates}
    own = [t.words for t in c.templates]
    deep, first = by[f'long{LONG_RUN - 1}'], by['long0']
    lastpos = by['last5']
    out = {
        'lane0': place(c, WAVE, {0: deep}),
        'lane63': place(c, WAVE, {63: lastpos}),
        'all64': [own[(7 * i + 1) % len(own)] for i in range(WAVE)],
        'partial_last_wave': place(c, WAVE + 37, {WAVE + 36: deep}),
        'block_last_wave': place(c, BLOCK + 44, {192: by['g40_63'], 255: deep, 256: lastpos, BLOCK + 43: by['g50_all']}),
    }
    # one wave: most lanes retire on the long run's first candidate, a few on the 2nd, 3rd, 35th and
    # 70th, one after the whole run rejected
    mixed = {i: first for i in range(WAVE)}
    rej = c.files[c.pick(kind='run_rejects', run='long')[0]]
    mixed.update({5: deep, 6: by['long2'], 20: by['long34'], 21: by['long1'], 40: rej, 62: by['long2'], 63: deep})
    out['mixed_depths'] = place(c, WAVE, mixed)
    assert len({frozenset(W) for W in out['all64']}) >= WAVE - 2
    return out


def sized(c: Corpus, n):
    """n of c's files, every file before any repeats."""
    files = list(dict.fromkeys(c.files))
    m = len(files)
    step = next(s for s in range(m // 3, m) if np.gcd(s, m) == 1)
    return [files[(i * step) % m] for i in range(n)]


# ---- texts for the device wordset scan ---------------------------------------------------------

def vocabulary(V):
    return [f'v{i}' for i in range(V)], [f'f{j}' for j in range(64)]


def texts_of(files):
    """Space-joined ASCII texts (uint8 text, offsets, text_len) whose wordsets are the files."""
    names = {}
    raw = []
    for W in files:
        ws = []
        for w in sorted(W, key=repr):
            if is_vocab(w):
                ws.append(f'v{w}')
            elif w[0] == 'f':
                ws.append(f'f{w[1]}')
            else:
                assert w[0] == 'x'
                ws.append('x' + str(names.setdefault(w, len(names))))
        raw.append(' '.join(ws).encode('ascii'))
    off = np.cumsum([0] + [(len(r) + 15) // 16 * 16 for r in raw]).astype(np.int64)
    text = np.zeros(max(int(off[-1]), 16), np.uint8)
    for r, o in zip(raw, off):
        text[o:o + len(r)] = np.frombuffer(r, np.uint8)
    return text, off[:-1].copy(), np.array([len(r) for r in raw], np.int32)
