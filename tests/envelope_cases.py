"""Inputs that sit on the last value inside, and the first value outside, every range that decides
which compare path or which kernel a file or a corpus takes, and a plain reference to judge them by.

The ranges ("Results are bit-exact"):
  file side      |W_F| < 2^20 and 0 <= len_F < 2^21: the exact rational compare, else IEEE doubles;
  corpus side    1 <= base < 2^18, template length < 2^20, 200 |Lf| < 1024 base (CORPUS_FAST, post_fast);
                 max |Lf| < 2^11 (NARROW_MUL, post_fast, dice_wave.h ge<true>);
  kernel choice  post_feasible (|Lf| < 65535, base <= 65535, slack in int16); the pruned kernel's
                 deferral of |W_F| >= 2^28; dice_pack_compact's LDS staging up to w64 = 127.

Nothing here imports oracle/ or reads the kernels: `Reference` restates the operation in Python
integers and floats (content_helper.rb:128-133, 337-347; dice.rb:23-53), the corpora are numpy
bit matrices whose overlaps follow from how the word blocks were laid out.
"""
from __future__ import annotations

from math import gcd

import numpy as np

from tests.helpers import ArrayCorpus

P20, P21, P28 = 1 << 20, 1 << 21, 1 << 28
WF_EDGES = (P20 - 1, P20, P28 - 1, P28)
LEN_EDGES = (0, P20 - 1, P21 - 1, P21, (1 << 31) - 1)


def unpack(bits, V):
    """[n][w64] uint64 bitsets -> [n][V] uint8."""
    return np.unpackbits(np.ascontiguousarray(bits, np.uint64).view(np.uint8), axis=1, bitorder='little')[:, :V]


def file_batch(V, word_lists, wf, length, cc):
    from licensee_amd._native import FileBatch
    w64 = (V + 63) // 64
    B = np.zeros((len(word_lists), w64 * 64), np.uint8)
    for i, ws in enumerate(word_lists):
        B[i, np.asarray(ws, np.int64)] = 1
    return FileBatch(np.packbits(B, axis=1, bitorder='little').view(np.uint64), np.asarray(wf, np.uint32),
                     np.asarray(length, np.int32), np.asarray(cc, np.uint8))


def head(fb, n):
    from licensee_amd._native import FileBatch
    return FileBatch(fb.bits[:n], fb.wordset_size[:n], fb.length[:n], fb.cc_false_positive[:n])


def take(fb, idx):
    from licensee_amd._native import FileBatch
    idx = np.asarray(idx, np.int64)
    return FileBatch(fb.bits[idx], fb.wordset_size[idx], fb.length[idx], fb.cc_false_positive[idx])


def corpus_from_sets(V, sets, fld, slack, length, cc) -> ArrayCorpus:
    """Templates given as word-id sets; |Lf| is the set's size."""
    T, w64 = len(sets), (V + 63) // 64
    B = np.zeros((T, w64 * 64), np.uint8)
    for t, ws in enumerate(sets):
        ws = np.asarray(sorted(ws), np.int64)
        assert ws.size == 0 or (0 <= ws[0] and ws[-1] < V)
        B[t, ws] = 1
    return ArrayCorpus(np.packbits(B, axis=1, bitorder='little').view(np.uint64), B.sum(1), fld, slack, length, cc, V)


# ---- the plain reference -----------------------------------------------------------------------

class Reference:
    """Every (file, template) pair in Python integers and floats:
        ov    = words the two unpacked bit rows share
        den   = |Lf| - |Fld| + |W_F| + adj // 4,  adj = d if slack < 0 else max(d - slack, 0),
                d = |len_t - len_F|
        score = (ov * 200.0) / den
    The input domain is 0 < den < 2^31 for every pair, asserted here."""

    def __init__(self, corpus, fb):
        V = corpus.n_vocab
        M = unpack(corpus.lf_bits, V)
        F = unpack(fb.bits, V)
        self.n, self.T = F.shape[0], M.shape[0]
        self.cc_t = [bool(x) for x in corpus.is_cc]
        self.cc_f = [bool(x) for x in fb.cc_false_positive]
        self.ov, self.den, self.score = [], [], []
        for i in range(self.n):
            words = np.flatnonzero(F[i])
            row = [int(x) for x in M[:, words].sum(1, dtype=np.int64)]
            wf, len_f = int(fb.wordset_size[i]), int(fb.length[i])
            assert len_f >= 0
            dens = []
            for t in range(self.T):
                slack = int(corpus.length_slack[t])
                d = abs(int(corpus.length[t]) - len_f)
                adj = d if slack < 0 else max(d - slack, 0)
                den = int(corpus.lf_size[t]) - int(corpus.fields_set_size[t]) + wf + adj // 4
                assert 0 < den < 2 ** 31, (i, t, den)
                dens.append(den)
            self.ov.append(row)
            self.den.append(dens)
            self.score.append([(o * 200.0) / d for o, d in zip(row, dens)])

    def candidates(self, i):
        return [t for t in range(self.T) if not (self.cc_t[t] and self.cc_f[i])]

    def top(self, i):
        best = -1
        for t in self.candidates(i):
            if best < 0 or self.score[i][t] >= self.score[i][best]:   # the later key takes a tie
                best = t
        return best

    def match(self, thr, confidence=False):
        """(best, overlap, score) of dice_match, or of dice_match_confidence."""
        best = np.full(self.n, -1, np.int32)
        ov = np.zeros(self.n, np.uint32)
        score = np.zeros(self.n, np.float64)
        for i in range(self.n):
            b = self.top(i)
            if b < 0:
                continue
            hit = self.score[i][b] >= thr
            best[i] = b if hit else -1
            if hit or not confidence:
                ov[i], score[i] = self.ov[i][b], self.score[i][b]
        return best, ov, score

    def matrix(self):
        return np.array(self.ov, np.uint32).reshape(self.n, self.T), np.array(self.score, np.float64).reshape(self.n, self.T)

    def ranked(self, i):
        return sorted(self.candidates(i), key=lambda t: (self.score[i][t], t), reverse=True)

    def topk(self, k):
        tki = np.full((self.n, k), -1, np.int32)
        tks = np.full((self.n, k), -1.0, np.float64)
        for i in range(self.n):
            r = self.ranked(i)[:k]
            tki[i, :len(r)] = r
            tks[i, :len(r)] = [self.score[i][t] for t in r]
        return tki, tks


# ---- corpora -----------------------------------------------------------------------------------

class Case:
    """A corpus, the templates whose own word sets become files, and what the limits prescribe."""

    def __init__(self, name, corpus, edges, **expect):
        self.name, self.corpus, self.edges, self.expect = name, corpus, edges, expect


def _span(a, b):
    return list(range(a, b))


def lf_case(L, T=6, variant=None) -> Case:
    """The largest template holds exactly L words (2,047: the last corpus whose compares run in 24-bit
    multiplies; 2,048: the first that needs 64-bit products); the twins differ in word 2047 alone.
    Template 'edge' has |Lf| = 1024 and |Fld| = 823, so base = 201 and 200 |Lf| = 204,800 <
    1024 base = 205,824 by the smallest margin a base allows, and length 2^20 - 1; 'zero' has length
    0. variant 'base200': |Fld| = 824, base = 200, 204,800 = 204,800 -- outside. variant 'len20':
    the edge template's length is 2^20 -- outside. T = 65 adds 59 small templates and spreads the six
    over both 64-template groups."""
    assert L in (2047, 2048) and T in (6, 65) and variant in (None, 'base200', 'len20')
    small = ('edge', 'zero', 'cc', 'wide', 'tail')
    size = {'edge': 1024, 'zero': 30, 'cc': 300, 'wide': 530, 'tail': 170}
    start = {'edge': 1000, 'zero': 0, 'cc': 200, 'wide': 400, 'tail': 1900}
    # words 2048-2199: 30 per small template, its own except that each one's last five also belong
    # to other small templates in a combination no other word has (classes of one word: the bit
    # region of the compact tile, the matrix-core stage's input); 2198 and 2199 are 'tail' alone
    sets = {k: set(_span(2048 + 30 * j, 2048 + 30 * j + (20 if k == 'zero' else 30))) for j, k in enumerate(small)}
    sets['tail'] |= {2198, 2199}
    combo = 1
    for j, k in enumerate(small):
        for w in _span(2048 + 30 * j + 15, 2048 + 30 * j + 20):
            others = [o for o in small if o != k]
            for b in range(4):
                if combo >> b & 1 and len(sets[others[b]]) < size[others[b]]:
                    sets[others[b]].add(w)
            combo = combo % 15 + 1
    for k in small:                                  # the rest of each set is a run of the big one's words
        need = size[k] - len(sets[k])
        assert need >= 0 and start[k] + need <= 2040
        sets[k] |= set(_span(start[k], start[k] + need))
    sets['big'] = set(_span(0, L))
    assert [len(sets[k]) for k in small] == [1024, 30, 300, 530, 170]
    const = {   # |Fld|, slack, length, cc
        'big': (3, 15, 12000, 0),
        'edge': (824 if variant == 'base200' else 823, -1, P20 if variant == 'len20' else P20 - 1, 0),
        'zero': (1, 0, 0, 0),
        'cc': (2, 5, 1800, 1),
        'wide': (4, 2000, 3100, 0),
        'tail': (3, -1, 1000, 0),
    }
    if T == 6:
        order, V = ['big', 'edge', 'zero', 'cc', 'wide', 'tail'], 2200
    else:
        V = 2200 + 59 * 6
        pos = {0: 'zero', 13: 'wide', 31: 'cc', 47: 'tail', 63: 'edge', 64: 'big'}
        order, f = [], 0
        for t in range(65):
            if t in pos:
                order.append(pos[t])
                continue
            name = f'f{f}'
            sets[name] = _span(2200 + 6 * f, 2206 + 6 * f) + [10 + 3 * f, 11 + 3 * f]
            const[name] = (1, (-1, 0, 5, 40)[f % 4], 50 + 7 * f, 1 if f == 20 else 0)
            order.append(name)
            f += 1
    c = corpus_from_sets(V, [sets[k] for k in order], *zip(*[const[k] for k in order]))
    assert int(c.lf_size.max()) == L
    in_fast = variant is None
    return Case(f'lf{L}' + (f'_{variant}' if variant else '') + ('_T65' if T == 65 else ''), c,
                [order.index(k) for k in ('big', 'edge', 'zero')],
                narrow_mul=int(L < 2048), corpus_fast=int(in_fast), post_fast=in_fast and L < 2048)


def base18_case(inside: bool) -> Case:
    """T = 3, V = 2^18 + 300. Template 0 holds 2^18 + 100 words; |Fld| = 101 puts its base on
    2^18 - 1, the last inside the envelope, |Fld| = 100 on 2^18. w64 = 4101: dice_pack_compact reads
    the rows from global memory."""
    n0 = (1 << 18) + 100
    V = (1 << 18) + 300
    sets = [_span(0, n0), _span(1 << 18, (1 << 18) + 200), _span(0, 50) + _span(n0 + 100, V)]
    c = corpus_from_sets(V, sets, (101 if inside else 100, 1, 0), (10, -1, 0), (900000, 1200, 700), (0, 1, 0))
    assert int(c.lf_size[0]) - int(c.fields_set_size[0]) == (1 << 18) - (1 if inside else 0)
    return Case('base18_in' if inside else 'base18_out', c, [0, 2], narrow_mul=0, corpus_fast=int(inside))


def pack_case(V) -> Case:
    """T = 5 over about 300 words spread from word 0 to word V - 1; every other vocabulary word is in
    no template. V = 8,128 is the last size dice_pack_compact stages through LDS (w64 = 127,
    64 * 255 * 4 = 65,280 bytes), V = 8,129 the first it reads from global memory."""
    ids = np.unique(np.rint(np.linspace(0, V - 1, 300)).astype(np.int64))
    sets = [set(ids[t::5].tolist()) for t in range(5)]
    for j, w in enumerate(ids[::10].tolist()):
        sets[(j + 1) % 5].add(w)
        sets[(j + 3) % 5].add(w)
    assert any(V - 1 in s for s in sets) and any(0 in s for s in sets)
    c = corpus_from_sets(V, sets, (1, 2, 0, 3, 1), (-1, 0, 25, 300, -1), (400, 0, 2500, P20 - 1, 900), (0, 0, 1, 0, 0))
    return Case(f'pack{V}', c, [0, 2, 4], narrow_mul=1, corpus_fast=1)


def post_case(kind) -> Case:
    """T = 65, V = 65,700, at post_feasible's limits. 'in': a template of 65,534 words without
    fields (overlap and base 65,534, the largest the postings kernels take) and one with slack
    32,767. 'lf': that template has 65,535 words. 'slack': 32,768. 'base65535' / 'base65536': a
    template of 65,600 words with 65 / 64 fields. A base of 65,535 needs |Lf| >= 65,535 because
    |Fld| >= 0, so both base corpora are infeasible by their |Lf| already: the base limit cannot be
    reached from inside, and the last feasible base is the 65,534 of 'in'."""
    assert kind in ('in', 'lf', 'slack', 'base65535', 'base65536')
    V = 65700
    nbig = {'in': 65534, 'lf': 65535, 'slack': 65534, 'base65535': 65600, 'base65536': 65600}[kind]
    fbig = {'base65535': 65, 'base65536': 64}.get(kind, 0)
    sets = {40: _span(0, nbig), 7: _span(100, 600), 22: _span(300, 420)}
    const = {40: (fbig, 12, 300000, 0), 7: (5, 32768 if kind == 'slack' else 32767, 200000, 0), 22: (2, -1, 900, 1)}
    f = 0
    for t in range(65):
        if t in sets:
            continue
        sets[t] = _span(65576 + 2 * f, 65578 + 2 * f) + _span(1000 + 5 * f, 1005 + 5 * f)
        const[t] = (1, (-1, 0, 5, 32767)[f % 4], 60 + 11 * f, 0)
        f += 1
    assert max(sets[64]) == V - 1
    c = corpus_from_sets(V, [sets[t] for t in range(65)], *zip(*[const[t] for t in range(65)]))
    return Case('post_' + kind, c, [40, 7], kernel_kind=3 if kind == 'in' else 2)


# ---- the file grid -----------------------------------------------------------------------------

def is_fast(wf, length):
    return wf < P20 and 0 <= length < P21


def grid(case: Case, seed=7, limit=None):
    """Word patterns x |W_F| x len_F x CC flag, ordered so that files 0-63 are inside the fast envelope
    (one whole wave on the exact rational compare), file 64 is outside (the slow file of the first
    65's partial tile), the following waves mix both kinds and the last file, in a partial tile, is
    outside. `limit` keeps the first 64 and an even sample of the rest."""
    c = case.corpus
    V = c.n_vocab
    M = unpack(c.lf_bits, V)
    rng = np.random.default_rng(seed)
    patterns = [np.arange(V)] + [np.flatnonzero(M[t]) for t in case.edges]
    patterns += [np.zeros(0, np.int64), np.flatnonzero(rng.random(V) < 1 / 3), np.array([V - 1])]
    assert M[:, V - 1].any()
    fast, slow = [], []
    for p, words in enumerate(patterns):
        j = 0
        for wf in (words.size,) + WF_EDGES:
            for ln in LEN_EDGES:
                for cc in (0, 1):
                    f = (j, p, max(wf, words.size), ln, cc)
                    (fast if is_fast(f[2], ln) else slow).append(f)
                    j += 1
    # round-robin over the patterns; the fast files nearest the cuts (|W_F| = 2^20 - 1, len_F = 2^21 - 1,
    # whose products pass 2^31) come first, so they are inside the all-fast wave
    fast.sort(key=lambda f: (-f[0], f[1]))
    slow.sort()
    assert len(fast) >= 64
    rest, extra = slow[:1], fast[64:]
    for j, f in enumerate(slow[1:]):
        rest.append(f)
        if j % 4 == 1 and extra:
            rest.append(extra.pop(0))
    rest[-1:-1] = extra
    if limit is not None:
        keep = np.unique(np.rint(np.linspace(0, len(rest) - 1, limit - 64)).astype(np.int64))
        rest = [rest[j] for j in keep]
    order = fast[:64] + rest
    n = len(order)
    kinds = [is_fast(f[2], f[3]) for f in order]
    assert all(kinds[:64]) and not kinds[64] and not kinds[-1] and n % 64
    assert any(0 < sum(kinds[a:a + 64]) < len(kinds[a:a + 64]) for a in range(64, n, 64))
    assert {f[1] for f in order[:64]} == set(range(len(patterns)))
    return file_batch(V, [patterns[f[1]] for f in order], [f[2] for f in order], [f[3] for f in order],
                      [f[4] for f in order])


def cut_waves(fb):
    """From a grid: a wave of 63 fast files and one with |W_F| = 2^20 (len_F inside), a wave of 63 fast
    files and one with len_F = 2^21 (|W_F| inside), and a partial all-fast tile. One lane one step
    past each cut sends its whole wave to the IEEE-double body: two of the three waves. The
    denominators of these two files still fit 21 bits, so only the vote -- which the host form of the
    generated program reports -- tells on which side of the cut the kernel put them."""
    wf, ln = fb.wordset_size.astype(np.int64), fb.length.astype(np.int64)
    assert all(is_fast(wf[i], ln[i]) for i in range(64))
    a = int(np.flatnonzero((wf == P20) & (ln < P21))[0])
    b = int(np.flatnonzero((ln == P21) & (wf < P20))[0])
    return take(fb, list(range(63)) + [a] + list(range(63)) + [b] + list(range(10))), 2


# ---- near-ties and ties of unequal terms -------------------------------------------------------

TIE_SIZES = (2047, 2039, 2027, 2011)
TIE_FLD = (7, 11, 13, 17)
TIE_LEN = (1000, P20 - 1, 300000, 700000)


def tie_case(T=4) -> Case:
    """Four templates over disjoint word blocks, slack -1, distinct lengths: a file that takes ov_t
    words of block t reaches any (ov_t, den_t) through |W_F| and len_F. T = 65 puts them at indices
    3, 20, 41 and 64 among templates the tie files share no word with."""
    assert T in (4, 65)
    starts = np.concatenate([[0], np.cumsum(TIE_SIZES)])
    blocks = [_span(int(starts[j]), int(starts[j + 1])) for j in range(4)]
    V0 = int(starts[4])
    if T == 4:
        c = corpus_from_sets(V0, blocks, TIE_FLD, (-1,) * 4, TIE_LEN, (0,) * 4)
        c.tie_pos = [0, 1, 2, 3]
    else:
        pos = [3, 20, 41, 64]
        sets, const, f = [], [], 0
        for t in range(65):
            if t in pos:
                j = pos.index(t)
                sets.append(blocks[j])
                const.append((TIE_FLD[j], -1, TIE_LEN[j], 0))
            else:
                sets.append(_span(V0 + 6 * f, V0 + 6 * f + 6))
                const.append((0, (-1, 0, 5, 40)[f % 4], 40 + 9 * f, 1 if f == 9 else 0))
                f += 1
        c = corpus_from_sets(V0 + 61 * 6, sets, *zip(*const))
        c.tie_pos = pos
    c.tie_blocks = blocks
    return Case('ties' + ('_T65' if T == 65 else ''), c, [], narrow_mul=1, corpus_fast=1, post_fast=True)


def _solve(a, b, den_a, den_b, ov_a, ov_b):
    """(|W_F|, len_F) inside the fast envelope that give tie templates a and b the denominators
    den_a and den_b, or None. den_t = base_t + |W_F| + |len_t - len_F| // 4 (slack -1)."""
    base = [s - f for s, f in zip(TIE_SIZES, TIE_FLD)]
    want = (den_a - den_b) - (base[a] - base[b])
    f = lambda x: abs(TIE_LEN[a] - x) // 4 - abs(TIE_LEN[b] - x) // 4
    lo, hi = sorted((TIE_LEN[a], TIE_LEN[b]))
    up = f(hi) >= f(lo)                              # f is monotone between the two lengths
    if not min(f(lo), f(hi)) <= want <= max(f(lo), f(hi)):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if (f(mid) < want) == up:
            lo = mid + 1
        else:
            hi = mid
    for x in (lo - 1, lo, lo + 1):
        if 0 <= x < P21 and f(x) == want:
            wf = den_a - base[a] - abs(TIE_LEN[a] - x) // 4
            if ov_a + ov_b <= wf < P20:
                assert base[b] + wf + abs(TIE_LEN[b] - x) // 4 == den_b
                return wf, x
    return None


def _tie_file(blocks, a, b, ov_a, ov_b, flip):
    wa = blocks[a][-ov_a:] if flip else blocks[a][:ov_a]
    wb = blocks[b][:ov_b] if flip else blocks[b][-ov_b:]
    return wa + wb


def tie_files(case: Case, n_near=200, n_equal=50):
    """n_near files whose two best templates have |ov_a den_b - ov_b den_a| = 1 and n_equal files
    whose two best have equal scores from unequal (ov, den), all inside the fast envelope with both
    denominators above 2^20; in half of each set the better (the larger-termed) template has the
    lower index. Found by a deterministic search: for coprime overlaps the pairs (den_a, den_b)
    with cross-difference s form one arithmetic progression, and _solve turns a pair into
    (|W_F|, len_F). Returns (FileBatch, [(a, b, s)]) with a < b tie-template numbers and s = +1
    (a ranks first), -1 (b ranks first) or 0 (equal scores: the later index b ranks first)."""
    blocks = case.corpus.tie_blocks
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    files, meta = [], []

    def add(a, b, s, ov_a, ov_b, den_a, den_b):
        got = _solve(a, b, den_a, den_b, ov_a, ov_b)
        if got is None:
            return False
        sa, sb = (ov_a * 200.0) / den_a, (ov_b * 200.0) / den_b
        assert ov_a * den_b - ov_b * den_a == s and min(den_a, den_b) > P20
        assert (sa > sb) if s > 0 else (sa < sb) if s < 0 else (sa == sb and (ov_a, den_a) != (ov_b, den_b))
        files.append((_tie_file(blocks, a, b, ov_a, ov_b, len(files) % 2 == 1), got[0], got[1]))
        meta.append((a, b, s))
        return True

    want = {+1: n_near // 2, -1: n_near - n_near // 2}
    it = 0
    for g in range(1, 400):
        for ov_b in range(2011, 900, -37):
            a, b = pairs[it % len(pairs)]
            s = +1 if want[+1] >= want[-1] else -1
            it += 1
            for ov_a in (ov_b - g, ov_b + g):
                if not (0 < ov_a <= TIE_SIZES[a] and ov_b <= TIE_SIZES[b] and gcd(ov_a, ov_b) == 1 and want[s]):
                    continue
                # ov_a den_b - ov_b den_a = s: den_b = d0 (mod ov_b)
                d0 = (s * pow(ov_a, -1, ov_b)) % ov_b
                j0 = (P20 + 1 + max(ov_a, ov_b) - d0) // ov_b + 1
                for j in range(j0, j0 + 400, 7):
                    den_b = d0 + j * ov_b
                    den_a = (ov_a * den_b - s) // ov_b
                    if den_a > P20 and add(a, b, s, ov_a, ov_b, den_a, den_b):
                        want[s] -= 1
                        break
        if not (want[+1] or want[-1]):
            break
    assert not (want[+1] or want[-1]), want
    # equal scores: (p m, p e) against (q m, q e)
    left, it = n_equal, 0
    for p, q in ((8, 7), (9, 8), (10, 9), (11, 10), (13, 12), (15, 14), (16, 15), (17, 16), (19, 18), (21, 20)):
        for m in range(40, 96, 3):
            for e in range(P20 // min(p, q) + 1000, P20 // min(p, q) + 40000, 3571):
                if not left:
                    break
                a, b = pairs[it % len(pairs)]
                it += 1
                pp, qq = (p, q) if left % 2 else (q, p)          # the larger terms at the lower index, or not
                if pp * m <= TIE_SIZES[a] and qq * m <= TIE_SIZES[b] and add(a, b, 0, pp * m, qq * m, pp * e, qq * e):
                    left -= 1
    assert not left, left
    V = case.corpus.n_vocab
    return file_batch(V, [f[0] for f in files], [f[1] for f in files], [f[2] for f in files], [0] * len(files)), meta
