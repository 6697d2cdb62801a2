"""Project#license on the device (dice_batch_projects; projects/project.rb:24-47,102-106,137-155).

Files whose per-file result is known by construction -- a template's own wordset (Exact and Dice
give that template), half of it or nothing ('other'), a Copyright flag ('no-license'), a Creative
Commons template's wordset with the CC flag (Exact gives it, Dice filters it) -- go through the real
upload / Exact / match at threshold 98. The *downloaded* per-file exact / best and the flags are then
given to tests/project_oracle.py, the list-based, ordered restatement of project.rb, and all four
outputs of the kernel (the order-free form) are compared with it exactly:
  - P = 1, 63, 64, 65 and 4,097 over the same resident files; project sizes 0, 1, 2, 3, 8, 9 (each
    side of the lane / wave cut), 31, 32, 33, 64, 65 and 1,000 in one batch; empty projects first,
    last and consecutive; the last project ending at n;
  - every lgpl? row for two files, GPL + LGPL + MIT, prioritize_lgpl with the lesser file third and
    deep inside a 1,000-file project, only copyright? files, a COPYRIGHT name without the matcher, a
    LICENSE with it, k_licenses 0 / 1 / 4 / 8, more than 8 distinct licenses;
  - the vendored T = 47 corpus and a T = 600 one (license ids and the LDS bitset past 64);
  - use_exact 0 against 1; the state and argument errors;
  - BatchDetector.detect_projects on the 52 fixture projects against projects.Project.
"""
import json
import os

import numpy as np
import pytest

from licensee_amd.license import License
from tests import project_oracle as PO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
SIZES = (0, 1, 2, 3, 8, 9, 31, 32, 33, 64, 65, 1000)


class Ctx:
    """A corpus on the device with Exact tables of the templates' own wordsets, and one resident
    batch of constructed files with their downloaded per-file results."""

    def __init__(self, corpus, seed):
        from licensee_amd._native import FileBatch, Scorer
        from licensee_amd.project_files import LicenseFile, is_copyright_file
        c = self.c = corpus
        T = self.T = len(c.lf_size)
        self.sc = Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, c.n_vocab, device=0)
        self.sc.exact_setup(c.lf_size, np.zeros_like(c.lf_bits), np.zeros(T, np.uint64))
        rng = self.rng = np.random.default_rng(seed)
        cc = np.flatnonzero(c.is_cc)
        plain = np.flatnonzero(c.is_cc == 0)
        g, l, m = (int(x) for x in plain[[len(plain) // 3, len(plain) // 2, len(plain) - 1]])   # past 64 when T is
        self.glm = (g, l, m)
        few = [int(x) for x in plain[:5]] + [g, l]
        L, N, CL, X = 'LICENSE', 'COPYING', 'COPYING.lesser', 'COPYRIGHT'
        S = lambda t: ('self', t)
        pr = []       # projects: lists of (name, kind, copyright matched)
        # every two-file combination of {GPL, LGPL, MIT} x {LICENSE, COPYING, COPYING.lesser}: the lgpl? table
        for na in (L, N, CL):
            for nb in (L, N, CL):
                for ta in (g, l, m):
                    for tb in (g, l, m):
                        pr.append([(na, S(ta), 0), (nb, S(tb), 0)])
        for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            three = [(L, S(g), 0), (CL, S(l), 0), ('LICENSE-MIT', S(m), 0)]
            pr.append([three[i] for i in perm])
        pr.append([(L, S(g), 0), ('LICENSE-MIT', S(m), 0), (CL, S(l), 0)])                        # lesser third
        pr.append([(L, S(g), 0), (CL, S(m), 0), ('LICENSE-MIT', S(m), 0), (CL, S(l), 0), (CL, S(l), 0)])
        pr.append([(L, S(m), 0), (CL, S(l), 0), (N, S(g), 0)])                                    # first is not GPL
        pr.append([(L, S(g), 0), (CL, ('half', l), 0), (CL, ('empty', 0), 0)])                    # no valid lesser file
        pr += [[(X, ('empty', 0), 1)], [(X, ('empty', 0), 1), ('COPYRIGHT.txt', ('empty', 0), 1)]]    # only copyright? files
        pr += [[(X, S(m), 0)], [(X, S(m), 0), (L, S(few[0]), 0)], [(X, ('empty', 0), 1), (L, S(m), 0)]]
        pr += [[(L, ('empty', 0), 1)], [(L, ('empty', 0), 1), ('LICENSE-MIT', S(m), 0)], [('COPYRIGHT-BSD', ('empty', 0), 1), (L, S(m), 0)]]
        pr += [[(L, ('half', m), 0)], [(L, ('empty', 0), 0)], [(L, ('half', m), 0), (N, ('empty', 0), 0)]]
        for t in cc[:2]:
            pr += [[(L, ('cc', int(t)), 0)], [(L, ('cc', int(t)), 0), (N, S(m), 0)]]
        distinct = [int(x) for x in plain[:24] if x not in (g, l, m)][:20]
        pr.append([(L, S(t), 0) for t in distinct[:8]])                                          # 8 distinct: the lane path
        pr.append([(L, S(t), 0) for t in distinct[:9]] + [(L, S(distinct[0]), 0)])                # 9 distinct: the wave path
        pr.append([(L, S(t), 0) for t in distinct[:12]] + [(L, ('half', m), 0), (X, ('empty', 0), 1)])   # 14 distinct
        big = [(L, S(g), 0)] + [(N, S(few[i % 3]), 0) for i in range(999)]                        # 1,000 files, lesser at 700
        big[700] = (CL, S(l), 0)
        big[800] = (CL, S(l), 0)
        pr.append(big)
        edge = [(L, S(g), 0)] + [(N, S(g), 0)] * 64                                               # lesser in the second 64-file step
        edge[64] = (CL, S(l), 0)
        pr.append(edge)
        names = [L, N, CL, X, 'COPYRIGHT.md', 'LICENSE-MIT']

        def rand_file():
            r = rng.random()
            kind = S(int(rng.choice(few))) if r < 0.7 else ('half', int(rng.choice(few))) if r < 0.8 else \
                ('empty', 0) if r < 0.9 else ('cc', int(rng.choice(cc[:2])))
            return (str(rng.choice(names)), kind, int(rng.random() < 0.15))
        pr.insert(0, [])                                                                          # an empty project first
        for s in SIZES + (0, 0, 5, 0):
            pr.append([rand_file() for _ in range(s)])
        pr.append([rand_file() for _ in range(1000)])
        pr += [[(L, S(m), 0)] * 1000, [], []]                                                     # one license; empty last
        self.projects = pr
        flat = [f for p in pr for f in p]
        n = self.n = len(flat)
        self.offsets = np.cumsum([0] + [len(p) for p in pr]).astype(np.int64)
        bits = np.zeros((n, c.w64), np.uint64)
        wf, ln, ccf = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        for i, (_, (kind, t), _) in enumerate(flat):
            if kind in ('self', 'cc'):
                bits[i], wf[i], ln[i], ccf[i] = c.lf_bits[t], c.lf_size[t], c.length[t], kind == 'cc'
            elif kind == 'half':
                row = np.unpackbits(c.lf_bits[t].view(np.uint8), bitorder='little')
                on = np.flatnonzero(row)
                row[on[::2]] = 0
                bits[i] = np.packbits(row, bitorder='little').view(np.uint64)
                wf[i], ln[i] = int(row.sum()), c.length[t] // 2
        self.names = [f[0] for f in flat]
        self.copyright = np.array([f[2] for f in flat], np.uint8)
        self.flags = self.copyright | np.array([(2 if is_copyright_file(nm) else 0) | (4 if LicenseFile.lesser_gpl_score(nm) else 0)
                                                for nm in self.names], np.uint8)
        self.b = self.sc.batch(n)
        self.b.upload(FileBatch(bits, wf, ln, ccf))
        self.b.exact(None)
        self.b.match(98.0, confidence=True)
        self.exact = self.b.download_exact()
        self.best, _, self.score = self.b.download_match()
        # what the files were built to give
        kinds = np.array([f[1][0] for f in flat])
        want = np.array([f[1][1] for f in flat])
        own = kinds == 'self'
        assert np.array_equal(self.exact[own], want[own]) and np.array_equal(self.best[own], want[own])
        assert (self.exact[(kinds == 'half') | (kinds == 'empty')] == -1).all()
        assert (self.best[(kinds == 'half') | (kinds == 'empty')] == -1).all()
        assert np.array_equal(self.exact[kinds == 'cc'], want[kinds == 'cc'])
        assert (self.best[kinds == 'cc'] != want[kinds == 'cc']).all()
        self.tflags = np.zeros(T, np.uint8)
        self.tflags[g] = 1
        self.tflags[l] = 2
        self.tflags[few[1]] = 1      # a second GPL and a second LGPL, as gpl-2.0 / lgpl-2.1
        self.tflags[few[2]] = 2

    def close(self):
        self.b.close()
        self.sc.close()

    def expect(self, offsets, use_exact, k):
        """The oracle over the downloaded per-file results, project by project."""
        T = self.T
        gpl, lgpl = np.flatnonzero(self.tflags & 1).tolist(), np.flatnonzero(self.tflags & 2).tolist()
        lic = [PO.file_license(T, bool(self.copyright[i]), self.exact[i], self.best[i], use_exact) for i in range(self.n)]
        P = len(offsets) - 1
        o_lic, o_mf, o_nl = np.full(P, -1, np.int32), np.full(P, -1, np.int32), np.zeros(P, np.int32)
        o_list = np.full((P, k), -1, np.int32)
        for p in range(P):
            a, e = int(offsets[p]), int(offsets[p + 1])
            proj = PO.OracleProject([(self.names[i], lic[i], bool(self.copyright[i]), i) for i in range(a, e)], gpl, lgpl, T)
            x = proj.license()
            o_lic[p] = -1 if x is None else x
            f = proj.matched_file()
            o_mf[p] = -1 if f is None else f[3]
            ls = proj.licenses()
            o_nl[p] = len(ls)
            o_list[p, :min(k, len(ls))] = ls[:k]
        return o_lic, o_mf, o_nl, o_list

    def check(self, offsets, use_exact=True, k=4):
        self.b.projects(offsets, self.flags, self.tflags, use_exact=use_exact, k=k)
        got = self.b.download_projects()
        want = self.expect(offsets, use_exact, k)
        for name, g, w in zip(('license', 'matched_file', 'n_licenses', 'licenses'), got, want):
            assert g.shape == w.shape and g.dtype == w.dtype, name
            if w.size == 0:
                continue
            bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
            assert bad.size == 0, (name, bad[:8], g[bad[:8]], w[bad[:8]], [int(offsets[p + 1] - offsets[p]) for p in bad[:8]])
        return got

    def partition(self, P):
        """P projects over the same resident files: random cuts, about a third of them empty."""
        if P == 1:
            return np.array([0, self.n], np.int64)
        cuts = np.sort(self.rng.integers(0, self.n + 1, P - 1))
        cuts[self.rng.random(P - 1) < 0.3] = 0
        return np.concatenate([[0], np.sort(cuts), [self.n]]).astype(np.int64)


@pytest.fixture(scope='module')
def vendored():
    from licensee_amd.corpus import TemplateCorpus
    ctx = Ctx(TemplateCorpus(License.all(hidden=True, pseudo=False)), seed=7)
    assert ctx.T == 47 and ctx.sc.info()[2] == 1
    yield ctx
    ctx.close()


@pytest.fixture(scope='module')
def large():
    from licensee_amd.corpus import TemplateCorpus
    from licensee_amd.synth_templates import synthetic_templates
    ctx = Ctx(TemplateCorpus(synthetic_templates(License.all(hidden=True, pseudo=False), 600, seed=20250202)), seed=8)
    assert ctx.T == 600 and ctx.sc.info()[2] == 3 and min(ctx.glm) > 64
    yield ctx
    ctx.close()


def _rules(ctx):
    T = ctx.T
    g, l, m = ctx.glm
    lic, mf, nl, lst = ctx.check(ctx.offsets, True, 4)
    sizes = np.diff(ctx.offsets)
    assert set(SIZES) <= set(sizes.tolist()) and sizes[0] == 0 and sizes[-1] == 0 and sizes[-2] == 0
    assert ctx.offsets[-1] == ctx.n
    # the rules came out as project.rb states them (the oracle agreeing is checked above)
    pr = ctx.projects
    two = {(p[0][0], p[1][0], p[0][1][1], p[1][1][1]): i for i, p in enumerate(pr)
           if len(p) == 2 and p[0][1][0] == p[1][1][0] == 'self' and not p[0][2] and not p[1][2]}
    i = two[('LICENSE', 'COPYING.lesser', g, l)]
    assert lic[i] == l and mf[i] == ctx.offsets[i] + 1 and lst[i].tolist() == [l, g, -1, -1]
    i = two[('COPYING.lesser', 'LICENSE', l, g)]
    assert lic[i] == l and mf[i] == ctx.offsets[i] and lst[i].tolist() == [l, g, -1, -1]
    for key in (('LICENSE', 'COPYING', g, l), ('LICENSE', 'COPYING.lesser', m, l), ('COPYING.lesser', 'LICENSE', g, l),
                ('LICENSE', 'COPYING.lesser', g, m)):
        assert lic[two[key]] == T and mf[two[key]] == -1, key
    i = two[('LICENSE', 'COPYING.lesser', l, l)]
    assert lic[i] == l and mf[i] == -1 and nl[i] == 1
    first = next(i for i, p in enumerate(pr) if len(p) == 3)
    assert (lic[first:first + 6] == T).all() and (nl[first:first + 6] == 3).all()
    assert lst[first + 6].tolist() == [l, g, m, -1]                       # prioritize_lgpl, the lesser file third
    only = next(i for i, p in enumerate(pr) if len(p) == 1 and p[0][0] == 'COPYRIGHT' and p[0][2])
    assert lic[only] == -1 and nl[only] == 1 and mf[only] == ctx.offsets[only] and lst[only, 0] == T + 1
    assert lic[only + 1] == -1 and nl[only + 1] == 1 and mf[only + 1] == -1
    assert lic[only + 2] == m                                              # a COPYRIGHT name the matcher did not match
    assert lic[only + 3] == T and lic[only + 4] == m
    assert lic[only + 5] == T + 1 and lic[only + 6] == T and lic[only + 7] == T
    big = next(i for i, p in enumerate(pr) if len(p) == 1000)
    assert lst[big, 0] == l and lst[big, 1] == g and lic[big] == T
    assert lst[big + 1].tolist()[:2] == [l, g] and nl[big + 1] == 2
    assert nl.max() == 14
    return lic, mf, nl, lst


def test_rules_vendored(vendored):
    _rules(vendored)


def test_rules_large_corpus(large):
    _rules(large)


@pytest.mark.parametrize('k', [0, 1, 8])
def test_k_licenses(vendored, large, k):
    for ctx in (vendored, large):
        lic, mf, nl, lst = ctx.check(ctx.offsets, True, k)
        assert lst.shape == (len(ctx.offsets) - 1, k) and nl.max() == 14     # the count is exact, the list is cut
        if k == 8:
            assert (lst[np.argmax(nl)] >= 0).all()


@pytest.mark.parametrize('P', [1, 63, 64, 65, 4097])
def test_project_counts(vendored, large, P):
    for ctx in (vendored, large):
        off = ctx.partition(P)
        assert len(off) == P + 1 and off[-1] == ctx.n
        ctx.check(off, True, 4)


def test_use_exact_0_against_1(vendored, large):
    for ctx in (vendored, large):
        with_exact = ctx.check(ctx.offsets, True, 4)
        without = ctx.check(ctx.offsets, False, 4)
        assert (with_exact[0] != without[0]).any()     # the CC files: Exact finds them, Dice filters them


def test_state_and_argument_errors(vendored):
    from licensee_amd._native import DiceError, FileBatch
    c, sc = vendored.c, vendored.sc
    n = 5
    fb = FileBatch(c.lf_bits[:n], c.lf_size[:n], c.length[:n], np.zeros(n, np.uint8))
    off, fl, tf = np.array([0, 2, 2, 5], np.int64), np.zeros(n, np.uint8), vendored.tflags

    def code(fn, *a, **kw):
        with pytest.raises(DiceError) as e:
            fn(*a, **kw)
        return e.value.code
    b = sc.batch(8)
    try:
        b.upload(fb)
        assert code(b.projects, off, fl, tf, use_exact=False) == -4        # resolve before match
        b.match(98.0)
        assert code(b.projects, off, fl, tf, use_exact=True) == -4         # use_exact without Exact
        b.n_projects, b.k_licenses = 3, 4
        assert code(b.download_projects) == -4                             # download before resolve
        b.projects(off, fl, tf, use_exact=False, k=4)
        lic = b.download_projects()[0]
        assert lic.tolist() == [vendored.T, -1, vendored.T]
        assert code(b.download_project_match, digest=True) == -4           # no content hash on this batch
        b.exact(None)
        b.projects(off, fl, tf, use_exact=True, k=4)
        for bad in ([1, 2, 2, 5], [0, 3, 2, 5], [0, 2, 2, 4], [0, 2, 2, 6]):
            assert code(b.projects, np.array(bad, np.int64), fl, tf) == -1, bad
        assert code(b.projects, off, fl, tf, k=9) == -1
        b.projects(off, fl, tf, use_exact=True, k=2)
        assert b.download_projects()[3].tolist() == [[0, 1], [-1, -1], [2, 3]]
        b.upload(fb)                                                       # a new upload invalidates the resolve
        assert code(b.download_projects) == -4
        assert code(b.projects, off, fl, tf, use_exact=False) == -4
        # an empty batch: every project is empty
        b.upload(FileBatch(c.lf_bits[:0], c.lf_size[:0], c.length[:0], np.zeros(0, np.uint8)))
        b.exact(None)
        b.match(98.0)
        b.projects(np.zeros(4, np.int64), np.zeros(0, np.uint8), tf)
        lic, mf, nl, lst = b.download_projects()
        assert lic.tolist() == mf.tolist() == [-1] * 3 and nl.tolist() == [0] * 3 and (lst == -1).all()
    finally:
        b.close()


# ---- end to end: BatchDetector.detect_projects on the reference's fixtures ------------------------

@pytest.fixture(scope='module')
def fixture_projects(reference_root):
    with open(os.path.join(GOLDEN, 'fixture_files.json'), encoding='utf-8') as fh:
        recs = json.load(fh)
    groups = {}
    for r in recs:
        groups.setdefault(r['fixture'], []).append(r)
    out = []
    for name, rs in groups.items():
        if any('unsupported' in r for r in rs):
            continue
        files = [('README.md', b'MIT License')]
        for r in reversed(rs):      # (not in find_files order: the host stage sorts)
            with open(os.path.join(reference_root, 'spec', 'fixtures', name, r['file']), 'rb') as fh:
                files.append((r['file'], fh.read()))
        out.append((name, rs[0]['expected'], files))
    assert len(out) == 52
    return out


@pytest.fixture(scope='module')
def per_project(fixture_projects):
    """projects.Project per fixture project (the per-file matcher chain), computed once."""
    from licensee_amd.projects import Project
    out = []
    for name, exp, files in fixture_projects:
        p = Project(files)
        lic, mf = p.license(), p.matched_file()
        m = mf.matcher() if mf is not None else None
        out.append((lic.key if lic is not None else None, mf.filename if mf is not None else None,
                    [l.key for l in p.licenses()], m.name if m is not None else None,
                    m.confidence() if m is not None else None, len(p.license_files())))
        assert out[-1][0] == exp['key'], name
    return out


def _same(det, want, name):
    assert (det.license.key if det.license is not None else None) == want[0], name
    assert det.matched_file == want[1], name
    assert [l.key for l in det.licenses] == want[2] and det.n_licenses == len(want[2]), name
    assert (det.matcher, det.confidence) == (want[3], want[4]), name
    assert det.n_files == want[5], name


@pytest.mark.parametrize('wordset_on', ['device', 'host'])
def test_detect_projects_equals_project(fixture_projects, per_project, wordset_on):
    from licensee_amd.batch import BatchDetector
    det = BatchDetector(nthreads=4, wordset_on=wordset_on)
    try:
        assert det.wordset_on == wordset_on
        got = det.detect_projects([files for _, _, files in fixture_projects])
        assert len(got) == 52
        for d, want, (name, _, _) in zip(got, per_project, fixture_projects):
            _same(d, want, name)
            assert d.content_hash is None
        # three batches through the pipeline, one of them without projects
        batches = [[f for _, _, f in fixture_projects[:20]], [], [f for _, _, f in fixture_projects[20:]]]
        streamed = list(det.detect_projects_stream(batches))
        assert [len(s) for s in streamed] == [20, 0, 32]
        assert streamed[0] + streamed[2] == got
        assert [det.detect_projects(bt) for bt in batches] == streamed
    finally:
        det.close()


def test_detect_projects_content_hash(fixture_projects, per_project):
    from licensee_amd.batch import BatchDetector
    det = BatchDetector(nthreads=4, content_hash=True)
    try:
        got = det.detect_projects([files for _, _, files in fixture_projects])
        hashed = 0
        for d, want, (name, exp, _) in zip(got, per_project, fixture_projects):
            _same(d, want, name)
            assert (d.content_hash is not None) == (d.matched_file is not None), name
            if exp.get('hash') and d.matched_file is not None:
                assert d.content_hash == exp['hash'], name
                hashed += 1
        assert hashed >= 30
    finally:
        det.close()
