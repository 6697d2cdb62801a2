"""Generate the committed golden vectors under tests/golden/ from the reference checkout.

Run in the build container (needs /root/reference; the GPU box never reads it):

    python tests/golden/make_golden.py [/root/reference]

Every vector is *data*: inputs in normalized space (derived with licensee_amd's normalizer,
which these same files pin against the reference's SHA1s) plus the expectations the
reference's own tests state. Outputs:

  reference_expectations.json  -- reference-stated expectations only: template SHA1s
                                  (spec/fixtures/license-hashes.json) and per-fixture
                                  key / matcher / SHA1 (spec/fixtures/fixtures.yml).
  fixture_files.json           -- for each fixture license file: normalized text, CC flag,
                                  our SHA1, and the expectations above.
  reference.tar.xz             -- the raw files behind them that tests normalize again (fixture
                                  license files, templates, SPDX XMLs, detect.json, license-hashes.json).
  dice_spec.json               -- spec/licensee/matchers/dice_matcher_spec.rb cases.
  vendored.json                -- spec/vendored_license_spec.rb property cases for all 47
                                  templates (rendered / rewrapped / title variants /
                                  75 random words), seeded.
"""
from __future__ import annotations

import json
import os
import random
import re
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from licensee_amd.content_helper import FIELD_REGEX, wrap_text  # noqa: E402
from licensee_amd.license import License, load_raw_corpus  # noqa: E402
from licensee_amd.project_files import LicenseFile  # noqa: E402

# spec/spec_helper.rb:65-79 field_values
FIELD_VALUES = {'fullname': 'Ben Balter', 'year': '2018', 'email': 'ben@github.invalid',
                'projecturl': 'http://github.invalid/benbalter/licensee', 'login': 'benbalter',
                'project': 'Licensee', 'description': 'Detects licenses'}

# lib/licensee/project_files/license_file.rb:17-57 (filename scores; discovery only)
_LIC = r'(un)?licen[sc]e'
_PREF = r'\.(?:md|markdown|txt|html)\Z'
_LEXT = r'\.(?!spdx|header)([^./]|\.\d)+\Z'
_OEXT = r'\.(?!xml|go|gemspec)([^./]|\.\d)+\Z'
_AEXT = r'\.([^./]|\.\d)+\Z'
NAME_SCORES = [
    (rf'\A{_LIC}\Z', 1.00), (rf'\A{_LIC}{_PREF}', 0.95), (r'\Acopying\Z', 0.90),
    (rf'\Acopying{_PREF}', 0.85), (rf'\A{_LIC}{_LEXT}', 0.80), (rf'\Acopying{_AEXT}', 0.75),
    (rf'\A{_LIC}[-_][^.]*({_OEXT})?\Z', 0.70), (rf'\Acopying[-_][^.]*({_OEXT})?\Z', 0.65),
    (rf'\A\w+[-_]{_LIC}[^.]*({_OEXT})?\Z', 0.60), (rf'\A\w+[-_]copying[^.]*({_OEXT})?\Z', 0.55),
    (rf'\Aofl{_PREF}', 0.50), (rf'\Aofl{_OEXT}', 0.45), (r'\Aofl\Z', 0.40), (r'\Acopyright\Z', 0.35),
    (rf'\Acopyright{_PREF}', 0.30), (rf'\Acopyright{_OEXT}', 0.25),
    (rf'\Acopyright[-_][^.]*({_OEXT})?\Z', 0.20), (r'\Apatents\Z', 0.15), (rf'\Apatents{_OEXT}', 0.10),
]


def name_score(name: str) -> float:
    for rx, score in NAME_SCORES:
        if re.search(rx, name, re.I):
            return score
    return 0.0


def render(license) -> str:
    """sub_copyright_info: Mustache render of content_for_mustache (spec_helper.rb:81-83)."""
    return FIELD_REGEX.sub(lambda m: FIELD_VALUES[m.group(1)], license.content)


def add_random_words(text: str, count: int, rng: random.Random, ipsum) -> str:
    """spec_helper.rb:86-95 (seeded Python RNG instead of Ruby's Kernel.srand)."""
    words = text.split()
    for _ in range(count):
        w = ipsum[rng.randrange(len(ipsum))]
        words.insert(rng.randrange(len(words)), w)
    return ' '.join(words)


def file_record(text, filename='LICENSE'):
    lf = LicenseFile(text, filename)
    n = lf.content_normalized()
    return {'normalized': n, 'cc_false_positive': bool(lf.potential_false_positive()),
            'sha1': lf.content_hash(), 'wordset_size': len(lf.wordset()), 'length': lf.length()}


def write_reference_archive(ref, records):
    """reference.tar.xz: the raw data files of the checkout that CPU tests read (conftest.py's
    reference_root unpacks it), at their paths in the checkout -- every supported fixture license
    file, detect.json, license-hashes.json, the 47 choosealicense.com templates and SPDX XMLs.
    Sorted members without times or owners: the same bytes from the same checkout."""
    import tarfile
    rel = [os.path.join('spec', 'fixtures', r['fixture'], r['file']) for r in records if 'unsupported' not in r]
    rel += [os.path.join('spec', 'fixtures', f) for f in ('detect.json', 'license-hashes.json')]
    for sub in (os.path.join('vendor', 'choosealicense.com', '_licenses'),
                os.path.join('vendor', 'license-list-XML', 'src')):
        rel += [os.path.join(sub, f) for f in os.listdir(os.path.join(ref, sub))]

    def plain(ti):
        ti.mtime, ti.uid, ti.gid, ti.uname, ti.gname, ti.mode = 0, 0, 0, '', '', 0o644
        return ti
    with tarfile.open(os.path.join(HERE, 'reference.tar.xz'), 'w:xz') as tar:
        for p in sorted(set(rel)):
            tar.add(os.path.join(ref, p), arcname=p, filter=plain)


def main(ref):
    corpus = load_raw_corpus(ref)
    License.set_corpus(corpus)
    fx = os.path.join(ref, 'spec', 'fixtures')
    with open(os.path.join(fx, 'license-hashes.json')) as fh:
        hashes = json.load(fh)
    with open(os.path.join(fx, 'fixtures.yml')) as fh:
        expectations = yaml.safe_load(fh)
    with open(os.path.join(HERE, 'reference_expectations.json'), 'w') as fh:
        json.dump({'source': 'spec/fixtures/license-hashes.json + spec/fixtures/fixtures.yml',
                   'template_sha1': hashes, 'fixtures': expectations}, fh, indent=1, sort_keys=True)

    # ---- fixture license files --------------------------------------------------------
    records = []
    for name in sorted(os.listdir(fx)):
        d = os.path.join(fx, name)
        if not os.path.isdir(d):
            continue
        exp = expectations.get(name) or {}
        cands = sorted((f for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)) and name_score(f) > 0),
                       key=lambda f: -name_score(f))
        for fn in cands:
            with open(os.path.join(d, fn), 'rb') as fh:
                raw = fh.read()
            rec = {'fixture': name, 'file': fn, 'expected': exp}
            try:
                rec.update(file_record(raw, fn))
            except NotImplementedError as e:
                rec['unsupported'] = str(e)
            lf = LicenseFile(raw, fn)
            from licensee_amd.matchers import Copyright, Exact
            if 'unsupported' not in rec:
                rec['copyright'] = Copyright(lf).match() is not None
                ex = Exact(lf).match()
                rec['exact'] = ex.key if ex else None
            records.append(rec)
    with open(os.path.join(HERE, 'fixture_files.json'), 'w') as fh:
        json.dump(records, fh, indent=1, sort_keys=True, ensure_ascii=False)
    write_reference_archive(ref, records)

    # ---- dice_matcher_spec.rb ----------------------------------------------------------
    gpl, mit, cc_by = License.find('gpl-3.0'), License.find('mit'), License.find('cc-by-4.0')
    with open(os.path.join(fx, 'cc-by-nd', 'LICENSE'), 'rb') as fh:
        cc_nd = fh.read().decode('utf-8')
    spec = {
        'gpl': {'file': file_record(render(gpl), 'LICENSE.txt'), 'match': 'gpl-3.0', 'confidence': 100.0,
                'by_similarity': [['gpl-3.0', 100.0], ['agpl-3.0', 94.56967213114754],
                                  ['lgpl-2.1', 26.821370750134918]]},
        'not_a_license': {'file': file_record('Not really a license', 'LICENSE.txt'), 'match': None, 'confidence': 0},
        'stacked': {'file': file_record(render(mit) + '\n\n' + render(gpl), 'LICENSE.txt'), 'match': None,
                    'confidence': 0},
        'cc_by': {'file': file_record(cc_by.content, 'LICENSE'), 'match': 'cc-by-4.0'},
        'cc_nd': {'file': file_record(cc_nd, 'LICENSE.txt'), 'match': None, 'confidence': 0},
    }
    with open(os.path.join(HERE, 'dice_spec.json'), 'w') as fh:
        json.dump({'source': 'spec/licensee/matchers/dice_matcher_spec.rb:23-78', 'cases': spec}, fh, indent=1,
                  sort_keys=True, ensure_ascii=False)

    # ---- vendored_license_spec.rb -------------------------------------------------------
    with open(os.path.join(fx, 'ipsum.txt')) as fh:
        ipsum = fh.read().split()
    rng = random.Random(20250202)
    vend = []
    for lic in License.all(hidden=True, pseudo=False):
        content = render(lic)
        title_stripped = LicenseFile(content, 'LICENSE.txt')
        title_stripped._strip_title()
        with_words = add_random_words(content, 75, rng, ipsum)
        cases = {
            'rendered': content,
            'without_title': title_stripped._cur(),
            'double_title': lic.name.replace('*', 'u', 1) + '\n\n' + content,
            'rewrapped': wrap_text(content, 60),
            'random_words': with_words,
            'rewrapped_random_words': wrap_text(with_words, 60),
        }
        expect = {'rendered': True, 'without_title': True, 'double_title': True, 'rewrapped': True,
                  'random_words': False, 'rewrapped_random_words': False}
        vend.append({'key': lic.key, 'cases': {k: dict(file_record(v, 'LICENSE.txt'), detected=expect[k])
                                               for k, v in cases.items()}})
    with open(os.path.join(HERE, 'vendored.json'), 'w') as fh:
        json.dump({'source': 'spec/vendored_license_spec.rb:9-94 (random words: seeded Python RNG)',
                   'templates': vend}, fh, ensure_ascii=False, sort_keys=True)
    print('golden vectors written to', HERE)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
