"""Host normalization (licensee_amd.content_helper) pinned by the reference's own goldens.

  spec/fixtures/license-hashes.json      (47 template SHA1s; vendored_license_spec.rb:31-37)
  spec/fixtures/fixtures.yml             (fixture SHA1s; fixture_spec.rb:25-43)
  spec/fixtures/detect.json              (normalized MIT text)
  spec/licensee/content_helper_spec.rb   (strip / normalize / title-regex cases)
  spec/licensee/project_files/license_file_spec.rb:49-57 (93 words, first 'permission')
Tests reading raw reference files read the copies in tests/golden/reference.tar.xz.
"""
import hashlib
import json
import os
import re

import pytest

from licensee_amd.content_helper import ContentHelper, wrap_text
from licensee_amd.license import License
from licensee_amd.project_files import LicenseFile

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def golden(name):
    with open(os.path.join(GOLDEN, name), encoding='utf-8') as fh:
        return json.load(fh)


class Helper(ContentHelper):
    """spec/licensee/content_helper_spec.rb:3-19 (ContentHelperTestHelper)."""

    def __init__(self, content, filename=None):
        self.content = content
        self.filename = filename

    @staticmethod
    def title_regex_provider():
        return License.title_regex()


def norm(content, filename='license.md'):
    return Helper(content, filename).content_normalized()


# ---- templates --------------------------------------------------------------------------
def test_template_table_sha1s_match_reference():
    exp = golden('reference_expectations.json')['template_sha1']
    lics = License.all(hidden=True, pseudo=False)
    assert len(lics) == 47
    for l in lics:
        assert hashlib.sha1(l.content_normalized().encode()).hexdigest() == exp[l.key], l.key


def test_template_table_regenerates_from_reference(reference_root):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), '..', 'tools'))
    from vendor_templates import build_table
    fresh = build_table(reference_root)
    with open(os.path.join(os.path.dirname(__file__), '..', 'licensee_amd', 'data', 'templates.json')) as fh:
        committed = json.load(fh)
    assert fresh['licenses'] == committed['licenses']
    License._corpus = None  # reload the committed corpus for later tests
    License._title_regex = None


def test_license_counts():
    # license_spec.rb:4-7 -- 47 vendored + 2 pseudo
    assert len(License.all(hidden=True)) == 49
    assert len(License.all(hidden=True, pseudo=False)) == 47
    assert License.find('MIT').key == 'mit'
    assert License.find('other').pseudo_license()
    assert License.find('mit').spdx_id == 'MIT' and License.find('other').spdx_id == 'NOASSERTION'


# ---- fixtures ------------------------------------------------------------------------------
def test_fixture_hashes_match_reference():
    recs = golden('fixture_files.json')
    checked = 0
    for r in recs:
        exp = r['expected'].get('hash')
        if exp and 'unsupported' not in r and sum(x['fixture'] == r['fixture'] for x in recs) == 1:
            assert r['sha1'] == exp, r['fixture']
            assert hashlib.sha1(r['normalized'].encode()).hexdigest() == exp
            checked += 1
    assert checked >= 40


def test_fixture_files_renormalize(reference_root):
    fx = os.path.join(reference_root, 'spec', 'fixtures')
    for r in golden('fixture_files.json'):
        if 'unsupported' in r:
            continue
        with open(os.path.join(fx, r['fixture'], r['file']), 'rb') as fh:
            lf = LicenseFile(fh.read(), r['file'])
        assert lf.content_normalized() == r['normalized'], r['fixture']


def test_detect_json_normalized_mit(reference_root):
    with open(os.path.join(reference_root, 'spec', 'fixtures', 'detect.json')) as fh:
        d = json.load(fh)['matched_files'][0]
    lf = LicenseFile(d['content'], d['filename'])
    assert lf.content_normalized() == d['content_normalized']
    assert lf.content_hash() == d['content_hash']


# ---- content_helper_spec.rb ------------------------------------------------------------------
SPEC_CONTENT = re.sub(r'(?m)^\s*', '', '''  # The MIT License
	=================

	Copyright 2016 Ben Balter
	*************************

  All rights reserved.

  The made
  * * * *
  up  license.

  This license provided 'as is'. Please respect the contributors' wishes when
  implementing the license's "software".
  -----------
''')


def test_spec_integration_fixture():
    h = Helper(SPEC_CONTENT, 'license.md')
    assert h.wordset() == {'the', 'made', 'up', 'license', 'this', 'provided', 'as', "is'", 'please',
                           'respect', "contributors'", 'wishes', 'when', 'implementing', "license's",
                           'software'}
    assert h.length() == 135
    assert h.length_delta(License.find('mit')) == 885
    assert h.content_hash() == '9b4bed43726cf39e17b11c2942f37be232f5709a'
    assert h.content_normalized() == ("the made up license. this license provided 'as is'. please respect the "
                                      "contributors' wishes when implementing the license's 'software'.")


@pytest.mark.parametrize('field,fixture', list({
    'version': "The MIT License\nVersion 1.0\nfoo",
    'hrs': "The MIT License\n=====\n-----\n*******\nfoo",
    'markdown_headings': "# The MIT License\n\nfoo",
    'whitespace': "The MIT License\n\n   foo  ",
    'all_rights_reserved': "Copyright 2016 Ben Balter\n\nfoo",
    'urls': "https://example.com\nfoo",
    'developed_by': "Developed By: Ben Balter\n\nFoo",
    'borders': '*   Foo    *',
    'title': "The MIT License\nfoo",
    'copyright': "The MIT License\nCopyright 2018 Ben Balter\nFoo",
    'copyright_bullet': "The MIT License\n* Copyright 2018 Ben Balter\nFoo",
    'copyright_italic': "The MIT License\n_Copyright 2018 Ben Balter_\nFoo",
    'end_of_terms': "Foo\nend of terms and conditions\nbar",
    'end_of_terms_hashes': "Foo\n# end of terms and conditions ####\nbar",
    'block_markup': '> Foo',
    'link_markup': '[Foo](http://exmaple.com)',
    'comment_markup': "/*\n* The MIT License\n* Foo\n*/",
    'copyright_title': "Copyright 2019 Ben Balter\nMIT License\nFoo",
    'title_in_parens': "(The MIT License)\n\nfoo",
    'multiple_copyrights': "Copyright 2016 Ben Balter\nCopyright 2017 Bob\nFoo",
}.items()))
def test_spec_strip(field, fixture):
    assert norm(fixture) == 'foo'


@pytest.mark.parametrize('content,expected', [
    ('_foo_ *foo* **foo** ~foo~', 'foo foo foo foo'),
    ('http://example.com', 'https://example.com'),
    ('Foo & Bar', 'foo and bar'),
    ("1. Foo\n * Bar", '- foo - bar'),
    ("- **(a)** Foo\n * b) Bar", '- foo - bar'),
    ('Foo-Bar—–baz-buzz', 'foo-bar-baz-buzz'),
    ("cc-\nlicensed", 'cc-licensed'),
    ("`a` 'b' \"c\" ‘d’ “e”", "'a' 'b' 'c' 'd' 'e'"),
    ('licence', 'license'),
])
def test_spec_normalizations(content, expected):
    assert norm(content) == expected


def test_spec_mit_similarity_and_wrap():
    mit = License.find('mit')
    assert mit.content_normalized(wrap=40).split('\n')[0].__len__() <= 40
    assert 'http:' not in License.find('ofl-1.1').content_normalized()
    assert '* *' not in License.find('mpl-2.0').content_normalized()


def test_spec_per_license_strips():
    # content_helper_spec.rb:282-311 over every license
    for l in License.all(hidden=True, pseudo=False):
        cn = l.content_normalized()
        assert not re.match(r'\A' + re.escape(l.name_without_version()), cn, re.I), l.key
        assert not re.match(r'\Aversion', cn, re.I)
        assert not re.search(r'all rights reserved', cn, re.I)
        assert not re.match(r'\Acopyright', cn, re.I)
        assert not re.search(r'END OF TERMS AND CONDITIONS', cn, re.I)
        assert not re.search(r'How to apply', cn, re.I)


@pytest.mark.parametrize('variation', ['key', 'title', 'nickname', 'name_without_version'])
def test_spec_title_regex(variation):
    # content_helper_spec.rb:333-396 with gpl-3.0
    gpl = License.find('gpl-3.0')
    v = {'key': gpl.key, 'title': gpl.title, 'nickname': gpl.nickname,
         'name_without_version': gpl.name_without_version()}[variation]
    tr = License.title_regex()
    for text in (v, f'The {v} license', f'({v})', f'(the {v} license)', f'     the {v} license'):
        assert tr.search(text), text
    assert not tr.search('gpl-3 0')
    assert not tr.search(f'The project is not licensed under the {v} license')


def test_wrap_and_percent():
    from licensee_amd.content_helper import format_percent
    assert format_percent(12.3456789) == '12.35%'
    w = wrap_text(License.find('mit').content_normalized(), 40)
    assert all(len(line) <= 40 for line in w.split('\n'))


def test_license_file_mit_wordset():
    # license_file_spec.rb:49-57 with sub_copyright_info(mit)
    vend = {t['key']: t for t in golden('vendored.json')['templates']}
    rec = vend['mit']['cases']['rendered']
    lf = LicenseFile(rec['normalized'], 'LICENSE.txt')
    words = lf.wordset_list()
    assert rec['wordset_size'] == 93 and words[0] == 'permission'


def test_decode_and_false_positive():
    lf = LicenseFile(b'Copyright \xff\xfe2016\r\nFoo\rBar', 'LICENSE')
    assert '\r' not in lf.content and '\xff' not in lf.content
    assert LicenseFile('Attribution-NonCommercial 4.0\nfoo').potential_false_positive()
    assert LicenseFile('Creative Commons Attribution-NoDerivatives').potential_false_positive()
    assert not LicenseFile('Attribution 4.0 International').potential_false_positive()


def test_html_is_unsupported():
    with pytest.raises(NotImplementedError):
        Helper('<ul><li>foo</li></ul>', 'license.html').content_normalized()
