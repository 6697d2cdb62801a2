"""Candidate files: restates ``Licensee::ProjectFiles::ProjectFile`` / ``LicenseFile``.

    ProjectFile#initialize (decode)     lib/licensee/project_files/project_file.rb:37-45
    ProjectFile#matcher/confidence      project_file.rb:69-80
    LicenseFile::CC_FALSE_POSITIVE_REGEX license_file.rb:63-65 (here 173-175 of the concatenated view)
    LicenseFile#possible_matchers       license_file.rb:67-69
    LicenseFile#potential_false_positive? license_file.rb:80-82
    LicenseFile#license                 license_file.rb:92-98 (falls back to License 'other')
    LicenseFile::FILENAME_REGEXES / .name_score   license_file.rb:8-59,100-102
    LicenseFile.lesser_gpl_score        license_file.rb:105-107
    LicenseFile#lgpl? / #gpl?           license_file.rb:84-90
    ProjectFile#copyright?              project_file.rb:90-95
"""
from __future__ import annotations

import re
from typing import Optional, Union

from .content_helper import ContentHelper, ruby_strip
from .license import License

CC_FALSE_POSITIVE_REGEX = re.compile(r'^(creative commons )?Attribution-(NonCommercial|NoDerivatives)',
                                     re.I | re.M)


# license_file.rb:8-35. A Regexp interpolated into another keeps its own flags (Ruby writes it as
# (?i-mx:...)), so only the interpolated pieces that carry /i ignore case: PREFERRED_EXT_REGEX does
# not, and 'LICENSE.MD' scores 0.80 (LICENSE_EXT_REGEX), not 0.95. Ruby's \w and \d are ASCII.
_PREFERRED_EXT = r'(?:\.(?:md|markdown|txt|html)\Z)'
_LICENSE_EXT = r'(?i:\.(?!spdx|header)([^./]|\.[0-9])+\Z)'
_OTHER_EXT = r'(?i:\.(?!xml|go|gemspec)([^./]|\.[0-9])+\Z)'
_ANY_EXT = r'(?i:\.([^./]|\.[0-9])+\Z)'
_LICENSE = r'(?i:(un)?licen[sc]e)'
_COPYING = r'(?i:copying)'
_COPYRIGHT = r'(?i:copyright)'
_OFL = r'(?i:ofl)'
_PATENTS = r'(?i:patents)'
_W = r'[a-zA-Z0-9_]'

# license_file.rb:38-59, in the reference's order; the first that matches gives the score
FILENAME_REGEXES = tuple((re.compile(rx), score) for rx, score in (
    (rf'\A{_LICENSE}\Z', 1.00),                                     # LICENSE
    (rf'\A{_LICENSE}{_PREFERRED_EXT}\Z', 0.95),                      # LICENSE.md
    (rf'\A{_COPYING}\Z', 0.90),                                     # COPYING
    (rf'\A{_COPYING}{_PREFERRED_EXT}\Z', 0.85),                      # COPYING.md
    (rf'\A{_LICENSE}{_LICENSE_EXT}\Z', 0.80),                        # LICENSE.textile
    (rf'\A{_COPYING}{_ANY_EXT}\Z', 0.75),                            # COPYING.textile
    (rf'\A{_LICENSE}[-_][^.]*{_OTHER_EXT}?\Z', 0.70),                # LICENSE-MIT
    (rf'\A{_COPYING}[-_][^.]*{_OTHER_EXT}?\Z', 0.65),                # COPYING-MIT
    (rf'\A{_W}+[-_]{_LICENSE}[^.]*{_OTHER_EXT}?\Z', 0.60),           # MIT-LICENSE-MIT
    (rf'\A{_W}+[-_]{_COPYING}[^.]*{_OTHER_EXT}?\Z', 0.55),           # MIT-COPYING
    (rf'\A{_OFL}{_PREFERRED_EXT}', 0.50),                            # OFL.md
    (rf'\A{_OFL}{_OTHER_EXT}', 0.45),                                # OFL.textile
    (rf'\A{_OFL}\Z', 0.40),                                         # OFL
    (rf'\A{_COPYRIGHT}\Z', 0.35),                                   # COPYRIGHT
    (rf'\A{_COPYRIGHT}{_PREFERRED_EXT}\Z', 0.30),                    # COPYRIGHT.txt
    (rf'\A{_COPYRIGHT}{_OTHER_EXT}\Z', 0.25),                        # COPYRIGHT.textile
    (rf'\A{_COPYRIGHT}[-_][^.]*{_OTHER_EXT}?\Z', 0.20),              # COPYRIGHT-MIT
    (rf'\A{_PATENTS}\Z', 0.15),                                     # PATENTS
    (rf'\A{_PATENTS}{_OTHER_EXT}\Z', 0.10),                          # PATENTS.txt
    (r'', 0.00),                                                     # catch all
))

# project_file.rb:94 (/io: the whole expression ignores case)
COPYRIGHT_NAME_REGEX = re.compile(r'\Acopyright(?:\.(?!xml|go|gemspec)([^./]|\.[0-9])+\Z)?\Z', re.I)


def is_copyright_file(filename: Optional[str]) -> bool:
    """The name half of ProjectFile#copyright? (project_file.rb:94)."""
    return filename is not None and COPYRIGHT_NAME_REGEX.search(filename) is not None


def decode_content(content: Union[str, bytes]) -> str:
    """project_file.rb:38-41: force UTF-8, drop invalid bytes, universal newline."""
    if isinstance(content, bytes):
        text = content.decode('utf-8', errors='ignore')
    else:
        text = content
    return text.replace('\r\n', '\n').replace('\r', '\n')


class ProjectFile:
    def __init__(self, content: Union[str, bytes], metadata=None):
        self.content = decode_content(content)
        if isinstance(metadata, str):
            metadata = {'name': metadata}
        self._data = metadata or {}

    @property
    def filename(self) -> Optional[str]:
        return self._data.get('name')

    path = filename

    def possible_matchers(self):
        raise NotImplementedError

    def matcher(self):
        if not hasattr(self, '_matcher'):
            self._matcher = None
            for cls in self.possible_matchers():
                m = cls(self)
                if m.match():
                    self._matcher = m
                    break
        return self._matcher

    def confidence(self):
        m = self.matcher()
        return None if m is None else m.confidence()

    def matched_license(self):
        lic = self.license()
        return None if lic is None else lic.spdx_id

    def copyright_p(self) -> bool:
        """project_file.rb:90-95: a COPYRIGHT file that holds only a copyright statement."""
        from .matchers import Copyright
        if not isinstance(self, LicenseFile):
            return False
        if not isinstance(self.matcher(), Copyright):
            return False
        return is_copyright_file(self.filename)


class LicenseFile(ContentHelper, ProjectFile):
    def __init__(self, content: Union[str, bytes], metadata=None):
        ProjectFile.__init__(self, content, metadata)

    @staticmethod
    def title_regex_provider():
        return License.title_regex()

    def possible_matchers(self):
        from .matchers import Copyright, Dice, Exact
        return [Copyright, Exact, Dice]

    def potential_false_positive(self) -> bool:
        return CC_FALSE_POSITIVE_REGEX.search(ruby_strip(self.content)) is not None

    def license(self) -> License:
        m = self.matcher()
        if m is not None and m.match():
            return m.match()
        return License.find('other')

    match = license

    def lgpl(self) -> bool:
        """license_file.rb:84-86"""
        return LicenseFile.lesser_gpl_score(self.filename) == 1 and self.license().lgpl()

    def gpl(self) -> bool:
        """license_file.rb:88-90"""
        return self.license().gpl()

    @staticmethod
    def name_score(filename: str) -> float:
        """license_file.rb:100-102"""
        return next(score for rx, score in FILENAME_REGEXES if rx.search(filename))

    @staticmethod
    def lesser_gpl_score(filename: Optional[str]) -> int:
        """license_file.rb:105-107 (casecmp folds ASCII letters only)"""
        if filename is None:
            return 0
        fold = str.maketrans('ABCDEFGHIJKLMNOPQRSTUVWXYZ', 'abcdefghijklmnopqrstuvwxyz')
        return 1 if filename.translate(fold) == 'copying.lesser' else 0

    def similarity(self, other) -> float:
        from .dice import pair_similarity
        return pair_similarity(self, other)
