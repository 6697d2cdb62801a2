"""Projects: restates ``Licensee::Projects::Project`` and the root-only part of ``FSProject``.

    Project#license                     lib/licensee/projects/project.rb:24-32
    Project#licenses                    project.rb:35-37
    Project#matched_file(s)             project.rb:40-47
    Project#license_file(s)             project.rb:50-66
    Project#lgpl?                       project.rb:102-106
    Project#find_files                  project.rb:111-117
    Project#prioritize_lgpl             project.rb:137-145
    Project#licenses_without_copyright  project.rb:153-155
    FSProject#files / #load_file        lib/licensee/projects/fs_project.rb:34-57 (the project's own
                                        directory only: no search_root walk)

``detect_readme`` and ``detect_packages`` are the reference's default, false: a project's files are its
license files. This is the per-project path over the per-file matcher chain (LicenseFile);
``BatchDetector.detect_projects`` resolves many projects at once on the device.

Order (parity-unpinned): ``find_files`` sorts with Ruby's ``sort``, which is not stable, so the
reference leaves the order of files of equal name score open. Here they keep the caller's order
(stable sort, score descending). ``license`` does not depend on that order; ``licenses``,
``matched_files`` and ``license_files`` do.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple, Union

from .license import License
from .project_files import LicenseFile


class Project:
    """A project over an in-memory list of ``(filename, content)``. ``file_class`` builds the
    license files (``file_class(content, filename)``): LicenseFile, or a subclass with another
    matcher chain."""

    def __init__(self, files: Sequence[Tuple[str, Union[str, bytes]]], file_class=LicenseFile):
        self._files = [{'name': name, 'content': content} for name, content in files]
        self._file_class = file_class

    # -- project.rb:24-32 ---------------------------------------------------------------
    def license(self) -> Optional[License]:
        if not hasattr(self, '_license'):
            without = self.licenses_without_copyright()
            if len(without) == 1 or self._lgpl():
                self._license = without[0] if without else None
            elif len(without) > 1:
                self._license = License.find('other')
            else:
                self._license = None
        return self._license

    # -- project.rb:35-37 ---------------------------------------------------------------
    def licenses(self) -> List[License]:
        if not hasattr(self, '_licenses'):
            self._licenses = _uniq(f.license() for f in self.matched_files())
        return self._licenses

    # -- project.rb:40-42 ---------------------------------------------------------------
    def matched_file(self) -> Optional[LicenseFile]:
        mf = self.matched_files()
        if len(mf) == 1 or self._lgpl():
            return mf[0] if mf else None
        return None

    # -- project.rb:45-47 ---------------------------------------------------------------
    def matched_files(self) -> List[LicenseFile]:
        if not hasattr(self, '_matched_files'):
            self._matched_files = [f for f in self._project_files() if f.license() is not None]
        return self._matched_files

    # -- project.rb:50-52 ---------------------------------------------------------------
    def license_file(self) -> Optional[LicenseFile]:
        lf = self.license_files()
        if len(lf) == 1 or self._lgpl():
            return lf[0] if lf else None
        return None

    # -- project.rb:54-66 ---------------------------------------------------------------
    def license_files(self) -> List[LicenseFile]:
        if not hasattr(self, '_license_files'):
            if not self.files():
                self._license_files = []
            else:
                found = self._find_files(LicenseFile.name_score)
                files = [self._file_class(self.load_file(f), f['name']) for f in found]
                self._license_files = self._prioritize_lgpl(files)
        return self._license_files

    # -- project.rb:102-106 -------------------------------------------------------------
    def _lgpl(self) -> bool:
        if not (len(self.licenses()) == 2 and len(self.license_files()) == 2):
            return False
        lf = self.license_files()
        return lf[0].lgpl() and lf[1].gpl()

    # -- project.rb:111-117 -------------------------------------------------------------
    def _find_files(self, score):
        if not self.files():
            return []
        found = [dict(f, score=score(f['name'])) for f in self.files()]
        found = [f for f in found if f['score'] > 0]
        return sorted(found, key=lambda f: -f['score'])     # stable: the caller's order within a score

    # -- project.rb:137-145 -------------------------------------------------------------
    @staticmethod
    def _prioritize_lgpl(files: List[LicenseFile]) -> List[LicenseFile]:
        if not files:
            return files
        first = files[0].license()
        if not (first is not None and first.gpl()):
            return files
        lesser = next((i for i, f in enumerate(files) if f.lgpl()), None)
        if lesser is not None:
            files.insert(0, files.pop(lesser))
        return files

    # -- project.rb:147-149 (no readme, no package file) ----------------------------------
    def _project_files(self) -> List[LicenseFile]:
        return list(self.license_files())

    # -- project.rb:153-155 -------------------------------------------------------------
    def licenses_without_copyright(self) -> List[License]:
        if not hasattr(self, '_without_copyright'):
            self._without_copyright = _uniq(f.license() for f in self.matched_files() if not f.copyright_p())
        return self._without_copyright

    # -- project.rb:157-163: the subclass hooks -------------------------------------------
    def files(self):
        return self._files

    def load_file(self, file):
        return file['content']


class FSProject(Project):
    """The files of one directory (fs_project.rb:34-57 with ``search_root`` equal to the directory;
    a path to a file gives the project of that one file)."""

    def __init__(self, path: str, file_class=LicenseFile):
        self._file_class = file_class
        if os.path.isfile(path):
            self._pattern = os.path.basename(path)
            self._dir = os.path.abspath(os.path.dirname(path))
        else:
            self._pattern = None
            self._dir = os.path.abspath(path)
        self._fs_files = None

    def files(self):
        if self._fs_files is None:
            # Dir.glob('*'): sorted, no dot files; regular files only
            names = [self._pattern] if self._pattern is not None else \
                sorted(n for n in os.listdir(self._dir) if not n.startswith('.'))
            self._fs_files = [{'name': n, 'dir': '.'} for n in names if os.path.isfile(os.path.join(self._dir, n))]
        return self._fs_files

    def load_file(self, file):
        with open(os.path.join(self._dir, file['name']), 'rb') as fh:
            return fh.read()     # (ProjectFile decodes: UTF-8, invalid bytes dropped)


def _uniq(items) -> list:
    """Array#uniq: first occurrences, in order (License equality is by key)."""
    out, seen = [], set()
    for x in items:
        k = x.key
        if k not in seen:
            seen.add(k)
            out.append(x)
    return out
