"""Independent checker for project resolution: lib/licensee/projects/project.rb restated literally
over lists of ``(filename, license_id, copyright_matched)`` tuples, one per license file, in
``find_files`` order (name score descending, files that score 0 dropped).

It is the *ordered* form -- real ``uniq``, real ``delete_at`` / ``unshift``, ``count == 1 || lgpl?`` --
where the device kernel is the order-free form, and it shares no code with licensee_amd/projects.py
or the kernel. License ids: ``0 .. T-1`` the templates, ``T`` = 'other', ``T + 1`` = 'no-license';
``None`` stands for Ruby's nil. ``gpl`` / ``lgpl`` are the sets of template ids with License#gpl? /
#lgpl? (license.rb:200-206). The filename tests are written out here (casecmp, the copyright?
regex of project_file.rb:94), not imported.
"""
import re

_COPYRIGHT_NAME = re.compile(r'\Acopyright(?:\.(?!xml|go|gemspec)([^./]|\.\d)+\Z)?\Z', re.I | re.A)


def name_is_lesser(name):
    """LicenseFile.lesser_gpl_score(filename) == 1 (license_file.rb:105-107)."""
    return name.lower() == 'copying.lesser'


def name_is_copyright(name):
    """The filename test of ProjectFile#copyright? (project_file.rb:94)."""
    return _COPYRIGHT_NAME.search(name) is not None


def uniq(xs):
    out = []
    for x in xs:
        if x not in out:
            out.append(x)
    return out


class OracleProject:
    def __init__(self, files, gpl, lgpl, T):
        self.found = list(files)          # [(filename, license_id, copyright_matched)]
        self.gpl_ids, self.lgpl_ids, self.T = set(gpl), set(lgpl), T
        self._license_files = None

    # LicenseFile#lgpl? / #gpl? (license_file.rb:84-90)
    def file_lgpl(self, f):
        return name_is_lesser(f[0]) and f[1] in self.lgpl_ids

    def file_gpl(self, f):
        return f[1] in self.gpl_ids

    # ProjectFile#copyright? (project_file.rb:90-95): the matcher is Copyright and the name is COPYRIGHT[.ext]
    def file_copyright(self, f):
        if not f[2]:
            return False
        return name_is_copyright(f[0])

    def prioritize_lgpl(self, files):
        if len(files) == 0:
            return files
        if not self.file_gpl(files[0]):
            return files
        lesser = next((i for i, f in enumerate(files) if self.file_lgpl(f)), None)
        if lesser is not None:
            x = files[lesser]
            del files[lesser]            # delete_at
            files.insert(0, x)           # unshift
        return files

    def license_files(self):
        if self._license_files is None:
            self._license_files = self.prioritize_lgpl(list(self.found))
        return self._license_files

    def matched_files(self):
        return [f for f in self.license_files() if f[1] is not None]     # select(&:license)

    def licenses(self):
        return uniq([f[1] for f in self.matched_files()])

    def licenses_without_copyright(self):
        return uniq([f[1] for f in self.matched_files() if not self.file_copyright(f)])

    def lgpl(self):
        if not (len(self.licenses()) == 2 and len(self.license_files()) == 2):
            return False
        lf = self.license_files()
        return self.file_lgpl(lf[0]) and self.file_gpl(lf[1])

    def license(self):
        lwc = self.licenses_without_copyright()
        if len(lwc) == 1 or self.lgpl():
            return lwc[0] if lwc else None
        if len(lwc) > 1:
            return self.T                # License.find('other')
        return None

    def matched_file(self):
        mf = self.matched_files()
        if len(mf) == 1 or self.lgpl():
            return mf[0] if mf else None
        return None

    def license_file(self):
        lf = self.license_files()
        if len(lf) == 1 or self.lgpl():
            return lf[0] if lf else None
        return None


def file_license(T, copyright_matched, exact, best, use_exact=True):
    """LicenseFile#license (license_file.rb:92-98) over [Copyright, Exact, Dice] as a license id."""
    if copyright_matched:
        return T + 1
    if use_exact and exact >= 0:
        return int(exact)
    if best >= 0:
        return int(best)
    return T
