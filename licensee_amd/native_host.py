"""Native host preparation (licensee_amd/lib/liblicensee_host.so, csrc/normalize.cpp + rx.cpp).

Batched LicenseFile preparation in C++ threads: decode -> content_normalized -> wordset ->
vocabulary bitset, plus the CC flag, the Copyright matcher and the Exact matcher. The regular
expressions are exactly the compiled patterns of ``content_helper.py`` (handed over here),
so the two host paths share one pattern source, and Python's own Unicode tables
(``unicode_tables``: lower-casing, ``\\w``) so non-ASCII text stays native. Texts the native
path does not cover (HTML; the five characters whose Python semantics are contextual, see
normalize.cpp ``python_only``) fall back to the Python path per file.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import content_helper as ch
from ._native import FileBatch
from .license import License

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'liblicensee_host.so')
_FLAG_MASK = 2 | 8 | 16   # re.I | re.M | re.S
_lib = None


def _load():
    global _lib
    if _lib is None:
        l = ctypes.CDLL(LIB_PATH)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        cpp = ctypes.POINTER(ctypes.c_char_p)
        l.lh_create.restype = vp
        l.lh_create.argtypes = [i32, cpp, cpp, vp, i32, cpp, cpp, i32, cpp, ctypes.c_char_p, i32]
        l.lh_destroy.argtypes = [vp]
        l.lh_set_templates.restype = ctypes.c_int
        l.lh_set_templates.argtypes = [vp, i32, vp, vp, vp, cpp]
        l.lh_normalize.restype = i64
        l.lh_normalize.argtypes = [vp, ctypes.c_char_p, i64, ctypes.c_char_p, i32, ctypes.c_char_p, i64]
        l.lh_prep_files.restype = ctypes.c_int
        l.lh_prep_files.argtypes = [vp, i64, cpp, vp, cpp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        l.lh_template_field_masks.restype = i32
        l.lh_template_field_masks.argtypes = [vp, vp]
        l.lh_normalize_files.restype = i64
        l.lh_normalize_files.argtypes = [vp, i64, cpp, vp, cpp, i32, vp, i64, vp, vp, vp, vp, vp, vp]
        l.lh_normalize_files_utf8.restype = i64
        l.lh_normalize_files_utf8.argtypes = l.lh_normalize_files.argtypes
        l.lh_set_unicode.restype = ctypes.c_int
        l.lh_set_unicode.argtypes = [vp, i32, vp, vp, i32, vp, vp]
        _lib = l
    return _lib


_UNICODE = None


def unicode_tables():
    """Python's own per-character semantics the native normalizer needs for non-ASCII text:
    (lower_from, lower_to) for every code point whose ``str.lower()`` is a different single
    code point, and the inclusive ranges of non-ASCII code points with ``str.isalnum()``
    (``re``'s Unicode ``\\w``, which decides ``\\b``)."""
    global _UNICODE
    if _UNICODE is None:
        import sys
        frm, to, lo, hi = [], [], [], []
        start = None
        for cp in range(128, sys.maxunicode + 1):
            ch = chr(cp)
            low = ch.lower()
            if low != ch and len(low) == 1:
                frm.append(cp)
                to.append(ord(low))
            if ch.isalnum():
                if start is None:
                    start = cp
            elif start is not None:
                lo.append(start)
                hi.append(cp - 1)
                start = None
        if start is not None:
            lo.append(start)
            hi.append(sys.maxunicode)
        _UNICODE = tuple(np.array(a, np.uint32) for a in (frm, to, lo, hi))
    return _UNICODE


def _bytes_data_offset():
    """Offset of a bytes object's data from its id() in this interpreter (CPython: the object
    header), or None if that does not hold -- checked against ctypes' own pointer."""
    import sys
    off = sys.getsizeof(b'') - 1
    probe = [b'licensee', b'x' * 100, bytes(range(1, 200))]
    for b in probe:
        if ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value != id(b) + off:
            return None
    return off


_BYTES_OFF = _bytes_data_offset()


def _cstrs(items: Sequence[Union[str, bytes]]):
    """(char** of the items' UTF-8 bytes, the list that keeps them alive). Bytes items are passed
    without a copy; the pointer array is built from their addresses in one numpy step (building
    it through ctypes cost ~0.8 us per item, as much as a tenth of the native preparation)."""
    enc = [x if isinstance(x, bytes) else x.encode('utf-8') for x in items]
    if _BYTES_OFF is None or not enc:
        arr = (ctypes.c_char_p * max(len(enc), 1))(*enc)
        return arr, enc
    ptrs = np.fromiter(map(id, enc), np.uint64, len(enc)) + np.uint64(_BYTES_OFF)
    return ctypes.cast(ptrs.ctypes.data, ctypes.POINTER(ctypes.c_char_p)), (enc, ptrs)


def host_patterns():
    """(name, compiled pattern) pairs the native normalizer runs (content_helper.py)."""
    from .project_files import CC_FALSE_POSITIVE_REGEX
    R, N = ch.REGEXES, ch.NORMALIZATIONS
    pats = {k: R[k] for k in ('hrs', 'comment_markup', 'markdown_headings', 'link_markup', 'version', 'bom',
                             'cc_dedication', 'cc_wiki', 'cc_legal_code', 'cc0_info', 'cc0_disclaimer',
                             'unlicense_info', 'border_markup', 'url', 'block_markup', 'developed_by',
                             'whitespace', 'mit_optional', 'bullet', 'span_markup')}
    pats.update({k: N[k][0] for k in ('lists', 'https', 'dashes', 'quote', 'hyphenated')})
    pats.update({'spelling': ch._SPELLING_REGEX, 'bullet_paren': ch._BULLET_PAREN_REGEX,
                 'end_of_terms': ch.END_OF_TERMS_REGEX, 'strip_copyright': ch._STRIP_COPYRIGHT_REGEX,
                 'title': License.title_regex(), 'cc_false_positive': CC_FALSE_POSITIVE_REGEX,
                 'copyright_match': ch.COPYRIGHT_MATCH_REGEX})
    return pats


class HostPrep:
    def __init__(self, corpus=None):
        """``corpus``: a TemplateCorpus (vocabulary + Exact data); None = normalize only."""
        lib = _load()
        pats = host_patterns()
        names, self._k1 = _cstrs(list(pats))
        srcs, self._k2 = _cstrs([p.pattern for p in pats.values()])
        flags = np.array([p.flags & _FLAG_MASK for p in pats.values()], np.int32)
        sf, self._k3 = _cstrs(list(ch.VARIETAL_WORDS))
        st, self._k4 = _cstrs(list(ch.VARIETAL_WORDS.values()))
        vocab = corpus.vocab if corpus is not None else []
        vw, self._k5 = _cstrs(vocab)
        err = ctypes.create_string_buffer(512)
        self._flags = flags
        self._c = lib.lh_create(len(pats), names, srcs, flags.ctypes.data, len(ch.VARIETAL_WORDS), sf, st,
                                len(vocab), vw, err, 512)
        if not self._c:
            raise RuntimeError('lh_create failed: ' + err.value.decode())
        self._uni = unicode_tables()
        lf, lt, wl, wh = self._uni
        if lib.lh_set_unicode(self._c, len(lf), lf.ctypes.data, lt.ctypes.data, len(wl), wl.ctypes.data,
                              wh.ctypes.data) != 0:
            raise RuntimeError('lh_set_unicode rejected the tables')
        self.corpus = corpus
        if corpus is not None:
            tpl = corpus.templates
            ws = np.array([len(t.wordset()) for t in tpl], np.uint32)
            fields, off = [], [0]
            for t in tpl:
                fs = sorted(set(t.fields_normalized()))
                fields.extend(fs)
                off.append(len(fields))
            fw, self._k6 = _cstrs(fields)
            self._off = np.array(off, np.int32)
            self._ws = ws
            self._lf = np.ascontiguousarray(corpus.lf_bits)
            lib.lh_set_templates(self._c, len(tpl), self._lf.ctypes.data, ws.ctypes.data, self._off.ctypes.data, fw)
            # Exact on the device (dice_batch_exact): the field words outside the vocabulary,
            # numbered in first-appearance order as the native side numbers them
            vocab_set = set(corpus.vocab)
            self.nv_fields = []
            for f in fields:
                if f not in vocab_set and f not in self.nv_fields:
                    self.nv_fields.append(f)
            need = np.zeros(len(tpl), np.uint64)
            cnt = lib.lh_template_field_masks(self._c, need.ctypes.data)
            self.field_need = need if cnt >= 0 else None
            assert cnt == (len(self.nv_fields) if len(self.nv_fields) <= 64 else -1)

    def __del__(self):
        if getattr(self, '_c', None):
            _load().lh_destroy(self._c)
            self._c = None

    def normalize(self, content: Union[str, bytes], filename: Optional[str] = None, is_file: bool = True) -> Optional[str]:
        """Native content_normalized, or None when the text needs the Python path."""
        data = content if isinstance(content, bytes) else content.encode('utf-8')
        fn = filename.encode('utf-8') if filename else None
        n = _load().lh_normalize(self._c, data, len(data), fn, 1 if is_file else 0, None, 0)
        if n < 0:
            return None
        buf = ctypes.create_string_buffer(n + 1)
        _load().lh_normalize(self._c, data, len(data), fn, 1 if is_file else 0, buf, n + 1)
        return buf.raw[:n].decode('utf-8')

    def content_hashes(self, contents: Sequence[Union[str, bytes]], filenames: Optional[Sequence[str]] = None) -> list:
        """ContentHelper#content_hash (content_helper.rb:136-138) of each file: the SHA-1 hex of the
        native content_normalized's UTF-8, or None for a file outside the native envelope. One
        normalization per file into a buffer reused over the call (a second only when the text
        outgrows it), hashed where it lies; both release the GIL, so callers run this in threads."""
        import hashlib
        lib = _load()
        out = []
        cap, ba, cbuf = 0, None, None
        for i, content in enumerate(contents):
            data = content if isinstance(content, bytes) else content.encode('utf-8')
            fn = filenames[i].encode('utf-8') if filenames is not None and filenames[i] else None
            if cap < len(data) + 256:
                cap = 2 * len(data) + 4096
                ba = bytearray(cap)
                cbuf = (ctypes.c_char * cap).from_buffer(ba)
            n = lib.lh_normalize(self._c, data, len(data), fn, 1, cbuf, cap)
            if n >= cap:    # (the text was not written)
                cap = 2 * n + 4096
                ba = bytearray(cap)
                cbuf = (ctypes.c_char * cap).from_buffer(ba)
                n = lib.lh_normalize(self._c, data, len(data), fn, 1, cbuf, cap)
            out.append(None if n < 0 else hashlib.sha1(memoryview(ba)[:n]).hexdigest())
        return out

    def prep_files(self, contents: Sequence[Union[str, bytes]], filenames: Optional[Sequence[str]] = None,
                   nthreads: int = 8, field_masks: bool = False) -> Tuple[FileBatch, np.ndarray, np.ndarray, np.ndarray]:
        """Returns (FileBatch, copyright flags, exact template index or -1, fell_back mask).
        Files the native path does not cover are prepared by the Python LicenseFile path.
        field_masks=True: Exact is left to the device (dice_batch_exact) and the third value is
        instead each file's field mask (bit k = its wordset holds ``self.nv_fields[k]``)."""
        if self.corpus is None:
            raise ValueError('prep_files needs a TemplateCorpus')
        n = len(contents)
        data, keep = _cstrs(contents)
        enc = keep[0] if isinstance(keep, tuple) else keep
        lens = np.fromiter(map(len, enc), np.int64, n)
        fns = None
        if filenames is not None:
            fns, self._kf = _cstrs(filenames)
        w64 = self.corpus.w64
        bits = np.zeros((n, w64), np.uint64)
        wf = np.zeros(n, np.uint32)
        ln = np.zeros(n, np.int32)
        cc = np.zeros(n, np.uint8)
        cr = np.zeros(n, np.uint8)
        ex = np.full(n, -1, np.int32)
        st = np.zeros(n, np.uint8)
        fm = np.zeros(n, np.uint64) if field_masks else None
        if field_masks and self.field_need is None:
            raise ValueError('more than 64 template field words outside the vocabulary')
        rc = _load().lh_prep_files(self._c, n, data, lens.ctypes.data, fns, nthreads, bits.ctypes.data,
                                   wf.ctypes.data, ln.ctypes.data, cc.ctypes.data, cr.ctypes.data,
                                   None if field_masks else ex.ctypes.data, st.ctypes.data,
                                   fm.ctypes.data if field_masks else None)
        if rc != 0:
            raise RuntimeError('lh_prep_files failed')
        fell = st != 0
        if fell.any():
            from .matchers import Copyright, Exact
            from .project_files import LicenseFile
            idx = {t.key: i for i, t in enumerate(self.corpus.templates)}
            for i in np.nonzero(fell)[0]:
                lf = LicenseFile(contents[i], filenames[i] if filenames is not None else 'LICENSE')
                bits[i], wf[i] = self.corpus.intern(lf.wordset() or frozenset())
                ln[i] = lf.length()
                cc[i] = lf.potential_false_positive()
                cr[i] = Copyright(lf).match() is not None
                e = Exact(lf).match()
                ex[i] = idx.get(e.key, -1) if e is not None else -1
                if field_masks:
                    ws = lf.wordset() or frozenset()
                    fm[i] = sum(1 << k for k, w in enumerate(self.nv_fields) if w in ws)
        if field_masks:
            return FileBatch(bits, wf, ln, cc), cr.astype(bool), fm, fell
        return FileBatch(bits, wf, ln, cc), cr.astype(bool), ex, fell

    def normalize_files(self, contents: Sequence[Union[str, bytes]], filenames: Optional[Sequence[str]] = None,
                        nthreads: int = 8, out=None, utf8: bool = False):
        """Batched content_normalized for the device wordset scan (``lh_normalize_files``;
        ``DeviceBatch.upload_text``). Returns (text uint8 [bytes], offsets [n] int64 (16-byte
        aligned), text_len [n] int32, length [n] int32, cc [n] uint8, copyright [n] bool, fell [n]
        bool): file i's normalized text at ``text[offsets[i]:offsets[i] + text_len[i]]``, one byte
        per character (non-ASCII characters as 0x80: the wordset's ``[\\w/-]`` is ASCII). Files the
        native path does not cover (``fell``) are normalized by the Python path and appended.
        ``utf8=True`` (``lh_normalize_files_utf8``; ``upload_text(..., utf8=True)``): every text,
        the appended ones too, is the UTF-8 of content_normalized, ``text_len`` in bytes and
        ``length`` in characters.
        ``out``: a callable ``out(nbytes) -> uint8 array`` giving the buffer to write into (e.g. a
        page-locked one, ``_native.PinnedBuffer``); default a new numpy array."""
        lib = _load()
        n = len(contents)
        data, keep = _cstrs(contents)
        enc = keep[0] if isinstance(keep, tuple) else keep
        lens = np.fromiter(map(len, enc), np.int64, n)
        fns = None
        if filenames is not None:
            fns, _kf = _cstrs(filenames)
        cap = int(lens.sum()) + 16 * n + (1 << 16)
        buf = out(cap) if out is not None else np.empty(cap, np.uint8)
        cap = int(buf.shape[0])
        off = np.full(n, -1, np.int64)
        tl = np.zeros(n, np.int32)
        ln = np.zeros(n, np.int32)
        cc = np.zeros(n, np.uint8)
        cr = np.zeros(n, np.uint8)
        st = np.zeros(n, np.uint8)
        fn = lib.lh_normalize_files_utf8 if utf8 else lib.lh_normalize_files
        used = fn(self._c, n, data, lens.ctypes.data, fns, nthreads, buf.ctypes.data, cap, off.ctypes.data,
                  tl.ctypes.data, ln.ctypes.data, cc.ctypes.data, cr.ctypes.data, st.ctypes.data)
        if used < 0:
            raise RuntimeError('lh_normalize_files failed')
        # the rest by Python (no room left: rare expansions; outside the native envelope), appended
        extra = []
        for i in np.nonzero(st != 0)[0]:
            i = int(i)
            if st[i] == 3:   # normalized natively (flags set) but no room left in the buffer
                txt = self.normalize(contents[i], filenames[i] if filenames is not None else None)
                extra.append((i, txt, None))
                continue
            from .matchers import Copyright
            from .project_files import LicenseFile
            lf = LicenseFile(contents[i], filenames[i] if filenames is not None else 'LICENSE')
            cn = lf.content_normalized() or ''
            extra.append((i, cn, (lf.potential_false_positive(), Copyright(lf).match() is not None)))
        if extra:
            parts = []
            at = int(used)
            for i, txt, flags in extra:
                if utf8 or txt.isascii():
                    b = txt.encode('utf-8')
                else:
                    b = bytes(c if c < 0x80 else 0x80 for c in (ord(ch) for ch in txt))
                off[i] = at
                tl[i] = len(b)
                ln[i] = len(txt)
                if flags is not None:
                    cc[i], cr[i] = flags
                pad = (-len(b)) % 16
                parts.append(b + b'\0' * pad)
                at += len(b) + pad
            tail = np.frombuffer(b''.join(parts), np.uint8)
            buf = np.concatenate([buf[:used], tail])
            used = at
        return buf[:used], off, tl, ln, cc, cr.astype(bool), st == 1
