"""Batched LicenseFile#license / #confidence / matcher over many files.

The reference evaluates ``[Copyright, Exact, Dice].map(new).find(&:match)`` per file
(license_file.rb:67-69, project_file.rb:69-80) and falls back to ``License 'other'``
(license_file.rb:92-98). Here the whole chain runs in bulk:

  host (liblicensee_host.so, threads): decode, content_normalized, Copyright, the CC flag
  GPU  (liblicensee_dice.so):          the wordset scan + vocabulary bitsets + field-word
                                       masks (dice_batch_upload_text, content_helper.rb:108-110),
                                       Exact#match (dice_batch_exact: |W_F| == |W_t| and
                                       W_t ⊆ W_F, exact.rb:6-12) and Dice#match / #confidence
                                       on the same resident batch; with ``content_hash=True``
                                       also ContentHelper#content_hash (dice_batch_content_hash:
                                       SHA-1 of the resident texts, content_helper.rb:136-138;
                                       the texts are then resident as UTF-8)
(``wordset_on='host'`` scans and interns in the host threads instead, the round-5 split;
``exact_on='host'`` keeps Exact in the host threads too, the round-2 split.)

Results equal the per-file Python chain (tests/test_gpu_golden.py::test_batch_chain).

``detect_projects`` answers for whole projects (Project#license, projects/project.rb:24-32): the
license files of all projects go through the same single upload / Exact / match, the device reduces
the resident per-file results to one record per project (dice_batch_projects), and only those
records are downloaded and turned into objects (tests/test_gpu_projects.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple, Union

from . import config
from .license import License


@dataclass(slots=True)
class Detection:
    license: License            # matched License, or License 'other'
    matcher: Optional[str]      # 'copyright' | 'exact' | 'dice' | None
    confidence: object          # 100 (copyright/exact), Float (dice), None (no matcher)
    content_hash: Optional[str] = None   # content_hash (SHA-1 hex), BatchDetector(content_hash=True) only


@dataclass(slots=True)
class ProjectDetection:
    license: Optional[License]          # Project#license (project.rb:24-32); None for nil
    matched_file: Optional[str]         # Project#matched_file's filename (project.rb:40-42), or None
    matcher: Optional[str]              # the matched file's matcher: 'copyright' | 'exact' | 'dice' | None
    confidence: object                  # its confidence: 100, Float (dice), None (no matcher or no matched file)
    licenses: List[License]             # the first k_licenses entries of Project#licenses (project.rb:35-37)
    n_licenses: int                     # Project#licenses.count, exact
    n_files: int                        # Project#license_files.count
    content_hash: Optional[str] = None  # the matched file's content_hash, BatchDetector(content_hash=True) only


class BatchDetector:
    """One resident template corpus on the device + one native host context.

    ``engine`` defaults to the process-wide :func:`dice.default_engine` (the vendored
    corpus); pass a :class:`dice.DiceEngine` to use another corpus or device.

    ``content_hash=True`` fills ``Detection.content_hash`` (ContentHelper#content_hash,
    content_helper.rb:136-138) for every file, whatever matcher decided it: the device hashes the
    normalized texts it already holds for the wordset scan. Those texts are then kept as the UTF-8
    of content_normalized (``lh_normalize_files_utf8`` / ``dice_batch_upload_text_utf8``), so the
    device's digest is content_hash for non-ASCII files too; only a file the device flags is hashed
    on the host threads, and ``host_hashed`` counts those of the last ``detect`` or stream batch
    (none on this path). ``content_hash=False`` keeps the one-byte-per-character texts."""

    def __init__(self, engine=None, nthreads: int = 8, exact_on: str = 'device', wordset_on: str = 'device',
                 content_hash: bool = False):
        from .dice import default_engine
        from .native_host import HostPrep
        if exact_on not in ('device', 'host'):
            raise ValueError("exact_on is 'device' or 'host'")
        if wordset_on not in ('device', 'host'):
            raise ValueError("wordset_on is 'device' or 'host'")
        self.engine = engine if engine is not None else default_engine()
        self.host = HostPrep(self.engine.corpus)
        self.nthreads = nthreads
        self.exact_on = exact_on if self.host.field_need is not None else 'host'
        # the device scan reports the non-vocabulary field words as mask bits for device Exact
        self.wordset_on = wordset_on if self.exact_on == 'device' else 'host'
        if content_hash and self.wordset_on != 'device':
            raise ValueError("content_hash=True hashes the normalized texts resident on the device, which only "
                             "wordset_on='device' uploads (it resolved to 'host': wordset_on or exact_on is 'host', "
                             "or the corpus has more than 64 field words outside the vocabulary)")
        self.content_hash = bool(content_hash)
        self._batch = None          # one device batch, reused by every detect() and grown on demand
        self._pinned = [None, None]  # page-locked text buffers: batch k uploads from one while k + 1 fills the other
        self._turn = 0
        self._pool = None           # threads of the content-hash completion (content_hash=True, on demand)
        self.host_hashed = 0        # files of the last batch whose content_hash came from the host
        self._name_info = {}        # detect_projects: filename -> (name score, name bits)
        if self.exact_on == 'device':
            self.engine.scorer.exact_setup(*exact_tables(self.engine.corpus, self.host))
        if self.wordset_on == 'device':
            self.engine.scorer.vocab_setup(self.engine.corpus.vocab, self.host.nv_fields)

    def _device_batch(self, n: int):
        if self._batch is None or self._batch.capacity < n:
            if self._batch is not None:
                self._batch.close()
            cap = max(n, 64) if self._batch is None else max(n, 2 * self._batch.capacity)
            self._batch = self.engine.scorer.batch(cap)
        return self._batch

    def close(self):
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None
        if self._batch is not None:
            self._batch.close()
            self._batch = None
        for i, p in enumerate(self._pinned):
            if p is not None:
                p.close()
                self._pinned[i] = None

    def _text_buffer(self, nbytes: int):
        """The next page-locked text buffer (alternating, grown on demand)."""
        from ._native import PinnedBuffer
        i = self._turn
        self._turn ^= 1
        p = self._pinned[i]
        if p is None or p.nbytes < nbytes:
            if p is not None:
                p.close()
            p = self._pinned[i] = PinnedBuffer(max(nbytes, 2 * p.nbytes if p is not None else nbytes))
        return p.array

    def detect(self, contents: Sequence[Union[str, bytes]], filenames: Optional[Sequence[str]] = None,
               threshold=None) -> List[Detection]:
        thr = config.confidence_threshold() if threshold is None else threshold
        return self._score(self._prep(contents, filenames), thr)

    def detect_stream(self, batches: Iterable[Tuple[Sequence[Union[str, bytes]], Optional[Sequence[str]]]],
                      threshold=None) -> Iterator[List[Detection]]:
        """detect() over a stream of (contents, filenames) batches as a two-stage pipeline: the
        native host threads prepare batch k + 1 (decode, normalize, intern, Copyright) while batch
        k is uploaded, matched on the device and turned into Detections. Yields one list per batch,
        in order, each equal to detect() of that batch."""
        from concurrent.futures import ThreadPoolExecutor
        thr = config.confidence_threshold() if threshold is None else threshold
        it = iter(batches)
        with ThreadPoolExecutor(1) as ex:
            nxt = next(it, None)
            fut = ex.submit(self._prep, *nxt) if nxt is not None else None
            while fut is not None:
                prepped = fut.result()
                nxt = next(it, None)
                fut = ex.submit(self._prep, *nxt) if nxt is not None else None
                yield self._score(prepped, thr)

    def detect_projects(self, projects: Sequence[Sequence[Tuple[str, Union[str, bytes]]]], threshold=None,
                        k_licenses: int = 4) -> List[ProjectDetection]:
        """Project#license, #matched_file and #licenses (projects/project.rb:24-47; detect_readme and
        detect_packages false) for every project: a sequence of ``(filename, content)`` per project,
        any files, in the caller's order. Equal to ``projects.Project(files)`` per project."""
        thr = config.confidence_threshold() if threshold is None else threshold
        return self._score_projects(self._prep_projects(projects), thr, k_licenses)

    def detect_projects_stream(self, batches: Iterable[Sequence[Sequence[Tuple[str, Union[str, bytes]]]]],
                               threshold=None, k_licenses: int = 4) -> Iterator[List[ProjectDetection]]:
        """detect_projects() over a stream of batches of projects, as detect_stream's two-stage
        pipeline: the host prepares batch k + 1 while batch k is on the device. Yields one list per
        batch, in order, each equal to detect_projects() of that batch."""
        from concurrent.futures import ThreadPoolExecutor
        thr = config.confidence_threshold() if threshold is None else threshold
        it = iter(batches)
        with ThreadPoolExecutor(1) as ex:
            nxt = next(it, None)
            fut = ex.submit(self._prep_projects, nxt) if nxt is not None else None
            while fut is not None:
                prepped = fut.result()
                nxt = next(it, None)
                fut = ex.submit(self._prep_projects, nxt) if nxt is not None else None
                yield self._score_projects(prepped, thr, k_licenses)

    def _prep_projects(self, projects):
        """Host stage of detect_projects: Project#find_files per project (project.rb:111-117: name
        scores, files that score 0 dropped, score descending -- stably, the caller's order within a
        score), all license files of all projects as one flat batch through _prep, and per file the
        name bits of dice_batch_projects' file_flags."""
        import numpy as np
        from .project_files import LicenseFile, is_copyright_file
        if self.exact_on != 'device':
            raise ValueError("detect_projects reduces the device's resident Exact results: it needs exact_on='device'")
        # per file only list comprehensions and a dictionary lookup; the select, the stable sort and
        # the offsets are array operations over the whole batch
        flat = [f for files in projects for f in files]
        names = [f[0] for f in flat]
        known = self._name_info      # filename -> (name score, name bits)
        if len(known) > (1 << 16):
            known.clear()
        for nm in set(names).difference(known):
            known[nm] = (LicenseFile.name_score(nm),
                         (2 if is_copyright_file(nm) else 0) | (4 if LicenseFile.lesser_gpl_score(nm) else 0))
        info = [known[nm] for nm in names]
        n_all = len(flat)
        score = np.fromiter((e[0] for e in info), np.float64, n_all)
        bits = np.fromiter((e[1] for e in info), np.uint8, n_all)
        sizes = np.fromiter((len(files) for files in projects), np.int64, len(projects))
        pid = np.repeat(np.arange(len(projects)), sizes)
        keep = np.flatnonzero(score > 0)
        order = keep[np.lexsort((-score[keep], pid[keep]))]      # (a stable sort: project, then score descending)
        offsets = np.zeros(len(projects) + 1, np.int64)
        np.cumsum(np.bincount(pid[keep], minlength=len(projects)), out=offsets[1:])
        if order.size == n_all and np.array_equal(order, np.arange(n_all)):
            contents = [f[1] for f in flat]     # (nothing dropped, nothing moved)
        else:
            order_l = order.tolist()
            names = [names[i] for i in order_l]
            contents = [flat[i][1] for i in order_l]
            bits = bits[order]
        return self._prep(contents, names), names, offsets, bits

    def _template_flags(self):
        """dice_batch_projects' template_flags: bit 0 License#gpl?, bit 1 #lgpl? (license.rb:200-206)."""
        import numpy as np
        if getattr(self, '_tflags', None) is None:
            self._tflags = np.fromiter(((1 if l.gpl() else 0) | (2 if l.lgpl() else 0) for l in self.engine.templates),
                                       np.uint8, len(self.engine.templates))
        return self._tflags

    def _score_projects(self, prepped, thr, k) -> List[ProjectDetection]:
        """Device stage of detect_projects: the flat batch's upload / Exact / match as detect() runs
        them, the project reduction on their resident results, and one record per project back."""
        import numpy as np
        inner, names, offsets, bits = prepped
        if inner[0] == 'text':
            b = self._resident_text(inner)
            copyright = inner[1][5]
        else:
            fb, copyright, third = inner
            b = self._device_batch(max(fb.n, 1))
            b.upload(fb)
            b.exact(third)
        b.match(float(thr), confidence=True)
        self.host_hashed = 0
        flags = (np.asarray(copyright).astype(np.uint8) & 1) | bits
        b.projects(offsets, flags, self._template_flags(), use_exact=True, k=k)
        lic, mf, nl, lst = b.download_projects()
        mt, cf, dg = b.download_project_match(digest=self.content_hash)
        templates = self.engine.templates
        tab = list(templates) + [License.find('other'), License.find('no-license'), None]    # (-1: nil)
        matcher_names = ('copyright', 'exact', 'dice', None)
        hx = dg.tobytes().hex() if dg is not None else None
        sizes = np.diff(offsets).tolist()
        import gc
        paused = gc.isenabled()
        gc.disable()     # (as _detections)
        try:
            out = []
            for p, (l, f, m, c, row, cnt, sz) in enumerate(zip(lic.tolist(), mf.tolist(), mt.tolist(), cf.tolist(),
                                                               lst.tolist(), nl.tolist(), sizes)):
                out.append(ProjectDetection(
                    tab[l], names[f] if f >= 0 else None, matcher_names[m],
                    (c if m == 2 else 100) if m >= 0 else None,
                    [tab[x] for x in row if x >= 0], cnt, sz,
                    hx[40 * p:40 * p + 40] if hx is not None and f >= 0 else None))
            return out
        finally:
            if paused:
                gc.enable()

    def _prep(self, contents, filenames=None):
        """Host stage (liblicensee_host.so threads; ctypes releases the GIL during the call)."""
        if self.wordset_on == 'device':
            return ('text', self.host.normalize_files(contents, filenames, nthreads=self.nthreads,
                                                      out=self._text_buffer, utf8=self.content_hash),
                    contents, filenames)
        field_masks = self.exact_on == 'device'
        fb, copyright, third, _ = self.host.prep_files(contents, filenames, nthreads=self.nthreads,
                                                       field_masks=field_masks)
        return fb, copyright, third

    def _score_text(self, prepped, thr):
        """Device stage of wordset_on='device': upload the normalized texts (the device scans and
        interns the wordsets), patch the rare files whose distinct non-vocabulary words overflow
        the device set with host-prepared rows, then Exact + Dice#match/#confidence."""
        _, (text, off, tl, ln, cc, copyright, _), contents, filenames = prepped
        b = self._resident_text(prepped)
        b.match(float(thr), confidence=True)
        exact = b.download_exact()
        best, _, score = b.download_match()
        self.host_hashed = 0
        hashes = self._hashes(b, contents, filenames) if self.content_hash else None
        return copyright, exact, best, score, hashes

    def _resident_text(self, prepped):
        """The texts of a wordset_on='device' batch made resident: upload and scan, the content hash
        when asked for, host-prepared rows for the files the device scan flagged, and Exact."""
        import numpy as np
        _, (text, off, tl, ln, cc, copyright, _), contents, filenames = prepped
        n = len(off)
        b = self._device_batch(max(n, 1))
        st = b.upload_text(text, off, tl, ln, cc, utf8=self.content_hash)   # (as _prep normalized them)
        if self.content_hash:
            b.content_hash()
        over = np.nonzero(st)[0]
        if over.size:
            sub = [contents[i] for i in over]
            sfn = [filenames[i] for i in over] if filenames is not None else None
            fb, _, fm, _ = self.host.prep_files(sub, sfn, nthreads=self.nthreads, field_masks=True)
            b.set_rows(over, fb.bits, fb.wordset_size, fm)
        b.exact(None)
        return b

    def _hashes(self, b, contents, filenames) -> List[str]:
        """content_hash per file as hex: the device digests, and for the files the device flagged
        (none when the resident texts are UTF-8; in the one-byte form a text with a non-ASCII
        character, resident as 0x80) the SHA-1 of content_normalized's UTF-8 from the host threads
        (the native normalize releases the GIL)."""
        import hashlib
        import numpy as np
        digest, status = b.download_content_hash()
        hx = digest.tobytes().hex()     # in bulk (as _detections: no per-file numpy work)
        hashes = [hx[i:i + 40] for i in range(0, len(hx), 40)]
        flagged = np.nonzero(status)[0].tolist()
        self.host_hashed = len(flagged)
        if flagged:
            # contiguous slices, one per thread: few hand-overs of the GIL between the native calls
            k = max(1, min(self.nthreads, len(flagged) // 8))
            parts = [flagged[len(flagged) * j // k:len(flagged) * (j + 1) // k] for j in range(k)]

            def some(part):
                sub = [contents[i] for i in part]
                sfn = [filenames[i] for i in part] if filenames is not None else None
                done = self.host.content_hashes(sub, sfn)
                for j, i in enumerate(part):
                    if done[j] is None:     # outside the native normalizer's envelope
                        from .project_files import LicenseFile
                        lf = LicenseFile(sub[j], sfn[j] if sfn is not None else 'LICENSE')
                        done[j] = hashlib.sha1((lf.content_normalized() or '').encode('utf-8')).hexdigest()
                return done
            if k > 1:
                if self._pool is None:
                    from concurrent.futures import ThreadPoolExecutor
                    self._pool = ThreadPoolExecutor(self.nthreads)
                results = list(self._pool.map(some, parts))
            else:
                results = [some(parts[0])]
            for part, done in zip(parts, results):
                for i, h in zip(part, done):
                    hashes[i] = h
        return hashes

    def _score(self, prepped, thr) -> List[Detection]:
        """Device stage: Exact (device) + Dice#match/#confidence, then the matcher chain's order."""
        if prepped[0] == 'text':
            copyright, exact, best, score, hashes = self._score_text(prepped, thr)
            return self._detections(copyright, exact, best, score, hashes)
        fb, copyright, third = prepped
        if self.exact_on == 'device':
            b = self._device_batch(max(fb.n, 1))
            b.upload(fb)
            b.exact(third)
            b.match(float(thr), confidence=True)
            exact = b.download_exact()
            best, _, score = b.download_match()
        else:
            exact = third
            best, _, score = self.engine.scorer.match(fb, float(thr), confidence=True)
        return self._detections(copyright, exact, best, score)

    def _detections(self, copyright, exact, best, score, hashes=None) -> List[Detection]:
        templates = self.engine.templates
        no_license, other = License.find('no-license'), License.find('other')
        # the matcher chain's order per file (Copyright, Exact, Dice, else 'other'), over Python lists
        # (numpy scalar indexing per file cost as much as the host preparation of the next batch);
        # the cyclic collector paused while the batch's objects are made (they hold no cycles, and
        # in a process with a large heap its passes cost more than the objects themselves)
        import gc
        paused = gc.isenabled()
        gc.disable()
        try:
            if hashes is not None:
                return [Detection(no_license, 'copyright', 100, h) if c else
                        Detection(templates[e], 'exact', 100, h) if e >= 0 else
                        Detection(templates[bi], 'dice', sc, h) if bi >= 0 else
                        Detection(other, None, None, h)
                        for c, e, bi, sc, h in zip(copyright.tolist(), exact.tolist(), best.tolist(), score.tolist(),
                                                   hashes)]
            return [Detection(no_license, 'copyright', 100) if c else
                    Detection(templates[e], 'exact', 100) if e >= 0 else
                    Detection(templates[bi], 'dice', sc) if bi >= 0 else
                    Detection(other, None, None)
                    for c, e, bi, sc in zip(copyright.tolist(), exact.tolist(), best.tolist(), score.tolist())]
        finally:
            if paused:
                gc.enable()


def exact_tables(corpus, host):
    """dice_exact_setup's tables for a TemplateCorpus: |wordset| per template, its field words
    that are vocabulary words as bitsets, the others as bits of ``host.nv_fields``
    (content_helper.rb:323-335: wordset = wordset_fieldless + the field words)."""
    import numpy as np
    T = len(corpus.templates)
    bits = np.zeros((T, corpus.w64), np.uint64)
    for t, tpl in enumerate(corpus.templates):
        for w in set(tpl.fields_normalized()):
            i = corpus.index.get(w)
            if i is not None:
                bits[t, i >> 6] |= np.uint64(1 << (i & 63))
    return host._ws, bits, host.field_need
