"""What resolving projects on the device costs against doing it on the host (dice_batch_projects).

    python tools/project_rate.py [--files 1000000] [--launches 20] [--streams 3] [--no-stream]

Part 1 -- a resident synthetic batch of `--files` config-2 files, matched, cut into projects of 1-5
files (about 0.4 projects per file). Two ways to one record per project, each timed with HIP events
around the calls, the median of `--launches`:
  device  dice_batch_projects + dice_batch_download_projects (16 B + 4 k B per project come back)
  host    dice_batch_download_exact + dice_batch_download_match (20 B per file come back) and a numpy
          restatement of the same reduction (license, matched_file, n_licenses; not the ordered list),
          whose time is the wall clock of the numpy part added to the event time of the downloads
The two agree on license / matched_file / n_licenses (asserted).

Part 2 -- bench.py's 16,000 synthetic texts as 4,000-file batches, two passes (its end-to-end text
workload), every file named LICENSE and grouped three to a project: detect_projects_stream against
detect_stream followed by the same grouping done on the host over the Detection objects, `--streams`
streams each, alternating. One JSON line per part.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    s = sorted(v)
    return s[len(s) // 2]


def timed(fn, stream, launches):
    """Per launch of fn(): microseconds between two HIP events; fn returns extra host microseconds."""
    import torch
    us = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        extra = fn() or 0.0
        e1.record(stream)
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 + extra)
    return us


def numpy_resolve(offsets, flags, tflags, exact, best, T):
    """The order-free rule of csrc/dice_project.hip over whole arrays (no licenses[] list)."""
    import numpy as np
    P = len(offsets) - 1
    L = np.where(flags & 1, T + 1, np.where(exact >= 0, exact, np.where(best >= 0, best, T))).astype(np.int64)
    size = np.diff(offsets)
    pid = np.repeat(np.arange(P), size)
    # distinct licenses per project: unique (project, license) pairs
    pairs = np.unique(pid * (T + 2) + L)
    nl = np.bincount(pairs // (T + 2), minlength=P).astype(np.int32)
    keep = (flags & 3) != 3
    kp = np.unique(pid[keep] * (T + 2) + L[keep])
    d = np.bincount(kp // (T + 2), minlength=P)
    first = np.full(P, -1, np.int64)
    first[(kp // (T + 2))[::-1]] = (kp % (T + 2))[::-1]
    lic = np.where(d == 1, first, np.where(d > 1, T, -1)).astype(np.int32)
    mf = np.where(size == 1, offsets[:-1], -1).astype(np.int32)
    # lgpl?: two files, one COPYING.lesser with an LGPL license, the other with a GPL license
    two = np.flatnonzero(size == 2)
    a, b = offsets[two], offsets[two] + 1
    tf = np.concatenate([tflags, [0, 0]])
    la, lb = (flags[a] & 4) != 0, (flags[b] & 4) != 0
    lg0 = la & ((tf[L[a]] & 2) != 0) & ((tf[L[b]] & 1) != 0)
    lg1 = lb & ((tf[L[b]] & 2) != 0) & ((tf[L[a]] & 1) != 0) & ~lg0
    lic[two[lg0]], mf[two[lg0]] = L[a[lg0]], a[lg0]
    lic[two[lg1]], mf[two[lg1]] = L[b[lg1]], b[lg1]
    return lic, mf, nl


def resident(args, stream):
    import numpy as np
    import bench
    from licensee_amd._native import Scorer
    from licensee_amd.synth import SyntheticCorpus
    c = bench.build_workload(2)
    n = args.files
    fb = SyntheticCorpus(c).generate(0, n, seed=20250202, nthreads=16)
    sc = Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, n_vocab=c.n_vocab, device=0)
    T = sc.n_templates
    sc.exact_setup(c.lf_size, np.zeros_like(c.lf_bits), np.zeros(T, np.uint64))
    rng = np.random.default_rng(20250202)
    sizes = rng.choice(np.arange(1, 6), n, p=[0.30, 0.25, 0.20, 0.15, 0.10])   # mean 2.5: ~0.4 projects per file
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    offsets = offsets[:np.searchsorted(offsets, n, 'right')]
    if offsets[-1] != n:
        offsets = np.append(offsets, n)
    offsets = offsets.astype(np.int64)
    P = len(offsets) - 1
    flags = (rng.random(n) < 0.02).astype(np.uint8) | (2 * (rng.random(n) < 0.05)).astype(np.uint8) | \
        (4 * (rng.random(n) < 0.05)).astype(np.uint8)
    keys = [t.key for t in c.templates]
    tflags = np.array([(1 if k in ('gpl-2.0', 'gpl-3.0') else 0) | (2 if k in ('lgpl-2.1', 'lgpl-3.0') else 0) for k in keys],
                      np.uint8)
    s = stream.cuda_stream
    b = sc.batch(n)
    b.upload(fb, s)
    b.exact(None, s)
    b.match(98.0, s, confidence=True)
    k = 4

    def device():
        b.projects(offsets, flags, tflags, use_exact=True, k=k, stream=s)
        device.out = b.download_projects(s)

    def host():
        exact = b.download_exact(s)
        best = b.download_match(s)[0]
        t0 = time.perf_counter()
        host.out = numpy_resolve(offsets, flags, tflags, exact, best, T)
        return (time.perf_counter() - t0) * 1e6

    def downloads():
        b.download_exact(s)
        b.download_match(s)

    device(), host()
    for x, y, name in zip(device.out[:3], host.out, ('license', 'matched_file', 'n_licenses')):
        assert np.array_equal(x, y), name
    dv, ho, dl = timed(device, stream, args.launches), timed(host, stream, args.launches), timed(downloads, stream, args.launches)
    kern = timed(lambda: b.projects(offsets, flags, tflags, use_exact=True, k=k, stream=s), stream, args.launches)
    print(json.dumps({'part': 'resident', 'files': n, 'projects': P, 'templates': T, 'k_licenses': k,
                      'device_resolve_and_download_us': {'median': round(med(dv), 1), 'min': round(min(dv), 1), 'max': round(max(dv), 1)},
                      'device_resolve_alone_us': {'median': round(med(kern), 1), 'min': round(min(kern), 1), 'max': round(max(kern), 1)},
                      'host_download_and_numpy_us': {'median': round(med(ho), 1), 'min': round(min(ho), 1), 'max': round(max(ho), 1)},
                      'host_download_alone_us': {'median': round(med(dl), 1), 'min': round(min(dl), 1), 'max': round(max(dl), 1)},
                      'bytes_back': {'device': P * (12 + 4 * k), 'host': n * 20}, 'launches': args.launches}), flush=True)
    b.close()
    sc.close()


def streams(args):
    import bench
    from licensee_amd.batch import BatchDetector
    from licensee_amd.dice import DiceEngine
    from licensee_amd.synth import SyntheticCorpus
    c = bench.build_workload(2)
    synth = SyntheticCorpus(c)
    big = [synth.text(i)[0].encode('utf-8') for i in range(16000)]
    chunks = [big[i:i + 4000] for i in range(0, len(big), 4000)] * 2
    file_batches = [(ch, ['LICENSE'] * len(ch)) for ch in chunks]
    proj_batches = [[[('LICENSE', t) for t in ch[i:i + 3]] for i in range(0, len(ch), 3)] for ch in chunks]
    det = BatchDetector(DiceEngine(device=0), nthreads=16)

    def by_files():
        out = 0
        for dets in det.detect_stream(file_batches):
            # the host's own project.rb over Detection objects: distinct licenses per group of three
            for i in range(0, len(dets), 3):
                keys = {d.license.key for d in dets[i:i + 3] if d.matcher != 'copyright'}
                out += len(keys) == 1
        return out

    def by_projects():
        return sum(sum(1 for d in ds if d.license is not None and d.license.key != 'other')
                   for ds in det.detect_projects_stream(proj_batches))

    by_files(), by_projects()      # both page-locked buffers and the project buffers allocated
    n = sum(len(ch) for ch in chunks)
    rates = {'detect_stream_plus_host_grouping': [], 'detect_projects_stream': []}
    for _ in range(args.streams):
        for name, fn in (('detect_stream_plus_host_grouping', by_files), ('detect_projects_stream', by_projects)):
            t0 = time.perf_counter()
            fn()
            rates[name].append(round(n / (time.perf_counter() - t0)))
    print(json.dumps({'part': 'streams', 'files': n, 'batches': len(chunks), 'files_per_project': 3,
                      'files_per_s': rates, 'median': {k: med(v) for k, v in rates.items()}}), flush=True)
    det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=1_000_000)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--streams', type=int, default=3)
    ap.add_argument('--no-stream', action='store_true')
    ap.add_argument('--no-resident', action='store_true')
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    if not args.no_resident:
        resident(args, stream)
    if not args.no_stream:
        streams(args)


if __name__ == '__main__':
    main()
