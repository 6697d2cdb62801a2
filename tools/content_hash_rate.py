"""What ContentHelper#content_hash costs on the device (dice_batch_content_hash, csrc/dice_hash.hip).

    python tools/content_hash_rate.py [--streams 3] [--launches 20] [--threads 16] [--stream-off-only]

On bench.py's 16,000 synthetic config-2 texts, one JSON line with
  - the SHA-1 kernel's time by HIP events around dice_batch_content_hash alone, for 4,000 and 16,000
    resident texts (median and range of `--launches` launches), and the share of files it flags;
  - the BatchDetector.detect_stream rate (8 x 4,000 texts, bench.py's end-to-end leg) with
    content_hash False and True, alternating, `--streams` streams each: medians and ranges;
  - the host alternative on the same normalized texts: hashlib.sha1 per file on `--threads` threads.
--stream-off-only measures only the content_hash=False stream (it uses nothing the feature added,
so the same file runs in a checkout of an earlier commit for an A/B of the hashes-off path).
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    s = sorted(v)
    return s[len(s) // 2]


def stream_rate(det, chunks):
    t0 = time.perf_counter()
    n = sum(len(d) for d in det.detect_stream(chunks))
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--stream-off-only', action='store_true')
    args = ap.parse_args()
    import numpy as np
    import torch
    from licensee_amd.batch import BatchDetector
    from licensee_amd.dice import DiceEngine
    from licensee_amd.native_host import HostPrep
    from licensee_amd.synth import SyntheticCorpus
    eng = DiceEngine(device=0)
    corpus = eng.corpus
    syn = SyntheticCorpus(corpus)
    big = [syn.text(i)[0].encode('utf-8') for i in range(16000)]
    chunks = [(big[i:i + 4000], None) for i in range(0, len(big), 4000)] * 2
    out = {'n_texts': len(big), 'avg_raw_bytes': round(sum(map(len, big)) / len(big), 1)}

    modes = (False,) if args.stream_off_only else (False, True)
    dets = {m: (BatchDetector(eng, nthreads=args.threads, content_hash=True) if m else
                BatchDetector(eng, nthreads=args.threads)) for m in modes}
    for det in dets.values():
        for _ in det.detect_stream(chunks[:2]):   # both page-locked text buffers allocated
            pass
    rates = {m: [] for m in modes}
    for _ in range(args.streams):
        for m in modes:
            rates[m].append(stream_rate(dets[m], chunks))
    for m in modes:
        key = 'stream_hash_on' if m else 'stream_hash_off'
        out[key + '_files_per_s'] = round(med(rates[m]))
        out[key + '_runs'] = [round(r) for r in rates[m]]
    if not args.stream_off_only:
        # the two stages alone per 4,000-file batch, with and without the hash
        for m in modes:
            det = dets[m]
            t0 = time.perf_counter()
            prepped = [det._prep(*c) for c in chunks[:4]]
            t1 = time.perf_counter()
            for p in prepped:
                det._score(p, 98.0)
            out[('stage_ms_hash_on' if m else 'stage_ms_hash_off')] = {
                'host': round((t1 - t0) / 4 * 1e3, 3), 'device': round((time.perf_counter() - t1) / 4 * 1e3, 3)}
        # the hash's share of the device stage, one 4,000-file batch with nothing else running: the
        # digest download + hex, and with it the host completion of the flagged files
        det = dets[True]
        contents = chunks[0][0]
        det.detect(contents)
        t0 = time.perf_counter()
        digest, status = det._batch.download_content_hash()
        hx = digest.tobytes().hex()
        _ = [hx[i:i + 40] for i in range(0, len(hx), 40)]
        t1 = time.perf_counter()
        det._hashes(det._batch, contents, None)
        t2 = time.perf_counter()
        out['hash_download_hex_ms_per_batch'] = round((t1 - t0) * 1e3, 3)
        out['hash_host_completion_ms_per_batch'] = round((t2 - t1 - (t1 - t0)) * 1e3, 3)
        out['hash_host_completion_files_per_batch'] = int(status.sum())
    for det in dets.values():
        det.close()
    if args.stream_off_only:
        print(json.dumps(out))
        return

    hp = HostPrep(corpus)
    norm = text, off, tl, ln, cc = hp.normalize_files(big, None, nthreads=args.threads)[:5]
    out['avg_normalized_bytes'] = round(float(tl.mean()), 1)
    out['max_normalized_bytes'] = int(tl.max())
    stream = torch.cuda.Stream()
    for n in (4000, 16000):
        b = eng.scorer.batch(n)
        if n < len(big):    # (the threads of normalize_files each fill a region of their own: no prefix)
            text, off, tl, ln, cc, _, _ = hp.normalize_files(big[:n], None, nthreads=args.threads)
        else:
            text, off, tl, ln, cc = norm
        b.upload_text(text, off, tl, ln, cc, stream.cuda_stream)
        b.content_hash(stream.cuda_stream)
        digest, status = b.download_content_hash(stream.cuda_stream)
        want = hashlib.sha1(text[int(off[0]):int(off[0]) + int(tl[0])].tobytes()).digest()
        assert digest[0].tobytes() == want
        ms = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            b.content_hash(stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[f'kernel_ms_{n}'] = {'median': round(med(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}
        out[f'flagged_share_{n}'] = round(float(status.mean()), 5)
        b.close()

    # the tail one long file leaves: the first 4,000 texts and one 200 KB text (SHA-1 cannot be
    # split, so its chain bounds the kernel from below)
    n = 4000
    text, off, tl, ln, cc, _, _ = hp.normalize_files(big[:n], None, nthreads=args.threads)
    end = (len(text) + 15) // 16 * 16
    long_len = 200 * 1024
    long_text = np.resize(text[int(off[0]):int(off[0]) + int(tl[0])], long_len)
    text2 = np.concatenate([text, np.zeros(end - len(text), np.uint8), long_text])
    b = eng.scorer.batch(n + 1)
    b.upload_text(text2, np.append(off[:n], end), np.append(tl[:n], long_len), np.append(ln[:n], long_len),
                  np.append(cc[:n], 0), stream.cuda_stream)
    b.content_hash(stream.cuda_stream)
    digest, _ = b.download_content_hash(stream.cuda_stream)
    assert digest[n].tobytes() == hashlib.sha1(long_text.tobytes()).digest()
    ms = []
    for _ in range(args.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        b.content_hash(stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out['kernel_ms_4000_plus_one_200KB'] = {'median': round(med(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}
    b.close()

    # the host alternative: hashlib.sha1 per normalized text (it releases the GIL above 2 KiB)
    from concurrent.futures import ThreadPoolExecutor
    text, off, tl, ln, cc = norm
    views = [text[int(o):int(o) + int(l)] for o, l in zip(off.tolist(), tl.tolist())]

    def part(k):
        return [hashlib.sha1(v).digest() for v in views[k::args.threads]]
    with ThreadPoolExecutor(args.threads) as ex:
        list(ex.map(part, range(args.threads)))
        reps = []
        for _ in range(3):
            t0 = time.perf_counter()
            list(ex.map(part, range(args.threads)))
            reps.append(len(views) / (time.perf_counter() - t0))
    out['host_sha1_texts_per_s'] = round(med(reps))
    out['host_sha1_threads'] = args.threads
    t0 = time.perf_counter()
    for v in views[:2000]:
        hashlib.sha1(v).digest()
    out['host_sha1_us_per_text_1_thread'] = round((time.perf_counter() - t0) / 2000 * 1e6, 2)
    print(json.dumps(out))
    eng.scorer.close()


if __name__ == '__main__':
    main()
