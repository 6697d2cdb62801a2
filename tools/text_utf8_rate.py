"""What counting content_normalized.length on the device costs (dice_text_chars_kernel, csrc/dice_words.hip).

    python tools/text_utf8_rate.py [--launches 30] [--threads 16]

dice_batch_upload_text_utf8 with ``length == NULL`` has the device count each file's characters from
its resident UTF-8 bytes instead of copying the caller's lengths. On bench.py's synthetic config-2
texts (4,000 and 16,000 of them, normalized by lh_normalize_files_utf8 into page-locked memory), one
JSON line with the time of the whole upload call by HIP events around it, with the host's lengths
and with ``length=None``, alternating: medians, ranges, and the median of the paired differences --
the kernel's cost net of the [n] int32 copy it replaces. Beside it the expectation from bytes over
bandwidth: the kernel reads every text byte once, at the 6.3 TB/s this part streams from HBM (an
upper bound on its time: the bytes were just written by the H2D copy and read by the scan, so part
of them is still in the Infinity Cache), plus one dependent-launch boundary of about 1.5 us.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
BOUNDARY_US = 1.5


def med(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--threads', type=int, default=16)
    args = ap.parse_args()
    import numpy as np
    import torch
    from licensee_amd._native import PinnedBuffer
    from licensee_amd.dice import DiceEngine
    from licensee_amd.native_host import HostPrep
    from licensee_amd.synth import SyntheticCorpus
    eng = DiceEngine(device=0)
    hp = HostPrep(eng.corpus)
    eng.scorer.vocab_setup(eng.corpus.vocab, hp.nv_fields)
    syn = SyntheticCorpus(eng.corpus)
    big = [syn.text(i)[0].encode('utf-8') for i in range(16000)]
    stream = torch.cuda.Stream()
    out = {}
    for n in (4000, 16000):
        pins = []

        def pinned(nbytes):
            pins.append(PinnedBuffer(nbytes))
            return pins[-1].array
        text, off, tl, ln, cc, _, _ = hp.normalize_files(big[:n], None, nthreads=args.threads, out=pinned, utf8=True)
        b = eng.scorer.batch(n)
        b.upload_text(text, off, tl, None, cc, stream.cuda_stream, utf8=True)
        assert np.array_equal(b.download_length(stream.cuda_stream), ln)
        ms = {True: [], False: []}
        for _ in range(args.launches):
            for host_len in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                b.upload_text(text, off, tl, ln if host_len else None, cc, stream.cuda_stream, utf8=True)
                e1.record(stream)
                e1.synchronize()
                ms[host_len].append(e0.elapsed_time(e1))
        diff = [d - h for h, d in zip(ms[True], ms[False])]
        nbytes = int(tl.sum())
        out[f'n_{n}'] = {
            'text_bytes': nbytes, 'non_ascii_share': round(float((tl > ln).mean()), 4),
            'upload_ms_host_length': {'median': round(med(ms[True]), 4), 'min': round(min(ms[True]), 4),
                                      'max': round(max(ms[True]), 4)},
            'upload_ms_device_length': {'median': round(med(ms[False]), 4), 'min': round(min(ms[False]), 4),
                                        'max': round(max(ms[False]), 4)},
            'paired_difference_us': {'median': round(med(diff) * 1e3, 2), 'min': round(min(diff) * 1e3, 2),
                                     'max': round(max(diff) * 1e3, 2)},
            'expected_kernel_us': round(nbytes / HBM_BYTES_PER_S * 1e6 + BOUNDARY_US, 2),
        }
        b.close()
        for p in pins:
            p.close()
    print(json.dumps(out))
    eng.scorer.close()


if __name__ == '__main__':
    main()
