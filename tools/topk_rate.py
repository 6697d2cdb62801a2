"""What the top-k-only call costs against the matrix call (dice_batch_topk vs dice_batch_matrix).

    python tools/topk_rate.py [--shapes 2,3] [--k 3] [--runs 3] [--launches 20] [--stage-ab 6]
                              [--files N] [--create]

Per shape -- config 2 (1,000,000 files x the 47 vendored templates, sparse program) and config 3
(1,250,000 files x 600 templates through the postings kernels) -- the files are made resident once;
then dice_batch_matrix(k) and dice_batch_topk(k) alternate, `--runs` runs each, a run being the median
of `--launches` launches timed by HIP events around the call alone. One JSON line per shape with both
series (microseconds), matrix_bytes() and the device memory the batch holds before and after the
matrix call first allocates its N x T buffers, and the algorithmic bytes per file of both calls.

--stage-ab R (config 2 only): the top-k call under DICE_PROG_MATCH=valu against the default (the
matrix-core accumulate stage where the cost rule picks it), R runs each, alternating -- the A/B that
decides whether dice_prog_topk4_mfma stays.
--create: time dice_create of the config-2 corpus on a warm code-object cache (the module holds more
kernels than before), median of 5.
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


def timed_run(fn, stream, launches):
    """Median over `launches` launches of fn(), each between two HIP events, in microseconds."""
    import torch
    us = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return round(med(us), 1)


def used_bytes():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def scorer_for(c, env=None):
    from licensee_amd._native import Scorer
    saved = {k: os.environ.get(k) for k in (env or {})}
    for k, v in (env or {}).items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, n_vocab=c.n_vocab,
                      device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def workload(cfg, n):
    import bench
    from licensee_amd.synth import SyntheticCorpus
    c = bench.build_workload(cfg)
    return c, SyntheticCorpus(c).generate(0, n, seed=20250202, nthreads=16)


def shape(cfg, n, args, stream):
    import numpy as np
    c, fb = workload(cfg, n)
    base = used_bytes()
    sc = scorer_for(c)
    T, V, kind, _ = sc.info()
    b = sc.batch(n)
    b.upload(fb, stream.cuda_stream)
    b.topk(args.k, stream.cuda_stream)
    tk = b.download_topk(args.k, stream.cuda_stream)
    out = {'config': cfg, 'files': n, 'templates': T, 'kernel_kind': kind, 'k': args.k, 'program_stage': sc.program_stage(),
           'matrix_bytes_after_topk': b.matrix_bytes(), 'device_bytes_after_topk': used_bytes() - base}
    b.matrix(args.k, stream.cuda_stream)
    mk = b.download_matrix(args.k, stream.cuda_stream)[2:]
    assert np.array_equal(tk[0], mk[0]) and np.array_equal(tk[1], mk[1])
    out['matrix_bytes_after_matrix'] = b.matrix_bytes()
    out['device_bytes_after_matrix'] = used_bytes() - base
    in_bytes = b.bytes_per_file() if kind != 3 else 8 * ((V + 63) // 64)
    out['algo_bytes_per_file'] = {'topk': in_bytes + 9 + 12 * args.k, 'matrix': in_bytes + 9 + 12 * T + 12 * args.k}
    series = {'matrix': [], 'topk': []}
    for _ in range(args.runs):
        series['matrix'].append(timed_run(lambda: b.matrix(args.k, stream.cuda_stream), stream, args.launches))
        series['topk'].append(timed_run(lambda: b.topk(args.k, stream.cuda_stream), stream, args.launches))
    out['matrix_us'], out['topk_us'] = series['matrix'], series['topk']
    for kk in (1, 16):
        if kk != args.k:
            out[f'topk_us_k{kk}'] = timed_run(lambda: b.topk(kk, stream.cuda_stream), stream, args.launches)
            out[f'matrix_us_k{kk}'] = timed_run(lambda: b.matrix(kk, stream.cuda_stream), stream, args.launches)
    print(json.dumps(out), flush=True)
    b.close()
    if cfg == 2 and args.stage_ab:
        legs = {'valu': scorer_for(c, {'DICE_PROG_MATCH': 'valu'}), 'default': sc}
        bs = {}
        for name, s in legs.items():
            bs[name] = s.batch(n)
            bs[name].upload(fb, stream.cuda_stream)
            bs[name].topk(args.k, stream.cuda_stream)
        ref = bs['valu'].download_topk(args.k, stream.cuda_stream)
        got = bs['default'].download_topk(args.k, stream.cuda_stream)
        assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
        ab = {'stage_ab': True, 'files': n, 'k': args.k, 'stage': {m: s.program_stage() for m, s in legs.items()},
              'valu_us': [], 'default_us': []}
        for _ in range(args.stage_ab):
            for name in ('valu', 'default'):
                ab[name + '_us'].append(timed_run(lambda: bs[name].topk(args.k, stream.cuda_stream), stream, args.launches))
        print(json.dumps(ab), flush=True)
        for x in bs.values():
            x.close()
        legs['valu'].close()
    sc.close()


def create_time():
    import bench
    c = bench.build_workload(2)
    scorer_for(c).close()      # the cache is warm from here on
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        s = scorer_for(c)
        ms.append((time.perf_counter() - t0) * 1e3)
        s.close()
    print(json.dumps({'dice_create_warm_ms': round(med(ms), 2), 'runs': [round(x, 2) for x in ms]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='2,3')
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--stage-ab', type=int, default=0)
    ap.add_argument('--files', type=int, default=0)
    ap.add_argument('--create', action='store_true')
    args = ap.parse_args()
    import torch
    import bench
    stream = torch.cuda.Stream()
    if args.create:
        create_time()
    for cfg in [int(x) for x in args.shapes.split(',') if x]:
        os.environ['DICE_POST_PRUNE'] = '0'    # irrelevant to both calls; kept fixed
        shape(cfg, args.files or bench.DEFAULT_FILES[cfg], args, stream)


if __name__ == '__main__':
    main()
