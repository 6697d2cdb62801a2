"""bench.py --gpus N starts its own ranks: with no RANK in the environment
the parent makes no GPU call, runs a child torch.distributed.run on 127.0.0.1 and relays rank 0's
JSON line. CPU: the launcher with a stub rank script (gloo, world size 2). GPU: the real bench at
--gpus 2 on the one-GPU box (both ranks on device 0, gloo coordination): n_gpus 2, a cpu_baseline
and zero parity mismatches summed over both ranks' shards."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = '''
import json, os, sys
import torch.distributed as dist
dist.init_process_group('gloo')
import torch
t = torch.tensor([float(dist.get_rank() + 1)])
dist.all_reduce(t)
if dist.get_rank() == 0:
    print('banner line a native library might print')
    print(json.dumps({'world': dist.get_world_size(), 'sum': float(t[0]), 'argv': sys.argv[1:]}))
dist.destroy_process_group()
'''


def test_self_launch_relays_rank0_line(tmp_path):
    stub = tmp_path / 'rank.py'
    stub.write_text(STUB)
    code = ('import sys; sys.path.insert(0, %r); import bench; '
            'sys.exit(bench.self_launch(2, ["--steps", "3"], script=%r))' % (ROOT, str(stub)))
    p = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out == {'world': 2, 'sum': 3.0, 'argv': ['--steps', '3']}


def test_external_launch_must_match_gpus():
    env = dict(os.environ, RANK='0', WORLD_SIZE='2', LOCAL_RANK='0', MASTER_PORT='1', MASTER_ADDR='127.0.0.1')
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '4'], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=env)
    assert p.returncode != 0 and 'WORLD_SIZE=2 but --gpus 4' in p.stderr


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu():
    cmd = [sys.executable, 'bench.py', '--full', '--gpus', '2', '--steps', '3', '--warmup', '1',
           '--files-per-gpu', '40000', '--extra-configs', '3,5', '--extra-files-per-gpu', '20000', '--no-extras',
           '--cpu-seconds', '1']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line['n_gpus'] == 2 and line['config']['global_files'] == 80000
    assert line['extras']['process_group']['world_size'] == 2
    assert line['cpu_baseline'] and line['cpu_baseline']['value'] > 0
    assert line['parity']['mismatches'] == 0 and line['parity']['ranks_checked'] == 2
    # the host gather: both ranks' results in rank 0's shared host buffer, checked
    ex = line['extras']
    assert ex['host_gather_mismatches'] == 0 and ex['host_gather_checked'] is True, ex
    assert ex['gather_winner'] == 'host' and 'no RCCL' in ex['gather_note'] and ex['host_gather_ms'] > 0
    for tag in ('3', '3-top1', '3-allpairs', '5'):
        rec = line['extras']['configs'][tag]
        assert rec['global_files'] == 40000 and rec['parity']['mismatches'] == 0, (tag, rec)
        assert rec['cpu_baseline']['value'] > 0


@pytest.mark.gpu
def test_bench_abi_sharded_leg_three_contexts():
    """--shard-mode abi: dice_match_sharded_confidence over 3 contexts (all on device 0 of the test
    box), host and device gathers timed, results equal to the resident batch's."""
    cmd = [sys.executable, 'bench.py', '--full', '--steps', '3', '--warmup', '1', '--files-per-gpu', '50000',
           '--extra-configs=', '--no-extras', '--no-cpu-baseline', '--shard-mode', 'abi', '--abi-contexts', '3']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])['extras']['abi_sharded']
    assert rec['contexts'] == 3 and rec['devices'] == [0, 0, 0] and rec['files'] == 50000
    for mode in ('host', 'device'):
        assert rec[mode]['mismatches'] == 0 and rec[mode]['files_per_s'] > 0, rec
    # one device: no peer path exercised, and no gather winner claimed from same-device timings
    assert rec['host']['dice_last_gather_peer'] == -1 and rec['device']['dice_last_gather_peer'] == -1
    assert rec['winner'] is None and 'distinct device' in rec['winner_reason']


def test_dump_outputs_samples_the_same_files_of_every_array(tmp_path, monkeypatch):
    """--dump-outputs: float64 arrays, whole while they fit the byte limit; beyond it the same seeded
    sample of the files for every array (sample_rows.npy), the same from call to call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    n = 1000
    arrs = {'best': np.arange(n, dtype=np.int32) - 1, 'score_matrix': np.arange(n * 3, dtype=np.float64).reshape(n, 3)}
    load = lambda d: {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    bench.dump_outputs(str(tmp_path / 'whole'), arrs)
    whole = load(tmp_path / 'whole')
    assert sorted(whole) == ['best', 'score_matrix']
    for k, a in whole.items():
        assert a.dtype == np.float64 and np.array_equal(a, arrs[k])
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 4096)
    bench.dump_outputs(str(tmp_path / 'a'), arrs)
    bench.dump_outputs(str(tmp_path / 'b'), arrs)
    a, b = load(tmp_path / 'a'), load(tmp_path / 'b')
    assert sorted(a) == ['best', 'sample_rows', 'score_matrix']
    rows = a['sample_rows'].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert sum(x.nbytes for x in a.values()) <= 4096
    for k in arrs:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], arrs[k][rows]), k
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_plain_run_refuses_a_leg_behind_full():
    p = subprocess.run([sys.executable, 'bench.py', '--shard-mode', 'abi'], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode != 0 and '--full' in p.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline figure alone (no cpu_baseline, parity or extras),
    --steps is the number of timed steps behind ms_per_step, and --dump-outputs writes the timed
    batch's results: equal to one dice_match call over the same files."""
    import numpy as np
    n = 30000
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--files-per-gpu', str(n),
           '--dump-outputs', str(tmp_path / 'out')]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['n_gpus'] == 1
    assert line['cpu_baseline'] is None and line['parity'] is None and line['extras'] == {}
    assert line['unit'] == 'files/s' and line['higher_is_better'] is True and line['dtype'] == 'u32'
    assert line['ms_per_step'] > 0
    assert abs(line['value'] - n / (line['ms_per_step'] * 1e-3)) <= 1e-9 * line['value']
    got = {k: np.load(tmp_path / 'out' / f'{k}.npy') for k in ('best', 'overlap', 'score')}
    assert sorted(os.listdir(tmp_path / 'out')) == ['best.npy', 'overlap.npy', 'score.npy']
    sys.path.insert(0, ROOT)
    import bench
    from licensee_amd._native import Scorer
    from licensee_amd.synth import SyntheticCorpus
    c = bench.build_workload(2)
    fb = SyntheticCorpus(c).generate(0, n, seed=20250202, nthreads=16)
    sc = Scorer(c.lf_bits, c.lf_size, c.fields_set_size, c.length_slack, c.length, c.is_cc, n_vocab=c.n_vocab)
    try:
        exp = dict(zip(('best', 'overlap', 'score'), sc.match(fb, 98.0)))
    finally:
        sc.close()
    assert (exp['best'] >= 0).any() and (exp['best'] < 0).any()
    for k, a in got.items():
        assert a.dtype == np.float64 and a.shape == (n,) and np.array_equal(a, exp[k]), k


def test_config3_traffic_file_per_entry_point():
    """Config 3's roofline.traffic comes from the PMC file of the entry point measured: '3' through
    dice_batch_match_confidence (pmc_config3.json), '3-top1' through dice_batch_match
    (pmc_config3_top1.json), '3-allpairs' on the postings kernels (pmc_config3_post.json)."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    from types import SimpleNamespace as R
    assert bench.traffic_variant(3, R(match_kernel=4, confidence=True)) == ''
    assert bench.traffic_variant(3, R(match_kernel=4, confidence=False)) == '_top1'
    assert bench.traffic_variant(3, R(match_kernel=3, confidence=False)) == '_post'
    assert bench.traffic_variant(2, R(match_kernel=1, confidence=False)) == ''
    for name in ('pmc_config3.json', 'pmc_config3_top1.json', 'pmc_config3_post.json'):
        assert os.path.exists(os.path.join(ROOT, 'profiles', name)), name
