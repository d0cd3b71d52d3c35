"""bench.py's plain run and --dump-outputs: the result line of a plain run, and the seeded sample of the block the last timed
step assembled, which must be what getDense() hands a caller for the same problem."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    import torch
    import bench
    N = 1000
    # A[i, j] = i N + j: every sampled value tells where it came from
    A = torch.arange(N*N, dtype=torch.float64).reshape(N, N)
    bench.dump_outputs(str(tmp_path/'a'), A)
    bench.dump_outputs(str(tmp_path/'b'), A.clone())
    names = sorted(os.listdir(tmp_path/'a'))
    assert names == ['A_diagonal.npy', 'A_entries.npy', 'A_rows.npy']
    total = 0
    for name in names:
        a, b = np.load(tmp_path/'a'/name), np.load(tmp_path/'b'/name)
        assert a.dtype == np.float64 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path/'a'/'A_diagonal.npy'), np.arange(N)*(N+1.))
    rows = np.load(tmp_path/'a'/'A_rows.npy')
    assert rows.shape[1] == N and np.array_equal(rows, (rows[:, :1]//N)*N+np.arange(N))
    assert len(np.unique(rows[:, 0])) == rows.shape[0]
    entries = np.load(tmp_path/'a'/'A_entries.npy')
    assert entries.size == 1 << 20 and entries.min() >= 0 and entries.max() < N*N


def test_dump_outputs_needs_one_gpu(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--dump-outputs', 'out'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


@pytest.mark.gpu
def test_plain_run_dumps_what_getDense_returns(tmp_path):
    """a plain run at noRef 3: the result line, no --full figures, and the dumped sample equal to the same sample of
    getDense()'s matrix (the bench's workload: disc, P1, s = 0.5, target_order 0.5, zeroExterior)"""
    import torch
    import bench
    from pynucleus_amd import disc, P1_DoFMap, PHYSICAL, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--noRef', '3',
                        '--dump-outputs', str(tmp_path/'bench')], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['unit'] == 'element-pairs/s' and line['dtype'] == 'f64'
    assert line['higher_is_better'] is True and line['value'] > 0 and line['ms_per_step'] > 0
    assert not {'roofline', 'operator', 'cpu_baseline', 'configs'} & set(line)
    dm = P1_DoFMap(disc(3), PHYSICAL)
    A = nonlocalBuilder(dm, getFractionalKernel(2, 0.5), {'target_order': 0.5}, zeroExterior=True).getDense().toarray()
    bench.dump_outputs(str(tmp_path/'ref'), torch.from_numpy(np.ascontiguousarray(A)))
    scale = np.abs(A).max()
    for name in ('A_diagonal', 'A_rows', 'A_entries'):
        got, ref = np.load(tmp_path/'bench'/(name+'.npy')), np.load(tmp_path/'ref'/(name+'.npy'))
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert np.abs(got-ref).max() <= 1e-12*scale, name
