"""GPU: a plain bench run (no --full) times exactly --steps steps, leaves the --full fields null and, with --dump-outputs, writes what
its last timed step computed.  In the deterministic mode two runs with the same arguments write the same bits: same inputs, same weights."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '2', '--size', '128',
           '--deterministic', '--dump-outputs', str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith('{"metric"')][-1])
    return line, {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(str(out), '*.npy')))}


def test_plain_run_dumps_the_last_step_and_repeats(tmp_path):
    line, a = _run(tmp_path / 'a')
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'images/sec' and line['higher_is_better'] is True and line['dtype'] == 'bf16x3'
    assert line['roofline'] is None and line['phase_rates'] is None and line['cpu_baseline'] is None and line['hua'] is None
    assert line['precision']['other_mode'] is None
    for k in ('train_loss', 'train_loss_cls', 'train_loss_bbox', 'train_loss_noR', 'train_loss_L', 'train_params', 'score_dets',
              'score_labels', 'score_unc'):
        assert k in a, (k, sorted(a))
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a['score_dets'].shape == (2, 100, 5) and a['score_labels'].shape == (2, 100) and a['score_unc'].shape == (2,)
    assert a['train_loss'] > 0 and a['train_params'].size > 0
    _, b = _run(tmp_path / 'b')
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
