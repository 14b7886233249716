"""Every tile instance of the weight gradient (csrc/conv_wgrad.hip WGRAD_INSTANCES), through the single and through the grouped wrapper, once:
(a) the plan names the intended instance, (b) the gradient matches an fp64 contraction of the same operands -- plain bf16:
close(., ., 5e-3, 5e-3 * max|ref|) as in test_gpu_kernels.py; x3: relative max error < 1e-4 as in test_gpu_sparse_backward.py --, (c) the slab
bytes hash to the digest recorded from the parent commit's library (tests/wgrad_instances_util.py): same instance, same grid, same splits,
same parameters.  The atomic form is checked by (a) and (b).  The three instances no default plan reaches run in fresh child processes with
their once-per-process switch set."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from tests import wgrad_instances_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planned_instance(name):
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd import functional as AF
    prev = AF.get_precision()
    AF.set_precision(U.CASES[name][0])
    try:
        descs, flags = U.descs(name)
    finally:
        AF.set_precision(prev)
    n, pl = len(descs), _C.WgradPlan()
    rc = _C.lib.aod_conv2d_wgrad_plan_ex((C.c_void_p * n)(*[C.addressof(d) for d in descs]), n, flags, C.byref(pl))
    assert rc == 0, (name, rc, _C.lib.aod_last_error())
    return (pl.wide, pl.waves, pl.tile, pl.x3, pl.sparse), pl.grouped


def check(name):
    mode, n, cin, cout, rows, maps, atomic, inst, switch = U.CASES[name]
    assert rows % 64 == U.TAIL or not maps or inst == U.X8B
    assert planned_instance(name) == (inst, int(n > 1)), name
    grads, refs, digest = U.run(name)
    for g, r in zip(grads, refs):
        scale = float(r.abs().max())
        err = float((g.double() - r).abs().max()) / scale
        print(f'{name}: relative max error {err:.3e}')
        if mode == 'bf16':
            assert torch.allclose(g.float().cpu(), r.float().cpu(), rtol=5e-3, atol=5e-3 * scale), (name, err)
        else:
            assert 0 < err < 1e-4, (name, err)
    if atomic:
        assert digest is None
    else:
        assert name in U.DIGESTS, f'{name}: no recorded digest'
        assert digest == U.DIGESTS[name], f'{name}: the slabs differ from those of commit {U.PARENT}'


def check_switch(switch):
    """the cases of one once-per-process switch (child processes)"""
    names = [k for k, c in U.CASES.items() if c[8] == switch]
    for name in names:
        check(name)
    return len(names)


@pytest.mark.parametrize('name', [k for k, c in U.CASES.items() if c[8] is None])
def test_instance(name):
    if any(k.startswith('AOD_WGRAD_') for k in os.environ):
        pytest.fail('an AOD_WGRAD_* switch is set in the environment: the default plans are not what this test launches')
    check(name)


@pytest.mark.parametrize('switch', sorted({c[8] for c in U.CASES.values() if c[8]}))
def test_instances_behind_a_switch(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith('AOD_WGRAD_')}
    env[switch] = '0'
    code = f'import tests.test_gpu_wgrad_instances as t; print("cases", t.check_switch({switch!r}))'
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    n = sum(c[8] == switch for c in U.CASES.values())
    assert r.returncode == 0 and f'cases {n}' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
