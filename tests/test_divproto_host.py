"""CPU tests (no GPU) of the ENMS + DivProto acquisition: the float64 restatements of tests/divproto_util.py on hand-computed
cases, the host half (scoring.divproto_order, scoring.divproto_quotas), every refusal of the Python and C entry points, the driver's parser
and the exported names."""
import ctypes
import importlib.util
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import divproto_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _detector(config='configs/_base_/Config_RetinaNet.py'):
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    return cfg, build_detector(cfg.model)


class _Loader:
    batch_size = 2
    dataset = [0] * 4
    collate_fn = None


# ---------------------------------------------------------------------------------------------------------------- the restatements by hand
def test_enms_restatement_on_the_hand_case():
    c = U.hand_enms_case()
    E, kept, picks, amb = U.enms_float64(c['feat'], c['cls'], c['h'], c['cnt'])
    assert picks == c['picks'] == [1, 2, 3] and kept == 3 and amb == []          # the bit-equal tie of objects 1 and 2 is no ambiguity
    assert E == c['E'] and abs(E - 1.6) < 1e-7
    # t_enms = 1: nothing is suppressed (0.9 and 1 are not above 1) -> every object is picked, by h descending, ties by index
    E1, kept1, picks1, _ = U.enms_float64(c['feat'], c['cls'], c['h'], c['cnt'], t_enms=1.0)
    assert picks1 == [1, 2, 0, 3] and kept1 == 4 and abs(E1 - 2.1) < 1e-7
    # objects 0 and 2 share their feature but not their class; once all four share one class, the first pick (1) suppresses both
    E2, kept2, picks2, _ = U.enms_float64(c['feat'], np.zeros(4, np.int32), c['h'], c['cnt'])
    assert picks2 == [1, 3] and kept2 == 2 and abs(E2 - 0.9) < 1e-7
    assert U.enms_float64(c['feat'], c['cls'], c['h'], 0) == (0.0, 0, [], [])    # no object: E = 0, kept = 0
    # ambiguity: two measures closer than 1e-6 relative that are not bit-equal; a product within 1e-5 of the threshold
    h = c['h'].copy()
    h[2] = np.nextafter(h[1], np.float32(1))
    assert [a[0] for a in U.enms_float64(c['feat'], c['cls'], h, 4)[3]] == ['h']
    assert [a[0] for a in U.enms_float64(c['feat'], c['cls'], c['h'], 4, t_enms=0.9)[3]] == ['dot']


def test_prototype_restatement_on_two_objects():
    K, C = 3, 8
    e = np.eye(C, dtype=np.float32)
    feat = np.stack([e[0], e[2], e[1]])
    cls = np.array([5, 2, 5], np.int32)
    h = np.array([0.5, 1.0, 0.25], np.float32)
    w = np.array([0.4, 0.6, 0.8], np.float32)
    proto, pcls, pconf, pcnt, bound = U.prototypes_float64(feat, cls, w, h, 3)
    assert pcnt == 2 and pcls.tolist() == [2, 5, -1] and pconf.tolist() == [np.float32(0.6), np.float32(0.8), 0.0]      # ascending classes
    a, b = 0.5 + 2.0 ** -10, 0.25 + 2.0 ** -10
    n = math.sqrt(a * a + b * b)
    want = np.zeros(C)
    want[0], want[1] = a / n, b / n
    assert np.allclose(proto[1], want, rtol=1e-15, atol=0) and np.allclose(proto[0], e[2], rtol=1e-15) and not proto[2].any()
    assert 0 < bound[1, 0] < 1e-6 and bound[1, 3] == 0 and not bound[2].any()
    # h = -2^-10 on an only object: the weight is 0, the prototype all zeros
    p0 = U.prototypes_float64(feat[:1], cls[:1], w[:1], np.array([-2.0 ** -10], np.float32), 1)[0]
    assert not p0.any()


@pytest.mark.parametrize('budget', [7, 4, 2])
def test_selection_restatement_on_the_hand_pool(budget):
    c = U.hand_pool()
    assert U.quotas(3, budget) == {7: (2, 3, 1), 4: (2, 2, 1), 2: (2, 1, 0)}[budget]
    picks, stage, amb = U.select_float64(range(7), c['proto'], c['pcls'], c['pconf'], c['pcnt'], 3, budget)
    assert (picks.tolist(), stage.tolist()) == c['answers'][budget] and amb == []
    if budget == 7:
        # without the balance stage every image that passes the intra-class check is accepted: 4 now joins S with its class-1 prototype e_1,
        # so 5 (class 1, e_1: cosine 1) is redundant like 1; both are filled in behind the sweep
        picks, stage, _ = U.select_float64(range(7), c['proto'], c['pcls'], c['pconf'], c['pcnt'], 3, 7, class_balance=False)
        assert picks.tolist() == [0, 2, 3, 4, 6, 1, 5] and stage.tolist() == [1] * 5 + [3, 3]


def test_order_and_quotas_on_the_host():
    from aod_meh_hua_amd import scoring
    e = torch.tensor([0.5, 2.0, 0.5, 0.0, 2.0, 1.0])
    assert scoring.divproto_order(e, [4]).tolist() == [1, 5, 0, 2, 3] == U.sweep_order(e.numpy(), [4]).tolist()
    assert scoring.divproto_order(e, []).tolist() == [1, 4, 5, 0, 2, 3] and scoring.divproto_order(e, [0, 0, 3]).dtype == np.int64
    with pytest.raises(ValueError, match='NaN'):
        scoring.divproto_order(torch.tensor([0.0, float('nan')]), [])
    with pytest.raises(ValueError, match=r'outside \[0, 6\)'):
        scoring.divproto_order(e, [6])
    for n_cls, budget, a, b in ((20, 1000, 0.5, 0.75), (80, 2345, 0.5, 0.75), (4, 7, 0.5, 1.0), (3, 2, 0.5, 0.75), (1, 1, 1.0, 1.0), (4, 1, 0.3, 0.01)):
        got = scoring.divproto_quotas(n_cls, budget, a, b)
        assert got == U.quotas(n_cls, budget, a, b) and got[0] >= 1 and got[1] >= 1 and 0 <= got[2] < budget
    assert scoring.divproto_quotas(20, 1000) == (10, 75, 250) and scoring.divproto_chunk() >= 1


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def _objs(B=3, K=4, C=16):
    return [torch.zeros(B, K, C), torch.zeros(B, K, dtype=torch.int32), torch.zeros(B, K), torch.zeros(B, K), torch.zeros(B, dtype=torch.int32)]


def test_enms_prototypes_and_object_measure_refuse_bad_arguments_and_cpu_tensors():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    for K in (0, 65):
        with pytest.raises(ValueError, match='1..64 objects'):
            scoring.enms_prototypes(*_objs(K=K))
    for C in (12, 264):
        with pytest.raises(ValueError, match='multiple of 8 in 8..256'):
            scoring.enms_prototypes(*_objs(C=C))
    a = _objs()
    a[1] = a[1].long()
    with pytest.raises(ValueError, match='cls is not a 2-D int32'):
        scoring.enms_prototypes(*a)
    a = _objs()
    a[3] = a[3].double()
    with pytest.raises(ValueError, match='h is not a 2-D float32'):
        scoring.enms_prototypes(*a)
    a = _objs()
    a[3] = torch.zeros(3, 5)
    with pytest.raises(ValueError, match=r'h has shape \(3, 5\), expected \(3, 4\)'):
        scoring.enms_prototypes(*a)
    a = _objs()
    a[4] = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'cnt has shape \(4,\), expected \(3,\)'):
        scoring.enms_prototypes(*a)
    a = _objs()
    a[0] = torch.zeros(3, 4, 32)[:, :, ::2]
    with pytest.raises(ValueError, match='no copy is made'):
        scoring.enms_prototypes(*a)
    with pytest.raises(ValueError, match='t_enms is NaN'):
        scoring.enms_prototypes(*_objs(), t_enms=float('nan'))
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.enms_prototypes(*_objs())
    om = lambda **kw: scoring.object_measure(torch.zeros(2, 6), torch.zeros(2, 6, 5), torch.zeros(2, dtype=torch.int32), **kw)
    for bad in (0, 65):
        with pytest.raises(ValueError, match='max_obj must be in 1..64'):
            om(max_obj=bad)
    with pytest.raises(ValueError, match='NaN'):
        om(score_thr=float('nan'))
    with pytest.raises(ValueError, match=r'obj_cand has shape \(2, 5\)'):
        om(obj_cand=torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match='dets'):
        scoring.object_measure(torch.zeros(2, 6), torch.zeros(2, 7, 5), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(AodHipError, match='CPU tensor'):
        om()


def _pool(N=5, K=4, C=16):
    return [torch.zeros(N, K, C), torch.zeros(N, K, dtype=torch.int32), torch.zeros(N, K), torch.zeros(N, dtype=torch.int32)]


def test_divproto_select_refuses_bad_arguments_and_cpu_tensors():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    sel = lambda pool=None, order=range(5), n_cls=3, budget=2, **kw: scoring.divproto_select(np.array(list(order)), *(pool or _pool()), n_cls, budget, **kw)
    for K in (0, 65):
        with pytest.raises(ValueError, match='1..64 objects'):
            sel(_pool(K=K))
    for C in (12, 264):
        with pytest.raises(ValueError, match='multiple of 8 in 8..256'):
            sel(_pool(C=C))
    for n_cls in (0, 129):
        with pytest.raises(ValueError, match='n_cls must be in 1..128'):
            sel(n_cls=n_cls)
    with pytest.raises(ValueError, match='budget must be at least 1'):
        sel(budget=0)
    with pytest.raises(ValueError, match='budget 6 exceeds the 5 images'):
        sel(budget=6)
    with pytest.raises(ValueError, match='budget 3 exceeds the 2 images'):
        sel(order=[4, 1], budget=3)
    for kw in (dict(t_intra=float('nan')), dict(t_inter=float('nan'))):
        with pytest.raises(ValueError, match='NaN'):
            sel(**kw)
    for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float('nan')), dict(beta=0.0), dict(beta=-0.1), dict(beta=1.01)):
        with pytest.raises(ValueError, match=r'must lie in \(0, 1\]'):
            sel(**kw)
    with pytest.raises(ValueError, match='duplicated'):
        sel(order=[0, 1, 1])
    with pytest.raises(ValueError, match=r'outside \[0, 5\)'):
        sel(order=[0, 5])
    with pytest.raises(ValueError, match='integer indices'):
        scoring.divproto_select(np.array([0.0, 1.0]), *_pool(), 3, 1)
    a = _pool()
    a[1] = a[1].long()
    with pytest.raises(ValueError, match='pcls is not a 2-D int32'):
        sel(a)
    a = _pool()
    a[2] = torch.zeros(5, 3)
    with pytest.raises(ValueError, match=r'pconf has shape \(5, 3\), expected \(5, 4\)'):
        sel(a)
    a = _pool()
    a[3] = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'pcnt has shape \(4,\), expected \(5,\)'):
        sel(a)
    a = _pool()
    a[0] = torch.zeros(5, 4, 32)[:, :, ::2]
    with pytest.raises(ValueError, match='no copy is made'):
        sel(a)
    with pytest.raises(AodHipError, match='CPU tensor'):
        sel()


def test_uncertainty_fns_divproto_needs_the_labelled_set_and_the_names_are_exported():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis.test import Uncertainty_fns
    for name in ('DivProto_uncertainty', 'ENMS_uncertainty', 'single_gpu_enms'):
        assert name in apis.__all__ and callable(getattr(apis, name)), name
    assert callable(Uncertainty_fns.ENMS) and callable(Uncertainty_fns.DivProto)
    cfg, model = _detector()
    cfg.uncertainty_pool = 'DivProto'
    with pytest.raises(TypeError, match='X_L'):
        Uncertainty_fns.DivProto(cfg, model, _Loader())
    with pytest.raises(TypeError, match='X_L'):
        apis.calculate_uncertainty(cfg, model, _Loader(), score_thr=0.3, clsW=False)
    with pytest.raises(TypeError, match='X_L'):
        apis.DivProto_uncertainty(cfg, model, _Loader())
    for kw, msg in ((dict(max_obj=0), 'max_obj must be in 1..64'), (dict(max_obj=65), 'max_obj must be in 1..64'),
                    (dict(measure='variance'), 'unknown measure'), (dict(score_thr=float('nan')), 'NaN'), (dict(t_enms=float('nan')), 'NaN')):
        with pytest.raises(ValueError, match=msg):
            apis.single_gpu_enms(model, _Loader(), **kw)
    with pytest.raises(ValueError, match='objUnc is offered together with objDesc only'):
        model.simple_test(torch.zeros(1, 3, 64, 64), [{}], isEval=True, _padded=True, objUnc=True)
    with pytest.raises(ValueError, match='objUnc is offered together with objDesc only'):
        from aod_meh_hua_amd import scoring
        scoring.score_batch(model.bbox_head, [], [], [], [], [], model.bbox_head.test_cfg, isEval=True, _padded=True, objUnc=True)


def test_ssd_is_refused_by_name():
    from aod_meh_hua_amd import apis
    cfg, model = _detector('configs/_base_/Config_SSD.py')
    with pytest.raises(NotImplementedError, match='SSD'):
        apis.DivProto_uncertainty(cfg, model, _Loader(), X_L=[0], budget=1)
    with pytest.raises(NotImplementedError, match='SSD'):
        apis.ENMS_uncertainty(cfg, model, _Loader())
    with pytest.raises(NotImplementedError, match='SSD'):
        apis.single_gpu_enms(model, _Loader())
    with pytest.raises(NotImplementedError, match='SSD'):
        model.simple_test(torch.zeros(1, 3, 300, 300), [{}], isEval=True, _padded=True, objDesc=8, objUnc=True)


def test_the_driver_parser_accepts_both_pools_and_the_new_flags(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_divproto', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.setenv('LOCAL_RANK', '0')
    for pool in ('ENMS', 'DivProto'):
        monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', pool, '--synthetic', '8'])
        args = drv.parse_args()
        assert args.uncertainty_pool == pool and args.max_objects == 32
        assert (args.enms_thr, args.intra_thr, args.inter_thr, args.minority_alpha, args.minority_beta, args.no_class_balance) == (0.5, 0.7, 0.3, 0.5, 0.75, False)
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'DivProto', '--enms-thr', '0.4', '--intra-thr', '0.6', '--inter-thr', '0.2',
                                      '--minority-alpha', '0.25', '--minority-beta', '1', '--no-class-balance', '--max-objects', '16'])
    args = drv.parse_args()
    assert (args.enms_thr, args.intra_thr, args.inter_thr, args.minority_alpha, args.minority_beta, args.no_class_balance, args.max_objects) == \
        (0.4, 0.6, 0.2, 0.25, 1.0, True, 16)
    for bad in (['--minority-alpha', '0'], ['--minority-beta', '1.5'], ['--intra-thr', 'nan']):
        monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'DivProto'] + bad)
        with pytest.raises(SystemExit):
            drv.parse_args()
    capsys.readouterr()
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--help'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    out = capsys.readouterr().out
    assert all(s in out for s in ('ENMS', 'DivProto', '--enms-thr', '--intra-thr', '--inter-thr', '--minority-alpha', '--minority-beta', '--no-class-balance'))
    src = open(os.path.join(ROOT, 'tools', 'train_RetinaNet.py')).read()
    assert "cfg.uncertainty_pool == 'DivProto'" in src and 'zeroRate=0 if coreset else zeroRate' in src


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    for name in ('aod_object_measure', 'aod_enms_prototypes', 'aod_divproto_chunk', 'aod_divproto_ws_len', 'aod_divproto_select'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _C._SIGS[name]
    return lib


def test_entry_points_are_declared_exported_and_name_the_paper(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'Progressive' in hdr and 'CVPR 2022' in hdr and 'DESIGN 3s' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('aod_object_measure', 'aod_enms_prototypes', 'aod_divproto_chunk', 'aod_divproto_select'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr) and hasattr(lib, name), name
    assert re.search(r'\bsize_t\s+aod_divproto_ws_len\s*\(', hdr)
    assert lib.aod_divproto_chunk() == 64
    # the workspace: a header, 8 bytes per list entry, a byte per position; 0 for sizes the entry refuses
    small, big = lib.aod_divproto_ws_len(100, 4, 10), lib.aod_divproto_ws_len(100, 4, 20)
    assert big - small == 4 * 10 * 8 and small >= 4 * 10 * 8 + 100 and small % 8 == 0
    for bad in ((0, 4, 1), (2 ** 31, 4, 1), (10, 0, 1), (10, 129, 1), (10, 4, 0), (10, 4, 11)):
        assert lib.aod_divproto_ws_len(*bad) == 0, bad
    for doc in ('INTEGRATION.md', 'DESIGN.md', 'README.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'DivProto' in text and 'ENMS' in text, doc


def _rc(lib, rc, pattern):
    assert rc == -1 and re.search(pattern, lib.aod_last_error().decode()), (rc, lib.aod_last_error())


def test_c_entries_refuse_bad_arguments_before_any_launch(lib):
    """every refusal fires on the arguments alone: the pointers are fake (never dereferenced) and no GPU is needed"""
    p = ctypes.c_void_p(4096)
    nan = float('nan')
    enms = lambda B=2, K=4, C=16, t=0.5, feat=p, pick=p: lib.aod_enms_prototypes(feat, p, p, p, p, B, K, C, t, p, p, p, p, p, p, pick, None)
    _rc(lib, enms(B=0), 'batch must be positive')
    for K in (0, 65):
        _rc(lib, enms(K=K), r'max_obj must be in 1\.\.64')
    for C in (12, 264, 0):
        _rc(lib, enms(C=C), r'multiple of 8 in 8\.\.256')
    _rc(lib, enms(t=nan), 't_enms is NaN')
    _rc(lib, enms(feat=None), 'null pointer')
    _rc(lib, enms(feat=ctypes.c_void_p(4100)), '16-B aligned')
    _rc(lib, enms(pick=ctypes.c_void_p(4098)), '4-B aligned')
    om = lambda B=2, mn=8, K=4, t=0.3, h=p: lib.aod_object_measure(p, p, p, None, B, mn, K, t, h, None)
    _rc(lib, om(B=0), 'batch must be positive')
    for mn in (0, 1025):
        _rc(lib, om(mn=mn), r'max_num must be in 1\.\.1024')
    for K in (0, 65):
        _rc(lib, om(K=K), r'max_obj must be in 1\.\.64')
    _rc(lib, om(t=nan), 'NaN')
    _rc(lib, om(h=None), 'null pointer')

    def sel(M=10, N=10, K=4, C=16, n_cls=3, budget=2, ti=0.7, te=0.3, n_minor=2, quota=1, free=0, chunk=0, ws=p, proto=p):
        return lib.aod_divproto_select(p, M, N, proto, p, p, p, K, C, n_cls, budget, ti, te, n_minor, quota, free, 1, chunk, p, p, ws, None)
    for M in (0, 2 ** 31):
        _rc(lib, sel(M=M, N=2 ** 31), 'candidates')
    _rc(lib, sel(N=9), 'the pool holds 9 images')
    for K in (0, 65):
        _rc(lib, sel(K=K), r'max_obj must be in 1\.\.64')
    for C in (12, 264):
        _rc(lib, sel(C=C), r'multiple of 8 in 8\.\.256')
    for n_cls in (0, 129):
        _rc(lib, sel(n_cls=n_cls), r'n_cls must be in 1\.\.128')
    for budget in (0, 11):
        _rc(lib, sel(budget=budget), r'budget -?\d+ outside 1 \.\. 10')
    _rc(lib, sel(ti=nan), 'threshold is NaN')
    _rc(lib, sel(te=nan), 'threshold is NaN')
    for n_minor in (0, 4):
        _rc(lib, sel(n_minor=n_minor), 'n_minor')
    for quota in (0, 3):
        _rc(lib, sel(quota=quota), 'quota')
    for free in (-1, 3):
        _rc(lib, sel(free=free), 'free slots')
    for chunk in (-1, 65537):
        _rc(lib, sel(chunk=chunk), 'chunk')
    _rc(lib, sel(ws=None), 'null pointer')
    _rc(lib, sel(ws=ctypes.c_void_p(4100)), 'aligned')
    _rc(lib, sel(proto=ctypes.c_void_p(4104)), '16-B aligned')
