"""CPU tests (no GPU) of the CDAL acquisition: the float64 restatement of tests/cdal_util.py on hand-worked cases, the argument
checks of the public entry points, the driver's parser, and the C entry points' declaration and validation."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests.cdal_util import EPS, descriptor_float64, entropy_float64, greedy, replay_ratios, rows_float64, softmax_float64, symkl

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


# ---------------------------------------------------------------------------------------------------------------- the reference by hand
def test_one_region_gives_its_own_distribution():
    """C = 3, thr = 0.3.  Row 0 = ln [6, 3, 1]: p = [0.6, 0.3, 0.1], a region of class 0.  Row 1 = [0, 0, 0]: p = 1/3 each, 1/3 > 0.3, a
    region of class 0 too (lowest index) -- so it is pushed below the threshold with thr = 0.5 in the second half."""
    x = np.log(np.array([[[6., 3., 1.], [1., 1., 1.]]]))
    P, lnP, R, amb = descriptor_float64([x], 3, 0.5)
    assert R.tolist() == [[1, 0, 0]]
    want0 = (1 - EPS) * np.array([0.6, 0.3, 0.1]) + EPS / 3
    assert np.allclose(P[0, 0], want0, rtol=1e-14, atol=0) and np.allclose(P[0, 1:], 1 / 3, rtol=1e-14, atol=0)
    assert np.allclose(lnP, np.log(P), rtol=0, atol=0) and np.allclose(P.sum(axis=2), 1.0, rtol=1e-14)
    assert (0, 0, 1) in amb and (0, 0, 0) not in amb                  # the uniform row has no top-two gap
    # thr = 0.3: both rows are regions of class 0; weights H + 2^-10
    P, _, R, _ = descriptor_float64([x], 3, 0.3)
    p0, p1 = np.array([0.6, 0.3, 0.1]), np.full(3, 1 / 3)
    w0, w1 = entropy_float64(p0) + EPS, np.log(3.) + EPS
    assert R.tolist() == [[2, 0, 0]]
    assert np.allclose(P[0, 0], (1 - EPS) * (w0 * p0 + w1 * p1) / (w0 + w1) + EPS / 3, rtol=1e-14, atol=0)
    # two levels add up; a second image is independent
    x2 = np.concatenate([x, np.log(np.array([[[1., 8., 1.], [1., 1., 8.]]]))])
    P2, _, R2, _ = descriptor_float64([x2[:, :1], x2[:, 1:]], 3, 0.5)
    assert R2.tolist() == [[1, 0, 0], [0, 1, 1]] and np.array_equal(P2[0], descriptor_float64([x], 3, 0.5)[0][0])
    assert np.allclose(P2[1, 1], (1 - EPS) * np.array([.1, .8, .1]) + EPS / 3, rtol=1e-14, atol=0) and np.allclose(P2[1, 0], 1 / 3, rtol=1e-14)


def test_no_region_gives_the_uniform_descriptor_and_a_one_hot_row_weighs_the_floor():
    for C in (3, 7, 20):
        P, lnP, R, _ = descriptor_float64([np.zeros((2, 5, C))], C, 0.5)
        assert R.sum() == 0 and np.allclose(P, 1 / C, rtol=1e-15, atol=0) and np.allclose(lnP, -np.log(C), rtol=1e-14, atol=0)
    x = np.zeros((1, 2, 4))
    x[0, 0, 0] = 800.                                                 # one-hot in float64 too: H = 0 (0 ln 0 = 0), weight 2^-10, no NaN
    x[0, 1] = np.log([5., 2., 2., 1.])
    p = softmax_float64(x)
    assert p[0, 0].tolist() == [1., 0., 0., 0.] and entropy_float64(p)[0, 0] == 0
    P, lnP, R, _ = descriptor_float64([x], 4, 0.3)
    w1 = entropy_float64(p[0, 1]) + EPS
    assert np.isfinite(P).all() and np.isfinite(lnP).all() and R.tolist() == [[2, 0, 0, 0]]
    assert np.allclose(P[0, 0], (1 - EPS) * (EPS * p[0, 0] + w1 * p[0, 1]) / (EPS + w1) + EPS / 4, rtol=1e-14, atol=0)
    rows, _, _ = rows_float64([x], 4, 0.3)
    assert rows.shape == (1, 32) and np.array_equal(rows[0, :16], P.reshape(-1)) and np.array_equal(rows[0, 16:], lnP.reshape(-1))


def test_symkl_is_zero_on_the_diagonal_symmetric_and_the_symmetrised_kl():
    g = np.random.default_rng(3)
    P = g.random((6, 12)) + 0.01
    P /= P.reshape(6, 3, 4).sum(axis=2).repeat(4, axis=1)             # three distributions of four classes per row
    X = np.concatenate([P, np.log(P)], axis=1)
    D = np.stack([symkl(X, c) for c in range(6)])
    assert (np.diag(D) == 0).all() and np.array_equal(D, D.T) and (D[~np.eye(6, dtype=bool)] > 0).all()
    kl = lambda p, q: (p * np.log(p / q)).sum()
    assert np.isclose(D[1, 4], 0.5 * (kl(P[1], P[4]) + kl(P[4], P[1])), rtol=1e-12)
    # [A | 2A]: the squared Euclidean distance of A, exactly -- and the greedy under it is coreset_util's
    from tests import coreset_util
    A = g.integers(-3, 4, (20, 5)).astype(np.float64)
    X = np.concatenate([A, 2 * A], axis=1)
    assert all(np.array_equal(symkl(X, c), coreset_util.sqdist(A, c)) for c in range(20))
    pk, rk, _ = greedy(X, [3, 7], 6)
    pe, re_, _ = coreset_util.greedy(A, [3, 7], 6)
    assert pk.tolist() == pe.tolist() and np.array_equal(rk, re_)
    assert replay_ratios(X, [3, 7], pk).tolist() == [1.] * 6
    assert coreset_util.sqdist(A, 0)[0] == 0 and coreset_util.greedy.__module__ == 'tests.coreset_util'      # (the swap is undone)
    assert np.array_equal(coreset_util.sqdist(X, 1), ((X - X[1]) ** 2).sum(axis=1))


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_cdal_descriptor_refuses_what_it_cannot_describe():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    cl = lambda *s: torch.zeros(*s).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match='1..8 levels'):
        scoring.cdal_descriptor([], 20)
    with pytest.raises(ValueError, match='1..8 levels'):
        scoring.cdal_descriptor([cl(2, 20, 1, 1)] * 9, 20)
    with pytest.raises(ValueError, match=r'up to 32 classes .*2048'):
        scoring.cdal_descriptor([cl(2, 33 * 9, 2, 2)], 33)
    with pytest.raises(ValueError, match=r'up to 32 classes'):
        scoring.cdal_descriptor([cl(2, 80 * 9, 2, 2)], 80)
    with pytest.raises(ValueError, match='n_cls must be positive'):
        scoring.cdal_descriptor([cl(2, 20, 2, 2)], 0)
    with pytest.raises(ValueError, match='not an fp32'):
        scoring.cdal_descriptor([cl(2, 20, 2, 2).double()], 20)
    with pytest.raises(ValueError, match='not an fp32'):
        scoring.cdal_descriptor([torch.zeros(2, 20)], 20)
    with pytest.raises(ValueError, match='same positive batch size'):
        scoring.cdal_descriptor([cl(2, 20, 2, 2), cl(3, 20, 1, 1)], 20)
    with pytest.raises(ValueError, match='not a multiple of n_cls'):
        scoring.cdal_descriptor([cl(2, 50, 2, 2)], 20)
    with pytest.raises(ValueError, match='rows of 7 columns'):
        scoring.cdal_descriptor([torch.zeros(2, 9, 7)], 20)
    with pytest.raises(ValueError, match='no copy is made'):
        scoring.cdal_descriptor([torch.zeros(2, 40, 2, 2)], 20)
    with pytest.raises(ValueError, match='no copy is made'):
        scoring.cdal_descriptor([torch.zeros(2, 9, 40)[:, :, ::2]], 20)
    with pytest.raises(ValueError, match='NaN'):
        scoring.cdal_descriptor([cl(2, 20, 2, 2)], 20, score_thr=float('nan'))
    # a CPU tensor that passes every check: there is no CPU fallback
    for maps, C in (([cl(2, 180, 2, 2), cl(2, 180, 1, 1)], 20), ([torch.zeros(2, 9, 7)], 7), ([cl(1, 32, 1, 1)], 32)):
        with pytest.raises(AodHipError, match='CPU tensor'):
            scoring.cdal_descriptor(maps, C)


def test_kcenter_greedy_refuses_an_unknown_metric_and_an_odd_width_for_symkl():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    desc = torch.rand(10, 8) + 0.1
    for bad in ('euclid', 'kl', None, 1):
        with pytest.raises(ValueError, match='unknown metric'):
            scoring.kcenter_greedy(desc, [0], 1, metric=bad)
    with pytest.raises(ValueError, match=r"'symkl' .*D = 7 is odd"):
        scoring.kcenter_greedy(desc[:, :7].contiguous(), [0], 1, metric='symkl')
    with pytest.raises(ValueError, match='2048'):
        scoring.kcenter_greedy(torch.zeros(2, 2050), [0], 1, metric='symkl')
    for metric in ('sqeuclid', 'symkl'):                              # everything else is checked as before, and there is no CPU fallback
        with pytest.raises(ValueError, match='duplicated'):
            scoring.kcenter_greedy(desc, [2, 2], 1, metric=metric)
        with pytest.raises(AodHipError, match='CPU tensor'):
            scoring.kcenter_greedy(desc, [0, 1], 3, metric=metric)
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.kcenter_greedy(desc[:, :7].contiguous(), [0], 1)       # an odd D is fine for the default metric


def test_uncertainty_fns_cdal_needs_the_labelled_set():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis.test import Uncertainty_fns
    assert 'CDAL_uncertainty' in apis.__all__ and 'single_gpu_cdal_descriptors' in apis.__all__
    cfg, model = _detector()
    cfg.uncertainty_pool = 'CDAL'
    with pytest.raises(TypeError, match='X_L'):
        Uncertainty_fns.CDAL(cfg, model, _Loader())
    with pytest.raises(TypeError, match='X_L'):
        apis.calculate_uncertainty(cfg, model, _Loader(), score_thr=0.3, clsW=False)
    with pytest.raises(TypeError, match='X_L'):
        apis.CDAL_uncertainty(cfg, model, _Loader())


def test_ssd_is_refused_by_name():
    from aod_meh_hua_amd.apis import CDAL_uncertainty, single_gpu_cdal_descriptors
    cfg, model = _detector('configs/_base_/Config_SSD.py')
    with pytest.raises(NotImplementedError, match='SSD'):
        CDAL_uncertainty(cfg, model, _Loader(), X_L=[0], budget=1)
    with pytest.raises(NotImplementedError, match='SSD'):
        single_gpu_cdal_descriptors(model, _Loader())


def test_more_than_32_classes_are_refused_by_the_pool_pass():
    from aod_meh_hua_amd.apis import single_gpu_cdal_descriptors
    cfg, model = _detector()
    head = model.bbox_head
    head.num_classes = head.cls_out_channels = 80                     # (COCO; no forward is run: the check precedes the loop)
    with pytest.raises(ValueError, match='up to 32 classes'):
        single_gpu_cdal_descriptors(model, _Loader())


def test_the_driver_parser_accepts_cdal(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_cdal', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'CDAL', '--synthetic', '8'])
    args = drv.parse_args()
    assert args.uncertainty_pool == 'CDAL' and args.hua_score_thr == 0.3
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--help'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    assert 'CDAL' in capsys.readouterr().out
    src = open(os.path.join(ROOT, 'tools', 'train_RetinaNet.py')).read()
    assert "cfg.uncertainty_pool in ('Coreset', 'CDAL')" in src        # the X_L / zeroRate = 0 branch is Core-set's, widened


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    P, I32, I64, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.aod_cdal_ws_len.restype = ctypes.c_size_t
    lib.aod_cdal_ws_len.argtypes = [I32, P, I32, I32]
    lib.aod_cdal_descriptor.restype = ctypes.c_int
    lib.aod_cdal_descriptor.argtypes = [P, I32, P, I32, I32, F32, P, I64, P, I64, P]
    lib.aod_kcenter_greedy_ex.restype = ctypes.c_int
    lib.aod_kcenter_greedy_ex.argtypes = [P, I64, I32, P, I64, I64, P, P, P, P, P, I32]
    return lib


def test_entry_points_are_declared_exported_and_name_the_paper(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'Agarwal' in hdr and 'Contextual' in hdr and 'ECCV 2020' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for ret, name in (('int', 'aod_cdal_descriptor'), ('size_t', 'aod_cdal_ws_len'), ('int', 'aod_cdal_chunk'), ('int', 'aod_kcenter_greedy_ex'),
                      ('int', 'aod_kcenter_greedy')):
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), hdr) and hasattr(lib, name)
    from aod_meh_hua_amd import _C
    assert len(_C._SIGS['aod_kcenter_greedy_ex'][1]) == 12 and len(_C._SIGS['aod_cdal_descriptor'][1]) == 11
    assert len(_C._SIGS['aod_kcenter_greedy'][1]) == 11               # the old entry stays in the ABI
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'aod_cdal_descriptor' in integ and 'aod_kcenter_greedy_ex' in integ
    ch = lib.aod_cdal_chunk()
    assert ch >= 64 and ch % 64 == 0
    rows = (ctypes.c_int64 * 4)(1, 63, 65, 4099)
    per_image = sum(-(-r // ch) for r in rows)
    assert lib.aod_cdal_ws_len(4, rows, 20, 3) == 3 * per_image * 20 * 21
    assert lib.aod_cdal_ws_len(4, rows, 33, 3) == 0 and lib.aod_cdal_ws_len(0, rows, 20, 3) == 0 and lib.aod_cdal_ws_len(4, rows, 20, 0) == 0


def _greedy_ex(lib, N=100, D=16, n_lab=3, budget=5, desc=16, lab=16, picks=16, radius=16, mind=16, ws=16, metric=1):
    return lib.aod_kcenter_greedy_ex(desc, N, D, lab, n_lab, budget, picks, radius, mind, ws, None, metric)


@pytest.mark.parametrize('kw, msg', [
    (dict(D=15), b'is odd'), (dict(D=2047), b'is odd'), (dict(D=2049), b'descriptor columns'), (dict(D=2050), b'descriptor columns'),
    (dict(D=0), b'descriptor columns'), (dict(metric=2), b'metric 2'), (dict(metric=-1), b'metric -1'), (dict(N=0), b'rows'),
    (dict(budget=98), b'budget'), (dict(desc=None), b'null pointer'), (dict(desc=20), b'16-B aligned'),
    (dict(D=2049, metric=0), b'descriptor columns'), (dict(budget=0, metric=0), b'budget'),
])
def test_kcenter_ex_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    """validation precedes every launch: this machine has no GPU, a launch attempt would fail differently (-3) or crash"""
    assert _greedy_ex(lib, **kw) == -1
    assert msg in lib.aod_last_error()


def _desc(lib, L=2, rows=(40, 7), C=20, B=3, thr=0.3, maps=(16, 32), out=16, stride=800, ws=16, cap=1 << 20):
    r = (ctypes.c_int64 * 8)(*(list(rows) + [1] * 8)[:8]) if rows is not None else None
    m = (ctypes.c_void_p * 8)(*(list(maps) + [16] * 8)[:8]) if maps is not None else None
    return lib.aod_cdal_descriptor(m, L, r, C, B, thr, out, stride, ws, cap, None)


@pytest.mark.parametrize('kw, msg, rc', [
    (dict(L=0), b'1..8 levels', -1), (dict(L=9), b'1..8 levels', -1), (dict(C=33), b'1..32 classes', -1), (dict(C=0), b'1..32 classes', -1),
    (dict(B=0), b'batch', -1), (dict(rows=None), b'null level sizes', -1), (dict(rows=(40, 0)), b'level 1', -1), (dict(maps=None), b'null pointer', -1),
    (dict(out=None), b'null pointer', -1), (dict(ws=None), b'null pointer', -1), (dict(stride=799), b'row stride', -1),
    (dict(maps=(16, 0)), b'null map pointer (level 1)', -1), (dict(maps=(18, 32)), b'not 4-B aligned (level 0)', -1),
    (dict(thr=float('nan')), b'NaN', -1), (dict(cap=100), b'workspace too small', -2),
])
def test_descriptor_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg, rc):
    assert _desc(lib, **kw) == rc
    assert msg in lib.aod_last_error()
