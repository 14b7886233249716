"""CPU tests (no GPU) of the Core-set acquisition: the float64 greedy of tests/coreset_util.py on a hand-worked case, the score
encoding update_X_L turns back into the picks, the argument checks of the public entry points, and the C entry points' declaration."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.coreset_util import descriptor_float64, greedy, replay_ratios

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


def test_greedy_on_a_hand_worked_case():
    """five points on a line, x = 0, 1, 5, 9, 10, point 1 labelled:
         mind = [1, 0, 16, 64, 81]                       -> pick 4, radius 81
         d(., 10) = [100, 81, 25, 1, 0]: mind [1, 0, 16, 1, 0]  -> pick 2, radius 16
         d(., 5)  = [25, 16, 0, 16, 25]: mind [1, 0, 0, 1, 0]   -> points 0 and 3 tie at 1: the lower index, pick 0, radius 1
         d(., 0)  = [0, 1, 25, 81, 100]: mind [0, 0, 0, 1, 0]   -> pick 3, radius 1"""
    X = np.array([[0.], [1.], [5.], [9.], [10.]])
    picks, radius, ties = greedy(X, [1], 4)
    assert picks.tolist() == [4, 2, 0, 3] and radius.tolist() == [81., 16., 1., 1.] and ties == 1
    assert replay_ratios(X, [1], picks).tolist() == [1., 1., 1., 1.]
    assert replay_ratios(X, [1], [4, 2, 3, 0]).tolist() == [1., 1., 1., 1.]          # (the other side of the tie is as good in float64)
    assert replay_ratios(X, [1], [4, 0]).tolist() == [1., 1 / 16]
    assert replay_ratios(X, [1], [3, 3]).tolist() == [64 / 81, -1.]                  # a worse pick, a repeated pick
    # the empty labelled set: every mind is +inf, the first pick is row 0 with radius inf
    picks, radius, _ = greedy(X, [], 2)
    assert picks.tolist() == [0, 4] and radius.tolist() == [np.inf, 100.]
    # duplicates: a selected point never wins, even when every remaining mind is 0
    picks, radius, ties = greedy(np.zeros((4, 3)), [2], 3)
    assert picks.tolist() == [0, 1, 3] and radius.tolist() == [0., 0., 0.] and ties == 2
    assert np.array_equal(descriptor_float64([np.arange(12.).reshape(1, 4, 3), np.ones((1, 1, 2))]), [[4.5, 5.5, 6.5, 1., 1.]])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_score_encoding_selects_exactly_the_picks(seed):
    """Coreset_uncertainty's vector (pick t scores budget - t, everything else 0) through update_X_L with a falsy zeroRate"""
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    g = np.random.default_rng(seed)
    N, budget = 60, 7
    perm = g.permutation(N)
    X_L, picks = np.sort(perm[:9]), perm[9:9 + budget]
    scores = torch.zeros(N)
    scores[torch.from_numpy(picks)] = torch.arange(budget, 0, -1, dtype=torch.float32)
    for zero_rate in (0, None):
        X_L_next, X_U_next = update_X_L(scores, np.arange(N), X_L, budget, zeroRate=zero_rate)
        assert X_L_next.tolist() == sorted(X_L.tolist() + picks.tolist())
        assert not set(X_U_next.tolist()) & set(X_L_next.tolist())


def test_kcenter_greedy_refuses_what_it_cannot_select():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    desc = torch.randn(10, 8)
    for bad in (desc[0], desc.double(), desc[:, ::2], desc.unsqueeze(0), [[0.0] * 8] * 10):
        with pytest.raises(ValueError, match='contiguous 2-D fp32'):
            scoring.kcenter_greedy(bad, [0], 1)
    for lab in ([10], [-1], torch.tensor([3, 11])):
        with pytest.raises(ValueError, match=r'outside \[0, 10\)'):
            scoring.kcenter_greedy(desc, lab, 1)
    with pytest.raises(ValueError, match='duplicated'):
        scoring.kcenter_greedy(desc, [2, 5, 2], 1)
    for b in (0, -3):
        with pytest.raises(ValueError, match='budget must be at least 1'):
            scoring.kcenter_greedy(desc, [0], b)
    with pytest.raises(ValueError, match='exceeds the 7 unselected rows'):
        scoring.kcenter_greedy(desc, [0, 1, 2], 8)
    with pytest.raises(ValueError, match='2048'):
        scoring.kcenter_greedy(torch.zeros(2, 2049), [0], 1)
    # a CPU tensor that passes every check: there is no CPU fallback
    for lab in ([0, 1, 2], [], np.array([4]), torch.tensor([9, 0])):
        with pytest.raises(AodHipError, match='CPU tensor'):
            scoring.kcenter_greedy(desc, lab, 7)


def test_pool_descriptor_refuses_what_it_cannot_pool():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    cl = lambda *s: torch.zeros(*s, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match='1..8 levels'):
        scoring.pool_descriptor([])
    with pytest.raises(ValueError, match='1..8 levels'):
        scoring.pool_descriptor([cl(2, 64, 1, 1)] * 9)
    with pytest.raises(ValueError, match='not a bf16'):
        scoring.pool_descriptor([cl(2, 64, 2, 2).float()], x3=False)
    with pytest.raises(ValueError, match='same positive batch size and width'):
        scoring.pool_descriptor([cl(2, 64, 2, 2), cl(3, 64, 1, 1)], x3=False)
    with pytest.raises(ValueError, match='channels_last'):
        scoring.pool_descriptor([torch.zeros(2, 64, 2, 2, dtype=torch.bfloat16)], x3=False)
    with pytest.raises(ValueError, match='multiple of 8'):
        scoring.pool_descriptor([cl(2, 36, 2, 2)], x3=False)
    with pytest.raises(ValueError, match='multiple of 64'):
        scoring.pool_descriptor([cl(2, 96, 2, 2)], x3=True)
    with pytest.raises(ValueError, match='do not make rows of 192'):
        scoring.pool_descriptor([cl(2, 192, 2, 2)], x3=True, channels=48)
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.pool_descriptor([cl(2, 192, 2, 2), cl(2, 192, 1, 1)], x3=True, channels=72)
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.pool_descriptor([cl(2, 64, 2, 2)], x3=False)


def test_uncertainty_fns_coreset_needs_the_labelled_set():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis.test import Uncertainty_fns
    assert 'Coreset_uncertainty' in apis.__all__ and 'single_gpu_descriptors' in apis.__all__
    cfg, model = _detector()
    cfg.uncertainty_pool = 'Coreset'
    with pytest.raises(TypeError, match='X_L'):
        Uncertainty_fns.Coreset(cfg, model, _Loader())
    with pytest.raises(TypeError, match='X_L'):
        apis.calculate_uncertainty(cfg, model, _Loader(), score_thr=0.3, clsW=False)
    with pytest.raises(TypeError, match='X_L'):
        apis.Coreset_uncertainty(cfg, model, _Loader())


def test_ssd_is_refused_by_name():
    from aod_meh_hua_amd.apis import Coreset_uncertainty
    cfg, model = _detector('configs/_base_/Config_SSD.py')
    with pytest.raises(NotImplementedError, match='SSD'):
        Coreset_uncertainty(cfg, model, _Loader(), X_L=[0], budget=1)
    with pytest.raises(NotImplementedError, match='SSD'):
        model.simple_test(torch.zeros(1, 3, 300, 300), [{}], isEval=True, justFeat=True)


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.aod_pool_descriptor.restype = ctypes.c_int
    lib.aod_pool_descriptor.argtypes = [P, I32, P, P, I32, I32, I32, P, I64, P]
    lib.aod_kcenter_ws_len.restype = ctypes.c_size_t
    lib.aod_kcenter_ws_len.argtypes = [I64]
    lib.aod_kcenter_greedy.restype = ctypes.c_int
    lib.aod_kcenter_greedy.argtypes = [P, I64, I32, P, I64, I64, P, P, P, P, P]
    return lib


def test_entry_points_are_declared_exported_and_name_the_paper(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'Sener' in hdr and 'Core-Set' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for ret, name in (('int', 'aod_pool_descriptor'), ('int', 'aod_kcenter_greedy'), ('size_t', 'aod_kcenter_ws_len'), ('int', 'aod_kcenter_chunk')):
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), hdr) and hasattr(lib, name)
    from aod_meh_hua_amd import _C
    assert len(_C._SIGS['aod_kcenter_greedy'][1]) == 11 and len(_C._SIGS['aod_pool_descriptor'][1]) == 10
    assert lib.aod_kcenter_chunk() >= 1
    assert lib.aod_kcenter_ws_len(0) == 0 and lib.aod_kcenter_ws_len(16551) >= 16551 and lib.aod_kcenter_ws_len(16551) % 8 == 0


def _greedy(lib, N=100, D=16, n_lab=3, budget=5, desc=16, lab=16, picks=16, radius=16, mind=16, ws=16):
    return lib.aod_kcenter_greedy(desc, N, D, lab, n_lab, budget, picks, radius, mind, ws, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(N=0), b'rows'), (dict(D=0), b'descriptor columns'), (dict(D=2049), b'descriptor columns'), (dict(n_lab=-1), b'labelled count'),
    (dict(n_lab=101), b'labelled count'), (dict(budget=0), b'budget'), (dict(budget=98), b'budget'), (dict(desc=None), b'null pointer'),
    (dict(lab=None), b'null pointer'), (dict(picks=None), b'null pointer'), (dict(radius=None), b'null pointer'), (dict(mind=None), b'null pointer'),
    (dict(ws=None), b'null pointer'), (dict(desc=20), b'16-B aligned'), (dict(ws=20), b'8-B aligned'),
])
def test_kcenter_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    """validation precedes every launch: this machine has no GPU, a launch attempt would fail differently (-3) or crash"""
    assert _greedy(lib, **kw) == -1
    assert msg in lib.aod_last_error()


def _desc(lib, nseg=2, row0=(0, 12), hw=(4, 1), C=64, x3=0, B=3, base=16, out=16, stride=128):
    r = (ctypes.c_int64 * 8)(*(list(row0) + [0] * 8)[:8]) if row0 is not None else None
    h = (ctypes.c_int32 * 8)(*(list(hw) + [1] * 8)[:8]) if hw is not None else None
    return lib.aod_pool_descriptor(base, nseg, r, h, C, x3, B, out, stride, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(nseg=0), b'1..8 segments'), (dict(nseg=9), b'1..8 segments'), (dict(base=None), b'null pointer'), (dict(out=None), b'null pointer'),
    (dict(row0=None), b'null pointer'), (dict(hw=None), b'null pointer'), (dict(C=0), b'multiple of 8'), (dict(C=36), b'multiple of 8'),
    (dict(B=0), b'batch'), (dict(stride=127), b'row stride'), (dict(base=24), b'16-B aligned'), (dict(hw=(4, 0)), b'segment 1'),
    (dict(row0=(-1, 0)), b'segment 0'),
])
def test_descriptor_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    assert _desc(lib, **kw) == -1
    assert msg in lib.aod_last_error()
