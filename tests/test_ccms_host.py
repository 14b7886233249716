"""CPU tests (no GPU) of the CCMS acquisition: the float64 restatement of tests/ccms_util.py on a hand-computed case, the host
half of the two-stage pick (scoring.ccms_candidates), the argument checks of the public entry points, the driver's parser, and the C entry
points' declaration and validation."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests.ccms_util import directed_similarity, distance_matrix, greedy_matrix, object_descriptors_float64

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
def _three_images():
    """A: (class 0, f = (1, 0), w = 0.5), (class 1, f = (0, 1), w = 1);  B: (class 0, f = (0.6, 0.8), w = 0.8);  C: no object"""
    feat = np.zeros((3, 2, 2))
    feat[0, 0], feat[0, 1], feat[1, 0] = (1, 0), (0, 1), (0.6, 0.8)
    cls = np.array([[0, 1], [0, -1], [-1, -1]])
    w = np.array([[0.5, 1.0], [0.8, 0.0], [0.0, 0.0]])
    return feat, cls, w, np.array([2, 1, 0])


def test_restatement_on_a_hand_computed_case():
    feat, cls, w, cnt = _three_images()
    # S(A -> B): object 0 meets B's class-0 object at cosine 0.6, object 1 has no class-1 partner: (0.5 * 0.6 + 1 * 0) / 1.5 = 0.2
    assert np.isclose(directed_similarity(feat[0], cls[0], w[0], feat[1, :1], cls[1, :1]), 0.2, rtol=1e-15)
    # S(B -> A): its one object meets A's class-0 object: 0.6
    assert np.isclose(directed_similarity(feat[1, :1], cls[1, :1], w[1, :1], feat[0], cls[0]), 0.6, rtol=1e-15)
    assert directed_similarity(feat[2, :0], cls[2, :0], w[2, :0], feat[0], cls[0]) == 0.0          # no object: 0
    assert directed_similarity(feat[0], cls[0], w[0], feat[2, :0], cls[2, :0]) == 0.0              # no partner: 0
    D = distance_matrix(feat, cls, w, cnt)
    assert np.allclose(D, [[0, 0.6, 1], [0.6, 0, 1], [1, 1, 0]], rtol=1e-15) and np.array_equal(D, D.T)
    # a negative cosine counts as no match; the pad rows (class -1 on both sides) never match each other
    neg = np.array([[-1.0, 0.0]])
    assert directed_similarity(feat[0], cls[0], w[0], neg, np.array([0])) == 0.0
    assert directed_similarity(neg, np.array([0]), np.array([1.0]), feat[0], cls[0]) == 0.0
    # an identical pair of images: S = 1 both ways, d = 0
    D2 = distance_matrix(feat[[0, 0]], cls[[0, 0]], w[[0, 0]], cnt[[0, 0]])
    assert D2[0, 1] == 0.0


def test_object_restatement_gate_cut_and_missing():
    """two levels (2 cells x 3 anchors, 1 cell x 2 anchors), C = 2: anchors 0..5 are level 0, 6..7 level 1"""
    levels = [np.array([[[3., 4.], [0., 0.]]]), np.array([[[0., -2.]]])]
    cand_anchor = np.array([[7, 4, 0, 99]])                         # -> level 1 cell 0, level 0 cell 1, level 0 cell 0, outside
    dets = np.zeros((1, 6, 5), np.float32)
    dets[0, :, 4] = [0.9, 0.3, 0.8, 0.7, 0.6, 0.95]                 # row 1 sits on the threshold (strict: no object), row 5 is >= num
    labels = np.array([[5, 1, 2, 3, 4, 6]])
    obj_cand = np.array([[0, 1, -1, 3, 1, 2]])                      # row 2: no candidate; row 3: an anchor outside every level
    feat, cls, w, cnt, missing = object_descriptors_float64(levels, [3, 2], cand_anchor, dets, labels, np.array([5]), obj_cand, 4, 0.3)
    assert cnt.tolist() == [2] and missing.tolist() == [2]
    assert cls.tolist() == [[5, 4, -1, -1]] and np.allclose(w, [[np.float32(0.9), np.float32(0.6), 0, 0]], rtol=0)
    assert np.allclose(feat[0, 0], [0, -1]) and np.array_equal(feat[0, 1], [0, 0]) and not feat[0, 2:].any()      # an all-zero row stays zero
    feat, cls, w, cnt, missing = object_descriptors_float64(levels, [3, 2], cand_anchor, dets, labels, np.array([5]), obj_cand, 1, 0.3)
    assert cnt.tolist() == [1] and missing.tolist() == [2] and cls.tolist() == [[5]]                               # the cut keeps the first


def test_greedy_on_a_matrix_by_hand():
    D = np.array([[0, 1, 4, 4], [1, 0, 2, 3], [4, 2, 0, 3], [4, 3, 3, 0]], np.float32)
    picks, radius, ties = greedy_matrix(D, [], 4)
    # row 0 first (radius inf); then rows 2 and 3 tie at 4: the lower index; then mind = [0, 1, 0, 3]
    assert picks.tolist() == [0, 2, 3, 1] and radius.tolist() == [np.inf, 4, 3, 1] and ties == 2
    picks, radius, _ = greedy_matrix(D, [3], 2)
    assert picks.tolist() == [0, 2] and radius.tolist() == [4, 3]      # mind = D[3] = [4, 3, 3, 0]; then min with D[0]: [0, 1, 3, 0]


# ---------------------------------------------------------------------------------------------------------------- stage 1
def test_candidates_order_ties_exclusion_and_cut():
    from aod_meh_hua_amd.scoring import ccms_candidates
    u = np.array([0.5, 2.0, 2.0, 0.0, 0.5, 3.0, 0.0, 2.0], np.float32)
    got = ccms_candidates(u, [], 2, 4)
    assert got.dtype == np.int64 and got.tolist() == [5, 1, 2, 7, 0, 4, 3, 6]             # ties by ascending index; M = min(8, 8)
    assert ccms_candidates(u, [5, 2], 2, 2).tolist() == [1, 7, 0, 4]                      # X_L never appears; M = ceil(2 * 2)
    assert ccms_candidates(u, [5, 2], 2, 1.2).tolist() == [1, 7, 0]                       # ceil(2.4) = 3
    assert ccms_candidates(torch.from_numpy(u), torch.tensor([1]), 3, 1).tolist() == [5, 2, 7]
    assert ccms_candidates(u, np.arange(6), 2, 4).tolist() == [7, 6]                      # cut by the number of unlabelled images
    assert ccms_candidates(np.zeros(5), [], 1, 3).tolist() == [0, 1, 2]                   # all tied: index order


def test_candidates_raise_on_too_few_and_too_many():
    from aod_meh_hua_amd.scoring import CCMS_MAX_IMAGES, ccms_candidates
    u = np.arange(10, dtype=np.float32)
    with pytest.raises(ValueError, match='fewer than the budget'):
        ccms_candidates(u, np.arange(8), 3, 4)                      # two unlabelled images, budget 3
    with pytest.raises(ValueError, match='fewer than the budget'):
        ccms_candidates(u, [], 4, 0.5)                              # factor < 1
    assert CCMS_MAX_IMAGES == 32768
    big = np.zeros(CCMS_MAX_IMAGES + 8, np.float32)
    with pytest.raises(ValueError, match='32768'):
        ccms_candidates(big, [], (CCMS_MAX_IMAGES + 4) // 4 + 1, 4)
    assert ccms_candidates(big, [], CCMS_MAX_IMAGES // 4, 4).shape == (CCMS_MAX_IMAGES,)
    with pytest.raises(ValueError, match='budget must be at least 1'):
        ccms_candidates(u, [], 0, 4)
    with pytest.raises(ValueError, match='outside'):
        ccms_candidates(u, [10], 1, 4)
    with pytest.raises(ValueError, match='NaN'):
        ccms_candidates(np.array([0.0, np.nan]), [], 1, 2)
    with pytest.raises(ValueError, match='candidate_factor'):
        ccms_candidates(u, [], 1, 0)


# ---------------------------------------------------------------------------------------------------------------- argument checks
def _gather_args(B=2, n=5, max_num=4, width=16):
    feats = [torch.zeros(B, width, 2, 2, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last),
             torch.zeros(B, width, 1, 1, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)]

    class Cand:
        cand_anchor = torch.zeros(B, n, dtype=torch.int32)
    return [feats, Cand, torch.zeros(B, max_num, 5), torch.zeros(B, max_num, dtype=torch.int64), torch.zeros(B, dtype=torch.int32),
            torch.zeros(B, max_num, dtype=torch.int32), 9]


def test_object_descriptors_refuses_what_it_cannot_describe():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    od = lambda a, **kw: scoring.object_descriptors(*a, **dict(dict(max_obj=8, score_thr=0.3, x3=False), **kw))
    with pytest.raises(ValueError, match='1..8 levels'):
        od([[]] + _gather_args()[1:])
    a = _gather_args()
    a[0][1] = a[0][1].float()
    with pytest.raises(ValueError, match=r'level 1 is not a bf16'):
        od(a)
    a = _gather_args()
    a[0][1] = torch.zeros(3, 16, 1, 1, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match=r'level 1 has shape \(3, 16, 1, 1\)'):
        od(a)
    with pytest.raises(ValueError, match='do not make rows of 20 columns'):
        od(_gather_args(width=20))
    with pytest.raises(ValueError, match='multiple of 64'):
        od(_gather_args(), x3=True)
    for bad in (0, 65):
        with pytest.raises(ValueError, match='max_obj must be in 1..64'):
            od(_gather_args(), max_obj=bad)
    with pytest.raises(ValueError, match='NaN'):
        od(_gather_args(), score_thr=float('nan'))
    a = _gather_args()
    a[6] = [9, 9, 9]
    with pytest.raises(ValueError, match='num_anchors'):
        od(a)
    a = _gather_args()
    a[5] = a[5].long()
    with pytest.raises(ValueError, match='obj_cand is not a 2-D int32'):
        od(a)
    a = _gather_args()
    a[3] = torch.zeros(2, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match=r'labels has shape \(2, 5\), expected \(2, 4\)'):
        od(a)
    a = _gather_args()
    a[2] = torch.zeros(2, 4, 6)
    with pytest.raises(ValueError, match=r'dets has shape \(2, 4, 6\)'):
        od(a)
    a = _gather_args()
    a[4] = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'num has shape \(3,\)'):
        od(a)
    with pytest.raises(AodHipError, match='CPU tensor'):            # a CPU call that passes every check: there is no CPU fallback
        od(_gather_args())


def test_ccms_distance_and_matrix_greedy_refuse_bad_shapes_and_cpu_tensors():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    ok = lambda M=3, K=4, C=16: [torch.zeros(M, K, C), torch.zeros(M, K, dtype=torch.int32), torch.zeros(M, K), torch.zeros(M, dtype=torch.int32)]
    with pytest.raises(ValueError, match=r'feat has shape \(3, 65, 16\).*1..64 objects'):
        scoring.ccms_distance(*ok(K=65))
    for C in (12, 264):
        with pytest.raises(ValueError, match=r'multiple of 8 in 8..256'):
            scoring.ccms_distance(*ok(C=C))
    a = ok()
    a[1] = a[1].long()
    with pytest.raises(ValueError, match='cls is not a 2-D int32'):
        scoring.ccms_distance(*a)
    a = ok()
    a[2] = torch.zeros(3, 5)
    with pytest.raises(ValueError, match=r'w has shape \(3, 5\), expected \(3, 4\)'):
        scoring.ccms_distance(*a)
    a = ok()
    a[3] = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'cnt has shape \(4,\), expected \(3,\)'):
        scoring.ccms_distance(*a)
    a = ok()
    a[0] = torch.zeros(3, 4, 32)[:, :, ::2]
    with pytest.raises(ValueError, match='no copy is made'):
        scoring.ccms_distance(*a)
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.ccms_distance(*ok())
    D = torch.zeros(6, 6)
    with pytest.raises(ValueError, match='square'):
        scoring.kcenter_greedy_matrix(torch.zeros(6, 5), [], 1)
    with pytest.raises(ValueError, match='square'):
        scoring.kcenter_greedy_matrix(D.double(), [], 1)
    with pytest.raises(ValueError, match='duplicated'):
        scoring.kcenter_greedy_matrix(D, [2, 2], 1)
    with pytest.raises(ValueError, match=r'outside \[0, 6\)'):
        scoring.kcenter_greedy_matrix(D, [6], 1)
    with pytest.raises(ValueError, match='exceeds the 4 unselected rows'):
        scoring.kcenter_greedy_matrix(D, [0, 1], 5)
    with pytest.raises(ValueError, match='at least 1'):
        scoring.kcenter_greedy_matrix(D, [], 0)
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.kcenter_greedy_matrix(D, [0], 2)


def test_uncertainty_fns_ccms_needs_the_labelled_set():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis.test import Uncertainty_fns
    assert 'CCMS_uncertainty' in apis.__all__ and 'single_gpu_object_descriptors' in apis.__all__
    cfg, model = _detector()
    cfg.uncertainty_pool = 'CCMS'
    with pytest.raises(TypeError, match='X_L'):
        Uncertainty_fns.CCMS(cfg, model, _Loader())
    with pytest.raises(TypeError, match='X_L'):
        apis.calculate_uncertainty(cfg, model, _Loader(), score_thr=0.3, clsW=False)
    with pytest.raises(TypeError, match='X_L'):
        apis.CCMS_uncertainty(cfg, model, _Loader())
    for kw, msg in ((dict(max_obj=65), 'max_obj must be in 1..64'), (dict(measure='variance'), 'unknown measure'),
                    (dict(aggregate='median'), 'unknown aggregate'), (dict(score_thr=float('nan')), 'NaN')):
        with pytest.raises(ValueError, match=msg):
            apis.single_gpu_object_descriptors(model, _Loader(), **kw)


def test_ssd_is_refused_by_name():
    from aod_meh_hua_amd.apis import CCMS_uncertainty, single_gpu_object_descriptors
    cfg, model = _detector('configs/_base_/Config_SSD.py')
    with pytest.raises(NotImplementedError, match='SSD'):
        CCMS_uncertainty(cfg, model, _Loader(), X_L=[0], budget=1)
    with pytest.raises(NotImplementedError, match='SSD'):
        single_gpu_object_descriptors(model, _Loader())
    with pytest.raises(NotImplementedError, match='SSD'):
        model.simple_test(torch.zeros(1, 3, 300, 300), [{}], isEval=True, _padded=True, objDesc=8)
    _, retina = _detector()
    with pytest.raises(ValueError, match='padded evaluation outputs'):
        retina.simple_test(torch.zeros(1, 3, 64, 64), [{}], isEval=True, objDesc=8)


def test_the_driver_parser_accepts_ccms(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_ccms', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'CCMS', '--synthetic', '8'])
    args = drv.parse_args()
    assert args.uncertainty_pool == 'CCMS' and args.candidate_factor == 4.0 and args.max_objects == 32
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'CCMS', '--candidate-factor', '2.5', '--max-objects', '16'])
    args = drv.parse_args()
    assert args.candidate_factor == 2.5 and args.max_objects == 16
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--help'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    out = capsys.readouterr().out
    assert 'CCMS' in out and '--candidate-factor' in out and '--max-objects' in out
    src = open(os.path.join(ROOT, 'tools', 'train_RetinaNet.py')).read()
    assert "cfg.uncertainty_pool == 'CCMS'" in src and 'zeroRate=0 if coreset else zeroRate' in src      # Core-set's branch, widened


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    P, I32, I64, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.aod_object_descriptors.restype = ctypes.c_int
    lib.aod_object_descriptors.argtypes = [P, I32, P, P, I32, I32, I32, P, I32, P, P, P, P, I32, I32, F32, P, P, P, P, P, P]
    lib.aod_ccms_distance.restype = ctypes.c_int
    lib.aod_ccms_distance.argtypes = [P, P, P, P, I32, I32, I32, P, P]
    lib.aod_kcenter_greedy_matrix.restype = ctypes.c_int
    lib.aod_kcenter_greedy_matrix.argtypes = [P, I64, P, I64, I64, P, P, P, P, P]
    lib.aod_det_uncertainty_ex.restype = ctypes.c_int
    lib.aod_det_uncertainty_ex.argtypes = [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, F32, P, P, P, P, P]
    return lib


def test_entry_points_are_declared_exported_and_name_the_paper(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'Plug and Play Active Learning' in hdr and 'CVPR 2024' in hdr and 'DESIGN 3o' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('aod_object_descriptors', 'aod_ccms_distance', 'aod_kcenter_greedy_matrix', 'aod_det_uncertainty_ex', 'aod_ccms_max_images',
                 'aod_det_uncertainty', 'aod_kcenter_greedy'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr) and hasattr(lib, name), name
    from aod_meh_hua_amd import _C
    assert len(_C._SIGS['aod_object_descriptors'][1]) == 22 and len(_C._SIGS['aod_ccms_distance'][1]) == 9
    assert len(_C._SIGS['aod_kcenter_greedy_matrix'][1]) == 10 and len(_C._SIGS['aod_det_uncertainty_ex'][1]) == 18
    assert len(_C._SIGS['aod_det_uncertainty'][1]) == 17            # the old entry stays in the ABI
    assert lib.aod_ccms_max_images() == 32768
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(n in integ for n in ('aod_object_descriptors', 'aod_ccms_distance', 'aod_kcenter_greedy_matrix'))


def _dist(lib, feat=16, cls=16, w=16, cnt=16, M=5, K=32, C=256, out=16):
    return lib.aod_ccms_distance(feat, cls, w, cnt, M, K, C, out, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(M=0), b'1..32768 images'), (dict(M=32769), b'1..32768 images'), (dict(K=0), b'max_obj must be in 1..64'),
    (dict(K=65), b'max_obj must be in 1..64'), (dict(C=264), b'multiple of 8 in 8..256'), (dict(C=0), b'multiple of 8 in 8..256'),
    (dict(C=100), b'multiple of 8 in 8..256'), (dict(feat=None), b'null pointer'), (dict(out=None), b'null pointer'),
    (dict(feat=24), b'16-B aligned'), (dict(cnt=18), b'4-B aligned'),
])
def test_distance_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    """validation precedes every launch: this machine has no GPU, a launch attempt would fail differently (-3) or crash"""
    assert _dist(lib, **kw) == -1
    assert msg in lib.aod_last_error()


def _gather(lib, nseg=2, base=(32, 64), hw=(20, 6), na=(9, 9), C=256, x3=0, B=3, anchor=16, n=50, dets=16, labels=16, num=16, cand=16, max_num=8,
            max_obj=8, thr=0.3, feat=16, cls=16, w=16, cnt=16, missing=16):
    pb = (ctypes.c_void_p * 8)(*(list(base) + [16] * 8)[:8]) if base is not None else None
    return lib.aod_object_descriptors(pb, nseg, (ctypes.c_int32 * 8)(*(list(hw) + [1] * 8)[:8]), (ctypes.c_int32 * 8)(*(list(na) + [1] * 8)[:8]), C, x3,
                                      B, anchor, n, dets, labels, num, cand, max_num, max_obj, thr, feat, cls, w, cnt, missing, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(nseg=0), b'1..8 levels'), (dict(nseg=9), b'1..8 levels'), (dict(C=20), b'multiple of 8 in 8..1024'), (dict(C=1032), b'multiple of 8'),
    (dict(B=0), b'batch must be positive'), (dict(n=0), b'candidate row'), (dict(max_num=0), b'max_num must be in 1..1024'),
    (dict(max_num=1025), b'max_num must be in 1..1024'), (dict(max_obj=0), b'max_obj must be in 1..64'), (dict(max_obj=65), b'max_obj must be in 1..64'),
    (dict(thr=float('nan')), b'score_thr is NaN'), (dict(base=None), b'null pointer'), (dict(cand=None), b'null pointer'),
    (dict(base=(32, 72)), b'level 1: rows must be 16-B aligned'), (dict(hw=(20, 0)), b'level 1: 0 cells'), (dict(na=(0, 9)), b'level 0'),
    (dict(feat=24), b'feat must be 16-B aligned'), (dict(labels=20), b'aligned to their element size'),
])
def test_gather_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    assert _gather(lib, **kw) == -1
    assert msg in lib.aod_last_error()


@pytest.mark.parametrize('kw, msg', [
    (dict(N=0), b'rows'), (dict(n_lab=-1), b'labelled count'), (dict(n_lab=11), b'labelled count'), (dict(budget=0), b'budget'),
    (dict(budget=8), b'budget'), (dict(dist=None), b'null pointer'), (dict(lab=None), b'null pointer'), (dict(ws=20), b'8-B aligned'),
])
def test_matrix_greedy_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    a = dict(dict(dist=16, N=10, lab=16, n_lab=3, budget=5, picks=16, radius=16, mind=16, ws=16), **kw)
    assert lib.aod_kcenter_greedy_matrix(a['dist'], a['N'], a['lab'], a['n_lab'], a['budget'], a['picks'], a['radius'], a['mind'], a['ws'], None) == -1
    assert msg in lib.aod_last_error()


def test_det_uncertainty_ex_validates_like_the_old_entry(lib):
    rc = lib.aod_det_uncertainty_ex(16, 16, 16, 16, 16, 2, 10, 21, 8, 3, 0, 0, 0.3, 16, None, None, 16, None)
    assert rc == -1 and b'layout 3' in lib.aod_last_error()
    rc = lib.aod_det_uncertainty_ex(16, 16, 16, 16, 16, 2, 10, 21, 8, 0, 0, 0, 0.3, 16, None, None, 18, None)
    assert rc == -1 and b'aligned to their element size' in lib.aod_last_error()
