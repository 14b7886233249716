"""CPU tests (no GPU) of the class difficulty: the float64 restatement of tests/difficulty_util.py on a hand-computed case, the
delta-only box quality against boxes decoded from real anchors, the weight formula's end points, the C entries' declaration and refusals,
the wrappers' refusals, the heads' state_dict keys and checkpoint behaviour, the driver's flags, and the cross-rank broadcast helper."""
import ctypes
import importlib.util
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import difficulty_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD = dict(xi=0.6, momentum=0.99, alpha=0.3, beta=0.2)


def _cfg(config='configs/_base_/Config_RetinaNet.py'):
    from aod_meh_hua_amd.mmcv_lite import Config
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    return cfg


def _head(config='configs/_base_/Config_RetinaNet.py', **extra):
    from aod_meh_hua_amd.models.builder import build_head
    cfg = _cfg(config)
    return build_head(dict(cfg.model.bbox_head, train_cfg=cfg.model.train_cfg, test_cfg=cfg.model.test_cfg, **extra))


# ---------------------------------------------------------------------------------------------------------------- the reference by hand
def test_restatement_on_a_hand_computed_case():
    # four rows, C = 2: row 0 positive of class 0 with the prediction on the target; row 1 background; row 2 positive of class 1 whose
    # prediction is the target moved by half a width; row 3 a foreground label without weight
    cls = np.array([[0.0, 0.0], [9.0, 9.0], [0.0, math.log(3.0)], [1.0, 1.0]], np.float32)
    labels, lw = np.array([0, 2, 1, 1]), np.array([1.0, 1.0, 0.5, 0.0], np.float32)
    bt = np.zeros((4, 4), np.float32)
    bp = np.zeros((4, 4), np.float32)
    bp[2, 0] = 0.5
    assert U.positives(labels, lw, 2).tolist() == [0, 2]
    # softmax: row 0 -> 1/2, row 2 -> 3/4 (float32 log(3) carries 3e-8); sigmoid: 1/2 and 3/4 as well
    assert U.class_prob64(cls[0], 0, 'edl') == 0.5 and abs(U.class_prob64(cls[2], 1, 'edl') - 0.75) < 1e-7
    assert U.class_prob64(cls[0], 0, 'sigmoid') == 0.5 and abs(U.class_prob64(cls[2], 1, 'sigmoid') - 0.75) < 1e-7
    # unit boxes: identical -> 1; moved by half a width -> overlap 1/2, union 3/2
    assert U.delta_iou64(bp[0], bt[0]) == 1.0 and abs(U.delta_iou64(bp[2], bt[2]) - 1.0 / 3.0) < 1e-15
    S, n, qs = U.batch_stat64(cls, labels, lw, bp, bt, 'edl')
    q0, q2 = 1.0 - 0.5 ** 0.6, 1.0 - 0.75 ** 0.6 * (1.0 / 3.0) ** 0.4
    assert n.tolist() == [1, 1] and abs(S[0] - q0) < 1e-12 and abs(S[1] - q2) < 1e-7 and sorted(qs) == [0, 2]
    # the EMA moves the classes that were seen and keeps the others' value
    d = U.ema64(np.array([1.0, 0.25], np.float32), np.array([q0, 0.0]), np.array([1, 0]))
    assert abs(d[0] - (0.99 + 0.01 * q0)) < 1e-15 and d[1] == 0.25
    # q's edges: P = 0 or IoU = 0 -> 1, both 1 -> 0
    assert U.difficulty64(0.0, 1.0) == 1.0 and U.difficulty64(1.0, 0.0) == 1.0 and U.difficulty64(1.0, 1.0) == 0.0
    # the clamp of dw: beyond |ln(16 / 1000)| both widths are the clamp's, the boxes coincide
    far = np.array([0, 0, 9.0, 0], np.float32), np.array([0, 0, 7.0, 0], np.float32)
    assert U.delta_iou64(*far) == 1.0


def test_delta_only_iou_equals_the_iou_of_boxes_decoded_against_anchors():
    g = np.random.default_rng(5)
    worst = 0.0
    for means, stds in (((0., 0., 0., 0.), (1., 1., 1., 1.)), ((0.01, -0.02, 0.03, 0.0), (0.1, 0.1, 0.2, 0.2))):
        for _ in range(500):
            x1, y1 = g.uniform(-50, 400, 2)
            anchor = (x1, y1, x1 + g.uniform(4, 300), y1 + g.uniform(4, 300))
            scale = 1.0 / np.asarray(stds)
            dp = (g.standard_normal(4) * (0.4, 0.4, 0.6, 0.6) * scale).astype(np.float32)
            dt = (g.standard_normal(4) * (0.4, 0.4, 0.6, 0.6) * scale).astype(np.float32)
            a, b = U.delta_iou64(dp, dt, means, stds), U.anchor_iou64(anchor, dp, dt, means, stds)
            worst = max(worst, abs(a - b))
    assert worst < 1e-12, worst


def test_weight_formula_end_points():
    w = U.class_weight64(np.array([0.0, 1.0, 0.5]))
    assert w[0] == 1.0 and abs(w[1] - 1.2) < 1e-15 and 1.0 < w[2] < 1.2
    assert np.all(np.diff(U.class_weight64(np.linspace(0, 1, 50))) > 0)
    head = _head(class_difficulty=CD)
    assert head.class_weight.shape == (21,) and head.class_difficulty.tolist() == [1.0] * 20
    assert np.allclose(head.class_weight[:20].numpy(), 1.2, rtol=0, atol=2.0 ** -22) and float(head.class_weight[20]) == 1.0
    head.class_difficulty.zero_()
    assert head.refresh_class_weight().tolist() == [1.0] * 21
    head.class_difficulty.copy_(torch.linspace(0, 1, 20))
    got = head.refresh_class_weight().numpy().astype(np.float64)
    assert np.abs(got[:20] - U.class_weight64(np.linspace(0, 1, 20, dtype=np.float32))).max() < 4 * 2.0 ** -23 and got[20] == 1.0


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    P, I32, I64, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.aod_class_difficulty_ws_len.restype = ctypes.c_size_t
    lib.aod_class_difficulty_ws_len.argtypes = [I64, I32]
    lib.aod_class_difficulty_accum.restype = ctypes.c_int
    lib.aod_class_difficulty_accum.argtypes = [P, P, P, P, P, I64, I32, I32, P, P, F32, F32, P, P, P]
    lib.aod_class_difficulty_update.restype = ctypes.c_int
    lib.aod_class_difficulty_update.argtypes = [P, P, I32, F32, P]
    lib.aod_det_uncertainty_w.restype = ctypes.c_int
    lib.aod_det_uncertainty_w.argtypes = [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, F32, P, P, P, P, P, P]
    return lib


def test_entry_points_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'DESIGN 3p' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('aod_class_difficulty_accum', 'aod_class_difficulty_update', 'aod_det_uncertainty_w', 'aod_det_uncertainty_ex'):
        assert re.search(r'\bint\s+%s\s*\(' % name, code) and hasattr(lib, name), name
    assert re.search(r'\bsize_t\s+aod_class_difficulty_ws_len\s*\(', code) and hasattr(lib, 'aod_class_difficulty_ws_len')
    from aod_meh_hua_amd import _C, hipops, scoring
    assert len(_C._SIGS['aod_class_difficulty_accum'][1]) == 15 and len(_C._SIGS['aod_class_difficulty_update'][1]) == 5
    assert len(_C._SIGS['aod_det_uncertainty_w'][1]) == 19 and len(_C._SIGS['aod_det_uncertainty_ex'][1]) == 18
    assert callable(hipops.class_difficulty_accum) and callable(hipops.class_difficulty_update)
    import inspect
    assert inspect.signature(scoring.det_uncertainty).parameters['class_w'].default is None
    # the workspace: one [2C] row per block, at most 256 blocks of 1024 rows
    assert lib.aod_class_difficulty_ws_len(1, 20) == 40 and lib.aod_class_difficulty_ws_len(1025, 20) == 80
    assert lib.aod_class_difficulty_ws_len(10 ** 7, 80) == 256 * 160 and lib.aod_class_difficulty_ws_len(0, 20) == 0


def test_c_entries_refuse_bad_arguments_before_a_launch(lib):
    F4 = ctypes.c_float * 4
    m, s = F4(0, 0, 0, 0), F4(1, 1, 1, 1)

    def accum(cls=16, labels=16, lw=16, bp=16, bt=16, nrows=8, C=20, form=0, means=m, stds=s, clip=0.016, xi=0.6, acc=16, ws=16):
        rc = lib.aod_class_difficulty_accum(cls, labels, lw, bp, bt, nrows, C, form, means, stds, clip, xi, acc, ws, None)
        return rc, lib.aod_last_error().decode()
    for kw, msg in ((dict(nrows=-1), 'negative row count'), (dict(C=0), 'C must be in 1..128'), (dict(C=129), 'C must be in 1..128'),
                    (dict(form=2), 'form 2'), (dict(form=-1), 'form -1'), (dict(xi=1.5), 'xi must be in'), (dict(xi=-0.1), 'xi must be in'),
                    (dict(xi=float('nan')), 'xi must be in'), (dict(clip=0.0), 'wh_ratio_clip'), (dict(clip=float('nan')), 'wh_ratio_clip'),
                    (dict(means=None), 'means4'), (dict(stds=None), 'means4'), (dict(means=F4(0, float('inf'), 0, 0)), 'not finite'),
                    (dict(acc=None), 'null pointer'), (dict(acc=18), 'acc must be aligned'), (dict(cls=None), 'null pointer'),
                    (dict(labels=None), 'null pointer'), (dict(lw=None), 'null pointer'), (dict(bp=None), 'null pointer'),
                    (dict(bt=None), 'null pointer'), (dict(ws=None), 'null pointer'), (dict(cls=18), 'aligned'), (dict(labels=20), 'aligned'),
                    (dict(lw=17), 'aligned'), (dict(bp=24), 'aligned'), (dict(bt=8), 'aligned'), (dict(ws=6), 'aligned')):
        rc, err = accum(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    assert accum(nrows=0, cls=None, labels=None, lw=None, bp=None, bt=None, ws=None)[0] == 0          # no row: nothing to read, no launch

    def update(acc=16, d=16, C=20, mom=0.99):
        return lib.aod_class_difficulty_update(acc, d, C, mom, None), lib.aod_last_error().decode()
    for kw, msg in ((dict(C=0), 'C must be in 1..128'), (dict(C=129), 'C must be in 1..128'), (dict(mom=1.01), 'momentum must be in'),
                    (dict(mom=-0.5), 'momentum must be in'), (dict(mom=float('nan')), 'momentum must be in'), (dict(acc=None), 'null pointer'),
                    (dict(d=None), 'null pointer'), (dict(acc=18), 'aligned'), (dict(d=2), 'aligned')):
        rc, err = update(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    # the weighted entry keeps the checks of aod_det_uncertainty_ex and adds the alignment of class_w
    rc = lib.aod_det_uncertainty_w(16, 16, 16, 16, 16, 2, 10, 21, 8, 3, 0, 0, 0.3, 16, None, None, None, 16, None)
    assert rc != 0 and 'layout 3' in lib.aod_last_error().decode()
    rc = lib.aod_det_uncertainty_w(16, 16, 16, 16, 16, 2, 10, 21, 8, 0, 0, 0, 0.3, 16, None, None, None, 18, None)
    assert rc != 0 and 'aligned' in lib.aod_last_error().decode()
    rc = lib.aod_det_uncertainty_w(None, 16, 16, 16, 16, 2, 10, 21, 8, 0, 0, 0, 0.3, 16, None, None, None, 16, None)
    assert rc != 0 and 'null pointer' in lib.aod_last_error().decode()


def test_wrappers_refuse_bad_arguments_before_a_launch():
    from types import SimpleNamespace
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    n, C = 6, 20
    ok = dict(cls=torch.zeros(n, C), labels=torch.zeros(n, dtype=torch.int64), label_w=torch.ones(n), bbox_pred=torch.zeros(n, 4),
              bbox_tgt=torch.zeros(n, 4), acc=torch.zeros(2 * C))
    for kw, msg in ((dict(form='softmax'), 'unknown form'), (dict(xi=1.2), 'xi must be in'), (dict(xi=float('nan')), 'xi must be in'),
                    (dict(wh_ratio_clip=0), 'wh_ratio_clip'), (dict(means=(0, 0, 0)), 'four finite'), (dict(stds=(1, 1, 1, float('nan'))), 'four finite'),
                    (dict(cls=torch.zeros(n, C, dtype=torch.float64)), '2-D fp32'), (dict(cls=torch.zeros(n * C)), '2-D fp32'),
                    (dict(cls=torch.zeros(n, 129)), '1..128 classes'), (dict(cls=torch.zeros(C, n).t()), 'not contiguous'),
                    (dict(labels=torch.zeros(n, dtype=torch.int32)), 'labels must be'), (dict(labels=torch.zeros(n + 1, dtype=torch.int64)), 'labels must be'),
                    (dict(label_w=torch.ones(n + 1)), 'label_w must be'), (dict(bbox_pred=torch.zeros(n, 5)), 'bbox_pred must be'),
                    (dict(bbox_tgt=torch.zeros(n, 4, dtype=torch.float16)), 'bbox_tgt must be'), (dict(acc=torch.zeros(C)), 'acc must be'),
                    (dict(bbox_pred=torch.zeros(4, n).t()), 'not contiguous')):
        with pytest.raises(ValueError, match=msg):
            ho.class_difficulty_accum(**dict(ok, **kw))
    with pytest.raises(AodHipError, match='CPU tensor'):
        ho.class_difficulty_accum(**ok)
    for kw, msg in ((dict(momentum=1.5), 'momentum must be in'), (dict(momentum=float('nan')), 'momentum must be in'),
                    (dict(d=torch.ones(129)), '1..128 classes'), (dict(d=torch.ones(C, dtype=torch.float64)), '1..128 classes'),
                    (dict(acc=torch.zeros(C)), 'acc must be')):
        with pytest.raises(ValueError, match=msg):
            ho.class_difficulty_update(**dict(dict(acc=torch.zeros(2 * C), d=torch.ones(C)), **kw))
    with pytest.raises(AodHipError, match='CPU tensor'):
        ho.class_difficulty_update(torch.zeros(2 * C), torch.ones(C))
    # det_uncertainty: class_w is checked with the other operands, before the device check
    cand = SimpleNamespace(boxes=torch.zeros(1, 4, 4), scores=torch.zeros(1, 4, 21))
    dets, labels, num = torch.zeros(1, 5, 5), torch.zeros(1, 5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    for w, msg in ((torch.ones(20), 'one weight per column'), (torch.ones(21, dtype=torch.float64), 'one weight per column'),
                   (torch.ones(42)[::2], 'not contiguous')):
        with pytest.raises(ValueError, match=msg):
            scoring.det_uncertainty(cand, dets, labels, num, 'cat', class_w=w)
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.det_uncertainty(cand, dets, labels, num, 'cat', class_w=torch.ones(21))


# ---------------------------------------------------------------------------------------------------------------- heads
@pytest.mark.parametrize('config', ['configs/_base_/Config_RetinaNet.py', 'configs/_base_/Config_RetinaNet_plain.py'])
def test_state_dict_keys_and_checkpoints(config):
    plain, tracked = _head(config), _head(config, class_difficulty=CD)
    assert plain.class_difficulty_cfg is None and not hasattr(plain, 'class_difficulty') and not hasattr(plain, 'class_weight')
    assert [n for n, _ in plain.named_buffers()] == []                       # the default head: no buffer of any kind
    assert set(tracked.state_dict()) - set(plain.state_dict()) == {'class_difficulty', 'class_weight'}
    assert set(plain.state_dict()) <= set(tracked.state_dict())
    assert sorted(n for n, _ in tracked.named_buffers()) == ['_class_difficulty_acc', 'class_difficulty', 'class_weight']
    C = tracked.cls_out_channels
    assert tracked.class_difficulty.shape == (C,) and tracked.class_weight.shape == (C + 1,) and tracked._class_difficulty_acc.shape == (2 * C,)
    assert tracked.class_difficulty_cfg == CD
    # a checkpoint without the keys: the ones stay, one warning however often it is loaded
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        tracked.load_state_dict(plain.state_dict(), strict=True)
        tracked.load_state_dict(plain.state_dict(), strict=True)
    assert sum('class_difficulty' in str(w.message) for w in rec) == 1
    assert tracked.class_difficulty.tolist() == [1.0] * C
    # a checkpoint with them: restored
    other = _head(config, class_difficulty=CD)
    other.class_difficulty.copy_(torch.linspace(0.1, 0.9, C))
    other.refresh_class_weight()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        tracked.load_state_dict(other.state_dict(), strict=True)
    assert torch.equal(tracked.class_difficulty, other.class_difficulty) and torch.equal(tracked.class_weight, other.class_weight)
    # eval mode or a head without the option: nothing is enqueued (CPU tensors would raise)
    tracked.eval()
    tracked._track_class_difficulty(torch.zeros(4, C), torch.zeros(4, dtype=torch.int64), torch.ones(4), torch.zeros(4, 4), torch.zeros(4, 4))
    plain._track_class_difficulty(torch.zeros(4, C), torch.zeros(4, dtype=torch.int64), torch.ones(4), torch.zeros(4, 4), torch.zeros(4, 4))
    plain._step_class_difficulty(), tracked._step_class_difficulty()


def test_option_is_validated_and_ssd_is_a_follow_up():
    for bad, msg in ((dict(CD, xi=1.5), 'xi and momentum'), (dict(CD, momentum=-1), 'xi and momentum'), (dict(CD, alpha=0), 'alpha must be positive'),
                     (dict(CD, gamma=2.0), 'unknown keys')):
        with pytest.raises(ValueError, match=msg):
            _head(class_difficulty=bad)
    assert _head(class_difficulty={}).class_difficulty_cfg == CD              # the defaults are PPAL's constants
    with pytest.raises(NotImplementedError, match='follow-up'):
        _head('configs/_base_/Config_SSD.py', class_difficulty=CD)
    # class_weighted on a head without the option: refused by name, with the way to enable it; the SSD head: a follow-up
    from aod_meh_hua_amd import scoring
    with pytest.raises(ValueError, match='bbox_head.class_difficulty=dict'):
        scoring.score_batch(_head(), [], [], [], [], [], None, class_weighted=True)
    with pytest.raises(NotImplementedError, match='follow-up'):
        scoring.score_batch(_head('configs/_base_/Config_SSD.py'), [], [], [], [], [], None, class_weighted=True)
    with pytest.raises(ValueError, match='tracks no class difficulty'):
        _head().refresh_class_weight()


class _Loader:
    batch_size = 2
    dataset = [0] * 4
    collate_fn = None


def test_pools_by_name():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis.test import Uncertainty_fns, _option_key
    from aod_meh_hua_amd.models import build_detector
    cfg = _cfg()
    model = build_detector(cfg.model)
    cfg.uncertainty_pool = 'PPAL'
    with pytest.raises(TypeError, match='X_L'):
        Uncertainty_fns.PPAL(cfg, model, _Loader())
    with pytest.raises(TypeError, match='X_L'):
        apis.calculate_uncertainty(cfg, model, _Loader(), score_thr=0.3, clsW=False)
    # a detector without the option: refused before a batch is read
    with pytest.raises(ValueError, match='bbox_head.class_difficulty=dict'):
        apis.CCMS_uncertainty(cfg, model, _Loader(), X_L=[0], budget=1, class_weighted=True)
    with pytest.raises(ValueError, match='bbox_head.class_difficulty=dict'):
        apis.Posterior_uncertainty(cfg, model, _Loader(), class_weighted=True)
    with pytest.raises(ValueError, match='bbox_head.class_difficulty=dict'):
        Uncertainty_fns.PPAL(cfg, model, _Loader(), X_L=[0], budget=1)
    ssd = build_detector(_cfg('configs/_base_/Config_SSD.py').model)
    with pytest.raises(NotImplementedError, match='follow-up'):
        apis.Posterior_uncertainty(cfg, ssd, _Loader(), class_weighted=True)
    import inspect
    assert inspect.signature(apis.Posterior_uncertainty).parameters['class_weighted'].default is False
    assert inspect.signature(apis.CCMS_uncertainty).parameters['class_weighted'].default is False
    assert 'sync_class_difficulty' in apis.__all__
    # the option is a hashable part of the scoring graph's key, and absent from it when off
    on, off = _option_key(dict(uPool='Entropy', class_weighted=True)), _option_key(dict(uPool='Entropy'))
    assert on is not None and on != off and ('class_weighted', 'bool', True) in on


def test_the_driver_flags(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_difficulty', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'PPAL', '--synthetic', '8'])
    args = drv.parse_args()
    assert args.uncertainty_pool == 'PPAL' and args.class_difficulty is False and args.candidate_factor == 4.0
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'Entropy', '--class-difficulty'])
    assert drv.parse_args().class_difficulty is True
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py'])
    assert drv.parse_args().class_difficulty is False
    assert drv.CLASS_DIFFICULTY == CD
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--help'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    out = capsys.readouterr().out
    assert 'PPAL' in out and '--class-difficulty' in out
    src = open(os.path.join(ROOT, 'tools', 'train_RetinaNet.py')).read()
    assert "cfg.uncertainty_pool == 'PPAL'" in src and 'cfg.model.bbox_head.class_difficulty = dict(CLASS_DIFFICULTY)' in src
    assert 'zeroRate=0 if coreset else zeroRate' in src
    # the config key builds a tracking head
    cfg = _cfg()
    cfg.model.bbox_head.class_difficulty = dict(drv.CLASS_DIFFICULTY)
    from aod_meh_hua_amd.models.builder import build_head
    head = build_head(dict(cfg.model.bbox_head, train_cfg=cfg.model.train_cfg, test_cfg=cfg.model.test_cfg))
    assert head.class_difficulty_cfg == CD


# ---------------------------------------------------------------------------------------------------------------- two ranks
def _worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from aod_meh_hua_amd.apis import sync_class_difficulty
    head = _head(class_difficulty=CD)
    with torch.no_grad():
        head.class_difficulty.copy_(torch.linspace(0.1, 0.9, 20) if rank == 0 else torch.full((20,), 0.5))      # each rank's own EMA
    stale = head.class_weight.clone()
    sync_class_difficulty(_Holder(head))
    q.put((rank, head.class_difficulty.tolist(), head.class_weight.tolist(), stale.tolist()))
    dist.destroy_process_group()


class _Holder(torch.nn.Module):
    def __init__(self, head):
        super().__init__()
        self.bbox_head = head


def test_two_ranks_end_with_rank_zeros_difficulty():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 977) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = torch.linspace(0.1, 0.9, 20)
    for rank, d, w, stale in res:
        assert d == want.tolist()                                   # rank 0's vector on every rank
        assert np.abs(np.array(w[:20]) - U.class_weight64(want.numpy())).max() < 4 * 2.0 ** -23 and w[20] == 1.0 and w != stale
    assert res[0][2] == res[1][2]                                   # ... and the same weights
