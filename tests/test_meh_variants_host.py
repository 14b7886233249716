"""CPU tests (no GPU) of the MEH ablation heads: the four registry names build from the RetinaNet config with only `type` swapped and share
Lambda_L2Net's state_dict keys, the float64 restatement of the three loss forms reproduces what the reference recorded
(tests/golden/meh_variants.npz) within the recorded e_ref, the pool entry Entropy_Avg exists and is refused by a head whose reference has
no such branch, and the new C-ABI entry points are declared and exported."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.meh_variants_util import FORMS, LOSS_LEVELS, meh_loss_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'meh_variants.npz')
NAMES = ('Lambda_L1Net', 'Lambda_MSLENet', 'Lambda_L2Net_NoL', 'Lambda_L2Net_ablation')
NEW_SYMBOLS = ('aod_meh_loss_fwd_ex', 'aod_meh_loss_bwd_ex', 'aod_meh_loss_levels_fwd_ex', 'aod_meh_loss_levels_bwd_ex', 'aod_hua_score_ex2')


def _head(name):
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_head
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    hc = dict(cfg.model.bbox_head)
    hc['type'] = name
    return build_head(dict(hc, train_cfg=cfg.model.train_cfg, test_cfg=cfg.model.test_cfg))


@pytest.mark.parametrize('name', NAMES)
def test_ablation_heads_build_with_only_the_type_swapped(name):
    base, head = _head('Lambda_L2Net'), _head(name)
    assert type(head).__name__ == name and isinstance(head, type(base))
    sd, sb = head.state_dict(), base.state_dict()
    assert list(sd.keys()) == list(sb.keys()) and all(sd[k].shape == sb[k].shape for k in sb)
    base.load_state_dict(sd, strict=True)                    # a checkpoint of one loads into another
    attrs = {k: getattr(head, k) for k in ('_meh_form', '_hua_lam', '_hua_thr_kwargs', '_hua_entropy_avg')}
    assert attrs == {'Lambda_L1Net': dict(_meh_form='l1', _hua_lam='scaled', _hua_thr_kwargs=False, _hua_entropy_avg=False),
                     'Lambda_MSLENet': dict(_meh_form='msle', _hua_lam='scaled', _hua_thr_kwargs=False, _hua_entropy_avg=False),
                     'Lambda_L2Net_ablation': dict(_meh_form='l2', _hua_lam='scaled', _hua_thr_kwargs=True, _hua_entropy_avg=False),
                     'Lambda_L2Net_NoL': dict(_meh_form='l2', _hua_lam='none', _hua_thr_kwargs=True, _hua_entropy_avg=True)}[name]


def test_default_head_attributes_are_the_unchanged_behaviour():
    from aod_meh_hua_amd.models import Lambda_L2Net
    assert (Lambda_L2Net._meh_form, Lambda_L2Net._hua_lam, Lambda_L2Net._hua_thr_kwargs, Lambda_L2Net._hua_entropy_avg) == ('l2', 'scaled', False, False)


@pytest.mark.parametrize('form', FORMS)
def test_float64_restatement_reproduces_the_reference_within_e_ref(form):
    g = np.load(GOLD)
    e_val, e_grad = float(g[f'{form}_e_val']), float(g[f'{form}_e_grad'])
    assert 0 < e_val < 1e-6 and 0 < e_grad < 1e-7            # float32 rounding of O(1) values / O(1e-1) gradients
    for l in range(len(LOSS_LEVELS)):
        v, gr = meh_loss_float64(form, g[f'loss_lam{l}'], g[f'loss_prev{l}'], g[f'loss_w{l}'])
        assert v == g[f'{form}_val64'][l] and np.array_equal(gr, g[f'{form}_grad64_{l}'])
        assert abs(v - float(g[f'{form}_val'][l])) <= e_val
        assert np.abs(gr - g[f'{form}_grad{l}'].astype(np.float64)).max() <= e_grad


def test_fixture_holds_the_cases_the_loss_kernels_can_get_wrong():
    g = np.load(GOLD)
    ties = zeros = 0
    for l, (h, w) in enumerate(LOSS_LEVELS):
        lam = np.transpose(g[f'loss_lam{l}'], (0, 2, 3, 1)).reshape(-1)
        prev, wt, tie = g[f'loss_prev{l}'], g[f'loss_w{l}'], g[f'loss_tie{l}']
        assert lam.size == 2 * 9 * h * w and (prev >= 0).all() and set(np.unique(wt)) == {0, 1}
        assert np.array_equal(tie, (lam + np.float32(1e-9)) == prev)
        assert np.array_equal(lam, np.round(lam * 1024) / 1024) and 0.3 < (lam == 0).mean() < 0.7
        ties += int(tie.sum())
        zeros += int(((lam == 0) & (prev == 0)).sum())
        gl1 = np.transpose(g[f'l1_grad{l}'], (0, 2, 3, 1)).reshape(-1)
        assert (gl1[tie] == 0).all() and (gl1[wt == 0] == 0).all() and (gl1[(wt == 1) & ~tie] != 0).all()
    assert ties >= 8 and zeros >= 8
    # scoring: the thresholds change the pair lists, and Entropy_Avg sees a level without foreground rows next to levels with some
    assert not np.array_equal(g['nol_030_050_pairs0'], g['nol_030_090_pairs0'])
    assert not np.array_equal(g['abl_030_090_pairs1'], g['abl_050_050_pairs1'])
    fc = g['nol_avg_fg_counts']
    assert (fc == 0).any(1).any() and (fc > 0).any(1).all()
    assert os.path.getsize(GOLD) <= 150 * 1024


def test_entropy_avg_pool_entry_exists_and_is_refused_by_a_head_without_it():
    from aod_meh_hua_amd.apis.test import Uncertainty_fns
    from aod_meh_hua_amd import scoring
    assert callable(Uncertainty_fns.Entropy_Avg)
    head = _head('Lambda_L2Net')
    with pytest.raises(NotImplementedError, match='Lambda_L2Net'):
        scoring.score_batch(head, [torch.zeros(1, 180, 2, 2)], [torch.zeros(1, 36, 2, 2)], [torch.zeros(36, 4)], [(16, 16, 3)], [np.ones(4)],
                            head.test_cfg, isUnc='Epistemic', uPool='Entropy_Avg', uPool2='objectSum_scaleMax_classSum', isEval=False,
                            L_scores=[torch.zeros(1, 9, 2, 2)])
    with pytest.raises(ValueError, match='lam_mode'):
        scoring.hua_score(None, None, None, None, 100, lam_mode='x')
    with pytest.raises(ValueError, match='scale_mode'):
        scoring.hua_score(None, None, None, None, 100, scale_mode='sum')


def test_new_entry_points_are_declared_and_exported():
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'aod_hip.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, f'{name} is not declared in include/aod_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        old = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % (name[:-3] if name.endswith('_ex') else 'aod_hua_score_ex'), hdr)
        assert m.group(1).count(',') == old.group(1).count(',') + 1          # one new argument each: form / lam_mode
        assert re.search(r'\bint\s+(form|lam_mode)\b', m.group(1)) and not re.search(r'\b(form|lam_mode)\b', old.group(1))
        assert len(_C._SIGS[name][1]) == m.group(1).count(',') + 1
    # argument checks run on the host before any launch
    lib.aod_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    lib.aod_meh_loss_fwd_ex.argtypes = _C._SIGS['aod_meh_loss_fwd_ex'][1]
    assert lib.aod_meh_loss_fwd_ex(P, P, P, 4, 3, P, P, None) != 0 and b'form' in lib.aod_last_error()
    lib.aod_hua_score_ex2.argtypes = _C._SIGS['aod_hua_score_ex2'][1]
    ls = (ctypes.c_int32 * 2)(0, 4)
    go = lambda scale_mode, lam_mode: lib.aod_hua_score_ex2(P, P, P, P, P, P, ls, P, P, 1, 4, 1, 20, 2, 0.3, 0.5, 0.3, 50, 20, None, 0, scale_mode,
                                                            0, P, None, 8, P, 0, lam_mode, None, None, P, None)
    assert go(0, 2) != 0 and b'lam_mode' in lib.aod_last_error()
    assert go(3, 0) != 0 and b'scale_mode' in lib.aod_last_error()
