"""CPU tests (no GPU) of the localization-stability pool: the float64 restatement of tests/loc_stability_util.py on hand cases,
the argument checks of hipops.pixel_noise, scoring.loc_stability, apis.single_gpu_loc_stability and of the two C entries (all before any
launch), the pool names in Uncertainty_fns / apis.__all__, and the drivers' parser."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import loc_stability_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the restatement by hand
def _slots(K, B=2, max_num=3):
    dets = np.zeros((K + 1, B, max_num, 5), np.float32)
    labels = np.zeros((K + 1, B, max_num), np.int64)
    num = np.zeros((K + 1, B), np.int32)
    return dets, labels, num


def test_identical_slots_are_perfectly_stable():
    dets, labels, num = _slots(3)
    ref = np.array([[[2, 3, 30, 40, .9], [5, 5, 9, 25, .5], [0, 0, 4, 4, .2]], [[1, 1, 8, 8, .31], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]], np.float32)
    dets[:] = ref[None]
    num[:] = np.array([3, 1], np.int32)[None]
    r = U.reference(dets, labels, num)
    assert r['count'].tolist() == [2, 1] and r['unc'].tolist() == [0.0, 0.0]
    assert r['stab'][0, :2].tolist() == [1.0, 1.0] and np.isnan(r['stab'][0, 2]) and r['stab'][1, 0] == 1.0 and np.isnan(r['stab'][1, 1:]).all()
    c = U.reference(dets, labels, num, combine='ls+c')
    assert np.allclose(c['unc'], [1 - np.float64(np.float32(.9)), 1 - np.float64(np.float32(.31))], rtol=1e-15)


def test_empty_noisy_slots_no_object_and_the_strict_gate():
    dets, labels, num = _slots(2)
    dets[0, 0, 0] = [0, 0, 10, 10, .8]
    dets[0, 1, 0] = [0, 0, 10, 10, np.float32(.3)]                    # exactly the threshold: no object
    num[0] = [1, 1]
    r = U.reference(dets, labels, num)
    assert r['unc'].tolist() == [1.0, 0.0] and r['count'].tolist() == [1, 0] and r['stab'][0, 0] == 0.0
    below = float(np.nextafter(np.float32(.3), np.float32(0)))
    assert U.reference(dets, labels, num, score_thr=below)['count'].tolist() == [1, 1]
    # rows >= num are never read
    dets[1:, :, :, :] = np.nan
    assert U.reference(dets, labels, num)['unc'].tolist() == [1.0, 0.0]
    num[0] = [0, 0]
    assert U.reference(dets, labels, num)['unc'].tolist() == [0.0, 0.0]


def test_weighted_mean_levels_same_class_and_ls_plus_c():
    dets, labels, num = _slots(2, B=1, max_num=2)
    dets[0, 0] = [[0, 0, 10, 10, .75], [20, 20, 30, 40, .5]]
    labels[0, 0] = [1, 2]
    # level 0: box 0 shifted by 5 in x (IoU 50 / 150), box 1 unchanged but of another class; level 1: box 0 halved, box 1 gone
    dets[1, 0] = [[5, 0, 15, 10, .7], [20, 20, 30, 40, .5]]
    labels[1, 0] = [1, 3]
    dets[2, 0] = [[0, 0, 10, 5, .6], [0, 0, 0, 0, 0]]
    labels[2, 0] = [1, 0]
    num[:, 0] = [2, 2, 1]
    r = U.reference(dets, labels, num)
    s0, s1 = (1 / 3 + .5) / 2, (1 + 0) / 2
    assert np.allclose(r['stab'][0], [s0, s1], rtol=1e-15)
    s_img = (.75 * s0 + .5 * s1) / 1.25
    assert np.isclose(r['unc'][0], 1 - s_img, rtol=1e-14)
    rs = U.reference(dets, labels, num, same_class=True)
    assert np.allclose(rs['stab'][0], [s0, 0.0], rtol=1e-15) and np.isclose(rs['unc'][0], 1 - .75 * s0 / 1.25, rtol=1e-14)
    rc = U.reference(dets, labels, num, combine='ls+c')
    assert np.isclose(rc['unc'][0], r['unc'][0] + 1 - .75, rtol=1e-14)
    assert U.iou64([0, 0, 0, 0], [0, 0, 0, 0]) == 0.0                  # the clamped union
    assert U.bound(100, 6) == 138 * 2.0 ** -23


def test_noise_restatement_is_keyed_by_pixel_not_by_window():
    a = U.noise_z64(7, 1, (1 << 33) + 5, 2, 8, 16)
    b = U.noise_z64(7, 1, (1 << 33) + 5, 2, 5, 7)
    assert a.shape == (8, 16) and np.array_equal(a[:5, :7], b)
    for other in (U.noise_z64(8, 1, (1 << 33) + 5, 2, 8, 16), U.noise_z64(7, 2, (1 << 33) + 5, 2, 8, 16), U.noise_z64(7, 1, 5, 2, 8, 16),
                  U.noise_z64(7, 1, (1 << 33) + 5, 1, 8, 16)):
        assert not np.array_equal(a, other)
    z = U.noise_z64(0, 0, 3, 0, 256, 256)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    src = np.ones((1, 1, 4, 8), np.float32)
    out, live = U.noisy64(src, [(3, 5)], [2.0], 8.0, 0, 0, [3])
    assert live.sum() == 15 and np.array_equal(out[~live], src[~live].astype(np.float64))
    assert np.allclose(out[0, 0, :3, :5], 1 + 4.0 * z[:3, :5], rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- wrappers
def _stack(K=2, B=2, max_num=4):
    return (torch.zeros(K + 1, B, max_num, 5), torch.zeros(K + 1, B, max_num, dtype=torch.int64), torch.zeros(K + 1, B, dtype=torch.int32))


def test_loc_stability_wrapper_refuses_before_any_launch():
    from aod_meh_hua_amd import _C, scoring
    d, l, n = _stack()
    with pytest.raises(ValueError, match='unknown combine'):
        scoring.loc_stability(d, l, n, combine='lsc')
    with pytest.raises(ValueError, match='score_thr is NaN'):
        scoring.loc_stability(d, l, n, score_thr=float('nan'))
    for K in (0, 17):
        with pytest.raises(ValueError, match='noise levels'):
            scoring.loc_stability(*_stack(K=K))
    for max_num in (0, 1025):
        with pytest.raises(ValueError, match='max_num'):
            scoring.loc_stability(*_stack(max_num=max_num))
    with pytest.raises(ValueError, match='labels has shape'):
        scoring.loc_stability(d, l[:, :, :3].contiguous(), n)
    with pytest.raises(ValueError, match='num has shape'):
        scoring.loc_stability(d, l, n[:2].contiguous())
    with pytest.raises(ValueError, match='4-D float32'):
        scoring.loc_stability(d.double(), l, n)
    with pytest.raises(ValueError, match='not contiguous'):
        scoring.loc_stability(d.transpose(1, 2), l, n)
    with pytest.raises(_C.AodHipError, match='no CPU fallback'):
        scoring.loc_stability(d, l, n)
    assert scoring.LOCSTAB_SIGMAS == (8, 16, 24, 32, 40, 48) and scoring.LOCSTAB_COMBINES == {'ls': 0, 'ls+c': 1}


def test_pixel_noise_wrapper_refuses_before_any_launch():
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd import hipops as ho
    src, dst = torch.zeros(2, 3, 8, 16), torch.zeros(2, 3, 8, 16)
    hw, ids, inv = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match='out of place'):
        ho.pixel_noise(src, src, hw, inv, 8.0, 0, 0, ids)
    with pytest.raises(ValueError, match='out of place'):
        buf = torch.zeros(3, 3, 8, 16)
        ho.pixel_noise(buf[:2], buf[1:], hw, inv, 8.0, 0, 0, ids)
    with pytest.raises(ValueError, match='Wp % 4'):
        ho.pixel_noise(torch.zeros(2, 3, 8, 14), torch.zeros(2, 3, 8, 14), hw, inv, 8.0, 0, 0, ids)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='sigma must be finite'):
            ho.pixel_noise(src, dst, hw, inv, bad, 0, 0, ids)
    for level in (-1, 16):
        with pytest.raises(ValueError, match='level must be in'):
            ho.pixel_noise(src, dst, hw, inv, 8.0, level, 0, ids)
    with pytest.raises(ValueError, match='inv_std'):
        ho.pixel_noise(src, dst, hw, [1.0, 1.0], 8.0, 0, 0, ids)
    with pytest.raises(ValueError, match='1..4 channels'):
        ho.pixel_noise(torch.zeros(2, 5, 8, 16), torch.zeros(2, 5, 8, 16), hw, [1.0] * 5, 8.0, 0, 0, ids)
    with pytest.raises(ValueError, match='hw must be'):
        ho.pixel_noise(src, dst, hw.float(), inv, 8.0, 0, 0, ids)
    with pytest.raises(ValueError, match='image_ids must be'):
        ho.pixel_noise(src, dst, hw, inv, 8.0, 0, 0, ids.int())
    with pytest.raises(_C.AodHipError, match='no CPU fallback'):
        ho.pixel_noise(src, dst, hw, inv, 8.0, 0, 0, ids)


def test_pool_pass_refuses_bad_options_and_differing_std():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as T
    for sig in ((), tuple(range(17)), (8, -1), (8, float('nan')), (float('inf'),), 8):
        with pytest.raises(ValueError, match='noise level'):
            apis.single_gpu_loc_stability(None, None, sigmas=sig)
    with pytest.raises(ValueError, match='unknown combine'):
        apis.single_gpu_loc_stability(None, None, combine='c')
    with pytest.raises(ValueError, match='score_thr is NaN'):
        apis.single_gpu_loc_stability(None, None, score_thr=float('nan'))
    a = dict(img_norm_cfg=dict(mean=[1., 2., 3.], std=[58.395, 57.12, 57.375], to_rgb=True))
    b = dict(img_norm_cfg=dict(mean=[1., 2., 3.], std=[1., 1., 1.], to_rgb=True))
    assert T._noise_inv_std([a, dict(a)], 3) == [1 / 58.395, 1 / 57.12, 1 / 57.375]
    assert T._noise_inv_std([{}, {}], 3) == [1.0, 1.0, 1.0]               # not normalised by the pipeline: Collect's default std
    with pytest.raises(ValueError, match='different std'):
        T._noise_inv_std([a, b], 3)
    with pytest.raises(ValueError, match='finite positive'):
        T._noise_inv_std([dict(img_norm_cfg=dict(std=[1., 0., 1.]))], 3)
    with pytest.raises(ValueError, match='finite positive'):
        T._noise_inv_std([a], 1)


def test_pool_names_exist_and_ignore_the_hua_kwargs(monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as T
    assert 'LocStability_uncertainty' in apis.__all__ and 'single_gpu_loc_stability' in apis.__all__
    seen = []
    monkeypatch.setattr(T, 'LocStability_uncertainty', lambda cfg, model, loader, **kw: seen.append(kw) or torch.zeros(3))
    cfg = type('Cfg', (), {})()
    hua = dict(return_box=False, showNMS=False, saveUnc=False, saveMaxConf=False, clsW=False, scaleUnc=False, score_thr=0.25, iou_thr=0.9)
    for name, combine in (('LocStability', 'ls'), ('LocStability_C', 'ls+c')):
        cfg.uncertainty_pool = name
        out = apis.calculate_uncertainty(cfg, 'model', 'loader', sigmas=(4.0, 8.0), seed=5, **hua)
        assert torch.equal(out, torch.zeros(3))
        assert seen[-1] == dict(score_thr=0.25, combine=combine, sigmas=(4.0, 8.0), seed=5)
        apis.calculate_uncertainty(cfg, 'model', 'loader', **dict(hua, score_thr=None), same_class=True)
        assert seen[-1] == dict(score_thr=0.3, combine=combine, same_class=True)


def test_both_drivers_parse_the_new_flags(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_locstab', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.setenv('LOCAL_RANK', '0')
    for config, size in (('configs/_base_/Config_RetinaNet.py', 512), ('configs/_base_/Config_SSD.py', 300)):      # train_SSD.py: main(config, 300)
        monkeypatch.setattr(sys, 'argv', ['drv.py', '--uncertainty-pool', 'LocStability'])
        args = drv.parse_args(config, size)
        assert args.uncertainty_pool == 'LocStability' and args.noise_levels == '8,16,24,32,40,48' and args.noise_seed == 0
        monkeypatch.setattr(sys, 'argv', ['drv.py', '--uncertainty-pool', 'LocStability_C', '--noise-levels', '4,8.5', '--noise-seed', '11'])
        args = drv.parse_args(config, size)
        assert args.uncertainty_pool == 'LocStability_C' and args.noise_levels == '4,8.5' and args.noise_seed == 11 and args.noise_sigmas == (4.0, 8.5)
    for bad in ('8,x', '', '8,-1', '8,nan', '8,inf', ','.join(['1'] * 17)):                    # refused at start-up, not at the first acquisition step
        monkeypatch.setattr(sys, 'argv', ['drv.py', '--noise-levels', bad])
        with pytest.raises(SystemExit):
            drv.parse_args()
    capsys.readouterr()
    monkeypatch.setattr(sys, 'argv', ['drv.py', '--help'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    out = capsys.readouterr().out
    assert all(w in out for w in ('LocStability', 'LocStability_C', '--noise-levels', '--noise-seed', 'Kao'))
    assert 'from train_RetinaNet import main' in open(os.path.join(ROOT, 'tools', 'train_SSD.py')).read()          # SSD shares the parser and the loop


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    P, I32, F32, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_uint64
    lib.aod_pixel_noise.restype = lib.aod_loc_stability.restype = ctypes.c_int
    lib.aod_pixel_noise.argtypes = [P, P, I32, I32, I32, I32, P, P, F32, I32, U64, P, P]
    lib.aod_loc_stability.argtypes = [P, P, P, I32, I32, I32, F32, I32, I32, P, P, P]
    return lib


def test_the_entries_are_declared_exported_and_documented(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'DESIGN 3m' in hdr and 'Kao' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    from aod_meh_hua_amd import _C
    for name, n in (('aod_pixel_noise', 13), ('aod_loc_stability', 12)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr) and hasattr(lib, name) and len(_C._SIGS[name][1]) == n
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read() and name in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3m' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    from aod_meh_hua_amd import scoring
    assert lib.aod_loc_stability_max_levels() == scoring.LOCSTAB_MAX_LEVELS == 16          # written once, in the C source
    assert 'LocStability' in open(os.path.join(ROOT, 'README.md')).read()


def _stab(lib, dets=16, labels=16, num=16, K=6, B=2, max_num=100, thr=0.3, same_class=0, combine=0, unc=16, stab=16):
    return lib.aod_loc_stability(dets, labels, num, K, B, max_num, thr, same_class, combine, unc, stab, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(K=0), b'K must be in 1..16'), (dict(K=17), b'K must be in 1..16'), (dict(max_num=0), b'max_num must be in 1..1024'),
    (dict(max_num=1025), b'max_num must be in 1..1024'), (dict(B=0), b'batch'), (dict(combine=2), b'combine 2'), (dict(combine=-1), b'combine -1'),
    (dict(same_class=2), b'same_class'), (dict(thr=float('nan')), b'score_thr is NaN'), (dict(dets=None), b'null pointer'),
    (dict(labels=None), b'null pointer'), (dict(num=None), b'null pointer'), (dict(unc=None), b'null pointer'), (dict(dets=18), b'aligned'),
    (dict(labels=20), b'aligned'), (dict(stab=6), b'aligned'),
])
def test_loc_stability_entry_rejects_bad_arguments_without_a_gpu(lib, kw, msg):
    """validation precedes the launch: this machine has no GPU, a launch attempt would fail differently (-3) or crash"""
    assert _stab(lib, **kw) == -1
    assert msg in lib.aod_last_error()


def _noise(lib, src=4096, dst=1 << 20, B=2, C=3, Hp=8, Wp=16, hw=16, inv_std=(1.0, 1.0, 1.0, 1.0), sigma=8.0, level=0, seed=0, ids=16):
    inv = (ctypes.c_float * 4)(*inv_std) if inv_std is not None else None
    return lib.aod_pixel_noise(src, dst, B, C, Hp, Wp, hw, inv, sigma, level, seed, ids, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(Wp=18), b'multiple of 4'), (dict(Wp=262148), b'padded width'), (dict(Hp=65537), b'padded height'), (dict(Hp=0), b'padded height'),
    (dict(C=5), b'1..4 channels'), (dict(C=0), b'1..4 channels'), (dict(B=0), b'batch'), (dict(sigma=-1.0), b'sigma must be finite'),
    (dict(sigma=float('nan')), b'sigma must be finite'), (dict(sigma=float('inf')), b'sigma must be finite'), (dict(level=-1), b'level must be'),
    (dict(level=16), b'level must be'), (dict(dst=4096), b'dst == src'), (dict(dst=4096 + 64), b'overlaps'), (dict(src=None), b'null pointer'),
    (dict(dst=None), b'null pointer'), (dict(hw=None), b'null pointer'), (dict(inv_std=None), b'null pointer'), (dict(ids=None), b'null pointer'),
    (dict(inv_std=(1.0, 0.0, 1.0, 1.0)), b'inv_std[1]'), (dict(inv_std=(1.0, 1.0, float('nan'), 1.0)), b'inv_std[2]'), (dict(src=4100), b'aligned'),
    (dict(ids=20), b'aligned'),
])
def test_pixel_noise_entry_rejects_bad_arguments_without_a_gpu(lib, kw, msg):
    assert _noise(lib, **kw) == -1
    assert msg in lib.aod_last_error()
