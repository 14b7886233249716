"""CPU tests (no GPU) of the ensemble mutual-information acquisition: the float64 restatement the GPU tests compare against reproduces the
reference's recorded outputs (tests/golden/ensemble_mi.npz, tools/golden/make_golden_ensemble.py), the C entry point is declared,
exported and validates its arguments before any launch, and the Python layers refuse what they cannot score."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.ensemble_mi_util import CASES, GOLDEN, LEVELS, bound, load_case, mi_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    lib.aod_ensemble_mi.restype = ctypes.c_int
    lib.aod_ensemble_mi.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.aod_ensemble_mi_partials_len.restype = ctypes.c_size_t
    lib.aod_ensemble_mi_partials_len.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    return lib


@pytest.mark.parametrize('case', CASES)
def test_float64_restatement_reproduces_the_reference(golden, case):
    members, ref, e_ref, total_mean = load_case(golden, case)
    assert len(members) == (5 if case.endswith('k5') else 3) and len(members[0]) == len(LEVELS)
    for l, (h, w) in enumerate(LEVELS):
        assert members[0][l].shape == (3, 40, h, w) and members[0][l].dtype == np.float32
    got, tm = mi_float64(members, 20)
    assert np.isfinite(ref).all() and ref.shape == (3,)
    assert np.abs(got - ref.astype(np.float64)).max() <= e_ref
    assert tm == pytest.approx(total_mean, rel=1e-12)
    # the recorded error is an fp32 rounding error, not a disagreement about the formula: a few ulp of the `total` mean
    assert 0 < e_ref < 16 * 2.0 ** -24 * total_mean
    assert bound(e_ref, total_mean) < 1e-5 * np.abs(ref).min()


def test_saturated_case_is_saturated_and_prior_case_is_the_prior(golden):
    sat = np.concatenate([golden[f'saturated_k3_x{l}'].ravel() for l in range(3)])
    pri = np.concatenate([golden[f'prior_k3_x{l}'].ravel() for l in range(3)])
    assert sat.min() < -25 and sat.max() > 25 and np.abs(sat).max() <= 30
    assert abs(pri.mean() + 4.6) < 0.1 and abs(pri.std() - 2.0) < 0.1


def test_entry_point_is_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'CalEnsembleUnc.py:164-180' in hdr and 'CalMCDropoutUnc.py:183-199' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+aod_ensemble_mi\s*\(', hdr) and re.search(r'\bsize_t\s+aod_ensemble_mi_partials_len\s*\(', hdr)
    assert hasattr(lib, 'aod_ensemble_mi') and hasattr(lib, 'aod_ensemble_mi_partials_len')
    from aod_meh_hua_amd import _C
    assert 'aod_ensemble_mi' in _C._SIGS and len(_C._SIGS['aod_ensemble_mi'][1]) == 10


def _call(lib, K=3, L=2, B=2, n_cls=20, n=(4000, 40), maps='ok', out=16, ws=16, cap=1 << 20, sizes='ok'):
    one = 16
    arr = None
    if maps == 'ok':
        arr = (ctypes.c_void_p * max(K * L, 1))(*([one] * max(K * L, 1)))
    elif maps == 'hole':
        arr = (ctypes.c_void_p * (K * L))(*([one] * (K * L - 1) + [None]))
    sz = (ctypes.c_int64 * max(L, 1))(*(list(n) + [n[-1]] * 8)[:max(L, 1)]) if sizes == 'ok' else None
    return lib.aod_ensemble_mi(arr, K, L, sz, B, n_cls, out, ws, cap, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(K=1), b'2..32 members'), (dict(K=33), b'2..32 members'), (dict(L=0), b'1..8 levels'), (dict(L=9), b'1..8 levels'),
    (dict(B=0), b'batch'), (dict(n_cls=0), b'n_cls'), (dict(maps=None), b'null pointer'), (dict(maps='hole'), b'null map pointer'),
    (dict(out=None), b'null pointer'), (dict(ws=None), b'null pointer'), (dict(sizes=None), b'null level sizes'),
    (dict(n=(4001, 40)), b'multiple of n_cls'),
])
def test_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    """validation precedes every launch: this machine has no GPU, a launch attempt would fail differently (-3) or crash"""
    assert _call(lib, **kw) == -1
    assert msg in lib.aod_last_error()


def test_workspace_is_counted_per_fixed_chunk_and_checked(lib):
    n = (ctypes.c_int64 * 3)(4096, 4097, 40)
    per_image = 1 + 2 + 1                       # one partial per chunk of 4096 elements: the count depends on n_l only
    assert lib.aod_ensemble_mi_partials_len(3, n, 1) == per_image
    assert lib.aod_ensemble_mi_partials_len(3, n, 5) == 5 * per_image
    assert lib.aod_ensemble_mi_partials_len(9, n, 5) == 0
    assert _call(lib, L=3, B=5, n=(4096, 4097, 40), n_cls=1, cap=5 * per_image - 1) == -2
    assert b'workspace too small' in lib.aod_last_error()


def test_public_names_are_importable():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import Ensemble_uncertainty, single_gpu_ensemble      # noqa: F401
    assert 'Ensemble_uncertainty' in apis.__all__ and callable(Ensemble_uncertainty)
    with pytest.raises(TypeError, match='data loader'):
        Ensemble_uncertainty(None)
    with pytest.raises(TypeError, match='pool loader'):
        Ensemble_uncertainty(None, torch.nn.Linear(1, 1), torch.nn.Linear(1, 1))


def test_scoring_ensemble_mi_refuses_what_it_cannot_score(golden):
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    members = [[torch.from_numpy(t) for t in m] for m in load_case(golden, 'prior_k3')[0]]
    with pytest.raises(AodHipError, match='CPU tensor'):
        scoring.ensemble_mi(members, 20)
    with pytest.raises(ValueError, match='2..32 members'):
        scoring.ensemble_mi(members[:1], 20)
    with pytest.raises(ValueError, match='2..32 members'):
        scoring.ensemble_mi(members * 11, 20)
    bad = [members[0], members[1][:2] + [members[1][2][:, :, :, :1]], members[2]]
    with pytest.raises(ValueError, match='member 1 level 2 has shape'):
        scoring.ensemble_mi(bad, 20)
    with pytest.raises(ValueError, match='levels'):
        scoring.ensemble_mi([members[0], members[1][:2]], 20)
    with pytest.raises(ValueError, match='not an fp32 tensor'):
        scoring.ensemble_mi([members[0], [t.double() for t in members[1]]], 20)
    with pytest.raises(ValueError, match='multiple of n_cls'):
        scoring.ensemble_mi(members, 21)


def test_scores_select_the_top_images_through_update_X_L(golden):
    """host logic only: the [N] score tensor is what utils.active_datasets.update_X_L takes"""
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    scores = np.concatenate([mi_float64(load_case(golden, c)[0], 20)[0] for c in CASES])        # 9 'images'
    unc = torch.tensor(scores, dtype=torch.float32)
    X_all, X_L = np.arange(9), np.array([6, 0])           # image 6 (a saturated-case top scorer) is labelled already
    np.random.seed(3)
    X_L_next, X_U_next = update_X_L(unc, X_all, X_L, 3)
    pool = np.array([i for i in X_all if i not in X_L])
    want = pool[np.argsort(scores[pool])[-3:]]
    assert sorted(X_L_next.tolist()) == sorted(X_L.tolist() + want.tolist())
    assert set(want.tolist()) == {3, 7, 8}                # the two remaining saturated images and the best of the K = 5 case
    assert not set(X_U_next.tolist()) & set(X_L_next.tolist())
