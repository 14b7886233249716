"""CPU tests (no GPU) of the closed-form HUA estimator / per-detection uncertainty interface: the extended C-ABI entry is declared and
exported, the estimator name is validated before any tensor is touched, and unc2result splits rows exactly as bbox2result does."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    return ctypes.CDLL(build(verbose=False))


def test_hua_score_ex_is_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    m = re.search(r'\bint\s+aod_hua_score_ex\s*\(([^;]*)\)\s*;', hdr)
    assert m, 'aod_hua_score_ex is not declared in include/aod_hip.h'
    args = m.group(1)
    assert re.search(r'\bint\s+estimator\b', args) and re.search(r'float\s*\*\s*obj_out\b', args) and re.search(r'int32_t\s*\*\s*obj_pairs\b', args)
    old = re.search(r'\bint\s+aod_hua_score\s*\(([^;]*)\)\s*;', hdr)
    assert old and 'estimator' not in old.group(1)                       # the old entry keeps its signature
    assert args.count(',') == old.group(1).count(',') + 3
    assert hasattr(lib, 'aod_hua_score_ex') and hasattr(lib, 'aod_hua_score')
    from aod_meh_hua_amd import _C
    assert len(_C._SIGS['aod_hua_score_ex'][1]) == len(_C._SIGS['aod_hua_score'][1]) + 3


def test_bad_estimator_and_half_given_object_outputs_are_rejected_without_a_gpu(lib):
    """argument checks of the new entry run on the host before any launch"""
    lib.aod_hua_score_ex.restype = ctypes.c_int
    from aod_meh_hua_amd import _C
    lib.aod_hua_score_ex.argtypes = _C._SIGS['aod_hua_score_ex'][1]
    lib.aod_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    ls = (ctypes.c_int32 * 2)(0, 4)

    def go(estimator, obj_out, obj_pairs, scale_mode=0):
        return lib.aod_hua_score_ex(P, P, P, P, P, P, ls, P, P, 1, 4, 1, 20, 2, 0.3, 0.5, 0.3, 500, 20, None, 0, scale_mode, 0, P, None, 8, P,
                                    estimator, obj_out, obj_pairs, P, None)
    assert go(2, None, None) != 0 and b'estimator' in lib.aod_last_error()
    assert go(0, P, None) != 0 and b'obj_out' in lib.aod_last_error()
    assert go(1, P, P, scale_mode=1) != 0 and b'scale_mode' in lib.aod_last_error()


def test_unknown_estimator_raises_before_touching_a_tensor():
    from aod_meh_hua_amd import scoring
    with pytest.raises(ValueError, match='estimator'):
        scoring.hua_score(None, None, None, None, 100, estimator='x')
    assert set(scoring.HUA_ESTIMATORS) == {'mc', 'closed'}


def test_unc2result_is_row_aligned_with_bbox2result():
    from aod_meh_hua_amd.core import bbox2result, unc2result
    boxes = np.arange(7 * 5, dtype=np.float32).reshape(7, 5)
    labels = np.array([2, 0, 2, 1, 0, 2, 4])
    unc = np.stack([boxes[:, 4] * 10, -boxes[:, 4]], 1).astype(np.float32)           # each row is a function of its box's score column
    unc[3] = np.nan
    for conv in (lambda a: a, torch.from_numpy):
        br = bbox2result(conv(boxes), conv(labels), 5)
        ur = unc2result(conv(unc), conv(labels), 5)
        assert len(ur) == len(br) == 5
        for c in range(5):
            assert ur[c].shape == (br[c].shape[0], 2) and ur[c].dtype == np.float32
            exp = np.stack([br[c][:, 4] * 10, -br[c][:, 4]], 1)
            ok = ~np.isnan(ur[c][:, 0])
            assert np.array_equal(ur[c][ok], exp[ok])
        assert np.isnan(ur[1]).all() and ur[3].shape == (0, 2)
    empty = unc2result(np.zeros((0, 2), np.float32), np.zeros((0,), np.int64), 5)
    assert len(empty) == 5 and all(a.shape == (0, 2) and a.dtype == np.float32 for a in empty)
    eb = bbox2result(np.zeros((0, 5), np.float32), np.zeros((0,), np.int64), 5)
    assert [a.shape[0] for a in empty] == [a.shape[0] for a in eb]
