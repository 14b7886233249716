"""GPU: the CDAL acquisition -- aod_cdal_descriptor (scoring.cdal_descriptor) and the symmetrised-KL metric of
aod_kcenter_greedy_ex (scoring.kcenter_greedy(metric='symkl')) against the float64 restatements of tests/cdal_util.py, their bit properties,
and the pool pass apis.single_gpu_cdal_descriptors / apis.CDAL_uncertainty (graph replay and eager).

Bounds (derived, not measured):
  descriptor  every sum of the definition is over non-negative terms.  A row's p and w carry a few ulp of relative error (expf, log1pf, one
              division, C non-negative entropy terms: below 8 C 2^-24 together); a class's numerator and denominator are sums of at most
              R = R_max(b) such terms in a fixed order (relative error below R 2^-24 each), followed by one division, the smoothing and, for
              the second half, logf.  Hence |P - P64| <= (R_max(b) + 8 C + 64) 2^-23 P64 with a factor two of margin, and
              |ln P - ln P64| <= that relative amount (d ln P = dP / P) + 4 * 2^-24 |ln P64| for logf and the fp32 store.
  greedy, symkl, float   every replay ratio >= 1 - 2 (D/2 + 8) 2^-23 against the float64 distance of the SAME stored fp32 rows: a term
              (P - Q)(ln P - ln Q) carries three roundings, D/2 non-negative terms are added ((D/2 + 8) 2^-24 relative in any order), the pick
              compares two such values, twice that as margin -- the form of the existing Core-set bound.
  greedy, symkl, [A | 2A] with small integers A: every operation is exact, d = sum (a - a')^2: picks and radii equal the float64 greedy's
              and the 'sqeuclid' call on A, ties included."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import coreset_util
from tests.cdal_util import EPS, bound, greedy, replay_ratios, rows_float64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.3


def _chunk():
    from aod_meh_hua_amd import _C
    return int(_C.lib.aod_cdal_chunk())


def _row_counts():
    """one row, just under a wave, just over a wave, a ragged multi-chunk level -- and one row past the kernel's chunk"""
    base = [1, 63, 65, 4099]
    return base + ([_chunk() + 1] if _chunk() + 1 not in base else [])


def _dev(levels):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in levels]


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(C):
    """(levels fp32 [3, rows, C], float64 rows, R, ambiguous, device rows) of the issue's input: logits 3 N(0, 1) from default_rng(100 + C)"""
    from aod_meh_hua_amd import scoring
    g = np.random.default_rng(100 + C)
    levels = [(3 * g.standard_normal((3, r, C))).astype(np.float32) for r in _row_counts()]
    want, R, amb = rows_float64(levels, C, THR)
    got = scoring.cdal_descriptor(_dev(levels), C, THR)
    return levels, want, R, amb, got


def _check(got, want, R, C, what):
    tol = bound(want, R, C)
    err = np.abs(_f64(got) - want)
    print(f'{what}: max err / bound = {(err / tol).max():.4f} (P half {(err / tol)[:, :C * C].max():.4f}), R_max {R.max(axis=1).tolist()}')
    assert np.isfinite(_f64(got)).all() and (err <= tol).all(), what


# ---------------------------------------------------------------------------------------------------------------- descriptor
@pytest.mark.parametrize('C', [20, 7, 32])
def test_descriptor_matches_float64_within_the_derived_bound(C):
    levels, want, R, amb, got = _case(C)
    assert got.shape == (3, 2 * C * C) and got.dtype == torch.float32 and got.is_cuda
    assert amb == [], amb[:5]                                         # no row whose decision a rounding could flip: a flip cannot hide
    assert (R > 0).all() and 3500 <= R.sum(axis=1).min()              # every class is occupied, thousands of regions per image
    print(f'C = {C}: regions per image {R.sum(axis=1).tolist()}')
    _check(got, want, R, C, f'descriptor C={C}')
    P = _f64(got)[:, :C * C].reshape(3, C, C)
    assert np.abs(P.sum(axis=2) - 1).max() < 1e-4 and (P > 0).all()


@pytest.mark.parametrize('C', [20, 7])
def test_empty_classes_get_the_uniform_vector(C):
    from aod_meh_hua_amd import scoring
    levels = [x.copy() for x in _case(C)[0]]
    for x in levels:
        x[:, :, [2, 5]] -= 20
    want, R, amb = rows_float64(levels, C, THR)
    assert amb == [] and (R[:, [2, 5]] == 0).all() and (np.delete(R, [2, 5], axis=1) > 0).all()
    got = scoring.cdal_descriptor(_dev(levels), C, THR)
    _check(got, want, R, C, f'empty classes C={C}')
    P = got[:, :C * C].view(3, C, C)[:, [2, 5]].cpu().numpy()
    uni = np.float32(1) / np.float32(C)
    assert (np.abs(P - uni) <= 2 * np.spacing(uni)).all()             # uniform before smoothing: 1 / C again after it, within 2 ulp


def test_an_image_below_the_threshold_is_uniform_and_its_neighbours_are_unchanged():
    from aod_meh_hua_amd import scoring
    C = 20
    levels, _, _, _, ref = _case(C)
    levels = [x.copy() for x in levels]
    g = np.random.default_rng(9)
    for x in levels:                                                  # small logits: max p stays below 0.3 (checked in float64 below)
        x[1] = (0.1 * g.standard_normal(x[1].shape)).astype(np.float32)
    want, R, amb = rows_float64(levels, C, THR)
    assert R[1].sum() == 0 and all(b == 1 for _, b, _ in amb)         # (near-ties among probabilities around 0.05 decide nothing)
    got = scoring.cdal_descriptor(_dev(levels), C, THR)
    assert torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(_bits(got[2]), _bits(ref[2]))
    uni = np.float32(1) / np.float32(C)
    P, lnP = got[1, :C * C].cpu().numpy(), got[1, C * C:].cpu().numpy()
    print(f'no region: P in [{P.min()!r}, {P.max()!r}], 1 / C = {uni!r}')
    assert (np.abs(P - uni) <= 2 * np.spacing(uni)).all()
    assert (np.abs(lnP.astype(np.float64) + np.log(C)) <= 4 * 2.0 ** -23 * np.log(C)).all()


def _single_rows(rows, C, thr):
    """images of ONE row each (one level) -> (device rows, float64 rows, R)"""
    from aod_meh_hua_amd import scoring
    x = np.asarray(rows, np.float32).reshape(len(rows), 1, C)
    want, R, _ = rows_float64([x], C, thr)
    return scoring.cdal_descriptor(_dev([x]), C, thr), want, R


def test_the_threshold_is_strict_and_a_tie_goes_to_the_lower_class():
    C = 5
    lo = [-1e4] * (C - 2)
    got, want, R = _single_rows([[0., 0.] + lo, [1e-3, 0.] + lo, [0., 0.] + lo], C, 0.5)
    assert np.float32(1) / (np.float32(1) + np.float32(1)) == np.float32(0.5)        # max p is exactly 0.5 in fp32: NOT a region
    assert R.tolist() == [[0] * C, [1] + [0] * (C - 1), [0] * C]
    uni = np.float32(1) / np.float32(C)
    P = got[:, :C * C].view(3, C, C).cpu().numpy()
    assert (np.abs(P[[0, 2]] - uni) <= 2 * np.spacing(uni)).all()
    _check(got, want, R, C, 'strictness')
    assert abs(P[1, 0, 0] - 0.5) < 2e-3 and P[1, 0, 0] > 0.5 * (1 - 2 * EPS) and (np.abs(P[1, 1:] - uni) <= 2 * np.spacing(uni)).all()
    # two equal top logits above the threshold: class 0 (class 1 and 3, 4 with the tie moved) owns the region
    got, want, R = _single_rows([[2., 2.] + lo, [-1e4, 7., -1e4, 7., -1e4], [-1e4, -1e4, -1e4, 1., 1.]], C, 0.4)
    assert R.tolist() == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 1, 0]]
    _check(got, want, R, C, 'ties')
    P = got[:, :C * C].view(3, C, C).cpu().numpy()
    for b, c in ((0, 0), (1, 1), (2, 3)):
        others = np.delete(P[b], c, axis=0)
        assert abs(P[b, c].max() - 0.5) < 1e-3 and (np.abs(others - uni) <= 2 * np.spacing(uni)).all(), (b, c)


def test_a_one_hot_row_weighs_the_floor_and_gives_no_nan():
    from aod_meh_hua_amd import scoring
    C = 20
    hot = [40.] + [0.] * (C - 1)
    soft = np.log(np.array([20., 2., 2.] + [1.] * (C - 3)))            # p[0] = 20 / 41
    # image 0: the one-hot row alone; image 1: with a soft row of the same class (weights 2^-10 against H + 2^-10); image 2: the soft row alone
    x = np.array([[hot, hot], [hot, soft], [soft, soft]], np.float32)
    want, R, _ = rows_float64([x], C, THR)
    assert R[:, 0].tolist() == [2, 2, 2]
    got = scoring.cdal_descriptor(_dev([x]), C, THR)
    assert bool(torch.isfinite(got).all())
    _check(got, want, R, C, 'one-hot')
    P = got[:, :C * C].view(3, C, C).cpu().numpy().astype(np.float64)
    p_soft = np.exp(soft) / np.exp(soft).sum()
    w_soft = -(p_soft * np.log(p_soft)).sum() + EPS
    mix = (EPS * np.eye(C)[0] + w_soft * p_soft) / (EPS + w_soft)     # (the one-hot row's entropy is below 1e-14)
    assert np.allclose(P[1, 0], (1 - EPS) * mix + EPS / C, rtol=1e-5, atol=0)
    assert np.allclose(P[0, 0], (1 - EPS) * np.eye(C)[0] + EPS / C, rtol=1e-5, atol=0)


def test_unaligned_image_bases_read_the_same_values():
    """C = 7 and odd row counts: an image's base is not 16-B aligned (scalar loads); the same data at a 16-B aligned and at a shifted
    base give the same bits, and a level whose bases ARE aligned (C = 8) takes the vector path next to its float64 value"""
    from aod_meh_hua_amd import scoring
    C, B = 7, 3
    g = np.random.default_rng(77)
    levels = [(3 * g.standard_normal((B, r, C))).astype(np.float32) for r in (5, 131)]
    want, R, amb = rows_float64(levels, C, THR)
    assert amb == [] and all((x[0].size * 4) % 16 for x in levels)
    aligned = _dev(levels)
    got = scoring.cdal_descriptor(aligned, C, THR)
    _check(got, want, R, C, 'unaligned C=7')
    shifted = []
    for x in levels:
        buf = torch.zeros(x.size + 3, device='cuda')
        v = buf[1:1 + x.size].view(x.shape)
        v.copy_(torch.from_numpy(x))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        shifted.append(v)
    assert torch.equal(_bits(scoring.cdal_descriptor(shifted, C, THR)), _bits(got))
    # C = 8, 4-D channels_last maps [B, A * C, h, w] as the head hands them out: every base 16-B aligned
    maps = [(3 * g.standard_normal((B, h, w, 9 * 8))).astype(np.float32) for h, w in ((7, 9), (3, 3))]
    want, R, amb = rows_float64([m.reshape(B, -1, 8) for m in maps], 8, THR)
    assert amb == []
    dev = [torch.from_numpy(m).cuda().permute(0, 3, 1, 2) for m in maps]
    got = scoring.cdal_descriptor(dev, 8, THR)
    _check(got, want, R, 8, 'channels_last C=8')
    assert torch.equal(_bits(scoring.cdal_descriptor([d.permute(0, 2, 3, 1).reshape(B, -1, 8) for d in dev], 8, THR)), _bits(got))


def test_a_descriptor_has_the_same_bits_alone_and_anywhere_in_a_batch():
    from aod_meh_hua_amd import scoring
    C = 20
    levels, _, _, _, ref = _case(C)
    pick = lambda order: _dev([x[order] for x in levels])
    alone = scoring.cdal_descriptor(pick([1]), C, THR)
    first = scoring.cdal_descriptor(pick([1, 2]), C, THR)
    last = scoring.cdal_descriptor(pick([0, 2, 1]), C, THR)
    assert alone.shape == (1, 2 * C * C)
    for got, row in ((alone, 0), (first, 0), (last, 2)):
        assert torch.equal(_bits(got[row]), _bits(ref[1]))
    assert torch.equal(_bits(first[1]), _bits(ref[2])) and torch.equal(_bits(last[0]), _bits(ref[0]))
    assert torch.equal(_bits(scoring.cdal_descriptor(_dev(levels), C, THR)), _bits(ref))          # two calls on the same input
    # into rows 2..4 of a larger pool matrix: the other rows are not touched
    pool = torch.full((7, 2 * C * C), -7.0, device='cuda')
    out = scoring.cdal_descriptor(_dev(levels), C, THR, out=pool[2:5])
    assert out.data_ptr() == pool[2:5].data_ptr() and torch.equal(_bits(pool[2:5]), _bits(ref))
    assert bool((pool[:2] == -7).all()) and bool((pool[5:] == -7).all())


# ---------------------------------------------------------------------------------------------------------------- the metric
@pytest.mark.parametrize('H', [3, 64, 400])
def test_symkl_greedy_is_exact_on_integer_planes(H):
    """desc = [A | 2A], small integers: (a - a')(2a - 2a') / 2 = (a - a')^2 and every fp32 operation is exact.  H = 3: the scalar tail,
    64: one vector step, 400: VOC's width"""
    from aod_meh_hua_amd import scoring
    N, n_lab, budget = 40, 3, 14
    A = np.random.default_rng(H).integers(-2, 3, (N, H)).astype(np.float64)
    A[N // 2] = A[1]                                                  # a duplicate row
    X = np.concatenate([A, 2 * A], axis=1)
    lab = list(range(N - n_lab, N))
    picks, radius, ties = greedy(X, lab, budget)
    pe, re_, _ = coreset_util.greedy(A, lab, budget)
    p32, r32, _ = greedy(X, lab, budget, dtype=np.float32)
    assert ties >= 1 and picks.tolist() == pe.tolist() == p32.tolist() and np.array_equal(radius, re_) and np.array_equal(r32.astype(np.float64), radius)
    got_p, got_r = scoring.kcenter_greedy(torch.from_numpy(X.astype(np.float32)).cuda(), lab, budget, metric='symkl')
    euc_p, euc_r = scoring.kcenter_greedy(torch.from_numpy(A.astype(np.float32)).cuda(), lab, budget)
    print(f'H = {H}: {ties} tied steps, picks {got_p.tolist()[:8]}..., radius {got_r.tolist()[:4]}...')
    assert got_p.dtype == torch.int64 and got_r.dtype == torch.float32 and got_p.shape == (budget,)
    assert got_p.tolist() == picks.tolist() and np.array_equal(_f64(got_r), radius)
    assert torch.equal(got_p, euc_p) and torch.equal(_bits(got_r), _bits(euc_r))
    # no labelled row: the first pick is row 0 with radius inf, as for the default metric
    p0, r0 = scoring.kcenter_greedy(torch.from_numpy(X.astype(np.float32)).cuda(), [], 3, metric='symkl')
    assert p0.tolist() == greedy(X, [], 3)[0].tolist() and p0[0].item() == 0 and np.isinf(r0[0].item())


@pytest.fixture(scope='module')
def float_case():
    """48 synthetic images (one level of 300 rows, a per-image class bias so that the mixtures differ), their descriptors from the kernel"""
    from aod_meh_hua_amd import scoring
    C, N = 20, 48
    g = np.random.default_rng(48)
    x = (3 * g.standard_normal((N, 300, C)) + 2 * g.standard_normal((N, 1, C))).astype(np.float32)
    desc = scoring.cdal_descriptor(_dev([x]), C, THR)
    lab = [5, 17]
    picks, radius = scoring.kcenter_greedy(desc, lab, 12, metric='symkl')
    return desc, lab, picks, radius


def test_symkl_greedy_on_kernel_descriptors_picks_within_the_rounding_bound(float_case):
    desc, lab, picks, radius = float_case
    X = desc.cpu().numpy()                                             # the stored fp32 planes: the float64 distance is taken from THEM
    D = X.shape[1]
    assert D == 800 and np.isfinite(X).all()
    tol = 1.0 - 2.0 * (D / 2 + 8) * 2.0 ** -23
    ratios, r64 = replay_ratios(X, lab, picks.cpu().numpy(), return_radius=True)
    print(f'symkl greedy: min replay ratio {ratios.min():.9f} (bound {tol:.9f}), {int((ratios < 1).sum())} of {len(ratios)} steps below 1, '
          f'radius {r64[0]:.4f} .. {r64[-1]:.4f}')
    assert (ratios >= tol).all()
    p = picks.cpu().numpy()
    assert len(set(p.tolist())) == len(p) and not set(p.tolist()) & set(lab) and p.min() >= 0 and p.max() < X.shape[0]
    r = radius.cpu().numpy()
    assert np.isfinite(r).all() and (r[1:] <= r[:-1]).all() and r[-1] > 0
    assert (np.abs(r - r64) <= (D / 2 + 8) * 2.0 ** -24 * r64).all()
    # the other metric on the same rows selects by another distance (the argument is honoured)
    from aod_meh_hua_amd import scoring
    _, r_euc = scoring.kcenter_greedy(desc, lab, 12)
    d64 = np.asarray(X, np.float64)
    assert np.isclose(r_euc[0].item(), max(min(coreset_util.sqdist(d64, c)[i] for c in lab) for i in range(48)), rtol=1e-4)
    assert not np.isclose(r_euc[0].item(), r[0], rtol=1e-3)


def test_symkl_greedy_does_not_depend_on_the_order_of_the_centers_or_on_the_call(float_case):
    from aod_meh_hua_amd import scoring
    desc, lab, picks, radius = float_case
    for order in (lab, lab[::-1], torch.tensor(lab[::-1])):
        p2, r2 = scoring.kcenter_greedy(desc, order, 12, metric='symkl')
        assert torch.equal(p2, picks) and torch.equal(_bits(r2), _bits(radius))
    many = np.random.default_rng(6).permutation(48)[:2 * scoring.kcenter_chunk() + 3]
    pa, ra = scoring.kcenter_greedy(desc, many, 9, metric='symkl')
    pb, rb = scoring.kcenter_greedy(desc, np.sort(many)[::-1].copy(), 9, metric='symkl')
    assert torch.equal(pa, pb) and torch.equal(_bits(ra), _bits(rb))
    p4, r4 = scoring.kcenter_greedy(desc, lab, 5, metric='symkl')
    assert torch.equal(p4, picks[:5]) and torch.equal(r4, radius[:5])


def test_the_c_entry_refuses_an_odd_or_too_wide_row():
    from aod_meh_hua_amd import _C
    dev = torch.device('cuda')
    desc = torch.ones(8, 2050, device=dev)
    picks, radius, mind = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(2, device=dev), torch.empty(8, device=dev)
    ws = torch.empty(int(_C.lib.aod_kcenter_ws_len(8)), dtype=torch.uint8, device=dev)
    lab = torch.zeros(1, dtype=torch.int64, device=dev)
    for D, metric, msg in ((15, 1, 'is odd'), (2050, 1, 'descriptor columns'), (2049, 1, 'descriptor columns'), (16, 2, 'metric 2')):
        rc = _C.lib.aod_kcenter_greedy_ex(_C.ptr(desc), 8, D, _C.ptr(lab), 1, 2, _C.ptr(picks), _C.ptr(radius), _C.ptr(mind), _C.ptr(ws), _C.stream(),
                                          metric)
        assert rc == -1 and msg in _C.lib.aod_last_error().decode(), (D, metric)
    rc = _C.lib.aod_kcenter_greedy_ex(_C.ptr(desc), 8, 15, _C.ptr(lab), 1, 2, _C.ptr(picks), _C.ptr(radius), _C.ptr(mind), _C.ptr(ws), _C.stream(), 0)
    assert rc == 0                                                    # an odd D is the default metric's business as before
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the whole pass
def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


def _eager_reference(model, ds):
    """descriptor_float64 on the maps the model itself returns eagerly (isEval=True, justOut=True), in batches of 3 -> (rows, R, ambiguous)"""
    from aod_meh_hua_amd.apis.test import _unwrap
    rows, Rs, ambs = [], [], []
    with torch.no_grad():
        for data in _loader(ds, 3):
            data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
            maps = model(return_loss=False, rescale=True, isEval=True, justOut=True, **data)
            assert all(torch.is_tensor(t) and t.dtype == torch.float32 and t.shape[1] == 9 * 20 for t in maps)
            levels = [t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, 20).cpu().numpy() for t in maps]
            w, R, amb = rows_float64(levels, 20, THR)
            rows.append(w), Rs.append(R), ambs.extend(amb)
    return np.concatenate(rows), np.concatenate(Rs), ambs


@pytest.fixture(scope='module')
def pool():
    """a small RetinaNet and 6 synthetic images at 128 x 128.  retina_cls's weights are scaled (x 1, 2, 4, ...) until every image owns
    regions: the seeded head's logits are wide enough at x 1 today, and the loop keeps the fixture meaningful if the recipe changes"""
    from aod_meh_hua_amd.datasets import build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    prev = os.environ.pop('AOD_HIP_GRAPH', None)
    try:
        cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
        cfg.model.backbone.pop('init_cfg')
        ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=6, size=(128, 128)), dict(test_mode=True))
        sd = om.seeded_state_dict(cls_bias=-2.0)
        for scale in (1, 2, 4, 8, 16, 32):
            state = dict(sd)
            state['bbox_head.retina_cls.weight'] = sd['bbox_head.retina_cls.weight'] * scale
            model = build_detector(cfg.model)
            model.load_state_dict(state, strict=True)
            model = MMDataParallel(model.cuda()).eval()
            want, R, amb = _eager_reference(model, ds)
            if R.sum(axis=1).min() >= 20:
                break
        print(f'pool fixture: retina_cls x {scale}, regions per image {R.sum(axis=1).tolist()}')
        return cfg, model, ds, want, R, amb
    finally:
        if prev is not None:
            os.environ['AOD_HIP_GRAPH'] = prev


def test_descriptor_pass_is_batch_invariant_eager_or_replayed_and_matches_float64(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as apis_test
    cfg, model, ds, want, R, amb = pool
    assert (R.sum(axis=1) >= 20).all() and np.abs(want[0] - want[1]).max() > 1e-4      # regions everywhere, images that differ: not vacuous
    assert amb == [], amb[:5]
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    d2 = apis.single_gpu_cdal_descriptors(model, _loader(ds, 2))
    d3 = apis.single_gpu_cdal_descriptors(model, _loader(ds, 3), score_thr=THR)
    d1 = apis.single_gpu_cdal_descriptors(model, _loader(ds, 1))
    assert d2.shape == (6, 800) and d2.dtype == torch.float32 and d2.is_cuda
    assert torch.equal(_bits(d2), _bits(d3)) and torch.equal(_bits(d2), _bits(d1))
    # the forward was replayed: the single-member graph of single_gpu_ensemble's keying, one captured graph per batch shape
    gs = [v for k, v in apis_test._GSCORE.get(model).items() if k[:2] == ('just_out', 0)]
    assert len(gs) == 1 and len(gs[0].cache) == 3 and not gs[0].pipe
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    for bs in (1, 2, 3):
        assert torch.equal(_bits(apis.single_gpu_cdal_descriptors(model, _loader(ds, bs))), _bits(d2)), bs
    _check(d2, want, R, 20, 'descriptor pass')
    # another threshold is another descriptor (the argument reaches the kernel)
    assert not torch.equal(apis.single_gpu_cdal_descriptors(model, _loader(ds, 3), score_thr=0.9), d2)


def test_cdal_uncertainty_marks_the_picks_and_update_X_L_takes_them(pool, monkeypatch):
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    cfg, model, ds = pool[:3]
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    X_L = np.array([0, 3])
    unc = apis.CDAL_uncertainty(cfg, model, _loader(ds, 2), X_L=X_L, budget=2)
    assert unc.shape == (6,) and unc.dtype == torch.float32 and not unc.is_cuda
    assert sorted(unc.tolist()) == [0., 0., 0., 0., 1., 2.] and unc[0] == 0 and unc[3] == 0
    desc = apis.single_gpu_cdal_descriptors(model, _loader(ds, 2))
    picks, radius = scoring.kcenter_greedy(desc, X_L, 2, metric='symkl')
    assert unc[picks[0]].item() == 2 and unc[picks[1]].item() == 1 and radius[0] >= radius[1] > 0
    want_p, _, _ = greedy(desc.cpu().numpy().astype(np.float64), X_L, 2)
    ratios = replay_ratios(desc.cpu().numpy(), X_L, picks.cpu().numpy())
    assert (ratios >= 1.0 - 2.0 * (400 + 8) * 2.0 ** -23).all(), (ratios, want_p)
    cfg.uncertainty_pool = 'CDAL'
    try:
        again = apis.calculate_uncertainty(cfg, model, _loader(ds, 3), X_L=X_L, budget=2, score_thr=0.3, clsW=False)
    finally:
        cfg.uncertainty_pool = 'Entropy_NMS'
    assert torch.equal(again, unc)
    X_L_next, _ = update_X_L(unc, np.arange(6), X_L, 2, zeroRate=0)
    assert X_L_next.tolist() == sorted([0, 3] + picks.tolist())
