"""GPU: the class difficulty of DESIGN 3p -- aod_class_difficulty_accum / _update against the float64 restatement of
tests/difficulty_util.py and their bit properties; aod_det_uncertainty_w (scoring.det_uncertainty(class_w=...)) against
tests/posterior_unc_util.py's values times the weight; the heads' EMA inside the training step (eager, replayed, per-level launches,
checkpoints); and the class-weighted pools (Posterior_uncertainty(class_weighted=True), Uncertainty_fns.PPAL).

Tolerances.  S[c] / n[c] and the updated d: atol 1e-5 (difficulty_util: q <= 1, a few ulp per sample, a mean over at most 64 positives).
Weighted measures: section 3l's tolerances (posterior_unc_util) with one more fp32 rounding of a value <= 1.2 times the unweighted one:
entropy / sums rtol 2e-5 + 2^-23, atol 1e-7; margin / least confidence and their max atol (4 * 1.2 + 1.2) * 2^-24 = 6 * 2^-24."""
import functools
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import difficulty_util as D
from tests import posterior_unc_util as U
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD = dict(xi=0.6, momentum=0.99, alpha=0.3, beta=0.2)
GRID_ROUND = 256 * 1024          # rows of one grid-stride round: 256 blocks of 1024 rows


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(x):
    return {k: torch.from_numpy(v).cuda() for k, v in x.items()}


def _accum(x, form, acc=None, **kw):
    from aod_meh_hua_amd import hipops as ho
    C = x['cls'].shape[1]
    acc = torch.zeros(2 * C, device='cuda') if acc is None else acc
    return ho.class_difficulty_accum(x['cls'], x['labels'], x['label_w'], x['bbox_pred'], x['bbox_tgt'], acc, form=form, **kw)


def _check(x, form, what, **kw):
    """one accumulate + one update on x (numpy) against float64: exact counts, means and the updated d within ATOL, unseen classes keep
    their bits, acc is zeroed.  Returns (acc before the update, d after it)."""
    from aod_meh_hua_amd import hipops as ho
    C = x['cls'].shape[1]
    S, n, _ = D.batch_stat64(**x, form=form, **kw)
    acc = _accum(_dev(x), form, **kw)
    got = _np(acc).astype(np.float64)
    assert np.array_equal(got[C:], n.astype(np.float64)), (what, got[C:], n)
    seen = n > 0
    assert not got[:C][~seen].any()
    err = np.abs(got[:C][seen] / n[seen] - S[seen] / n[seen]).max(initial=0.0)
    d0 = torch.linspace(0.05, 1.0, C, device='cuda')
    d = d0.clone()
    before = acc.clone()
    ho.class_difficulty_update(acc, d, D.MOMENTUM)
    want = D.ema64(_np(d0), S, n)
    err_d = np.abs(_np(d).astype(np.float64) - want).max()
    print(f'{what}: {int(n.sum())} positives, at most {int(n.max(initial=0))} per class, max |mean - float64| {err:.3e}, max |d - float64| {err_d:.3e} '
          f'(atol {D.ATOL:g})')
    assert n.max(initial=0) <= D.MAX_POS_PER_CLASS
    assert err <= D.ATOL and err_d <= D.ATOL, what
    assert torch.equal(_bits(d[~torch.from_numpy(seen).cuda()]), _bits(d0[~torch.from_numpy(seen).cuda()]))
    assert not bool(acc.any())
    return before, d


# ---------------------------------------------------------------------------------------------------------------- accumulate / update
@pytest.mark.parametrize('form', D.FORMS)
@pytest.mark.parametrize('C', [1, 20, 80])
@pytest.mark.parametrize('nrows', [1, 255, 257, 5000])
def test_accumulate_and_update_match_float64(nrows, C, form):
    x = D.make_inputs(nrows, C, seed=1000 * C + nrows)
    assert D.positives(x['labels'], x['label_w'], C)[-1] == nrows - 1          # a positive in the last row
    _check(x, form, f'{form} C={C} nrows={nrows}')
    # the heads' coder: non-trivial means and stds
    if nrows == 257:
        _check(x, form, f'{form} C={C} nrows={nrows} coder', means=(0.01, -0.02, 0.03, 0.0), stds=(0.1, 0.1, 0.2, 0.2))


@pytest.mark.parametrize('form', D.FORMS)
def test_more_rows_than_one_grid_stride_round(form):
    nrows = GRID_ROUND + 1500                                                # the first block walks a second chunk
    from aod_meh_hua_amd import _C
    assert int(_C.lib.aod_class_difficulty_ws_len(nrows, 20)) == 256 * 40
    g = np.random.default_rng(76)
    rows = np.unique(np.concatenate([g.choice(nrows, 600, replace=False), [3, 1023, 1024, GRID_ROUND - 1, GRID_ROUND, nrows - 1]]))
    x = D.make_inputs(nrows, 20, seed=77, pos_rows=rows)
    pos = D.positives(x['labels'], x['label_w'], 20)
    assert (pos >= GRID_ROUND).sum() >= 1 and (pos < 1024).sum() >= 1 and pos[-1] == nrows - 1
    _check(x, form, f'{form} nrows={nrows}')


def _edge_rows(C):
    """hand-made positives on a background of NaN rows: dw beyond the clamp, disjoint boxes, identical boxes with a saturated logit, logits
    that underflow P to 0, one class with a single positive"""
    n = 40
    x = D.make_inputs(n, C, seed=5, pos_rows=[])
    assert np.isnan(x['cls']).all() and np.isnan(x['bbox_pred']).all()
    lab, lw, cls, bp, bt = x['labels'], x['label_w'], x['cls'], x['bbox_pred'], x['bbox_tgt']
    lab[:] = C
    lab[[3, 17]] = -1

    def put(r, c, logits, dp, dt):
        lab[r], lw[r], cls[r], bp[r], bt[r] = c, 1.0, logits, dp, dt
    base = np.full(C, -2.0, np.float32)
    one = lambda c, v: np.concatenate([base[:c], [v], base[c + 1:]]).astype(np.float32)
    put(0, 0, one(0, 1.0), [0.1, 0.0, 9.0, 0.2], [0.0, 0.1, 7.0, 0.1])                # dw beyond the clamp on both boxes
    put(5, 1 % C, one(1 % C, 2.0), [5.0, 5.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])         # disjoint boxes: q = 1
    put(9, 2 % C, one(2 % C, 60.0), [0.2, -0.1, 0.3, 0.1], [0.2, -0.1, 0.3, 0.1])      # identical boxes, saturated logit: q <= 1e-6
    under = np.full(C, 120.0, np.float32)
    under[3 % C] = -120.0
    put(21, 3 % C, under, [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])                 # P underflows to 0 (both forms): q = 1
    put(n - 1, 4 % C, one(4 % C, 0.5), [0.05, 0.0, 0.1, 0.0], [0.0, 0.0, 0.0, 0.0])    # the last row
    lab[30], lw[30] = 1 % C, 0.0                                                       # a foreground label without weight: skipped
    return x


@pytest.mark.parametrize('form', D.FORMS)
def test_edges(form):
    from aod_meh_hua_amd import hipops as ho
    C = 20
    x = _edge_rows(C)
    S, n, qs = D.batch_stat64(**x, form=form)
    assert sorted(qs) == [0, 5, 9, 21, 39] and qs[5] == 1.0 and qs[21] == 1.0 and qs[9] <= 1e-6 and 0 < qs[0] < 1
    assert n.tolist() == [1, 1, 1, 1, 1] + [0] * 15                              # every class here has a single positive
    acc, d = _check(x, form, f'{form} edges')
    got = _np(acc)
    assert got[1] == 1.0 and got[3] == 1.0 and got[2] <= 1e-6 and np.isfinite(got).all()
    # no positive at all: acc stays zero, d keeps its bits through the update
    none = D.make_inputs(700, C, seed=6, pos_rows=[])
    acc = _accum(_dev(none), form)
    assert not bool(acc.any())
    d0 = torch.rand(C, device='cuda')
    d = d0.clone()
    ho.class_difficulty_update(acc, d, 0.99)
    assert torch.equal(_bits(d), _bits(d0))
    # every positive in one workgroup: 64 per class in the first chunk of several
    full = D.make_inputs(3000, 4, seed=8, pos_rows=np.arange(0, 512, 2))
    S, n, _ = D.batch_stat64(**full, form=form)
    assert n.tolist() == [64] * 4
    _check(full, form, f'{form} one workgroup')
    # no row at all is a no-op
    empty = {k: v[:0] for k, v in _dev(full).items()}
    assert not bool(_accum(empty, form).any())


@pytest.mark.parametrize('form', D.FORMS)
def test_two_calls_on_the_halves_and_run_to_run_bits(form):
    from aod_meh_hua_amd import hipops as ho
    C, nrows = 20, 5001
    x = D.make_inputs(nrows, C, seed=12)
    dx = _dev(x)
    S, n, _ = D.batch_stat64(**x, form=form)
    whole = _accum(dx, form)
    again = _accum(dx, form)
    assert torch.equal(_bits(whole), _bits(again))                             # the same call twice: the same bits
    # the halves: the second starts at an odd row, so its labels are 8-byte aligned only
    h = 2501
    acc = torch.zeros(2 * C, device='cuda')
    for sl in (slice(0, h), slice(h, nrows)):
        part = {k: v[sl] for k, v in dx.items()}
        assert part['cls'].is_contiguous() and (sl.start == 0 or part['labels'].data_ptr() % 16 == 8)
        _accum(part, form, acc=acc)
    got = _np(acc).astype(np.float64)
    assert np.array_equal(got[C:], n.astype(np.float64)) and np.array_equal(_np(whole)[C:], _np(acc)[C:])
    seen = n > 0
    assert np.abs(got[:C][seen] / n[seen] - S[seen] / n[seen]).max() <= D.ATOL
    d = torch.ones(C, device='cuda')
    ho.class_difficulty_update(acc, d, 0.99)
    assert np.abs(_np(d).astype(np.float64) - D.ema64(np.ones(C), S, n)).max() <= D.ATOL
    # an odd start alone: the same bits as the same rows behind a 16-byte aligned pointer
    part = {k: v[h:] for k, v in dx.items()}
    moved = {k: v.clone() for k, v in part.items()}
    assert part['labels'].data_ptr() % 16 == 8 and moved['labels'].data_ptr() % 16 == 0
    assert torch.equal(_bits(_accum(part, form)), _bits(_accum(moved, form)))


def test_wrappers_refuse_on_the_device():
    from aod_meh_hua_amd import hipops as ho
    dx = _dev(D.make_inputs(16, 20, seed=1))
    with pytest.raises(ValueError, match='16-byte aligned'):
        ho.class_difficulty_accum(dx['cls'], dx['labels'], dx['label_w'], torch.zeros(65, device='cuda')[1:].view(16, 4), dx['bbox_tgt'],
                                  torch.zeros(40, device='cuda'))
    with pytest.raises(ValueError, match='acc must be'):
        ho.class_difficulty_accum(dx['cls'], dx['labels'], dx['label_w'], dx['bbox_pred'], dx['bbox_tgt'], torch.zeros(20, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------- det_uncertainty(class_w)
from tests.test_gpu_posterior_unc import _case  # noqa: E402  (the device path's own tensors for seeded maps, checked on the host)


def _weighted_reference(c, w, measure, aggregate, thr=None):
    want = U.reference(*c.host, c.layout, measure, aggregate, c.thr if thr is None else thr)
    labels = c.host[3]
    obj = want['obj'].copy()
    ok = want['rows'] >= 0
    obj[ok] = obj[ok] * w.astype(np.float64)[labels[ok]]
    unc = np.zeros(obj.shape[0])
    for b in range(obj.shape[0]):
        v = obj[b][ok[b]]
        if len(v):
            unc[b] = dict(max=v.max(), mean=v.sum() / len(v), sum=v.sum())[aggregate]
    return dict(want, obj=obj, unc=unc)


def _weighted_tolerances(measure, aggregate):
    per, img = U.tolerances(measure, aggregate)
    one_more = lambda t: (t[0] + 2.0 ** -23, t[1]) if t[0] else (0.0, 6 * 2.0 ** -24)
    return one_more(per), one_more(img)


@pytest.mark.parametrize('layout', U.LAYOUTS)
def test_no_weights_and_unit_weights_are_todays_bits(layout):
    from aod_meh_hua_amd import scoring
    c = _case(layout, 20)
    W = c.cand.scores.shape[2]
    for measure, aggregate in itertools.product(U.MEASURES, U.AGGREGATES):
        ref = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, c.thr, want_objects=True)
        ref_c = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, c.thr, want_objects=True, want_cand=True)
        for w in (None, torch.ones(W, device='cuda')):
            got = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, c.thr, want_objects=True, class_w=w)
            assert len(got) == 3 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ref, got)), (measure, aggregate, w is None)
            got = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, c.thr, want_objects=True, want_cand=True,
                                          class_w=w)
            assert len(got) == 4 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ref_c, got))
            alone = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, c.thr, class_w=w)
            assert torch.equal(_bits(alone), _bits(ref[0]))


@pytest.mark.parametrize('max_num', [7, 100])
@pytest.mark.parametrize('layout', U.LAYOUTS)
def test_weighted_measures_match_float64_and_are_batch_invariant(layout, max_num):
    from aod_meh_hua_amd import scoring
    c = _case(layout, 20, 3, max_num, 0.3)
    W = c.cand.scores.shape[2]
    w = torch.from_numpy(np.random.default_rng(3).uniform(1.0, 1.2, W).astype(np.float32)).cuda()
    for measure, aggregate in itertools.product(U.MEASURES, U.AGGREGATES):
        unc, obj, missing = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, c.thr, want_objects=True, class_w=w)
        want = _weighted_reference(c, _np(w), measure, aggregate)
        tol_obj, tol_unc = _weighted_tolerances(measure, aggregate)
        assert np.array_equal(np.isnan(_np(obj)), want['rows'] < 0) and _np(missing).tolist() == [0] * 3
        assert U.close(_np(obj), want['obj'], tol_obj), (measure, aggregate)
        assert U.close(_np(unc), want['unc'], tol_unc), (measure, aggregate)
        plain = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, c.thr)
        assert bool((unc[:-1] > plain[:-1]).any()) and float(unc[-1]) == 0.0                    # the weights are felt; no object: 0
        if (measure, aggregate) in (('entropy', 'sum'), ('margin', 'mean'), ('leastconf', 'max')):
            for order, row, img in (([1], 0, 1), ([1, 0, 2], 0, 1), ([2, 0, 1], 2, 1), ([0], 0, 0), ([2, 0], 1, 0)):
                pick = lambda t: t[order].contiguous()
                cand = SimpleNamespace(boxes=pick(c.cand.boxes), scores=pick(c.cand.scores))
                u, o, _ = scoring.det_uncertainty(cand, pick(c.dets), pick(c.labels), pick(c.num), layout, measure, aggregate, c.thr,
                                                  want_objects=True, class_w=w)
                assert torch.equal(_bits(u[row]), _bits(unc[img])) and torch.equal(_bits(o[row]), _bits(obj[img])), (measure, order)


def test_the_weights_flip_an_entropy_order():
    from aod_meh_hua_amd import scoring
    # one candidate and one object per image: image 0 is a class-1 object with the larger entropy, image 1 a class-0 object
    boxes = torch.tensor([[[1., 2., 30., 40.]], [[5., 6., 20., 9.]]], device='cuda')
    scores = torch.tensor([[[.1, .7, .2, 0.]], [[.72, .14, .14, 0.]]], device='cuda')
    dets, labels, keep, num = scoring.multiclass_nms_batch(boxes, scores, 0.05, 0.5, 5)
    cand = SimpleNamespace(boxes=boxes, scores=scores)
    host = tuple(_np(t) for t in (boxes, scores, dets, labels, num))
    w = np.array([1.2, 1.0, 1.1, 1.0], np.float32)
    c = SimpleNamespace(host=host, layout='cat', thr=0.3)
    plain, weighted = U.reference(*host, 'cat', 'entropy', 'max', 0.3), _weighted_reference(c, w, 'entropy', 'max')
    assert plain['count'].tolist() == [1, 1]
    assert plain['unc'][0] > plain['unc'][1] + 1e-3 and weighted['unc'][1] > weighted['unc'][0] + 1e-3        # it flips on the CPU
    u0 = scoring.det_uncertainty(cand, dets, labels, num, 'cat', 'entropy', 'max', 0.3)
    u1 = scoring.det_uncertainty(cand, dets, labels, num, 'cat', 'entropy', 'max', 0.3, class_w=torch.from_numpy(w).cuda())
    assert float(u0[0]) > float(u0[1]) and float(u1[1]) > float(u1[0])
    assert U.close(_np(u1), weighted['unc'], _weighted_tolerances('entropy', 'max')[1])


# ---------------------------------------------------------------------------------------------------------------- the model
KINDS = ('SSL_L_RetinaNet', 'MyRetinaNet')


def _build_train(kind, tracked=True, lr=2e-4):
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    from tests import plain_retina_util as PU
    config, sd = {'SSL_L_RetinaNet': ('configs/_base_/Config_RetinaNet.py', lambda: om.seeded_state_dict(cls_bias=-2.0)),
                  'MyRetinaNet': ('configs/_base_/Config_RetinaNet_plain.py', lambda: PU.plain_state_dict(cls_bias=-2.0))}[kind]
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    if tracked:
        cfg.model.bbox_head.class_difficulty = dict(CD)
    model = build_detector(cfg.model)
    assert type(model).__name__ == kind
    model.load_state_dict(sd(), strict=not tracked)          # (the seeded checkpoint has no difficulty keys: the ones stay)
    model = model.cuda().train()
    cfg.optimizer.lr = lr
    opt, opt_L = build_optimizers(model, cfg)
    return model, cfg, opt, opt_L


def _batch(seed, B=4, H=64):
    gtb, gtl = synth.random_gts(B, H, H, seed=seed, gmin=1, gmax=3)
    return dict(img=synth.images(B, H, H, seed=seed).cuda(), img_metas=synth.metas(B, H, H), gt_bboxes=gtb, gt_labels=gtl)


def _record_loss_operands(monkeypatch):
    """wraps the loss forwards' launches (hipops.edl_focal_l1_levels_fwd / edl_focal_l1_fwd): host copies of the operands of every call"""
    from aod_meh_hua_amd import hipops as ho
    seen = []
    for name in ('edl_focal_l1_levels_fwd', 'edl_focal_l1_fwd'):
        orig = getattr(ho, name)

        def wrapped(cls, labels, label_w, bbox_pred, bbox_tgt, *a, _orig=orig, _name=name, **kw):
            seen.append(dict(name=_name, form=kw.get('form', 'edl'), cls=_np(cls), labels=_np(labels), label_w=_np(label_w), bbox_pred=_np(bbox_pred),
                             bbox_tgt=_np(bbox_tgt)))
            return _orig(cls, labels, label_w, bbox_pred, bbox_tgt, *a, **kw)
        monkeypatch.setattr(ho, name, wrapped)
    return seen


@pytest.mark.parametrize('levels', [True, False], ids=['all-levels', 'per-level'])
@pytest.mark.parametrize('kind', KINDS)
def test_one_train_step_updates_the_difficulty_from_its_own_loss_operands(kind, levels, monkeypatch):
    from aod_meh_hua_amd import functional as AF
    monkeypatch.setattr(AF, 'LOSS_LEVELS', levels)           # (what AOD_LOSS_LEVELS=0 selects at import: one loss launch per level)
    model, cfg, opt, opt_L = _build_train(kind)
    head = model.bbox_head
    assert head.class_difficulty.tolist() == [1.0] * 20 and head.class_difficulty.is_cuda
    seen = _record_loss_operands(monkeypatch)
    out, *_ = model.train_step(_batch(31), Labeled=True, Pseudo=False)
    torch.cuda.synchronize()
    assert [s['name'] for s in seen] == (['edl_focal_l1_levels_fwd'] if levels else ['edl_focal_l1_fwd'] * 5)
    form = 'sigmoid' if kind == 'MyRetinaNet' else 'edl'
    assert all(s['form'] == form for s in seen)
    x = {k: np.concatenate([s[k] for s in seen]) for k in ('cls', 'labels', 'label_w', 'bbox_pred', 'bbox_tgt')}
    S, n, _ = D.batch_stat64(**x, form=form, means=tuple(head.bbox_coder.means), stds=tuple(head.bbox_coder.stds))
    want = D.ema64(np.ones(20), S, n)
    got = _np(head.class_difficulty).astype(np.float64)
    print(f'{kind} levels={levels}: positives per class {n.tolist()}, d {got.tolist()}, max |d - float64| {np.abs(got - want).max():.3e}')
    assert 1 <= (n > 0).sum() < 20 and n.max() <= D.MAX_POS_PER_CLASS
    assert np.abs(got - want).max() <= D.ATOL and (got <= 1.0).all() and (got[n > 0] < 1.0).any()      # (a class whose positives all have q = 1 stays at 1)
    assert (got[n == 0] == 1.0).all()                                            # classes absent from the batch stay exactly 1
    assert not bool(head._class_difficulty_acc.any())


def _three_iterations(kind, tracked, graphed):
    model, cfg, opt, opt_L = _build_train(kind, tracked)
    losses, ds = [], []
    gs = None
    if graphed:
        from aod_meh_hua_amd.graphs import GraphedTrainStep
        gs = GraphedTrainStep(model, opt, opt_L, warmup=2, Labeled=True, Pseudo=False)
    for seed in (31, 32, 33):
        d = _batch(seed)
        if graphed:
            losses.append(float(gs(d)['loss']))
        else:
            out, head_out, feat_out, prev = model.train_step(d, Labeled=True, Pseudo=False)
            opt.zero_grad()
            out['loss'].backward()
            opt.step()
            if opt_L is not None:
                lossL = model.train_step_L(prev, head_out, feat_out)
                opt_L.zero_grad()
                lossL['loss'].backward()
                opt_L.step()
            losses.append(float(out['loss'].detach()))
        if tracked:
            ds.append(model.bbox_head.class_difficulty.detach().cpu().clone())
    torch.cuda.synchronize()
    if graphed:
        assert len(gs.cache) == 1                                                # one capture (two warm-up iterations, undone), three replays
    return losses, ds, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize('kind', KINDS)
def test_three_iterations_eager_replayed_and_untracked(kind):
    """deterministic mode (ordered column sums: eager and replayed iterations are the same bits): the EMA after every iteration is the same
    eager and replayed -- the replayed run's first batch ran two warm-up iterations that the snapshot / restore of the module buffers
    undid -- and the losses and weights are those of a model without the option"""
    from aod_meh_hua_amd import functional as AF
    AF.set_deterministic(True)
    try:
        l_off, _, sd_off = _three_iterations(kind, False, False)
        l_on, d_on, sd_on = _three_iterations(kind, True, False)
        l_g, d_g, sd_g = _three_iterations(kind, True, True)
    finally:
        AF.set_deterministic(False)
    print(kind, 'losses', l_on, 'd after 3', d_on[-1].tolist())
    assert l_on == l_off and l_g == l_on and all(np.isfinite(l_on))
    assert set(sd_on) - set(sd_off) == {'bbox_head.class_difficulty', 'bbox_head.class_weight'}
    for k in sd_off:
        assert torch.equal(sd_off[k], sd_on[k]), ('tracked vs untracked', k)
    for k in sd_on:
        assert torch.equal(sd_on[k], sd_g[k]), ('replayed vs eager', k)
    for a, b in zip(d_on, d_g):
        assert torch.equal(_bits(a), _bits(b))
    assert bool((d_on[0] < 1).any()) and not torch.equal(d_on[0], d_on[1]) and not torch.equal(d_on[1], d_on[2])
    # exactly three updates: a class seen in every batch has moved three times, never more than 3 * (1 - m) away from 1
    assert float((1 - d_on[-1]).max()) <= 3 * (1 - CD['momentum']) + 1e-6


@pytest.mark.parametrize('kind', KINDS)
def test_checkpoint_round_trip_through_the_runner(kind, tmp_path, monkeypatch):
    from aod_meh_hua_amd.mmcv_lite import MMDataParallel, build_runner
    from aod_meh_hua_amd.utils import get_root_logger
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')

    def runner_of(model, cfg, opt, opt_L):
        r = build_runner(cfg.runner, default_args=dict(model=MMDataParallel(model, device_ids=[0]), optimizer=opt, work_dir=None,
                                                       logger=get_root_logger(log_level='ERROR'), meta=None))
        r.optimizer_L = opt_L
        return r
    model, cfg, opt, opt_L = _build_train(kind)
    runner = runner_of(model, cfg, opt, opt_L)
    for seed in (41, 42):
        runner.run_iter(_batch(seed), train_mode=True, Labeled=True, Pseudo=False)
    d = model.bbox_head.class_difficulty.detach().clone()
    assert bool((d < 1).any())
    runner.save_checkpoint(str(tmp_path), create_symlink=False)
    ck = torch.load(str(tmp_path / 'epoch_1.pth'), map_location='cpu')
    assert torch.equal(ck['state_dict']['bbox_head.class_difficulty'], d.cpu()) and 'bbox_head._class_difficulty_acc' not in ck['state_dict']
    model2, cfg2, opt2, opt_L2 = _build_train(kind)
    assert model2.bbox_head.class_difficulty.tolist() == [1.0] * 20
    runner_of(model2, cfg2, opt2, opt_L2).load_checkpoint(str(tmp_path / 'epoch_1.pth'))
    assert torch.equal(_bits(model2.bbox_head.class_difficulty), _bits(d))
    assert torch.equal(_bits(model2.bbox_head.class_weight), _bits(model.bbox_head.class_weight))


# ---------------------------------------------------------------------------------------------------------------- the pools
N_POOL = 14


def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


@functools.lru_cache(maxsize=None)
def _pool(kind):
    """the small synthetic detectors of the CCMS tests with the option on, and the gate of that fixture (the smallest top score)"""
    from aod_meh_hua_amd.apis.test import _unwrap
    from aod_meh_hua_amd.datasets import build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    from tests import plain_retina_util as PU
    config, sd = {'SSL_L_RetinaNet': ('configs/_base_/Config_RetinaNet.py', lambda: om.seeded_state_dict(cls_bias=-2.0)),
                  'MyRetinaNet': ('configs/_base_/Config_RetinaNet_plain.py', lambda: PU.plain_state_dict(cls_bias=-0.5))}[kind]
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    cfg.model.bbox_head.class_difficulty = dict(CD)
    model = build_detector(cfg.model)
    model.load_state_dict(sd(), strict=False)
    model = model.cuda().eval()
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=N_POOL, size=(64, 64)), dict(test_mode=True))
    batches = []
    for data in _loader(ds, 4):
        data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
        batches.append((data['img'][0].cuda(), data['img_metas'][0]))
    if kind == 'SSL_L_RetinaNet':
        import bench
        bench.calibrate_head(model, batches[0][0])
    tops = []
    for img, metas in batches:
        with torch.no_grad():
            dets, labels, num = model(return_loss=False, rescale=True, isEval=True, _padded=True, isUnc=False, img=[img], img_metas=[metas])
        tops += [float(dets[b, :int(num[b]), 4].max()) if int(num[b]) else 0.0 for b in range(dets.shape[0])]
    return cfg, MMDataParallel(model).eval(), ds, float(np.float32(min(tops)))


@pytest.mark.parametrize('kind', KINDS)
def test_weighted_posterior_pool_eager_replayed_batch_sizes_and_float64(kind, monkeypatch):
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd.apis.test import _unwrap
    cfg, model, ds, thr = _pool(kind)
    head = model.module.bbox_head
    layout = scoring.ACTIVATION_LAYOUT[head.last_activation]
    # a fresh model: every class weighs 1 + beta -- the maximum of the detections' values scales with it exactly
    with torch.no_grad():
        head.class_difficulty.fill_(1.0)
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    plain = apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure='entropy', aggregate='max', score_thr=thr)
    fresh = apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure='entropy', aggregate='max', score_thr=thr, class_weighted=True)
    w1 = float(head.class_weight[0])
    assert abs(w1 - 1.2) <= 2.0 ** -22 and head.class_weight[:-1].eq(w1).all() and float(head.class_weight[-1]) == 1.0
    assert int((plain > 0).sum()) >= N_POOL // 2
    assert torch.equal(_bits(fresh), _bits((plain * np.float32(w1)).float()))               # one rounding: the multiply itself
    # a trained model's difficulties differ per class: the stale weights are refreshed before the first batch
    with torch.no_grad():
        head.class_difficulty.copy_(torch.linspace(0.05, 0.95, 20))
    for measure, aggregate in (('entropy', 'sum'), ('margin', 'max')):
        eager = apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure=measure, aggregate=aggregate, score_thr=thr, class_weighted=True)
        w = _np(head.class_weight)
        assert np.abs(w[:20] - D.class_weight64(np.linspace(0.05, 0.95, 20, dtype=np.float32))).max() < 4 * 2.0 ** -23 and w[20] == 1.0
        assert torch.equal(_bits(apis.Posterior_uncertainty(cfg, model, _loader(ds, 1), measure=measure, aggregate=aggregate, score_thr=thr,
                                                            class_weighted=True)), _bits(eager))
        # against the util on the tensors score_batch handed to the kernel
        pool = {'entropy': 'Entropy', 'margin': 'Margin'}[measure]
        want, direct = [], []
        with torch.no_grad():
            for data in _loader(ds, 4):
                data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
                _, unc, it = model(return_loss=False, rescale=True, isEval=False, isUnc='Epistemic', uPool=pool, unc_aggregate=aggregate,
                                   score_thr=thr, class_weighted=True, _return_internals=True, **data)
                c = SimpleNamespace(host=tuple(_np(t) for t in (it['cand'].boxes, it['cand'].scores, it['dets'], it['labels'], it['num'])),
                                    layout=layout, thr=thr)
                want.append(_weighted_reference(c, w, measure, aggregate)['unc'])
                direct.append(unc.cpu())
        assert torch.equal(_bits(torch.cat(direct)), _bits(eager))
        assert U.close(eager.numpy(), np.concatenate(want), _weighted_tolerances(measure, aggregate)[1])
        unweighted = apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure=measure, aggregate=aggregate, score_thr=thr)
        assert bool((eager >= unweighted).all()) and bool((eager > unweighted).any())
        # replayed: the captured graph reads the refreshed buffer; new difficulties reach a graph that is already captured
        monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
        for bs in (4, 1):
            got = apis.Posterior_uncertainty(cfg, model, _loader(ds, bs), measure=measure, aggregate=aggregate, score_thr=thr, class_weighted=True)
            assert torch.equal(_bits(got), _bits(eager)), (measure, bs)
        monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    with torch.no_grad():
        head.class_difficulty.fill_(1.0)
    again = apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure='margin', aggregate='max', score_thr=thr, class_weighted=True)
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    assert torch.equal(_bits(again), _bits(apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure='margin', aggregate='max', score_thr=thr,
                                                                      class_weighted=True)))
    assert not torch.equal(again, eager)


@pytest.mark.parametrize('kind', KINDS)
def test_ppal_marks_the_picks_and_update_X_L_takes_them(kind, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    cfg, model, ds, thr = _pool(kind)
    head = model.module.bbox_head
    with torch.no_grad():
        head.class_difficulty.copy_(torch.linspace(0.95, 0.05, 20))
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    X_L, budget = np.array([0, 9]), 3
    keep, cfg.uncertainty_pool = cfg.uncertainty_pool, 'PPAL'
    try:
        unc = apis.calculate_uncertainty(cfg, model, _loader(ds, 4), X_L=X_L, budget=budget, candidate_factor=2, max_obj=8, score_thr=thr, clsW=False,
                                         iou_thr=0.5)
    finally:
        cfg.uncertainty_pool = keep
    assert unc.shape == (N_POOL,) and unc.dtype == torch.float32 and not unc.is_cuda
    assert sorted(unc.tolist()) == [0.0] * (N_POOL - budget) + [1.0, 2.0, 3.0] and unc[0] == 0 and unc[9] == 0      # budget..1 on unlabelled images
    assert torch.equal(unc, apis.CCMS_uncertainty(cfg, model, _loader(ds, 4), X_L=X_L, budget=budget, candidate_factor=2, max_obj=8, score_thr=thr,
                                                  class_weighted=True))
    # the first pick: the most class_weighted-uncertain unlabelled image (stage 1 is the weighted posterior pool's sum)
    stage1 = apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure='entropy', aggregate='sum', score_thr=thr, class_weighted=True)
    free = np.setdiff1d(np.arange(N_POOL), X_L)
    first = int(free[np.argmax(stage1.numpy()[free])])
    assert int(torch.argmax(unc)) == first and float(unc[first]) == 3.0
    store = apis.single_gpu_object_descriptors(model, _loader(ds, 4), max_obj=8, score_thr=thr, class_weighted=True)
    assert torch.equal(_bits(store['unc'].cpu()), _bits(stage1))
    X_L_next, _ = update_X_L(unc, np.arange(N_POOL), X_L, budget, zeroRate=0)
    assert X_L_next.tolist() == sorted([0, 9] + torch.nonzero(unc).flatten().tolist())


def test_ssd_detector_raises():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_SSD.py'))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model).cuda().eval()

    class _L:
        batch_size, dataset, collate_fn = 2, [0] * 4, None
    with pytest.raises(NotImplementedError, match='follow-up'):
        apis.Posterior_uncertainty(cfg, model, _L(), class_weighted=True)
    with pytest.raises(NotImplementedError, match='follow-up'):
        apis.CCMS_uncertainty(cfg, model, _L(), X_L=[0], budget=1, class_weighted=True)
    cfg.model.bbox_head.class_difficulty = dict(CD)
    with pytest.raises(NotImplementedError, match='follow-up'):
        build_detector(cfg.model)
