"""GPU: the MC-dropout baseline -- the factor kernel against its numpy restatement (exact), the in-place apply kernel against torch
(exact, both arithmetic modes' layouts), the dropout forward against the oracle under the same masks, replay against eager (bits), and
the pool pass apis.MCDropout_uncertainty against a float64 evaluation of the mutual-information formula on the product's own maps."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import synth
from tests.ensemble_mi_util import bound, mi_float64, mi_fp32_torch
from tests.mc_dropout_util import keep_scale, masks_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREC = os.environ.get('AOD_CONV_PREC', 'bf16x3')


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('rate', [0.0, 0.1, 0.5])
def test_mask_kernel_equals_the_numpy_restatement(rate):
    from aod_meh_hua_amd import hipops as ho
    ids, channels = [0, 7, 4000000000], [64, 20, 256]            # (20: not a multiple of 4 -- the last quad is partial and the next site misaligned)
    T = sum(channels)
    offs = torch.tensor([0, 64, 84], dtype=torch.int32).cuda()
    dev_ids = torch.tensor(ids, dtype=torch.int64).cuda()
    got = {}
    for sample in (0, 3):
        table = torch.full((4, T), -7.0, device='cuda')          # (one row more than images: it must stay untouched)
        ho.dropout2d_masks(table, dev_ids, offs, rate, 0x1234567887654321, sample)
        want = masks_numpy(ids, channels, rate, 0x1234567887654321, sample)
        got[sample] = table.cpu().numpy()
        assert np.array_equal(got[sample][:3], want), (rate, sample)
        assert (got[sample][3] == -7.0).all()
        assert np.isin(want, [np.float32(0), keep_scale(rate)]).all()
        alone = torch.zeros(1, T, device='cuda')
        ho.dropout2d_masks(alone, dev_ids[1:2].clone(), offs, rate, 0x1234567887654321, sample)
        assert np.array_equal(alone.cpu().numpy()[0], got[sample][1])                # image 7 alone = image 7 in the batch
    if rate == 0.0:
        assert (got[0][:3] == 1.0).all()
    else:
        assert (got[0][:3] != got[3][:3]).mean() > 0.05


def _x_cols(C):
    c = torch.arange(C)
    head = (c // 32) * 64 + c % 32
    return head, head + 32


def _apply_reference(x_rows, f_rows, C, x3):
    """x_rows [M, width] bf16 (CPU), f_rows [M, C] fp32: the product definition in torch ops"""
    if not x3:
        return (x_rows.float() * f_rows).bfloat16()
    head, tail = _x_cols(C)
    out = x_rows.clone()
    h, l = x_rows[:, head], x_rows[:, tail]
    w = (h.float() + l.float()) * f_rows
    nh = w.bfloat16()
    nl = (w - nh.float()).bfloat16()
    keep = f_rows == 1.0                                      # a factor of exactly 1 leaves the (head, tail) bits alone
    out[:, head] = torch.where(keep, h, nh)
    out[:, tail] = torch.where(keep, l, nl)
    return out


@pytest.mark.parametrize('x3, C, col0', [(False, 64, 16), (False, 64, 17), (True, 20, 16), (True, 20, 3), (True, 256, 40), (True, 256, 41)])
def test_apply_kernel_equals_torch_in_place(x3, C, col0):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    AF.set_precision('bf16x3' if x3 else 'bf16')
    B, H, W = 2, 3, 5                                          # HW = 15: image boundaries fall inside a workgroup's stride
    g = torch.Generator().manual_seed(C + col0)
    vals = torch.randn(B * H * W, C, generator=g) * 3
    x = ho.x3_split(vals.cuda()) if x3 else vals.bfloat16().cuda()
    assert tuple(x.shape) == (B * H * W, ho.width(C))
    table = torch.full((B + 1, 400), float('nan'))            # row stride 400 > C; everything outside the slice is poison
    f = torch.tensor(masks_numpy([5, 9], [C], 0.5, 11, 0))
    f[0, :3] = 1.0                                             # (a factor of one beside zeros and twos)
    f[1, C // 2] = 0.3
    table[:B, col0:col0 + C] = f
    before = x.cpu().clone()
    ret = ho.dropout2d_apply(x, table.cuda(), col0, B, H * W, C)
    assert ret.data_ptr() == x.data_ptr()
    want = _apply_reference(before, f.repeat_interleave(H * W, 0), C, x3)
    got = x.cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not torch.isnan(got.float()).any()
    if x3 and C % 32:
        head, tail = _x_cols(32)
        assert (got[:, head[C:]] == 0).all() and (got[:, tail[C:]] == 0).all()           # pad columns stay zero
    assert (got.float() == 0).any() and (got.float() != 0).any()


@pytest.mark.parametrize('x3', [False, True])
def test_multi_segment_apply_equals_one_launch_per_level(x3):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    AF.set_precision('bf16x3' if x3 else 'bf16')
    B, C, hws = 3, 64, [15, 6, 1]                              # three 'levels' as adjacent row ranges of one buffer, 3 rows of slack between
    row0, r = [], 2
    for hw in hws:
        row0.append(r)
        r += B * hw + 3
    g = torch.Generator().manual_seed(3)
    vals = torch.randn(r, C, generator=g)
    x = ho.x3_split(vals.cuda()) if x3 else vals.bfloat16().cuda()
    table = torch.tensor(masks_numpy([1, 2, 3], [C, 7, C, C], 0.5, 5, 1)).cuda()
    offs = [0, C + 7, 2 * C + 7]
    one = x.clone()
    for r0, hw, off in zip(row0, hws, offs):
        ho.dropout2d_apply(one[r0:r0 + B * hw], table, off, B, hw, C)
    ho.dropout2d_apply_multi(x, table, B, list(zip(row0, hws, offs)), C)
    assert torch.equal(x.view(torch.int16), one.view(torch.int16))
    keep = torch.ones(r, dtype=torch.bool)
    for r0, hw in zip(row0, hws):
        keep[r0:r0 + B * hw] = False
    before = ho.x3_split(vals.cuda()) if x3 else vals.bfloat16().cuda()
    assert torch.equal(x[keep.cuda()].view(torch.int16), before[keep.cuda()].view(torch.int16))         # the slack rows are untouched


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.fixture(scope='module')
def built():
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    sd = om.seeded_state_dict()
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    sites = AF.dropout_sites(model)
    return model, sd, sites


def _forward(model, sites, img, ids, rate, seed, sample, table=None):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    table = torch.ones(img.shape[0], sites.T, device='cuda') if table is None else table
    ho.dropout2d_masks(table, ids, sites.offsets(img.device), rate, seed, sample)
    H, W = img.shape[-2:]
    with torch.no_grad():
        out = model(img=[img], img_metas=[synth.metas(img.shape[0], H, W)], return_loss=False, rescale=True, isEval=True, justOut=True,
                    mc_dropout=AF.MCDropoutState(table, sites))
    return [t.clone() for t in out], table


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize('prec', ['bf16', 'bf16x3'])
def test_dropout_forward_matches_the_oracle_under_the_same_masks(built, monkeypatch, prec):
    """Tolerances: those of the no-dropout forward parity of each mode on the classification maps (max |a - b| / max |b|) --
    bf16: 3e-2 (tests/test_gpu_model.py:60), bf16x3: 2e-4 (tests/test_gpu_precision_x3.py:74)."""
    from aod_meh_hua_amd import functional as AF
    from oracle import model as om
    model, sd, sites = built
    AF.set_precision(prec)
    tol = 3e-2 if prec == 'bf16' else 2e-4
    img = synth.images(2, 64, 64, seed=5)
    ids = torch.tensor([3, 4000000001], dtype=torch.int64).cuda()
    got, table = _forward(model, sites, img.cuda(), ids, 0.5, 9, 2)
    tab = table.cpu()
    assert 0.4 < float((tab == 0).float().mean()) < 0.6
    f = {k: tab[:, off:off + ch] for k, (_, off, ch) in sites.items()}
    used = set()

    def relu_dropout(z, key):
        if key not in f:
            return F.relu(z)
        used.add(key)
        return F.relu(z) * f[key][:, :, None, None]
    monkeypatch.setattr(om, '_relu', relu_dropout)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        want = om.head_forward(sd, om.fpn(sd, om.backbone(sd, img)))[0]
        monkeypatch.undo()
        plain = om.head_forward(sd, om.fpn(sd, om.backbone(sd, img)))[0]
    assert used == set(sites)
    assert len(got) == len(want) == 5
    for l, (a, b, p) in enumerate(zip(got, want, plain)):
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape)
        r, moved = _rel(a.cpu().numpy(), b.numpy()), _rel(p.numpy(), b.numpy())
        print(f'{prec} level {l}: dropout forward vs oracle under the same masks {r:.3e} (tolerance {tol:.0e}); the masks move the maps by {moved:.3e}')
        assert r < tol, (prec, l, r)
        assert moved > 10 * tol                                 # the comparison is not vacuous: without the masks the maps are elsewhere


@pytest.mark.parametrize('prec', ['bf16', 'bf16x3'])
def test_rate_zero_equals_the_plain_unfused_forward_bit_for_bit(built, monkeypatch, prec):
    from aod_meh_hua_amd import functional as AF
    model, sd, sites = built
    AF.set_precision(prec)
    img = synth.images(2, 64, 64, seed=6).cuda()
    ids = torch.tensor([0, 1], dtype=torch.int64).cuda()
    got, table = _forward(model, sites, img, ids, 0.0, 9, 0)
    assert bool((table == 1).all())
    for k in ('AOD_FUSE_BOTTLENECK', 'AOD_FUSE_BOTTLENECK128', 'AOD_GROUP_TOWERS'):      # the existing switches: three launches per block, one
        monkeypatch.setenv(k, '0')                                                        # launch per tower conv
    with torch.no_grad():
        plain = model(img=[img], img_metas=[synth.metas(2, 64, 64)], return_loss=False, rescale=True, isEval=True, justOut=True)
    for a, b in zip(got, plain):
        assert torch.equal(a, b)


def test_replay_equals_eager_bit_for_bit(built):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd.graphs import GraphedScore
    model, sd, sites = built
    img = synth.images(2, 64, 64, seed=7).cuda()
    ids = torch.tensor([10, 11], dtype=torch.int64).cuda()
    mt = synth.metas(2, 64, 64)
    eager = [_forward(model, sites, img, ids, 0.1, 21, k)[0] for k in range(3)]
    table = torch.ones(2, sites.T, device='cuda')
    gs = GraphedScore(model, rescale=True, isEval=True, justOut=True, mc_dropout=AF.MCDropoutState(table, sites))
    from aod_meh_hua_amd import hipops as ho
    replay = []
    for k in range(3):                                          # ONE capture (k = 0), then replays: only the table changes in between
        ho.dropout2d_masks(table, ids, sites.offsets(img.device), 0.1, 21, k)
        replay.append([t.clone() for t in gs(img, mt, ids)])
    assert len(gs.cache) == 1
    for k in range(3):
        for a, b in zip(eager[k], replay[k]):
            assert torch.equal(a, b), k
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert not any(torch.equal(a, b) for a, b in zip(eager[i], eager[j]))


# ---------------------------------------------------------------------------------------------------------------- the pool pass
def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


@pytest.fixture(scope='module')
def pool():
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd.datasets import build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.load_state_dict(om.seeded_state_dict(cls_bias=-2.0), strict=True)
    model = MMDataParallel(model.cuda()).eval()
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=6, size=(64, 64)), dict(test_mode=True))
    return cfg, model, ds, AF.dropout_sites(model)


def _float64_reference(model, sites, ds, n, rate, seed, n_cls=20):
    """the float64 formula on the product's own maps, taken eagerly sample by sample in batches of 3 -> (score [N], bound)"""
    from aod_meh_hua_amd.apis.test import _unwrap
    scores, e_ref, totals, pos = [], 0.0, [], 0
    for data in _loader(ds, 3):
        img = data['img']
        while not torch.is_tensor(img):                           # (test-mode batches: [DataContainer / tensor])
            img = img[0] if isinstance(img, (list, tuple)) else _unwrap(img)
        img = img.cuda()
        ids = torch.arange(pos, pos + img.shape[0], dtype=torch.int64).cuda()
        pos += img.shape[0]
        members = [[t.cpu().contiguous().numpy() for t in _forward(model, sites, img, ids, rate, seed, k)[0]] for k in range(n)]
        want, tm = mi_float64(members, n_cls)
        fp32 = mi_fp32_torch([[torch.from_numpy(t) for t in m] for m in members], n_cls).double().numpy()
        e_ref = max(e_ref, float(np.abs(fp32 - want).max()))
        scores.append(want)
        totals.append(tm)
    return np.concatenate(scores), bound(e_ref, float(np.mean(totals)))


def test_pool_pass_is_batch_invariant_and_matches_float64(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    cfg, model, ds, sites = pool
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    got4 = apis.MCDropout_uncertainty(cfg, model, _loader(ds, 4), n=4, rate=0.1, seed=3)
    got3 = apis.MCDropout_uncertainty(cfg, model, _loader(ds, 3), n=4, rate=0.1, seed=3)
    assert got4.shape == (6,) and got4.dtype == torch.float32 and not got4.is_cuda
    assert torch.equal(got4, got3)
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    assert torch.equal(apis.MCDropout_uncertainty(cfg, model, _loader(ds, 3), n=4, rate=0.1, seed=3), got4)          # eager = replayed
    want, tol = _float64_reference(model, sites, ds, 4, 0.1, 3)
    err = np.abs(got4.double().numpy() - want).max()
    print(f'MC-dropout pool pass: scores {got4.tolist()}, max |pass - float64| = {err:.3e}, bound {tol:.3e}')
    assert want.min() > 1e-6                                    # the samples do disagree
    assert err <= tol
    assert not torch.equal(apis.MCDropout_uncertainty(cfg, model, _loader(ds, 3), n=4, rate=0.1, seed=4), got4)      # the seed matters


def test_rate_zero_scores_zero(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    cfg, model, ds, sites = pool
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    got = apis.MCDropout_uncertainty(cfg, model, _loader(ds, 3), n=4, rate=0.0, seed=3)
    want, tol = _float64_reference(model, sites, ds, 4, 0.0, 3)
    assert np.abs(want).max() < 1e-12                           # identical members carry no mutual information
    err = np.abs(got.double().numpy()).max()
    print(f'rate 0: max |score| = {err:.3e}, bound {tol:.3e}')
    assert err <= tol
