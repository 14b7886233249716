"""CPU tests (no GPU) of the plumbing the four pool drivers of apis/test.py share: _PoolPass (shard, global image ids, loader, gather) on
torch.device('cpu') over a fake 23-item dataset, and the graph-cache helper's key builder and gates.  What the drivers compute with it is
pinned bit for bit by the GPU suites (test_gpu_pool.py, test_gpu_ensemble_mi.py, test_gpu_mc_dropout.py, test_gpu_eval_device.py)."""
import pytest
import torch

from aod_meh_hua_amd import parallel
from aod_meh_hua_amd.apis import test as apis_test

N = 23
CPU = torch.device('cpu')


class _Items:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {'img': [torch.full((3, 2, 2), float(i))], 'img_metas': [[{'idx': i}]], 'gt_bboxes': None}


def _collate(items):
    return {'img': [torch.stack([it['img'][0] for it in items])], 'img_metas': [[it['img_metas'][0][0] for it in items]],
            'gt_bboxes': [it['gt_bboxes'] for it in items]}


class _Loader:
    num_workers = 0
    collate_fn = staticmethod(_collate)

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, batch_size


def _run(monkeypatch, rank, world, bs, interleaved, n=N, **kw):
    monkeypatch.setattr(apis_test, 'get_dist_info', lambda: (rank, world))
    pool = apis_test._PoolPass(_Loader(_Items(n), bs), CPU, interleaved)
    return pool, list(pool.batches(**kw))


@pytest.mark.parametrize('rank,world', [(0, 1), (0, 2), (1, 2), (0, 3), (2, 3)])
def test_batches_ids_and_images(monkeypatch, rank, world):
    for bs in (1, 5, 16, 23, 32):
        for interleaved in (False, True):
            pool, got = _run(monkeypatch, rank, world, bs, interleaved)
            want = parallel.shard_batches(N, bs, rank, world, interleaved)
            assert [idxs for idxs, _, _ in got] == want
            assert (pool.N, pool.bs, pool.rank, pool.world) == (N, bs, rank, world)
            assert pool.my_idx == [i for b in want for i in b] and pool.prog_bar.completed == len(pool.my_idx)
            for idxs, image_ids, data in got:
                assert image_ids.dtype == torch.int64 and image_ids.tolist() == idxs           # GLOBAL ids
                assert sorted(data) == ['img', 'img_metas']
                assert len(data['img']) == 1 and data['img'][0].shape == (len(idxs), 3, 2, 2)
                assert data['img'][0][:, 0, 0, 0].tolist() == [float(i) for i in idxs]
                assert (data['img'][0] == data['img'][0][:, :1, :1, :1]).all()
                assert [m['idx'] for m in data['img_metas'][0]] == idxs


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('interleaved', [False, True])
def test_ranks_cover_the_pool_exactly_once(monkeypatch, world, interleaved):
    for bs in (1, 5, 16, 23, 32):
        seen = [i for r in range(world) for idxs, _, _ in _run(monkeypatch, r, world, bs, interleaved)[1] for i in idxs]
        assert sorted(seen) == list(range(N)) and len(seen) == N


def test_empty_pool(monkeypatch):
    for interleaved in (False, True):
        pool, got = _run(monkeypatch, 0, 1, 5, interleaved, n=0)
        assert got == [] and pool.all_ids.numel() == 0
        z = pool.cat([])
        assert z.shape == (0,) and z.dtype == torch.float32
        assert pool.gather(z).shape == (0,)
    assert torch.equal(pool.cat([torch.ones(2), torch.zeros(1)]), torch.tensor([1., 1., 0.]))


def test_gather_takes_the_partitions_route(monkeypatch):
    calls = []
    for name in ('gather_scores', 'gather_scores_indexed'):
        monkeypatch.setattr(apis_test, name, lambda *a, _f=getattr(parallel, name), _n=name, **k: calls.append((_n, a[1:], k)) or _f(*a, **k))
    score = lambda idx: torch.tensor([1.5 * i + 1 for i in idx])
    # world 1: dataset order either way
    for interleaved, name in ((False, 'gather_scores'), (True, 'gather_scores_indexed')):
        pool, _ = _run(monkeypatch, 0, 1, 5, interleaved)
        del calls[:]
        assert torch.equal(pool.gather(score(pool.my_idx)), score(range(N)))
        assert [c[0] for c in calls] == [name]
    assert calls[0][1:] == ((list(range(N)), N), {'per': 25})               # ceil(ceil(23 / 5) / 1) * 5 slots
    # a rank's strided batches are NOT a block of the pool: its scores come back at their global positions (this process is world 1
    # for parallel's own collectives, so the other rank's slots stay 0)
    pool, _ = _run(monkeypatch, 1, 2, 5, True)
    assert pool.my_idx == list(range(5, 10)) + list(range(15, 20))
    del calls[:]
    full = pool.gather(score(pool.my_idx))
    want = torch.zeros(N)
    want[pool.my_idx] = score(pool.my_idx)
    assert torch.equal(full, want) and not torch.equal(full[:10], score(pool.my_idx))
    assert calls == [('gather_scores_indexed', (pool.my_idx, N), {'per': 15})]    # ceil(ceil(23 / 5) / 2) * 5 slots


class _DevicePool(_Items):
    size = (2, 2)

    def device_batch(self, idxs, device, image_ids=None, out=None):
        self.outs.append(out)
        return {'img': [torch.zeros(len(idxs), 3, 2, 2)], 'img_metas': [[{'idx': i} for i in idxs]]}


def test_device_generated_pool_and_static_image(monkeypatch):
    monkeypatch.setattr(apis_test, 'get_dist_info', lambda: (0, 1))
    ds = _DevicePool(7)
    ds.outs = []
    asked = []
    got = list(apis_test._PoolPass(_Loader(ds, 4), CPU).batches(static_image=lambda shape: asked.append(shape) or ('buf', shape)))
    assert [idxs for idxs, _, _ in got] == [[0, 1, 2, 3], [4, 5, 6]]
    assert asked == [(4, 3, 2, 2), (3, 3, 2, 2)] and ds.outs == [('buf', s) for s in asked]
    ds.outs = []
    assert len(list(apis_test._PoolPass(_Loader(ds, 4), CPU).batches())) == 2 and ds.outs == [None, None]
    # the evaluation pass reads the host loader whatever the dataset offers
    ds.outs = []
    got = list(apis_test._PoolPass(_Loader(ds, 4), CPU, device_batch=False).batches())
    assert ds.outs == [] and got[1][2]['img'][0][:, 0, 0, 0].tolist() == [4., 5., 6.]


def test_option_key():
    key = apis_test._option_key
    assert key(dict(isUnc='Epistemic', uPool2='x', scaleUnc=False)) == key(dict(scaleUnc=False, uPool2='x', isUnc='Epistemic'))
    assert key({}) == ()
    assert len({key(dict(a=1)), key(dict(a=1.0)), key(dict(a=True))}) == 3          # 1 == 1.0 == True, and they hash alike
    assert key(dict(a=None, b='s')) == (('a', 'NoneType', None), ('b', 'str', 's'))
    assert key(dict(a=torch.zeros(1))) is None and key(dict(a=[1])) is None


class _Model:
    pass


def test_graph_cache_gates_and_keys(monkeypatch):
    from aod_meh_hua_amd import graphs
    built = []

    class Fake:
        def __init__(self, model, **kw):
            built.append((model, kw))
    monkeypatch.setattr(graphs, 'GraphedScore', Fake)
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    m, gpu = _Model(), torch.device('cuda')
    kw = dict(isUnc=False, n=1)
    # no graph, no error, nothing built or cached
    assert apis_test._graphed(m, gpu, (), dict(kw, t=torch.zeros(1)), isEval=True) is None
    assert apis_test._graphed(m, CPU, (), kw, isEval=True) is None
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    assert apis_test._graphed(m, gpu, (), kw, isEval=True) is None
    assert built == [] and m not in apis_test._GSCORE
    monkeypatch.setenv('AOD_HIP_GRAPH', '1')
    g = apis_test._graphed(m, gpu, (), kw, isEval=False, batchIdx=0)
    assert built == [(m, dict(rescale=True, isEval=False, batchIdx=0, isUnc=False, n=1))]
    assert apis_test._graphed(m, gpu, (), dict(n=1, isUnc=False), isEval=False, batchIdx=0) is g and len(built) == 1
    e = apis_test._graphed(m, gpu, ('eval_padded',), kw, isEval=True, _padded=True)
    j = [apis_test._graphed(m, gpu, ('just_out', k), kw, isEval=True, justOut=True) for k in (0, 1)]
    assert len({id(x) for x in [g, e] + j}) == 4
    opts = apis_test._option_key(kw)
    assert apis_test._GSCORE[m] == {opts: g, ('eval_padded',) + opts: e, ('just_out', 0) + opts: j[0], ('just_out', 1) + opts: j[1]}
    assert len(apis_test._GSCORE[m]) == 4 and apis_test._graphed(m, gpu, (), dict(kw, n=1.0), isEval=False, batchIdx=0) is not g
    # a caller's own cache (the MC-dropout entry) is used instead of _GSCORE
    own = {'table': None}
    d = apis_test._graphed(m, gpu, ('graph',), kw, cache=own, isEval=True, justOut=True, mc_dropout='state')
    assert own[('graph',) + opts] is d and len(apis_test._GSCORE[m]) == 5 and built[-1][1]['mc_dropout'] == 'state'
