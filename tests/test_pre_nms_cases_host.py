"""Host-side guard of the pre-NMS edge cases (no GPU): the case builders of tests/pre_nms_util.py and the oracle only.  It asserts that the
preconditions which tests/test_gpu_pre_nms_edges.py relies on hold for the committed seeds, so that a seed change cannot silently turn an
edge test into a plain one: ties where ties are intended and none where they are not, every radix-select exit depth and the residual
histogram path reached, the decode's clamp and clip edges reached, the level gate's margins.  It also states, on a host restatement of the
kernel's key, that the section-1 cases tell a flipped tie rule and a cache read past its end from the correct kernel."""
import numpy as np
import pytest
import torch

from oracle import detect as odetect
from oracle.model import nhwc_flat
from tests import pre_nms_util as U


@pytest.mark.parametrize('A,k', U.TOPK_SHAPES)
def test_topk_rows_meet_their_preconditions(A, k):
    for dist in U.TOPK_DISTS:
        x = U.topk_scores(dist, A, k)
        assert x.dtype == torch.float32 and x.shape == (U.TOPK_B, A)
        assert bool(torch.isfinite(x).all()) and bool((x >= 0).all()) and not bool((x == 0).logical_and(torch.signbit(x)).any())
        _, exp = odetect.stable_topk(x, k)
        pairs, straddle = zip(*[U.tie_stats(x[b], k) for b in range(U.TOPK_B)])
        distinct = [len(torch.unique(x[b])) for b in range(U.TOPK_B)]
        print(f'{dist:12s} A={A} k={k}: tied pairs in the top k+1 {pairs}, k-th place straddled {straddle}, distinct values {distinct}')
        if dist in U.TIE_FREE_DISTS:
            assert distinct == [A] * U.TOPK_B, dist                                   # no two equal scores anywhere in the row
            _, exp64 = odetect.stable_topk(x.double(), k)
            assert torch.equal(exp, exp64), dist
        elif dist in ('const', 'two_level'):
            assert all(straddle), dist                                                # the tie group straddles the k-th place
        elif dist == 'edges':
            assert all(p >= 1 for p in pairs), dist                                   # the planted 1.0s
            assert all(float(x[b].min()) == 0.0 and float(x[b].max()) == 1.0 for b in range(U.TOPK_B))
            assert all(bool((x[b] == U.FLT_MIN).any()) and bool(((x[b] > 0) & (x[b] < U.FLT_MIN)).any()) for b in range(U.TOPK_B))
        else:                                                                         # quantised, ulp_cluster: at most 9 / 256 values
            assert all(d <= 256 for d in distinct) and (k == 1 or all(p >= 1 for p in pairs)), dist
        if dist == 'const':
            assert torch.equal(exp, torch.arange(k)[None].expand(U.TOPK_B, k))
        if dist == 'ramp_up':
            assert bool((exp[:, 0] == A - 1).all())
            if A > U.CACHE_N + k:
                assert bool((exp >= U.CACHE_N).all())                                 # every winner lies in the uncached tail
        # the host restatement of the key orders as the oracle does; the two hand-made errors do not
        for b in range(U.TOPK_B):
            e = exp[b].numpy()
            assert np.array_equal(U.host_topk(x[b], k), e), dist
            if dist in ('const', 'two_level') and k < A:
                assert not np.array_equal(U.host_topk(x[b], k, tie='high'), e), dist           # `| i` in place of `| (0xffffffff - i)`
            if A > U.CACHE_N and dist in ('uniform', 'ramp_up', 'edges'):
                assert not np.array_equal(U.host_topk(x[b], k, ncache=U.CACHE_N), e), dist      # s_cache[i] read for i >= ncache


def test_radix_select_paths_are_reached():
    """whole_bin exit at every pass depth that a row of these sizes can reach, and waves with more than two distinct digits (the residual
    atomics of hist_add) next to waves with one (the leader rounds)"""
    exits = set()
    for p, A, k in U.EXIT_CASES:
        x = U.exit_scores(p, A, k)
        assert bool(torch.isfinite(x).all()) and bool((x > 0).all())
        for b in range(U.TOPK_B):
            kth, got, _ = U.radix_trace(x[b], k)
            assert got == p, (p, got)
            assert int((U.topk_keys(x[b]) >= np.uint64(kth)).sum()) == k            # the early exit's threshold selects exactly k keys
        exits.add(p)
    _, p, waves = U.radix_trace(U.topk_scores('const', 1025, 1024)[0], 1024)
    assert p == 1 and max(waves.values()) <= 2
    exits.add(p)
    _, p, waves = U.radix_trace(U.topk_scores('const', 2304, 1000)[0], 1000)
    assert p == 0 and waves[0] == 64 and all(waves[q] == 1 for q in range(1, 8))    # only the last index byte separates the 1000th key
    exits.add(p)
    assert exits == {7, 6, 5, 4, 2, 1, 0}
    _, _, waves = U.radix_trace(U.topk_scores('uniform', 2304, 1000)[1], 1000)
    assert max(waves.values()) > 2
    _, _, waves = U.radix_trace(U.topk_scores('quantised', 2304, 1000)[0], 1000)
    assert max(waves.values()) > 2
    _, _, waves = U.radix_trace(U.topk_scores('ulp_cluster', 2304, 1000)[0], 1000)
    assert waves[7] == waves[6] == waves[5] == 1 and waves[4] > 2                   # dominant bin on the three high passes, one high-entropy pass


def test_case_list_covers_what_the_issue_names():
    ids = [U.case_id(c) for c in U.CASES]
    assert len(set(ids)) == len(ids)
    have = {(c[2], c[3]) for c in U.CASES}
    assert {(20, False), (21, True), (80, False), (81, True), (1, False)} <= have
    assert any(not c[4] and c[2] == 20 for c in U.CASES)
    assert {c[5] for c in U.CASES if c[0] == 'five' and c[2] in (20, 21)} == set('abcd')
    five, big, seven = (U.build_case(next(c for c in U.CASES if c[0] == n)) for n in ('five', 'big', 'seven'))
    assert five['A'] == [2295, 648, 180, 54, 18] and U.ks_of(five) == [100, 100, 100, 54, 18]
    assert big['A'] == [37422] and big['A'][0] > U.CACHE_N and big['B'] == 2 and U.ks_of(big) == [1000]
    assert len(seven['A']) == 7 and all(a % 2 == 1 for a in seven['A'])
    assert 648 % 256 != 0


@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_pre_nms_case_meets_its_preconditions(case):
    c, ref = U.build_case(case), U.reference(case)
    B, C = c['B'], c['C']
    ks = U.ks_of(c)
    assert len({tuple(s) for s in c['img_shapes']}) == B
    # the row reference is the oracle's statement (same bits) wherever the oracle offers the mode
    if not c['has_bg']:
        flat = lambda xs, n: [nhwc_flat(x, n) for x in xs]
        o = odetect.pre_nms(flat(c['cls'], C), flat(c['reg'], 4), [nhwc_flat(x, 1)[..., 0] for x in c['lam']], c['anchors'], c['img_shapes'],
                            c['scale_factors'], nms_pre=c['nms_pre'], num_classes=C)
        for l in range(len(ks)):
            assert torch.equal(o['rowmax'][l], ref['rowmax32'][l])
            assert torch.equal(o['level_any_fg'][l], ref['level_any_fg'][l])
    # level gate: no row within the rounding bound of the threshold
    bound = 4 * max(ref['e_rowmax'], ref['e_alpha'])
    print(f"{U.case_id(case)}: e_rowmax {ref['e_rowmax']:.3g} e_alpha {ref['e_alpha']:.3g} e_scores {ref['e_scores']:.3g} "
          f"e_boxes(rel) {ref['e_boxes']:.3g} gate margin {ref['gate_margin']:.3g}")
    assert ref['e_rowmax'] > 0 and ref['e_scores'] > 0 and ref['e_boxes'] > 0
    assert ref['gate_margin'] > bound
    fg = torch.stack(ref['level_any_fg'])                      # [L, B]
    if c['recipe'] == 'd':
        want = torch.zeros_like(fg)
        want[1, 1] = True
        assert torch.equal(fg, want)
        assert float(ref['max_alpha'][1][1, -1]) > 0.9 and c['A'][1] % 256 != 0
    # decode edges, on the oracle's own selection
    sel = U.oracle_selection(case)
    shares = U.edge_shares(ref, sel)
    print('   edge shares of the selected rows:', {k: round(v, 3) for k, v in shares.items()})
    assert all(v > 0.02 for v in shares.values()), shares
    # ties in the ranked row max
    for l, (A, k) in enumerate(zip(c['A'], ks)):
        if k == A:
            continue
        stats = [U.tie_stats(ref['rowmax32'][l][b], k) for b in range(B)]
        print(f'   level {l} A={A} k={k}: (tied pairs in the top k+1, straddle) {stats}')
        if C == 1 or (c['recipe'] == 'b' and l == 0):
            assert all(s == (k, True) for s in stats)                     # one value over the whole level
            assert torch.equal(sel[l], torch.arange(k)[None].expand(B, k))
        elif c['recipe'] == 'c' and C <= 21:
            assert all(s[0] > 0 for s in stats), stats
