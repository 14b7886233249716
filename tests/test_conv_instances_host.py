"""The case table of tests/conv_instances_util.py against the dispatch, without a device (the CU count then counts as 256, the MI355X's):
every case's descriptor, built as hipops builds it, must get exactly the plan the case names from aod_conv2d_plan under the default
thresholds, and the cases together must name every tuple of the two X-macro lists that are the launch switch (csrc/conv.hip
CONV_IGEMM_INSTANCES, csrc/conv_x3p.hip X3P_INSTANCES).  A change that adds an instance without a case, or moves a rule so that a case no
longer reaches its instance, fails here before anything is launched."""
import pytest

from tests import conv_instances_util as U


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    build(verbose=False)
    from aod_meh_hua_amd._C import lib
    return lib


@pytest.fixture(autouse=True)
def default_dispatch():
    names = U.dispatch_variables_set()
    if names:
        pytest.fail(f'{names} set in the environment: the default plans are not what these cases reach')


@pytest.mark.parametrize('name', list(U.CASES))
def test_case_reaches_its_plan(lib, name):
    c = U.CASES[name]
    got = U.planned(name)
    assert got == c.plan, (name, dict(zip(U.PLAN_FIELDS, got)), dict(zip(U.PLAN_FIELDS, c.plan)))
    assert (c.plan[0] == U.PW) == (c.pw_tile is not None)
    rows = sum(b * ((h + 2 * (c.k // 2) - c.k) // c.stride + 1) * ((w + 2 * (c.k // 2) - c.k) // c.stride + 1) for b, h, w in c.segs)
    rows = sum(b * h * w for b, h, w in c.segs) if c.dgrad else rows
    assert rows <= 70000, f'{name}: a launch of {rows} rows'


def test_pointwise_mode_is_restored(lib):
    prev = lib.aod_set_pointwise_mode(-1)
    try:
        for name, c in U.CASES.items():
            if c.pw_mode is not None:
                U.planned(name)
                assert lib.aod_set_pointwise_mode(-1) == -1, name
    finally:
        lib.aod_set_pointwise_mode(prev)


def test_every_instance_has_a_case_and_every_case_an_instance():
    ig, xp = U.instance_lists()
    assert len(ig) == len(set(ig)) == 23 and all(len(t) == 7 for t in ig), ig
    assert len(xp) == len(set(xp)) == 10 and all(len(t) == 4 for t in xp), xp
    named = {'igemm': {}, 'x3p': {}}
    for name, c in U.CASES.items():
        inst = U.instance_of(c.plan)
        if inst is None:
            assert c.plan == U.PW_STREAM, name
            continue
        assert inst[1] in (ig if inst[0] == 'igemm' else xp), f'{name}: its plan names {inst}, which is in no instance list'
        named[inst[0]].setdefault(inst[1], []).append(name)
    missing = [t for t in ig if t not in named['igemm']] + [t for t in xp if t not in named['x3p']]
    assert not missing, f'instances no case reaches: {missing}'
    # the four tile forms of the streaming kernel (inferred, see conv_instances_util._case)
    assert {c.pw_tile for c in U.CASES.values() if c.pw_tile} == {(64, 64), (128, 64), (64, 128), (128, 128)}
