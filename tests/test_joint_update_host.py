"""Joint policy + value update on the host: the four new C entry points (header, library, ctypes signatures), a planner that adds
no scratch for them, and the gradient slices DataParallelLearner.joint_step reduces.  No GPU."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = ('cdrl_learner_joint_forward_backward', 'cdrl_learner_joint_forward_backward_resample', 'cdrl_learner_joint_apply',
         'cdrl_bn_small_bwd_pair')


def _engine(B, **kw):
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    return LearnerEngine(B, device=None, **kw)


def test_header_declares_and_library_exports_the_calls():
    from carla_driving_rl_agent_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cdrl.h')).read()
    lib = _lib.load()
    for name in CALLS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        fn = getattr(lib, name)         # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes is not None, name
    # argument counts as the header spells them: (l, batch, returns, grad_scale, stream), (... seed, offset ...), (l, stream), and
    # 3 tensors + M, C + 2 statistics blocks + 6 per-BatchNorm outputs + dx + stream
    assert [len(getattr(lib, n).argtypes) for n in CALLS] == [5, 7, 2, 15]
    assert lib.cdrl_learner_joint_forward_backward_resample.argtypes[3:5] == [C.c_uint64, C.c_uint64]


def test_header_states_what_differs_from_the_reference():
    header = open(os.path.join(ROOT, 'include', 'cdrl.h')).read()
    start = header.index('joint policy + value update')
    text = ' '.join(header[start:header.index('int cdrl_learner_joint_apply', start)].split())
    for phrase in ('ONE trunk optimizer step per minibatch', 'moving statistics are updated once',
                   'policy total loss + value total loss', 'B > 2048', 'clipped once, by its own threshold'):
        assert phrase in text, phrase


# workspace_bytes of the two BASELINE shapes as DESIGN.md records them for the planner before this feature: the joint pass reuses
# the tensors of the separate passes and allocates nothing
@pytest.mark.parametrize('B,kw,expect', [(256, dict(H=90, W=120), 7271345664),
                                         (1024, dict(H=90, W=120, compute='bf16s'), 13925212160)])
def test_planner_adds_no_scratch(B, kw, expect):
    assert _engine(B, **kw).workspace_bytes == expect


@pytest.mark.parametrize('frozen', [False, True])
def test_joint_step_slices(frozen):
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner
    eng = _engine(32, H=48, W=64, freeze_trunk=frozen)
    dp = DataParallelLearner(eng)
    p0, pn = eng.region('policy', True)
    t0, tn = eng.region('trunk', True)
    v0, vn = eng.region('value', True)
    total = eng.grads_total
    assert total == pn + tn + vn

    def exact_cover(slices, want):
        """`slices` are disjoint and their union is exactly the union of `want`."""
        got = sorted((lo, hi) for lo, hi in slices if hi > lo)
        for (_, hi), (lo, _) in zip(got, got[1:]):
            assert hi <= lo, got          # no element twice
        merged = []
        for lo, hi in got:
            if merged and merged[-1][1] == lo:
                merged[-1] = (merged[-1][0], hi)
            else:
                merged.append((lo, hi))
        assert merged == want, (merged, want)

    heads = [(p0, p0 + pn), (v0, v0 + vn)]
    if frozen:
        assert dp._comm is None
        exact_cover(dp._joint_slices, heads)
    else:
        # without a communication stream: the whole arena as one slice; with one: the early group plus the tower slice
        exact_cover(dp._joint_slices, [(0, total)])
        tower_n = eng.tail_offset()
        assert dp._joint_early == [(0, pn), (t0 + tower_n, t0 + tn + vn)]
        exact_cover(dp._joint_early + [dp._tower], [(0, total)])
