"""SHA-256 digests of the learner's arenas after three minibatch steps, one line per configuration: two builds whose lines are equal
compute the same update bit for bit (the proof of a host-side refactor of the pass / apply layer).

Per configuration: an engine at B = 4, H = 48, W = 64, init_engine_parameters(seed=4), three steps on tests/util.make_batches(seed=21),
then one digest over params, adam_m, adam_v, grads, the two metrics buffers, get_optimizer_state() and, with train stats, the ring's rows.
Configurations: pass kind (separate / joint, stored action / re-sampled with seed 9, offset 3 + step) x gradient gate x frozen trunk, and
on top of the two stored kinds one of optimizer='nadam', train_stats=8, compute='bf16s', compute='bf16' (bf16 MFMA operands on float32
tensors); on top of separate-stored the update kernel's
forms (word `update`): every optimizer, Adam and Nadam with polyak=0.9, skip_nonfinite alone.  CDRL_GRAPH is the caller's.

    python tools/arena_digest.py                         (every configuration)
    python tools/arena_digest.py --only stored,gate=0    (the configurations whose line holds every given word)
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 4, 48, 64
STEPS = 3
KINDS = ('separate-stored', 'separate-resample', 'joint-stored', 'joint-resample')
GATE = dict(clip_mode='global', skip_nonfinite=True)


def configurations():
    """(label, pass kind, engine keywords)"""
    out = []
    for kind in KINDS:
        for gate in (0, 1):
            for frozen in (0, 1):
                out.append((f'{kind} gate={gate} frozen={frozen}', kind, dict(GATE if gate else {}, freeze_trunk=bool(frozen))))
    for kind in ('separate-stored', 'joint-stored'):
        for extra in (dict(optimizer='nadam'), dict(train_stats=8), dict(compute='bf16s'), dict(compute='bf16')):
            (k, v), = extra.items()
            out.append((f'{kind} {k}={v}', kind, extra))
    # the update kernel: every optimizer, polyak averaging, and the tensor-mode gate (skip_nonfinite alone: per-tensor clip)
    from carla_driving_rl_agent_amd import _lib
    extras = [dict(optimizer=o) for o in _lib.OPTIMIZERS]
    extras += [dict(optimizer=o, polyak=0.9) for o in ('adam', 'nadam')] + [dict(skip_nonfinite=True)]
    for extra in extras:
        label = ','.join(f'{k}={v}' for k, v in extra.items())
        out.append((f'separate-stored update {label}', 'separate-stored', extra))
    return out


def step(eng, kind, k, pol, val, joint):
    resample = dict(seed=9, offset=3 + k)
    if kind == 'separate-stored':
        eng.policy_forward_backward(pol)
    elif kind == 'separate-resample':
        eng.policy_forward_backward_resample(pol, **resample)
    elif kind == 'joint-stored':
        eng.joint_forward_backward(joint)
    else:
        eng.joint_forward_backward_resample(joint, **resample)
    if kind.startswith('joint'):
        eng.joint_apply()
        return
    eng.policy_apply()
    eng.value_forward_backward(val)
    eng.value_apply()


def digest(kind, kw, batches):
    import torch
    from carla_driving_rl_agent_amd import _lib
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    eng = LearnerEngine(B, device='cuda:0', H=H, W=W, **kw)
    init_engine_parameters(eng, seed=4)
    for k in range(STEPS):
        step(eng, kind, k, *batches)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (eng.params, eng.adam_m, eng.adam_v, eng.grads, eng.buffer(_lib.BUF_METRICS_P), eng.buffer(_lib.BUF_METRICS_V)):
        h.update(t.cpu().numpy().tobytes())
    h.update(repr(sorted(eng.get_optimizer_state().items())).encode())
    if kw.get('train_stats'):
        h.update(repr(eng.train_stats()).encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='', help='comma-separated words; a configuration runs when its line holds all of them')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('[arena_digest] needs a GPU')
    torch.cuda.set_device(0)
    from tests.util import make_batches, to_dev
    pol, val = make_batches(B, H, W, seed=21)
    dpol, dval = to_dev(pol), to_dev(val)
    batches = (dpol, dval, dict(dpol, returns=dval['returns']))
    words = [w for w in args.only.split(',') if w]
    for label, kind, kw in configurations():
        if all(w in label.split() or w in kind.split('-') for w in words):
            print(f'{label}: {digest(kind, kw, batches)}', flush=True)


if __name__ == '__main__':
    main()
