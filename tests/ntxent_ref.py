"""Float64 PyTorch restatement of the NT-Xent objective (cdrl_ntxent_loss / cdrl_learner_repr_forward_backward, include/cdrl.h;
DESIGN.md 6.11), differentiated by autograd, and the input recipe of the kernel tests.

  ntxent         loss and metric slots on embeddings z (B, D), rows i and i + B/2 the two views of one observation
  ntxent_grad    ... with dL/dz
  make_views     the seeded inputs every kernel test uses
  repr_grads     the representation pass on an OracleLearner: train-mode trunk, NT-Xent on its output, trunk gradients"""
import numpy as np
import torch

from oracle import model as OM


def ntxent(z, temperature):
    """-> (L, [L, top-1 accuracy, pair cosine, negatives' cosine, mean norm, temperature] as floats)."""
    B = z.shape[0]
    N = B // 2
    zn = torch.nn.functional.normalize(z, dim=1, eps=1e-12)
    cos = zn @ zn.t()
    s = cos / temperature
    eye = torch.eye(B, dtype=torch.bool)
    pair = torch.roll(eye, N, dims=1)                       # pair[i, (i + N) mod B]
    lse = torch.logsumexp(s.masked_fill(eye, float('-inf')), dim=1)
    L = (lse - s[pair]).mean()
    neg = ~(eye | pair)
    sd, cd, zd = s.detach(), cos.detach(), z.detach()
    hit = sd[pair] > sd.masked_fill(~neg, float('-inf')).max(dim=1).values if B > 2 else torch.ones(B, dtype=torch.bool)
    neg_cos = float(cd[neg].mean()) if B > 2 else 0.0
    return L, [float(L.detach()), float(hit.double().mean()), float(cd[pair].mean()), neg_cos, float(zd.norm(dim=1).mean()),
               float(temperature)]


def ntxent_grad(z, temperature, dtype=torch.float64):
    """z: numpy (B, D).  -> (dL/dz as numpy, metric slots), computed in `dtype` on the CPU."""
    zt = torch.tensor(np.asarray(z), dtype=dtype, requires_grad=True)
    L, slots = ntxent(zt, temperature)
    L.backward()
    return zt.grad.numpy(), slots


def make_views(B, D, seed=0, noise=1.0):
    """A seeded base (N, D), two views base + noise (unit noise), every row scaled by exp(normal).  float32 (B, D)."""
    rng = np.random.default_rng(1000 * B + D + seed)
    N = B // 2
    base = rng.standard_normal((N, D))
    z = np.concatenate([base + noise * rng.standard_normal((N, D)), base + noise * rng.standard_normal((N, D))], axis=0)
    return (z * np.exp(rng.standard_normal((B, 1)))).astype(np.float32)


def repr_grads(learner, states, temperature):
    """The representation pass on an OracleLearner (tests/util.make_pair): states = dict of numpy arrays.
    -> (L, trunk gradients, metric slots, the trunk's output)."""
    b = learner._cast(dict(states=states))
    d = OM.dynamics_forward(b['states'], learner.trunk, learner.cfg, training=True)
    L, slots = ntxent(d, temperature)
    return L, learner._grads(L, learner.trunk, learner.tspec), slots, d.detach()
