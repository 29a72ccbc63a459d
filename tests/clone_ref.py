"""Float64 PyTorch restatement of the behaviour-cloning objective (cdrl_beta_clone_loss / cdrl_learner_clone_forward_backward,
include/cdrl.h), composed from the oracle's own functions and differentiated by autograd.

  clone_terms      the objective on activated heads (alpha, beta, speed, similarity predictions)
  clone_from_lin   ... on the linear head outputs the loss kernel reads: (B, 2A+2) = A alpha, A beta, similarity, speed columns
  clone_grads      ... on the oracle model: train-mode trunk, policy head, objective, gradients of policy head and trunk"""
import torch

from oracle import model as OM


def clone_terms(alpha, beta, speed_pred, sim_pred, u, weight=None, speed=None, similarity=None, entropy_coef=0.0, aux_weight=1.0):
    """-> (total, dict of the metric slots and the per-element alpha / beta / log_prob / entropy)."""
    x = torch.clamp(u, OM.EPSILON, 1.0 - OM.EPSILON).detach()           # _clip_actions; the expert action carries no gradient
    log_prob = OM.beta_log_prob(x, alpha, beta)
    ent = OM.beta_entropy(alpha, beta)
    w = torch.ones_like(log_prob[:, 0]) if weight is None else weight
    clone = (w * (-log_prob.mean(dim=1))).mean()
    entropy = ent.mean()
    zero = torch.zeros((), dtype=alpha.dtype)
    speed_loss = 0.5 * ((speed_pred.reshape(-1) - speed.reshape(-1)) ** 2).mean() if speed is not None else zero
    sim_loss = 0.5 * ((sim_pred.reshape(-1) - similarity.reshape(-1)) ** 2).mean() if similarity is not None else zero
    total = clone - entropy_coef * entropy + aux_weight * (speed_loss + sim_loss)
    mode = (alpha - 1.0) / (alpha + beta - 2.0)
    out = dict(total=total, clone=clone, entropy=entropy, speed_loss=speed_loss, sim_loss=sim_loss, weight=w.mean(),
               log_prob_mean=log_prob.mean(), mode_error=(mode - x).abs().mean(), alpha=alpha, beta=beta, log_prob=log_prob,
               entropy_elems=ent)
    return total, out


def clone_from_lin(lin, u, weight=None, speed=None, similarity=None, entropy_coef=0.0, aux_weight=1.0):
    A = u.shape[1]
    alpha, beta = OM.softplus101(lin[:, :A]), OM.softplus101(lin[:, A:2 * A])
    sim_pred, speed_pred = torch.tanh(lin[:, 2 * A]), 2.0 * torch.sigmoid(lin[:, 2 * A + 1])
    return clone_terms(alpha, beta, speed_pred, sim_pred, u, weight, speed, similarity, entropy_coef, aux_weight)


def metric_slots(out):
    """metrics[0..7] of the kernel, as float64 numbers."""
    keys = ('total', 'clone', 'entropy', 'speed_loss', 'sim_loss', 'weight', 'log_prob_mean', 'mode_error')
    return [float(out[k].detach()) for k in keys]


def clone_grads(learner, batch, aux_weight=1.0):
    """The clone pass on an OracleLearner (tests/util.make_pair): batch = dict(states, u, and optionally weight, speed,
    similarity) of numpy arrays.  -> (total, policy-head gradients, trunk gradients, terms); entropy_coef is the learner's."""
    b = learner._cast(batch)
    d = OM.dynamics_forward(b['states'], learner.trunk, learner.cfg, training=True)
    alpha, beta, speed_pred, sim_pred = OM.policy_heads(d, learner.policy, True)
    total, out = clone_terms(alpha, beta, speed_pred, sim_pred, b['u'], b.get('weight'), b.get('speed'), b.get('similarity'),
                             learner.hp['entropy_coef'], aux_weight)
    return total, learner._grads(total, learner.policy, learner.pspec), learner._grads(total, learner.trunk, learner.tspec), out
