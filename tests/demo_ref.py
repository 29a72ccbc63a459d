"""Float64 numpy restatement of the mixed policy loss (cdrl_beta_mixed_policy_loss / cdrl_learner_demo_forward_backward,
include/cdrl.h) and of the host-side minibatch composition of the demonstration-augmented update().

  mixed_loss        the objective on linear head outputs, its closed-form gradient and the kernel's metric slots
  mixed_total_torch the same total as a torch float64 scalar (autograd cross-check of the closed form)
  split             D and the fresh rows per minibatch for (batch_size, fraction)"""
import numpy as np
from scipy.special import digamma, polygamma

from tests.trust_ref import head_alpha_beta, ln_beta, sigmoid

F32_EPS = float(np.finfo(np.float32).eps)


def split(batch_size: int, fraction: float):
    """-> (D demonstration rows, batch_size - D fresh rows) of one policy minibatch; ValueError outside 1 <= D < batch_size."""
    d = int(round(fraction * batch_size))
    if not 1 <= d < batch_size:
        raise ValueError(f'demo_fraction={fraction!r} gives {d} demonstration rows of {batch_size}')
    return d, batch_size - d


def mixed_loss(lin, adv, old_logp, speed, similarity, u, demo_u, demo_w, clip_ratio, entropy_coef, du_da=None, du_db=None):
    """Row b is a demonstration row iff demo_w[b] > 0.  -> dict(total, dlin (B, 2A+2), metrics (11,), passes (B,) bool: the
    surrogate's minimum took the unclipped branch (False on demonstration rows), demo (B,) bool, alpha, beta, log_prob, entropy
    (B, A)).  adv / old_logp / u / du_da / du_db of a demonstration row are never used (they may be NaN)."""
    lin = np.asarray(lin, np.float64)
    B, L = lin.shape
    A = (L - 2) // 2
    demo_w = np.asarray(demo_w, np.float64)
    demo = demo_w > 0.0
    ND = int(demo.sum())
    NP = B - ND
    col = demo[:, None]
    # float32 actions, clipped in float32 as _clip_actions does; the comparisons of the `inside` rule are float32 too
    act = np.where(col, np.asarray(demo_u, np.float32), np.asarray(u, np.float32)).astype(np.float32)
    lo, hi = np.float32(F32_EPS), np.float32(1.0) - np.float32(F32_EPS)
    x = np.clip(act, lo, hi).astype(np.float64)
    inside = (act >= lo) & (act <= hi) & ~col
    zero = np.zeros((B, A))
    ja = np.where(col, 0.0, zero if du_da is None else np.asarray(du_da, np.float64))
    jb = np.where(col, 0.0, zero if du_db is None else np.asarray(du_db, np.float64))
    advp = np.where(demo, 0.0, np.asarray(adv, np.float64))
    oldp = np.where(col, 0.0, np.asarray(old_logp, np.float64))
    al, be = head_alpha_beta(lin)
    lnB = ln_beta(al, be)
    pa, pb, pab = digamma(al), digamma(be), digamma(al + be)
    logp = (al - 1.0) * np.log(x) + (be - 1.0) * np.log1p(-x) - lnB
    ent = lnB - (al - 1.0) * pa - (be - 1.0) * pb + (al + be - 2.0) * pab
    dlx = np.where(inside, (al - 1.0) / x - (be - 1.0) / (1.0 - x), 0.0)
    dlp_da = np.log(x) - pa + pab + dlx * ja
    dlp_db = np.log1p(-x) - pb + pab + dlx * jb
    tab = polygamma(1, al + be)
    dH_da = -(al - 1.0) * polygamma(1, al) + (al + be - 2.0) * tab
    dH_db = -(be - 1.0) * polygamma(1, be) + (al + be - 2.0) * tab
    # PPO rows
    e = np.exp(logp - oldp)
    ratio = e.mean(axis=1)
    s = ratio * advp
    minadv = np.where(advp > 0.0, (1.0 + clip_ratio) * advp, (1.0 - clip_ratio) * advp)
    passes = (s <= minadv) & ~demo
    term = np.where(passes, s, minadv)
    ppo = -term[~demo].sum() / NP if NP else 0.0
    # demonstration rows
    nll = -logp.mean(axis=1)
    dterm = float((demo_w[demo] * nll[demo]).sum() / ND) if ND else 0.0
    dL_dlogp = np.where(col, -(demo_w[:, None] / (A * ND)) if ND else 0.0,
                        np.where(passes[:, None], -(advp[:, None] * e / (A * NP)) if NP else 0.0, 0.0))
    dL_dH = -entropy_coef / (B * A)
    dlin = np.zeros_like(lin)
    dlin[:, :A] = (dL_dlogp * dlp_da + dL_dH * dH_da) * sigmoid(lin[:, :A])
    dlin[:, A:2 * A] = (dL_dlogp * dlp_db + dL_dH * dH_db) * sigmoid(lin[:, A:2 * A])
    sim = np.tanh(lin[:, 2 * A])
    sgs = sigmoid(lin[:, 2 * A + 1])
    dsim, dspd = sim - np.asarray(similarity, np.float64), 2.0 * sgs - np.asarray(speed, np.float64)
    dlin[:, 2 * A] = dsim * (1.0 - sim * sim) / B
    dlin[:, 2 * A + 1] = dspd * 2.0 * sgs * (1.0 - sgs) / B
    entropy = ent.mean()
    speed_loss, sim_loss = 0.5 * (dspd ** 2).mean(), 0.5 * (dsim ** 2).mean()
    total = ppo - entropy_coef * entropy + speed_loss + sim_loss + dterm
    mode = (al - 1.0) / (al + be - 2.0)
    metrics = np.array([total, ppo, entropy, speed_loss, sim_loss,
                        ratio[~demo].mean() if NP else 0.0, logp[~demo].mean() if NP else 0.0,
                        dterm, logp[demo].mean() if ND else 0.0, np.abs(mode - x)[demo].mean() if ND else 0.0, float(ND)])
    return dict(total=total, dlin=dlin, metrics=metrics, passes=passes, demo=demo, alpha=al, beta=be, log_prob=logp, entropy=ent)


def mixed_total_torch(lin, adv, old_logp, speed, similarity, u, demo_u, demo_w, clip_ratio, entropy_coef, du_da=None, du_db=None):
    """The total of mixed_loss as a torch float64 scalar on `lin` (a float64 tensor that may require grad), composed from the
    oracle's own functions.  The other arguments are numpy arrays without NaN."""
    import torch
    from oracle import model as OM
    tt = lambda a: torch.tensor(np.asarray(a, np.float64))
    B, A = lin.shape[0], (lin.shape[1] - 2) // 2
    demo = tt(demo_w) > 0
    ND = int(demo.sum())
    NP = B - ND
    alpha, beta = OM.softplus101(lin[:, :A]), OM.softplus101(lin[:, A:2 * A])
    z = np.zeros((B, A))
    us = OM._InjectedSample.apply(alpha, beta, tt(u), tt(z if du_da is None else du_da), tt(z if du_db is None else du_db))
    lp_ppo = OM.beta_log_prob(torch.clamp(us, OM.EPSILON, 1.0 - OM.EPSILON), alpha, beta)
    lp_demo = OM.beta_log_prob(torch.clamp(tt(demo_u), OM.EPSILON, 1.0 - OM.EPSILON), alpha, beta)
    ratio = torch.exp(lp_ppo - tt(old_logp)).mean(dim=1)
    advt = tt(adv)
    min_adv = torch.where(advt > 0, (1 + clip_ratio) * advt, (1 - clip_ratio) * advt)
    surrogate = torch.minimum(ratio * advt, min_adv)
    zero = torch.zeros((), dtype=torch.float64)
    ppo = -surrogate[~demo].sum() / NP if NP else zero
    dterm = (tt(demo_w) * -lp_demo.mean(dim=1))[demo].sum() / ND if ND else zero
    ent = OM.beta_entropy(alpha, beta).mean()
    sim_loss = 0.5 * ((torch.tanh(lin[:, 2 * A]) - tt(similarity)) ** 2).mean()
    speed_loss = 0.5 * ((2.0 * torch.sigmoid(lin[:, 2 * A + 1]) - tt(speed)) ** 2).mean()
    return ppo - entropy_coef * ent + speed_loss + sim_loss + dterm
