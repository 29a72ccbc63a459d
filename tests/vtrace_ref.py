"""Float64 numpy restatement of cdrl_vtrace_segments (include/cdrl.h), written from the formulas, sharing nothing with the kernel:
plain Python loops for the recurrences, math.lgamma for the Beta normaliser.  Only the float32 steps the interface defines are float32
here as well: V = base * 10^exp, the clip of the action, the casts of the outputs and the decomposition of the returns."""
import math

import numpy as np

EPS = np.float32(1.1920929e-07)


def values(values_be):
    """(n, 2) float32 (base, exp) -> float32 base * 10^exp."""
    v = np.asarray(values_be, np.float32)
    return (v[:, 0] * np.power(10.0, v[:, 1].astype(np.float64)).astype(np.float32)).astype(np.float32)


def log_pi(alpha, beta, actions):
    """Joint Beta log-density of every row, float64."""
    alpha, beta = np.asarray(alpha, np.float64), np.asarray(beta, np.float64)
    u = np.clip(np.asarray(actions, np.float32), EPS, np.float32(1.0) - EPS).astype(np.float64)
    lgamma = np.vectorize(math.lgamma, otypes=[np.float64])
    ln_b = lgamma(alpha) + lgamma(beta) - lgamma(alpha + beta)
    return ((alpha - 1.0) * np.log(u) + (beta - 1.0) * np.log1p(-u) - ln_b).sum(axis=1)


def ratios(alpha, beta, actions, log_prob_old):
    """Unclipped importance ratio of every row, float64 (inf where exp overflows)."""
    diff = log_pi(alpha, beta, actions) - np.asarray(log_prob_old, np.float64).sum(axis=1)
    with np.errstate(over='ignore'):
        return np.exp(diff)


def decompose(x):
    x, e = np.float32(x), 0
    while abs(x) > np.float32(1.0):
        x = np.float32(x / np.float32(10.0))
        e += 1
    return x, np.float32(e)


def trajectory(rewards, values_be, alpha, beta, actions, log_prob_old, gamma, lam, rho_bar, c_bar, scale):
    """One trajectory: rewards (n + 1,), values_be (n + 1, 2) incl. the bootstrap entry, the rest (n, A).
    -> dict of float64 arrays: returns, adv_raw, adv, rho (unclipped), and returns_be (n, 2) float32."""
    n = len(rewards) - 1
    V = values(values_be).astype(np.float64)
    r = np.asarray(rewards, np.float32).astype(np.float64)
    ratio = ratios(alpha, beta, actions, log_prob_old)
    rho, c = np.minimum(rho_bar, ratio), np.minimum(c_bar, ratio)
    td = r[:n] + gamma * V[1:] - V[:n]
    x, y = np.zeros(n + 1), np.zeros(n + 1)
    for i in range(n - 1, -1, -1):
        x[i] = rho[i] * td[i] + gamma * lam * c[i] * x[i + 1]
        y[i] = rho[i] * td[i] + gamma * c[i] * y[i + 1]
    adv_raw = td + gamma * lam * x[1:]
    vs = V[:n] + y[:n]
    a32 = adv_raw.astype(np.float32).astype(np.float64)
    pos, neg = np.where(a32 > 0, a32, 0.0), np.where(a32 < 0, a32, 0.0)
    adv = (pos / (a32.max() + 1e-3) + neg / -(a32.min() - 1e-3)) * scale
    returns_be = np.array([decompose(v) for v in vs.astype(np.float32)], np.float32).reshape(n, 2)
    return dict(returns=vs, adv_raw=adv_raw, adv=adv, rho=ratio, returns_be=returns_be)


def segments(rewards, values_be, alpha, beta, actions, log_prob_old, lengths, gamma, lam, rho_bar, c_bar, scale):
    """The padded / packed layout of the kernel: every trajectory on its own, outputs concatenated."""
    outs, row = [], 0
    for s, n in enumerate(lengths):
        pad = slice(row + s, row + s + n + 1)
        d = slice(row, row + n)
        outs.append(trajectory(rewards[pad], values_be[pad], alpha[d], beta[d], actions[d], log_prob_old[d], gamma, lam, rho_bar,
                               c_bar, scale))
        row += n
    return {k: np.concatenate([o[k] for o in outs], axis=0) for k in outs[0]}
