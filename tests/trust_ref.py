"""Float64 restatement of the trust-region guard's KL (cdrl_beta_kl, include/cdrl.h): the analytic KL between an anchor
Beta policy and the Beta head on linear outputs, with scipy's gammaln / digamma, and its gradient w.r.t. the linear outputs from
the closed form.  `kl_torch` states the same KL in torch float64, for the autograd cross-check of the closed-form gradient."""
import numpy as np
from scipy.special import digamma, gammaln

OFFSET = 1.01       # alpha = softplus(lin) + 1.01: the constant of the policy head (policy_loss_kernel)


def softplus(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def ln_beta(a, b):
    return gammaln(a) + gammaln(b) - gammaln(a + b)


def kl_beta(a0, b0, a, b):
    """KL(Beta(a0, b0) || Beta(a, b)), elementwise, float64."""
    a0, b0, a, b = (np.asarray(x, np.float64) for x in (a0, b0, a, b))
    return ln_beta(a, b) - ln_beta(a0, b0) + (a0 - a) * digamma(a0) + (b0 - b) * digamma(b0) + (a - a0 + b - b0) * digamma(a0 + b0)


def head_alpha_beta(lin):
    """lin (B, 2A+2) -> alpha, beta (B, A), float64."""
    lin = np.asarray(lin, np.float64)
    A = (lin.shape[1] - 2) // 2
    return softplus(lin[:, :A]) + OFFSET, softplus(lin[:, A:2 * A]) + OFFSET


def kl_from_lin(lin, anchor):
    """lin (B, 2A+2), anchor (B, 2, A) -> dict(rows (B,) = sum over the actions, kl = mean over the rows UNCLAMPED, metrics = what the
    kernel reports: [max(kl, 0), max over rows, max(kl, 0) / A], dlin (B, 2A+2) = d kl / d lin, zero in the two auxiliary columns)."""
    lin = np.asarray(lin, np.float64)
    anchor = np.asarray(anchor, np.float64)
    B, L = lin.shape
    A = (L - 2) // 2
    a, b = head_alpha_beta(lin)
    a0, b0 = anchor[:, 0], anchor[:, 1]
    rows = kl_beta(a0, b0, a, b).sum(axis=1)
    kl = rows.mean()
    pab, pab0 = digamma(a + b), digamma(a0 + b0)
    dlin = np.zeros_like(lin)
    dlin[:, :A] = (digamma(a) - pab - digamma(a0) + pab0) * sigmoid(lin[:, :A]) / B
    dlin[:, A:2 * A] = (digamma(b) - pab - digamma(b0) + pab0) * sigmoid(lin[:, A:2 * A]) / B
    clamped = kl if not kl < 0.0 else 0.0
    return dict(rows=rows, kl=kl, metrics=np.array([clamped, rows.max() if not np.isnan(rows).any() else np.nan, clamped / A]), dlin=dlin)


def kl_torch(lin, anchor):
    """The same mean KL as a torch float64 scalar that autograd can differentiate w.r.t. `lin` (a float64 tensor)."""
    import torch
    A = (lin.shape[1] - 2) // 2
    a = torch.nn.functional.softplus(lin[:, :A]) + OFFSET
    b = torch.nn.functional.softplus(lin[:, A:2 * A]) + OFFSET
    a0, b0 = anchor[:, 0], anchor[:, 1]
    lnb = lambda x, y: torch.lgamma(x) + torch.lgamma(y) - torch.lgamma(x + y)
    k = lnb(a, b) - lnb(a0, b0) + (a0 - a) * torch.digamma(a0) + (b0 - b) * torch.digamma(b0) + (a - a0 + b - b0) * torch.digamma(a0 + b0)
    return k.sum(dim=1).mean()
