"""numpy / float64 restatement of cdrl_beta_score (csrc/score.hip): the score block from (alpha, beta, value, u,
returns, speed, similarity), with scipy's betainc / gammaln / digamma in place of the device's continued fraction, lgamma and
digamma series.  Pure host code."""
import numpy as np
from scipy import special

from carla_driving_rl_agent_amd.engine import SCORE_BINS, SCORE_LAYOUT, score_block_size

EPS = np.float32(1.1920929e-07)
HEAD, ACTION = SCORE_LAYOUT['head'], SCORE_LAYOUT['action']
EDGES = np.concatenate([np.arange(1, SCORE_BINS) / SCORE_BINS, [0.25, 0.75, 0.05, 0.95]])     # where a count can flip


def clip(u):
    """x = clip(u, eps, 1 - eps) in float32, widened."""
    return np.clip(np.asarray(u, np.float32), EPS, np.float32(1.0) - EPS).astype(np.float64)


def pit(alpha, beta, u):
    """F = I_x(alpha, beta): the Beta CDF at the clipped expert action."""
    return special.betainc(np.asarray(alpha, np.float64), np.asarray(beta, np.float64), clip(u))


def edge_distance(F):
    """Distance of every PIT value to the nearest bin edge or coverage bound."""
    return np.abs(np.asarray(F, np.float64)[..., None] - EDGES).min(axis=-1)


def pit_counts(F):
    """-> (histogram (SCORE_BINS,), count inside [0.25, 0.75], count inside [0.05, 0.95]) of 1-D PIT values."""
    F = np.asarray(F, np.float64).reshape(-1)
    bins = np.minimum(SCORE_BINS - 1, np.floor(F * SCORE_BINS).astype(np.int64))
    hist = np.bincount(bins, minlength=SCORE_BINS).astype(np.float64)
    return hist, float(((F >= 0.25) & (F <= 0.75)).sum()), float(((F >= 0.05) & (F <= 0.95)).sum())


def decode(be):
    be = np.asarray(be, np.float64)
    return be[:, 0] * 10.0 ** be[:, 1]


def block(alpha, beta, value, u, returns=None, speed=None, similarity=None, no_pit=None, prior=None):
    """The block one launch leaves: alpha, beta, u (n, A) float32; value (n, 4) float32 (base, exp, speed, similarity); returns
    (n, 2) or None; speed, similarity (n,) or None.  no_pit: boolean (n, A), the elements whose PIT the device does not form (the
    iteration cap).  prior: the block the sums are added to (None: zeros)."""
    alpha, beta = np.asarray(alpha, np.float32), np.asarray(beta, np.float32)
    n, A = alpha.shape
    out = np.zeros(score_block_size(A)) if prior is None else np.array(prior, np.float64)
    al, be, x = alpha.astype(np.float64), beta.astype(np.float64), clip(u)
    finite = np.isfinite(al) & np.isfinite(be)
    no_pit = np.zeros((n, A), bool) if no_pit is None else np.asarray(no_pit, bool)
    out[HEAD['rows']] += n
    out[HEAD['nonfinite']] += (~finite).sum()
    out[HEAD['pit_unconverged']] += (finite & no_pit).sum()
    for a in range(A):
        k = finite[:, a]
        p, q, t = al[k, a], be[k, a], x[k, a]
        lnB = special.gammaln(p) + special.gammaln(q) - special.gammaln(p + q)
        logp = (p - 1.0) * np.log(t) + (q - 1.0) * np.log1p(-t) - lnB
        mean = p / (p + q)
        ent = lnB - (p - 1.0) * special.digamma(p) - (q - 1.0) * special.digamma(q) + (p + q - 2.0) * special.digamma(p + q)
        g = out[SCORE_LAYOUT['head_size'] + a * SCORE_LAYOUT['action_size']:][:SCORE_LAYOUT['action_size']]
        g[ACTION['count']] += k.sum()
        g[ACTION['log_prob']] += logp.sum()
        g[ACTION['mode_error']] += np.abs((p - 1.0) / (p + q - 2.0) - t).sum()
        g[ACTION['error']] += (mean - t).sum()
        g[ACTION['error2']] += ((mean - t) ** 2).sum()
        g[ACTION['variance']] += (p * q / ((p + q) ** 2 * (p + q + 1.0))).sum()
        g[ACTION['entropy']] += ent.sum()
        keep = ~no_pit[k, a]
        hist, c50, c90 = pit_counts(special.betainc(p[keep], q[keep], t[keep]))
        g[ACTION['cover_50']] += c50
        g[ACTION['cover_90']] += c90
        g[ACTION['histogram']:ACTION['histogram'] + SCORE_BINS] += hist
    value = np.asarray(value, np.float32)
    if returns is not None:
        V, R = decode(value[:, :2]), decode(returns)
        out[HEAD['rows_returns']] += n
        out[HEAD['value_error']] += (V - R).sum()
        out[HEAD['value_error2']] += ((V - R) ** 2).sum()
        out[HEAD['returns']] += R.sum()
        out[HEAD['returns2']] += (R ** 2).sum()
    if speed is not None:
        out[HEAD['rows_aux']] += n
        out[HEAD['speed_error2']] += ((value[:, 2].astype(np.float64) - np.asarray(speed, np.float32).astype(np.float64)) ** 2).sum()
        out[HEAD['similarity_error2']] += ((value[:, 3].astype(np.float64)
                                            - np.asarray(similarity, np.float32).astype(np.float64)) ** 2).sum()
    return out


def count_slots(A):
    """Indices of the block entries that are counts (compared exactly)."""
    slots = [HEAD[k] for k in ('rows', 'rows_returns', 'rows_aux', 'nonfinite', 'pit_unconverged')]
    for a in range(A):
        base = SCORE_LAYOUT['head_size'] + a * SCORE_LAYOUT['action_size']
        slots += [base + ACTION['count'], base + ACTION['cover_50'], base + ACTION['cover_90']]
        slots += list(range(base + ACTION['histogram'], base + ACTION['histogram'] + SCORE_BINS))
    return np.array(slots)


def compare(got, want, A, bound=1e-9):
    """-> (the counts are equal, the worst |got - want| / max(1, |want|) over all entries)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    c = count_slots(A)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return bool(np.array_equal(got[c], want[c])), float(err.max())
