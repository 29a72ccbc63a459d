"""Numpy restatement of the gradient gate (cdrl_config.clip_mode = global, skip_nonfinite; include/cdrl.h): the squared norm of an
optimizer's gradient list, the global-norm scale and the skip decision.  Shared by tests/test_grad_gate_host.py and
tests/test_gpu_grad_gate.py; the optimizer steps themselves are tests/optim_ref.py."""
import numpy as np

F = np.float32


def list_sqnorm(g, segments):
    """S of a gradient list: the sum in float64 of the squares of the float32 elements of its tensors.  `segments` are (start,
    count) pairs into the flat array `g`; whatever lies between them (the padding between tensors) is not part of the list."""
    g32 = np.asarray(g, dtype=F)
    with np.errstate(over='ignore', invalid='ignore'):
        return float(sum(np.sum(g32[s:s + c].astype(np.float64) ** 2) for s, c in segments))


def global_scale(S64, c):
    """s = float32(c / max(sqrt(S), c)) for a float32 threshold c > 0, computed in double and rounded once; 1 for c <= 0 (the
    list is not scaled).  sqrt(S) <= c gives exactly 1."""
    if c is None or not c > 0:
        return F(1.0)
    c = float(F(c))
    with np.errstate(invalid='ignore'):
        return np.float32(c / max(np.sqrt(S64), c))


def clip_by_global_norm(g, segments, c, dt=np.float64):
    """tf.clip_by_global_norm of one list as the kernels evaluate it: every element times the list's float32 scale.  Returns the
    scaled flat array in `dt` (all of it: the padding is scaled too and never compared), the norm and the scale."""
    g32 = np.asarray(g, dtype=F)
    S = list_sqnorm(g32, segments)
    s = global_scale(S, c)
    return g32.astype(dt) * dt(s), float(np.sqrt(S)), s


def should_skip(sqnorms):
    """The guard's decision from the squared norms of the lists the step consumes: skip when any is not finite (exactly when some
    element is NaN or +-Inf: finite float32 squares cannot overflow a float64 sum)."""
    return not all(np.isfinite(S) for S in sqnorms)
