"""Numpy restatement of the optimizers of cdrl_config.optimizer and of polyak averaging (include/cdrl.h table; Keras
optimizer_v2 classes of TF 2.3 and the training ops they call).  Scalar coefficients are float32, as TensorFlow computes them;
element-wise arithmetic runs in `dt` (float64 by default; float32 evaluates every element-wise operation in the kernel's order).
Shared by tests/test_optimizers_host.py and tests/test_gpu_optimizers.py."""
import numpy as np

F = np.float32
OPTIMIZERS = ('adam', 'sgd', 'rmsprop', 'adagrad', 'adadelta', 'adamax', 'nadam', 'ftrl')
# (adam_m arena, adam_v arena): Keras slot name or None, and the initial value
SLOTS = dict(adam=('m', 'v'), sgd=(None, None), rmsprop=(None, 'rms'), adagrad=(None, 'accumulator'),
             adadelta=('accum_var', 'accum_grad'), adamax=('m', 'v'), nadam=('m', 'v'), ftrl=('linear', 'accumulator'))
INIT = dict(adagrad=(0.0, 0.1), ftrl=(0.0, 0.1))
B1, B2, EPS = 0.9, 0.999, 1e-7


def slot_init(opt):
    return INIT.get(opt, (0.0, 0.0))


def nadam_mu(t, b1=B1):
    """mu_t = beta1 (1 - 0.5 * 0.96^(0.004 t)) in float32."""
    return F(F(b1) * (F(1) - F(0.5) * F(np.power(F(0.96), F(F(0.004) * F(t))))))


class OptState:
    """One optimizer: the two slot arrays, the step count and Nadam's m_cache."""

    def __init__(self, opt, n, dt=np.float64):
        m0, v0 = slot_init(opt)
        self.opt, self.dt = opt, dt
        self.m = np.full(n, F(m0), dtype=dt)       # (the arenas are float32: 0.1 is float32(0.1))
        self.v = np.full(n, F(v0), dtype=dt)
        self.t = 0
        self.m_cache = F(1)


def step(st: OptState, p, g, lr, b1=B1, b2=B2, eps=EPS):
    """One optimizer step on flat arrays; returns the new parameters (the slots and counters of `st` advance in place)."""
    dt = st.dt
    p = np.asarray(p, dtype=dt)
    g = np.asarray(g, dtype=dt)
    st.t += 1
    t = st.t
    lr, b1, b2, eps = F(lr), F(b1), F(b2), F(eps)
    c = lambda x: dt(F(x))      # a float32 scalar coefficient, used in dt arithmetic
    m, v = st.m, st.v
    if st.opt == 'adam':
        alpha = F(lr * np.sqrt(F(1) - F(np.power(b2, F(t)))) / (F(1) - F(np.power(b1, F(t)))))
        m += (g - m) * c(F(1) - b1)
        v += (g * g - v) * c(F(1) - b2)
        return p - (m * c(alpha)) / (np.sqrt(v) + c(eps))
    if st.opt == 'sgd':
        return p - g * c(lr)
    if st.opt == 'rmsprop':
        rho = F(0.9)
        v[:] = c(rho) * v + c(F(1) - rho) * (g * g)
        return p - c(lr) * g / (np.sqrt(v) + c(eps))
    if st.opt == 'adagrad':
        v += g * g
        return p - g * c(lr) / (np.sqrt(v) + c(eps))
    if st.opt == 'adadelta':
        rho = F(0.95)
        v[:] = v * c(rho) + (g * g) * c(F(1) - rho)                        # accum_grad
        u = np.sqrt(m + c(eps)) * (dt(1) / np.sqrt(v + c(eps))) * g
        m[:] = m * c(rho) + (u * u) * c(F(1) - rho)                        # accum_var
        return p - u * c(lr)
    if st.opt == 'adamax':
        m += (g - m) * c(F(1) - b1)
        v[:] = np.maximum(c(b2) * v, np.abs(g))
        return p - c(lr / (F(1) - F(np.power(b1, F(t))))) * (m / (v + c(eps)))
    if st.opt == 'nadam':
        mu, mu1 = nadam_mu(t, b1), nadam_mu(t + 1, b1)
        s_t = F(st.m_cache * mu)
        st.m_cache = s_t
        s_next = F(s_t * mu1)
        gp = g / c(F(1) - s_t)
        m[:] = c(b1) * m + c(F(1) - b1) * g
        v[:] = c(b2) * v + c(F(1) - b2) * (g * g)
        mbar = c(F(1) - mu) * gp + c(mu1) * (m / c(F(1) - s_next))
        return p - c(lr) * mbar / (np.sqrt(v / c(F(1) - F(np.power(b2, F(t))))) + c(eps))
    if st.opt == 'ftrl':
        n1 = v + g * g
        m += g - (np.sqrt(n1) - np.sqrt(v)) / c(lr) * p
        v[:] = n1
        return np.where(np.abs(m) > 0, -m / (np.sqrt(n1) / c(lr)), dt(0))
    raise ValueError(st.opt)


def clip_by_norm(g, clip_norm, dt=np.float64):
    """tf.clip_by_norm of one float32 tensor as the kernels evaluate it: squared norm summed in double, rounded to float32."""
    g32 = np.asarray(g, dtype=F)
    if not clip_norm or clip_norm <= 0:
        return g32.astype(dt)
    l2 = F(np.sum(g32.astype(np.float64) ** 2))
    norm = F(np.sqrt(l2)) if l2 > 0 else l2
    cn = F(clip_norm)
    denom = max(norm, cn)
    return g32.astype(dt) * dt(cn) / dt(denom)


def polyak(p_new, p_old, a, dt=np.float64):
    """utils.polyak_averaging (reference rl/utils.py:105-117): a * new + (1 - a) * old with a = float32(polyak) and
    1 - polyak formed in double from it, then rounded to float32."""
    a32 = F(a)
    c32 = F(1.0 - float(a32))
    return dt(a32) * np.asarray(p_new, dtype=dt) + dt(c32) * np.asarray(p_old, dtype=dt)
