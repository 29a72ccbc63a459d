"""References of the fused depthwise block (cdrl_dwconv_bn_fwd / _bwd), shared by tests/test_gpu_ops.py::test_dwconv_bn_fused,
tests/test_gpu_bf16_storage.py::test_dwconv_bn_bf16_storage and tests/test_gpu_dw_variants.py.

float32 tensors: torch autograd of the unfused composition  [BN + ReLU6] -> dw3x3 -> BN  in float64 (`draw` + `evaluate`).
bf16 storage: the storage contract is exact -- the bf16-tensor run against the float32-tensor run of the same kernels on the same
(widened) values, and float64 sums of the rounded output for the statistics (`bf16_inputs`, `check_bf16_forward`,
`check_bf16_backward`)."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import model as OM

BF = torch.bfloat16


@contextlib.contextmanager
def cpu_threads():
    """The reference's torch CPU threads: what the machine grants this process (its OpenMP setting and its CPU affinity), 16 at most --
    never the machine's CPU count."""
    n = 16
    if os.environ.get('OMP_NUM_THREADS', '').isdigit():
        n = min(n, max(1, int(os.environ['OMP_NUM_THREADS'])))
    if hasattr(os, 'sched_getaffinity'):
        n = min(n, max(1, len(os.sched_getaffinity(0))))
    old = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        yield n
    finally:
        torch.set_num_threads(old)


def draw(rng, T, B, H, W, Cc, stride, pre):
    """Inputs and parameters of one case (float32 arrays / float64 parameter tensors), in the draw order test_dwconv_bn_fused has
    always used; `dout` is drawn by `evaluate` (after the parameters)."""
    x = (rng.standard_normal((T, B, H, W, Cc)) * 1.5 + 0.4).astype(np.float32)
    w = rng.standard_normal((3, 3, Cc, 1)).astype(np.float32)
    b = rng.standard_normal(Cc).astype(np.float32)

    def bnp(name):
        return {f'{name}.gamma': torch.tensor(rng.uniform(0.5, 1.5, Cc), dtype=torch.float64),
                f'{name}.beta': torch.tensor(rng.uniform(1.0, 3.0, Cc), dtype=torch.float64),
                f'{name}.moving_mean': torch.tensor(rng.uniform(-0.2, 0.2, Cc), dtype=torch.float64),
                f'{name}.moving_var': torch.tensor(rng.uniform(0.5, 1.5, Cc), dtype=torch.float64)}
    p = {'c.w': torch.tensor(w, dtype=torch.float64), 'c.b': torch.tensor(b, dtype=torch.float64), **bnp('pre'), **bnp('post')}
    if pre == 2:
        # channels the backward must NOT take xhat1 = (a - beta) / gamma for (tiny |gamma|, large |beta| / |gamma|: it re-reads y1 there),
        # mixed with ordinary ones inside a thread's channel pair
        p['pre.gamma'][::5] = torch.tensor(rng.choice([-1.0, 1.0], len(p['pre.gamma'][::5])) * 0.01, dtype=torch.float64)
        p['pre.beta'][::5] = torch.tensor(rng.uniform(0.5, 2.5, len(p['pre.beta'][::5])), dtype=torch.float64)
        p['pre.gamma'][3::7] = 0.2
        p['pre.beta'][3::7] = 3.0 + 0.0 * p['pre.beta'][3::7]
    Ho, Wo = -(-H // stride), -(-W // stride)
    dout = rng.standard_normal((T, B, Ho, Wo, Cc)).astype(np.float32)
    return SimpleNamespace(T=T, B=B, H=H, W=W, C=Cc, stride=stride, pre=pre, Ho=Ho, Wo=Wo, x=x, w=w, b=b, dout=dout, p=p,
                           f32={k: v.detach().clone().float() for k, v in p.items()})


TRAINED = ('c.w', 'c.b', 'pre.gamma', 'pre.beta', 'post.gamma', 'post.beta')


def evaluate(inp, dtype=torch.float64, decisions=None):
    """The unfused composition and its gradients by torch autograd in `dtype` (float64: the reference; float32: what float32
    arithmetic itself loses on it, the measure of tests/util.py::check3).  `decisions`: the (inside, above) ReLU6 regions of the
    pre-BN output, (T, B, C, H, W) booleans, forced onto the forward (oracle.model.Decisions replay) -- the gradient is then that of
    a smooth function, whichever side of a kink rounding puts an element on.  Returns numpy arrays in the kernels' layouts."""
    T, B, H, W, Cc, N = inp.T, inp.B, inp.H, inp.W, inp.C, inp.T * inp.B
    p = {k: v.detach().clone().to(dtype).requires_grad_(k in TRAINED) for k, v in inp.p.items()}
    xt = torch.tensor(inp.x, dtype=dtype).permute(0, 1, 4, 2, 3).requires_grad_(True)        # (T,B,C,H,W)
    if inp.pre:
        z = OM.bn_slices(xt, p, 'pre', True, True)
        if decisions is not None:
            OM.DEC.items = [decisions]
            OM.DEC.start('replay')
        try:
            a = OM.relu6(z)
        finally:
            OM.DEC.start('off')
    else:
        a = xt
    y2 = OM.conv_dw(a, p, 'c', inp.stride)
    out = OM.bn_slices(y2, p, 'post', True, True)
    out.backward(torch.tensor(inp.dout, dtype=dtype).permute(0, 1, 4, 2, 3))
    y2n = y2.detach().permute(0, 1, 3, 4, 2).reshape(N, inp.Ho, inp.Wo, Cc).numpy()
    y2g = y2n.reshape(T, -1, Cc).astype(np.float64)
    r = SimpleNamespace(p=p, y=y2n, mean=y2g.mean(axis=1), rstd=1.0 / np.sqrt(y2g.var(axis=1) + 1e-3),
                        moving_mean=p['post.moving_mean'].detach().numpy(), moving_var=p['post.moving_var'].detach().numpy(),
                        dx=xt.grad.permute(0, 1, 3, 4, 2).reshape(N, H, W, Cc).numpy(), dw=p['c.w'].grad.numpy(),
                        dgamma_post=p['post.gamma'].grad.numpy(), dbeta_post=p['post.beta'].grad.numpy())
    if inp.pre:
        r.dgamma_pre, r.dbeta_pre = p['pre.gamma'].grad.numpy(), p['pre.beta'].grad.numpy()
    return r


# ---- bf16 activation storage ----------------------------------------------------------------------------------------------------

def _dev(x, device, dt=torch.float32):
    return torch.tensor(np.asarray(x, np.float32), device=device).to(dt)


def bf16_inputs(rng, T, B, H, W, Cc, stride, device):
    """Device tensors of one bf16-storage case, in the draw order test_dwconv_bn_bf16_storage has always used."""
    N, Ho, Wo = T * B, -(-H // stride), -(-W // stride)
    xb = _dev(rng.standard_normal((N, H, W, Cc)) * 1.5 + 0.4, device, BF)
    w, b = _dev(rng.standard_normal((3, 3, Cc, 1)), device), _dev(rng.standard_normal(Cc), device)
    dob = _dev(rng.standard_normal((N, Ho, Wo, Cc)), device, BF)
    g1, b1 = _dev(rng.uniform(0.5, 1.5, Cc), device), _dev(rng.uniform(1.0, 3.0, Cc), device)
    g2, b2 = _dev(rng.uniform(0.5, 1.5, Cc), device), _dev(rng.uniform(-0.5, 0.5, Cc), device)
    return SimpleNamespace(N=N, Ho=Ho, Wo=Wo, xb=xb, w=w, b=b, dob=dob, g1=g1, b1=b1, g2=g2, b2=b2)


def same_bits(a_bf16, ref_f32):
    return torch.equal(a_bf16, ref_f32.to(BF))


def check_bf16_forward(y_f32, y_bf16, stats_bf16, T, Cc):
    """forward: y = rounded float32 y; the following BatchNorm's statistics are those of the ROUNDED y"""
    assert same_bits(y_bf16, y_f32)
    yr = y_bf16.double().view(T, -1, Cc)
    st = stats_bf16.double().view(4, T, Cc)
    assert torch.allclose(st[0], yr.mean(1), rtol=1e-6, atol=1e-6)
    assert torch.allclose(st[1], 1.0 / torch.sqrt(yr.var(1, unbiased=False) + 1e-3), rtol=1e-5)


def check_bf16_backward(o0, o1, pre):
    """backward from a COMMON state (the rounded y and its statistics): activations rounded, everything else identical.
    o0 / o1: (dx, dw, db, [dgamma_post, dbeta_post, dgamma_pre, dbeta_pre], [coef_post, coef_pre]) of the float32-tensor and the
    bf16-tensor run."""
    assert torch.equal(o0[1], o1[1]) and torch.equal(o0[2], o1[2])                  # filter / bias gradients
    assert torch.equal(o0[3][0], o1[3][0]) and torch.equal(o0[3][1], o1[3][1]) and torch.equal(o0[4][0], o1[4][0])
    if pre:
        # dz1 (the masked gradient at the pre-BN's output) is the kernel's activation output; the op wrapper then applies the
        # pre-BN backward IN PLACE on it (reads the stored dz1): float32 vs bf16 storage differ by that one rounding
        assert torch.equal(o0[3][2], o1[3][2]) and torch.equal(o0[3][3], o1[3][3])  # BN1 sums come from the unrounded registers
        e = (o1[0].float() - o0[0]).abs().max().item() / o0[0].abs().max().item()
        assert e < 2.0 ** -7, e
    else:
        assert same_bits(o1[0], o0[0])
