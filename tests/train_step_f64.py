"""One float64 numpy restatement of a teacher-forced training step (LBDRNmodel.py:79-82, LBDRNloss.py:9,
torch/optim/adam.py): nl = 1..3 hidden layers of Sine(30) or ReLU, a sigmoid head, the MSE over B x C, Adam with torch's
defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay) and a learning rate per step.  What exact arithmetic gives, to
tell a kernel's rounding from a float32 reference run's own.

A plain module: no fixture, no marker, no device.  Parameters are flat in state_dict order: W_0 [bc][F], b_0, W_1 [bc][bc],
b_1, .., W_last [C][bc], b_last."""
import numpy as np

W0_SINE = 30.0   # LBDRNmodel.py: Sine(w0 = 30)


def layer_slices(F, bc, C, nl):
    """[(weights slice, (rows, cols), bias slice)] per layer of the flat parameter vector, the output layer last."""
    out, o = [], 0
    for l in range(nl + 1):
        rows, cols = (bc if l < nl else C), (F if l == 0 else bc)
        out.append((slice(o, o + rows * cols), (rows, cols), slice(o + rows * cols, o + rows * cols + rows)))
        o += rows * cols + rows
    return out


def param_count(F, bc, C, nl):
    return layer_slices(F, bc, C, nl)[-1][2].stop


def _activation(act):
    if act == "relu":
        return (lambda z: np.maximum(z, 0.0)), (lambda z: (z > 0).astype(np.float64))
    if act == "sine":
        return (lambda z: np.sin(W0_SINE * z)), (lambda z: W0_SINE * np.cos(W0_SINE * z))
    raise ValueError(act)


def forward_f64(p, xb, F, bc, C, nl, act):
    """-> (hidden pre-activations [z_0 .. z_{nl-1}], layer inputs [x, h_0 .. h_{nl-1}], y)"""
    fwd, _ = _activation(act)
    zs, hs = [], [xb]
    L = layer_slices(F, bc, C, nl)
    for l in range(nl):
        w, shape, b = L[l]
        z = hs[-1] @ p[w].reshape(shape).T + p[b]
        zs.append(z)
        hs.append(fwd(z))
    w, shape, b = L[nl]
    y = 1.0 / (1.0 + np.exp(-(hs[-1] @ p[w].reshape(shape).T + p[b])))
    return zs, hs, y


def loss_and_grad_f64(p, xb, tb, F, bc, C, nl, act):
    """-> (MSE over B x C, its flat gradient) at parameters p on the minibatch (xb, tb), all float64"""
    _, der = _activation(act)
    L = layer_slices(F, bc, C, nl)
    zs, hs, y = forward_f64(p, xb, F, bc, C, nl, act)
    d = y - tb
    loss = float(np.mean(d * d))
    g = np.zeros_like(p)
    dz = 2 * d / d.size * y * (1 - y)
    for l in range(nl, -1, -1):
        w, shape, b = L[l]
        g[w] = (dz.T @ hs[l]).ravel()
        g[b] = dz.sum(0)
        if l:
            dz = (dz @ p[w].reshape(shape)) * der(zs[l - 1])
    return loss, g


def train_step_f64(p, m, v, xb, tb, F, bc, C, nl, act, lr, step):
    """One update (step = 1 for the first): -> (loss, gradient, parameters, exp_avg, exp_avg_sq) after it."""
    loss, g = loss_and_grad_f64(p, xb, tb, F, bc, C, nl, act)
    m = 0.9 * m + 0.1 * g
    v = 0.999 * v + 0.001 * g * g
    p = p - (lr / (1 - 0.9 ** step)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** step) + 1e-8)
    return loss, g, p, m, v


def f64_steps(x, t, params0, batches, F, bc, C, lrs, act="sine", nl=2):
    """The teacher-forced updates over `batches` (index arrays into x / t) from zero moments: -> (params, exp_avg,
    exp_avg_sq) after the last one."""
    x, t = np.asarray(x).astype(np.float64), np.asarray(t).astype(np.float64)
    p = np.asarray(params0).astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for s, b in enumerate(batches):
        _, _, p, m, v = train_step_f64(p, m, v, x[b], t[b], F, bc, C, nl, act, lrs[s], s + 1)
    return p, m, v


def f64_trace(x, t, params0, batches, F, bc, C, lrs, act="sine", nl=2):
    """f64_steps keeping every step: -> [(loss, gradient, params, exp_avg, exp_avg_sq)]"""
    x, t = np.asarray(x).astype(np.float64), np.asarray(t).astype(np.float64)
    p = np.asarray(params0).astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for s, b in enumerate(batches):
        loss, g, p, m, v = train_step_f64(p, m, v, x[b], t[b], F, bc, C, nl, act, lrs[s], s + 1)
        out.append((loss, g, p, m, v))
    return out


def kink_margin(p, xb, F, bc, C, nl):
    """ReLU: min over the hidden layers of (smallest |z|) / (largest |z|) of that layer's pre-activations.  A float32
    evaluation can put a pre-activation on the other side of 0 only where this is at rounding level."""
    zs, _, _ = forward_f64(np.asarray(p, np.float64), np.asarray(xb, np.float64), F, bc, C, nl, "relu")
    return min(float(np.abs(z).min() / np.abs(z).max()) for z in zs)
