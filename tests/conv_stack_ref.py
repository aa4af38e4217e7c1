"""Float64 twins of the models' convolution stack, on the CPU in plain torch (nothing of the package is imported):

    dense_twin     FlowEstimatorDense:  x_{k+1} = cat([lrelu(conv(x_k, w_k) + b_k), x_k], 1), k = 1..5;
                                        flow = conv(x_6, w_head) + b_head                          -> (x_6, flow)
    context_twin   ContextNetwork:      seven 3x3 layers, dilations 1, 2, 4, 8, 16, 1, 1, padding = dilation, LeakyReLU behind
                                        the first six

with their gradients from float64 autograd (dense_grads / context_grads), each tensor's MAGNITUDE, fixtures on which no
LeakyReLU kink can flip, and the any-order fp32 cap of every tensor.

Magnitude.  M(t) is the same graph evaluated on absolute values -- |x|, |w|, |b|, |g| -- with the activation replaced by the
identity (|lrelu z| <= |z|, |lrelu'| <= 1): the measure of tests/test_splitconv_gpu.py, sum |w| |x|, carried through the layers.
e(t) = max |t_gpu - t_64| / M(t); an element with M = 0 must be exact (rel_err returns inf otherwise).

Fixtures.  x is randn; every bias is +-(1 + 0.25 rand), the sign alternating by channel; every layer's weights are randn,
rescaled in float64 so that max |conv(x_k, w_k)| = 0.25 and then rounded to fp32.  Each pre-activation's sign is then its
bias's sign (|z| >= 0.75): half of the channels take the slope branch, the convolution still contributes to every value and
every gradient, and -- since |z| / M(z) stays far above the cap below (tests/test_conv_stack_cpu.py asserts it for every
fixture the GPU tests use) -- no correct fp32 implementation can flip a sign, so no element has to be excluded.  The
activations depend on the slope, so a fixture is built for one slope.

Cap.  gamma(n) = n u / (1 - n u), u = 2^-24, n = the fp32 roundings on the longest path to the tensor, each relative to
M (tests/test_headconv_gpu.py's criterion 2 composed: (1 + gamma(a))(1 + gamma(b)) <= 1 + gamma(a + b)).  Counted as:

    conv of C channels, bias, activation   9C + 2   (one product, 9C - 1 additions, the bias, the slope product)
      ... on the split-bf16 kernels          + 3      (a product there carries the dropped plane products, below 2.01 u of it,
                                                       tests/test_splitconv_wgrad_gpu.py; counted for every 3x3 layer but the heads)
    data gradient of a layer with K outputs  9K + 3   (no bias), the heads' 9 * 2 = 18
    gather of m sources                      m, + 1 for the activation's derivative
    weight gradient over P = N H W pixels    P + 3 + n(x_k) + n(gy_k)  (both factors carry their own path)
    bias gradient                            P + n(gy_k)

  dense estimator, C_k = ch_in + (0, 128, 256, 352, 416), C_6 = ch_in + 448:
    a_k (slot k of x6)   sum_{j <= k} (9 C_j + 5);   x6 = a_5's;   flow = n(x6) + 9 C_6 + 2
    gy_5 = 2 + 1 + 18;   dx_k = 9 oc_k + 3 + n(gy_k);   gy_m = (2 + 5 - m) + 1 + n(dx_{m+1})  (the longest source);
    dx = 7 + n(dx_1);   dw_k, db_k as above with x_1 exact and x_k = a_{k-1}'s;   dw_head = P + n(x6);   db_head = P
  context net, (C_k -> K_k) = (ch_in, 128, 128, 128, 96, 64, 32) -> (128, 128, 128, 96, 64, 32, 2), the moves between
  phase mosaics being copies:
    a_k = sum_{j <= k} (9 C_j + 5), k = 1..6;   out = n(a_6) + 9 * 32 + 2
    dx_7 = 18;   gy_k = n(dx_{k+1}) + 1;   dx_k = 9 K_k + 3 + n(gy_k);   dx = dx_1;   dw_k, db_k as above (gy_7 exact)

dense_counts / context_counts return these n per tensor; for ch_in = 147 the largest is about 2.3e4, a cap of 1.4e-3 M."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
DENSE_OCS = (128, 128, 96, 64, 32)
CONTEXT_KS = (128, 128, 128, 96, 64, 32, 2)
CONTEXT_DILATIONS = (1, 2, 4, 8, 16, 1, 1)


def gamma(n):
    return n * U / (1.0 - n * U)


def lrelu(z, slope):
    return torch.where(z > 0, z, z * slope)


def to64(ts, dtype=torch.float64):
    return [t.detach().cpu().to(dtype) for t in ts]


def rel_err(got, ref, mag):
    """e = max |got - ref| / M; inf where an element with M = 0 is not exact."""
    d = (got.detach().cpu().double() - ref).abs()
    inf = torch.full_like(d, float('inf'))
    r = torch.where(mag > 0, d / mag.clamp_min(1e-300), torch.where(d > 0, inf, torch.zeros_like(d)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------
def dense_twin(x, params, slope, taps=None, mutate=None):
    """(x6, flow); params = (w1, b1, ..., w5, b5, w_head, b_head).  taps: a list that receives the five pre-activations.
    mutate (for tests/test_conv_stack_cpu.py): 'slot_order' -- layer 5's activation written behind its input instead of in
    front; 'drop_source' -- layer 4 reads a_3 detached, so a_3's gradient misses its last gather source dx_4."""
    for k in range(5):
        xin = x
        if mutate == 'drop_source' and k == 3:
            xin = torch.cat([x[:, :DENSE_OCS[2]].detach(), x[:, DENSE_OCS[2]:]], 1)
        z = F.conv2d(xin, params[2 * k], params[2 * k + 1], padding=1)
        if taps is not None:
            taps.append(z)
        a = lrelu(z, slope)
        x = torch.cat([x, a] if (mutate == 'slot_order' and k == 4) else [a, x], 1)
    return x, F.conv2d(x, params[10], params[11], padding=1)


def dense_grads(x, params, slope, g_x6, g_flow, mutate=None, dtype=torch.float64):
    """Everything the GPU tests compare, in float64: {'x6', 'flow', 'dx', 'dw': [6], 'db': [6], 'z': [5]}.
    mutate 'bias_slot': layer 3's bias gradient summed over layer 4's slot of x6 (channels 32.. instead of 96..).
    dtype=torch.float32: the same expression as a plain fp32 evaluation on the CPU, the CPU tests' stand-in for a vendor path."""
    x, g_x6, g_flow = to64([x, g_x6, g_flow], dtype)
    x.requires_grad_(True)
    params = [p.requires_grad_(True) for p in to64(params, dtype)]
    taps = []
    x6, flow = dense_twin(x, params, slope, taps, mutate)
    grads = torch.autograd.grad([x6, flow], [x] + params + taps, [g_x6, g_flow])
    dw, db, gz = list(grads[1:13:2]), list(grads[2:13:2]), grads[13:]
    if mutate == 'bias_slot':
        gy6 = torch.cat(gz[::-1], 1)  # the pre-activation gradients in x6's slot order: a_5, a_4, ..., a_1
        off = DENSE_OCS[4]
        db[2] = gy6[:, off:off + DENSE_OCS[2]].sum((0, 2, 3))
    return {'x6': x6.detach(), 'flow': flow.detach(), 'dx': grads[0], 'dw': dw, 'db': db, 'z': [z.detach() for z in taps]}


def dense_magnitudes(x, params, g_x6, g_flow):
    """dense_grads on absolute values with the identity for the activation."""
    return dense_grads(x.abs(), [p.abs() for p in params], 1.0, g_x6.abs(), g_flow.abs())


def _scaled_layer(cur, oc, gen):
    """(w, b) in fp32 for the float64 input `cur`: max |conv(cur, w)| = 0.25, b = +-(1 + 0.25 rand) alternating by channel."""
    b = (1.0 + 0.25 * torch.rand(oc, generator=gen)) * (1.0 - 2.0 * (torch.arange(oc) % 2))
    w = torch.randn(oc, cur.shape[1], 3, 3, generator=gen).double()
    return w, b.float()


def dense_fixture(ch_in, N, H, W, slope, seed=0):
    """{'x', 'params', 'g_x6', 'g_flow', 'slope'}: fp32 tensors on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ch_in, H, W, generator=gen)
    cur, params = x.double(), []
    for k, oc in enumerate(DENSE_OCS + (2,)):
        w, b = _scaled_layer(cur, oc, gen)
        w = (w * (0.25 / float(F.conv2d(cur, w, padding=1).abs().max()))).float()
        params += [w, b]
        if k < 5:
            cur = torch.cat([lrelu(F.conv2d(cur, w.double(), b.double(), padding=1), slope), cur], 1)
    g_x6 = torch.randn(N, ch_in + sum(DENSE_OCS), H, W, generator=gen)
    g_flow = torch.randn(N, 2, H, W, generator=gen)
    return {'x': x, 'params': params, 'g_x6': g_x6, 'g_flow': g_flow, 'slope': float(slope)}


def dense_counts(ch_in, N, H, W):
    """n per tensor: {'x6', 'flow', 'dx', 'dw': [6], 'db': [6], 'z': [5]} (layers 1..5, then the head)."""
    P = N * H * W
    cins = [ch_in + sum(DENSE_OCS[:k]) for k in range(5)]
    n_a, acc = [], 0
    for c in cins:
        acc += 9 * c + 5
        n_a.append(acc)
    n = {'x6': n_a[4], 'flow': n_a[4] + 9 * (ch_in + sum(DENSE_OCS)) + 2, 'z': list(n_a)}
    n_gy, longest = [0] * 5, 18
    for m in range(5, 0, -1):
        n_gy[m - 1] = (2 + 5 - m) + 1 + longest
        longest = 9 * DENSE_OCS[m - 1] + 3 + n_gy[m - 1]
    n['dx'] = 7 + longest
    n_x = [0] + n_a[:4]
    n['dw'] = [P + 3 + n_x[k] + n_gy[k] for k in range(5)] + [P + n['x6']]
    n['db'] = [P + n_gy[k] for k in range(5)] + [P]
    return n


# ------------------------------------------------------------------------------------------------------------------
def context_twin(x, params, slope, taps=None, dilations=CONTEXT_DILATIONS, mutate=None):
    """The network's output; params = (w1, b1, ..., w7, b7).  mutate 'phase_shift': phase (0, 0) of layer 2's activation
    (its pixels (2i, 2j)) shifted by one pixel of the phase image along W, zero filled."""
    for k, d in enumerate(dilations):
        x = F.conv2d(x, params[2 * k], params[2 * k + 1], padding=d, dilation=d)
        if k < 6:
            if taps is not None:
                taps.append(x)
            x = lrelu(x, slope)
        if mutate == 'phase_shift' and k == 1:
            ph = x[:, :, 0::2, 0::2]
            x = x.clone()
            x[:, :, 0::2, 0::2] = torch.cat([torch.zeros_like(ph[..., :1]), ph[..., :-1]], 3)
    return x


def context_grads(x, params, slope, g_out, dilations=CONTEXT_DILATIONS, mutate=None, dtype=torch.float64):
    """{'out', 'dx', 'dw': [7], 'db': [7], 'z': [6]} in float64 (dtype: as dense_grads)."""
    x, g_out = to64([x, g_out], dtype)
    x.requires_grad_(True)
    params = [p.requires_grad_(True) for p in to64(params, dtype)]
    taps = []
    out = context_twin(x, params, slope, taps, dilations, mutate)
    grads = torch.autograd.grad(out, [x] + params, g_out)
    return {'out': out.detach(), 'dx': grads[0], 'dw': list(grads[1::2]), 'db': list(grads[2::2]), 'z': [z.detach() for z in taps]}


def context_magnitudes(x, params, g_out):
    return context_grads(x.abs(), [p.abs() for p in params], 1.0, g_out.abs())


def context_fixture(ch_in, N, H, W, slope, seed=0):
    """{'x', 'params', 'g_out', 'slope'}: fp32 tensors on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ch_in, H, W, generator=gen)
    cur, params = x.double(), []
    for k, (oc, d) in enumerate(zip(CONTEXT_KS, CONTEXT_DILATIONS)):
        w, b = _scaled_layer(cur, oc, gen)
        w = (w * (0.25 / float(F.conv2d(cur, w, padding=d, dilation=d).abs().max()))).float()
        params += [w, b]
        if k < 6:
            cur = lrelu(F.conv2d(cur, w.double(), b.double(), padding=d, dilation=d), slope)
    g_out = torch.randn(N, 2, H, W, generator=gen)
    return {'x': x, 'params': params, 'g_out': g_out, 'slope': float(slope)}


def context_counts(ch_in, N, H, W):
    """n per tensor: {'out', 'dx', 'dw': [7], 'db': [7], 'z': [6]}."""
    P = N * H * W
    cs = (ch_in,) + CONTEXT_KS[:6]
    n_a, acc = [], 0
    for c in cs[:6]:
        acc += 9 * c + 5
        n_a.append(acc)
    n = {'out': n_a[5] + 9 * cs[6] + 2, 'z': list(n_a)}
    n_gy, n_dx = [0] * 7, 18
    for k in range(5, -1, -1):
        n_gy[k] = n_dx + 1
        n_dx = 9 * CONTEXT_KS[k] + 3 + n_gy[k]
    n['dx'] = n_dx
    n_x = [0] + n_a
    n['dw'] = [P + 3 + n_x[k] + n_gy[k] for k in range(7)]
    n['db'] = [P + n_gy[k] for k in range(7)]
    return n


def sign_margins(zs, mag_zs):
    """min |z| / M(z) per layer: how far every pre-activation is from its kink, in the unit of the caps."""
    return [float((z.abs() / m).min()) for z, m in zip(zs, mag_zs)]
