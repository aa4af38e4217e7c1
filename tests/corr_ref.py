"""Shared by tests/test_corr_ref_cpu.py and tests/test_corr_gpu.py: float64 restatements, in plain torch on the CPU, of the two
kernel families at the front of every pyramid level -- the cost volume with its fused LeakyReLU (csrc/corr.hip,
csrc/corr_v2.hpp), forward and both input gradients, and the feature normalisation in front of it (csrc/featnorm.hip),
forward, statistics and both gradients -- together with the error bounds the GPU tests hold the kernels to, the launch
predicates of both families restated, the seeded inputs and every shape list of those tests, and deliberate mutations.
Nothing here imports the oracle or the product.

Reference arithmetic: models/correlation_native.py:13-23, models/pwclite_uflow.py:30-38 ('joint'),
models/uflow_model.py:8-50 as PWCFlow calls it ('avg').  u = 2^-24 is the unit roundoff of fp32.

COST VOLUME
    pre[b, i n + j, y, x] = (1/C) sum_c x1[b,c,y,x] x2[b,c,y+i-d,x+j-d]   (x2 = 0 outside the image), n = 2d + 1
    S  (companion)        = (1/C) sum_c |x1| |x2|
    out = pre if pre > 0 else slope pre        (slope: the fp32 value the kernel is handed)
    ge  = go if pre > 0 else go slope          (at pre <= 0 the derivative is `slope`: the kernels test `v > 0`)
    gx1[c,p] = (1/C) sum_dsp ge[dsp,p] x2[c,p+dsp]        A1 = (1/C) sum |ge| |x2|
    gx2[c,q] = (1/C) sum_dsp ge[dsp,q-dsp] x1[c,q-dsp]    A2 = (1/C) sum |ge| |x1|     (p = q - dsp inside the image)

  Bound of a sum of k fp32 products accumulated in ANY order and grouping, fused or not: every product carries at most
  one rounding (u; none under fma) and every partial sum one more, a term passes through at most k - 1 additions, so the
  sum errs by at most ((1 + u)^k - 1) sum |a||b| = k u sum|a||b| to first order.  The scale by the ROUNDED 1/C costs 2u (the
  constant, the product), a division by C costs u.  (k + 3) u S covers both and the second-order terms for every k used
  here (k u < 2^-14).  It knows nothing of the order: the three waves of the fast path, its four channel groups meeting
  through LDS, the channel split of the backward over workgroups and the serial loop of the generic kernels are all
  covered.
      forward   |pre - ref| <= (C + 3) u S =: Ef;   |out - ref| <= max(1, slope) Ef + u |out|   (LeakyReLU is Lipschitz
                with max(1, slope), so a sign of pre that differs inside Ef is covered too; + u for the product with slope)
      gradient  k = n^2 terms per element; ge = go slope is one rounding more per term:  (n^2 + 4) u A
  LeakyReLU kink: the backward takes the derivative from the sign of the KERNEL's pre-activation.  The recipes zero go
  wherever 0 < |pre| <= Ef or Ef > 0 = pre (kink_mask): everywhere else kernel and reference have the same sign.  Where
  Ef = 0 every product is exactly zero (a displacement outside the image), both sides hold pre = 0 exactly and take
  `slope`.  Nothing is excluded from any comparison; the CPU test caps the zeroed share of go at 0.1 %.
  bf16 storage: the reference is taken on the bf16-rounded inputs; products of two bf16 values are exact in fp32, the
  same bound holds.

FEATURE NORMALISATION   (x1, x2: [B, n]; N = 2n; one (mu, var) per sample; sd = sqrt(var + 1e-16); y_i = (x_i - mu) / sd)
    joint: mu = sum(x1, x2) / N,      var = sum((x - mu)^2 over both) / (N - 1)
    avg:   mu = (m1 + m2) / 2,        var = (v1 + v2) / 2,  v_i = sum((x_i - m_i)^2) / (n - 1)
    backward, r = 1/sd, G = sum g, Q = sum g (x - mu) over both tensors:
    joint: dx   = r g - r G / N - r^3 Q (x - mu) / (N - 1)
    avg:   dx_i = r g - r G / N - r^3 Q (x - m_i) / (2 (n - 1))

  What the kernels round.  The longest fp32 partial they form holds k = 16 values per tensor (moment_kernel and
  fwd_small_kernel: 4 float4 per thread and trip, featnorm::moment_partials of csrc/featnorm_stats.hpp, which
  moment_kernel writes out around the same featnorm::moment_step); from there on everything is double.  The scalar
  loops, which replace the float4 loops altogether when n % 4 != 0, convert every value to double before its first
  operation: k = 1, no fp32 rounding at all.  The bounds take k from n % 4 (`partial=`; the CPU test's comparison with the
  fp32 oracle, which has no such path, asks for k = 16 everywhere).  With S = sum |x|, Q2 = sum x^2 and
  dbl = 2^-53 (n / 256 + 64) -- no value passes through more double additions than that: at most n / 256 in its thread,
  6 in its wave, 16 across the waves, 32 + 6 over the partial rows --
      eA = (k - 1) u + dbl    sum of k values, any order:      |d sum x|   <= eA S         (15 u for the float4 loops)
      eQ = k u + dbl          chain of k fma (0 for k = 1):    |d sum x^2| <= eQ Q2        (16 u)
      abs_m_i = eA S_i / n + u |m_i|                           (the rounding of the statistic to fp32)
      abs_mu  = eA (S_1 + S_2) / N + u |mu|
      joint:  d var = (eQ (Q2_1 + Q2_2) + 2 |mu| eA (S_1 + S_2)) / (N - 1)         [var = (sum x^2 - N mu^2) / (N - 1)]
      avg:    d var = 1/2 sum_i (eQ Q2_i + 2 |m_i| eA S_i) / (n - 1)
      rel_var = d var / var = u (N / (N - 1)) (16 kappa + 30 kappa') + ...,   kappa = E[x^2] / var,  kappa' = |mu| E|x| / var
      rel_sd  = rel_var / (1 + sqrt(1 - rel_var)) + 2 u      (exact for the downward side; 2u: var to fp32, + 1e-16f, sqrtf)
  kappa is the cancellation factor of sum x^2 - N mu^2: 1 for centred features, (offset / spread)^2 + 1 otherwise.
      forward   |y - ref| <= |y| (2u + rel_sd / (1 - rel_sd)) + abs_mu / sd     (2u: the subtraction and the division, both
                correctly rounded: hipcc's default for fp32, the Makefile passes no fast-math flag)
      stats     m_i: abs_m_i;  mu: abs_mu;  sd: rel_sd sd
  Backward.  The sums hold 2k = 32 values per fp32 partial (two tensors): eG = 31 u + dbl for G against Gabs = sum |g|;
  eQg = 33 u + dbl for Q against Qabs = sum |g| |x - mu| (the rounded x - mu, 32 fma); the scalar loops round x - mu in
  fp32 and nothing else: eG = dbl, eQg = u + dbl.  Q is centred on the ROUNDED mu: + |G| abs_mu.  rs = rel_sd / (1 - rel_sd) is the relative error of r.  The three coefficients are rounded to fp32:
      d rf = r (rs + u)
      d cg = |cg| (rs + u) + r eG Gabs / N                                        cg = r G / N
      d cq = |cq| (3 rs (1 + rs)^2 + u) + r^3 (eQg Qabs + |G| abs_mu) / den       cq = r^3 Q / den, den = N - 1 or 2 (n - 1)
      |dx - ref| <= |g| d rf + d cg + |x - c| d cq + |cq| abs_c + 2u (|r g| + |cg|) + 3u |cq (x - c)|
  with c the centre (mu or m_i) and abs_c its bound; the last two terms are fma(rf, g, -cg), x - c, the product and the
  final subtraction.  The GPU test hands the backward the statistics the forward kernel wrote, as the product does.

  What this says about "exact to fp32 for any mean / spread ratio" (csrc/featnorm.hip's header before this change): the
  double stage is exact, but the 16-value fp32 partials in front of it are not, and their error is amplified by kappa.
  At offset 25 / spread 1 (kappa = 480 .. 500 for the recipes here) the derived forward bound is |y| 7e-4 + 2.4e-5, about
  3e-3 at |y| = 4: NOT tighter than the atol = 4e-4 tests/test_hip_parity.py allows there (the CPU test pins this figure).
  At offset 1 / spread 1e-3 (kappa = 8e5) rel_var >= 1: the worst case cancels the whole variance and the bound is
  infinite for the float4 loops -- the comparison then only demands finite outputs.  That is no artefact of the
  derivation: on the MI355X the float4 paths return sd 0.2 .. 0.4 % off there (y up to 1.6e-2 off).  The scalar loops
  (k = 1) keep a finite bound there, |y| 2e-6 + u |mu| / sd = 5e-5, and the kernels hold it: sd to 4e-8 (DESIGN.md
  section 23).  The claim held for the double stage only; the comment now says so.
"""
import types

import torch
import torch.nn.functional as F

from tests.loss_kernels_ref import D, U, _gen, worst  # noqa: F401 (re-exported)

CORR_MUTATIONS_FWD = ('sign', 'swap', 'cplus1', 'replicate', 'window')
CORR_MUTATIONS_BWD = ('gx2_shifted', 'deriv1')
FEAT_MUTATIONS_FWD = ('bessel_joint', 'bessel_avg', 'joint_avg_moments')
FEAT_MUTATIONS_BWD = ('bessel_joint', 'bessel_avg', 'avg_centre_mu', 'joint_avg_moments', 'no_G')


def slope32(slope):
    """the value the kernel is handed: `slope` rounded to fp32"""
    return float(torch.tensor(float(slope), dtype=torch.float32))


# ======================================================================================================================
# cost volume
# ======================================================================================================================
def _shift(i, j, d, mutate):
    """(dy, dx) of volume channel i n + j, or None when the mutated window never computes it"""
    n = 2 * d + 1
    dy, dx = i - d, j - d
    if mutate == 'sign':
        dy, dx = -dy, -dx
    elif mutate == 'swap':
        dy, dx = dx, dy
    elif mutate == 'window' and (i == n - 1 or j == n - 1):
        return None
    return dy, dx


def corr_ref(x1, x2, d, slope=1.0, mutate=None):
    """-> namespace pre, S, bound_pre (= Ef), out, bound_out; all [B, n^2, H, W] float64.
    mutate (WRONG on purpose): 'sign' displacement sign flipped, 'swap' dy / dx swapped, 'cplus1' division by C + 1,
    'replicate' border-replicate padding instead of zeros, 'window' the displacement loop stops at d - 1 (last row and
    column of the window left zero)."""
    x1, x2 = x1.to(D), x2.to(D)
    B, C, H, W = x1.shape
    n = 2 * d + 1
    sl = slope32(slope)
    if mutate == 'replicate':  # F.pad's replicate mode needs pad < size: index instead
        yi = torch.arange(-d, H + d).clamp(0, H - 1)
        xi = torch.arange(-d, W + d).clamp(0, W - 1)
        x2p = x2[:, :, yi][:, :, :, xi]
    else:
        x2p = F.pad(x2, (d, d, d, d))
    a1, a2p = x1.abs(), x2p.abs()
    pre, S = x1.new_zeros(B, n * n, H, W), x1.new_zeros(B, n * n, H, W)
    div = float(C + 1 if mutate == 'cplus1' else C)
    for i in range(n):
        for j in range(n):
            sh = _shift(i, j, d, mutate)
            if sh is None:
                continue
            w = x2p[:, :, d + sh[0]:d + sh[0] + H, d + sh[1]:d + sh[1] + W]
            pre[:, i * n + j] = (x1 * w).sum(1) / div
            S[:, i * n + j] = (a1 * a2p[:, :, d + sh[0]:d + sh[0] + H, d + sh[1]:d + sh[1] + W]).sum(1) / div
    out = types.SimpleNamespace(pre=pre, S=S)
    out.bound_pre = (C + 3) * U * S
    out.out = torch.where(pre > 0, pre, pre * sl)
    out.bound_out = max(1.0, abs(sl)) * out.bound_pre + U * out.out.abs()
    return out


def kink_mask(fwd):
    """[B, n^2, H, W] bool: where the sign of the kernel's pre-activation is not settled by the forward bound"""
    return (fwd.pre.abs() <= fwd.bound_pre) & (fwd.bound_pre > 0)


def corr_grads_ref(go, pre, x1, x2, d, slope=1.0, mutate=None):
    """-> namespace gx1, A1, bound1, gx2, A2, bound2 ([B,C,H,W] float64).  pre: the reference's pre-activation.
    mutate (WRONG on purpose): 'gx2_shifted' gx2 reads go at its own pixel q instead of q - dsp, 'deriv1' the LeakyReLU
    derivative below zero is taken as 1."""
    go, pre, x1, x2 = go.to(D), pre.to(D), x1.to(D), x2.to(D)
    B, C, H, W = x1.shape
    n = 2 * d + 1
    sl = 1.0 if mutate == 'deriv1' else slope32(slope)
    ge = torch.where(pre > 0, go, go * sl)
    x2p, a2p = F.pad(x2, (d, d, d, d)), F.pad(x2.abs(), (d, d, d, d))
    gx1, A1 = torch.zeros_like(x1), torch.zeros_like(x1)
    g2p, A2p = x1.new_zeros(B, C, H + 2 * d, W + 2 * d), x1.new_zeros(B, C, H + 2 * d, W + 2 * d)
    a1 = x1.abs()
    x1p, a1p = F.pad(x1, (d, d, d, d)), F.pad(a1, (d, d, d, d))
    for i in range(n):
        for j in range(n):
            g = ge[:, i * n + j].unsqueeze(1)
            gx1 += g * x2p[:, :, i:i + H, j:j + W]
            A1 += g.abs() * a2p[:, :, i:i + H, j:j + W]
            if mutate == 'gx2_shifted':  # gx2[q] += ge[dsp, q] x1[q - dsp]
                k, l = n - 1 - i, n - 1 - j
                g2p[:, :, d:d + H, d:d + W] += g * x1p[:, :, k:k + H, l:l + W]
                A2p[:, :, d:d + H, d:d + W] += g.abs() * a1p[:, :, k:k + H, l:l + W]
            else:
                g2p[:, :, i:i + H, j:j + W] += g * x1
                A2p[:, :, i:i + H, j:j + W] += g.abs() * a1
    out = types.SimpleNamespace(gx1=gx1 / C, A1=A1 / C, gx2=g2p[:, :, d:d + H, d:d + W] / C, A2=A2p[:, :, d:d + H, d:d + W] / C)
    out.bound1 = (n * n + 4) * U * out.A1
    out.bound2 = (n * n + 4) * U * out.A2
    return out


# ---- launch predicates, RESTATED.  If the kernels' thresholds change these drift silently: they only label test ids and let
# ---- the CPU test assert that the shape lists below reach every branch; no kernel result depends on them. -------------
def _up(a, b):
    return -(-a // b)


def fast_eligible(C, W, d):
    """corr_v2::eligible, csrc/corr_v2.hpp:650"""
    return d == 4 and W % 4 == 0 and C % 4 == 0


def fast_tiles(B, H, W, nmodes=1):
    """corr_v2.hpp:656 (forward) and :685 (backward: times the number of gradients asked for); tiles of 8 rows x 32 columns"""
    return _up(W, 32) * _up(H, 8) * B * nmodes


def fast_grid_pad(tiles):
    """padding workgroups of the rounded-up grid (grid_for_tiles, corr_v2.hpp:107)"""
    return 8 * _up(tiles, 8) - tiles


def fast_fwd_branch(B, C, H, W):
    """corr_v2::launch_fwd, corr_v2.hpp:663-670"""
    tiles = fast_tiles(B, H, W)
    if tiles <= 160 and (C // 4) % 4 == 0 and C // 4 >= 8:
        return 'groups4'
    return 'ring2' if tiles >= 768 else 'ring4'


def fast_bwd_nsplit(B, C, H, W, nmodes):
    """corr_v2::launch_bwd, corr_v2.hpp:686-687"""
    tiles, ns = fast_tiles(B, H, W, nmodes), 1
    while ns * 2 <= C // 4 and tiles * ns * 2 <= 1024:
        ns *= 2
    return ns


def fast_bwd_nsplit_uncut(C):
    """what the channel count alone would allow"""
    ns = 1
    while ns * 2 <= C // 4:
        ns *= 2
    return ns


def fast_bwd_ring(B, H, W, nmodes):
    """corr_v2.hpp:702-706"""
    return 2 if fast_tiles(B, H, W, nmodes) >= 768 else 3


def general_fwd_strip(B, H, W):
    """pixels per lane of dispatch_fwd, csrc/corr.hip:337-344"""
    px = B * H * W
    if W >= 24 and px >= 32768:
        return 8
    return 4 if (W >= 12 and px >= 8192) else 2


def general_bwd_threads(B, H, W):
    """workgroup size of dispatch_bwd, csrc/corr.hip:346-353"""
    px = B * H * W
    if W >= 48 and px >= 65536:
        return 256
    return 128 if (W >= 24 and px >= 8192) else 64


def generic_capped(elements):
    """the d > 4 kernels cap their grid at 65535 workgroups of 256 threads (corr.hip:396, :511)"""
    return _up(elements, 256) > 65535


def corr_path(B, C, H, W, d):
    if fast_eligible(C, W, d):
        return 'fast'
    return 'general' if d <= 4 else 'generic'


FEAT_SMALL_N = 16384  # SMALL_N of csrc/featnorm.hip


def feat_rows(B, n, floats_per_block=4096):
    """(workgroups per sample wanted, allowed): af_blocks_per_sample of csrc/common.hpp, as arflow_featnorm_fwd
    (csrc/featnorm.hip) calls it for its moment pass (NT * VPT: 256 threads x 16 floats per trip)"""
    return max(_up(n, floats_per_block), 1), _up(2048, B)


def feat_path(B, n):
    """'small' (one launch: n <= SMALL_N in arflow_featnorm_fwd, featnorm.hip), 'large' or 'capped' (the grid-stride loops of
    moment_kernel / bwd_sum_kernel take a second trip) + '/v4' or '/scalar' (n % 4: `n4` of featnorm::moment_partials,
    csrc/featnorm_stats.hpp)"""
    if n <= FEAT_SMALL_N:
        p = 'small'
    else:
        want, allowed = feat_rows(B, n)
        p = 'capped' if want > allowed else 'large'
    return p + ('/v4' if n % 4 == 0 else '/scalar')


# ---- inputs and shape lists ------------------------------------------------------------------------------------------
def corr_inputs(B, C, H, W, d):
    """(x1, x2, go) fp32, seeded by the shape"""
    gen = _gen(61, B, C, H, W, d)
    n = 2 * d + 1
    return (torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen),
            torch.randn(B, n * n, H, W, generator=gen))


def bf16_round(t):
    return t.to(torch.bfloat16).float()


SLOPES = (1.0, 0.1)
# fast path forward, d = 4: (B, C, H, W) -> branch
FAST_FWD = [
    ((1, 32, 9, 36), 'groups4'), ((3, 48, 8, 4), 'groups4'), ((160, 32, 8, 4), 'groups4'), ((161, 32, 8, 4), 'ring4'),
    ((1, 4, 3, 4), 'ring4'), ((2, 12, 20, 36), 'ring4'), ((1, 20, 17, 68), 'ring4'), ((1, 8, 100, 4), 'ring4'),
    ((768, 4, 8, 4), 'ring2'), ((767, 4, 8, 4), 'ring4'), ((80, 8, 33, 36), 'ring2'),
]
# fast path backward: (B, C, H, W), request ('both' / 'gx1' / 'gx2'), activation ('none': slope 1; 'sign': the autograd
# function with slope 0.1, sign words; 'out': the raw entry point with the forward output and no sign words)
FAST_BWD = ([((2, c, 20, 36), 'both', 'sign') for c in (4, 12, 20, 24, 32)]
            + [((40, 32, 8, 36), 'both', 'sign'), ((384, 4, 8, 4), 'both', 'sign'), ((768, 4, 8, 4), 'gx2', 'out'),
               ((768, 4, 8, 4), 'gx1', 'none')]
            + [((2, 12, 20, 36), r, a) for a in ('none', 'sign', 'out') for r in ('both', 'gx1', 'gx2')
               if (r, a) != ('both', 'sign')])
# general and generic paths, fp32: (B, C, H, W), d, backward too
GENERAL = ([((1, 7, 9, 11), dd, True) for dd in (1, 2, 3, 4)]
           + [((1, 3, 91, 91), 4, True), ((1, 3, 130, 253), 4, True), ((1, 5, 93, 90), 4, True), ((1, 3, 258, 255), 4, True),
              ((1, 3, 258, 255), 2, True), ((2, 3, 9, 14), 6, True), ((1, 1, 316, 316), 6, False)])
BF16 = (1, 8, 91, 92)
# recipes small enough for the fp32 oracle, the mutations and the kink cap on the CPU (outputs below ~1M elements)
CORR_CPU = ([(s, 4) for s, _ in FAST_FWD if s[0] * s[2] * s[3] <= 12000] + [(s, dd) for s, dd, _ in GENERAL if s[2] * s[3] <= 12000]
            + [(BF16, 4)])

# feature normalisation: (B, n, offset, spread)
FEAT_SHAPES = [(1, 2), (3, 5), (2, 16383), (2, 16384), (2, 16385), (2, 16388), (2, 20484), (2, 20487), (512, 20484), (512, 20487)]
FEAT_OFFSETS = [(0.0, 1.0), (3.0, 1.0), (25.0, 1.0), (1.0, 1e-3)]
FEAT_OFFSET_SHAPES = [(2, 792), (2, 16388), (2, 20487)]
FEAT = ([(B, n, 0.0, 1.0) for B, n in FEAT_SHAPES]
        + [(B, n, o, s) for B, n in FEAT_OFFSET_SHAPES for o, s in FEAT_OFFSETS if (B, n, o, s) != (2, 16388, 0.0, 1.0)
           and (B, n, o, s) != (2, 20487, 0.0, 1.0)])
FEAT_CPU = [r for r in FEAT if r[0] * r[1] <= 50000]
MODES = ('joint', 'avg')


def feat_inputs(B, n, offset, spread):
    """(x1, x2, g1, g2) fp32 [B, n].  The two tensors differ in mean and in spread (m1 != m2 != mu, v1 != v2), the output
    gradients have a mean (G matters at every size)."""
    gen = _gen(71, B, n, int(offset * 8), int(spread * 1e6))
    z = torch.randn(4, B, n, generator=gen)
    x1 = (offset + spread * z[0]).float()
    x2 = (offset + spread * (0.25 + 1.25 * z[1])).float()
    return x1.contiguous(), x2.contiguous(), (0.5 + z[2]).contiguous(), (z[3] - 0.25).contiguous()


# ======================================================================================================================
# feature normalisation
# ======================================================================================================================
def _dbl(n):
    return 2.0 ** -53 * (n / 256.0 + 64.0)


def feat_partial(n):
    """values per tensor in the longest fp32 partial: the float4 loops' 16 (featnorm::VPT), or 1 for the scalar loops
    (featnorm::moment_partials, csrc/featnorm_stats.hpp)"""
    return 16 if n % 4 == 0 else 1


def featnorm_ref(x1, x2, mode, mutate=None, partial=None):
    """x1, x2 [B, n].  -> namespace y1, y2, bound1, bound2 [B, n]; stats, stats_bound [B, 4] (m1, m2, mu, sd); kappa [B];
    abs_mu, abs_m1, abs_m2, rel_sd, rs [B, 1] (see the docstring of this file).
    mutate (WRONG on purpose): 'bessel_joint' 2n for 2n - 1, 'bessel_avg' n for n - 1, 'joint_avg_moments' the joint mode takes
    the avg variance.  partial: values per fp32 partial the bounds assume (default: feat_partial(n))."""
    assert mode in MODES
    x1, x2 = x1.to(D), x2.to(D)
    B, n = x1.shape
    N = 2 * n
    m1, m2 = x1.mean(1, keepdim=True), x2.mean(1, keepdim=True)
    mu = (x1.sum(1, keepdim=True) + x2.sum(1, keepdim=True)) / N
    S1, S2 = x1.abs().sum(1, keepdim=True), x2.abs().sum(1, keepdim=True)
    Q1, Q2 = (x1 * x1).sum(1, keepdim=True), (x2 * x2).sum(1, keepdim=True)
    k = feat_partial(n) if partial is None else partial
    eA, eQ = (k - 1) * U + _dbl(n), (k if k > 1 else 0) * U + _dbl(n)
    joint = mode == 'joint' and mutate != 'joint_avg_moments'
    if joint:
        den = N if mutate == 'bessel_joint' else N - 1
        var = (((x1 - mu) ** 2).sum(1, keepdim=True) + ((x2 - mu) ** 2).sum(1, keepdim=True)) / den
        dvar = (eQ * (Q1 + Q2) + 2 * mu.abs() * eA * (S1 + S2)) / (N - 1)
    else:
        den = n if mutate == 'bessel_avg' else n - 1
        var = 0.5 * (((x1 - m1) ** 2).sum(1, keepdim=True) + ((x2 - m2) ** 2).sum(1, keepdim=True)) / den
        dvar = 0.5 * ((eQ * Q1 + 2 * m1.abs() * eA * S1) + (eQ * Q2 + 2 * m2.abs() * eA * S2)) / (n - 1)
    sd = torch.sqrt(var + 1e-16)
    o = types.SimpleNamespace(m1=m1, m2=m2, mu=mu, var=var, sd=sd, n=n, mode=mode, partial=k)
    o.kappa = ((Q1 + Q2) / N / var).squeeze(1)
    o.abs_m1, o.abs_m2 = eA * S1 / n + U * m1.abs(), eA * S2 / n + U * m2.abs()
    o.abs_mu = eA * (S1 + S2) / N + U * mu.abs()
    inf = torch.full_like(var, float('inf'))
    o.rel_var = dvar / (var + 1e-16)
    # rel_var >= 1: the worst case of the fp32 partials cancels the whole variance -- nothing is guaranteed (bound = inf)
    o.rel_sd = torch.where(o.rel_var < 1, o.rel_var / (1 + torch.sqrt(1 - o.rel_var.clamp(max=1.0))) + 2 * U, inf)
    o.rs = torch.where(o.rel_sd < 1, o.rel_sd / (1 - o.rel_sd).clamp_min(1e-300), inf)
    o.y1, o.y2 = (x1 - mu) / sd, (x2 - mu) / sd
    o.bound1 = torch.nan_to_num(o.y1.abs() * (2 * U + o.rs) + o.abs_mu / sd, nan=float('inf'), posinf=float('inf'))
    o.bound2 = torch.nan_to_num(o.y2.abs() * (2 * U + o.rs) + o.abs_mu / sd, nan=float('inf'), posinf=float('inf'))
    o.stats = torch.cat([m1, m2, mu, sd], 1)
    o.stats_bound = torch.cat([o.abs_m1, o.abs_m2, o.abs_mu, o.rel_sd * sd], 1)
    return o


def featnorm_grads_ref(g1, g2, x1, x2, mode, mutate=None, partial=None):
    """-> namespace d1, d2, bound1, bound2 [B, n] float64: the gradients of sum(g1 y1) + sum(g2 y2) and their bounds.
    mutate (WRONG on purpose): featnorm_ref's, and 'avg_centre_mu' (avg centres the Q term on mu instead of m_i), 'no_G' (the
    G term dropped)."""
    g1, g2, x1, x2 = g1.to(D), g2.to(D), x1.to(D), x2.to(D)
    f = featnorm_ref(x1, x2, mode, mutate if mutate in FEAT_MUTATIONS_FWD else None, partial)
    n, N = f.n, 2 * f.n
    r = 1.0 / f.sd
    G = g1.sum(1, keepdim=True) + g2.sum(1, keepdim=True)
    Gabs = g1.abs().sum(1, keepdim=True) + g2.abs().sum(1, keepdim=True)
    Q = (g1 * (x1 - f.mu)).sum(1, keepdim=True) + (g2 * (x2 - f.mu)).sum(1, keepdim=True)
    Qabs = (g1 * (x1 - f.mu)).abs().sum(1, keepdim=True) + (g2 * (x2 - f.mu)).abs().sum(1, keepdim=True)
    if mode == 'joint':
        den = float(N if mutate == 'bessel_joint' else N - 1)
        c1 = c2 = f.mu
        ac1 = ac2 = f.abs_mu
    else:
        den = 2.0 * (n if mutate == 'bessel_avg' else n - 1)
        c1, c2 = (f.mu, f.mu) if mutate == 'avg_centre_mu' else (f.m1, f.m2)
        ac1, ac2 = f.abs_m1, f.abs_m2
    cg = torch.zeros_like(G) if mutate == 'no_G' else r * G / N
    cq = r ** 3 * Q / den
    eG, eQg = (2 * f.partial - 1) * U + _dbl(2 * n), ((2 * f.partial + 1) if f.partial > 1 else 1) * U + _dbl(2 * n)
    d_rf = r * (f.rs + U)
    d_cg = cg.abs() * (f.rs + U) + r * eG * Gabs / N
    d_cq = cq.abs() * (3 * f.rs * (1 + f.rs) ** 2 + U) + r ** 3 * (eQg * Qabs + G.abs() * f.abs_mu) / den
    o = types.SimpleNamespace(fwd=f)

    def one(g, x, c, ac):
        t = cq * (x - c)
        dx = r * g - cg - t
        b = g.abs() * d_rf + d_cg + (x - c).abs() * d_cq + cq.abs() * ac + 2 * U * ((r * g).abs() + cg.abs()) + 3 * U * t.abs()
        return dx, torch.nan_to_num(b, nan=float('inf'), posinf=float('inf'))
    o.d1, o.bound1 = one(g1, x1, c1, ac1)
    o.d2, o.bound2 = one(g2, x2, c2, ac2)
    return o
