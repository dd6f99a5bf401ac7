"""What tests/test_norm_edges_gpu.py and tests/test_norm_edges_cpu.py share: the seeded inputs of the normalisation / reduction
edge cases (csrc/norm.hip, dh_colsum of csrc/pointwise.hip), the float64 references written out, and the two checkers.

Every kernel gets ITS inputs from here, not from the kernel in front of it: the statistics the apply / backward kernels read are
formed in float64 from the dtype-rounded x and rounded to float32; the per-tile partials bn_finalize and bn_bwd_from_partials read
are summed per tile in float64 and rounded to float32.  The references work on those same rounded inputs, cast up.

Where a kernel only SUMS, the data are integers in [-8, 8]: exact in bf16 and float32, every partial and total below 2^24, so
the result is exact in any summation order and the tests assert equality (`exact`)."""
import functools

import torch
import torch.nn.functional as F

from _bounds import close

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
V = {F32: 4, BF16: 8}                     # elements of one 16-byte piece (common.h: V16<T>::N)

# ---- the launch arithmetic the shapes below are computed from ----
BLOCK = 256                               # threads of every kernel here
HOIST_WG = 2048                           # norm.hip hoist_grid(): cap = 2048 / groups workgroups per group
HOIST_PIECES_PER_WG = 512                 # norm.hip hoist_grid(): g = (gvec + 511) / 512 -- two pieces per thread
EW_WG = 4096                              # norm.hip ew_grid(): g > 4096 ? 4096 (generic bn_apply_kernel / bn_bwd_apply_kernel)
BWD_CHUNKS = 1024                         # norm.hip bn_bwd_impl(): bpg = 1024 / groups chunks of a group's pixels
FIN_WAVES, WAVE = 4, 64                   # norm.hip bn_finalize_kernel: wpg = 4 / G wavefronts per group, step = 64 * wpg
LN_BWD_WG, LN_BWD_ROWS = 512, 32          # norm.hip ln_bwd_grid(): g > 512 ? 512; ln_bwd_kernel: base += gridDim.x * 32
LN_ROWS_PER_WAVE = 8                      # norm.hip ln_fwd_kernel: 8 lanes per row, 64 lanes per wavefront
RED_PHASES, RED_UNROLL = 8, 4             # common.h dh_reduce_partials_body: 8 row phases, `t + 24 < nt`, t += 32
EXACT_LIMIT = 1 << 24                     # integers up to here are exact in float32
IMAX = 8                                  # |integer data| <= 8


def name(dtype):
    return "f32" if dtype == F32 else "bf16"


def hoisted(dtype, C):
    """norm.hip launch_bn_apply / launch_bn_bwd_apply: (256 * V) % C == 0 takes the hoisted kernel, anything else the generic one"""
    return (BLOCK * V[dtype]) % C == 0


def colsum_vector_form(dtype, C):
    """pointwise.hip colsum_partial_kernel: C % V == 0 && 256 % (C / V) == 0 takes the 16-byte form, anything else the scalar one"""
    v = V[dtype]
    return C % v == 0 and BLOCK % (C // v) == 0


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (1 << 31)
    return torch.Generator().manual_seed(seed)


def ints(shape, g, bound_rows):
    """integer-valued float64 in [-IMAX, IMAX]; `bound_rows` = the largest number of them any kernel adds up"""
    assert IMAX * bound_rows < EXACT_LIMIT, (bound_rows, "sums would leave float32's exact integers")
    return torch.randint(-IMAX, IMAX + 1, shape, generator=g).double()


def rounded(x, dtype):
    """float64 values of `x` after rounding to `dtype`"""
    return x.to(dtype).double()


# ---- checkers ----
def exact(got, want, what):
    """got == want in every element (want float64, exactly representable in float32)"""
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite" % what
    bad = int((got != want).sum())
    print("%s: %d of %d elements differ from the exact sum (max |diff| %.3e)" % (what, bad, want.numel(), float((got - want).abs().max()) if want.numel() else 0.0))
    assert bad == 0, "%s: %d elements differ, first at %s" % (what, bad, (got != want).nonzero()[0].tolist())


def bounded(got, want, dtype, what, factor=1.0):
    """_bounds.close (max |got - want| <= factor x tol(dtype) x max |want|) for tensors that stay where they are: the error and the
    scale are reduced on `got`'s device, `close` then sees the worst element against the whole tensor's scale"""
    want = want.detach().double().to(got.device)
    g = got.detach().double()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    assert bool(torch.isfinite(g).all()), "%s: non-finite" % what
    if want.numel() == 0:
        return 0.0
    err = (g - want).abs().reshape(-1)
    k = int(err.argmax())
    scale = float(want.abs().max())
    print("%s: max err %.3e at %d, scale %.3e, ratio %.3e (bound factor %g, %s)" % (what, float(err[k]), k, scale, float(err[k]) / max(scale, 1e-6), factor, name(dtype)))
    close(g.reshape(-1)[k:k + 1].cpu(), want.reshape(-1)[k:k + 1].cpu(), dtype, what, scale=scale, factor=factor)
    return float(err[k]) / max(scale, 1e-6)


# ---- BatchNorm: inputs ----
def bn_stats(x, eps=1e-5):
    """x [G, P, C] float64 -> mean, invstd [G, C] float64 (biased variance, torch.nn.BatchNorm2d)"""
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + eps)


def bn_affine(C, g):
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).float()
    beta = (0.1 * torch.randn(C, generator=g)).float()
    return gamma, beta


def bn_x(dtype, G, P, C, g, small=False):
    """x [G, P, C] float64 on the grid k / 32, k in [-100, 140] (mean 0.6, std 2.2; exact in bf16).  small: the grid k / 8192, for
    one or two pixels per group -- see bn_bwd_case"""
    u = 2.0 ** -13 if small else 2.0 ** -5
    x = torch.randint(-100, 141, (G, P, C), generator=g).double() * u
    assert bool((rounded(x, dtype) == x).all())
    return x, u


@functools.lru_cache(maxsize=4)
def bn_apply_case(dtype, C, G, P, seed=0):
    """x, res [G, P, C] (dtype-rounded float64), scale / shift [G, C] float32 formed in float64 from x's statistics"""
    g = gen(1, C, G, P, seed, dtype == BF16)
    x, _ = bn_x(dtype, G, P, C, g)
    res = rounded(torch.randn(G, P, C, generator=g).double(), dtype)
    gamma, beta = bn_affine(C, g)
    mean, invstd = bn_stats(x)
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * gamma.double() * invstd).float()
    return dict(x=x, res=res, scale=scale, shift=shift, gamma=gamma, beta=beta)


def bn_apply_ref(c, residual, relu):
    y = c["x"] * c["scale"].double()[:, None] + c["shift"].double()[:, None]
    if residual:
        y = y + c["res"]
    return y.clamp(min=0) if relu else y


def pack_mask(positive, v):
    """relu_mask_byte (norm.hip): byte i = the mask of the 16-byte piece i, bit j = (y[v i + j] > 0)"""
    m = positive.reshape(-1, v).to(torch.int32)
    w = (1 << torch.arange(v, dtype=torch.int32, device=m.device))
    return (m * w).sum(1).to(torch.uint8)


def pieces_per_pixel(dtype, C):
    return C // V[dtype]


def apply_pixel_counts(dtype, C):
    """pixels per group: one pixel, then the counts whose pieces lie just below / at / just above 256 (one workgroup's threads: at
    <= 256 pieces the hoisted kernel runs its tail only) and just above 512 (a second workgroup)"""
    cvn = pieces_per_pixel(dtype, C)
    out = {1, max(1, 255 // cvn), -(-256 // cvn), -(-257 // cvn), 256 // cvn + 1, -(-513 // cvn)}
    return sorted(out)


MASKS = ("none", "out_relu", "mask_scale", "bits")


def bwd_pixel_counts(G):
    bpg = BWD_CHUNKS // G
    return [1, 2, bpg - 1, bpg, bpg + 1, 1200]


def bn_bwd_case(dtype, C, G, P, seed=0):
    """One BatchNorm-backward input.  x [G, P, C] on a grid (bn_x), dout integers (dbeta is exact), out_relu integers clamped at 0
    (half of them EXACT zeros: the `> 0` tie), mask_scale a signed power of two and mask_shift on x's grid, so that
    x * mask_scale + mask_shift is exact in float32 with or without a fused multiply-add and is exactly 0 on many elements.

    One or two pixels per group take x on a grid 256 times finer: with two pixels dx = gamma invstd (dy1 - dy2) / 2 x eps / (var + eps),
    and at var ~ 5 the last factor is 2e-6 -- the float32 difference dy - (s1 + xhat s2) / 2 that forms it carries 6e-8, percents of
    dx.  At var ~ eps the factor is ~0.1 and the stated bound says something about the kernel.  (tests/test_norm_edges_cpu.py
    measures both with torch in float32.)"""
    g = gen(2, C, G, P, seed, dtype == BF16)
    x, u = bn_x(dtype, G, P, C, g, small=P <= 2)
    dout = ints((G, P, C), g, G * P)
    out = torch.randint(-3, 4, (G, P, C), generator=g).double().clamp(min=0)
    ms = (2.0 ** torch.randint(-1, 2, (G, C), generator=g).double()) * (torch.randint(0, 2, (G, C), generator=g).double() * 2 - 1)
    mh = torch.randint(-100, 101, (G, C), generator=g).double() * u
    gamma, _ = bn_affine(C, g)
    mean, invstd = bn_stats(x)
    return dict(x=x, dout=dout, out=out, ms=ms.float(), mh=mh.float(), gamma=gamma, mean=mean.float(), invstd=invstd.float(), P=P, G=G, C=C)


def bn_bwd_dy(c, mask):
    if mask == "none":
        return c["dout"]
    if mask in ("out_relu", "bits"):
        return c["dout"] * (c["out"] > 0)
    pre = c["x"] * c["ms"].double()[:, None] + c["mh"].double()[:, None]      # exact: multiples of u / 2
    return c["dout"] * (pre > 0)


def bn_bwd_formula(x, dy, mean, invstd, gamma, sums=None):
    """float64, the backward of train-mode BatchNorm written out: x, dy [G, P, C]; mean, invstd [G, C]; gamma [C].
    sums = (s1, s2) [G, C] replaces the reduction (bn_bwd_from_partials).  Returns dx, dgamma, dbeta."""
    xhat = (x - mean[:, None]) * invstd[:, None]
    s1, s2 = (dy.sum(1), (dy * xhat).sum(1)) if sums is None else sums
    dx = gamma * invstd[:, None] * (dy - (s1[:, None] + xhat * s2[:, None]) / x.shape[1])
    return dx, s2.sum(0), s1.sum(0)


def bn_bwd_ref(c, mask):
    dy = bn_bwd_dy(c, mask)
    dx, dgamma, dbeta = bn_bwd_formula(c["x"], dy, c["mean"].double(), c["invstd"].double(), c["gamma"].double())
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dres=dy)


def tile_sizes(ntiles):
    """pixels of each tile: 1, 2, 3, 1, 2, 3, ..."""
    return torch.tensor([1 + (t % 3) for t in range(ntiles)])


def tile_sums(v, ntiles):
    """v [G, P, C] float64, P = tile_sizes(ntiles).sum() -> per-tile sums [C, G * ntiles] (one channel's tiles contiguous, group
    after group: the layout of the convolution epilogue's statistics)"""
    G, P, C = v.shape
    tid = torch.repeat_interleave(torch.arange(ntiles), tile_sizes(ntiles))
    assert tid.numel() == P
    s = torch.zeros(G, ntiles, C, dtype=torch.float64).index_add_(1, tid, v)
    return s.permute(2, 0, 1).reshape(C, G * ntiles)


def bn_bwd_partials_case(dtype, C, G, tpg, seed=0):
    """bn_bwd_from_partials: g (the masked gradient, integers), x, and the per-tile partials [2][C][G tpg] = (sum g, sum g xhat)
    in float32, summed per tile in float64"""
    P = int(tile_sizes(tpg).sum())
    c = bn_bwd_case(dtype, C, G, P, seed=seed + 50)
    xhat = (c["x"] - c["mean"].double()[:, None]) * c["invstd"].double()[:, None]
    part = torch.stack([tile_sums(c["dout"], tpg), tile_sums(c["dout"] * xhat, tpg)]).float()
    c["partial"] = part
    s = part.double().reshape(2, C, G, tpg).sum(-1).permute(0, 2, 1)       # [2][G][C]
    c["ref"] = bn_bwd_formula(c["x"], c["dout"], c["mean"].double(), c["invstd"].double(), c["gamma"].double(), sums=(s[0], s[1]))
    return c


# ---- bn_finalize: synthetic partials ----
FIN_C, FIN_CP = 24, 32
FIN_TILES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513]      # tiles per group: around 64 wpg and 2 x 64 wpg for wpg in (1, 2, 4)
FIN_INT = list(range(19)) + [20]          # integer-valued channels: sum x and sum x^2 are exact, so is the mean's float32 rounding
FIN_CONST = [19, 20]                      # constant over each group: 1.3f (E[x^2] - mean^2 of its rounded partials is -2e-8 .. -6e-8: the clamp) and 3 + group (exactly 0)
FIN_OFFSET = 21                           # mean = 8 x std
FIN_REAL = [21, 22, 23]


@functools.lru_cache(maxsize=64)
def finalize_case(G, tpg):
    """x [G, P, 24] float32 values (float64 tensor), P = 1 + 2 + 3 + 1 + ... pixels in `tpg` tiles per group (ONE pixel when tpg = 1:
    count = 1, var = 0 and the unbiased guard), and the partials [2][32][G tpg] float32 with NaN in the padding channels"""
    g = gen(3, G, tpg)
    P = int(tile_sizes(tpg).sum())
    x = ints((G, P, FIN_C), g, 64 * P)          # x^2 <= 64
    x[..., 19] = float(torch.tensor(1.3, dtype=F32))
    x[..., 20] = 3.0 + torch.arange(G, dtype=torch.float64)[:, None]
    x[..., FIN_OFFSET] = rounded(8.0 + torch.randn(G, P, generator=g).double(), F32)
    x[..., 22:] = rounded(torch.randn(G, P, 2, generator=g).double() * 1.5 + 0.3, F32)
    part = torch.full((2, FIN_CP, G * tpg), float("nan"), dtype=F32)
    part[0, :FIN_C] = tile_sums(x, tpg).float()
    part[1, :FIN_C] = tile_sums(x * x, tpg).float()
    assert bool((part[:, FIN_INT].double() == torch.stack([tile_sums(x, tpg), tile_sums(x * x, tpg)])[:, FIN_INT]).all())
    gamma, beta = bn_affine(FIN_C, g)
    rm = (0.1 * torch.randn(FIN_C, generator=g)).float()
    rv = (1 + 0.1 * torch.rand(FIN_C, generator=g)).float()
    return dict(x=x, partial=part, gamma=gamma, beta=beta, rm=rm, rv=rv, count=P, G=G, tpg=tpg)


def finalize_ref(c, momentum, eps, clamp=True):
    """float64 of the SAME float32 partials: mean, var (E[x^2] - mean^2, clamped at 0), invstd, scale, shift [G, C]; the running buffers
    after group 0, 1, ... in order with the unbiased variance (count > 1)"""
    G, tpg, n = c["G"], c["tpg"], float(c["count"])
    p = c["partial"][:, :FIN_C].double().reshape(2, FIN_C, G, tpg).sum(-1).permute(0, 2, 1)
    mean = p[0] / n
    var = p[1] / n - mean * mean
    if clamp:
        var = var.clamp(min=0)
    e, m = float(torch.tensor(eps, dtype=F32)), float(torch.tensor(momentum, dtype=F32))
    invstd = 1.0 / torch.sqrt(var + e)
    scale = c["gamma"].double() * invstd
    shift = c["beta"].double() - mean * scale
    rm, rv = c["rm"].double(), c["rv"].double()
    for k in range(G):
        rm = (1 - m) * rm + m * mean[k]
        rv = (1 - m) * rv + m * (var[k] * n / (n - 1) if n > 1 else var[k])
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, rm=rm, rv=rv)


# ---- LayerNorm(32) ----
LN_ROWS = [1, 7, 33, 1001, 49189]          # 49189 = 3 x 16384 + 37; 1001 rows end in a partly filled wavefront


def ln_special_rows(rows):
    """(constant row, rows with mean = 100 x std); none when there is a single row"""
    return ([3], [5, 6] if rows > 7 else [5]) if rows >= 7 else ([], [])


@functools.lru_cache(maxsize=4)
def ln_case(dtype, rows):
    g = gen(4, rows, dtype == BF16)
    x = torch.randn(rows, 32, generator=g).double() * 2 + 0.5
    const, offset = ln_special_rows(rows)
    for r in const:
        x[r] = 2.5
    for r in offset:
        x[r] = 100.0 + torch.randn(32, generator=g).double()
    x = rounded(x, dtype)
    dy = ints((rows, 32), g, rows)
    extra = rounded(torch.randn(rows, 32, generator=g).double(), dtype)
    gamma = (1 + 0.1 * torch.randn(32, generator=g)).float()
    beta = (0.1 * torch.randn(32, generator=g)).float()
    return dict(x=x, dy=dy, extra=extra, gamma=gamma, beta=beta, rows=rows, special=sorted(const + offset))


def ln_stats(x, eps):
    """float64 [rows, 2] = (mean, rstd), eps as its float32 value"""
    e = float(torch.tensor(eps, dtype=F32))
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + e)], 1)


def ln_fwd_ref(c, eps):
    st = ln_stats(c["x"], eps)
    return (c["x"] - st[:, :1]) * st[:, 1:] * c["gamma"].double() + c["beta"].double(), st


def ln_bwd_formula(x, dy, stats, gamma):
    xhat = (x - stats[:, :1]) * stats[:, 1:]
    gh = dy * gamma
    dx = stats[:, 1:] * (gh - (gh.sum(1, keepdim=True) + xhat * (gh * xhat).sum(1, keepdim=True)) / 32.0)
    return dx, (dy * xhat).sum(0), dy.sum(0)


def split_rows(rows, special):
    keep = torch.ones(rows, dtype=torch.bool)
    keep[special] = False
    return keep


# ---- reductions ----
RED_NT = [1, 7, 8, 9, 31, 32, 33, 257]
RED_N = [1, 31, 32, 33, 100]
COLSUM_C = [1, 3, 4, 8, 12, 24, 32, 48, 64, 129, 200, 256]
COLSUM_P = [1, 5, 255, 4097, 20001]


def reduce_case(nt, n):
    g = gen(5, nt, n)
    return ints((nt, n), g, nt + 1), ints((n,), g, 1)        # partial rows, `out` before


def colsum_case(dtype, C, P):
    g = gen(6, C, P, dtype == BF16)
    return ints((P, C), g, P + 1), ints((C,), g, 1)


# ---- shapes past one grid pass ----
HOIST_LARGE = [(F32, 64, 1, 65548), (BF16, 128, 1, 65548),      # (dtype, C, groups, npix): 1,048,768 pieces = one trip of the two-piece loop + the one-piece tail
               (F32, 64, 2, 131096)]                            # 1,048,768 pieces per group of 1024 workgroups: two trips + the tail
GENERIC_LARGE = [(F32, 48, 2, 87382), (BF16, 48, 1, 174763)]    # 1,048,584 / 1,048,578 pieces > 4096 x 256 threads: a second grid-stride pass
BWD_LARGE = (F32, 64, 2, 65548)                                 # 524,384 pieces per group of 1024 workgroups: one trip + the tail


def hoist_trips(dtype, C, groups, npix):
    """(full trips of `for (; i + stride < group_vec; i += 2 * stride)` made by thread 0 of workgroup 0, whether it then runs the tail)"""
    gvec = npix // groups * C // V[dtype]
    wg = min(max((gvec + HOIST_PIECES_PER_WG - 1) // HOIST_PIECES_PER_WG, 1), HOIST_WG // groups)
    stride, i, trips = wg * BLOCK, 0, 0
    while i + stride < gvec:
        i += 2 * stride
        trips += 1
    return trips, i < gvec


# ---- torch's own autograd, for tests/test_norm_edges_cpu.py ----
def bn_autograd(x, dy, gamma, dtype=torch.float64, eps=1e-5):
    """F.batch_norm (training) per group; x, dy [G, P, C] -> dx, dgamma, dbeta in `dtype`"""
    G, P, C = x.shape
    gm = gamma.to(dtype).clone().requires_grad_(True)
    bt = torch.zeros(C, dtype=dtype, requires_grad=True)
    xs = x.to(dtype).clone().requires_grad_(True)
    for k in range(G):
        y = F.batch_norm(xs[k].t().reshape(1, C, P), None, None, gm, bt, True, 0.1, eps)
        (y * dy[k].to(dtype).t().reshape(1, C, P)).sum().backward()
    return xs.grad, gm.grad, bt.grad


def ln_autograd(x, dy, gamma, beta, eps, dtype=torch.float64):
    xs = x.to(dtype).clone().requires_grad_(True)
    gm, bt = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    y = F.layer_norm(xs, (32,), gm, bt, eps)
    y.backward(dy.to(dtype))
    return y.detach(), xs.grad, gm.grad, bt.grad
