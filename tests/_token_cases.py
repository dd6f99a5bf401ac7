"""What tests/test_token_edges_gpu.py and tests/test_token_edges_cpu.py share: the seeded inputs of the token-side edge cases
(csrc/tokens.hip: tokenizer, cross-attention operand preparation, grouped softmax, self-attention core; csrc/encoder_fused.hip: the
fused token encoder), the float64 references written out in plain torch, the launch arithmetic the shapes are derived from, and the
checkers.

Every kernel gets ITS inputs from here, not from the kernel in front of it.  For the bf16 forms the inputs are generated
representable in bf16 (activations, the packed transposes, and the fp32 masters the matrix-core kernels round on the way in: master
and packed copy carry the same values), so the reference works on exactly what the kernel reads.  Gradients come from torch
autograd on the float64 forward; a backward kernel that reads a saved intermediate (the preparation's mn / mstats / k / v, the
attention probabilities, the softmax output) gets it formed in float64 and rounded to fp32 (to the activation type where the kernel
takes it in that type).

Buffers a kernel ADDS to are prefilled at the size of the gradient itself (0.5 x its maximum x a normal variate): the compared
quantity is prefill + gradient, and a prefill much larger than the gradient would hide the gradient's error in the bound."""
import functools
import math

import torch

from _bounds import close, tol

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [F32, BF16]
D = 32                                     # tokens.hip / encoder_fused.hip: constexpr int D = 32 (transformer width)
SCALE = 32 ** -0.5                         # ops.encoder_fwd / XattnPrep / self_attn default
EPS = 1e-5

# ---- the launch arithmetic the shapes below are derived from (the source line each mirrors) ----
TOK_ROWS_PER_CHUNK = 1024                  # tokens.hip tok_chunks(): c = HW / 1024, clamped to [1, 64]
TOK_MAX_CHUNKS = 64
TOK_LOGIT_BLOCK = 256                      # tokens.hip tok_logits_body: p = bx * 256 + threadIdx.x; tok_stats_body: n += 256
TOK_BWD_BLOCK = 64                         # tokens.hip tok_bwd_body: n = bx * 64 + (threadIdx.x >> 2), four lanes per pixel row
TOK_DWA_CHUNK = 1024                       # tokens.hip: constexpr int TOK_DWA_CHUNK = 1024; nblk = dh_cdiv(S * HW, TOK_DWA_CHUNK)
RED_PHASES = 8                             # common.h dh_reduce_partials_body: 8 row phases
TB_MAXJ = 4                                # tokens.hip: constexpr int TB_MAXJ = 4 (recorded tokenizer calls per launch)
XB_MAXJ = 4                                # tokens.hip: constexpr int XB_MAXJ = 4 (recorded preparation stacks per family)
ENC_MAXJ = 4                               # encoder_fused.hip: constexpr int ENC_MAXJ = 4 (recorded encoder stacks per launch)
ENC_MAXN = 8                               # encoder_fused.hip: constexpr int MAXN = 8
ENC_LDS_BYTES = 160 * 1024                 # encoder_fused.hip dh_encoder_supported: bwd <= 160 * 1024
PREP_PHASES = 8                            # tokens.hip xattn_prep_wgrad_body: for (s = ph; s < S; s += 8)
PREP_MFMA_IMAGES = 4                       # tokens.hip xattn_prep_mfma_body: s = bid.x * 4 + (pl >> 2)
PREP_WG_STEP = 8                           # tokens.hip xattn_prep_wgrad_mfma_body: for (s0 = 0; s0 < S; s0 += 8) -- 32 token rows


def cdiv(a, b):
    return -(-a // b)


def name(dtype):
    return "f32" if dtype == F32 else "bf16"


def tok_chunks(HW):
    """tokens.hip tok_chunks()"""
    return min(max(HW // TOK_ROWS_PER_CHUNK, 1), TOK_MAX_CHUNKS)


def tok_chunk_sizes(HW):
    """dh_tokenizer_fwd: chunk = dh_cdiv(HW, nch); tok_pool_partial_body: [bx * chunk, min(bx * chunk + chunk, HW))"""
    nch = tok_chunks(HW)
    chunk = cdiv(HW, nch)
    return [min(k * chunk + chunk, HW) - k * chunk for k in range(nch)]


def tok_nblk(S, HW):
    """dh_tokenizer_bwd: a.nblk = dh_cdiv(a.P, TOK_DWA_CHUNK)"""
    return cdiv(S * HW, TOK_DWA_CHUNK)


def hlp(heads, L):
    """ops.XattnPrep: HLP = cdiv(heads * L, 32) * 32"""
    return cdiv(heads * L, 32) * 32


def prep_mfma_supported(dtype, S, L, heads, dim_head):
    """tokens.hip dh_xattn_prep_mfma_supported (without its environment switch)"""
    H = hlp(heads, L)
    return dtype == BF16 and L == 4 and S % PREP_MFMA_IMAGES == 0 and dim_head in (32, 64) and heads >= 1 and heads * L <= H and H == 32


def prep_wgrad_mfma(S, dim_head):
    """dh_xattn_prep_bwd_stack_mfma: dim_head == 64 && S % 8 == 0 takes xattn_prep_wgrad_mfma_kernel + the ln_only launch, anything
    else the scalar xattn_prep_wgrad_kernel"""
    return dim_head == 64 and S % PREP_WG_STEP == 0


def enc_carve(n, heads, dim_head, mlp):
    """encoder_fused.hip carve() and enc_bwd_body: the float offset of every LDS buffer, forward buffers then gradient scratch"""
    inner = heads * dim_head
    sizes = [("x", n * D), ("xn", n * D), ("qkv", n * 3 * inner), ("p", heads * n * n), ("o", n * inner), ("x1", n * D), ("x1n", n * D),
             ("z", n * mlp), ("h", n * mlp), ("xh1", n * D), ("xh2", n * D), ("st", 4 * n), ("red", 8 * n * D),
             ("dx2", n * D), ("dz", n * mlp), ("dx1n", n * D), ("dx1", n * D), ("d_o", n * inner), ("dqkv", n * 3 * inner), ("dxn", n * D),
             ("dp", heads * n * n)]
    offs, o = {}, 0
    for k, s in sizes:
        offs[k] = o
        o += s
    offs["end"] = o
    return offs


def enc_saved_img_floats(n, heads, dim_head, mlp):
    """encoder_fused.hip saved_img_floats()"""
    inner = heads * dim_head
    return n * D * 6 + n * 3 * inner + heads * n * n + n * inner + 2 * n * mlp + 4 * n


def enc_supported(n, heads, dim_head, mlp):
    """encoder_fused.hip dh_encoder_supported()"""
    if n < 1 or n > ENC_MAXN or mlp > 64 or mlp < 1 or heads < 1 or dim_head % 16:
        return False
    if (heads * n * n) % 4 or (n * mlp) % 4:
        return False
    return enc_carve(n, heads, dim_head, mlp)["end"] * 4 <= ENC_LDS_BYTES and heads * n * 4 <= 256


# ---- the cases ----
TOK_HW = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3100]
TOK_FORMS = [(2, 1), (6, 3), (2, 2)]       # (S, B): two streams of one / three images; ONE stream of two images
TOK_L = [4, 8]
TOK_RECORDED = [(65, 2, 1), (2049, 6, 3), (256, 2, 2), (1, 6, 3), (3100, 2, 1)]       # (HW, S, B): five calls, the fifth flushes four

ENC_CASES = [(6, 8, 1, 8, 64, 64), (5, 8, 4, 8, 64, 64), (3, 8, 2, 4, 64, 32), (2, 8, 1, 1, 16, 17), (7, 6, 3, 4, 48, 32),
             (1, 4, 1, 1, 16, 5), (3, 2, 2, 2, 32, 6), (9, 1, 1, 4, 16, 4)]           # (B, n, depth, heads, dim_head, mlp)
ENC_BATCHED = [0, 2, 4, 6, 7]              # indices into ENC_CASES: five stacks in one EncoderBatch
ENC_REFUSED = [(1, 1, 16, 1), (3, 2, 48, 17), (3, 1, 16, 4)]                          # (n, heads, dim_head, mlp)
NET_SHAPES = [(8, h, 64, m) for h in (8, 4) for m in (64, 32)]

PREP_SCALAR = [(8, 64, 4, 8, 4, 1), (3, 8, 4, 3, 3, 1), (4, 32, 8, 6, 3, 2), (5, 16, 8, 9, 9, 3)]      # (heads, dim_head, L, S, B, layers)
PREP_MFMA = [(8, 64, 8, 4, 1), (8, 64, 4, 2, 2), (3, 64, 16, 8, 3), (2, 64, 24, 12, 1), (1, 32, 12, 6, 1), (8, 32, 8, 8, 2)]      # (heads, dim_head, S, B, layers), L = 4
PREP_RECORDED = [(8, 64, 8, 4, 1), (3, 64, 16, 8, 3), (2, 64, 24, 12, 2)]             # dim_head 64, S % 8 == 0: every family recorded

ATTN_CASES = [(2, 1, 1, 16), (3, 5, 3, 16), (2, 16, 8, 64)]                           # (B, n, heads, dim_head)
SOFTMAX_CASES = [(1, 8, 4, 32), (257, 3, 4, 32), (300, 5, 8, 64), (65, 2, 16, 32)]    # (rows, heads, L, HLP)

# bound factors (x tol(dtype) x max |want|)
F_FWD, F_DATA, F_PARAM, F_DWA = 1, 4, 4, 8


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (1 << 31)
    return torch.Generator().manual_seed(seed)


def rounded(x, dtype):
    """float64 values of `x` after rounding to `dtype`"""
    return x.to(dtype).double()


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def prefill(g, grad, dtype=F32):
    """what an accumulating kernel starts from: 0.5 x max |grad| x N(0, 1) in `dtype` (1 when the gradient is exactly zero)"""
    m = float(grad.abs().max())
    return rounded(randn(g, *grad.shape, scale=0.5 * (m if m > 0 else 1.0)), dtype)


# ---- checkers ----
def bounded(got, want, dtype, what, factor=1.0, scale=None):
    """_bounds.close: max |got - want| <= factor x tol(dtype) x max |want| (or `scale`), the figure printed first.  Returns the
    ratio max |got - want| / scale."""
    want = want.detach().double().cpu()
    g = got.detach().double().cpu()
    assert g.shape == want.shape, (what, tuple(g.shape), tuple(want.shape))
    assert bool(torch.isfinite(g).all()), "%s: non-finite" % what
    if want.numel() == 0:
        return 0.0
    err = (g - want).abs().reshape(-1)
    k = int(err.argmax())
    s = float(want.abs().max()) if scale is None else float(scale)
    ratio = float(err[k]) / max(s, 1e-6)
    print("%s: max err %.3e at %d, scale %.3e, ratio %.3e (bound %g x %g, %s)" % (what, float(err[k]), k, s, ratio, factor, tol(dtype), name(dtype)))
    close(g.reshape(-1)[k:k + 1], want.reshape(-1)[k:k + 1], dtype, what, scale=s, factor=factor)
    return ratio


def same_bits(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a, b), "%s: %d elements differ" % (what, int((a != b).sum()))


def check_all(got, want, spec, what, worst=None, shrink=1.0):
    """got, want: {key: tensor}; spec: {key: (dtype, factor) or (dtype, factor, scale)}.  Every key of spec is compared; `worst`
    ({key: ratio}) keeps the largest ratio seen.  shrink: every factor times this (the CPU test asks a quarter of each bound of the
    reference's own float32 evaluation)"""
    for k, sp in spec.items():
        r = bounded(got[k], want[k], sp[0], "%s %s" % (what, k), factor=sp[1] * shrink, scale=sp[2] if len(sp) > 2 else None)
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), r)


# ---- 1. tokenizer ----
@functools.lru_cache(maxsize=8)
def tok_case(dtype, L, HW, S, B):
    """x [S, HW, 32] in `dtype`, wa [L, 32], pos [2L, 32], dtok [B, 2L, 32] (zero in the rows of a stream that is absent: nothing
    was computed from them), tok0 the prefill of tok_cat; dx0 / dwa0 / dpos0 the prefills of the accumulating backward"""
    g = gen(11, L, HW, S, B, dtype == BF16)
    c = dict(dtype=dtype, L=L, HW=HW, S=S, B=B)
    c["x"] = rounded(randn(g, S, HW, D), dtype)
    c["wa"] = rounded(randn(g, L, D, scale=0.5), F32)
    c["pos"] = rounded(randn(g, 2 * L, D, scale=0.5), F32)
    c["dtok"] = rounded(randn(g, B, 2 * L, D), F32)
    c["tok0"] = rounded(randn(g, B, 2 * L, D), F32)
    if S == B:
        c["dtok"][:, L:] = 0
    r = tok_ref(c)
    c["dx0"] = prefill(g, r["dx"], dtype)
    c["dwa0"] = prefill(g, r["dwa"])
    c["dpos0"] = prefill(g, r["dpos"])
    c["ref"] = r
    return c


def tok_ref(c, dtype=F64, drop_chunk=None):
    """logits = x Wa^T, p = softmax over the HW pixels, tok = p^T x placed at [b, stream * L + l] + pos; gradients by autograd.
    drop_chunk: leave that chunk's pixels out of the pooled sum (a planted error for the checker test)"""
    L, S, B, HW = c["L"], c["S"], c["B"], c["HW"]
    x = c["x"].to(dtype).clone().requires_grad_(True)
    wa = c["wa"].to(dtype).clone().requires_grad_(True)
    pos = c["pos"].to(dtype).clone().requires_grad_(True)
    logits = x @ wa.t()                                        # [S, HW, L]
    p = torch.softmax(logits, 1)
    if drop_chunk is not None:
        sizes = tok_chunk_sizes(HW)
        keep = torch.ones(HW, dtype=dtype)
        keep[sum(sizes[:drop_chunk]):sum(sizes[:drop_chunk + 1])] = 0
        p = p * keep[None, :, None]
    tok = p.transpose(1, 2) @ x                                # [S, L, 32]
    cat = c["tok0"].to(dtype).clone()
    parts = [tok[st * B:(st + 1) * B] + pos[st * L:(st + 1) * L] for st in range(S // B)]
    cat = torch.cat(parts + [cat[:, len(parts) * L:]], 1)
    (cat * c["dtok"].to(dtype)).sum().backward()
    mx = logits.detach().max(1).values                         # what the forward saves: logits, (max, 1 / sum exp) per (image, token),
    inv = 1.0 / torch.exp(logits.detach() - mx[:, None]).sum(1)     # and the pooled tokens before pos
    return dict(tok=cat.detach(), logits=logits.detach(), stats=torch.stack([mx, inv], -1), pooled=tok.detach(), dx=x.grad, dwa=wa.grad,
                dpos=pos.grad)


def tok_cancel_scale(c):
    """HW = 1: p = 1, so dWa and the logit part of dx are zero by cancellation of terms of this size"""
    return float(c["dtok"].abs().max()) * float(c["x"].abs().max()) ** 2


def tok_spec(c, accumulate):
    """{key: (dtype, factor[, scale])} of the tokenizer's outputs.  Only dx is stored in the activation type: the tokens, dWa and dpos
    are fp32 results of fp32 arithmetic on inputs that are exact in either form, so they keep the fp32 bound in the bf16 form too"""
    spec = dict(tok=(F32, F_FWD), dx=(c["dtype"], F_DATA), dwa=(F32, F_DWA), dpos=(F32, F_PARAM))
    if c["HW"] == 1:
        s = tok_cancel_scale(c)
        spec["dwa"] = (F32, F_DWA, max(s, float(tok_want(c, accumulate)["dwa"].abs().max())))
    return spec


def tok_want(c, accumulate):
    r = c["ref"]
    return dict(tok=r["tok"], dx=c["dx0"] + r["dx"], dwa=r["dwa"] + (c["dwa0"] if accumulate else 0), dpos=r["dpos"] + (c["dpos0"] if accumulate else 0))


# ---- 2. fused token encoder ----
ENC_NAMES = ("ln1_g", "ln1_b", "wqkv", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2")


def enc_shapes(heads, dim_head, mlp):
    inner = heads * dim_head
    return [(D,), (D,), (3 * inner, D), (D, inner), (D,), (D,), (D,), (mlp, D), (mlp,), (D, mlp), (D,)]


def enc_layout(heads, dim_head, mlp):
    """offsets of the 11 parameters of one layer, each at a multiple of 4 floats, and the layer pitch (a multiple of 4, + 8 floats
    nothing uses): the kernels read weights with 16-byte loads"""
    offs, o = [], 0
    for sh in enc_shapes(heads, dim_head, mlp):
        offs.append(o)
        o += cdiv(math.prod(sh), 4) * 4
    return offs, o + 8


def enc_views(flat, depth, heads, dim_head, mlp):
    """[layer][parameter] views into a flat arena"""
    offs, stride = enc_layout(heads, dim_head, mlp)
    return [[flat[l * stride + o:l * stride + o + math.prod(sh)].view(sh) for o, sh in zip(offs, enc_shapes(heads, dim_head, mlp))]
            for l in range(depth)]


@functools.lru_cache(maxsize=16)
def enc_case(B, n, depth, heads, dim_head, mlp):
    g = gen(21, B, n, depth, heads, dim_head, mlp)
    _, stride = enc_layout(heads, dim_head, mlp)
    arena = rounded(randn(g, depth * stride, scale=0.2), F32)
    for layer in enc_views(arena, depth, heads, dim_head, mlp):
        layer[0] += 1.0
        layer[5] += 1.0
    arena = rounded(arena, F32)
    c = dict(B=B, n=n, depth=depth, heads=heads, dim_head=dim_head, mlp=mlp, stride=stride, arena=arena,
             x=rounded(randn(g, B * n, D), F32), dy=rounded(randn(g, B * n, D), F32))
    r = enc_ref(c)
    c["garena0"] = rounded(randn(g, depth * stride), F32)
    for gl, rl in zip(enc_views(c["garena0"], depth, heads, dim_head, mlp), r["grads"]):
        for gv, rv in zip(gl, rl):
            gv.copy_(prefill(g, rv))
    c["ref"] = r
    return c


def layer_norm(x, gamma, beta, eps=EPS):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def gelu_erf(z):
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))


def enc_forward(x, layers, B, n, heads, dim_head, scale=SCALE, eps=EPS):
    """x [B n, 32]: x1 = x + Wo attn(LN1(x)) + bo; y = x1 + W2 gelu(W1 LN2(x1) + b1) + b2, layer after layer"""
    x = x.view(B, n, D)
    for g1, b1_, wqkv, wo, bo, g2, b2_, w1, fb1, w2, fb2 in layers:
        xn = layer_norm(x, g1, b1_, eps)
        q, k, v = (xn @ wqkv.t()).view(B, n, 3, heads, dim_head).permute(2, 0, 3, 1, 4)      # each [B, heads, n, dim_head]
        a = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
        o = (a @ v).permute(0, 2, 1, 3).reshape(B, n, heads * dim_head)
        x1 = x + o @ wo.t() + bo
        x = x1 + gelu_erf(layer_norm(x1, g2, b2_, eps) @ w1.t() + fb1) @ w2.t() + fb2
    return x.reshape(B * n, D)


def enc_ref(c, dtype=F64):
    arena = c["arena"].to(dtype).clone().requires_grad_(True)
    x = c["x"].to(dtype).clone().requires_grad_(True)
    y = enc_forward(x, enc_views(arena, c["depth"], c["heads"], c["dim_head"], c["mlp"]), c["B"], c["n"], c["heads"], c["dim_head"])
    y.backward(c["dy"].to(dtype))
    return dict(y=y.detach(), dx=x.grad, grads=enc_views(arena.grad, c["depth"], c["heads"], c["dim_head"], c["mlp"]))


def enc_total(c, r, dtype=F64):
    """the gradient arena after an exact accumulating backward: prefill + the gradients of `r`, formed in `dtype`"""
    garena = c["garena0"].to(dtype).clone()
    for gv, rv in zip(enc_views(garena, c["depth"], c["heads"], c["dim_head"], c["mlp"]), r["grads"]):
        for a, b in zip(gv, rv):
            a.add_(b.to(dtype))
    return garena


def enc_gaps(c):
    """the floats of the arena that belong to no parameter"""
    m = torch.ones(c["depth"] * c["stride"], dtype=torch.bool)
    for layer in enc_views(m, c["depth"], c["heads"], c["dim_head"], c["mlp"]):
        for v in layer:
            v.fill_(False)
    return m


def enc_check(c, y, dx, garena, what, worst=None, ref=None, dtype=F32, shrink=1.0):
    """y, dx and the 11 gradient tensors of every layer (prefill + gradient) against the reference; the arena's gaps untouched"""
    gaps = enc_gaps(c)
    assert torch.equal(garena.detach().double().cpu()[gaps], c["garena0"][gaps]), "%s: wrote between the gradient tensors" % what
    r = c["ref"] if ref is None else ref
    got, want, spec = dict(y=y, dx=dx), dict(y=r["y"], dx=r["dx"]), dict(y=(dtype, F_FWD), dx=(dtype, F_FWD))
    gv = enc_views(garena, c["depth"], c["heads"], c["dim_head"], c["mlp"])
    g0 = enc_views(c["garena0"], c["depth"], c["heads"], c["dim_head"], c["mlp"])
    for l in range(c["depth"]):
        for i, nm in enumerate(ENC_NAMES):
            k = "d%s[%d]" % (nm, l)
            got[k], want[k], spec[k] = gv[l][i], g0[l][i] + r["grads"][l][i], (dtype, F_PARAM)
    check_all(got, want, spec, what, worst, shrink)


# ---- 3. cross-attention operand preparation ----
PREP_NAMES = ("wq", "wk", "wv", "wo", "g", "b")


def prep_layout(heads, dim_head):
    """one layer of the arena: wq, wk, wv [inner, 32], wo [32, inner], ln g, b [32]; layer pitch + 8 floats nothing uses"""
    inner = heads * dim_head
    shp = dict(wq=(inner, D), wk=(inner, D), wv=(inner, D), wo=(D, inner), g=(D,), b=(D,))
    offs = dict(wq=0, wk=inner * D, wv=2 * inner * D, wo=3 * inner * D, g=4 * inner * D, b=4 * inner * D + D)
    return shp, offs, 4 * inner * D + 2 * D + 8


def prep_view(flat, layer, nm, heads, dim_head):
    shp, offs, stride = prep_layout(heads, dim_head)
    o = layer * stride + offs[nm]
    return flat[o:o + math.prod(shp[nm])].view(shp[nm])


def prep_tok_base(c):
    """float offset of image s's token rows: (s % B) bstride + (s // B) sstride"""
    s = torch.arange(c["S"])
    return (s % c["B"]) * c["bstride"] + (s // c["B"]) * c["sstride"]


def prep_rows(tok_flat, c):
    idx = prep_tok_base(c)[:, None] + torch.arange(c["L"] * D)[None]
    return tok_flat[idx].view(c["S"], c["L"], D)


def ste_round(x, dtype):
    """x rounded to `dtype`, the identity for autograd"""
    return x + (x.detach().to(dtype).to(x.dtype) - x.detach())


@functools.lru_cache(maxsize=8)
def prep_case(dtype, heads, dim_head, L, S, B, layers, mfma=False):
    """tokens fp32 ([B, 2L, 32] for two streams, [B, L, 32] with sstride = 0 for one), the parameter arena (weights representable in
    bf16 for the bf16 form), dkq [layers, S, HLP, 32] / dvoT [layers, S, 32, HLP] with zeros in the padding, and the prefills"""
    g = gen(31, heads, dim_head, L, S, B, layers, dtype == BF16, mfma)
    streams = S // B
    shp, offs, stride = prep_layout(heads, dim_head)
    H = hlp(heads, L)
    c = dict(dtype=dtype, heads=heads, dim_head=dim_head, L=L, S=S, B=B, layers=layers, mfma=mfma, HLP=H, stride=stride,
             bstride=streams * L * D, sstride=L * D if streams == 2 else 0)
    c["tok"] = rounded(randn(g, B * streams * L * D), F32)
    arena = randn(g, layers * stride, scale=0.2)
    for l in range(layers):
        prep_view(arena, l, "g", heads, dim_head).add_(1.0)
    arena = rounded(arena, F32)
    if dtype == BF16:
        for l in range(layers):
            for nm in ("wq", "wk", "wv", "wo"):
                v = prep_view(arena, l, nm, heads, dim_head)
                v.copy_(rounded(v, BF16))
    c["arena"] = arena
    dkq = rounded(randn(g, layers, S, H, D), F32)
    dvoT = rounded(randn(g, layers, S, D, H), F32)
    dkq[:, :, heads * L:] = 0
    dvoT[:, :, :, heads * L:] = 0
    c["dkq"], c["dvoT"] = dkq, dvoT
    r = prep_ref(c)
    c["dtok0"] = prefill(g, r["dtok"])
    c["garena0"] = rounded(randn(g, layers * stride), F32)
    for l in range(layers):
        for nm in PREP_NAMES:
            prep_view(c["garena0"], l, nm, heads, dim_head).copy_(prefill(g, prep_view(r["garena"], l, nm, heads, dim_head)))
    c["ref"] = r
    return c


def prep_forward(rows, p, c, dtype):
    """one layer on the gathered token rows [S, L, 32]: mn, mstats, k, v, kq, vo (the last two padded to HLP rows).
    Matrix-core form: LN(tokens), k and v enter the products rounded to bf16 (tokens.hip: bmn = ppack8(mnv), kB / vB = ppack8(kb / vb))"""
    heads, dh, L, S = c["heads"], c["dim_head"], c["L"], c["S"]
    mean = rows.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((rows - mean) ** 2).mean(-1, keepdim=True) + EPS)
    mn = (rows - mean) * rstd * p["g"] + p["b"]
    m = ste_round(mn, BF16) if c["mfma"] else mn
    k, v = m @ p["wk"].t(), m @ p["wv"].t()
    kk, vv = (ste_round(k, BF16), ste_round(v, BF16)) if c["mfma"] else (k, v)
    kq = SCALE * torch.einsum("slhd,hdc->shlc", kk.view(S, L, heads, dh), p["wq"].view(heads, dh, D)).reshape(S, heads * L, D)
    vo = torch.einsum("slhd,chd->shlc", vv.view(S, L, heads, dh), p["wo"].view(D, heads, dh)).reshape(S, heads * L, D)
    pad = torch.zeros(S, c["HLP"] - heads * L, D, dtype=dtype)
    return dict(mn=mn, mstats=torch.cat([mean, rstd], -1), k=k, v=v, kq=torch.cat([kq, pad], 1), vo=torch.cat([vo, pad], 1))


def prep_ref(c, dtype=F64):
    """forward of every layer and, by autograd on sum(kq dkq) + sum(vo^T dvoT): the token gradient summed over the layers (also
    layer by layer and image by image, for the planted errors) and the parameter gradients in the arena's layout"""
    heads, dh, layers = c["heads"], c["dim_head"], c["layers"]
    tok = c["tok"].to(dtype).clone().requires_grad_(True)
    arena = c["arena"].to(dtype).clone().requires_grad_(True)
    fwd, dtok_layers, dimg_layers = [], [], []
    for l in range(layers):
        rows = prep_rows(tok, c)
        rows.retain_grad()
        f = prep_forward(rows, {nm: prep_view(arena, l, nm, heads, dh) for nm in PREP_NAMES}, c, dtype)
        before = tok.grad.clone() if tok.grad is not None else torch.zeros_like(tok)
        ((f["kq"] * c["dkq"][l].to(dtype)).sum() + (f["vo"].transpose(1, 2) * c["dvoT"][l].to(dtype)).sum()).backward()
        dtok_layers.append(tok.grad - before)
        dimg_layers.append(rows.grad.clone())
        fwd.append({k: v.detach() for k, v in f.items()})
    out = {k: torch.stack([f[k] for f in fwd]) for k in fwd[0]}
    out.update(dtok=tok.grad.clone(), dtok_layers=dtok_layers, dimg_layers=dimg_layers, garena=arena.grad.clone())
    return out


def prep_scatter(dimg, c, shift_image=None):
    """per-image token gradients [S, L, 32] -> the flat token buffer.  shift_image: that image's rows land one stream further (a
    planted error)"""
    base = prep_tok_base(c).clone()
    if shift_image is not None:
        base[shift_image] = (base[shift_image] + c["L"] * D) % c["tok"].numel()
    out = torch.zeros_like(c["tok"])
    idx = base[:, None] + torch.arange(c["L"] * D)[None]
    out.index_put_((idx.reshape(-1),), dimg.reshape(-1), accumulate=True)
    return out


def prep_fwd_dtypes(c):
    """(dtype of the fp32 outputs mn / mstats, of k / v, of kq / vo) for the bound: the LayerNorm is fp32 in every form; k and v are
    fp32 sums of exact products in the scalar forms (the weights are representable) and carry the bf16 rounding of LN(tokens) in the
    matrix-core form (a value next to a rounding tie may round the other way than the reference's); kq / vo are stored in `dtype`"""
    return F32, (BF16 if c["mfma"] else F32), c["dtype"]


def prep_check_fwd(c, got, what, worst=None, ref=None, shrink=1.0):
    """got: {mn, mstats, k, v, kq, kqT, vo, voT} stacked over the layers.  kqT / voT: bit-for-bit the transposes; rows >= heads L: zero"""
    r = c["ref"] if ref is None else ref
    t_ln, t_kv, t_out = prep_fwd_dtypes(c)
    spec = dict(mn=(t_ln, F_FWD), mstats=(t_ln, F_FWD), k=(t_kv, F_FWD), v=(t_kv, F_FWD), kq=(t_out, F_FWD), vo=(t_out, F_FWD))
    check_all(got, r, spec, what, worst, shrink)
    HL = c["heads"] * c["L"]
    for a, b in (("kq", "kqT"), ("vo", "voT")):
        same_bits(got[b], got[a].transpose(-1, -2).contiguous(), "%s %s is the transpose of %s" % (what, b, a))
        if HL < c["HLP"]:
            assert float(got[a][..., HL:, :].double().abs().max()) == 0.0, "%s %s: padding rows not zero" % (what, a)


def prep_bwd_dtype(c):
    """every operand and result of the scalar backward is fp32 (the packed wqT is representable); the matrix-core form rounds dkq /
    dvoT, dk / dv and the weight-gradient operands to bf16"""
    return BF16 if c["mfma"] else F32


def prep_bwd_want(c, accumulate=True, ref=None):
    r = c["ref"] if ref is None else ref
    heads, dh = c["heads"], c["dim_head"]
    want = dict(dtok=c["dtok0"] + r["dtok"])
    for l in range(c["layers"]):
        for nm in PREP_NAMES:
            add = accumulate or nm in ("g", "b")          # dln_g / dln_b are added unconditionally
            g0 = prep_view(c["garena0"], l, nm, heads, dh)
            want["d%s[%d]" % (nm, l)] = prep_view(r["garena"], l, nm, heads, dh) + (g0 if add else 0)
    return want


def prep_bwd_got(c, dtok, garena):
    got = dict(dtok=dtok.reshape(-1))
    for l in range(c["layers"]):
        for nm in PREP_NAMES:
            got["d%s[%d]" % (nm, l)] = prep_view(garena, l, nm, c["heads"], c["dim_head"])
    return got


def prep_check_bwd(c, got, what, accumulate=True, worst=None, ref=None, shrink=1.0):
    want = prep_bwd_want(c, accumulate, ref)
    t = prep_bwd_dtype(c)
    spec = {k: (t, F_DATA if k == "dtok" else F_PARAM) for k in want}
    check_all(got, want, spec, what, worst, shrink)


# ---- 4. layer-wise fallbacks ----
@functools.lru_cache(maxsize=4)
def attn_case(dtype, B, n, heads, dim_head):
    g = gen(41, B, n, heads, dim_head, dtype == BF16)
    c = dict(dtype=dtype, B=B, n=n, heads=heads, dim_head=dim_head, qkv=rounded(randn(g, B * n, 3 * heads * dim_head), dtype),
             dout=rounded(randn(g, B * n, heads * dim_head), dtype))
    c["ref"] = attn_ref(c)
    return c


def attn_ref(c, dtype=F64):
    B, n, heads, dh = c["B"], c["n"], c["heads"], c["dim_head"]
    qkv = c["qkv"].to(dtype).clone().requires_grad_(True)
    q, k, v = qkv.view(B, n, 3, heads, dh).permute(2, 0, 3, 1, 4)
    a = torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1)
    o = (a @ v).permute(0, 2, 1, 3).reshape(B * n, heads * dh)
    o.backward(c["dout"].to(dtype))
    return dict(o=o.detach(), attn=a.detach(), dqkv=qkv.grad)


@functools.lru_cache(maxsize=4)
def softmax_case(dtype, rows, heads, L, HLP):
    """x, dy [rows, HLP] (the padding columns hold values too: the kernels must not read them into the result); y for the backward
    is the float64 softmax rounded to `dtype`, and the reference gradient is the softmax backward AT that y"""
    g = gen(42, rows, heads, L, HLP, dtype == BF16)
    x, dy = rounded(randn(g, rows, HLP, scale=2.0), dtype), rounded(randn(g, rows, HLP), dtype)
    HL = heads * L
    y = torch.zeros(rows, HLP, dtype=F64)
    y[:, :HL] = torch.softmax(x[:, :HL].view(rows, heads, L), -1).reshape(rows, HL)
    ys = rounded(y, dtype)
    p, gy = ys[:, :HL].view(rows, heads, L), dy[:, :HL].view(rows, heads, L)
    dx = torch.zeros(rows, HLP, dtype=F64)
    dx[:, :HL] = (p * (gy - (p * gy).sum(-1, keepdim=True))).reshape(rows, HL)
    return dict(dtype=dtype, rows=rows, heads=heads, L=L, HLP=HLP, x=x, dy=dy, y=y, y_saved=ys, dx=dx)


def softmax_autograd(c, dtype=F64):
    """torch's own softmax and autograd on the same x / dy (no saved y): what the written-out backward is checked against"""
    HL = c["heads"] * c["L"]
    x = c["x"].to(dtype).clone().requires_grad_(True)
    y = torch.softmax(x[:, :HL].view(c["rows"], c["heads"], c["L"]), -1).reshape(c["rows"], HL)
    y.backward(c["dy"][:, :HL].to(dtype))
    return y.detach(), x.grad
