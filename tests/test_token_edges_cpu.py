"""CPU side of tests/test_token_edges_gpu.py: its cases reach the launch forms they name (mirrors of the launch arithmetic of
csrc/tokens.hip and csrc/encoder_fused.hip), its written-out float64 references agree with an independent formulation (torch.nn
modules for the encoder, the un-reassociated cross attention for the preparation, torch's own autograd for the grouped softmax), every
bound is met fourfold by the same reference evaluated in float32 (bf16: by the reference rounded to bf16), the checkers turn red on
planted errors, and dh_encoder_supported refuses the shapes whose LDS buffers would not be 16-byte aligned."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _token_cases as T
from _token_cases import F32, BF16, F64, D


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


# ---- the cases reach the forms they name ----
def test_tokenizer_pixel_counts_reach_the_chunk_and_block_forms():
    assert T.tok_chunk_sizes(2047) == [2047] and T.tok_chunk_sizes(2048) == [1024, 1024] and T.tok_chunk_sizes(2049) == [1025, 1024]
    assert T.tok_chunk_sizes(3100) == [1034, 1034, 1032]
    assert all(T.tok_chunks(hw) == 1 for hw in T.TOK_HW if hw < 2048)
    for block in (T.TOK_BWD_BLOCK, T.TOK_LOGIT_BLOCK):
        assert {block - 1, block, block + 1} <= set(T.TOK_HW)
    assert 1 in T.TOK_HW
    # dead quad lanes: a partly filled 64-pixel block
    assert any(hw % T.TOK_BWD_BLOCK for hw in T.TOK_HW) and any(hw % T.TOK_BWD_BLOCK == 0 for hw in T.TOK_HW)
    # the weighted column sum walks 64 phases: chunks shorter than, equal to and not a multiple of them
    assert any(s < 64 for hw in T.TOK_HW for s in T.tok_chunk_sizes(hw)) and any(s % 64 for s in T.tok_chunk_sizes(3100))
    nblk = {T.tok_nblk(S, hw) for S, B in T.TOK_FORMS for hw in T.TOK_HW}
    assert 1 in nblk and 2 in nblk and any(2 < k <= T.RED_PHASES for k in nblk) and any(k > T.RED_PHASES for k in nblk), sorted(nblk)
    assert T.tok_nblk(6, 3100) == 19 and T.tok_nblk(6, 255) == 2 and T.tok_nblk(2, 257) == 1
    assert {(S // B) for S, B in T.TOK_FORMS} == {1, 2} and {B for S, B in T.TOK_FORMS if S == 2 * B} == {1, 3}
    assert len(T.TOK_RECORDED) == T.TB_MAXJ + 1 and len({hw for hw, _, _ in T.TOK_RECORDED}) == 5
    assert {B for _, _, B in T.TOK_RECORDED} == {1, 2, 3}
    assert max(S * hw * D for S, B in T.TOK_FORMS for hw in T.TOK_HW) == 6 * 3100 * 32


def test_encoder_cases_reach_the_forms_they_name():
    for B, n, depth, heads, dh, mlp in T.ENC_CASES:
        assert T.enc_supported(n, heads, dh, mlp), (n, heads, dh, mlp)
        offs, stride = T.enc_layout(heads, dh, mlp)
        assert all(o % 4 == 0 for o in offs) and stride % 4 == 0
    B, n, depth, heads, dh, mlp = T.ENC_CASES[0]
    assert heads * n * 4 == 256 and (T.enc_carve(n, heads, dh, mlp)["red"] + 8 * n * D) * 4 > 64 * 1024      # forward LDS above 64 KB
    assert T.ENC_CASES[1][2] == 4 and T.ENC_CASES[1][0] * T.ENC_CASES[1][1] == 40
    B, n, depth, heads, dh, mlp = T.ENC_CASES[3]
    inner = heads * dh
    assert inner == 16 and mlp % 2 == 1
    total = 3 * inner * D + D * inner + 2 * mlp * D + D + mlp + D + 4 * D      # dh_encoder_bwd: the weight-gradient launch's outputs
    assert total % 64 != 0
    assert {c[1] for c in T.ENC_CASES} == {8, 6, 4, 2, 1} and T.ENC_CASES[4][4] // 4 == 12
    assert T.ENC_CASES[5][0] == 1 and T.ENC_CASES[5][0] * T.ENC_CASES[5][1] == 4
    assert sum(c[2] > 1 for c in T.ENC_CASES) >= 3 and sum(c[1] < T.ENC_MAXN for c in T.ENC_CASES) >= 4
    assert len(T.ENC_BATCHED) == T.ENC_MAXJ + 1
    assert any(T.ENC_CASES[i][1] < 8 for i in T.ENC_BATCHED) and any(T.ENC_CASES[i][2] > 1 for i in T.ENC_BATCHED)
    # n = 1: the probabilities are 1, the q and k blocks of dWqkv exactly zero, the v block is not
    c = T.enc_case(*T.ENC_CASES[7])
    g = c["ref"]["grads"][0][2]
    inner = c["heads"] * c["dim_head"]
    assert float(g[:2 * inner].abs().max()) == 0.0 and float(g[2 * inner:].abs().max()) > 0


def test_preparation_cases_reach_the_forms_they_name():
    for dtype in T.DTYPES:
        for heads, dh, L, S, B, layers in T.PREP_SCALAR:
            assert S in (B, 2 * B) and dh % 8 == 0
    heads, dh, L, S, B, layers = T.PREP_SCALAR[0]
    assert T.hlp(heads, L) == heads * L == 32 and S == 2 * B and layers == 1
    heads, dh, L, S, B, layers = T.PREP_SCALAR[1]
    assert S == B and S < T.PREP_PHASES and heads * L == 12 and T.hlp(heads, L) == 32 and T.prep_case(F32, *T.PREP_SCALAR[1])["sstride"] == 0
    heads, dh, L, S, B, layers = T.PREP_SCALAR[2]
    assert L == 8 and layers > 1 and T.prep_layout(heads, dh)[2] > 4 * heads * dh * D + 2 * D
    heads, dh, L, S, B, layers = T.PREP_SCALAR[3]
    assert T.hlp(heads, L) == 64 and heads * L == 40 and S > T.PREP_PHASES and layers == 3
    # the matrix-core cases are exactly those the predicate accepts
    for heads, dh, S, B, layers in T.PREP_MFMA + T.PREP_RECORDED:
        assert T.prep_mfma_supported(BF16, S, 4, heads, dh) and S in (B, 2 * B)
    for heads, dh, L, S, B, layers in T.PREP_SCALAR:
        assert not T.prep_mfma_supported(BF16, S, L, heads, dh) or (heads, dh, S, B, layers) in T.PREP_MFMA
        assert not T.prep_mfma_supported(F32, S, L, heads, dh)
    assert not T.prep_mfma_supported(BF16, 6, 4, 8, 64) and not T.prep_mfma_supported(BF16, 8, 8, 4, 64) and not T.prep_mfma_supported(BF16, 8, 4, 8, 16)
    forms = [(T.prep_wgrad_mfma(S, dh), dh, cdiv8(S), layers, heads % 4) for heads, dh, S, B, layers in T.PREP_MFMA]
    assert forms[0] == (True, 64, 1, 1, 0)                         # matrix-core weight gradient, one 32-row step
    assert forms[1][:2] == (False, 64) and forms[1][3] > 1         # matrix-core operand gradient, scalar weight gradient, layer reduce
    assert forms[2][0] and forms[2][2] == 2 and forms[2][4] != 0   # two steps (the prefetch), heads not a multiple of the four waves
    assert forms[3][0] and forms[3][2] == 3                        # three steps
    assert forms[4][:2] == (False, 32) and forms[5][:2] == (False, 32)
    assert T.PREP_MFMA[5][2] == T.PREP_MFMA[5][3]                  # S = B: one stream
    assert len(T.PREP_RECORDED) <= T.XB_MAXJ and all(dh == 64 and T.prep_wgrad_mfma(S, dh) for _, dh, S, _, _ in T.PREP_RECORDED)
    assert len({(h, S, ly) for h, _, S, _, ly in T.PREP_RECORDED}) == 3


def cdiv8(S):
    return T.cdiv(S, T.PREP_WG_STEP)


def test_fallback_cases_reach_the_forms_they_name():
    assert (2, 1, 1, 16) in T.ATTN_CASES and any(n * n == 256 for _, n, _, _ in T.ATTN_CASES) and any(n % 2 and h % 2 for _, n, h, _ in T.ATTN_CASES)
    for rows, heads, L, H in T.SOFTMAX_CASES:
        assert heads * L <= H and H % L == 0
    assert T.SOFTMAX_CASES[0][0] == 1 and (257 * (32 // 4)) % 256 != 0
    assert any(heads * L < H for _, heads, L, H in T.SOFTMAX_CASES) and {L for _, _, L, _ in T.SOFTMAX_CASES} == {4, 8, 16}


# ---- the predicate fix ----
def test_encoder_predicate_refuses_shapes_that_would_misalign_the_lds_buffers():
    from dahitra_amd import _lib
    L = _lib.lib()
    for shape in T.ENC_REFUSED:
        assert L.dh_encoder_supported(*shape) == 0 and not T.enc_supported(*shape), shape
    n, heads, dh, mlp = T.ENC_REFUSED[0]
    assert T.enc_saved_img_floats(n, heads, dh, mlp) == 263
    for B, n, depth, heads, dh, mlp in T.ENC_CASES:
        assert L.dh_encoder_supported(n, heads, dh, mlp) == 1
    for shape in T.NET_SHAPES:
        assert L.dh_encoder_supported(*shape) == 1
    assert L.dh_encoder_supported(16, 8, 64, 64) == 0
    accepted = 0
    for n in range(1, 10):
        for heads in (1, 2, 3, 4, 8):
            for dh in (16, 24, 32, 48, 64):
                for mlp in (1, 2, 3, 4, 5, 6, 17, 32, 64, 65):
                    ok = L.dh_encoder_supported(n, heads, dh, mlp)
                    assert bool(ok) == T.enc_supported(n, heads, dh, mlp), (n, heads, dh, mlp)
                    if ok:
                        accepted += 1
                        offs = T.enc_carve(n, heads, dh, mlp)
                        assert all(o % 4 == 0 for o in offs.values()), (n, heads, dh, mlp, offs)
                        assert T.enc_saved_img_floats(n, heads, dh, mlp) % 4 == 0
                        assert T.enc_saved_img_floats(n, heads, dh, mlp) == offs["red"]
                        assert _lib.lib().dh_encoder_saved_floats(3, n, 2, heads, dh, mlp) == 6 * offs["red"]
    assert accepted > 100


def test_matrix_core_predicate_mirror_equals_the_library():
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    for dtype in T.DTYPES:
        for S in (1, 3, 4, 6, 8, 9, 12, 24):
            for tl in (4, 8):
                for heads in (1, 2, 3, 5, 8, 9):
                    for dh in (8, 16, 32, 64):
                        got = L.dh_xattn_prep_mfma_supported(ops._DT[dtype], S, tl, heads, dh, T.hlp(heads, tl))
                        assert bool(got) == T.prep_mfma_supported(dtype, S, tl, heads, dh), (dtype, S, tl, heads, dh)
    for dtype in T.DTYPES:
        for heads, dh, tl, S, B, layers in T.PREP_SCALAR:
            for mfma in ((False, True) if T.prep_mfma_supported(dtype, S, tl, heads, dh) else (False,)):
                assert T.prep_case(dtype, heads, dh, tl, S, B, layers, mfma)["HLP"] == ops.cdiv(heads * tl, 32) * 32


# ---- references against an independent formulation ----
class Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x) + x


class PreNorm(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.norm, self.fn = nn.LayerNorm(D), fn

    def forward(self, x):
        return self.fn(self.norm(x))


class Attention(nn.Module):
    def __init__(self, heads, dim_head):
        super().__init__()
        self.heads, self.to_qkv, self.to_out = heads, nn.Linear(D, 3 * heads * dim_head, bias=False), nn.Linear(heads * dim_head, D)

    def forward(self, x):
        b, n, _ = x.shape
        q, k, v = (t.reshape(b, n, self.heads, -1).transpose(1, 2) for t in self.to_qkv(x).chunk(3, dim=-1))
        attn = F.softmax(torch.einsum("bhid,bhjd->bhij", q, k) * T.SCALE, dim=-1)
        return self.to_out(torch.einsum("bhij,bhjd->bhid", attn, v).transpose(1, 2).reshape(b, n, -1))


def feed_forward(mlp):
    return nn.Sequential(nn.Linear(D, mlp), nn.GELU(), nn.Linear(mlp, D))


@pytest.mark.parametrize("case", T.ENC_CASES, ids=lambda c: "-".join(map(str, c)))
def test_encoder_reference_equals_torch_nn_modules(case):
    c = T.enc_case(*case)
    B, n, depth, heads, dh, mlp = case
    layers = nn.ModuleList([nn.ModuleList([Residual(PreNorm(Attention(heads, dh))), Residual(PreNorm(feed_forward(mlp)))]) for _ in range(depth)]).double()
    order = lambda a, f: [a.fn.norm.weight, a.fn.norm.bias, a.fn.fn.to_qkv.weight, a.fn.fn.to_out.weight, a.fn.fn.to_out.bias,
                          f.fn.norm.weight, f.fn.norm.bias, f.fn.fn[0].weight, f.fn.fn[0].bias, f.fn.fn[2].weight, f.fn.fn[2].bias]
    with torch.no_grad():
        for (a, f), src in zip(layers, T.enc_views(c["arena"], depth, heads, dh, mlp)):
            for p, s in zip(order(a, f), src):
                p.copy_(s)
    x = c["x"].clone().view(B, n, D).requires_grad_(True)
    y = x
    for a, f in layers:
        y = f(a(y))
    y.backward(c["dy"].view(B, n, D))
    r = c["ref"]
    assert rel(y.reshape(B * n, D), r["y"]) < 1e-12 and rel(x.grad.reshape(B * n, D), r["dx"]) < 1e-12
    for (a, f), want in zip(layers, r["grads"]):
        for p, w, nm in zip(order(a, f), want, T.ENC_NAMES):
            assert float((p.grad - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1e-30) + 1e-300, nm


@pytest.mark.parametrize("case", T.PREP_SCALAR, ids=lambda c: "-".join(map(str, c)))
def test_preparation_reference_reproduces_the_dense_cross_attention(case):
    """q = to_q(LN(x)), k / v = to_k / to_v(LN(m)), softmax over the L keys of each head, to_out -- formed densely on a few pixel
    rows -- against LN(x) . Kq^T and attn . Vo of the reference's operands"""
    heads, dh, L, S, B, layers = case
    c = T.prep_case(F32, *case)
    r = c["ref"]
    g = T.gen(90, *case)
    xl = T.randn(g, S, 5, D)                      # five pixel rows per image, already normalised
    for ly in range(layers):
        p = {nm: T.prep_view(c["arena"], ly, nm, heads, dh) for nm in T.PREP_NAMES}
        m = F.layer_norm(T.prep_rows(c["tok"], c), (D,), p["g"], p["b"], T.EPS)
        assert rel(m, r["mn"][ly]) < 1e-12
        q = (xl @ p["wq"].t()).view(S, 5, heads, dh).transpose(1, 2)
        k = (m @ p["wk"].t()).view(S, L, heads, dh).transpose(1, 2)
        v = (m @ p["wv"].t()).view(S, L, heads, dh).transpose(1, 2)
        dots = q @ k.transpose(-1, -2) * T.SCALE                              # [S, heads, 5, L]
        attn = dots.softmax(-1)
        out = (attn @ v).transpose(1, 2).reshape(S, 5, heads * dh) @ p["wo"].t()
        HL = heads * L
        assert float(r["kq"][ly][:, HL:].abs().max() if HL < c["HLP"] else 0) == 0
        dots2 = (xl @ r["kq"][ly][:, :HL].transpose(1, 2)).view(S, 5, heads, L).transpose(1, 2)
        assert rel(dots2, dots) < 1e-12
        out2 = attn.transpose(1, 2).reshape(S, 5, HL) @ r["vo"][ly][:, :HL]
        assert rel(out2, out) < 1e-12
        st = r["mstats"][ly]
        rows = T.prep_rows(c["tok"], c)
        assert rel(st[..., 0], rows.mean(-1)) < 1e-12 and rel(st[..., 1], 1 / torch.sqrt(rows.var(-1, unbiased=False) + T.EPS)) < 1e-12
    # the token gradient, image by image, lands where the addressing says
    assert rel(sum(T.prep_scatter(d, c) for d in r["dimg_layers"]), r["dtok"]) < 1e-13
    assert rel(sum(r["dtok_layers"]), r["dtok"]) < 1e-13


def test_tokenizer_reference_equals_the_convolution_form():
    for S, B in T.TOK_FORMS:
        c = T.tok_case(F32, 4, 257, S, B)
        L = c["L"]
        x = c["x"].clone().requires_grad_(True)
        wa, pos = c["wa"].clone().requires_grad_(True), c["pos"].clone().requires_grad_(True)
        xi = x.transpose(1, 2).reshape(S, D, 257, 1)
        att = torch.softmax(F.conv2d(xi, wa.view(L, D, 1, 1)).reshape(S, L, -1), -1)
        tk = torch.einsum("sln,scn->slc", att, xi.reshape(S, D, -1))
        streams = [tk[i * B:(i + 1) * B] for i in range(S // B)]
        cat = torch.cat(streams, 1) + pos[:len(streams) * L]
        (cat * c["dtok"][:, :len(streams) * L]).sum().backward()
        r = c["ref"]
        assert rel(cat, r["tok"][:, :len(streams) * L]) < 1e-12 and torch.equal(r["tok"][:, len(streams) * L:], c["tok0"][:, len(streams) * L:])
        assert rel(x.grad, r["dx"]) < 1e-12 and rel(wa.grad, r["dwa"]) < 1e-11 and rel(pos.grad, r["dpos"]) < 1e-12
    c = T.tok_case(F32, 8, 1, 6, 3)
    assert float(c["ref"]["dwa"].abs().max()) == 0.0 and T.tok_cancel_scale(c) > 1.0


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.name)
def test_fallback_references(dtype):
    for case in T.SOFTMAX_CASES:
        c = T.softmax_case(dtype, *case)
        HL = c["heads"] * c["L"]
        y, dx = T.softmax_autograd(c)
        assert rel(c["y"][:, :HL], y) < 1e-13 and float(c["y"][:, HL:].abs().max() if HL < c["HLP"] else 0) == 0
        # the backward AT the rounded y differs from autograd's by y's rounding, times the factor-4 bound's quarter at most
        assert rel(c["dx"][:, :HL], dx[:, :HL]) <= (1e-6 if dtype == F32 else T.F_DATA * T.tol(dtype) / 4)
        if dtype == F32:
            assert rel(c["y_saved"], c["y"]) < 1e-7
    for case in T.ATTN_CASES:
        c = T.attn_case(dtype, *case)
        B, n, heads, dh = case
        qkv = c["qkv"].clone().requires_grad_(True)
        q, k, v = (t.reshape(B, n, heads, dh).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
        o = F.scaled_dot_product_attention(q, k, v, scale=T.SCALE).transpose(1, 2).reshape(B * n, heads * dh)
        o.backward(c["dout"])
        assert rel(o, c["ref"]["o"]) < 1e-12 and rel(qkv.grad, c["ref"]["dqkv"]) < 1e-12


# ---- every bound, against the reference alone ----
@pytest.mark.parametrize("L", T.TOK_L)
def test_tokenizer_bounds_hold_fourfold_for_the_float32_reference(L):
    worst = {}
    for S, B in T.TOK_FORMS:
        for HW in T.TOK_HW:
            c = T.tok_case(F32, L, HW, S, B)
            r = T.tok_ref(c, dtype=F32)
            for acc in (False, True):
                got = dict(tok=r["tok"], dx=c["dx0"].float() + r["dx"], dwa=r["dwa"] + (c["dwa0"].float() if acc else 0), dpos=r["dpos"] + (c["dpos0"].float() if acc else 0))
                T.check_all(got, T.tok_want(c, acc), T.tok_spec(c, acc), "float32 reference, tokenizer L=%d HW=%d S=%d B=%d" % (L, HW, S, B), worst, shrink=0.25)
            cb = T.tok_case(BF16, L, HW, S, B)
            want = T.tok_want(cb, True)
            T.check_all({k: (T.rounded(v, BF16) if k == "dx" else T.rounded(v, F32)) for k, v in want.items()}, want, T.tok_spec(cb, True),
                        "reference rounded to bf16, tokenizer", shrink=0.25)
    print("float32 reference of the tokenizer, worst ratios:", worst)


@pytest.mark.parametrize("case", T.ENC_CASES, ids=lambda c: "-".join(map(str, c)))
def test_encoder_bounds_hold_fourfold_for_the_float32_reference(case):
    c = T.enc_case(*case)
    r = T.enc_ref(c, dtype=F32)
    garena = T.enc_total(c, r, F32)
    worst = {}
    T.enc_check(c, r["y"], r["dx"], garena, "float32 reference, encoder %s" % (case,), worst, shrink=0.25)
    print("float32 reference of the encoder %s: worst ratio %.3e" % (case, max(worst.values())))


def prep_got_from(c, r, dtype_out):
    """what a kernel that computed `r` exactly would leave: the stored types' roundings, kqT / voT transposed"""
    got = {k: T.rounded(r[k], F32) for k in ("mn", "mstats", "k", "v")}
    for a, b in (("kq", "kqT"), ("vo", "voT")):
        got[a] = r[a].to(dtype_out)
        got[b] = got[a].transpose(-1, -2).contiguous()
    return got


@pytest.mark.parametrize("case", T.PREP_SCALAR, ids=lambda c: "-".join(map(str, c)))
def test_preparation_bounds_hold_fourfold_for_the_float32_reference(case):
    c = T.prep_case(F32, *case)
    r = T.prep_ref(c, dtype=F32)
    T.prep_check_fwd(c, prep_got_from(c, r, F32), "float32 reference, preparation %s" % (case,), shrink=0.25)
    garena = c["garena0"].float() + r["garena"]
    T.prep_check_bwd(c, T.prep_bwd_got(c, c["dtok0"].float() + r["dtok"], garena), "float32 reference, preparation %s" % (case,), shrink=0.25)
    cb = T.prep_case(BF16, *case)
    T.prep_check_fwd(cb, prep_got_from(cb, cb["ref"], BF16), "reference rounded to bf16, preparation %s" % (case,), shrink=0.25)


@pytest.mark.parametrize("case", T.PREP_MFMA, ids=lambda c: "-".join(map(str, c)))
def test_matrix_core_preparation_bounds_hold_fourfold_for_the_rounded_reference(case):
    heads, dh, S, B, layers = case
    c = T.prep_case(BF16, heads, dh, 4, S, B, layers, mfma=True)
    r = c["ref"]
    T.prep_check_fwd(c, prep_got_from(c, r, BF16), "reference rounded to bf16, matrix-core preparation %s" % (case,), shrink=0.25)
    # the roundings the kernel documents move k / v / kq / vo by less than a quarter of the bf16 bound from the unrounded product
    plain = T.prep_ref(dict(c, mfma=False))
    for k in ("k", "v", "kq", "vo"):
        assert rel(r[k], plain[k]) <= T.tol(BF16) / 4, k
    for k in ("dtok", "garena"):
        assert rel(r[k], plain[k]) <= T.F_DATA * T.tol(BF16) / 4, k


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.name)
def test_fallback_bounds_hold_fourfold(dtype):
    for case in T.ATTN_CASES:
        c = T.attn_case(dtype, *case)
        r = T.attn_ref(c, dtype=F32) if dtype == F32 else {k: T.rounded(v, BF16) for k, v in c["ref"].items()}
        T.check_all(r, c["ref"], dict(o=(dtype, T.F_FWD), attn=(F32, T.F_FWD) if dtype == F32 else (dtype, T.F_FWD), dqkv=(dtype, T.F_DATA)),
                    "attention %s" % (case,), shrink=0.25)
    for case in T.SOFTMAX_CASES:
        c = T.softmax_case(dtype, *case)
        y, dx = T.softmax_autograd(c, dtype=F32) if dtype == F32 else (T.rounded(c["y"], BF16)[:, :c["heads"] * c["L"]], T.rounded(c["dx"], BF16))
        HL = c["heads"] * c["L"]
        T.check_all(dict(y=y, dx=dx[:, :HL]), dict(y=c["y"][:, :HL], dx=c["dx"][:, :HL]), dict(y=(dtype, T.F_FWD), dx=(dtype, T.F_DATA)),
                    "grouped softmax %s" % (case,), shrink=0.25)


# ---- the checkers turn red on planted errors ----
def test_checkers_fail_on_planted_tokenizer_errors():
    c = T.tok_case(F32, 4, 2049, 2, 1)
    want, spec = T.tok_want(c, False), T.tok_spec(c, False)
    T.check_all({k: v.float() for k, v in want.items()}, want, spec, "exact")
    with pytest.raises(AssertionError, match="tok"):       # one chunk left out of the pooled sum
        T.check_all(dict(want, tok=T.tok_ref(c, drop_chunk=1)["tok"]), want, dict(tok=spec["tok"]), "planted")
    c1 = T.tok_case(F32, 4, 2, 2, 2)                        # the absent stream's rows overwritten
    bad = c1["ref"]["tok"].clone()
    bad[:, 4:] = 0
    with pytest.raises(AssertionError, match="absent"):
        T.same_bits(bad[:, 4:].float(), c1["tok0"][:, 4:].float(), "absent rows")
    # accumulate dropped: dwa overwritten where it should have been added
    c2 = T.tok_case(F32, 8, 65, 6, 3)
    with pytest.raises(AssertionError, match="dwa"):
        T.check_all(dict(T.tok_want(c2, True), dwa=c2["ref"]["dwa"]), T.tok_want(c2, True), T.tok_spec(c2, True), "planted")


def test_checkers_fail_on_planted_preparation_errors():
    case = T.PREP_SCALAR[2]
    heads, dh, L, S, B, layers = case
    c = T.prep_case(F32, *case)
    r = c["ref"]
    good = prep_got_from(c, r, F32)
    T.prep_check_fwd(c, good, "exact")
    bad = dict(good, kq=good["kq"].clone())                 # two heads swapped in Kq
    bad["kq"][:, :, 0:L], bad["kq"][:, :, L:2 * L] = good["kq"][:, :, L:2 * L], good["kq"][:, :, 0:L]
    bad["kqT"] = bad["kq"].transpose(-1, -2).contiguous()
    with pytest.raises(AssertionError, match="kq"):
        T.prep_check_fwd(c, bad, "planted")
    with pytest.raises(AssertionError, match="transpose"):  # kqT not transposed
        T.prep_check_fwd(c, dict(good, kqT=good["kq"].reshape(good["kqT"].shape)), "planted")
    cp = T.prep_case(F32, *T.PREP_SCALAR[1])                # heads L = 12 of HLP = 32 rows
    pad = prep_got_from(cp, cp["ref"], F32)
    T.prep_check_fwd(cp, pad, "exact")
    pad["vo"][0, 0, -1, 0] = 1e-30
    pad["voT"] = pad["vo"].transpose(-1, -2).contiguous()
    with pytest.raises(AssertionError, match="padding"):
        T.prep_check_fwd(cp, pad, "planted")
    want = T.prep_bwd_want(c)
    exact = {k: v.float() for k, v in want.items()}
    T.prep_check_bwd(c, exact, "exact")
    with pytest.raises(AssertionError, match="dtok"):       # one layer left out of the token gradient
        T.prep_check_bwd(c, dict(exact, dtok=c["dtok0"] + r["dtok"] - r["dtok_layers"][1]), "planted")
    with pytest.raises(AssertionError, match="dtok"):       # one image's rows shifted by one stream
        T.prep_check_bwd(c, dict(exact, dtok=c["dtok0"] + sum(T.prep_scatter(d, c, shift_image=1) for d in r["dimg_layers"])), "planted")
    with pytest.raises(AssertionError, match=r"dwq\[1\]"):  # scale dropped from dWq
        T.prep_check_bwd(c, {**exact, "dwq[1]": T.prep_view(c["garena0"], 1, "wq", heads, dh) + T.prep_view(r["garena"], 1, "wq", heads, dh) / T.SCALE}, "planted")
    with pytest.raises(AssertionError, match=r"dg\[0\]"):   # LayerNorm gradients overwritten instead of added
        T.prep_check_bwd(c, {**exact, "dg[0]": T.prep_view(r["garena"], 0, "g", heads, dh)}, "planted")
    # accumulate = 0 leaves the LayerNorm gradients added and the four matrices overwritten
    w0 = T.prep_bwd_want(c, accumulate=False)
    assert torch.equal(w0["dg[0]"], want["dg[0]"]) and torch.equal(w0["dwk[0]"], T.prep_view(r["garena"], 0, "wk", heads, dh))


def test_checkers_fail_on_planted_encoder_errors():
    c = T.enc_case(*T.ENC_CASES[2])
    r = c["ref"]
    garena = T.enc_total(c, r)
    T.enc_check(c, r["y"], r["dx"], garena, "exact")
    bad = garena.clone()
    v = T.enc_views(bad, c["depth"], c["heads"], c["dim_head"], c["mlp"])[1][2]
    inner = c["heads"] * c["dim_head"]
    v[inner:inner + c["dim_head"]] *= 1.001               # one head of one layer's k block off by 1e-3
    with pytest.raises(AssertionError, match=r"dwqkv\[1\]"):
        T.enc_check(c, r["y"], r["dx"], bad, "planted")
    with pytest.raises(AssertionError, match=r"dln2_g\[0\]"):      # not accumulated
        over = garena.clone()
        T.enc_views(over, c["depth"], c["heads"], c["dim_head"], c["mlp"])[0][5].copy_(r["grads"][0][5])
        T.enc_check(c, r["y"], r["dx"], over, "planted")
    with pytest.raises(AssertionError, match="between"):
        gap = garena.clone()
        gap[-1] += 1
        T.enc_check(c, r["y"], r["dx"], gap, "planted")
