"""Every launch form of the token-side kernels (csrc/tokens.hip: tokenizer, cross-attention operand preparation in its scalar and
matrix-core forms, grouped softmax, self-attention core; csrc/encoder_fused.hip: the fused token encoder) against a plain float64
computation of the same operation, at the sizes where the launch code takes another path.

One kernel family per comparison: the inputs of each come from tests/_token_cases.py, never from the kernel in front of it; a
backward that reads saved intermediates gets them formed in float64 (the tokenizer's logits / statistics / pooled tokens, the
preparation's mn / mstats / k / v, the attention probabilities, the softmax output).  The one exception is the fused encoder, whose
backward reads the opaque per-(layer, image) LDS image its own forward saved: forward and backward are checked as the pair they are.
The recorded forms (ops.EncoderBatch) run through the ops entry points as the engine calls them, so there the backward reads what
the forward saved; each result is compared with float64 AND bit for bit with its own unrecorded launch.

Bounds: _bounds.close, max |got - want| <= factor x tol(dtype) x max |want|, factor 1 for forward outputs and the encoder's dx, 4 for
data and parameter gradients, 8 for the tokenizer's dWa.  tol is the fp32 one wherever operands and result are fp32 in either form
(tokens, dWa, dpos, the saved fp32 tensors and every gradient of the scalar preparation), the bf16 one for tensors stored in bf16 and
for everything the matrix-core preparation computes from bf16-rounded operands.  tests/test_token_edges_cpu.py shows that the same
reference evaluated in float32 meets every bound fourfold.  Every figure is printed before it is asserted.

Worst distances measured on MI355X, as fractions of the tensor's maximum (bound in brackets): see each test's docstring."""
import contextlib

import pytest
import torch

import _token_cases as T
from _token_cases import F32, BF16, D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dahitra_amd import ops as o
    return o


def lib():
    from dahitra_amd import _lib
    return _lib.lib()


def dev(x, dtype=F32):
    return x.to(dtype).cuda().contiguous()


def nan_like(x):
    return torch.full(tuple(x.shape), float("nan"), dtype=F32, device="cuda")


def ids(cases):
    return ["-".join(map(str, c)) for c in cases]


def report(what, worst):
    print("WORST %s: %s" % (what, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


def fold(worst):
    """{key[layer]: ratio} -> {key: worst ratio over the layers}"""
    out = {}
    for k, v in worst.items():
        k = k.split("[")[0]
        out[k] = max(out.get(k, 0.0), v)
    return out


# ---- 1. tokenizer ----
def tokenizer_fwd_into(ops, x, wa, pos, B, L, tok):
    """ops.tokenizer_fwd with a caller-owned tok_cat (ops allocates it uninitialised: the rows of an absent stream could not be
    told from garbage); returns what the forward saves"""
    Sn, HW = x.shape[0], x.shape[1] * x.shape[2]
    logits = torch.empty(Sn * HW, L, dtype=F32, device="cuda")
    stats = torch.empty(Sn, L, 2, dtype=F32, device="cuda")
    pooled = torch.empty(Sn, L, D, dtype=F32, device="cuda")
    ws = ops.workspace(lib().dh_tokenizer_fwd_workspace_size(Sn, HW, L), x.device)
    ops._call("dh_tokenizer_fwd", ops.dt(x), ops.P(x), ops.P(wa), ops.P(pos), Sn, B, HW, L, ops.P(logits), ops.P(stats), ops.P(pooled),
              ops.P(tok), ops.P(ws), ops.S())
    return logits, stats, pooled


@pytest.mark.parametrize("form", T.TOK_FORMS, ids=ids(T.TOK_FORMS))
@pytest.mark.parametrize("L", T.TOK_L)
@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.name)
def test_tokenizer_every_chunk_block_and_accumulate_form(ops, dtype, L, form):
    """dh_tokenizer_fwd / _bwd at HW = 1, around the 64-pixel block of tok_bwd_body (dead quad lanes) and the 256-row block of
    tok_logits_body / tok_stats_body, one long chunk (2047), two chunks of 1024, 1025 + 1024, three chunks with a short last one
    (3100); two streams of one and three images and ONE stream of two (the absent stream's rows of a prefilled tok_cat stay as they
    were); S HW through 1, 2, up to 8 and more than 8 partials of the dWa reduce; dx added onto a nonzero dx_accum; accumulate = False
    onto NaN-filled dwa / dpos and accumulate = True onto prefilled ones.  At HW = 1 (p = 1) dWa is zero by cancellation and is
    held to the size of the cancelling terms max |dtok| max |x|^2.

    Measured on MI355X (worst over all 12 parametrisations): tok 7.9e-7 [2e-5], dx 7.0e-7 fp32 / 3.8e-3 bf16 [8e-5 / 0.1],
    dWa 1.5e-6 [1.6e-4], dpos 9.1e-8 [8e-5]; saved logits 2.9e-7, softmax maximum 2.8e-7, 1 / sum 1.9e-6, pooled tokens 1.1e-6 [2e-5]."""
    S, B = form
    streams, worst = S // B, {}
    for HW in T.TOK_HW:
        c = T.tok_case(dtype, L, HW, S, B)
        r = c["ref"]
        what = "tokenizer %s L=%d HW=%d S=%d B=%d (%s chunks, %d partials)" % (T.name(dtype), L, HW, S, B, T.tok_chunk_sizes(HW), T.tok_nblk(S, HW))
        x, wa, pos = dev(c["x"].view(S, HW, 1, D), dtype), dev(c["wa"]), dev(c["pos"])
        tok = dev(c["tok0"])
        logits, stats, pooled = tokenizer_fwd_into(ops, x, wa, pos, B, L, tok)
        if streams == 1:
            T.same_bits(tok[:, L:], dev(c["tok0"])[:, L:], what + " rows of the absent stream")
        # what the forward saves, against the float64 of the same inputs (the softmax maximum is exact: a maximum of fp32 logits)
        saved_spec = dict(logits=(F32, T.F_FWD), smax=(F32, T.F_FWD), sinv=(F32, T.F_FWD), pooled=(F32, T.F_FWD))
        T.check_all(dict(logits=logits.view(S, HW, L), smax=stats[..., 0], sinv=stats[..., 1], pooled=pooled),
                    dict(r, smax=r["stats"][..., 0], sinv=r["stats"][..., 1]), saved_spec, what + " saved", worst)
        saved = (dev(r["logits"].reshape(S * HW, L)), dev(r["stats"]), dev(r["pooled"]))
        for acc in (False, True):
            dx = dev(c["dx0"].view(S, HW, 1, D), dtype)
            dwa, dpos = (dev(c["dwa0"]), dev(c["dpos0"])) if acc else (nan_like(c["dwa0"]), nan_like(c["dpos0"]))
            ops.tokenizer_bwd(x, wa, saved, dev(c["dtok"]), dx, dwa, dpos, B, L, accumulate=acc)
            T.check_all(dict(tok=tok, dx=dx.view(S, HW, D), dwa=dwa, dpos=dpos), T.tok_want(c, acc), T.tok_spec(c, acc),
                        "%s accumulate=%d" % (what, acc), worst)
    report("tokenizer %s L=%d S=%d B=%d" % (T.name(dtype), L, S, B), worst)


@pytest.mark.parametrize("L", T.TOK_L)
@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.name)
def test_tokenizer_calls_recorded_in_an_encoder_batch(ops, dtype, L):
    """five tokenizer calls of one (dtype, token_len) and different HW / B inside ops.EncoderBatch(decoder=True): TB_MAXJ = 4, so
    the fifth call issues the first four (one call is pending afterwards), forward and backward.  Every result against float64 and
    bit for bit against the same calls outside a batch.

    Measured on MI355X: tok 7.7e-7 [2e-5], dx 4.5e-7 fp32 / 2.7e-3 bf16 [8e-5 / 0.1], dWa 6.6e-7 [1.6e-4], dpos 6.5e-8 [8e-5]."""
    cases = [T.tok_case(dtype, L, HW, S, B) for HW, S, B in T.TOK_RECORDED]
    ins = [dict(x=dev(c["x"].view(c["S"], c["HW"], 1, D), dtype), wa=dev(c["wa"]), pos=dev(c["pos"]), dtok=dev(c["dtok"])) for c in cases]

    def run(recorded):
        bufs = [dict(dx=dev(c["dx0"].view(c["S"], c["HW"], 1, D), dtype), dwa=dev(c["dwa0"]), dpos=dev(c["dpos0"])) for c in cases]
        with (ops.EncoderBatch(decoder=True) if recorded else contextlib.nullcontext()) as eb:
            if recorded:
                assert eb.on and eb.xprep
            fw = [ops.tokenizer_fwd(i["x"], i["wa"], i["pos"], c["B"], L) for i, c in zip(ins, cases)]
            if recorded:
                assert lib().dh_xprep_batch_pending() == len(cases) - T.TB_MAXJ
                eb.launch()
                assert lib().dh_xprep_batch_pending() == 0
            for i, c, b, (tok, saved) in zip(ins, cases, bufs, fw):
                ops.tokenizer_bwd(i["x"], i["wa"], saved, i["dtok"], b["dx"], b["dwa"], b["dpos"], c["B"], L, accumulate=True)
            if recorded:
                assert lib().dh_xprep_batch_pending() == len(cases) - T.TB_MAXJ
                eb.launch()
        torch.cuda.synchronize()
        return [dict(tok=tok[:, :(c["S"] // c["B"]) * L], dx=b["dx"].view(c["S"], c["HW"], D), dwa=b["dwa"], dpos=b["dpos"])
                for c, b, (tok, saved) in zip(cases, bufs, fw)]
    eager, recorded = run(False), run(True)
    worst = {}
    for c, e, g in zip(cases, eager, recorded):
        what = "recorded tokenizer %s L=%d HW=%d S=%d B=%d" % (T.name(dtype), L, c["HW"], c["S"], c["B"])
        want = T.tok_want(c, True)
        want["tok"] = want["tok"][:, :(c["S"] // c["B"]) * L]
        T.check_all(g, want, T.tok_spec(c, True), what, worst)
        for k in g:
            T.same_bits(g[k], e[k], "%s %s, recorded vs its own launch" % (what, k))
    report("recorded tokenizer %s L=%d" % (T.name(dtype), L), worst)


# ---- 2. fused token encoder ----
def encoder_device(c):
    arena, garena = dev(c["arena"]), dev(c["garena0"])
    v = lambda a: T.enc_views(a, c["depth"], c["heads"], c["dim_head"], c["mlp"])[0]
    return dict(arena=arena, garena=garena, params=v(arena), grads=v(garena), x=dev(c["x"]), dy=dev(c["dy"]),
                shape=(c["B"], c["n"], c["depth"], c["heads"], c["dim_head"], c["mlp"], c["stride"]))


@pytest.mark.parametrize("case", T.ENC_CASES, ids=ids(T.ENC_CASES))
def test_fused_encoder_against_float64_autograd(ops, case):
    """dh_encoder_fwd / dh_encoder_bwd (three kernels) on depth layers `pstride` floats apart in one flat arena, every parameter at a
    multiple of 4 floats: y, dx and all 11 gradient tensors of every layer, ADDED onto a nonzero gradient arena whose gaps stay
    untouched.  The product's shape (dynamic LDS above 64 KB, every pair lane live), four layers, half the heads, inner = 16 with an
    odd mlp, the generic n < 8 paths (n = 6, 4, 2), B = 1, and n = 1 where the q / k blocks of dWqkv are exactly zero.

    Measured on MI355X (worst case of the eight): y 6.9e-7, dx 7.1e-7 [2e-5]; parameter gradients 1.2e-6 (dln2_g of the four-layer
    stack) [8e-5]."""
    c = T.enc_case(*case)
    d = encoder_device(c)
    assert ops.encoder_supported(*case[1:2] + case[3:])
    y, xs = ops.encoder_fwd(d["x"], *d["shape"], d["params"], True)
    dx = ops.encoder_bwd(d["dy"], xs, *d["shape"], d["params"], d["grads"])
    worst = {}
    T.enc_check(c, y, dx, d["garena"], "encoder %s" % (case,), worst)
    report("encoder %s" % (case,), fold(worst))


def test_fused_encoder_stacks_recorded_in_one_batch_against_float64(ops):
    """five stacks of different shapes in one ops.EncoderBatch: ENC_MAXJ = 4, so recording the fifth issues the first four (one is
    pending afterwards), forward and backward + weight-gradient launch; every stack against float64

    Measured on MI355X: y 5.3e-7, dx 6.6e-7 [2e-5]; parameter gradients 6.4e-7 [8e-5]."""
    cases = [T.enc_case(*T.ENC_CASES[i]) for i in T.ENC_BATCHED]
    ds = [encoder_device(c) for c in cases]
    with ops.EncoderBatch() as eb:
        assert eb.on
        fw = [ops.encoder_fwd(d["x"], *d["shape"], d["params"], True) for d in ds]
        assert lib().dh_encoder_batch_pending() == len(cases) - T.ENC_MAXJ
        eb.launch()
        dxs = [ops.encoder_bwd(d["dy"], xs, *d["shape"], d["params"], d["grads"]) for d, (y, xs) in zip(ds, fw)]
        assert lib().dh_encoder_batch_pending() == len(cases) - T.ENC_MAXJ
        eb.launch()
    torch.cuda.synchronize()
    worst = {}
    for c, d, (y, xs), dx in zip(cases, ds, fw, dxs):
        T.enc_check(c, y, dx, d["garena"], "batched encoder B=%d n=%d depth=%d heads=%d" % (c["B"], c["n"], c["depth"], c["heads"]), worst)
    report("batched encoder", fold(worst))


# ---- 3. cross-attention operand preparation ----
def prep_device(c):
    heads, dh, layers, dt = c["heads"], c["dim_head"], c["layers"], c["dtype"]
    arena, garena = dev(c["arena"]), dev(c["garena0"])
    pack = {nm: torch.stack([T.prep_view(arena, l, nm, heads, dh).t().contiguous().to(dt).reshape(-1) for l in range(layers)])
            for nm in ("wq", "wk", "wv", "wo")}
    for nm in pack:                                # the packed copy carries the master's values
        assert torch.equal(pack[nm][0].float().view(T.prep_view(arena, 0, nm, heads, dh).t().shape), T.prep_view(arena, 0, nm, heads, dh).t())
    p0 = {nm: T.prep_view(arena, 0, nm, heads, dh) for nm in T.PREP_NAMES}
    g0 = {nm: T.prep_view(garena, 0, nm, heads, dh) for nm in T.PREP_NAMES}
    return dict(arena=arena, garena=garena, pack=pack, p0=p0, g0=g0, tok=dev(c["tok"]), dtok=dev(c["dtok0"]),
                addr=(c["bstride"], c["sstride"], c["B"], c["S"], c["L"], heads, dh))


def prep_stack(ops, c, d, **kw):
    p0, pack = d["p0"], d["pack"]
    masters = (p0["wk"], p0["wv"], p0["wo"], pack["wq"]) if c["mfma"] else None
    bstride, sstride, B, S, L, heads, dh = d["addr"]
    st = ops.XattnPrepStack(d["tok"], bstride, sstride, B, S, L, heads, dh, c["layers"], c["stride"], p0["g"], p0["b"], p0["wq"], pack["wk"],
                            pack["wv"], pack["wo"], c["dtype"], masters=masters, **kw)
    assert st.mfma == c["mfma"] and st.HLP == c["HLP"]
    return st


FWD_KEYS = ("mn", "mstats", "k", "v", "kq", "kqT", "vo", "voT")


def prep_load_saved(c, st):
    """the backward's inputs: mn / mstats / k / v formed in float64 and rounded to fp32, dkq / dvoT with zeros in the padding"""
    r = c["ref"]
    for k in ("mn", "mstats", "k", "v"):
        getattr(st, k).copy_(dev(r[k]).view(getattr(st, k).shape))
    if hasattr(st, "dkq"):
        st.dkq.copy_(dev(c["dkq"]))
        st.dvoT.copy_(dev(c["dvoT"]))


def prep_stack_backward(c, d, st):
    p0, g0, pack = d["p0"], d["g0"], d["pack"]
    st.backward(d["tok"], d["dtok"], p0["g"], pack["wq"], p0["wk"], p0["wv"], p0["wo"], g0["g"], g0["b"], g0["wq"], g0["wk"], g0["wv"], g0["wo"])


def prep_gaps_untouched(c, d, what):
    _, _, stride = T.prep_layout(c["heads"], c["dim_head"])
    for l in range(c["layers"]):
        T.same_bits(d["garena"][(l + 1) * stride - 8:(l + 1) * stride], dev(c["garena0"])[(l + 1) * stride - 8:(l + 1) * stride], what + " arena gap")


def run_prep_stack(ops, c, what, worst):
    d = prep_device(c)
    st = prep_stack(ops, c, d)
    T.prep_check_fwd(c, {k: getattr(st, k) for k in FWD_KEYS}, what, worst)
    prep_load_saved(c, st)
    prep_stack_backward(c, d, st)
    T.prep_check_bwd(c, T.prep_bwd_got(c, d["dtok"], d["garena"]), what, True, worst)
    prep_gaps_untouched(c, d, what)


@pytest.mark.parametrize("case", T.PREP_SCALAR, ids=ids(T.PREP_SCALAR))
@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.name)
def test_scalar_preparation_stack_against_float64(ops, dtype, case):
    """xattn_prep_kernel / xattn_prep_bwd_kernel / dtok_reduce_kernel / xattn_prep_wgrad_kernel (masters = None): L = 4 with every
    row of HLP = 32 live; ONE stream (sstride = 0) with S = 3 below the 8 image phases and 12 of 32 rows; L = 8 with two layers
    (dtok_part + dtok_reduce, the arena stride); HLP = 64 with S = 9 past the phases and three layers.  mn, mstats, k, v, kq, vo
    against float64, kqT / voT bit for bit the transposes, padding rows exactly zero; the token gradient ADDED onto a prefilled
    buffer with the tokens' addressing and summed over the layers; dwq / dwk / dwv / dwo accumulated, dln_g / dln_b added.

    Measured on MI355X: fp32 outputs (mn, mstats, k, v; kq, vo in fp32) below 3.2e-7 [2e-5], kq / vo in bf16 2.8e-3 [2.5e-2],
    token gradient 1.3e-7, parameter gradients 2.8e-7 [8e-5], in either form."""
    c = T.prep_case(dtype, *case)
    worst = {}
    run_prep_stack(ops, c, "scalar preparation %s %s" % (T.name(dtype), case), worst)
    report("scalar preparation %s %s" % (T.name(dtype), case), fold(worst))


@pytest.mark.parametrize("case", T.PREP_MFMA, ids=ids(T.PREP_MFMA))
def test_matrix_core_preparation_stack_against_float64(ops, case):
    """xattn_prep_mfma_kernel<64 / 32>, xattn_prep_bwd_mfma_kernel, and behind it either xattn_prep_wgrad_mfma_kernel + the ln_only
    launch (dim_head 64, S % 8 == 0: one, two -- the prefetch -- and three 32-row steps) or the scalar weight-gradient kernel
    (S = 4; dim_head 32), with heads that are not a multiple of the four waves, the layer reduce, and S = B.  The float64 reference
    applies the kernel's documented roundings (bf16 weights, LN(tokens), k and v rounded to bf16 before the products).

    Measured on MI355X: mn / mstats 1.2e-7 [2e-5]; k, v 9.8e-8 (no rounding tie fell the other way), kq / vo 3.1e-3 [2.5e-2]; token
    gradient 1.5e-3, parameter gradients 3.3e-3 (dln_g) [0.1]."""
    heads, dh, S, B, layers = case
    c = T.prep_case(BF16, heads, dh, 4, S, B, layers, mfma=True)
    worst = {}
    run_prep_stack(ops, c, "matrix-core preparation %s" % (case,), worst)
    report("matrix-core preparation %s" % (case,), fold(worst))


SINGLE = [(F32, False) + T.PREP_SCALAR[0], (BF16, False) + T.PREP_SCALAR[1], (BF16, True, 8, 64, 4, 8, 4, 1), (BF16, True, 1, 32, 4, 12, 6, 1)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", SINGLE, ids=["-".join([T.name(c[0]), "mfma" if c[1] else "scalar"] + list(map(str, c[2:]))) for c in SINGLE])
def test_single_layer_preparation_entry_honours_accumulate(ops, case, accumulate):
    """ops.XattnPrep / ops.xattn_prep_bwd (dh_xattn_prep_fwd, dh_xattn_prep_bwd, and the matrix-core entries with layers = 1):
    accumulate = 0 overwrites NaN-filled dwq / dwk / dwv / dwo, accumulate = 1 adds onto prefilled ones; dln_g / dln_b are added in
    both (the pixel-side LayerNorm backward wrote its part already)

    Measured on MI355X: scalar entry within the figures of the scalar stack test; matrix-core entry kq / vo 2.8e-3 [2.5e-2], token
    gradient 1.5e-3, parameter gradients 2.5e-3 (dwv, accumulate = 0) [0.1]."""
    dtype, mfma, heads, dh, L, S, B, layers = case
    c = T.prep_case(dtype, heads, dh, L, S, B, layers, mfma)
    d = prep_device(c)
    p0, g0, pack = d["p0"], d["g0"], d["pack"]
    masters = (p0["wk"], p0["wv"], p0["wo"], pack["wq"]) if mfma else None
    prep = ops.XattnPrep(d["tok"], *d["addr"], p0["g"], p0["b"], p0["wq"], pack["wk"][0], pack["wv"][0], pack["wo"][0], dtype, masters=masters)
    assert prep.mfma == mfma
    what, worst = "single-layer preparation %s accumulate=%d" % (case, accumulate), {}
    T.prep_check_fwd(c, {k: getattr(prep, k)[None] for k in FWD_KEYS}, what, worst)
    prep_load_saved(c, prep)
    if not accumulate:
        for nm in ("wq", "wk", "wv", "wo"):
            g0[nm].fill_(float("nan"))
    ops.xattn_prep_bwd(prep, d["tok"], d["dtok"], p0["g"], pack["wq"][0], p0["wk"], p0["wv"], p0["wo"], dev(c["dkq"][0]), dev(c["dvoT"][0]),
                       g0["g"], g0["b"], g0["wq"], g0["wk"], g0["wv"], g0["wo"], accumulate, dtype)
    T.prep_check_bwd(c, T.prep_bwd_got(c, d["dtok"], d["garena"]), what, bool(accumulate), worst)
    prep_gaps_untouched(c, d, what)
    report(what, fold(worst))


def test_preparation_stacks_recorded_in_an_encoder_batch(ops):
    """three dim_head = 64 stacks of different (heads, S, layers) recorded inside ops.EncoderBatch(decoder=True) and launched: the
    forward family as one launch, the backward as its four (operand gradients, token-gradient reduce, matrix-core weight
    gradients, LayerNorm sums).  Each against float64, and bit for bit against its own unrecorded launch.

    Measured on MI355X: kq / vo 2.7e-3 [2.5e-2], token gradient 1.5e-3, parameter gradients 2.4e-3 [0.1]."""
    cases = [T.prep_case(BF16, heads, dh, 4, S, B, layers, mfma=True) for heads, dh, S, B, layers in T.PREP_RECORDED]

    def run(recorded):
        ds = [prep_device(c) for c in cases]
        with (ops.EncoderBatch(decoder=True) if recorded else contextlib.nullcontext()) as eb:
            if recorded:
                assert eb.xprep and ops.xprep_recording()
            sts = [prep_stack(ops, c, d) for c, d in zip(cases, ds)]
            if recorded:
                assert lib().dh_xprep_batch_pending() == len(cases)
                eb.launch()
                assert lib().dh_xprep_batch_pending() == 0
            fwd = [{k: getattr(st, k).clone() for k in FWD_KEYS} for st in sts]
            for c, d, st in zip(cases, ds, sts):
                prep_load_saved(c, st)
                prep_stack_backward(c, d, st)
            if recorded:
                assert lib().dh_xprep_batch_pending() > 0
                eb.launch()
        torch.cuda.synchronize()
        return fwd, [T.prep_bwd_got(c, d["dtok"], d["garena"]) for c, d in zip(cases, ds)]
    eager, recorded = run(False), run(True)
    worst = {}
    for i, c in enumerate(cases):
        what = "recorded preparation %s" % (T.PREP_RECORDED[i],)
        T.prep_check_fwd(c, recorded[0][i], what, worst)
        T.prep_check_bwd(c, recorded[1][i], what, True, worst)
        for part in (0, 1):
            for k in recorded[part][i]:
                T.same_bits(recorded[part][i][k], eager[part][i][k], "%s %s, recorded vs its own launch" % (what, k))
    report("recorded preparation", fold(worst))


# ---- 4. layer-wise fallbacks ----
@pytest.mark.parametrize("case", T.ATTN_CASES, ids=ids(T.ATTN_CASES))
@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.name)
def test_self_attention_core_against_float64(ops, dtype, case):
    """dh_self_attn_fwd / _bwd: one token, odd token and head counts, n n = 256 (four trips of the 64 threads).  The backward reads
    the probabilities formed in float64.

    Measured on MI355X: out 4.3e-7 fp32 / 2.4e-3 bf16 [2e-5 / 2.5e-2], probabilities 4.3e-7 [2e-5], dqkv 2.5e-7 / 2.1e-3 [8e-5 / 0.1]."""
    B, n, heads, dh = case
    c = T.attn_case(dtype, *case)
    r = c["ref"]
    qkv = dev(c["qkv"], dtype)
    o, attn = ops.self_attn(qkv, B, n, heads, dh)
    dqkv = ops.self_attn_bwd(qkv, dev(r["attn"]), dev(c["dout"], dtype), B, n, heads, dh)
    worst = {}
    T.check_all(dict(o=o, attn=attn, dqkv=dqkv), r, dict(o=(dtype, T.F_FWD), attn=(F32, T.F_FWD), dqkv=(dtype, T.F_DATA)),
                "self-attention %s %s" % (T.name(dtype), case), worst)
    report("self-attention %s %s" % (T.name(dtype), case), worst)


@pytest.mark.parametrize("case", T.SOFTMAX_CASES, ids=ids(T.SOFTMAX_CASES))
@pytest.mark.parametrize("dtype", T.DTYPES, ids=T.name)
def test_grouped_softmax_against_float64(ops, dtype, case):
    """dh_softmax_groups_fwd / _bwd: a single row, padding groups with the grid's tail, L = 8 with 40 of 64 columns, L = 16.  The
    padding columns hold values on the way in and are exactly zero on the way out, forward and backward.

    Measured on MI355X: y 2.3e-7 fp32 / 2.0e-3 bf16 [2e-5 / 2.5e-2], dx 2.4e-7 / 3.3e-3 [8e-5 / 0.1]."""
    rows, heads, L, HLP = case
    c = T.softmax_case(dtype, *case)
    HL = heads * L
    y = ops.softmax_groups(dev(c["x"], dtype), heads, L)
    dx = ops.softmax_groups_bwd(dev(c["y_saved"], dtype), dev(c["dy"], dtype), heads, L)
    worst = {}
    T.check_all(dict(y=y, dx=dx), c, dict(y=(dtype, T.F_FWD), dx=(dtype, T.F_DATA)), "grouped softmax %s %s" % (T.name(dtype), case), worst)
    if HL < HLP:
        assert float(y[:, HL:].float().abs().max()) == 0.0 and float(dx[:, HL:].float().abs().max()) == 0.0
    report("grouped softmax %s %s" % (T.name(dtype), case), worst)
