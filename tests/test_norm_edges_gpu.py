"""Every launch form of the normalisation and reduction kernels (csrc/norm.hip: BatchNorm finalize / eval parameters / apply /
two-pass backward / backward from partials, LayerNorm forward / backward, reduce_partials; csrc/pointwise.hip: dh_colsum) against a
plain float64 computation of the same operation on the CPU, at the sizes where the launch code takes another path.

One kernel per comparison: the inputs of each come from tests/_norm_cases.py (statistics formed in float64 and rounded to float32,
per-tile partials synthesised), never from the kernel in front of it.  Kernels that only sum run on integers in [-8, 8] and must
be EXACT.  Everything else keeps the factor tests/test_kernels_gpu.py states for the same quantity (BatchNorm: forward 1, dx 4,
dgamma 8, dres 1; LayerNorm: forward 1, dx 3, dgamma 8), reduce_partials the 2^-23 of one or two float32 roundings of a float64 sum.
No case needed a wider bound: the constant channels and count = 1 of bn_finalize sit at 1e-7 of the float64 of the same partials
(measured on MI355X: every float32 figure of this file below 2e-6, every bf16 one below 4e-3 = one bf16 rounding of the output).
Every figure is printed before it is asserted; every output is checked for finiteness (in `exact` / `bounded`)."""
import itertools

import pytest
import torch

import _norm_cases as E
from _norm_cases import F32, BF16, bounded, exact

pytestmark = pytest.mark.gpu

SENTINEL = 777.0          # what accumulate=False must overwrite
DG0, DB0 = 0.5, 3.0       # what accumulate=True starts from (DB0 an integer: dbeta stays exact)
WIDTHS = [pytest.param(dt, C, id="%s-%d" % (E.name(dt), C)) for dt in E.DTYPES for C in (32, 64, 24, 48, 96)]
BWD_WIDTHS = [(BF16, 8), (BF16, 32), (BF16, 512), (BF16, 2048), (F32, 4), (F32, 64), (F32, 1024)]


@pytest.fixture(scope="module")
def ops():
    from dahitra_amd import ops as o
    return o


def dev(x, dtype):
    return x.to(dtype).cuda().contiguous()


def full(n, value):
    return torch.full((n,), value, dtype=F32, device="cuda")


# ---- 1. bn_finalize ----
@pytest.mark.parametrize("tpg", E.FIN_TILES)
@pytest.mark.parametrize("G", [1, 2, 4])
def test_bn_finalize_from_synthetic_partials(ops, G, tpg):
    """bn_finalize_kernel: the three wavefront layouts wpg = 4 / G, tiles per group below / at / above its step 64 wpg and twice
    that (the two-accumulator loop, its one-element tail), CP = 32 > C = 24 (NaN in the padding), count = 1 at one tile (var = 0,
    the unbiased guard), two channels constant over each group (the clamp at 0), a channel with mean = 8 std, momentum 0.1 / 0.3,
    eps 1e-5 / 1e-3, num_batches_tracked, and running_mean = None.  Reference: float64 of the same float32 partials."""
    c = E.finalize_case(G, tpg)
    C, n = E.FIN_C, c["count"]
    part, gamma, beta = c["partial"].cuda(), c["gamma"].cuda(), c["beta"].cuda()
    const = list(range(C)) if n == 1 else E.FIN_CONST          # one pixel: every channel is constant
    rest = [k for k in range(C) if k not in const]
    for momentum, eps in itertools.product((0.1, 0.3), (1e-5, 1e-3)):
        want = E.finalize_ref(c, momentum, eps)
        what = "finalize G=%d tiles=%d count=%d momentum=%g eps=%g" % (G, tpg, n, momentum, eps)
        rm, rv = c["rm"].cuda(), c["rv"].cuda()
        nbt = torch.tensor(5, dtype=torch.int64, device="cuda")
        got = dict(zip(("mean", "invstd", "scale", "shift"), ops.bn_finalize(part, C, G, n, gamma, beta, rm, rv, momentum, eps, nbt)))
        assert int(nbt) == 5 + G
        exact(got["mean"][:, E.FIN_INT], want["mean"][:, E.FIN_INT].float(), what + " mean (integer channels)")
        for k in ("mean", "invstd", "scale", "shift"):
            assert got[k].shape == (G, C)
            for idx, label in ((const, "constant channels"), (rest, "other channels")):
                if idx:
                    bounded(got[k][:, idx], want[k][:, idx], F32, "%s %s, %s" % (what, k, label))
        bounded(rm, want["rm"], F32, what + " running_mean")
        bounded(rv, want["rv"], F32, what + " running_var (unbiased)")
        if n > 1:
            # for information: what E[x^2] - mean^2 costs on the offset channel, against the variance of x itself in float64
            true_var = c["x"][..., E.FIN_OFFSET].var(1, unbiased=False)
            kvar = 1.0 / got["invstd"][:, E.FIN_OFFSET].double().cpu() ** 2 - float(torch.tensor(eps, dtype=F32))
            print("%s: offset channel, variance from the partials vs the float64 variance of x: %.3e relative (not a bound)"
                  % (what, float(((kvar - true_var).abs() / true_var).max())))
    # running_mean = None: the same statistics, nothing else written
    want = E.finalize_ref(c, 0.1, 1e-5)
    rv = full(C, SENTINEL)
    got = ops.bn_finalize(part, C, G, n, gamma, beta, None, rv, 0.1, 1e-5, None)
    bounded(got[0], want["mean"], F32, "finalize without running buffers: mean")
    for idx in (const, rest):
        if idx:
            bounded(got[1][:, idx], want["invstd"][:, idx], F32, "finalize without running buffers: invstd")
    assert bool((rv == SENTINEL).all())


# ---- 2. bn_eval_params ----
@pytest.mark.parametrize("C", [1, 63, 64, 65, 200])
def test_bn_eval_params(ops, C):
    """bn_eval_params_kernel: 64 threads per workgroup, C below / at / above one and several workgroups; a zero running variance"""
    g = E.gen(7, C)
    gamma, beta = E.bn_affine(C, g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.05
    rv[C // 2] = 0.0
    for eps in (1e-5, 1e-3):
        scale, shift = ops.bn_eval_params(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), eps)
        ws = gamma.double() / torch.sqrt(rv.double() + float(torch.tensor(eps, dtype=F32)))
        zero = torch.zeros(C, dtype=torch.bool)
        zero[C // 2] = True
        for idx, label in ((zero, "zero variance"), (~zero, "rest")):
            if bool(idx.any()):
                bounded(scale[0][idx], ws[idx], F32, "eval scale C=%d eps=%g %s" % (C, eps, label))
                bounded(shift[0][idx], (beta.double() - rm.double() * ws)[idx], F32, "eval shift C=%d eps=%g %s" % (C, eps, label))


# ---- 3. bn_apply ----
def check_apply(ops, dtype, C, G, P, combos):
    c = E.bn_apply_case(dtype, C, G, P)
    xd, rd = dev(c["x"].reshape(G * P, C), dtype), dev(c["res"].reshape(G * P, C), dtype)
    scale, shift = c["scale"].cuda(), c["shift"].cuda()
    for residual, relu, bits in combos:
        want = E.bn_apply_ref(c, residual, relu).reshape(G * P, C)
        what = "bn_apply %s C=%d (%s) G=%d P=%d res=%d relu=%d bits=%d" % (E.name(dtype), C, "hoisted" if E.hoisted(dtype, C) else "generic",
                                                                          G, P, residual, relu, bits)
        out = ops.bn_apply(xd, scale, shift, groups=G, act=ops.ACT_RELU if relu else ops.ACT_NONE, residual=rd if residual else None,
                           want_bits=bits)
        y, b = out if bits else (out, None)
        bounded(y, want, dtype, what, factor=1)
        if bits:
            assert b is not None and b.numel() == G * P * C // E.V[dtype]
            wb = E.pack_mask(y.reshape(-1) > 0, E.V[dtype])
            bad = int((b != wb).sum())
            print("%s: %d of %d mask bytes differ from (y > 0); %.1f %% of the bits set" % (what, bad, b.numel(), 100 * float((y > 0).float().mean())))
            assert bad == 0


APPLY_COMBOS = [(res, relu, bits) for res in (False, True) for relu, bits in ((False, False), (True, False), (True, True))]


@pytest.mark.parametrize("dtype,C", WIDTHS)
def test_bn_apply_hoisted_and_generic_widths(ops, dtype, C):
    """bn_apply_hoist_kernel (C = 32, 64) and bn_apply_kernel, the generic form ((256 V) % C != 0: C = 24, 48, 96), groups 1 / 2 / 4,
    one pixel per group and piece counts around one workgroup's 256 threads and 512 pieces, with / without residual, ReLU and mask bytes"""
    assert E.hoisted(dtype, C) == (C in (32, 64))
    for G in (1, 2, 4):
        for P in E.apply_pixel_counts(dtype, C):
            check_apply(ops, dtype, C, G, P, APPLY_COMBOS)


@pytest.mark.parametrize("dtype,C,G,npix", E.HOIST_LARGE + E.GENERIC_LARGE, ids=lambda v: E.name(v) if isinstance(v, torch.dtype) else str(v))
def test_bn_apply_past_one_grid_pass(ops, dtype, C, G, npix):
    """hoisted: more than 2 x 2048 x 256 pieces -- a full trip (two with groups = 2) of the two-pieces-in-flight loop, then the
    one-piece tail; generic (C = 48): more than 4096 x 256 pieces -- the grid-stride loop's second pass"""
    check_apply(ops, dtype, C, G, npix // G, [(False, False, False), (True, True, True)])


# ---- 4. bn_bwd, two-pass ----
def bwd_device_inputs(c, dtype):
    G, P, C = c["G"], c["P"], c["C"]
    flat = lambda t: dev(t.reshape(G * P, C), dtype)
    d = dict(x=flat(c["x"]), dout=flat(c["dout"]), out=flat(c["out"]), ms=c["ms"].cuda(), mh=c["mh"].cuda(), gamma=c["gamma"].cuda(),
             mean=c["mean"].cuda(), invstd=c["invstd"].cuda())
    d["bits"] = E.pack_mask(d["out"].reshape(-1) > 0, E.V[dtype])
    return d


def run_bwd(ops, d, mask, G, C, accumulate, want_dres):
    dg = full(C, DG0 if accumulate else SENTINEL)
    db = full(C, DB0 if accumulate else SENTINEL)
    out_relu = d["out"] if mask == "out_relu" else None
    kw = dict(mask_scale=d["ms"], mask_shift=d["mh"]) if mask == "mask_scale" else dict(bits=d["bits"]) if mask == "bits" else {}
    with ops.no_persist_bn():
        out = ops.bn_bwd(d["dout"], out_relu, d["x"], d["mean"], d["invstd"], d["gamma"], dg, db, groups=G, accumulate=accumulate,
                         want_dres=want_dres, **kw)
    dx, dres = out if want_dres else (out, None)
    return dx, dres, dg, db


def check_bwd(ops, dtype, C, G, P, variants, masks=E.MASKS):
    c = E.bn_bwd_case(dtype, C, G, P)
    d = bwd_device_inputs(c, dtype)
    for mask in masks:
        ref = E.bn_bwd_ref(c, mask)
        wdx, wdres = ref["dx"].reshape(G * P, C).cuda(), ref["dres"].reshape(G * P, C).cuda()
        for accumulate, want_dres in variants:
            what = "bn_bwd %s C=%d G=%d P=%d mask=%s acc=%d dres=%d" % (E.name(dtype), C, G, P, mask, accumulate, want_dres)
            dx, dres, dg, db = run_bwd(ops, d, mask, G, C, accumulate, want_dres)
            bounded(dx, wdx, dtype, what + " dx", factor=4)
            if want_dres:
                bounded(dres, wdres, dtype, what + " dres", factor=1)
            bounded(dg.double() - (DG0 if accumulate else 0.0), ref["dgamma"], dtype, what + " dgamma", factor=8)
            exact(db, ref["dbeta"] + (DB0 if accumulate else 0.0), what + " dbeta")


ALL_VARIANTS = list(itertools.product((False, True), (False, True)))


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("dtype,C", BWD_WIDTHS, ids=lambda v: E.name(v) if isinstance(v, torch.dtype) else str(v))
def test_bn_bwd_two_pass(ops, dtype, C, G):
    """bn_bwd_reduce_kernel<T, MASK 0..3> / bn_bwd_finalize_kernel / bn_bwd_apply_hoist_kernel<T, MASK 0..3> inside no_persist_bn():
    the narrowest widths (one vector column, rstep = 256) and the widest (256 columns, rstep = 1); 1 and 2 pixels per group (fewer
    pixels than the bpg = 1024 / G chunks), bpg - 1, bpg, bpg + 1 (chunk 1 -> 2: the two-pixel loop and its tail) and 1200; the four
    mask forms, with exact zeros in out_relu and in x * mask_scale + mask_shift; dres; accumulate both ways (sentinels overwritten).
    One and two pixels per group take x on a grid 256 times finer (_norm_cases.bn_bwd_case): on the coarse grid torch's own float32
    backward is 3.2e-3 of max |dx| from its float64 one at two pixels, on the fine grid 1.1e-7 (tests/test_norm_edges_cpu.py measures
    both), so the stated factor 4 (8e-5 in float32) is kept there too."""
    for P in E.bwd_pixel_counts(G):
        check_bwd(ops, dtype, C, G, P, ALL_VARIANTS)


def test_bn_bwd_apply_past_one_grid_pass(ops):
    """bn_bwd_apply_hoist_kernel at C = 64 fp32, groups = 2, 65548 pixels: 524,384 pieces per group of 1024 workgroups -- a full trip
    of the two-pieces-in-flight loop and the one-piece tail; the reduction's chunks are 33 pixels (rstep = 16: loop, loop, tail)"""
    dtype, C, G, npix = E.BWD_LARGE
    check_bwd(ops, dtype, C, G, npix // G, [(False, True)])


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("dtype,C", [(dt, C) for dt in E.DTYPES for C in (48, 64)], ids=lambda v: E.name(v) if isinstance(v, torch.dtype) else str(v))
def test_bn_bwd_from_partials(ops, dtype, C, G):
    """dh_bn_bwd_from_partials: bn_bwd_finalize_kernel over synthesised per-tile partials (1 and 65 tiles per group: one lane, and a
    second trip of its 64-lane loop), then bn_bwd_apply_kernel -- the GENERIC form at C = 48, which dh_bn_bwd cannot reach -- or the
    hoisted one at C = 64"""
    assert E.hoisted(dtype, C) == (C == 64)
    for tpg in (1, 65):
        c = E.bn_bwd_partials_case(dtype, C, G, tpg)
        P = c["P"]
        d = bwd_device_inputs(c, dtype)
        wdx, wdg, wdb = c["ref"]
        for accumulate in (False, True):
            what = "bn_bwd_from_partials %s C=%d G=%d tiles=%d P=%d acc=%d" % (E.name(dtype), C, G, tpg, P, accumulate)
            dg, db = full(C, DG0 if accumulate else SENTINEL), full(C, DB0 if accumulate else SENTINEL)
            dx = ops.bn_bwd_from_partials(d["dout"], d["x"], c["partial"].cuda(), d["mean"], d["invstd"], d["gamma"], dg, db, groups=G,
                                          accumulate=accumulate)
            bounded(dx, wdx.reshape(G * P, C), dtype, what + " dx", factor=4)
            bounded(dg.double() - (DG0 if accumulate else 0.0), wdg, dtype, what + " dgamma", factor=8)
            exact(db, wdb + (DB0 if accumulate else 0.0), what + " dbeta")


# ---- 6. LayerNorm ----
def ln_split(c):
    keep = E.split_rows(c["rows"], c["special"])
    return [(keep, "ordinary rows")] + ([(~keep, "constant and offset rows")] if c["special"] else [])


@pytest.mark.parametrize("rows", E.LN_ROWS)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=E.name)
def test_layernorm_forward(ops, dtype, rows):
    """ln_fwd_kernel: 8 lanes per row, so 1, 7, 33 and 1001 rows end in a partly filled wavefront (the shuffles of its idle lanes);
    49189 rows = 1538 workgroups; a constant row (rstd = 1 / sqrt(eps)), rows with mean = 100 std, eps 1e-5 / 1e-3, with and without
    the saved statistics, which are checked against the float64 mean and rstd"""
    c = E.ln_case(dtype, rows)
    xd, gamma, beta = dev(c["x"], dtype), c["gamma"].cuda(), c["beta"].cuda()
    for eps in (1e-5, 1e-3):
        wy, wst = E.ln_fwd_ref(c, eps)
        y, st = ops.layernorm(xd, gamma, beta, eps)
        y2 = ops.layernorm(xd, gamma, beta, eps, want_stats=False)
        assert torch.equal(y, y2)
        for idx, label in ln_split(c):
            what = "layernorm %s rows=%d eps=%g %s" % (E.name(dtype), rows, eps, label)
            bounded(y[idx.cuda()], wy[idx], dtype, what + " y", factor=1)
            bounded(st[idx.cuda(), 0], wst[idx, 0], F32, what + " saved mean", factor=1)
            bounded(st[idx.cuda(), 1], wst[idx, 1], F32, what + " saved rstd", factor=1)


@pytest.mark.parametrize("rows", E.LN_ROWS)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=E.name)
def test_layernorm_backward(ops, dtype, rows):
    """ln_bwd_kernel: groups of 32 rows, at most 512 workgroups -- 49189 rows = three strides of its grid-stride loop plus a partial
    group, 1 / 7 / 33 / 1001 rows a partial group; statistics given in float64-then-float32; dx_add present and absent; accumulate both
    ways with sentinels; integer dy, so dbeta is exact"""
    c = E.ln_case(dtype, rows)
    xd, dyd, extra, gamma = dev(c["x"], dtype), dev(c["dy"], dtype), dev(c["extra"], dtype), c["gamma"].cuda()
    for eps in (1e-5, 1e-3):
        st = E.ln_stats(c["x"], eps).float()
        wdx, wdg, wdb = E.ln_bwd_formula(c["x"], c["dy"], st.double(), c["gamma"].double())
        for add, accumulate in ALL_VARIANTS:
            what = "layernorm_bwd %s rows=%d eps=%g dx_add=%d acc=%d" % (E.name(dtype), rows, eps, add, accumulate)
            dg, db = full(32, DG0 if accumulate else SENTINEL), full(32, DB0 if accumulate else SENTINEL)
            dx = ops.layernorm_bwd(dyd, xd, st.cuda(), gamma, dg, db, dx_add=extra if add else None, accumulate=accumulate)
            want = wdx + c["extra"] if add else wdx
            for idx, label in ln_split(c):
                bounded(dx[idx.cuda()], want[idx], dtype, "%s dx, %s" % (what, label), factor=3)
            bounded(dg.double() - (DG0 if accumulate else 0.0), wdg, dtype, what + " dgamma", factor=8)
            exact(db, wdb + (DB0 if accumulate else 0.0), what + " dbeta")


@pytest.mark.parametrize("dtype", E.DTYPES, ids=E.name)
def test_layernorm_of_no_rows_touches_nothing(ops, dtype):
    x = torch.empty(0, 32, dtype=dtype, device="cuda")
    gamma, beta = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
    y, st = ops.layernorm(x, gamma, beta)
    assert y.shape == (0, 32) and st.shape == (0, 2)
    dg, db = full(32, SENTINEL), full(32, SENTINEL)
    dx = ops.layernorm_bwd(x, x, st, gamma, dg, db, accumulate=False)
    torch.cuda.synchronize()
    assert dx.shape == (0, 32) and bool((dg == SENTINEL).all()) and bool((db == SENTINEL).all())


# ---- 7. reduce_partials ----
@pytest.mark.parametrize("nt", E.RED_NT)
def test_reduce_partials(ops, nt):
    """reduce_partials_kernel through ops.reduce_rows: 8 row phases, the 4-way unrolled loop (`t + 24 < nt`, step 32: first entered at
    nt = 25 + phase) and its 8-step tail; n below / at / above one workgroup's 32 outputs.  Integers are exact at scale = 1; at
    scale = 0.37 the float64 sum is rounded once (twice with accumulate): 2^-23 of max(|want|, |out before|), element by element."""
    for n in E.RED_N:
        rows, before = E.reduce_case(nt, n)
        pd = rows.float().cuda()
        for scale, accumulate in itertools.product((1.0, 0.37), (False, True)):
            out = before.float().cuda() if accumulate else full(n, SENTINEL)
            ops.reduce_rows(pd, nt, n, out, accumulate=accumulate, scale=scale)
            want = rows.sum(0) * float(torch.tensor(scale, dtype=F32)) + (before if accumulate else 0.0)
            what = "reduce_partials nt=%d n=%d scale=%g acc=%d" % (nt, n, scale, accumulate)
            if scale == 1.0:
                exact(out, want, what)
            else:
                got = out.double().cpu()
                assert bool(torch.isfinite(got).all())
                lim = 2.0 ** -23 * torch.maximum(want.abs(), before.abs() if accumulate else torch.zeros_like(want))
                worst = float(((got - want).abs() / lim.clamp(min=1e-30)).max())
                print("%s: worst |err| / (2^-23 max(|want|, |before|)) = %.3f" % (what, worst))
                assert bool(((got - want).abs() <= lim).all()), what


# ---- 8. colsum ----
@pytest.mark.parametrize("C", E.COLSUM_C)
@pytest.mark.parametrize("dtype", E.DTYPES, ids=E.name)
def test_colsum(ops, dtype, C):
    """colsum_partial_kernel + reduce_partials: the 16-byte form (four row streams and their tail) and the scalar form of each dtype,
    idle lanes where 256 % C != 0, a single row phase at C = 129 / 200, 1 .. 20001 rows (fewer rows than workgroups, and 64 .. 256
    workgroups); accumulate both ways.  Integers: exact."""
    for P in E.COLSUM_P:
        x, before = E.colsum_case(dtype, C, P)
        xd = dev(x, dtype)
        for accumulate in (False, True):
            out = before.float().cuda() if accumulate else full(C, SENTINEL)
            ops.colsum(xd, out, accumulate=accumulate)
            exact(out, x.sum(0) + (before if accumulate else 0.0),
                  "colsum %s C=%d (%s) P=%d acc=%d" % (E.name(dtype), C, "vector" if E.colsum_vector_form(dtype, C) else "scalar", P, accumulate))
