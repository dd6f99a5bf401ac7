"""What tests/test_wgrad_exact_gpu.py and tests/test_wgrad_exact_cpu.py share: the case table of the weight gradient
(csrc/conv_wgrad.hip), the seeded integer inputs, the float64 references and the comparator.

The weight gradient is a sum of products over pixels.  x and dy are integers in [-3, 3]: exact in bf16, in fp32 and in the two
planes of the split fp32 form (the low plane is 0), every product at most 9 and every sum far below 2^24 -- so the result is exact
in fp32 in ANY summation order, whatever the tiling, the split-K factor and the order of the reduce, and the kernel must equal the
float64 reference bit for bit (`exact`, torch.equal).  One dropped, doubled or misplaced pixel changes an integer.

A BatchNorm-on-load input takes scale from {-1, 0.5, 1, 2} and an integer shift in [-2, 2]: relu(x * scale + shift) is a multiple
of 0.5 up to 8, exact in bf16, and the sums are multiples of 0.5 below 2^23.

Each case states the row dh_conv2d_wgrad_describe must report for it -- (family, co tile, ci channels per workgroup, ci wave
groups, split-K) -- its pixel tiles (8 rows x 16 columns) and the edges it exists for; tests/test_wgrad_exact_cpu.py asserts the
row and recomputes every edge from it on the host, so a change of the plan turns that test red instead of moving a GPU case onto
another branch.  The shapes are the smallest the plan grants the wanted row: split-K is min(ceil(target / slabs), tiles / 8, 1024)
(wg_splitk_estimate), so 9 slices need 72 tiles -- 13 images of 20 x 24 pixels are 78 tiles of which the last row has 4 rows and
the last column 8 columns, 6 tiles per image, slices of 9 or 8 tiles and a carry in the (image, ty, tx) counter at every step."""
import collections
import ctypes
import functools
import zlib

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
W1, WS, WS_BATCH, C32_BATCH, GENERIC, PHASE = range(6)      # the kernel families of dh_conv2d_wgrad_describe
FAMILIES = ("W1", "WS", "WS_BATCH", "C32_BATCH", "GENERIC", "PHASE")
TH, TW = 8, 16                            # conv_wgrad.hip: the pixel tile
W1_CHUNK = 64                             # conv_wgrad.hip W1_PS: wgrad1x1_kernel walks flat chunks of 64 pixels
IMAX = 3                                  # |integer data| <= 3
EXACT_LIMIT = 1 << 24                     # integers up to here are exact in float32
ACC_FILL, SENTINEL = 3.0, 777.0           # what accumulate=True starts from (an integer: stays exact) / accumulate=False must overwrite

# (name, dtype, dh_set_f32_mma_mode, use_tr): the four precisions of conv_wgrad_kernel
PRECS = (("bf16-tr", BF16, 0, True), ("bf16-notr", BF16, 0, False), ("f32", F32, 0, True), ("f32x3", F32, 1, True))

Case = collections.namedtuple("Case", [
    "name", "group",                      # group: GENERIC / WS / BATCH / W1 / PHASE -- one parametrised GPU test each
    "row",                                # (family, co tile, ci channels per workgroup, ci wave groups, split-K) of describe
    "tiles",                              # pixel tiles of one weight group
    "edges",                              # names in EDGES: what the case exists for, recomputed from the described row
    "N", "H", "W", "Cin", "Cout",         # x [N, H, W, pitch or Cin]; dW [Cout, Cin, ks, ks]
    "ks", "stride", "dil",
    "form",                               # plain / bn (BnInput) / split (SplitCat) / pergroup (groups == N) / phase (conv_up2_wgrad)
    "prec",                               # index into PRECS
    "dy_ch",                              # channels of dy when it is padded past Cout (cout_real = Cout), else 0
    "pitch",                              # channel pitch of x when wider than Cin (cin = Cin), else 0
    "bn_groups",                          # statistics groups of a BnInput
    "batch",                              # described (and run) inside an open batch
    "batch_row",                          # (family, split-K) the same layer gets inside an open batch; None: no batched form
], defaults=[3, 1, 1, "plain", 0, 0, 0, 0, False, None])


def dtype_of(c):
    return PRECS[c.prec][1]


def mma_of(c):
    return PRECS[c.prec][2]


def tr_of(c):
    return PRECS[c.prec][3]


def pad_of(c):
    return {1: 0, 2: 1, 3: c.dil, 4: 2}[c.ks]


def out_hw(c):
    """the dy grid: the phase form's COARSE grid (dy itself is [N, 2 H, 2 W, 32]); the 4x4 stem form keeps H x W"""
    if c.ks in (2, 4):
        return c.H, c.W
    p, d = pad_of(c), c.dil * (c.ks - 1)
    return (c.H + 2 * p - d - 1) // c.stride + 1, (c.W + 2 * p - d - 1) // c.stride + 1


def tile_grid(c):
    oh, ow = out_hw(c)
    return -(-oh // TH), -(-ow // TW)


def weight_groups(c):
    return c.N if c.form == "pergroup" else 1


def tiles_of(c):
    ty, tx = tile_grid(c)
    return c.N // weight_groups(c) * ty * tx


def dw_shape(c):
    return (c.N, c.Cout, c.Cin) if c.form == "pergroup" else (c.Cout, c.Cin, 3, 3) if c.ks == 2 else (c.Cout, c.Cin, c.ks, c.ks)


def describe(lib, c, batch=None):
    """dh_conv2d_wgrad_describe's row [family, ct, it, cig, ci_tiles, splitk, direct, grid x, y, z, threads, lds] for the launch
    ops.conv2d_wgrad (phase: ops.conv_up2_wgrad) makes of this case.  Host only."""
    out = (ctypes.c_int * 12)()
    oh, ow = out_hw(c)
    prev = lib.dh_get_f32_mma_mode()
    lib.dh_set_f32_mma_mode(mma_of(c))
    try:
        rc = lib.dh_conv2d_wgrad_describe(int(dtype_of(c) == BF16), 0, c.N, c.H, c.W, c.Cin, oh, ow, c.dy_ch or c.Cout, c.ks, c.stride,
                                          pad_of(c), weight_groups(c), 0, int(tr_of(c)), c.Cout if c.dy_ch else 0, c.pitch, c.dil,
                                          c.bn_groups, int(c.form == "bn"), int(c.form == "split"),
                                          int(c.batch if batch is None else batch), out)
    finally:
        lib.dh_set_f32_mma_mode(prev)
    assert rc == 0, (c.name, rc)
    return list(out)


def instantiation(c, row):
    """the conv_wgrad_kernel instantiation behind a GENERIC / PHASE row: (ks, stride, dilation, co tile, ci channels per workgroup,
    ci wave groups, precision) -- launch_generic's ladder is keyed by exactly these"""
    return (c.ks, c.stride, c.dil, row[1], row[2], row[3], PRECS[c.prec][0])


def reachable_instantiations():
    """every instantiation launch_generic can reach, written out from wg_tiles / launch / launch_ct: the co tile follows Cout
    (16 / 32 / 64); 3x3 stride 1 takes 32 ci channels, or 64 in two wave groups beside a 64-wide co tile; 3x3 stride 2 and 1x1
    stride 2 take 32; 1x1 stride 1 takes 32, 64 (Cin > 32) or 128 in two wave groups (Cin % 128 == 0, 64-wide co tile); the 4x4
    stem form takes 16; the 2x2 phase form has 32 output channels and 32 ci channels; each in four precisions"""
    out = set()
    for prec in PRECS:
        p = prec[0]
        for ct in (16, 32, 64):
            out |= {(3, 1, 1, ct, 32, 1, p), (3, 1, 2, ct, 32, 1, p), (3, 2, 1, ct, 32, 1, p), (1, 1, 1, ct, 32, 1, p),
                    (1, 1, 1, ct, 64, 1, p), (1, 2, 1, ct, 32, 1, p), (4, 1, 1, ct, 16, 1, p)}
        out |= {(3, 1, 1, 64, 64, 2, p), (3, 1, 2, 64, 64, 2, p), (1, 1, 1, 64, 128, 2, p), (2, 1, 1, 32, 32, 1, p)}
    return out


# ---- the edges, recomputed from the described row r (12 ints) ----
def _nbx(r):
    return r[7]


def _chunks(c):
    oh, ow = out_hw(c)
    return -(-c.N * oh * ow // W1_CHUNK)


EDGES = {
    # the tile walk
    "uneven": lambda c, r: r[5] > 1 and tiles_of(c) % r[5] != 0,                       # my_tiles differs between slices
    "carry": lambda c, r: r[5] % (tile_grid(c)[0] * tile_grid(c)[1]) != 0 and tile_grid(c)[0] * tile_grid(c)[1] > 1,   # drem != 0
    "ragged_rows": lambda c, r: out_hw(c)[0] % TH != 0,
    "ragged_cols": lambda c, r: out_hw(c)[1] % TW != 0,
    "remap": lambda c, r: _nbx(r) > 1 and r[5] % 8 == 0,                               # the XCD remap runs
    "no_remap": lambda c, r: not (_nbx(r) > 1 and r[5] % 8 == 0),
    "few_tiles": lambda c, r: tiles_of(c) < 8 and r[5] == 1,
    "tiles16": lambda c, r: tiles_of(c) == 16 and r[5] == 2,
    "one_slab": lambda c, r: r[5] == 1 and r[6] != 0,                                  # the direct form: no slab, no reduce
    "per_image": lambda c, r: r[9] == c.N and c.N > 1,                                 # grid z = weight groups
    # channels
    "ragged_ci": lambda c, r: c.Cin % r[2] != 0,
    "ragged_co": lambda c, r: c.Cout % r[1] != 0,
    "ci_tiles": lambda c, r: r[4] > 1,
    "cout_pad": lambda c, r: c.dy_ch > c.Cout,
    "pitch": lambda c, r: c.pitch > c.Cin,
    "unaligned": lambda c, r: (c.Cin * dtype_of(c).itemsize) % 16 != 0 and (c.Cout * dtype_of(c).itemsize) % 16 != 0,   # element loads
    "x3_half_piece": lambda c, r: PRECS[c.prec][0] == "f32x3" and c.Cin % 8 == 4,     # the zero-filled half of an 8-channel piece
    # geometry
    "odd_input": lambda c, r: c.stride == 2 and c.H % 2 == 1 and c.W % 2 == 1,
    "even_input": lambda c, r: c.stride == 2 and c.H % 2 == 0 and c.W % 2 == 0,
    "halo_past_map": lambda c, r: c.dil == 2 and c.H <= TH and c.W <= TH,              # dilation reaches past a whole map edge
    "bn_groups": lambda c, r: c.form == "bn" and c.bn_groups >= 2 and c.N % c.bn_groups == 0,
    "split_input": lambda c, r: c.form == "split" and c.Cin % 128 == 0,
    # wgrad1x1_kernel
    "ragged_chunk": lambda c, r: (c.N * out_hw(c)[0] * out_hw(c)[1]) % W1_CHUNK != 0,
    "chunks_uneven": lambda c, r: _chunks(c) % r[5] != 0,
    "w1_threshold": lambda c, r: r[0] == W1 and _nbx(r) * r[5] >= 256 and _nbx(r) * (r[5] - 1) < 256,
    "below_w1": lambda c, r: r[0] == GENERIC and c.ks == 1 and 9 * r[5] < 256 <= 9 * (r[5] + 1),   # 9 blocks of 256 x 128 would be 4 short
    # the batch
    "batch_round8": lambda c, r: tiles_of(c) // 32 >= 8 and r[5] % 8 == 0 and tiles_of(c) % r[5] != 0,
    "one_slice": lambda c, r: tiles_of(c) < 32 and r[5] == 1,
    "refused": lambda c, r: c.batch and r[0] == GENERIC,
}


# ---- the table ----
BASE = dict(N=13, H=20, W=24)            # 78 tiles, 6 per image, the last tile row 4 rows, the last tile column 8 columns
WALK = ("uneven", "carry", "ragged_rows", "ragged_cols")


def _sweep():
    """one case per reachable instantiation, all at 78 tiles and split-K 9 (stride 2: 39 x 47 inputs, the same 20 x 24 dy grid)"""
    shapes = []          # (ks, stride, dil, ct, it, cig, Cin, extra fields)
    for ct in (16, 32, 64):
        for dil in (1, 2):
            shapes.append((3, 1, dil, ct, 32, 1, 48 if ct == 64 else 32, {}))           # 48: two ci tiles, the second half empty
        shapes.append((3, 2, 1, ct, 32, 1, {16: 32, 32: 48, 64: 64}[ct], dict(H=39, W=47)))
        shapes.append((1, 1, 1, ct, 32, 1, 32, {}))
        shapes.append((1, 1, 1, ct, 64, 1, 80, {}))                                      # two ci tiles, 16 channels in the second
        shapes.append((1, 2, 1, ct, 32, 1, 64, dict(H=39, W=47)))
        shapes.append((4, 1, 1, ct, 16, 1, 16, dict(pitch=32)))                          # the stem: 16 channels of a 32-channel pitch
    for dil in (1, 2):
        shapes.append((3, 1, dil, 64, 64, 2, 96, {}))        # (Cin = 64 in bf16 with transpose reads is the wave-specialised family)
    shapes.append((1, 1, 1, 64, 128, 2, 128, {}))
    out = []
    for ks, stride, dil, ct, it, cig, cin, extra in shapes:
        for pi, prec in enumerate(PRECS):
            f = dict(BASE, Cin=cin, Cout=ct, ks=ks, stride=stride, dil=dil, prec=pi)
            f.update(extra)
            edges = WALK + (("odd_input",) if stride == 2 else ()) + (("ci_tiles",) if cin > it else ()) + \
                (("ragged_ci",) if cin % it else ()) + (("pitch",) if "pitch" in extra else ())
            if (ks, stride, dil, ct, pi) == (3, 1, 1, 32, 0):      # what the batch's 32-wide family takes: 78 / 32 = 2 slices
                f["batch_row"] = (C32_BATCH, 2)
            out.append(Case("k%ds%dd%d-co%d-ci%dx%d-%s" % (ks, stride, dil, ct, it // cig, cig, prec[0]), "GENERIC",
                            (GENERIC, ct, it, cig, 9), 78, edges, **f))
    return out


def _each_prec(name, group, row, tiles, edges, precs=(0, 1, 2, 3), c32=None, **f):
    """c32: the split-K of the layer inside an open batch where C32_BATCH takes it (bf16 with transpose reads only)"""
    return [Case("%s-%s" % (name, PRECS[p][0]), group, row, tiles, edges, prec=p,
                 batch_row=(C32_BATCH, c32) if c32 and p == 0 else None, **f) for p in precs]


def _generic():
    g = "GENERIC"
    out = _sweep()
    # 3x3 stride 2 on an even input (the sweep's are odd); 1x1 stride 2 alike
    out += _each_prec("k3s2-even", g, (GENERIC, 32, 32, 1, 9), 78, WALK + ("even_input",), (0, 2), N=13, H=40, W=48, Cin=32, Cout=32, stride=2)
    out += _each_prec("k1s2-even", g, (GENERIC, 64, 32, 1, 9), 78, WALK + ("even_input", "ci_tiles"), (0, 3), N=13, H=40, W=48, Cin=64,
                      Cout=64, ks=1, stride=2)
    # dilation 2 on 8 x 8 maps: one tile per image, the halo reaches past every edge of the map; 17 images in slices of 9 and 8
    out += _each_prec("k3d2-8x8", g, (GENERIC, 32, 32, 1, 2), 17, ("uneven", "halo_past_map"), N=17, H=8, W=8, Cin=32, Cout=32, dil=2)
    # two real output channels inside one 16-byte piece of dy (the class head)
    out += _each_prec("cout2-in-8", g, (GENERIC, 16, 32, 1, 9), 78, WALK + ("cout_pad", "ragged_co"), (0, 1), Cin=32, Cout=2, dy_ch=8, **BASE)
    out += _each_prec("cout2-in-4", g, (GENERIC, 16, 32, 1, 9), 78, WALK + ("cout_pad", "ragged_co"), (2, 3), Cin=32, Cout=2, dy_ch=4, **BASE)
    # Cin = 64 in the 512-thread form (two ci wave groups): what the wave-specialised family leaves to conv_wgrad_kernel
    out += _each_prec("cin64-cig2", g, (GENERIC, 64, 64, 2, 9), 78, WALK, (1, 2, 3), Cin=64, Cout=64, **BASE)
    # a channel pitch wider than Cin (bf16 with transpose reads at 64 -> 64: the pitch keeps it off the wave-specialised family)
    out += _each_prec("pitch48", g, (GENERIC, 32, 32, 1, 9), 78, WALK + ("pitch",), (0, 2), c32=2, Cin=32, Cout=32, pitch=48, **BASE)
    out += _each_prec("pitch96-cig2", g, (GENERIC, 64, 64, 2, 9), 78, WALK + ("pitch",), (0,), Cin=64, Cout=64, pitch=96, **BASE)
    # ragged channel tiles: 72 = 64 + 8 output channels, 36 = 32 + 4 input channels (f32x3: the half past a Cin % 8 == 4 tail)
    out += _each_prec("co72-ci48", g, (GENERIC, 64, 32, 1, 9), 78, WALK + ("ragged_co", "ragged_ci", "ci_tiles"), (0, 1), Cin=48, Cout=72, **BASE)
    out += _each_prec("co20-ci36", g, (GENERIC, 32, 32, 1, 9), 78, WALK + ("ragged_co", "ragged_ci", "ci_tiles"), (2,), Cin=36, Cout=20, **BASE)
    out += _each_prec("co20-ci36", g, (GENERIC, 32, 32, 1, 9), 78, WALK + ("ragged_co", "ragged_ci", "x3_half_piece"), (3,), Cin=36, Cout=20, **BASE)
    # bf16 channel counts that are no multiple of a 16-byte piece: element loads (the path without the branch-free fetch)
    out += _each_prec("co20-ci36", g, (GENERIC, 32, 32, 1, 9), 78, WALK + ("unaligned", "ragged_co", "ragged_ci"), (0, 1), c32=2, Cin=36, Cout=20, **BASE)
    # BatchNorm on load in conv_wgrad_kernel, two statistics groups
    out += _each_prec("bn2", g, (GENERIC, 32, 32, 1, 10), 84, ("uneven", "carry", "bn_groups"), c32=2, N=14, H=20, W=24, Cin=32, Cout=32,
                      form="bn", bn_groups=2)
    # 1x1: one slab, written straight into dW (assign and accumulate); per-image weights with and without a split
    out += _each_prec("k1-direct", g, (GENERIC, 64, 64, 1, 1), 12, ("one_slab",), (0, 2, 3), N=2, H=20, W=24, Cin=64, Cout=64, ks=1)
    out += _each_prec("k1-per-image", g, (GENERIC, 32, 32, 1, 2), 21, ("uneven", "per_image"), (0, 2), N=4, H=56, W=48, Cin=32, Cout=32,
                      ks=1, form="pergroup")
    out += _each_prec("k1-per-image-direct", g, (GENERIC, 32, 64, 1, 1), 6, ("one_slab", "per_image"), (0, 2), N=3, H=20, W=24, Cin=64,
                      Cout=32, ks=1, form="pergroup")
    # fewer than 8 tiles (one slice walks them all); exactly 16 tiles (two slices, 4 tiles per image)
    out += _each_prec("6-tiles", g, (GENERIC, 32, 32, 1, 1), 6, ("few_tiles", "ragged_rows", "ragged_cols"), (0, 2), c32=1, N=1, H=20, W=24, Cin=32, Cout=32)
    out += _each_prec("16-tiles", g, (GENERIC, 32, 32, 1, 2), 16, ("tiles16", "carry"), (0, 2), c32=1, N=4, H=16, W=32, Cin=32, Cout=32)
    return out


def _ws():
    g, r = "WS", lambda sk: (WS, 64, 64, 1, sk)
    return [
        Case("64x64", g, r(9), 78, WALK + ("no_remap",), Cin=64, Cout=64, batch_row=(WS_BATCH, 2), **BASE),
        Case("128x64-remap", g, r(8), 66, ("uneven", "carry", "remap", "ci_tiles"), N=11, H=24, W=24, Cin=128, Cout=64, batch_row=(WS_BATCH, 2)),
        Case("64x64-dil2", g, r(9), 78, WALK + ("no_remap",), Cin=64, Cout=64, dil=2, **BASE),
        Case("128x64-dil2-remap", g, r(8), 66, ("uneven", "carry", "remap"), N=11, H=24, W=24, Cin=128, Cout=64, dil=2),
        Case("64x64-bn2", g, r(10), 84, ("uneven", "carry", "bn_groups", "ragged_rows", "ragged_cols"), N=14, H=20, W=24, Cin=64, Cout=64,
             form="bn", bn_groups=2, batch_row=(WS_BATCH, 2)),
        Case("split-2x64", g, r(9), 78, WALK + ("split_input", "no_remap"), Cin=128, Cout=64, form="split", batch_row=(WS_BATCH, 2), **BASE),
        Case("split-2x64-remap", g, r(8), 66, ("uneven", "remap", "split_input"), N=11, H=24, W=24, Cin=128, Cout=64, form="split",
             batch_row=(WS_BATCH, 2)),
    ]


def _batch():
    """the layers of ONE recorded pass (ops.WgradPlan(device, batch=True)), in recording order"""
    g = "BATCH"
    return [
        Case("ws-300-tiles", g, (WS_BATCH, 64, 64, 1, 8), 300, ("batch_round8", "uneven", "carry", "no_remap"), N=50, H=20, W=24, Cin=64,
             Cout=64, batch=True),                                         # 300 / 32 = 9 -> 8 slices of 38 or 37 tiles
        Case("ws-18-tiles", g, (WS_BATCH, 64, 64, 1, 1), 18, ("one_slice",), N=3, H=20, W=24, Cin=64, Cout=64, batch=True),
        Case("ws-two-blocks", g, (WS_BATCH, 64, 64, 1, 8), 270, ("batch_round8", "remap", "uneven"), N=45, H=24, W=24, Cin=128, Cout=64,
             batch=True),
        Case("c32-300-tiles", g, (C32_BATCH, 32, 32, 1, 8), 300, ("batch_round8", "uneven", "carry"), N=50, H=20, W=24, Cin=32, Cout=32,
             batch=True),
        Case("c32-64to32-bn2", g, (C32_BATCH, 32, 32, 1, 8), 300, ("batch_round8", "remap", "bn_groups", "ci_tiles"), N=50, H=20, W=24,
             Cin=64, Cout=32, form="bn", bn_groups=2, batch=True),
        Case("c32-18-tiles", g, (C32_BATCH, 32, 32, 1, 1), 18, ("one_slice",), N=3, H=20, W=24, Cin=32, Cout=32, batch=True),
        Case("ws-split-2x64", g, (WS_BATCH, 64, 64, 1, 2), 78, ("split_input", "carry"), Cin=128, Cout=64, form="split", batch=True, **BASE),
        Case("16-out-refused", g, (GENERIC, 16, 32, 1, 37), 300, ("refused", "uneven", "carry"), N=50, H=20, W=24, Cin=32, Cout=16, batch=True),
    ]


def _w1():
    """wgrad1x1_kernel takes a 1x1 bf16 layer where its 256 x 128 blocks times the split fill 256 workgroups: 264 -> 520 channels are
    3 x 3 = 9 ragged blocks (520 = 2 x 256 + 8, 264 = 2 x 128 + 8), so the split must reach 29 -- 232 tiles.  31 x 31 pixels are 8
    tiles per image and 961 pixels: 29 images are 27,869 pixels = 435 chunks of 64 and one of 29"""
    g = "W1"
    return [
        Case("264x520-n29", g, (W1, 256, 128, 1, 29), 232, ("w1_threshold", "ragged_chunk", "chunks_uneven", "ragged_ci", "ragged_co", "no_remap"),
             N=29, H=31, W=31, Cin=264, Cout=520, ks=1),
        Case("264x520-n32-remap", g, (W1, 256, 128, 1, 32), 256, ("ragged_chunk", "chunks_uneven", "remap"), N=32, H=31, W=31, Cin=264,
             Cout=520, ks=1),
        Case("264x520-stride2", g, (W1, 256, 128, 1, 29), 232, ("w1_threshold", "ragged_chunk", "chunks_uneven", "odd_input"), N=29, H=61,
             W=61, Cin=264, Cout=520, ks=1, stride=2),
        Case("264x520-n28-generic", g, (GENERIC, 64, 64, 1, 28), 224, ("below_w1", "ragged_ci", "ragged_co", "ci_tiles"), N=28, H=31, W=31,
             Cin=264, Cout=520, ks=1),
    ]


def _phase():
    g = "PHASE"
    out = _each_prec("up2-32", g, (PHASE, 32, 32, 1, 9), 78, WALK, Cin=32, Cout=32, ks=2, form="phase", **BASE)
    out += _each_prec("up2-64", g, (PHASE, 32, 32, 1, 9), 78, WALK + ("ci_tiles",), Cin=64, Cout=32, ks=2, form="phase", **BASE)
    return out


CASES = _generic() + _ws() + _batch() + _w1() + _phase()
assert len({(c.group, c.name) for c in CASES}) == len(CASES)


def cases(group):
    return [c for c in CASES if c.group == group]


def ids(cs):
    return [c.name for c in cs]


# ---- the integer generator ----
def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def ints(shape, g, bound=IMAX):
    """integer-valued float32, uniform on [-bound, bound]"""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=g, dtype=torch.int8 if bound < 128 else torch.int32).float()


def _data_key(c):
    return (c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.dil, c.form, c.dy_ch, c.pitch, c.bn_groups)


@functools.lru_cache(maxsize=4)
def _data(key):
    N, H, W, Cin, Cout, ks, stride, dil, form, dy_ch, pitch, bn_groups = key
    c = Case("", "", None, 0, (), N, H, W, Cin, Cout, ks, stride, dil, form, 0, dy_ch, pitch, bn_groups)
    g = gen(*key)
    oh, ow = out_hw(c)
    d = {}
    if form == "split":          # the two halves of one [2 N, H, W, Cin / 2] tensor
        d["x"] = ints((2 * N, H, W, Cin // 2), g)
    else:                        # NHWC at the channel pitch: the channels past Cin hold integers too and must never be read
        d["x"] = ints((N, H, W, pitch or Cin), g)
    fine = 2 if form == "phase" else 1
    d["dy"] = ints((N, fine * oh, fine * ow, dy_ch or Cout), g)          # the channels past Cout alike
    if form == "bn":
        d["scale"] = torch.tensor([-1.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (bn_groups, Cin), generator=g)]
        d["shift"] = ints((bn_groups, Cin), g, 2)
    return d


def data(c):
    """the seeded inputs of a case, float32 on the CPU: x, dy (NHWC) and, for a BnInput, scale / shift [groups, Cin].  Shared by
    the precisions of a shape; treat as read-only"""
    return _data(_data_key(c))


# ---- the float64 reference ----
def effective_input(c, d, dtype=torch.float64):
    """NCHW `dtype`: the tensor the gradient is taken against"""
    x = d["x"].to(dtype)
    if c.form == "split":
        x = torch.cat([x[:c.N], x[c.N:]], 3)
    x = x[..., :c.Cin]
    if c.form == "bn":
        per = c.N // c.bn_groups
        grp = torch.arange(c.N) // per
        x = torch.relu(x * d["scale"].to(dtype)[grp][:, None, None, :] + d["shift"].to(dtype)[grp][:, None, None, :])
    return x.permute(0, 3, 1, 2).contiguous()


def last_tile_mask(c):
    """[N, dy rows, dy columns] bool: the pixels of the last pixel tile (last image, last tile row, last tile column)"""
    oh, ow = out_hw(c)
    ty, tx = tile_grid(c)
    fine = 2 if c.form == "phase" else 1
    m = torch.zeros(c.N, fine * oh, fine * ow, dtype=torch.bool)
    m[c.N - 1, fine * (ty - 1) * TH:, fine * (tx - 1) * TW:] = True
    return m


def reference_of(c, d, dtype=torch.float64, drop_last_tile=False):
    """dW in `dtype` from the inputs `d`: torch.nn.grad.conv2d_weight (per image: one matrix product each)"""
    x = effective_input(c, d, dtype)
    dy = d["dy"].to(dtype)[..., :c.Cout]
    if drop_last_tile:
        dy = dy * (~last_tile_mask(c))[..., None].to(dtype)
    dy = dy.permute(0, 3, 1, 2).contiguous()
    if c.form == "pergroup":
        assert c.ks == 1 and c.stride == 1
        return torch.einsum("nohw,nihw->noi", dy, x)
    if c.form == "phase":        # conv2d(interpolate(x, 2, "nearest"), w, padding=1)
        return torch.nn.grad.conv2d_weight(F.interpolate(x, scale_factor=2, mode="nearest"), (c.Cout, c.Cin, 3, 3), dy, padding=1)
    if c.ks == 4:                # the space-to-depth stem: 4x4, pad 2, the output cropped to H x W (its last row and column dropped)
        dy = F.pad(dy, (0, 1, 0, 1))
    return torch.nn.grad.conv2d_weight(x, (c.Cout, c.Cin, c.ks, c.ks), dy, stride=c.stride, padding=pad_of(c), dilation=c.dil)


@functools.lru_cache(maxsize=4)
def _reference(key, c):
    return reference_of(c, _data(key))


def reference(c):
    """float64 dW of a case, computed once per shape and shared by its precisions and launch forms; treat as read-only"""
    return _reference(_data_key(c), c._replace(name="", group="", row=None, tiles=0, edges=(), prec=0, batch=False, batch_row=None))


def granule(c):
    """the unit every product (and so every sum) is a multiple of"""
    return 0.5 if c.form == "bn" else 1.0


# ---- the reduce alone: synthetic partial slabs ----
RED_SPLITK = [1, 7, 8, 9, 24, 25, 32, 33, 57]       # around the 8 phases of a workgroup and the 32 slabs of its unrolled loop
RED_TAPS = [1, 4, 9, 16]
RED_O, RED_OSLAB = 5, 8                             # three padded rows per tap, filled with NaN
RED_I_VEC, RED_I_SCALAR = 12, 6                     # I % 4 == 0: one 16-byte load per slab and lane; else element loads
RED_MAX = 1000                                      # |partial| <= 1000: 57 of them stay far below 2^24


def reduce_job(splitk, taps, I, seed):
    """part [splitk, taps, Oslab, I] float32 (integers, NaN in rows O .. Oslab - 1), `before` [O, I, taps] float32 integers"""
    g = gen("reduce", splitk, taps, I, seed)
    part = ints((splitk, taps, RED_OSLAB, I), g, RED_MAX)
    part[:, :, RED_O:, :] = float("nan")
    before = ints((RED_O, I, taps), g, RED_MAX)
    return part, before


def reduce_ref(part, before, accumulate):
    """float64 [O, I, taps]: the sum of the same partials over the split, in dW's OIHW order"""
    s = part[:, :, :RED_O, :].double().sum(0).permute(1, 2, 0)
    return s + before.double() if accumulate else s


def reduce_jobs(splitk, swap):
    """the four jobs of one launch: taps 1, 4, 9, 16 with the vector and the scalar form alternating (swap: the other way round)"""
    return [(taps, (RED_I_VEC, RED_I_SCALAR)[(k + swap) % 2]) for k, taps in enumerate(RED_TAPS)]


# ---- the comparator ----
def exact(got, want, what):
    """torch.equal(got, want) for a float32 result and its float64 reference (exactly representable in float32); prints how many
    elements differ and where the first one lies"""
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), "%s: non-finite" % what
    ne = got != want
    bad = int(ne.sum())
    first = ne.nonzero()[0].tolist() if bad else None
    print("%s: %d of %d elements differ, first at %s (max |diff| %g)" % (what, bad, want.numel(), first,
                                                                       float((got - want).abs().max()) if want.numel() else 0.0))
    assert torch.equal(got, want), "%s: %d of %d elements differ, first at %s: got %r, want %r" % (
        what, bad, want.numel(), first, float(got[tuple(first)]), float(want[tuple(first)]))
