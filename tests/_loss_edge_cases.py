"""What tests/test_loss_optim_edges_gpu.py and tests/test_loss_optim_edges_cpu.py share: the seeded inputs of the loss / metric /
optimizer edge cases (float32 values on the CPU; the references cast them up to float64, so both sides see the same numbers)
and the float64 restatements that have no oracle function of their own."""
import functools

import torch
import torch.nn.functional as F

# (B, H, W) of the cases past one grid pass: the loss and metric kernels launch at most 1024 x 256 = 262144 threads
#   3 x 517 x 513 = 795663 pixels, four passes; the stride is below HW (focal_kernel: db = 0, occasional carries)
#   5 x 231 x 233: HW = 53823, db = 4, dp = 46852, the second pass partly filled
#   700 x 19 x 21: HW = 399, db = 657, dp = 1
PASS_SHAPES = [(3, 517, 513), (5, 231, 233), (700, 19, 21)]
GENERIC_SHAPE = PASS_SHAPES[1]           # where the generic focal kernel (C not in (2, 5)) also runs past one pass
CE_BWD_SHAPE = (1, 1031, 1021)           # 1052651 pixels > the 4096 x 256 threads of ce_bwd_kernel
IGNORE = 255


def shape_id(s):
    return "x".join(str(v) for v in s)


@functools.lru_cache(maxsize=2)
def pass_inputs(shape, C, ignore_rows=0):
    """logits [B, C, H, W] float32 (scale 2), labels [B, H, W] in 0..C-1 (`ignore_rows` rows of every image IGNORE),
    a binary map [B, 1, H, W] for the dice term"""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * C + B)
    logits = torch.randn(B, C, H, W, generator=g) * 2
    tgt = torch.randint(0, C, (B, H, W), generator=g)
    if ignore_rows:
        tgt[:, H // 3:H // 3 + ignore_rows] = IGNORE
    binary = (torch.rand(B, 1, H, W, generator=g) > 0.7).long()
    return logits, tgt, binary


def dice_constant64(logits, target, eps=1e-7):
    """cdnet_ref.dice_constant with float64 sums (that function casts to float32 itself): smp's binary DiceLoss on the arg-max mask"""
    pred = torch.argmax(logits, dim=1).double()
    bs = target.shape[0]
    y_true = target.reshape(bs, 1, -1).double()
    y_pred = F.logsigmoid(pred).exp().reshape(bs, 1, -1)
    inter = (y_pred * y_true).sum(dim=(0, 2))
    card = (y_pred + y_true).sum(dim=(0, 2))
    loss = (1.0 - 2.0 * inter / card.clamp_min(eps)) * (y_true.sum(dim=(0, 2)) > 0).double()
    return loss.mean()


TIE_SHAPE = (2, 33, 31)


def tie_inputs(C):
    """logits on the grid {-1, -0.5, 0, 0.5, 1}: rows 0-2 have all classes equal, rows 3-5 only the last two classes tie (at 1,
    the others <= 0.5), and on 60 % of the remaining pixels the maximum is copied into a second, randomly chosen class (before
    or after the first one).  Labels 0..C-1 with 255, C and -1 mixed in; a binary map for the dice term."""
    B, H, W = TIE_SHAPE
    g = torch.Generator().manual_seed(7000 + C)
    z = torch.randint(-2, 3, (B, C, H, W), generator=g).float() * 0.5
    first = z.argmax(1, keepdim=True)
    other = (first + 1 + torch.randint(0, max(C - 1, 1), first.shape, generator=g)) % C      # a class other than `first`
    dup = torch.rand(B, 1, H, W, generator=g) < 0.6
    z = torch.where(dup & (torch.arange(C).view(1, C, 1, 1) == other), z.max(1, keepdim=True).values, z)
    z[:, :, :3] = z[:, :1, :3]
    z[:, :, 3:6] = z[:, :, 3:6].clamp(max=0.5)
    z[:, C - 2:, 3:6] = 1.0
    tgt = torch.randint(0, C, (B, H, W), generator=g)
    u = torch.rand(B, H, W, generator=g)
    tgt[u < 0.05] = 255
    tgt[(u >= 0.05) & (u < 0.10)] = C
    tgt[(u >= 0.10) & (u < 0.12)] = -1
    binary = (torch.rand(B, 1, H, W, generator=g) > 0.6).long()
    return z, tgt, binary


def tied_fraction(z):
    """share of the pixels whose maximum is attained by more than one class"""
    return float(((z == z.max(1, keepdim=True).values).sum(1) > 1).float().mean())


SAT_GAPS = (0.0, 30.0, 90.0, 200.0)      # expf(-gap) is exactly 0 in float32 above 104


def saturation_inputs(C):
    """[2, C, 16, 16] logits of size ~1 and labels; on the first 32 pixels of each image one class is lifted or lowered by each
    of SAT_GAPS (both signs), with the label on that class and on another one, two pixels per combination"""
    B, H, W = 2, 16, 16
    g = torch.Generator().manual_seed(4000 + C)
    z = torch.randn(B, C, H * W, generator=g)
    tgt = torch.randint(0, C, (B, H * W), generator=g)
    p = 0
    for gap in SAT_GAPS:
        for sign in (1.0, -1.0):
            for on_class in (True, False):
                for _ in range(2):
                    k = p % C
                    z[:, k, p] += sign * gap
                    tgt[:, p] = k if on_class else (k + 1) % C
                    p += 1
    assert p == 32
    return z.reshape(B, C, H, W), tgt.reshape(B, H, W)


COMBO_SAT = (16.0, 17.0, 25.0)    # float32 sigmoid: 1 - 2^-23 and 1 - 2^-24, both beyond FocalLoss2d's clamp at 1 - 1e-6; exactly 1.0
COMBO_SCALE = 1.5                 # of the random logits: |x| < 8, where 1 - sigmoid(x) keeps 4 digits in float32 (see combo_inputs)


def combo_masks(B, C, H, W, g):
    return (torch.rand(B, C, H, W, generator=g) > 0.7).float()


def combo_inputs(B, C, H, W, seed):
    """logits [B, C, H, W] of scale COMBO_SCALE and 0 / 1 masks.  The scale keeps the random part where float32 is well
    conditioned: FocalLoss2d reads 1 - sigmoid(x), which float32 knows to 3e-8 absolute, i.e. to 3e-8 e^x relative -- at the
    |x| = 11 .. 15 that a scale of 3 reaches over a million pixels the float32 ORACLE's gradient is 8e-3 of the maximum away from
    its float64 self, and no float32 kernel could be held to 1e-5.  Saturated logits have a case of their own."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g) * COMBO_SCALE, combo_masks(B, C, H, W, g)


def combo_saturation_inputs():
    """[2, 5, 24, 20] logits and 0 / 1 masks; row r < 6 of every channel holds +-COMBO_SAT[r // 2], its left half on mask 1 and
    its right half on mask 0.  Returns logits, masks and the number of saturated rows (all of them outside the clamp)."""
    z, m = combo_inputs(2, 5, 24, 20, 4100)
    rows = 2 * len(COMBO_SAT)
    for r in range(rows):
        z[:, :, r] = COMBO_SAT[r // 2] * (1.0 if r % 2 == 0 else -1.0)
        m[:, :, r, :10] = 1.0
        m[:, :, r, 10:] = 0.0
    return z, m, rows


def combo_ref(logits, masks, weights, upstream=None):
    """float64: sum_c w_c ComboLoss{dice 1, focal 8}(channel c) by the oracle's combo_loss_channel, its channel terms, and the
    gradient of `upstream` x the loss when `upstream` is given"""
    import cdnet_ref as O
    lg = logits.double().requires_grad_(upstream is not None)
    ch = [O.combo_loss_channel(lg[:, c], masks[:, c].double()) for c in range(logits.shape[1])]
    loss = sum(float(w) * l for w, l in zip(weights.double().tolist(), ch))
    grad = None
    if upstream is not None:
        (loss * upstream).backward()
        grad = lg.grad
    return float(loss.detach()), [float(l.detach()) for l in ch], grad


OPT_N = 3145805                           # three passes of the optimizers' 4096 x 256 threads plus 77
NORM_TAILS = (1, 2, 3, 4, 5, 7, 1027)     # n & 3 in (0, 1, 2, 3) below, at and above one float4; 1027: a full workgroup of float4 and a tail of 3


def adamw_xbd_ref(p, m, v, gr, t, lr, b1, b2, eps, wd):
    """one step of the hand-rolled rule (xBD_code/adamw.py:66-84), in place, in the dtype of its arguments"""
    m.mul_(b1).add_(gr, alpha=1 - b1)
    v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
    denom = v.sqrt().add_(eps)
    step_size = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
    p.add_(p, alpha=-wd * lr)
    p.addcdiv_(m, denom, value=-step_size)


POOL_SHAPES = [(21, 27), (20, 27), (1, 7), (7, 1), (2, 2), (1, 1)]
POOL_LARGE = (3, 64, 420, 420)            # 3 x 210 x 210 x 16 = 2116800 pieces > the 8192 x 256 threads of ew_grid
