"""Thin torch-tensor wrappers over the C ABI (include/dahitra_hip.h).

torch is used for device memory and the current HIP stream only; every arithmetic result below is
produced by a kernel of libdahitra_hip.so.  All activations are NHWC tensors of dtype float32
(parity mode) or bfloat16 (throughput mode)."""
import bisect
import ctypes
import math
import os
import sys

import numpy as np
import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
_DT = {torch.float32: 0, torch.bfloat16: 1}
_vp = ctypes.c_void_p


def dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("dahitra_amd: unsupported activation dtype %s" % t.dtype)


def set_f32_mma_mode(mode):
    """dh_set_f32_mma_mode: 0 = exact fp32 MFMA, 1 = split-bf16 three-product form (two bf16 planes, unit roundoff 2^-17), 2 = the
    six-product form (three bf16 planes, 2^-23), 3 = the split-fp16 three-product form (two fp16 planes, ~2^-21; operands inside
    fp16's range) for the matrix products of every fp32 launch this host thread issues from now on (the Engine sets it at each
    of its entry points: compute_dtype="bf16x3" = form 3 forward, form 1 backward)."""
    _lib.check(_lib.lib().dh_set_f32_mma_mode(int(mode)), "dh_set_f32_mma_mode")


def get_f32_mma_mode():
    return int(_lib.lib().dh_get_f32_mma_mode())


class f32_mma_mode:
    """with ops.f32_mma_mode(1): ...  -- the mode for the block, the previous one restored after it"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = get_f32_mma_mode()
        set_f32_mma_mode(self.mode)
        return self

    def __exit__(self, *exc):
        set_f32_mma_mode(self.prev)
        return False


def chunk_channels(dtype):
    """channels per 64-byte MFMA K-chunk: the granularity of Cin for dh_conv2d_fwd"""
    return 32 if dtype == torch.bfloat16 else 16


def P(t):
    if t is None:
        return _vp(0)
    assert t.is_cuda and t.is_contiguous(), "dahitra_amd ops need contiguous device tensors"
    return _vp(t.data_ptr())


def S():
    return _vp(torch.cuda.current_stream().cuda_stream)


_ws = {}


def workspace(nbytes, device):
    """scratch for ONE launch at a time per stream (keyed by device AND current stream: the levels of the hierarchical model
    run on streams of their own, Engine._run_staged, and must not share it)"""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream) if torch.device(device).type == "cuda" else str(device)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def rekey_workspace(device, old_stream, new_stream):
    """hand the scratch buffer that `old_stream` grew (a graph's eager warm-up) to `new_stream` (its capture stream): the
    capture then finds a buffer of the right size that lives OUTSIDE the graph's private pool, and the warm-up stream --
    which is gone after the capture -- leaves no entry behind"""
    buf = _ws.pop((str(device), old_stream.cuda_stream), None)
    if buf is not None:
        cur = _ws.get((str(device), new_stream.cuda_stream))
        if cur is None or cur.numel() < buf.numel():
            _ws[(str(device), new_stream.cuda_stream)] = buf


_PINNED = []        # buffers a captured HIP graph points into: kept alive for the life of the process


def pin_captured_buffers(net):
    """Called right after a HIP-graph capture of `net`'s step.  The graph's kernel nodes hold RAW pointers into
    buffers that live outside the graph's private pool: the shared scratch workspace, the weight-gradient plan's slabs
    and device job table, the packed-weight plans, the parameter / gradient arenas.  Each of them is normally replaced
    (and the old tensor returned to the allocator) when a later eager call needs more room or another shape -- the
    last partial batch of an epoch, an eval forward at a larger size, another net in the process.  Holding a reference
    here means a replacement allocates a NEW buffer while the one the graph reads and writes stays valid."""
    keep = list(_ws.values())
    eng = net._engine
    if eng._wgrad_plan is not None:
        keep += list(eng._wgrad_plan.slots) + list(eng._wgrad_plan.tables.values())
    for pack, _, xstack, wstack in eng._plans.values():
        keep += [pack.table] + list(pack.keep) + list(xstack.values())
        for fwd_stack, dgrad_stack in wstack.values():
            keep += [fwd_stack, dgrad_stack]
    keep += [net._arena.flat, net._arena.grad]
    keep = [t for t in keep if t is not None]
    _PINNED.extend(keep)
    return keep


def _call(name, *args):
    L = _lib.lib()
    _lib.check(getattr(L, name)(*args), name)


def cdiv(a, b):
    return (a + b - 1) // b


def pad16(c):
    return cdiv(c, 16) * 16


# ---- weights -------------------------------------------------------------------------------------
def pack_weight(w, dtype, want_dgrad=True, dgrad_inner=0, out_scale=None, want_fwd=True, out_dgrad=None):
    """w: OIHW (or [O, I]) fp32 master.  Returns (fwd [taps, OPad, I], dgrad [taps, IPad, OK] | None).
    out_scale [O]: per-output-channel factor folded into the forward form (eval-mode BatchNorm).
    out_dgrad: write the data-gradient form into this (contiguous) buffer instead of a fresh one."""
    if w.dim() == 2:
        O, I = w.shape
        ks = 1
    else:
        O, I, ks, _ = w.shape
    OPad, IPad = pad16(O), pad16(I)
    OK = max(O, dgrad_inner)
    fwd = torch.empty(ks * ks, OPad, I, dtype=dtype, device=w.device) if want_fwd else None
    if out_dgrad is not None:
        assert out_dgrad.numel() == ks * ks * IPad * OK and out_dgrad.dtype == dtype
        dg = out_dgrad
    else:
        dg = torch.empty(ks * ks, IPad, OK, dtype=dtype, device=w.device) if want_dgrad else None
    _call("dh_pack_weight", _DT[dtype], P(w), P(out_scale), O, I, ks, OPad, P(fwd), IPad, OK, P(dg), S())
    return fwd, dg


class PackPlan:
    """persistent packed-weight buffers + the device job table of dh_pack_weights_multi (one launch per step)"""

    class _Job(ctypes.Structure):
        _fields_ = [("w", ctypes.c_void_p), ("fwd", ctypes.c_void_p), ("dgrad", ctypes.c_void_p), ("O", ctypes.c_int),
                    ("I", ctypes.c_int), ("KS", ctypes.c_int), ("OPad", ctypes.c_int), ("IPad", ctypes.c_int),
                    ("OK", ctypes.c_int), ("dtype", ctypes.c_int), ("first_block", ctypes.c_int), ("nblocks", ctypes.c_int)]

    def __init__(self, device):
        self.device, self.jobs, self.blocks, self.table, self.keep = device, [], 0, None, []

    def add(self, w, dtype, want_fwd=True, want_dgrad=True, dgrad_inner=0, out_dgrad=None, frag=False, out_fwd=None):
        """same contract as pack_weight; returns the (persistent) fwd / dgrad buffers.  frag (bf16 3x3 weights, I and
        dgrad_inner multiples of 32): the buffers are in FRAGMENT order [rows / 16, K / 32, taps, 64, 8] -- what the
        register-resident-weights convolution loads (conv2d's w_frag); add the layer a second time without it for the
        row-major form every other kernel reads"""
        if w.dim() == 2:
            (O, I), ks = w.shape, 1
        else:
            O, I, ks, _ = w.shape
        OPad, IPad, OK = pad16(O), pad16(I), max(O, dgrad_inner)
        ck = chunk_channels(dtype)
        if frag:
            assert ks == 3 and dtype == torch.bfloat16 and I % 32 == 0 and OK % 32 == 0 and out_dgrad is None
            fwd = torch.empty(OPad // 16, I // 32, ks * ks, 64, 8, dtype=dtype, device=w.device) if want_fwd else None
            dg = torch.empty(IPad // 16, OK // 32, ks * ks, 64, 8, dtype=dtype, device=w.device) if want_dgrad else None
        else:
            fwd = out_fwd if out_fwd is not None else \
                (torch.empty(ks * ks, OPad, I, dtype=dtype, device=w.device) if want_fwd else None)
            dg = out_dgrad if out_dgrad is not None else \
                (torch.empty(ks * ks, IPad, OK, dtype=dtype, device=w.device) if want_dgrad else None)
        n = max(fwd.numel() if fwd is not None else 0, dg.numel() if dg is not None else 0)
        assert n < 2 ** 31 and w.numel() < 2 ** 31, "pack_weights_multi indexes a layer with 32-bit arithmetic"
        nb = max(1, min(256, cdiv(n, 2048)))        # a lane packs 8 elements per pass (16-byte store): one pass per lane
        if ks == 3 and O % 32 == 0 and I % 32 == 0 and OK == O:
            nb = min(256, (O // 32) * (I // 32))       # the tiled form (csrc/pointwise.hip pack_job_tiled): one 32 x 32 x 9 tile per workgroup
        self.jobs.append(self._Job(w.data_ptr(), fwd.data_ptr() if fwd is not None else None,
                                   dg.data_ptr() if dg is not None else None, O, I, ks, OPad, IPad, OK,
                                   _DT[dtype] | (0x200 if frag else 0), self.blocks, nb))
        self.blocks += nb
        self.keep += [w, fwd, dg]
        return fwd, dg

    def run(self):
        if not self.jobs:
            return
        if self.table is None:
            assert ctypes.sizeof(self._Job) == _lib.lib().dh_pack_job_size()
            raw = b"".join(bytes(j) for j in self.jobs)
            self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        _call("dh_pack_weights_multi", P(self.table), len(self.jobs), self.blocks, S())


class WgradPlan:
    """The split-K reduces of one backward pass as ONE launch (dh_wgrad_reduce_multi): while a plan is active
    (`with plan:`), conv2d_wgrad writes its partial slabs into a per-layer persistent workspace and records a job;
    `run()` sums them all into the gradient arena.  The job table is built on the first pass and reused while the
    sequence of layers (gradient pointers, shapes, split factors) repeats -- which it does for a fixed network and
    batch shape, and what makes the table capturable in a HIP graph."""

    class _Job(ctypes.Structure):
        _fields_ = [("part", ctypes.c_void_p), ("dw", ctypes.c_void_p), ("splitk", ctypes.c_int), ("taps", ctypes.c_int),
                    ("Oslab", ctypes.c_int), ("O", ctypes.c_int), ("I", ctypes.c_int), ("accumulate", ctypes.c_int),
                    ("first_block", ctypes.c_int), ("nblocks", ctypes.c_int)]

    def __init__(self, device, batch=False):
        """batch: the wave-specialised 3x3 weight gradients of the pass are RECORDED by conv2d_wgrad and issued as one launch by
        run() (dh_wgrad_batch_*: fewer, longer K slices per layer, a quarter of the partial-slab traffic); their x / dy are
        kept alive until then.  Off under ops.PROFILE (the per-launch events need one launch per layer) and with
        DAHITRA_WGRAD_BATCH=0."""
        self.device, self.slots, self.cur, self.blocks = device, [], 0, 0
        self.tables, self.sigs, self.phase = {}, {}, 0      # one job table per run() of a pass (a split backward runs twice)
        self._prev = None
        self.post = []
        self.batch = batch and os.environ.get("DAHITRA_WGRAD_BATCH", "1") != "0"
        self.batching, self.keep = False, []

    def __enter__(self):
        global _WGRAD_PLAN
        self._prev, _WGRAD_PLAN = _WGRAD_PLAN, self
        self.cur = 0
        self.jobs = []
        self.post = []
        self.blocks = 0
        self.phase = 0
        self.keep = []
        self.batching = self.batch and PROFILE is None
        if self.batching:
            _call("dh_wgrad_batch_begin")
        elif self._prev is None:
            _call("dh_wgrad_batch_abort")       # a pass that never finished must not leave its batch open behind it
        return self

    def __exit__(self, *exc):
        global _WGRAD_PLAN
        _WGRAD_PLAN = self._prev
        if self.batching:
            self.batching = False
            if exc and exc[0] is not None:
                _lib.lib().dh_wgrad_batch_abort()      # drop what an aborted pass recorded
            else:
                _call("dh_wgrad_batch_end", S())
            self.keep = []
        return False

    def hold(self, *tensors):
        """operands of a recorded (not yet issued) weight-gradient launch"""
        if self.batching:
            self.keep += [t for t in tensors if t is not None]

    def slab(self, nbytes):
        """persistent workspace of the cur-th deferred layer of the pass"""
        if self.cur == len(self.slots):
            self.slots.append(torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device))
        elif self.slots[self.cur].numel() < nbytes:
            _PINNED.append(self.slots[self.cur])         # a captured graph may still point at the smaller buffer
            self.slots[self.cur] = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self.tables = {}
        buf = self.slots[self.cur]
        self.cur += 1
        return buf

    def add(self, part, dw, splitk, taps, oslab, o, i, accumulate):
        nb = cdiv(o * i * taps, _lib.lib().dh_wgrad_reduce_outputs_per_block(i))
        self.jobs.append(self._Job(part.data_ptr(), dw.data_ptr(), splitk, taps, oslab, o, i, int(accumulate),
                                   self.blocks, nb))
        self.blocks += nb

    def run(self):
        """reduce every layer deferred since the last run() of this pass (a split backward calls it once per part)"""
        if self.batching:
            _call("dh_wgrad_batch_launch", S())      # the recorded weight gradients, one launch
            self.keep = []
        if self.jobs:
            self._run_reduce()
        for fn in self.post:          # launches that consume reduced gradients (phase-gradient combine)
            fn()
        self.jobs, self.post, self.blocks = [], [], 0
        self.phase += 1

    def _run_reduce(self):
        sig = b"".join(bytes(j) for j in self.jobs)
        if self.tables.get(self.phase) is None or sig != self.sigs.get(self.phase):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("dahitra_amd: the weight-gradient plan changed during graph capture; run one eager "
                                   "step of the same shapes first")
            assert ctypes.sizeof(self._Job) == _lib.lib().dh_wgrad_reduce_job_size()
            if self.tables.get(self.phase) is not None:
                _PINNED.append(self.tables[self.phase])
            self.tables[self.phase] = torch.frombuffer(bytearray(sig), dtype=torch.uint8).to(self.device)
            self.sigs[self.phase] = sig
        _call("dh_wgrad_reduce_multi", P(self.tables[self.phase]), len(self.jobs), self.blocks, S())


_WGRAD_PLAN = None


# ---- convolution / linear ------------------------------------------------------------------------
PROFILE = None       # set to {} by bench.py to collect (events, algorithmic flops, algorithmic bytes) per launch
REPLAY = None        # set to {"key": class, "calls": []} by bench.py for ONE eager step: the C calls of that kernel class as
                     # closures (stream -> launch) with their tensors kept alive, to be re-issued back to back in a recorded graph


class _Prof:
    """bench.py's per-launch timer: HIP events recorded on the launch stream around ONE kernel launch of class `key`,
    with that launch's algorithmic FLOPs and bytes (what the launch must read + write, each tensor once)"""
    __slots__ = ("ev",)

    def __init__(self, key, flops, nbytes):
        self.ev = None
        if PROFILE is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            PROFILE.setdefault(key, []).append((self.ev, float(flops), float(nbytes)))

    def __enter__(self):
        if self.ev is not None:
            self.ev[0].record()

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
        return False


def _nb(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


def _bn_in_args(b):
    if b is None:
        return _vp(0), _vp(0), 0
    return P(b.scale), P(b.shift), b.groups


def _gate_args(gate):
    if gate is None:
        return _vp(0), _vp(0), _vp(0), _vp(0), 0
    out_relu, y, mean, invstd, groups = gate
    return P(out_relu), P(y), P(mean), P(invstd), groups


class BnInput:
    """An activation that exists only as (pre-normalisation conv output y, per-group scale / shift): the consumer
    kernels apply relu(y * scale + shift) while they load it (dh_conv2d_fwd's in_scale, dh_conv2d_wgrad_bn_in)."""
    __slots__ = ("y", "scale", "shift", "groups")

    def __init__(self, y, scale, shift, groups):
        self.y, self.scale, self.shift, self.groups = y, scale, shift, groups

    @property
    def shape(self):
        return self.y.shape

    @property
    def device(self):
        return self.y.device

    @property
    def dtype(self):
        return self.y.dtype


def conv3x3_res_bits_supported(xshape, cout, wp, dtype, has_frag):
    """does a kernel family apply the mask bytes of conv2d(..., residual=r, res_bits=b) for this 3x3 / stride 1 / pad 1 layer
    (dh_conv3x3_res_bits_supported)?  Where not, callers keep the masked copy of the residual."""
    N, H, W, Cin = xshape
    return dtype in _DT and bool(_lib.lib().dh_conv3x3_res_bits_supported(_DT[dtype], N, H, W, Cin, cout, wp.shape[-2], int(bool(has_frag))))


def _conv3x3_res_bits(x, wp, cout, residual, res_bits, alg_flops, w_frag):
    N, H, W, Cin = x.shape
    v = 8 if x.dtype == torch.bfloat16 else 4
    assert residual.shape == (N, H, W, cout) and residual.dtype == x.dtype and res_bits.dtype == torch.uint8 and \
        res_bits.numel() == residual.numel() // v
    if not conv3x3_res_bits_supported(x.shape, cout, wp, x.dtype, w_frag is not None):
        raise _lib.HipLibraryError("dahitra_amd: no kernel applies the residual's mask bytes for %s -> %d channels "
                                   "(ops.conv3x3_res_bits_supported)" % (tuple(x.shape), cout))
    cpad = wp.shape[-2]
    y = torch.empty(N, H, W, cout, dtype=x.dtype, device=x.device)
    nt_ = 64 if cpad % 64 == 0 else (32 if cpad % 32 == 0 else 16)
    key = "conv_mfma<%s,ks3,s1,nt%d>" % ("bf16" if x.dtype == torch.bfloat16 else "f32", nt_)
    flops = alg_flops if alg_flops else 2.0 * N * H * W * cout * Cin * 9
    fixed = (dt(x), P(x), P(wp), P(w_frag), P(residual), P(res_bits), P(y), N, H, W, Cin, cout, cpad)
    with _Prof(key, flops, _nb(x, y, wp, residual, res_bits)):
        _call("dh_conv3x3_res_bits_fwd", *fixed, S())
    if REPLAY is not None and key == REPLAY["key"]:
        REPLAY["calls"].append((lambda stream, fixed=fixed: _call("dh_conv3x3_res_bits_fwd", *fixed, stream),
                                (x, wp, w_frag, residual, res_bits, y), flops))
    return y


def conv2d(x, wp, cout, ks=3, stride=1, pad=1, bias=None, residual=None, act=ACT_NONE, want_stats=False,
           want_preact=False, npix_valid=0, w_image_stride=0, out_hw=None, alg_flops=0, dilation=1, gate=None, w_frag=None,
           res_bits=None):
    """gate = (out_relu | None, y_pre_bn, mean, invstd, groups): BN-backward gating of a data-gradient launch; the
    call then returns (g, partials) for bn_bwd_from_partials (see include/dahitra_hip.h).
    x may be a BnInput: BatchNorm-apply + ReLU happen on load.
    res_bits (3x3 / stride 1 / pad 1, nothing but the residual): the residual added is (bit ? residual : 0), the bits in the
    layout of bn_apply(want_bits=True); raises where no kernel applies them (conv3x3_res_bits_supported)."""
    if res_bits is not None:
        assert residual is not None and ks == 3 and stride == 1 and pad == 1 and dilation == 1 and bias is None and \
            act == ACT_NONE and not want_stats and not want_preact and not npix_valid and not w_image_stride and gate is None and \
            torch.is_tensor(x) and (out_hw is None or tuple(out_hw) == tuple(x.shape[1:3]))
        return _conv3x3_res_bits(x, wp, cout, residual, res_bits, alg_flops, w_frag)
    if isinstance(x, Up4Input):
        assert ks == 3 and stride == 1 and pad == 1 and dilation == 1 and residual is None and gate is None and not want_preact
        return _conv3x3_up4(x, wp, cout, bias, act, want_stats)
    bn_in = x if isinstance(x, BnInput) else None
    if bn_in is not None:
        x = bn_in.y
    N, H, W, Cin = x.shape
    if gate is not None:
        want_stats = True
    if out_hw is None:
        OH = (H + 2 * pad - dilation * (ks - 1) - 1) // stride + 1
        OW = (W + 2 * pad - dilation * (ks - 1) - 1) // stride + 1
    else:
        OH, OW = out_hw
    cpad = wp.shape[-2]
    y = torch.empty(N, OH, OW, cout, dtype=x.dtype, device=x.device)
    pre = torch.empty_like(y) if want_preact else None
    stats = None
    if want_stats:
        nt = _lib.lib().dh_conv2d_fwd_num_tiles(_DT[x.dtype], N, OH, OW, Cin, ks, stride)
        stats = torch.empty(2, cpad, nt, dtype=torch.float32, device=x.device)      # [sum | sumsq][channel][tile]
    nt_ = 64 if cpad % 64 == 0 else (32 if cpad % 32 == 0 else 16)
    key = "conv_mfma<%s,ks%d,s%d,nt%d>" % ("bf16" if x.dtype == torch.bfloat16 else "f32", ks, stride, nt_)
    flops = alg_flops if alg_flops else 2.0 * N * OH * OW * cout * Cin * ks * ks
    fixed = (dt(x), P(x), P(wp), P(y), P(bias), P(residual), P(stats), N, H, W, Cin, OH, OW, cout, cpad, ks, stride, pad, act,
             npix_valid, w_image_stride, P(pre), dilation, *_gate_args(gate), *_bn_in_args(bn_in), 0, P(w_frag))
    with _Prof(key, flops, _nb(x, y, wp, residual, pre)):
        _call("dh_conv2d_fwd", *fixed, S())
    if REPLAY is not None and key == REPLAY["key"]:
        REPLAY["calls"].append((lambda stream, fixed=fixed: _call("dh_conv2d_fwd", *fixed, stream),
                                (x, wp, y, bias, residual, stats, pre, w_frag, gate, bn_in), flops))
    out = [y]
    if want_stats:
        out.append(stats)
    if want_preact:
        out.append(pre)
    return out[0] if len(out) == 1 else tuple(out)


class Up4Input:
    """nn.Upsample(4, 'bilinear')(|a - b|) of two [N, h, w, 32] bf16 maps WITHOUT the [N, 4h, 4w, 32] tensor (models/networks.py:
    383-389: the input of classifier.0): conv2d interpolates its tiles from a and b while it loads (dh_conv3x3_up4_fwd);
    conv2d_wgrad materialises the map.  `.shape` is the shape the upsampled tensor would have."""
    __slots__ = ("a", "b")

    def __init__(self, a, b):
        assert a.shape == b.shape and a.dim() == 4 and a.shape[-1] == 32 and a.dtype == torch.bfloat16
        assert a.is_contiguous() and b.is_contiguous()
        self.a, self.b = a, b

    @property
    def shape(self):
        n, h, w, c = self.a.shape
        return torch.Size((n, 4 * h, 4 * w, c))

    def materialize(self):
        return absdiff_upsample4(self.a, self.b)


def _conv3x3_up4(u, wp, cout, bias, act, want_stats):
    N, H, W, _ = u.shape
    assert cout == 32 and tuple(wp.shape) == (9, 32, 32) and wp.dtype == torch.bfloat16
    y = torch.empty(N, H, W, 32, dtype=torch.bfloat16, device=u.a.device)
    stats = None
    if want_stats:
        stats = torch.empty(2, 32, _lib.lib().dh_conv2d_fwd_num_tiles(_DT[torch.bfloat16], N, H, W, 32, 3, 1), dtype=torch.float32, device=y.device)
    key, flops = "conv_mfma<bf16,ks3,s1,nt32>", 2.0 * N * H * W * 32 * 32 * 9
    fixed = (P(u.a), P(u.b), P(wp), P(bias), act, P(y), P(stats), N, H, W)
    with _Prof(key, flops, _nb(u.a, u.b, y, wp)):
        _call("dh_conv3x3_up4_fwd", *fixed, S())
    if REPLAY is not None and key == REPLAY["key"]:
        REPLAY["calls"].append((lambda stream, fixed=fixed: _call("dh_conv3x3_up4_fwd", *fixed, stream), (u.a, u.b, wp, bias, y, stats), flops))
    return (y, stats) if want_stats else y


class SplitCat:
    """torch.cat([t[:B], t[B:]], channel) of a [2B, H, W, C] tensor WITHOUT the concatenated tensor (models/networks.py:1344:
    cat([a_128, b_128], 1) -- the two temporal streams are the two halves of one batch here).  conv3x3_split / conv2d_wgrad
    read the two halves in place; `.shape` is the shape the concatenation would have."""
    __slots__ = ("t", "B")

    def __init__(self, t):
        assert t.dim() == 4 and t.shape[0] % 2 == 0 and t.is_contiguous()
        self.t, self.B = t, t.shape[0] // 2

    @property
    def shape(self):
        n, h, w, c = self.t.shape
        return torch.Size((n // 2, h, w, 2 * c))

    @property
    def split_bytes(self):
        return self.t[self.B:].data_ptr() - self.t.data_ptr()

    def materialize(self):
        return cat_halves(self.t)


def conv3x3_split_supported(B, H, W, cin, cout, dtype):
    """can the 3x3 / stride 1 / pad 1 layer cin -> cout on B x H x W pixels run with a SplitCat input (forward and weight
    gradient) and a split data-gradient output?  (bf16, register-resident-weights + wave-specialised kernels; dahitra_hip.h)"""
    return dtype == torch.bfloat16 and os.environ.get("DAHITRA_NO_SPLIT_CAT", "0") != "1" and \
        bool(_lib.lib().dh_conv3x3_split_supported(B, H, W, cin, cout))


def conv3x3_split(x, wp, w_frag, cout, want_stats=False, split_out=False, alg_flops=0):
    """3x3 / stride 1 / pad 1 convolution with a SplitCat input and / or (split_out) an output whose channel halves are the two
    batch halves of a [2N, H, W, cout / 2] tensor (the data gradient of a layer that read a SplitCat)."""
    xs = x if isinstance(x, SplitCat) else None
    N, H, W, Cin = x.shape
    xt = xs.t if xs is not None else x
    assert xt.dtype == torch.bfloat16 and w_frag is not None and (xs is not None or split_out)
    if split_out:
        y = torch.empty(2 * N, H, W, cout // 2, dtype=xt.dtype, device=xt.device)
        ysplit = y[N:].data_ptr() - y.data_ptr()
    else:
        y = torch.empty(N, H, W, cout, dtype=xt.dtype, device=xt.device)
        ysplit = 0
    stats = None
    if want_stats:
        nt = _lib.lib().dh_conv2d_fwd_num_tiles(_DT[xt.dtype], N, H, W, Cin, 3, 1)
        stats = torch.empty(2, cout, nt, dtype=torch.float32, device=xt.device)
    flops = alg_flops if alg_flops else 2.0 * N * H * W * cout * Cin * 9
    fixed = (P(xt), xs.split_bytes if xs is not None else 0, P(wp), P(w_frag), P(y), ysplit, P(stats), N, H, W, Cin, cout)
    key = "conv_mfma<bf16,ks3,s1,nt64>"
    with _Prof(key, flops, _nb(xt, y, wp)):
        _call("dh_conv3x3_split_fwd", *fixed, S())
    if REPLAY is not None and key == REPLAY["key"]:
        REPLAY["calls"].append((lambda stream, fixed=fixed: _call("dh_conv3x3_split_fwd", *fixed, stream), (xt, wp, w_frag, y, stats), flops))
    return (y, stats) if want_stats else y


HEAD_FWD = os.environ.get("DAHITRA_NO_HEAD_FWD", "0") != "1"


def conv3x3_head(x, wp, ncls, bias, w_oihw=None):
    """the class head: 3x3 / pad 1 convolution to `ncls` (<= 16) channels, fp32 NCHW logits written by the kernel itself.
    x may be a BnInput (BatchNorm-apply + ReLU on load).  With the fp32 master weights w_oihw [ncls, 32, 3, 3] at hand, bf16
    activations (or fp32 ones under f32_mma_mode 3) of 32 channels and ncls <= 2 go to dh_head_fwd (one MFMA per input pixel group for all nine taps, no halo)."""
    bn_in = x if isinstance(x, BnInput) else None
    if bn_in is not None:
        x = bn_in.y
    N, H, W, Cin = x.shape
    assert wp.shape[-2] == 16 and ncls <= 16
    out = torch.empty(N, ncls, H, W, dtype=torch.float32, device=x.device)
    if HEAD_FWD and w_oihw is not None and Cin == 32 and N * H * W * 128 < 2 ** 31 and _lib.lib().dh_head_fwd_supported(ncls, W) and \
            (x.dtype == torch.bfloat16 or (x.dtype == torch.float32 and get_f32_mma_mode() == 3)):
        assert w_oihw.shape == (ncls, 32, 3, 3) and w_oihw.dtype == torch.float32
        with _Prof("head_fwd", 2.0 * N * H * W * ncls * Cin * 9, _nb(x, out)):
            _call("dh_head_fwd", dt(x), P(x), P(w_oihw), P(bias), ncls, *_bn_in_args(bn_in), P(out), N, H, W, S())
        return out
    key = "conv_mfma<%s,ks3,s1,nt16>" % ("bf16" if x.dtype == torch.bfloat16 else "f32")
    with _Prof(key, 2.0 * N * H * W * ncls * Cin * 9, _nb(x, out, wp)):
        _call("dh_conv3x3_head_fwd", dt(x), P(x), P(wp), P(bias), N, H, W, Cin, ncls, *_bn_in_args(bn_in), P(out), S())
    return out


def rows_view(x2d):
    """[rows, C] -> the [1, ceil(rows/16), 16, C] image view used for linear layers (no copy when
    rows % 16 == 0; otherwise the tail rows are masked through npix_valid)."""
    rows, C = x2d.shape
    return rows, cdiv(rows, 16), C


def linear(x2d, wp, cout, bias=None, residual=None, act=ACT_NONE, want_preact=False, images=1, w_image_stride=0):
    """x2d [rows, Cin] (rows = images * rows_per_image).  Returns [rows, cout]."""
    rows, Cin = x2d.shape
    rpi = rows // images
    Hh = cdiv(rpi, 16)
    cpad = wp.shape[-2]
    y = torch.empty(rows, cout, dtype=x2d.dtype, device=x2d.device)
    pre = torch.empty_like(y) if want_preact else None
    _call("dh_conv2d_fwd", dt(x2d), P(x2d), P(wp), P(y), P(bias), P(residual), _vp(0), images, Hh, 16, Cin, Hh, 16, cout, cpad, 1,
          1, 0, act, rpi, w_image_stride, P(pre), 1, *_gate_args(None), *_bn_in_args(None), 0, _vp(0), S())
    # note: with rows_per_image % 16 != 0 the image stride used by the kernel (Hh*16 rows) would differ
    # from rpi; callers guarantee rpi % 16 == 0 whenever images > 1.
    assert images == 1 or rpi % 16 == 0
    return (y, pre) if want_preact else y


def conv2d_wgrad(x, dy, dw, ks, stride, pad, accumulate=False, groups=1, use_tr=True, cout_real=0, cin=0, dilation=1,
                 defer=True):
    """dw (OIHW fp32, or [N, Cout, Cin] when groups == N) (+)= weight gradient.
    cin > 0: use only the first `cin` channels of x (x keeps its own channel pitch).
    x may be a BnInput (gradient against relu(y * scale + shift), computed on load)."""
    if isinstance(x, BnInput):
        return _conv2d_wgrad_bn_in(x, dy, dw, ks, stride, pad, accumulate, use_tr, cout_real, dilation, defer)
    if isinstance(x, SplitCat):
        return _conv2d_wgrad_split(x, dy, dw, ks, stride, pad, accumulate, defer)
    if isinstance(x, Up4Input):
        # (the weight gradient with the interpolation on load was built and measured -- 94 us against 67 us for the plain
        # kernel, and not reproducible from run to run at >= 512 workgroups; removed, DESIGN.md section 6e: the map is formed here)
        x = x.materialize()
    N, H, W, pitch = x.shape
    Cin = cin if cin else pitch
    _, OH, OW, Cout = dy.shape
    L = _lib.lib()
    nbytes = L.dh_conv2d_wgrad_workspace_size(N, OH, OW, Cin, Cout, ks, groups)
    plan = _WGRAD_PLAN
    if plan is not None and groups == 1 and defer:      # defer=False: the caller reads dw right after this call
        # deferred: partial slabs into this layer's persistent workspace, summed later by plan.run()
        ws = plan.slab(nbytes)
        sk = (ctypes.c_int * 1)()       # int* splitk_out
        with _Prof("conv_wgrad<%s,ks%d,s%d>" % ("bf16" if x.dtype == torch.bfloat16 else "f32", ks, stride),
                   2.0 * N * OH * OW * Cout * Cin * ks * ks, _nb(x, dy)):
            _call("dh_conv2d_wgrad_partial", dt(x), P(x), P(dy), P(dw), accumulate, N, H, W, Cin, OH, OW, Cout, ks, stride, pad,
                  1, 0, use_tr, cout_real, pitch, dilation, P(ws), sk, S())
        plan.hold(x, dy)
        if sk[0] > 0:
            plan.add(ws, dw, sk[0], ks * ks, Cout, cout_real if cout_real else Cout, Cin, accumulate)
        return
    ws = workspace(nbytes, x.device)
    _call("dh_conv2d_wgrad", dt(x), P(x), P(dy), P(dw), accumulate, N, H, W, Cin, OH, OW, Cout, ks, stride, pad, groups, 0,
          use_tr, cout_real, pitch, dilation, P(ws), S())


def _conv2d_wgrad_split(xs, dy, dw, ks, stride, pad, accumulate, defer):
    """weight gradient against a SplitCat input (3x3 / stride 1 / pad 1, bf16): the two tensors are read in place"""
    assert ks == 3 and stride == 1 and pad == 1
    N, H, W, Cin = xs.shape
    Cout = dy.shape[-1]
    nbytes = _lib.lib().dh_conv2d_wgrad_workspace_size(N, H, W, Cin, Cout, 3, 1)
    plan, own = (_WGRAD_PLAN if defer else None), False
    if plan is None:
        plan, own = WgradPlan(dy.device), True
        plan.__enter__()
    try:
        ws = plan.slab(nbytes)
        sk = (ctypes.c_int * 1)()       # int* splitk_out
        with _Prof("conv_wgrad<bf16,ks3,s1>", 2.0 * N * H * W * Cout * Cin * 9, _nb(xs.t, dy)):
            _call("dh_conv2d_wgrad_split", P(xs.t), xs.split_bytes, P(dy), P(dw), accumulate, N, H, W, Cin, Cout, P(ws), sk, S())
        plan.hold(xs.t, dy)
        plan.add(ws, dw, sk[0], 9, Cout, Cout, Cin, accumulate)
        if own:
            plan.run()
    finally:
        if own:
            plan.__exit__(*sys.exc_info())


def _conv2d_wgrad_bn_in(b, dy, dw, ks, stride, pad, accumulate, use_tr, cout_real, dilation, defer):
    x = b.y
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    nbytes = _lib.lib().dh_conv2d_wgrad_workspace_size(N, OH, OW, Cin, Cout, ks, 1)
    plan = _WGRAD_PLAN if defer else None
    ws = plan.slab(nbytes) if plan is not None else workspace(nbytes, x.device)
    sk = (ctypes.c_int * 1)()       # int* splitk_out
    with _Prof("conv_wgrad<%s,ks%d,s%d>" % ("bf16" if x.dtype == torch.bfloat16 else "f32", ks, stride),
               2.0 * N * OH * OW * Cout * Cin * ks * ks, _nb(x, dy)):
        _call("dh_conv2d_wgrad_bn_in", dt(x), P(x), P(dy), P(dw), accumulate, N, H, W, Cin, OH, OW, Cout, ks, stride, pad, use_tr,
              cout_real, dilation, P(b.scale), P(b.shift), b.groups, P(ws), sk if plan is not None else None, S())
    if plan is not None:
        plan.hold(x, dy, b.scale, b.shift)
    if plan is not None and sk[0] > 0:
        plan.add(ws, dw, sk[0], ks * ks, Cout, cout_real if cout_real else Cout, Cin, accumulate)


# ---- conv3x3(nearest-upsample-x2(x)) with 32 output channels as four 2x2 phase convolutions (models/networks.py:251-256) ----
def pack_phase_weights(w, bias, dtype):
    """w OIHW fp32 [32, Cin, 3, 3] -> (fwd [4, 128, Cin], dgrad [4, Cin, 128], bias4 [128])"""
    O, I = w.shape[0], w.shape[1]
    assert O == 32 and tuple(w.shape[2:]) == (3, 3)
    fwd = torch.empty(4, 128, I, dtype=dtype, device=w.device)
    dg = torch.empty(4, I, 128, dtype=dtype, device=w.device)
    b4 = torch.empty(128, dtype=torch.float32, device=w.device)
    _call("dh_pack_phase_weights", _DT[dtype], P(w), P(bias), I, P(fwd), P(dg), P(b4), S())
    return fwd, dg, b4


def conv_up2_fwd(x, wfwd, bias4, act=ACT_NONE):
    """act(conv3x3(nearest-x2(x)) + bias): x [N, H, W, Cin] -> [N, 2H, 2W, 32]; the upsampled tensor is never materialised"""
    N, H, W, Cin = x.shape
    y = torch.empty(N, 2 * H, 2 * W, 32, dtype=x.dtype, device=x.device)
    key = "conv_phase<%s,up2_fwd>" % ("bf16" if x.dtype == torch.bfloat16 else "f32")         # its own class: KS = 2 launches
    with _Prof(key, 2.0 * N * 4 * H * W * 32 * Cin * 9, _nb(x, y, wfwd)):                       # algorithmic FLOPs (of the 3x3)
        _call("dh_conv2d_fwd", dt(x), P(x), P(wfwd), P(y), P(bias4), _vp(0), _vp(0), N, H, W, Cin, H, W, 128, 128, 2, 1, 1, act,
              0, 0, _vp(0), 1, *_gate_args(None), *_bn_in_args(None), 1, _vp(0), S())
    return y


def pack_s2_dgrad_phase_weights(w, dtype):
    """OIHW fp32 [Co, Ci, 3, 3] of a stride-2 conv -> [4, 4 * Ci, Co] phase weights of its data gradient"""
    Co, Ci = w.shape[0], w.shape[1]
    out = torch.empty(4, 4 * Ci, Co, dtype=dtype, device=w.device)
    _call("dh_pack_s2_dgrad_phase_weights", _DT[dtype], P(w), Co, Ci, P(out), S())
    return out


def conv3x3s2_dgrad(dy, wphase, cin, coarse_residual=None, alg_flops=0):
    """data gradient of a 3x3 / stride-2 / pad-1 convolution from dy [N, OH, OW, Co] straight to [N, 2 OH, 2 OW, cin]: four
    output-parity phases (1 + 2 + 2 + 4 of the 9 taps), no zero-inserted tensor; coarse_residual [N, OH, OW, cin] (the data
    gradient of a parallel 1x1 stride-2 convolution) lands on the even-even positions"""
    N, OH, OW, Co = dy.shape
    dx = torch.empty(N, 2 * OH, 2 * OW, cin, dtype=dy.dtype, device=dy.device)
    key = "conv_phase<%s,s2_dgrad>" % ("bf16" if dy.dtype == torch.bfloat16 else "f32")
    with _Prof(key, alg_flops if alg_flops else 2.0 * N * OH * OW * Co * cin * 9, _nb(dy, dx, wphase, coarse_residual)):
        _call("dh_conv2d_fwd", dt(dy), P(dy), P(wphase), P(dx), _vp(0), P(coarse_residual), _vp(0), N, OH, OW, Co, OH, OW,
              4 * cin, 4 * cin, 2, 1, 1, ACT_NONE, 0, 0, _vp(0), 1, *_gate_args(None), *_bn_in_args(None), 1, _vp(0), S())
    return dx


def conv_up2_dgrad(dy, wdgrad, cin):
    """gradient of conv_up2_fwd with respect to x: dy [N, 2H, 2W, 32] -> [N, H, W, cin]"""
    N, H2, W2, C = dy.shape
    assert C == 32 and H2 % 2 == 0 and W2 % 2 == 0 and (cin % 64 == 0 or cin == 32)
    H, W = H2 // 2, W2 // 2
    dx = torch.empty(N, H, W, cin, dtype=dy.dtype, device=dy.device)
    key = "conv_phase<%s,up2_dgrad>" % ("bf16" if dy.dtype == torch.bfloat16 else "f32")
    with _Prof(key, 2.0 * N * H2 * W2 * 32 * cin * 9, _nb(dy, dx, wdgrad)):
        _call("dh_conv2d_fwd", dt(dy), P(dy), P(wdgrad), P(dx), _vp(0), _vp(0), _vp(0), N, H, W, 128, H, W, cin, cin, 2, 1, 1,
              ACT_NONE, 0, 0, _vp(0), 1, *_gate_args(None), *_bn_in_args(None), 2, _vp(0), S())
    return dx


def conv_up2_wgrad(x, dy, dw, accumulate=True, use_tr=True):
    """dw (OIHW fp32 [32, Cin, 3, 3]) (+)= weight gradient of conv_up2_fwd: four per-phase 2x2 gradients (one launch), their
    split-K reduce (with the pass's other reduces when a WgradPlan is active), then the tap combine"""
    N, H, W, Cin = x.shape
    L = _lib.lib()
    plan, own = _WGRAD_PLAN, False
    if plan is None:
        plan, own = WgradPlan(x.device), True
        plan.__enter__()
    try:
        ws = plan.slab(L.dh_conv2d_wgrad_phase_workspace_size(N, H, W, Cin))
        dwab = plan.slab(4 * 32 * Cin * 4 * 4).view(torch.float32)
        sk = (ctypes.c_int * 1)()       # int* splitk_out
        with _Prof("conv_wgrad<%s,ks3,s1>" % ("bf16" if x.dtype == torch.bfloat16 else "f32"),
                   2.0 * N * 4 * H * W * 32 * Cin * 9, _nb(x, dy)):
            _call("dh_conv2d_wgrad_phase", dt(x), P(x), P(dy), N, H, W, Cin, use_tr, P(ws), sk, S())
        per = sk[0] * 4 * 32 * Cin * 4            # bytes of one phase's slabs
        for ph in range(4):
            plan.add(ws[ph * per:], dwab[ph * 32 * Cin * 4:], sk[0], 4, 32, 32, Cin, False)
        plan.post.append(lambda: _call("dh_phase_wgrad_combine", P(dwab), P(dw), Cin, accumulate, S()))
        if own:
            plan.run()
    finally:
        if own:
            plan.__exit__()


def linear_wgrad(x2d, dy2d, dw, accumulate=False, images=1, per_image=False, use_tr=True):
    rows, Cin = x2d.shape
    Cout = dy2d.shape[1]
    rpi = rows // images
    Hh = cdiv(rpi, 16)
    groups = images if per_image else 1
    L = _lib.lib()
    nbytes = L.dh_conv2d_wgrad_workspace_size(images, Hh, 16, Cin, Cout, 1, groups)
    ws = workspace(nbytes, x2d.device)
    assert images == 1 or rpi % 16 == 0
    _call("dh_conv2d_wgrad", dt(x2d), P(x2d), P(dy2d), P(dw), accumulate, images, Hh, 16, Cin, Hh, 16, Cout, 1, 1, 0, groups, rpi,
          use_tr, 0, 0, 1, P(ws), S())


def add_coarse_(x, coarse):
    """x[n, 2y, 2x, :] += coarse[n, y, x, :] in place (the coarse-grid data gradient of a 1x1 stride-2 convolution)"""
    N, H, W, C = x.shape
    n2, OH, OW, c2 = coarse.shape
    assert n2 == N and c2 == C and x.dtype == coarse.dtype and x.is_contiguous() and coarse.is_contiguous()
    _call("dh_add_coarse", dt(x), P(x), P(coarse), N, OH, OW, H, W, C, S())
    return x


def zero_insert2(dy, H, W):
    N, OH, OW, C = dy.shape
    z = torch.empty(N, H, W, C, dtype=dy.dtype, device=dy.device)
    _call("dh_zero_insert2", dt(dy), P(dy), P(z), N, OH, OW, H, W, C, S())
    return z


# ---- stem ----------------------------------------------------------------------------------------
def stem_space_to_depth(x_nchw, dtype):
    N, C, H, W = x_nchw.shape
    assert C == 3
    cp = chunk_channels(dtype)
    y = torch.empty(N, H // 2, W // 2, cp, dtype=dtype, device=x_nchw.device)
    _call("dh_stem_space_to_depth", _DT[dtype], P(x_nchw), P(y), N, H, W, cp, S())
    return y


def stem_pack_weight(w, dtype, out_scale=None):
    O = w.shape[0]
    cp = chunk_channels(dtype)
    out = torch.empty(16, O, cp, dtype=dtype, device=w.device)
    _call("dh_stem_pack_weight", _DT[dtype], P(w), P(out_scale), P(out), O, cp, S())
    return out


def stem7_fwd(x1, x2, w, out_scale=None, bias=None, relu=False, want_stats=False, want_xs=False, groups=1):
    """7x7/2 stem on the NCHW fp32 images of both streams (x2 may be None) -> (y bf16 NHWC [N,H/2,W/2,64], stats, xs16)"""
    B, C, H, W = x1.shape
    assert C == 3 and x1.dtype == torch.float32 and x1.is_contiguous() and (x2 is None or (x2.shape == x1.shape and x2.is_contiguous()))
    N = B if x2 is None else 2 * B
    y = torch.empty(N, H // 2, W // 2, 64, dtype=torch.bfloat16, device=x1.device)
    nt = _lib.lib().dh_stem7_fwd_num_slots(N, H, W, groups)
    stats = torch.empty(2, 64, nt, dtype=torch.float32, device=x1.device) if want_stats else None
    xs = torch.empty(N, H // 2, W // 2, 16, dtype=torch.bfloat16, device=x1.device) if want_xs else None
    with _Prof("stem7_fwd", 2.0 * N * (H // 2) * (W // 2) * 64 * 147, _nb(x1, x2, y, xs)):
        _call("dh_stem7_fwd", P(x1), P(x2), B, N, H, W, P(w), P(out_scale), P(bias), relu, P(y), P(stats), groups, P(xs), S())
    return y, stats, xs


def stem_pool_bn_bwd(arg, dpool, y, scale, shift, mean, invstd, gamma, dgamma, dbeta, groups, accumulate=True, extra=None):
    """maxpool backward + ReLU mask + BatchNorm-backward sums of the stem's tail in one pass -> (d masked, coef [groups,3,C]).
    extra: a second gradient of the pre-pool activation (same shape as y), added before the mask"""
    N, H, W, C = y.shape
    d = torch.empty_like(y)
    coef = torch.empty(groups, 3, C, dtype=torch.float32, device=y.device)
    L = _lib.lib()
    ws = workspace(L.dh_stem_pool_bn_bwd_workspace_size(C, groups), y.device)
    assert extra is None or (extra.shape == y.shape and extra.dtype == y.dtype)
    with _Prof("bn_bwd", 0, _nb(arg, dpool, y, d, extra)):
        _call("dh_stem_pool_bn_bwd_plus", P(arg), P(dpool), P(extra), P(y), P(scale), P(shift), P(mean), P(invstd), P(gamma), N,
              H, W, C, groups, P(d), P(coef), P(dgamma), P(dbeta), accumulate, P(ws), S())
    return d, coef


def stem_wgrad(x_s2d, dy, dw, accumulate=False, use_tr=True, bn=None):
    """bn = (y, coef, groups): dy is the masked gradient of the BatchNorm output; BatchNorm backward is applied on load"""
    N, H2, W2, cp = x_s2d.shape
    O = dy.shape[-1]
    dw2 = torch.empty(O, 16, 4, 4, dtype=torch.float32, device=dy.device)     # 12 real + 4 zero channels
    if bn is not None:
        y, coef, groups = bn
        assert cp == 16 and O == 64 and y.shape == dy.shape
        L = _lib.lib()
        ws = workspace(L.dh_conv2d_wgrad_workspace_size(N, H2, W2, 16, O, 4, 1), dy.device)
        with _Prof("conv_wgrad<bf16,ks4,s1>", 2.0 * N * H2 * W2 * O * 16 * 16, _nb(x_s2d, dy, y)):
            _call("dh_stem_wgrad_bn", P(x_s2d), P(dy), P(y), P(coef), groups, N, H2, W2, P(dw2), use_tr, P(ws), S())
    else:
        conv2d_wgrad(x_s2d, dy, dw2, ks=4, stride=1, pad=2, use_tr=use_tr, cin=16, defer=False)     # dw2 is unpacked next
    _call("dh_stem_unpack_grad", P(dw2), P(dw), O, 16, accumulate, S())


# ---- normalisation -------------------------------------------------------------------------------
def bn_finalize(stats, C, groups, count, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, nbt=None):
    """nbt: the layer's int64 num_batches_tracked buffer (device), incremented by `groups` in the same launch"""
    _, cp, nt = stats.shape
    dev = stats.device
    mean = torch.empty(groups, C, dtype=torch.float32, device=dev)
    invstd, scale, shift = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
    _call("dh_bn_finalize", P(stats), nt, cp, C, groups, float(count), P(gamma), P(beta), P(running_mean), P(running_var),
          momentum, eps, P(mean), P(invstd), P(scale), P(shift), P(nbt), S())
    return mean, invstd, scale, shift


def bn_eval_params(gamma, beta, rm, rv, eps=1e-5):
    C = gamma.numel()
    scale = torch.empty(1, C, dtype=torch.float32, device=gamma.device)
    shift = torch.empty_like(scale)
    _call("dh_bn_eval_params", P(gamma), P(beta), P(rm), P(rv), eps, C, P(scale), P(shift), S())
    return scale, shift


RELU_BITS = os.environ.get("DAHITRA_NO_RELU_BITS", "0") != "1"      # A/B switch of bn_apply(want_bits=True)


BN_APPLY_LAUNCHES = 0       # bn_apply launches issued (or recorded) by this process, and how many of them only wrote the
BN_SHORTCUT_APPLIES = 0     # BatchNorm output of a shortcut (BnResidual.materialize): what tests count
BN_DRES_REQUESTS = 0        # bn_bwd calls asked for the masked copy of their gradient (want_dres=True)


class BnResidual:
    """The BatchNorm output of a block's shortcut (no ReLU) that exists only as (conv output y, per-group scale / shift):
    bn_apply(residual=<BnResidual>) forms T(y * scale + shift) while it loads the residual (dh_bn_apply_res_affine), bit for
    bit what materialize() -- the bn_apply launch it stands for -- stores.  Any other consumer calls materialize()."""
    __slots__ = ("y", "scale", "shift", "groups")

    def __init__(self, y, scale, shift, groups):
        self.y, self.scale, self.shift, self.groups = y, scale, shift, groups

    @property
    def shape(self):
        return self.y.shape

    @property
    def dtype(self):
        return self.y.dtype

    def materialize(self):
        global BN_SHORTCUT_APPLIES
        BN_SHORTCUT_APPLIES += 1
        return bn_apply(self.y, self.scale, self.shift, self.groups)


def bn_apply(x, scale, shift, groups=1, act=ACT_NONE, residual=None, want_bits=False):
    """want_bits (ReLU): also returns the ReLU mask of y as one byte per 16-byte piece (dh_bn_apply_bits) -- what bn_bwd(bits=...)
    reads in place of the post-activation tensor; None with DAHITRA_NO_RELU_BITS=1.  residual may be a BnResidual."""
    global BN_APPLY_LAUNCHES
    BN_APPLY_LAUNCHES += 1
    C = x.shape[-1]
    npix = x.numel() // C
    y = torch.empty_like(x)
    bits = None
    v = 8 if x.dtype == torch.bfloat16 else 4
    if want_bits and RELU_BITS and act == ACT_RELU and C % v == 0:
        bits = torch.empty(x.numel() // v, dtype=torch.uint8, device=x.device)
    if isinstance(residual, BnResidual):
        r = residual
        assert r.y.shape == x.shape and r.y.dtype == x.dtype and r.groups == groups
        with _Prof("bn_apply", 0, _nb(x, r.y, y)):
            _call("dh_bn_apply_res_affine", dt(x), P(x), P(r.y), P(r.scale), P(r.shift), P(y), P(scale), P(shift), npix, C, groups,
                  act, P(bits), S())
        return (y, bits) if want_bits else y
    with _Prof("bn_apply", 0, _nb(x, residual, y)):
        if bits is not None:
            _call("dh_bn_apply_bits", dt(x), P(x), P(residual), P(y), P(scale), P(shift), npix, C, groups, act, P(bits), S())
        else:
            _call("dh_bn_apply", dt(x), P(x), P(residual), P(y), P(scale), P(shift), npix, C, groups, act, S())
    return (y, bits) if want_bits else y


_BN_SYNC = {}
BN_BWD_PERSIST = os.environ.get("DAHITRA_NO_PERSIST_BN", "0") != "1"      # True: where faster; "force": wherever supported (tests)
if os.environ.get("DAHITRA_PERSIST_BN_FORCE", "0") == "1":
    BN_BWD_PERSIST = "force"
_PERSIST_BLOCK = 0          # > 0: inside no_persist_bn(), its only writer -- another stream may run beside the launches made here
BN_PERSIST_LAUNCHES = 0     # persistent launches issued (or recorded into a graph) by this process: what tests assert the guard on


class no_persist_bn:
    """`with ops.no_persist_bn():` BatchNorm backward takes the two-pass kernels.  The persistent form (dh_bn_bwd_persist)
    holds a device-wide barrier across 256 one-per-CU workgroups: it must not be launched where a kernel of another
    stream -- the RCCL all-reduce of the overlapped data-parallel step -- may hold CUs."""

    def __enter__(self):
        global _PERSIST_BLOCK
        _PERSIST_BLOCK += 1

    def __exit__(self, *exc):
        global _PERSIST_BLOCK
        _PERSIST_BLOCK -= 1
        return False


def bn_sync_words(device):
    """the zeroed state of dh_bn_bwd_persist's device-wide barrier + fixed-point accumulators: one block per (device, stream)
    -- two streams must never share the counters -- that lives forever (captured HIP graphs point at it)"""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    t = _BN_SYNC.get(key)
    if t is None:
        t = _BN_SYNC[key] = torch.zeros(8192, dtype=torch.int32, device=device)
    return t


def bn_persist_check(device=None):
    """reads and clears the error word of every persistent-BatchNorm sync block of `device` (all devices if None): raises
    HipLibraryError when a launch since the last check timed out at its device-wide barrier or met a non-finite sum (the
    affected step's dgamma / dbeta are NaN by then).  One 4-byte device-to-host copy per block: call it every N steps."""
    bad = []
    for (dev, stream), t in list(_BN_SYNC.items()):
        if device is not None and dev != str(device):
            continue
        word = _lib.lib().dh_bn_bwd_persist_status(P(t), _vp(torch.cuda.current_stream(t.device).cuda_stream))
        if word:
            bad.append((dev, stream, word))
    if bad:
        raise _lib.HipLibraryError(
            "dahitra_amd: the persistent BatchNorm backward failed (device, stream, word): %s -- bit 0: its device-wide "
            "barrier timed out (another stream's kernel kept workgroups out: set DAHITRA_NO_PERSIST_BN=1 or keep such "
            "launches inside ops.no_persist_bn()), bit 1: non-finite gradient sums; the gradients of that step are NaN" % bad)


def bn_bwd(dout, out_relu, x, mean, invstd, gamma, dgamma, dbeta, groups=1, accumulate=False, want_dres=False,
           mask_scale=None, mask_shift=None, bits=None):
    """bits: the ReLU mask bytes of bn_apply(want_bits=True), used in place of out_relu"""
    C = x.shape[-1]
    npix = x.numel() // C
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    if want_dres:
        global BN_DRES_REQUESTS
        BN_DRES_REQUESTS += 1
    L = _lib.lib()
    ws = workspace(L.dh_bn_bwd_workspace_size(npix, C, groups), x.device)
    if BN_BWD_PERSIST and not _PERSIST_BLOCK and \
            (L.dh_bn_bwd_persist_preferred if BN_BWD_PERSIST is True else L.dh_bn_bwd_persist_supported)(dt(x), npix, C, groups):
        # one persistent launch, tensors held on chip across a device-wide barrier: every tensor is read once
        global BN_PERSIST_LAUNCHES
        BN_PERSIST_LAUNCHES += 1
        with _Prof("bn_bwd", 0, _nb(dout, bits if bits is not None else out_relu, x) + _nb(dx, dres)):
            if bits is not None:
                _call("dh_bn_bwd_persist_bits", P(dout), P(bits), P(x), P(mean), P(invstd), P(gamma), npix, C, groups, P(dx),
                      P(dres), P(dgamma), P(dbeta), accumulate, P(ws), P(bn_sync_words(x.device)), S())
            else:
                _call("dh_bn_bwd_persist", P(dout), P(out_relu), P(x), P(mean), P(invstd), P(gamma), npix, C, groups, P(dx),
                      P(dres), P(dgamma), P(dbeta), accumulate, P(mask_scale), P(mask_shift), P(ws), P(bn_sync_words(x.device)), S())
        return (dx, dres) if want_dres else dx
    # two passes (reduce, apply): dout / x (/ out) are read twice, dx (/ dres) written once
    with _Prof("bn_bwd", 0, 2 * _nb(dout, bits if bits is not None else out_relu, x) + _nb(dx, dres)):
        if bits is not None:
            _call("dh_bn_bwd_bits", dt(x), P(dout), P(bits), P(x), P(mean), P(invstd), P(gamma), npix, C, groups, P(dx), P(dres),
                  P(dgamma), P(dbeta), accumulate, P(ws), S())
        else:
            _call("dh_bn_bwd", dt(x), P(dout), P(out_relu), P(x), P(mean), P(invstd), P(gamma), npix, C, groups, P(dx), P(dres),
                  P(dgamma), P(dbeta), accumulate, P(mask_scale), P(mask_shift), P(ws), S())
    return (dx, dres) if want_dres else dx


def bn_bwd_from_partials(g, x, partial, mean, invstd, gamma, dgamma, dbeta, groups=1, accumulate=False):
    """BN backward fed by a gated data-gradient launch (conv2d(..., gate=...)): g already carries the ReLU mask"""
    C = x.shape[-1]
    npix = x.numel() // C
    _, cp, nt = partial.shape
    assert cp == C and g.shape == x.shape
    dx = torch.empty_like(x)
    ws = workspace(groups * 2 * C * 4, x.device)
    _call("dh_bn_bwd_from_partials", dt(x), P(g), P(x), P(partial), nt, P(mean), P(invstd), P(gamma), npix, C, groups, P(dx),
          P(dgamma), P(dbeta), accumulate, P(ws), S())
    return dx


def layernorm(x2d, gamma, beta, eps=1e-5, want_stats=True):
    rows, C = x2d.shape
    y = torch.empty_like(x2d)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x2d.device) if want_stats else None
    _call("dh_layernorm_fwd", dt(x2d), P(x2d), P(gamma), P(beta), P(y), P(stats), rows, C, eps, S())
    return (y, stats) if want_stats else y


def layernorm_bwd(dy, x2d, stats, gamma, dgamma, dbeta, dx_add=None, accumulate=False):
    rows, C = x2d.shape
    dx = torch.empty_like(x2d)
    L = _lib.lib()
    ws = workspace(L.dh_layernorm_bwd_workspace_size(rows), x2d.device)
    _call("dh_layernorm_bwd", dt(x2d), P(dy), P(x2d), P(stats), P(gamma), P(dx), P(dx_add), P(dgamma), P(dbeta), accumulate, rows,
          C, P(ws), S())
    return dx


# ---- pointwise -----------------------------------------------------------------------------------
def nchw_to_nhwc(x, dtype, cpad=0):
    N, C, H, W = x.shape
    cp = max(C, cpad)
    y = torch.empty(N, H, W, cp, dtype=dtype, device=x.device)
    _call("dh_nchw_to_nhwc", _DT[dtype], P(x), P(y), N, C, H * W, cp, S())
    return y


def head_dgrad3x3(dy, w_oihw, ncls, relu_out=None):
    """data gradient of the 3x3 class head (32 -> ncls): dy [N,H,W,CP] with one 16-byte piece per pixel -> [N,H,W,32].
    relu_out: the head's input is the output of a ReLU (given here); the gradient comes back already masked by it"""
    N, H, W, CP = dy.shape
    assert w_oihw.shape == (ncls, 32, 3, 3) and w_oihw.dtype == torch.float32
    dx = torch.empty(N, H, W, 32, dtype=dy.dtype, device=dy.device)
    if relu_out is not None:
        if dy.dtype == torch.bfloat16 and CP == 8 and ncls <= 2:
            _call("dh_head_dgrad3x3_relu", P(dy), P(w_oihw), ncls, P(relu_out), P(dx), N, H, W, S())
            return dx
        return act_bwd(head_dgrad3x3(dy, w_oihw, ncls), relu_out, ACT_RELU)
    _call("dh_head_dgrad3x3", dt(dy), P(dy), CP, P(w_oihw), ncls, P(dx), N, H, W, S())
    return dx


def head_dgrad3x3_bn(dy, w_oihw, ncls, y, scale, shift, mean, invstd, groups):
    """head_dgrad3x3 gated for the BatchNorm + ReLU behind its 32 output channels: returns (g masked [N,H,W,32], partials
    [2, 32, blocks]) for bn_bwd_from_partials"""
    N, H, W, CP = dy.shape
    assert w_oihw.shape == (ncls, 32, 3, 3) and dy.dtype == torch.bfloat16 and CP == 8 and ncls <= 2 and y.shape == (N, H, W, 32)
    g = torch.empty(N, H, W, 32, dtype=dy.dtype, device=dy.device)
    nb = _lib.lib().dh_head_dgrad3x3_bn_blocks(N, H, W, groups)
    partial = torch.empty(2, 32, nb, dtype=torch.float32, device=dy.device)
    with _Prof("bn_bwd", 0, _nb(dy, y, g)):
        _call("dh_head_dgrad3x3_bn", P(dy), P(w_oihw), ncls, P(y), P(scale), P(shift), P(mean), P(invstd), groups, P(g),
              P(partial), N, H, W, S())
    return g, partial


def head_dlogits_pack(dl_nchw, dtype=torch.bfloat16):
    """dlogits [N, ncls <= 8, H, W] fp32 -> the zero-bordered class map of head_bn_bwd / head_relu_bwd (int32 words of bf16
    pairs, _head_dlp_shape); dtype float32 (the bf16x3 mode): the plane of bf16 heads, then the plane of bf16 remainders"""
    N, C, H, W = dl_nchw.shape
    assert C <= 8 and dl_nchw.dtype == torch.float32 and dl_nchw.is_contiguous()
    dlp = torch.empty(_head_dlp_shape(N, H, W, C, dtype), dtype=torch.int32, device=dl_nchw.device)
    _call("dh_head_dlogits_pack", _DT[dtype], P(dl_nchw), N, C, H, W, P(dlp), S())
    return dlp


def _head_dlp_shape(N, H, W, ncls, dtype):
    """[N, H + 2, W + 2] + (planes * words per piece,): a piece = 2 classes (one word) for ncls <= 2, 8 classes (4 words) above;
    one plane for bf16, two (heads, remainders) for the split fp32 form"""
    words = (1 if ncls <= 2 else 4) * (1 if dtype == torch.bfloat16 else 2)
    return (N, H + 2, W + 2) if words == 1 else (N, H + 2, W + 2, words)


def _head_dlp_ok(dlp, y, ncls):
    N, H, W, C = y.shape
    return dlp.dtype == torch.int32 and tuple(dlp.shape) == _head_dlp_shape(N, H, W, ncls, y.dtype) and C == 32 and \
        y.dtype in (torch.bfloat16, torch.float32)


def head_bn_bwd(dlp, w_oihw, ncls, y, scale, shift, mean, invstd, gamma, dgamma, dbeta, groups, accumulate=True, dw=None, db=None):
    """class head's data gradient + the backward of the BatchNorm + ReLU behind it without the gradient tensor in between
    (dh_head_bn_bwd): dlp = head_dlogits_pack(dlogits, y.dtype) -> the gradient of the pre-BatchNorm activation y [N,H,W,32].
    dw [ncls,32,3,3] / db [ncls]: the head convolution's own weight / bias gradient from the same pass.  y fp32: the bf16x3
    mode's arithmetic (three split bf16 products) -- not for the exact fp32 mode"""
    assert (dw is None) == (db is None) and (dw is None or (dw.shape == (ncls, 32, 3, 3) and dw.is_contiguous()))
    N, H, W, _ = y.shape
    assert w_oihw.shape == (ncls, 32, 3, 3) and ncls <= 8 and _head_dlp_ok(dlp, y, ncls)
    dx = torch.empty_like(y)
    ws = workspace(_lib.lib().dh_head_bn_bwd_workspace_size(N, H, W, groups), y.device)
    with _Prof("bn_bwd", 0, _nb(y, y, dx)):
        _call("dh_head_bn_bwd", dt(y), P(dlp), P(w_oihw), ncls, P(y), P(scale), P(shift), P(mean), P(invstd), P(gamma), groups,
              P(dx), P(dgamma), P(dbeta), P(dw), P(db), 1 if accumulate else 0, N, H, W, P(ws), S())
    return dx


def head_relu_bwd(dlp, w_oihw, ncls, relu_out, dw, db, accumulate=True):
    """class head behind a ReLU: data gradient (masked by relu_out > 0) + the head's weight / bias gradient in one pass over
    relu_out [N,H,W,32] (dh_head_relu_bwd); dlp = head_dlogits_pack(dlogits, relu_out.dtype)"""
    N, H, W, C = relu_out.shape
    assert w_oihw.shape == (ncls, 32, 3, 3) and ncls <= 8 and _head_dlp_ok(dlp, relu_out, ncls) and dw.shape == (ncls, 32, 3, 3) and \
        dw.is_contiguous()
    dx = torch.empty_like(relu_out)
    ws = workspace(_lib.lib().dh_head_bn_bwd_workspace_size(N, H, W, 1), dlp.device)
    with _Prof("act_bwd", 0, _nb(relu_out, dx)):
        _call("dh_head_relu_bwd", dt(relu_out), P(dlp), P(w_oihw), ncls, P(relu_out), P(dx), P(dw), P(db), 1 if accumulate else 0,
              N, H, W, P(ws), S())
    return dx


def nhwc_to_nchw(x):
    N, H, W, C = x.shape
    y = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    _call("dh_nhwc_to_nchw", dt(x), P(x), P(y), N, C, H * W, S())
    return y


def copy_channels(src, sc0, dst, dc0, cn):
    Cs, Cd = src.shape[-1], dst.shape[-1]
    Pn = src.numel() // Cs
    _call("dh_copy_channels", dt(src), P(src), Cs, sc0, P(dst), Cd, dc0, cn, Pn, S())


# ---- small element-wise launches of independent levels, recorded and issued as one job-table launch (dh_ew_multi) ----
EW_ADD_POS, EW_CAT_HALVES, EW_SPLIT_HALVES, EW_ABSDIFF_HALVES, EW_ABSDIFF_HALVES_BWD, EW_ADD_POS_BWD = 1, 2, 3, 4, 5, 6
EW_MAXJ = 12
_EW_BATCH = None         # while an EncoderBatch(ew=True) is open: [(op, a, b, c, i0, i1, l0)] of the recorded calls (tensors kept alive)


def _ew_record(op, a, b, c, i0, i1, l0):
    """True: the call was recorded (its result is valid after the batch's next launch)"""
    if _EW_BATCH is None:
        return False
    if len(_EW_BATCH) == EW_MAXJ:
        ew_flush()
    _EW_BATCH.append((op, a, b, c, int(i0), int(i1), int(l0)))
    return True


def ew_flush():
    """issue what has been recorded (one launch); a no-op without pending jobs"""
    if not _EW_BATCH:
        return
    n = len(_EW_BATCH)
    ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    ops_ = (ctypes.c_int * n)(*[j[0] for j in _EW_BATCH])
    a = (ctypes.c_void_p * n)(*[ptr(j[1]) for j in _EW_BATCH])
    b = (ctypes.c_void_p * n)(*[ptr(j[2]) for j in _EW_BATCH])
    c = (ctypes.c_void_p * n)(*[ptr(j[3]) for j in _EW_BATCH])
    i0 = (ctypes.c_int * n)(*[j[4] for j in _EW_BATCH])
    i1 = (ctypes.c_int * n)(*[j[5] for j in _EW_BATCH])
    l0 = (ctypes.c_long * n)(*[j[6] for j in _EW_BATCH])
    _call("dh_ew_multi", n, ops_, a, b, c, i0, i1, l0, S())
    del _EW_BATCH[:]


def cat_halves(t):
    """torch.cat([t[:B], t[B:]], channel) of a contiguous [2B, H, W, C] tensor, one launch"""
    n, h, w, c = t.shape
    cat = torch.empty(n // 2, h, w, 2 * c, dtype=t.dtype, device=t.device)
    assert t.is_contiguous()
    if t.dtype == torch.bfloat16 and c % 8 == 0 and _ew_record(EW_CAT_HALVES, t, None, cat, c, 0, (n // 2) * h * w):
        return cat
    _call("dh_cat_halves", dt(t), P(t), P(cat), c, (n // 2) * h * w, 0, S())
    return cat


def split_halves(cat):
    """the inverse: [B, H, W, 2C] -> [2B, H, W, C] (the gradient of cat_halves)"""
    n, h, w, c2 = cat.shape
    t = torch.empty(2 * n, h, w, c2 // 2, dtype=cat.dtype, device=cat.device)
    assert cat.is_contiguous()
    if cat.dtype == torch.bfloat16 and (c2 // 2) % 8 == 0 and _ew_record(EW_SPLIT_HALVES, cat, None, t, c2 // 2, 0, n * h * w):
        return t
    _call("dh_cat_halves", dt(cat), P(t), P(cat), c2 // 2, n * h * w, 1, S())
    return t


def add(a, b):
    y = torch.empty_like(a)
    _call("dh_add", dt(a), P(a), P(b), P(y), a.numel(), S())
    return y


def add_pos(x, pos):
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    assert x.is_contiguous() and pos.is_contiguous()
    if x.dtype == torch.bfloat16 and C % 8 == 0 and _ew_record(EW_ADD_POS, x, pos, y, N, C, H * W):
        return y
    _call("dh_add_pos", dt(x), P(x), P(pos), P(y), N, H * W, C, S())
    return y


def add_pos_bwd(dy, dpos, accumulate=False):
    N, H, W, C = dy.shape
    assert dy.is_contiguous() and dpos.is_contiguous()
    if dy.dtype == torch.bfloat16 and C == 32 and _ew_record(EW_ADD_POS_BWD, dy, None, dpos, N, int(accumulate), H * W):
        return
    _call("dh_add_pos_bwd", dt(dy), P(dy), P(dpos), N, H * W, C, accumulate, S())


def act_bwd(dy, ref, act):
    dx = torch.empty_like(dy)
    _call("dh_act_bwd", dt(dy), P(dy), P(ref), P(dx), dy.numel(), act, S())
    return dx


def maxpool(x, want_arg=False, bn=None):
    """bn = (scale, shift, groups): x is a pre-BatchNorm tensor, relu(x * scale + shift) is applied on load"""
    N, H, W, C = x.shape
    y = torch.empty(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=x.dtype, device=x.device)
    arg = torch.empty(y.shape, dtype=torch.uint8, device=x.device) if want_arg else None
    sc, sh, groups = bn if bn is not None else (None, None, 0)
    _call("dh_maxpool3x3s2_fwd", dt(x), P(x), P(y), P(arg), N, H, W, C, P(sc), P(sh), groups, S())
    return (y, arg) if want_arg else y


def maxpool_bwd(arg, dy, in_shape):
    N, H, W, C = in_shape
    dx = torch.empty(N, H, W, C, dtype=dy.dtype, device=dy.device)
    _call("dh_maxpool3x3s2_bwd", dt(dy), P(arg), P(dy), P(dx), N, H, W, C, S())
    return dx


def upsample2(x):
    N, H, W, C = x.shape
    y = torch.empty(N, 2 * H, 2 * W, C, dtype=x.dtype, device=x.device)
    _call("dh_upsample2_nearest_fwd", dt(x), P(x), P(y), N, H, W, C, S())
    return y


def upsample2_bwd(dy):
    N, H2, W2, C = dy.shape
    dx = torch.empty(N, H2 // 2, W2 // 2, C, dtype=dy.dtype, device=dy.device)
    _call("dh_upsample2_nearest_bwd", dt(dy), P(dy), P(dx), N, H2 // 2, W2 // 2, C, S())
    return dx


def absdiff_upsample4(a, b):
    N, H, W, C = a.shape
    y = torch.empty(N, 4 * H, 4 * W, C, dtype=a.dtype, device=a.device)
    _call("dh_absdiff_upsample4_fwd", dt(a), P(a), P(b), P(y), N, H, W, C, S())
    return y


def absdiff_upsample4_bwd(a, b, dy):
    N, H, W, C = a.shape
    da, db = torch.empty_like(a), torch.empty_like(b)
    _call("dh_absdiff_upsample4_bwd", dt(a), P(a), P(b), P(dy), P(da), P(db), N, H, W, C, S())
    return da, db


def conv3x3_dgrad_through_up4(dy, wdgrad, a, b, da=None, db=None):
    """backward of conv3x3(bilinear_x4(|a - b|)) with respect to a and b, from dy [N, 4H, 4W, K] (gradient of the conv's
    output) and the conv's data-gradient pack [9, 32, K]: the fine-grid gradient [N, 4H, 4W, 32] is never written -- the
    convolution reduces each tile to the coarse pixels it interpolates from, a second small launch sums and applies the sign.
    Returns (da, db) like a, b [N, H, W, 32] bf16."""
    N, H, W, C = a.shape
    assert C == 32 and a.dtype == torch.bfloat16 and dy.shape[:3] == (N, 4 * H, 4 * W) and wdgrad.shape[-2] == 32
    L = _lib.lib()
    partial = torch.empty(L.dh_conv3x3_dgrad_up4_partial_floats(N, 4 * H, 4 * W), dtype=torch.float32, device=a.device)
    with _Prof("conv_mfma<bf16,ks3,s1,nt32>", 2.0 * N * 16 * H * W * 32 * dy.shape[-1] * 9, _nb(dy, wdgrad, partial)):
        _call("dh_conv3x3_dgrad_up4", dt(dy), P(dy), P(wdgrad), N, 4 * H, 4 * W, dy.shape[-1], P(partial), S())
    da = torch.empty_like(a) if da is None else da
    db = torch.empty_like(b) if db is None else db
    _call("dh_absdiff_up4_combine", P(partial), P(a), P(b), P(da), P(db), N, H, W, S())
    return da, db


def absdiff(a, b):
    y = torch.empty_like(a)
    _call("dh_absdiff", dt(a), P(a), P(b), P(y), a.numel(), S())
    return y


def absdiff_bwd(a, b, dy, da, db, accumulate=True):
    _call("dh_absdiff_bwd", dt(a), P(a), P(b), P(dy), P(da), P(db), a.numel(), accumulate, S())


def colsum(x2d, out, accumulate=False):
    C = x2d.shape[-1]
    Pn = x2d.numel() // C
    ws = workspace(1024 * C * 4 + 1024, x2d.device)          # up to 1024 partial rows
    _call("dh_colsum", dt(x2d), P(x2d), Pn, C, P(out), accumulate, P(ws), S())


def cast_from_f32(src, dtype):
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    _call("dh_cast_from_f32", _DT[dtype], P(src), P(dst), src.numel(), S())
    return dst


def cast_to_f32(src, dst=None, accumulate=False):
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    _call("dh_cast_to_f32", dt(src), P(src), P(dst), src.numel(), accumulate, S())
    return dst


# ---- token side ----------------------------------------------------------------------------------
def tokenizer_fwd(x, wa, pos, B, L):
    """x [S, H, W, 32]; returns (tok_cat [B, 2L, 32] fp32 written for the S/B streams present, saved).  Tokens are
    fp32 in every compute mode (csrc/tokens.hip header)."""
    Sn, H, W, C = x.shape
    HW = H * W
    dev = x.device
    logits = torch.empty(Sn * HW, L, dtype=torch.float32, device=dev)
    stats = torch.empty(Sn, L, 2, dtype=torch.float32, device=dev)
    pooled = torch.empty(Sn, L, 32, dtype=torch.float32, device=dev)
    tok = torch.empty(B, 2 * L, 32, dtype=torch.float32, device=dev)
    nws = _lib.lib().dh_tokenizer_fwd_workspace_size(Sn, HW, L)
    args = lambda ws: (dt(x), P(x), P(wa), P(pos), Sn, B, HW, L, P(logits), P(stats), P(pooled), P(tok), P(ws), S())
    if _XPREP_BATCH is not None and _ENC_BATCH is not None:
        # recorded (EncoderBatch): issued with the other levels' tokenizers, right before the recorded encoder stacks that read
        # the tokens -- scratch of its own until then.  (A caller that reads `tok` with an immediate launch instead calls
        # flush_recorded_tokens() first: Engine.encoder's layer-wise path.)
        ws = torch.empty(max(int(nws), 1), dtype=torch.uint8, device=dev)
        _XPREP_BATCH.extend((ws, x, pos))
        _call("dh_tokenizer_fwd", *args(ws))
    else:
        with _XprepPaused():
            _call("dh_tokenizer_fwd", *args(workspace(nws, dev)))
    return tok, (logits, stats, pooled)


def flush_recorded_tokens():
    """inside an EncoderBatch: issue the recorded tokenizer / preparation forward launches now (their results are read next by
    a launch that is not a recorded one)"""
    if _XPREP_BATCH is not None:
        _call("dh_xprep_batch_launch_fwd", S())


def tokenizer_bwd(x, wa, saved, dtok_cat, dx_accum, dwa, dpos, B, L, accumulate=False):
    Sn, H, W, C = x.shape
    HW = H * W
    logits, stats, pooled = saved
    Lb = _lib.lib()
    nws = Lb.dh_tokenizer_bwd_workspace_size(Sn, HW, L)
    if _XPREP_BATCH is not None:          # recorded: dx_accum / dwa / dpos are valid after the EncoderBatch's next launch()
        ws = torch.empty(max(int(nws), 1), dtype=torch.uint8, device=x.device)
        _XPREP_BATCH.extend((ws, dtok_cat, dx_accum, dpos))
    else:
        ws = workspace(nws, x.device)
    assert dtok_cat.dtype == torch.float32
    _call("dh_tokenizer_bwd", dt(x), P(x), P(wa), Sn, B, HW, L, P(logits), P(stats), P(pooled), P(dtok_cat), P(dx_accum), P(dwa),
          P(dpos), accumulate, P(ws), S())


def prep_mfma_supported(dtype, Sn, L, heads, dim_head, HLP):
    return bool(_lib.lib().dh_xattn_prep_mfma_supported(_DT[dtype], Sn, L, heads, dim_head, HLP))


DEC_RECORD = None    # set to [] by bench.py for ONE eager step: every fused-decoder call (layer / stack, forward / backward /
                     # finalize) as {"kind", "rows", "depth", "mlp", "call"} in program order, with {"kind": "launch"} where an
                     # EncoderBatch issued what it had recorded -- bench.py re-issues them, grouped the same way, inside a recorded
                     # graph to time the attention blocks by themselves (the `attention` record of its line)


def _dec_recorded(kind, rows_of, depth_of, mlp_of):
    """decorator of the fused-decoder entry points: see DEC_RECORD"""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            if DEC_RECORD is not None:
                DEC_RECORD.append(dict(kind=kind, rows=rows_of(a), depth=depth_of(a), mlp=mlp_of(a, k),
                                       call=functools.partial(fn, *a, **k)))
            return fn(*a, **k)
        return wrapped
    return deco


class XattnPrep:
    """Per-image operands of the re-associated cross attention (see csrc/tokens.hip)."""

    def __init__(self, tok, bstride, sstride, B, Sn, L, heads, dim_head, ln_g, ln_b, wq, wkT, wvT, woT, dtype,
                 scale=32 ** -0.5, eps=1e-5, masters=None):
        """masters = (wk, wv, wo fp32 masters, wqT in `dtype`): lets the matrix-core form run where it serves the shape"""
        dev = tok.device
        assert tok.dtype == torch.float32, "tokens are fp32 in every compute mode"
        inner = heads * dim_head
        self.HLP = cdiv(heads * L, 32) * 32
        self.args = (bstride, sstride, B, Sn, L, heads, dim_head)
        self.scale = scale
        self.mn = torch.empty(Sn, L, 32, dtype=torch.float32, device=dev)
        self.mstats = torch.empty(Sn, L, 2, dtype=torch.float32, device=dev)
        self.k = torch.empty(Sn, L, inner, dtype=torch.float32, device=dev)
        self.v = torch.empty_like(self.k)
        self.kq = torch.empty(Sn, self.HLP, 32, dtype=dtype, device=dev)
        self.kqT = torch.empty(Sn, 32, self.HLP, dtype=dtype, device=dev)
        self.vo = torch.empty(Sn, self.HLP, 32, dtype=dtype, device=dev)
        self.voT = torch.empty(Sn, 32, self.HLP, dtype=dtype, device=dev)
        self.mfma = masters is not None and prep_mfma_supported(dtype, Sn, L, heads, dim_head, self.HLP)
        self._bwd_ops = (wq, woT, wkT, wvT)
        if self.mfma:
            wk, wv, wo, wqT = masters
            with _XprepPaused():
                _call("dh_xattn_prep_fwd_stack_mfma", P(tok), bstride, sstride, B, Sn, heads, dim_head, self.HLP, scale, eps, 1,
                      0, P(ln_g), P(ln_b), P(wk), P(wv), P(wo), P(wqT), P(self.mn), P(self.mstats), P(self.k), P(self.v),
                      P(self.kq), P(self.kqT), P(self.vo), P(self.voT), S())
            return
        _call("dh_xattn_prep_fwd", _DT[dtype], P(tok), bstride, sstride, B, Sn, L, heads, dim_head, self.HLP, scale, eps, P(ln_g),
              P(ln_b), P(wq), P(wkT), P(wvT), P(woT), P(self.mn), P(self.mstats), P(self.k), P(self.v), P(self.kq), P(self.kqT),
              P(self.vo), P(self.voT), S())


class _PrepView:
    """one layer of an XattnPrepStack, with the attributes of XattnPrep"""
    __slots__ = ("mn", "mstats", "k", "v", "kq", "kqT", "vo", "voT", "HLP", "args", "scale")


class XattnPrepStack:
    """XattnPrep for ALL layers of a decoder stack in one launch (they read the same tokens).  ln_g0 / ln_b0 / wq0 are
    the first layer's fp32 parameters, consecutive layers lie `param_stride` floats apart (the net's flat arena);
    wkT / wvT / woT are stacked [layers, 32 * inner] transposes in `dtype`."""

    def __init__(self, tok, bstride, sstride, B, Sn, L, heads, dim_head, layers, param_stride, ln_g0, ln_b0, wq0, wkT, wvT,
                 woT, dtype, scale=32 ** -0.5, eps=1e-5, masters=None, record=True):
        """masters = (wk0, wv0, wo0 fp32 masters of the first layer, stacked wqT): see XattnPrep.
        record=False: launch at once even inside an EncoderBatch (the caller's next launch is not a recorded one)"""
        dev = tok.device
        assert tok.dtype == torch.float32, "tokens are fp32 in every compute mode"
        inner = heads * dim_head
        self.layers, self.param_stride, self.dtype = layers, param_stride, dtype
        self.HLP = cdiv(heads * L, 32) * 32
        self.args = (bstride, sstride, B, Sn, L, heads, dim_head)
        self.scale = scale
        f32 = dict(dtype=torch.float32, device=dev)
        self.mn = torch.empty(layers, Sn, L, 32, **f32)
        self.mstats = torch.empty(layers, Sn, L, 2, **f32)
        self.k = torch.empty(layers, Sn, L, inner, **f32)
        self.v = torch.empty_like(self.k)
        self.kq = torch.empty(layers, Sn, self.HLP, 32, dtype=dtype, device=dev)
        self.kqT = torch.empty(layers, Sn, 32, self.HLP, dtype=dtype, device=dev)
        self.vo = torch.empty_like(self.kq)
        self.voT = torch.empty_like(self.kqT)
        # per-image weight gradients of every layer, filled by the layers' backward kernels
        self.dkq = torch.empty(layers, Sn, self.HLP, 32, **f32)
        self.dvoT = torch.empty(layers, Sn, 32, self.HLP, **f32)
        self.mfma = masters is not None and prep_mfma_supported(dtype, Sn, L, heads, dim_head, self.HLP)
        self._bwd_ops = (wq0, woT, wkT, wvT)          # what the matrix-core backward reads
        if self.mfma:
            wk0, wv0, wo0, wqT = masters
            if _XPREP_BATCH is not None and not record:
                _lib.lib().dh_xprep_batch_pause(1)
            try:
                _call("dh_xattn_prep_fwd_stack_mfma", P(tok), bstride, sstride, B, Sn, heads, dim_head, self.HLP, scale, eps,
                      layers, param_stride, P(ln_g0), P(ln_b0), P(wk0), P(wv0), P(wo0), P(wqT), P(self.mn), P(self.mstats),
                      P(self.k), P(self.v), P(self.kq), P(self.kqT), P(self.vo), P(self.voT), S())
            finally:
                if _XPREP_BATCH is not None and not record:
                    _lib.lib().dh_xprep_batch_pause(0)
            if _XPREP_BATCH is not None and record:
                _XPREP_BATCH.append(tok)
            return
        _call("dh_xattn_prep_fwd_stack", _DT[dtype], P(tok), bstride, sstride, B, Sn, L, heads, dim_head, self.HLP, scale, eps,
              layers, param_stride, P(ln_g0), P(ln_b0), P(wq0), P(wkT), P(wvT), P(woT), P(self.mn), P(self.mstats), P(self.k),
              P(self.v), P(self.kq), P(self.kqT), P(self.vo), P(self.voT), S())

    def layer(self, i):
        v = _PrepView()
        for n in ("mn", "mstats", "k", "v", "kq", "kqT", "vo", "voT"):
            setattr(v, n, getattr(self, n)[i])
        v.HLP, v.args, v.scale = self.HLP, self.args, self.scale
        return v

    def backward(self, tok, dtok_accum, ln_g0, wqT, wk0, wv0, wo0, dln_g0, dln_b0, dwq0, dwk0, dwv0, dwo0):
        """after every layer's backward stored its dkq / dvoT: token gradient (accumulated into dtok_accum), the
        to_q / to_k / to_v / to_out weight gradients and the shared LayerNorm's, for all layers, in one pass"""
        bstride, sstride, B, Sn, L, heads, dim_head = self.args
        dk = torch.empty_like(self.k)
        dv = torch.empty_like(self.v)
        nws = _lib.lib().dh_xattn_prep_bwd_stack_workspace_size(Sn, L, self.layers)
        if _XPREP_BATCH is not None and self.mfma:
            # recorded (EncoderBatch): the launch comes later, next to other stacks' -- scratch of its own until then
            ws = torch.empty(max(int(nws), 1), dtype=torch.uint8, device=tok.device)
            _XPREP_BATCH.extend((ws, dk, dv, tok, dtok_accum))
        else:
            ws = workspace(nws, tok.device)
            if _DEC_BATCH is not None:            # launched at once: a held-back stack finalize produces the dkq / dvoT read here
                _call("dh_decoder_batch_launch", S())
        if self.mfma:
            wq0, woT, wkT, wvT = self._bwd_ops
            _call("dh_xattn_prep_bwd_stack_mfma", P(tok), P(dtok_accum), bstride, sstride, B, Sn, heads, dim_head, self.HLP,
                  self.scale, self.layers, self.param_stride, P(ln_g0), P(wq0), P(woT), P(wkT), P(wvT), P(self.mn),
                  P(self.mstats), P(self.k), P(self.v), P(self.dkq), P(self.dvoT), P(dk), P(dv), P(dln_g0), P(dln_b0), P(dwq0),
                  P(dwk0), P(dwv0), P(dwo0), 1, P(ws), S())
            return
        _call("dh_xattn_prep_bwd_stack", _DT[self.dtype], P(tok), P(dtok_accum), bstride, sstride, B, Sn, L, heads, dim_head,
              self.HLP, self.scale, self.layers, self.param_stride, P(ln_g0), P(wqT), P(wk0), P(wv0), P(wo0), P(self.mn),
              P(self.mstats), P(self.k), P(self.v), P(self.dkq), P(self.dvoT), P(dk), P(dv), P(dln_g0), P(dln_b0), P(dwq0),
              P(dwk0), P(dwv0), P(dwo0), 1, P(ws), S())


def xattn_prep_bwd(prep, tok, dtok_accum, ln_g, wqT, wk, wv, wo, dkq, dvoT, dln_g, dln_b, dwq, dwk, dwv, dwo,
                   accumulate, dtype):
    bstride, sstride, B, Sn, L, heads, dim_head = prep.args
    dk = torch.empty_like(prep.k)
    dv = torch.empty_like(prep.v)
    Lb = _lib.lib()
    if getattr(prep, "mfma", False):
        wq0, woT, wkT, wvT = prep._bwd_ops
        ws = workspace(Lb.dh_xattn_prep_bwd_stack_workspace_size(Sn, L, 1), tok.device)
        with _XprepPaused():
            _call("dh_xattn_prep_bwd_stack_mfma", P(tok), P(dtok_accum), bstride, sstride, B, Sn, heads, dim_head, prep.HLP,
                  prep.scale, 1, 0, P(ln_g), P(wq0), P(woT), P(wkT), P(wvT), P(prep.mn), P(prep.mstats), P(prep.k), P(prep.v),
                  P(dkq), P(dvoT), P(dk), P(dv), P(dln_g), P(dln_b), P(dwq), P(dwk), P(dwv), P(dwo), accumulate, P(ws), S())
        return
    ws = workspace(Lb.dh_xattn_prep_bwd_workspace_size(Sn), tok.device)
    _call("dh_xattn_prep_bwd", _DT[dtype], P(tok), P(dtok_accum), bstride, sstride, B, Sn, L, heads, dim_head, prep.HLP,
          prep.scale, P(ln_g), P(wqT), P(wk), P(wv), P(wo), P(prep.mn), P(prep.mstats), P(prep.k), P(prep.v), P(dkq), P(dvoT),
          P(dk), P(dv), P(dln_g), P(dln_b), P(dwq), P(dwk), P(dwv), P(dwo), accumulate, P(ws), S())


@_dec_recorded("fwd", lambda a: a[0].shape[0], lambda a: 1, lambda a, k: a[12])
def decoder_layer_fwd(x2d, prep, rows_per_image, ln1_g, ln1_b, bo, ln2_g, ln2_b, w1, b1, w2, b2, mlp, eps=1e-5, fp8=False):
    """fused cross-attention + MLP decoder layer (csrc/decoder_fused.hip); x2d [rows, 32] bf16.
    fp8=True: the four MFMA products on OCP e4m3 operands (csrc/decoder_fp8.hip)"""
    y = torch.empty_like(x2d)
    with _Prof("decoder_layer_fwd", 0, _nb(x2d, y)):
        _call("dh_decoder_layer_fwd_fp8" if fp8 else "dh_decoder_layer_fwd", P(x2d), P(y), P(prep.kq), P(prep.voT), P(ln1_g),
              P(ln1_b), P(bo), P(ln2_g), P(ln2_b), P(w1), P(b1), P(w2), P(b2), x2d.shape[0], rows_per_image, mlp, eps, S())
    if _DEC_BATCH is not None and not fp8:        # recorded: operands alive until the batch is issued
        _DEC_BATCH.extend((x2d, y, prep.kq, prep.voT))
    return y


@_dec_recorded("bwd", lambda a: a[0].shape[0], lambda a: 1, lambda a, k: a[16])
def decoder_layer_bwd(x2d, dy, prep, rows_per_image, ln1_g, ln1_b, bo, ln2_g, ln2_b, w1, w1T, b1, w2, w2T, b2, grads, mlp,
                      eps=1e-5, dkq=None, dvoT=None, partial=None):
    """returns (dx, dkq [S,32,32] fp32, dvoT [S,32,32] fp32); grads = (dw1, dw2, db1, db2, dbo, dg1, dbe1, dg2, dbe2)
    are accumulated in place.  partial (a per-layer buffer of decoder_layer_bwd_partial_floats floats): only the data
    gradient runs, the parameter gradients are summed later by decoder_stack_bwd_finalize (grads is ignored)."""
    rows = x2d.shape[0]
    images = rows // rows_per_image
    dx = torch.empty_like(x2d)
    if dkq is None:
        dkq = torch.empty(images, 32, 32, dtype=torch.float32, device=x2d.device)
        dvoT = torch.empty(images, 32, 32, dtype=torch.float32, device=x2d.device)
    if partial is not None:
        ws, gp = partial, [_vp(0)] * 9
    else:
        ws = workspace(_lib.lib().dh_decoder_layer_bwd_workspace_size(rows, rows_per_image, mlp), x2d.device)
        gp = [P(t) for t in grads]
    with _Prof("decoder_layer_bwd", 0, _nb(x2d, dy, dx)):
        _call("dh_decoder_layer_bwd", P(x2d), P(dy), P(dx), P(prep.kq), P(prep.voT), P(prep.vo), P(prep.kqT), P(ln1_g), P(ln1_b),
              P(bo), P(ln2_g), P(ln2_b), P(w1), P(w1T), P(b1), P(w2), P(w2T), P(b2), *gp, P(dkq), P(dvoT), rows, rows_per_image,
              mlp, eps, P(ws), S())
    if _DEC_BATCH is not None and partial is not None:
        _DEC_BATCH.extend((x2d, dy, dx, ws, prep.kq, prep.voT, prep.vo, prep.kqT))
    return dx, dkq, dvoT


@_dec_recorded("fwd", lambda a: a[0].shape[0], lambda a: a[1].layers, lambda a, k: a[7])
def decoder_stack_fwd(x2d, stack, rows_per_image, params0, w1s, w2s, par_stride, mlp, eps=1e-5):
    """ALL layers of a fused decoder stack in one launch (csrc/decoder_fused.hip, DecArgs::depth): a workgroup takes its
    pixel rows through every layer.  stack: the XattnPrepStack of the layers; params0 = (ln1_g, ln1_b, bo, ln2_g, ln2_b, b1,
    b2) of layer 0, the others `par_stride` floats further; w1s / w2s: the packed MLP weights stacked [depth, ...].
    Returns ys [depth, rows, 32]: every layer's output (ys[-1] = the stack's)."""
    depth, rows = stack.layers, x2d.shape[0]
    ys = torch.empty(depth, rows, 32, dtype=x2d.dtype, device=x2d.device)
    g1, b1_, bo, g2, b2_, fb1, fb2 = params0
    with _Prof("decoder_layer_fwd", 0, depth * _nb(x2d, x2d)):
        _call("dh_decoder_stack_fwd", P(x2d), P(ys), P(stack.kq), P(stack.voT), P(g1), P(b1_), P(bo), P(g2), P(b2_), P(w1s),
              P(fb1), P(w2s), P(fb2), depth, stack.kq[0].numel(), w1s[0].numel(), par_stride, rows, rows_per_image, mlp, eps, S())
    if _DEC_BATCH is not None:
        _DEC_BATCH.extend((x2d, ys, stack.kq, stack.voT, w1s, w2s))
    return ys


@_dec_recorded("bwd", lambda a: a[0].shape[0], lambda a: a[3].layers, lambda a, k: a[11])
def decoder_stack_bwd(x2d, ys, dy, stack, rows_per_image, params0, w1s, w1Ts, w2s, w2Ts, par_stride, mlp, partials, eps=1e-5):
    """data gradient of decoder_stack_fwd in one launch; the per-workgroup parameter-gradient partials of layer l land in
    partials[l] (decoder_stack_bwd_finalize sums them).  Returns dx."""
    depth, rows = stack.layers, x2d.shape[0]
    dx, dwork = torch.empty_like(x2d), torch.empty_like(x2d)
    g1, b1_, bo, g2, b2_, fb1, fb2 = params0
    assert partials.shape[0] == depth and partials.is_contiguous()
    with _Prof("decoder_layer_bwd", 0, depth * _nb(x2d, dy, dx)):
        _call("dh_decoder_stack_bwd", P(x2d), P(ys), P(dy), P(dx), P(dwork), P(stack.kq), P(stack.voT), P(stack.vo), P(stack.kqT),
              P(g1), P(b1_), P(bo), P(g2), P(b2_), P(w1s), P(w1Ts), P(fb1), P(w2s), P(w2Ts), P(fb2), depth, stack.kq[0].numel(),
              w1s[0].numel(), par_stride, rows, rows_per_image, mlp, eps, P(partials), S())
    if _DEC_BATCH is not None:
        _DEC_BATCH.extend((x2d, ys, dy, dx, dwork, partials, stack.kq, stack.voT, stack.vo, stack.kqT, w1s, w1Ts, w2s, w2Ts))
    return dx


def decoder_layer_bwd_partial_floats(rows, rows_per_image, mlp):
    return _lib.lib().dh_decoder_layer_bwd_workspace_size(rows, rows_per_image, mlp) // 4


@_dec_recorded("fin", lambda a: a[1], lambda a: a[0].shape[0], lambda a, k: a[3])
def decoder_stack_bwd_finalize(partials, rows, rows_per_image, mlp, grads0, grad_stride, dkq, dvoT):
    """one launch for the parameter gradients of all layers of a decoder stack: partials [depth, floats], grads0 = the nine
    gradient tensors of layer 0 (layer l's sit grad_stride floats further), dkq / dvoT [depth, images, 32, 32]"""
    _call("dh_decoder_stack_bwd_finalize", P(partials), partials.shape[0], rows, rows_per_image, mlp, *(P(t) for t in grads0),
          grad_stride, P(dkq), P(dvoT), S())


def encoder_supported(n, heads, dim_head, mlp):
    return bool(_lib.lib().dh_encoder_supported(n, heads, dim_head, mlp))


def encoder_fwd(tok2d, B, n, depth, heads, dim_head, mlp, pstride, params, save, scale=32 ** -0.5, eps=1e-5):
    """fused token encoder stack (csrc/encoder_fused.hip).  tok2d [B*n, 32] fp32; params: the 11 first-layer tensors
    (ln1_g, ln1_b, wqkv, wo, bo, ln2_g, ln2_b, w1, b1, w2, b2).  Returns (y, saved per-layer forward images | None)."""
    assert tok2d.dtype == torch.float32 and tok2d.shape == (B * n, 32)
    y = torch.empty_like(tok2d)
    xs = torch.empty(_lib.lib().dh_encoder_saved_floats(B, n, depth, heads, dim_head, mlp), dtype=torch.float32,
                     device=tok2d.device) if save else None          # [depth][B][forward image]
    _call("dh_encoder_fwd", P(tok2d), P(y), P(xs), B, n, depth, heads, dim_head, mlp, scale, eps, pstride, *(P(t) for t in params), S())
    if _ENC_BATCH is not None:
        _ENC_BATCH.extend((tok2d, y, xs))
    return y, xs


def encoder_bwd(dy, xs, B, n, depth, heads, dim_head, mlp, pstride, params, grads, scale=32 ** -0.5, eps=1e-5):
    """dx of the fused encoder; `grads` (same order as params, first layer, in the gradient arena) are accumulated"""
    dx = torch.empty_like(dy)
    nbytes = _lib.lib().dh_encoder_bwd_workspace_size(B, n, depth, heads, dim_head, mlp)
    if _ENC_BATCH is not None:         # recorded, issued later with other stacks: a workspace of its own, alive until then
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dy.device)
        _ENC_BATCH.extend((dy, dx, xs, ws))
    else:
        ws = workspace(nbytes, dy.device)
    _call("dh_encoder_bwd", P(dy), P(dx), P(xs), B, n, depth, heads, dim_head, mlp, scale, eps, pstride, *(P(t) for t in params),
          *(P(t) for t in grads), P(ws), S())
    return dx


_ENC_BATCH = None        # while an EncoderBatch is open: the tensors of the recorded launches
_DEC_BATCH = None        # ... and of its recorded decoder layers
_XPREP_BATCH = None      # ... and of its recorded cross-attention preparations (their own workspaces, dk / dv)


def xprep_recording():
    """True while XattnPrepStack launches are only recorded: their results are valid after the EncoderBatch's next launch()"""
    return _XPREP_BATCH is not None


class _XprepPaused:
    """the single-layer preparation calls launch at once even inside an open batch (their callers read the result next)"""

    def __enter__(self):
        if _XPREP_BATCH is not None:
            _lib.lib().dh_xprep_batch_pause(1)

    def __exit__(self, *exc):
        if _XPREP_BATCH is not None:
            _lib.lib().dh_xprep_batch_pause(0)
        return False


class EncoderBatch:
    """`with EncoderBatch() as eb:` -- encoder_fwd / encoder_bwd calls inside only RECORD their launches (dh_encoder_batch_*);
    eb.launch() issues them together (one workgroup per image each: stacks of independent levels share the chip).  Their
    outputs are valid after launch().  Inert under ops.PROFILE (per-launch events) and with DAHITRA_ENC_BATCH=0."""

    def __init__(self, decoder=False, ew=False):
        """ew=True: add_pos / add_pos_bwd / cat_halves / split_halves / absdiff_halves(_bwd) calls are recorded too (one
        dh_ew_multi launch per round, issued FIRST): the caller pauses between such a call and the first use of its result.
        DAHITRA_EW_BATCH=0 switches that part off.
        decoder=True: the fused decoder layers (decoder_layer_fwd, and decoder_layer_bwd with `partial`) are recorded too
        (dh_decoder_batch_*): layers of independent stacks share a launch.  DAHITRA_DEC_BATCH=0 switches that part off."""
        self.on = PROFILE is None and os.environ.get("DAHITRA_ENC_BATCH", "1") != "0"
        self.dec = decoder and PROFILE is None and os.environ.get("DAHITRA_DEC_BATCH", "1") != "0"
        # with the decoder stacks, their token-side preparation (XattnPrepStack and its backward, dh_xprep_batch_*) and the
        # stack's parameter-gradient finalize are recorded as well.  DAHITRA_XPREP_BATCH=0 switches that part off.
        self.xprep = self.dec and os.environ.get("DAHITRA_XPREP_BATCH", "1") != "0"
        self.ew = ew and PROFILE is None and os.environ.get("DAHITRA_EW_BATCH", "1") != "0"

    def __enter__(self):
        global _ENC_BATCH, _DEC_BATCH, _XPREP_BATCH, _EW_BATCH
        if self.ew:
            assert _EW_BATCH is None, "EncoderBatch(ew=True) is not re-entrant"
            _EW_BATCH = []
        if self.on or self.dec:
            assert _ENC_BATCH is None and _DEC_BATCH is None and _XPREP_BATCH is None, "EncoderBatch is not re-entrant"
        if self.on:
            _ENC_BATCH = []
            _call("dh_encoder_batch_begin")
        if self.dec:
            _DEC_BATCH = []
            _call("dh_decoder_batch_begin")
        if self.xprep:
            _XPREP_BATCH = []
            _call("dh_xprep_batch_begin")
        return self

    def launch(self):
        """program order of what one round may have recorded: a stack's preparation before its forward; a stack's finalize
        (which the decoder batch issues after its backward launches) before the preparation's backward"""
        if self.ew:
            ew_flush()
        if self.xprep:
            _call("dh_xprep_batch_launch_fwd", S())
        if self.on:
            _call("dh_encoder_batch_launch", S())
            del _ENC_BATCH[:]
        if self.dec:
            _call("dh_decoder_batch_launch", S())
            del _DEC_BATCH[:]
            if DEC_RECORD is not None:
                DEC_RECORD.append(dict(kind="launch"))
        if self.xprep:
            _call("dh_xprep_batch_launch_bwd", S())
            del _XPREP_BATCH[:]

    def __exit__(self, *exc):
        global _ENC_BATCH, _DEC_BATCH, _XPREP_BATCH, _EW_BATCH
        failed = bool(exc) and exc[0] is not None
        if self.ew:
            if not failed:
                ew_flush()
            _EW_BATCH = None
        if self.xprep:
            if failed:
                _lib.lib().dh_xprep_batch_abort()
                _XPREP_BATCH = None
            else:
                _call("dh_xprep_batch_launch_fwd", S())
        if self.on:
            if failed:
                _lib.lib().dh_encoder_batch_abort()
            else:
                _call("dh_encoder_batch_end", S())
            _ENC_BATCH = None
        if self.dec:
            if failed:
                _lib.lib().dh_decoder_batch_abort()
            else:
                _call("dh_decoder_batch_end", S())
            _DEC_BATCH = None
        if self.xprep and not failed:
            _call("dh_xprep_batch_end", S())      # after the decoder batch: a pending finalize precedes the preparation's backward
            _XPREP_BATCH = None
        return False


def softmax_groups(x2d, heads, L):
    rows, HLP = x2d.shape
    y = torch.empty_like(x2d)
    _call("dh_softmax_groups_fwd", dt(x2d), P(x2d), P(y), rows, heads, L, HLP, S())
    return y


def softmax_groups_bwd(y, dy, heads, L):
    rows, HLP = y.shape
    dx = torch.empty_like(y)
    _call("dh_softmax_groups_bwd", dt(y), P(y), P(dy), P(dx), rows, heads, L, HLP, S())
    return dx


def self_attn(qkv, B, n, heads, dim_head, scale=32 ** -0.5):
    inner = heads * dim_head
    o = torch.empty(B * n, inner, dtype=qkv.dtype, device=qkv.device)
    attn = torch.empty(B, heads, n, n, dtype=torch.float32, device=qkv.device)
    _call("dh_self_attn_fwd", dt(qkv), P(qkv), P(o), P(attn), B, n, heads, dim_head, scale, S())
    return o, attn


def self_attn_bwd(qkv, attn, dout, B, n, heads, dim_head, scale=32 ** -0.5):
    dqkv = torch.empty_like(qkv)
    _call("dh_self_attn_bwd", dt(qkv), P(qkv), P(attn), P(dout), P(dqkv), B, n, heads, dim_head, scale, S())
    return dqkv


# ---- loss / mask / optimizer ---------------------------------------------------------------------
def focal_loss(logits_nchw, target, want_grad=True, grad_scale=1.0, alpha=0.5):
    B, C, H, W = logits_nchw.shape
    loss = torch.empty((), dtype=torch.float32, device=logits_nchw.device)
    dl = torch.empty_like(logits_nchw) if want_grad else None
    ws = workspace(4096, logits_nchw.device)
    _call("dh_focal_loss", P(logits_nchw), P(target), B, C, H * W, alpha, grad_scale, P(loss), P(dl), P(ws), S())
    return loss, dl


def cross_entropy_fwd(logits_nchw, target, ignore_index=255):
    """returns out [2] (device): mean CE over the non-ignored pixels, their count"""
    B, C, H, W = logits_nchw.shape
    out = torch.empty(2, dtype=torch.float32, device=logits_nchw.device)
    ws = workspace(16384, logits_nchw.device)
    _call("dh_cross_entropy_fwd", P(logits_nchw), P(target), B, C, H * W, ignore_index, P(out), P(ws), S())
    return out


def cross_entropy_bwd(logits_nchw, target, fwd_out, upstream, ignore_index=255):
    B, C, H, W = logits_nchw.shape
    dl = torch.empty_like(logits_nchw)
    _call("dh_cross_entropy_bwd", P(logits_nchw), P(target), B, C, H * W, ignore_index, P(fwd_out), P(upstream), P(dl), S())
    return dl


def dice_argmax_constant(logits_nchw, target, eps=1e-7):
    B, C, H, W = logits_nchw.shape
    loss = torch.empty((), dtype=torch.float32, device=logits_nchw.device)
    ws = workspace(24576, logits_nchw.device)
    _call("dh_dice_argmax_constant", P(logits_nchw), P(target), B, C, H * W, eps, P(loss), P(ws), S())
    return loss


def confusion_matrix(logits_nchw, target, counts, want_mask=False):
    """counts [C, C] int64 (device) += confusion of argmax(logits) against target; optionally returns the mask"""
    B, C, H, W = logits_nchw.shape
    mask = torch.empty(B, H, W, dtype=torch.int64, device=logits_nchw.device) if want_mask else None
    _call("dh_confusion_matrix", P(logits_nchw), P(target), B, C, H * W, P(mask), P(counts), S())
    return mask


def argmax_nchw(logits_nchw):
    B, C, H, W = logits_nchw.shape
    mask = torch.empty(B, H, W, dtype=torch.int64, device=logits_nchw.device)
    _call("dh_argmax_nchw", P(logits_nchw), P(mask), B, C, H * W, S())
    return mask


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _call("dh_adamw_step", P(param), P(grad), P(exp_avg), P(exp_avg_sq), param.numel(), lr, beta1, beta2, eps, weight_decay, step,
          grad_scale, S())


# ---- xBD train step (csrc/xbd_step.hip) ---------------------------------------------------------------
def combo_loss_fwd(logits, masks, weights_dev, dice_weight=1.0, focal_weight=8.0):
    """per-channel ComboLoss{dice, focal} (xBD_code/losses.py:95-126).  Returns (loss [], channel_loss [C], sums [C,4])"""
    B, C, H, W = logits.shape
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ch = torch.empty(C, dtype=torch.float32, device=dev)
    sums = torch.empty(C, 4, dtype=torch.float32, device=dev)
    ws = workspace(_lib.lib().dh_combo_loss_workspace_size(C), dev)
    _call("dh_combo_loss_fwd", P(logits), P(masks), B, C, H * W, P(weights_dev), dice_weight, focal_weight, P(sums), P(ch),
          P(loss), P(ws), S())
    return loss, ch, sums


def combo_loss_bwd(logits, masks, sums, weights_dev, upstream, dice_weight=1.0, focal_weight=8.0):
    B, C, H, W = logits.shape
    dl = torch.empty_like(logits)
    _call("dh_combo_loss_bwd", P(logits), P(masks), P(sums), P(weights_dev), P(upstream), dice_weight, focal_weight, B, C, H * W,
          P(dl), S())
    return dl


def grad_norm_clip_coef(grad_flat, max_norm, out):
    """out [2] fp32 (device): total L2 norm of the flat gradient arena, clip_grad_norm_ coefficient"""
    ws = workspace(_lib.lib().dh_grad_norm_workspace_size(), grad_flat.device)
    _call("dh_grad_norm_clip_coef", P(grad_flat), grad_flat.numel(), max_norm, P(out), P(ws), S())


def adamw_xbd_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale_dev=None):
    _call("dh_adamw_xbd_step", P(param), P(grad), P(exp_avg), P(exp_avg_sq), param.numel(), lr, beta1, beta2, eps, weight_decay,
          step, P(grad_scale_dev), S())


# ---- arguments, outputs and workspaces of the checked wrappers below: xBD losses, loaders, evaluation, cd_* ------
class _Args:
    """The argument checker of the wrappers from here to cd_view_counts -- the xBD losses, loaders and evaluation, the cd_* ones;
    xbd_val_count / xbd_val_sweep keep _xbd_val_args' checks, which convert dtypes: ValueError, before any launch, for whatever
    the kernel cannot read as it lies.  tensor() refuses at once an argument whose type, dtype or shape does not fit,
        "<fn>: <name> <shape> <dtype> is not <dtype> <text>",
    and placed(), called when all of them fit, checks device and storage -- so a wrong shape shows whatever device the tensors
    are on.  Two placement policies: a tensor that is not on the first one's GPU is a ValueError (the xBD loaders and evaluation
    wrappers); with cpu_error=True tensors that are ALL on the CPU are a HipLibraryError (there is no CPU path) and only mixed
    devices a ValueError (the xBD losses, xbd_class_table, cd_eval_vis, cd_tile_stitch, cd_view_counts)."""

    def __init__(self, what, cpu_error=False):
        self.what, self.cpu_error, self.checked = what, cpu_error, []

    def tensor(self, name, t, dtype, fits, text=None):
        """fits: the shape, or a predicate on the tensor; text: how the message describes it (default: the shape).  Returns t"""
        if not torch.is_tensor(t) or t.dtype != dtype or not (fits(t) if callable(fits) else tuple(t.shape) == tuple(fits)):
            raise ValueError("%s: %s %s %s is not %s %s" % (self.what, name, tuple(getattr(t, "shape", ())), getattr(t, "dtype", type(t)),
                                                            str(dtype).replace("torch.", ""), str(list(fits)) if text is None else text))
        self.checked.append((name, t))
        return t

    def image(self, name, t, dtype):
        """a non-empty [N, H, W] map: returns (N, H, W)"""
        return tuple(self.tensor(name, t, dtype, lambda t: t.dim() == 3 and t.numel() > 0, "[N, H, W], not empty").shape)

    def out(self, t, dtype, shape, name="out", text=None):
        """an output buffer: the given one, checked like any argument, or a fresh tensor beside the first argument"""
        if t is None:
            return torch.empty(tuple(shape), dtype=dtype, device=self.checked[0][1].device)
        return self.tensor(name, t, dtype, shape, text)

    def workspace(self, ws):
        """a caller's workspace, if one is given: uint8 of any shape (_workspace checks its size once the need is known)"""
        if ws is not None:
            self.tensor("ws", ws, torch.uint8, lambda t: True, "workspace")

    def placed(self):
        first_name, first = self.checked[0]
        if self.cpu_error and not any(t.is_cuda for _, t in self.checked):
            raise _lib.HipLibraryError("dahitra_amd %s runs on MI355X only (no CPU fallback): its tensors are on the CPU" % self.what)
        for name, t in self.checked:
            if not t.is_cuda or t.device != first.device:
                if self.cpu_error:
                    raise ValueError("%s: %s is on %s and %s on %s; the kernel takes all its tensors on one GPU"
                                     % (self.what, name, t.device, first_name, first.device))
                raise ValueError("%s: %s is on %s; the kernel runs on the MI355X and all its tensors on one device"
                                 % (self.what, name, t.device))
            if not t.is_contiguous():
                raise ValueError("%s: %s is not contiguous (strides %s)" % (self.what, name, t.stride()))


def _ws_bytes(entry, *dims):
    """what the library's size query `entry` answers for `dims`: the bytes of a kernel's workspace"""
    n = ctypes.c_long(0)
    if getattr(_lib.lib(), entry)(*dims, ctypes.byref(n)) != 0:
        raise ValueError(_lib.lib().dh_last_error().decode())
    return int(n.value)


def _workspace(what, ws, need, device):
    """the caller's workspace (an _Args-checked uint8 buffer) if it holds `need` 4-byte aligned bytes, or a fresh one"""
    if ws is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if ws.numel() < need or ws.data_ptr() % 4:
        raise ValueError("%s: ws holds %d bytes at offset %d, %d 4-byte aligned ones are needed" % (what, ws.numel(), ws.data_ptr() % 4, need))
    return ws


# ---- losses of the two xBD training scripts (csrc/xbd_script_loss.hip) -------------------------------------------
XBD_UNET_LABELS = {"lbl_msk": 0, "damage": 1}
# lanes of one forward grid pass (dh_xbd_unet_loss_grid_pass): that many pixels where H * W is no multiple of 4 (one pixel per
# lane), four times as many where it is; a batch beyond it is strided over
XBD_UNET_LOSS_PASS = 1024 * 256
XBD_UNET_PARTS = ("loss0", "loss1", "loss2", "loss3", "loss4", "ce", "dice", "bad_labels")
# lanes of one forward grid pass (dh_xbd_adapt_loss_grid_pass), as XBD_UNET_LOSS_PASS
XBD_ADAPT_LOSS_PASS = 1024 * 256
XBD_ADAPT_PARTS = ("loss0", "loss1", "loss2", "loss3", "ce", "zero")

# form -> channels, sums handed to the backward, parts, the entries' and refusals' prefix, whether the entries take lbl
_XBD_LOSS_FORMS = {"unet": (5, 24, len(XBD_UNET_PARTS), "xbd_unet_loss", True),
                   "adapt": (4, 18, len(XBD_ADAPT_PARTS), "xbd_adapt_loss", False)}


def _xbd_loss_args(form, tail, logits, msk, lbl, labels, weights_dev, extra=()):
    """the tensors of a form's loss _fwd / _bwd, refused before any launch: ValueError for a label mode, dtype or shape that does
    not fit and for mixed devices, HipLibraryError when everything is on the CPU.  Returns the label arguments of the C entry
    (lbl and label_mode, or none where the form has no lbl), B, H, W"""
    C, _, _, prefix, has_lbl = _XBD_LOSS_FORMS[form]
    what = prefix + tail
    if has_lbl:
        if labels not in XBD_UNET_LABELS:
            raise ValueError("%s: labels %r is not one of %s" % (what, labels, sorted(XBD_UNET_LABELS)))
        if labels == "lbl_msk" and lbl is None:
            raise ValueError("%s: labels='lbl_msk' reads lbl, which is None" % what)
    a = _Args(what, cpu_error=True)
    B, _, H, W = a.tensor("logits", logits, torch.float32, lambda t: t.dim() == 4 and t.shape[1] == C and t.numel() > 0,
                          "[B, %d, H, W], not empty" % C).shape
    a.tensor("msk", msk, torch.uint8, (B, C, H, W), "[%d, %d, %d, %d] like logits" % (B, C, H, W))
    if lbl is not None:
        a.tensor("lbl", lbl, torch.uint8, (B, H, W), "[%d, %d, %d] like logits" % (B, H, W))
    a.tensor("weights_dev", weights_dev, torch.float32, (2 * C,), "[%d]: %d channel weights, %d class weights" % (2 * C, C, C))
    for name, t, shape in extra:
        if t is not None:
            a.tensor(name, t, torch.float32, lambda t, n=math.prod(shape): t.numel() == n, str(list(shape)))
    a.placed()
    if not has_lbl:
        return (), B, H, W
    mode = XBD_UNET_LABELS[labels]
    return (P(lbl if mode == 0 else None), mode), B, H, W


def _xbd_loss_fwd(form, logits, msk, lbl, labels, weights_dev, dice_weight, focal_weight, ce_weight):
    _, n_sums, n_parts, prefix, _ = _XBD_LOSS_FORMS[form]
    label_args, B, H, W = _xbd_loss_args(form, "_fwd", logits, msk, lbl, labels, weights_dev)
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    parts = torch.empty(n_parts, dtype=torch.float32, device=dev)
    sums = torch.empty(n_sums, dtype=torch.float32, device=dev)
    ws = workspace(_ws_bytes("dh_%s_workspace_size" % prefix), dev)
    _call("dh_%s_fwd" % prefix, P(logits), P(msk), *label_args, B, H * W, P(weights_dev), float(dice_weight), float(focal_weight),
          float(ce_weight), P(sums), P(parts), P(loss), P(ws), ws.numel(), S())
    return loss, parts, sums


def _xbd_loss_bwd(form, logits, msk, lbl, labels, sums, weights_dev, upstream, dice_weight, focal_weight, ce_weight):
    _, n_sums, _, prefix, _ = _XBD_LOSS_FORMS[form]
    if sums is None:
        raise ValueError("%s_bwd: sums is None; it is %s_fwd's third result" % (prefix, prefix))
    label_args, B, H, W = _xbd_loss_args(form, "_bwd", logits, msk, lbl, labels, weights_dev,
                                         (("sums", sums, (n_sums,)), ("upstream", upstream, (1,))))
    dl = torch.empty_like(logits)
    _call("dh_%s_bwd" % prefix, P(logits), P(msk), *label_args, P(sums), P(weights_dev), P(upstream), float(dice_weight),
          float(focal_weight), float(ce_weight), B, H * W, P(dl), S())
    return dl


def xbd_unet_loss_fwd(logits, msk, lbl, labels, weights_dev, dice_weight=1.0, focal_weight=8.0, ce_weight=8.0):
    """The loss of xBD_code/train_unettransformer.py:438-461 in one pass and a finalize launch (dh_xbd_unet_loss_fwd): five weighted
    ComboLoss{dice, focal} terms + ce_weight * the class-weighted cross-entropy of the logits multiplied by (y > 0).
    logits fp32 [B, 5, H, W]; msk uint8 [B, 5, H, W], the loader's bytes; labels 'lbl_msk': y = lbl, uint8 [B, H, W]; labels
    'damage': y = the first set channel among 1 .. 4 of msk (lbl is not read and may be None); weights_dev fp32 [10] = the 5
    channel weights, then the 5 class weights.  Returns (loss [], parts [8] = XBD_UNET_PARTS, sums [24] for xbd_unet_loss_bwd),
    all on the device; nothing is read by the host."""
    return _xbd_loss_fwd("unet", logits, msk, lbl, labels, weights_dev, dice_weight, focal_weight, ce_weight)


def xbd_unet_loss_bwd(logits, msk, lbl, labels, sums, weights_dev, upstream=None, dice_weight=1.0, focal_weight=8.0, ce_weight=8.0):
    """dloss / dlogits of xbd_unet_loss_fwd, one pass (dh_xbd_unet_loss_bwd): fp32 [B, 5, H, W].  sums: the forward's third result;
    upstream: a device scalar fp32 [1] that multiplies the gradient, or None for 1."""
    return _xbd_loss_bwd("unet", logits, msk, lbl, labels, sums, weights_dev, upstream, dice_weight, focal_weight, ce_weight)


def xbd_adapt_loss_fwd(logits, msk, weights_dev, dice_weight=1.0, focal_weight=8.0, ce_weight=5.0):
    """The loss of xBD_code/train_adapt.py:332-342 in one pass and a finalize launch (dh_xbd_adapt_loss_fwd): four weighted
    ComboLoss{dice, focal} terms + ce_weight * the class-weighted cross-entropy of the RAW logits against y = the first maximum
    of (1 - m0, m1, m2, m3), derived from the mask bytes in the kernel.  logits fp32 [B, 4, H, W]; msk uint8 [B, 4, H, W], the
    loader's bytes; weights_dev fp32 [8] = the 4 channel weights, then the 4 class weights.  Returns (loss [], parts [6] =
    XBD_ADAPT_PARTS, sums [18] for xbd_adapt_loss_bwd), all on the device; nothing is read by the host."""
    return _xbd_loss_fwd("adapt", logits, msk, None, None, weights_dev, dice_weight, focal_weight, ce_weight)


def xbd_adapt_loss_bwd(logits, msk, sums, weights_dev, upstream=None, dice_weight=1.0, focal_weight=8.0, ce_weight=5.0):
    """dloss / dlogits of xbd_adapt_loss_fwd, one pass (dh_xbd_adapt_loss_bwd): fp32 [B, 4, H, W].  sums: the forward's third
    result; upstream: a device scalar fp32 [1] that multiplies the gradient, or None for 1."""
    return _xbd_loss_bwd("adapt", logits, msk, None, None, sums, weights_dev, upstream, dice_weight, focal_weight, ce_weight)


# ---- xBD losses: the Lovasz, Jaccard and BCE terms of ComboLoss (csrc/xbd_seg_losses.hip) ------------------------------
XBD_LOVASZ_MODES = {"hinge": 0, "probas": 1, "sigmoid": 2}
XBD_LOVASZ_TILE = 2048             # elements a workgroup takes per pass: dh_xbd_lovasz_tile
XBD_LOVASZ_MAX_SEGMENTS = 256
XBD_SEG_TERMS = ("jaccard", "bce", "mask_bceavg", "dice", "focal")
_TARGET_KINDS = {torch.float32: 0, torch.uint8: 1}


def _seg_loss_args(what, x, target, channel_weights_dev, extra=()):
    """x fp32 [B, C, ...] and a target of its shape, fp32 or uint8; the optional fp32 tensors of `extra` = (name, tensor, numel).
    ValueError for what does not fit, HipLibraryError when everything is on the CPU.  Returns (a, B, C, HW, target_kind)"""
    a = _Args(what, cpu_error=True)
    a.tensor("x", x, torch.float32, lambda t: t.dim() >= 3 and t.numel() > 0, "[B, C, ...], not empty")
    B, C = x.shape[:2]
    if not torch.is_tensor(target) or target.dtype not in _TARGET_KINDS:
        raise ValueError("%s: target %s is neither a float32 nor a uint8 tensor" % (what, getattr(target, "dtype", type(target))))
    a.tensor("target", target, target.dtype, tuple(x.shape), "%s like x" % list(x.shape))
    if channel_weights_dev is not None:
        a.tensor("channel_weights_dev", channel_weights_dev, torch.float32, (C,), "[%d]: a weight per channel" % C)
    for name, t, numel in extra:
        if t is not None:
            a.tensor(name, t, torch.float32, lambda t, n=numel: t.numel() == n, "%d numbers" % numel)
    a.placed()
    return a, B, C, x.numel() // (B * C), _TARGET_KINDS[target.dtype]


def _lovasz_call(what, x, target, mode, per_image, ignore, channel_weights_dev):
    if mode not in XBD_LOVASZ_MODES and mode not in XBD_LOVASZ_MODES.values():
        raise ValueError("%s: mode %r is not one of %s" % (what, mode, sorted(XBD_LOVASZ_MODES)))
    ignore = -1 if ignore is None else int(ignore)
    if not -1 <= ignore <= 255:
        raise ValueError("%s: ignore=%r is neither None nor a byte" % (what, ignore))
    a, B, C, HW, kind = _seg_loss_args(what, x, target, channel_weights_dev)
    segments = B * C if per_image else C
    if segments > XBD_LOVASZ_MAX_SEGMENTS or x.numel() > 1 << 30:
        raise ValueError("%s: %d segments of %d elements; at most %d segments and 2^30 elements are sorted"
                         % (what, segments, x.numel() // segments, XBD_LOVASZ_MAX_SEGMENTS))
    ws = workspace(_ws_bytes("dh_xbd_lovasz_workspace_size", x.numel(), segments), x.device)
    return (P(x), P(target), kind, B, C, HW, XBD_LOVASZ_MODES.get(mode, mode), int(bool(per_image)), ignore), ws


def xbd_lovasz(x, target, mode, per_image=False, ignore=255, channel_weights_dev=None, bad_out=None):
    """lovasz_hinge / lovasz_sigmoid of xBD_code/losses.py:129-225 for every channel, with the gradient (dh_xbd_lovasz_fwd).
    x fp32 [B, C, H, W] (or [B, C, n]); target of its shape, fp32 or uint8 (the same bits either way).  mode 'hinge' (0): x are
    logits; 'probas' (1): x are probabilities; 'sigmoid' (2): x are logits and the sigmoid is taken in the kernel.  per_image: a
    channel's loss is the mean over its images (an image without a valid element counts 0) instead of one sort over the batch.
    ignore: the target value that is dropped, or None.  Equal errors keep flat index order, so the gradient is defined.
    Returns (loss [] = sum_c w_c channel_loss_c, channel_losses [C], dx like x = d loss / d x); w = channel_weights_dev or 1.
    bad_out: an int32 [1] device tensor that receives the number of targets that are neither 0, 1 nor `ignore` (they are dropped).
    No host read.  The only allocations are the three results and, when the current stream's ops.workspace is smaller than the
    call needs, that workspace: a capture whose stream holds a workspace grown by a warm-up (ops.rekey_workspace, as
    GraphedXbdStep does) records the call with nothing but its results in the graph's pool."""
    args, ws = _lovasz_call("xbd_lovasz", x, target, mode, per_image, ignore, channel_weights_dev)
    if bad_out is not None and not (torch.is_tensor(bad_out) and bad_out.dtype == torch.int32 and bad_out.numel() == 1
                                    and bad_out.device == x.device):
        raise ValueError("xbd_lovasz: bad_out is not an int32 [1] tensor beside x")
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    channel = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    _call("dh_xbd_lovasz_fwd", *args, P(channel_weights_dev), P(loss), P(channel), P(dx), P(bad_out), P(ws), ws.numel(), S())
    return loss, channel, dx


def xbd_lovasz_order(x, target, mode, per_image=False, ignore=255):
    """The order xbd_lovasz sums in (dh_xbd_lovasz_order): int32 [n] flat indices into x, segment after segment (a segment is a
    channel over the batch, c, or with per_image a plane, b * C + c), descending error inside a segment, equal errors in index
    order, dropped elements last."""
    args, ws = _lovasz_call("xbd_lovasz_order", x, target, mode, per_image, ignore, None)
    order = torch.empty(x.numel(), dtype=torch.int32, device=x.device)
    _call("dh_xbd_lovasz_order", *args, P(order), P(ws), ws.numel(), S())
    return order


def xbd_seg_terms_fwd(x, target, channel_weights_dev=None, jaccard=0.0, bce=0.0, mask_bceavg=0.0, dice=0.0, focal=0.0, probs=False):
    """The jaccard, bce and mask_bceavg terms of ComboLoss (xBD_code/losses.py:36-45, 70-92) per channel over the batch, in one
    pass and a finalize launch (dh_xbd_seg_terms_fwd).  x fp32 [B, C, H, W]: logits, the sigmoid taken in the kernel, or with
    probs=True probabilities (what the reference's stand-alone classes take; bce reads x as logits either way); target of its
    shape, fp32 or uint8.  dice and focal are the same kernel's forms of soft_dice_loss and FocalLoss2d for those classes.
    Returns (loss [] = sum_c w_c sum_k weight_k term_kc, terms [C, 5] = XBD_SEG_TERMS, sums [C, 4] for xbd_seg_terms_bwd), on
    the device."""
    _, B, C, HW, kind = _seg_loss_args("xbd_seg_terms_fwd", x, target, channel_weights_dev)
    dev = x.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    terms = torch.empty(C, len(XBD_SEG_TERMS), dtype=torch.float32, device=dev)
    sums = torch.empty(C, 4, dtype=torch.float32, device=dev)
    ws = workspace(_ws_bytes("dh_xbd_seg_terms_workspace_size", C), dev)
    _call("dh_xbd_seg_terms_fwd", P(x), P(target), kind, int(bool(probs)), B, C, HW, P(channel_weights_dev), float(jaccard),
          float(bce), float(mask_bceavg), float(dice), float(focal), P(sums), P(terms), P(loss), P(ws), ws.numel(), S())
    return loss, terms, sums


def xbd_seg_terms_bwd(x, target, sums, channel_weights_dev=None, upstream=None, jaccard=0.0, bce=0.0, mask_bceavg=0.0, dice=0.0,
                      focal=0.0, probs=False):
    """d loss / d x of xbd_seg_terms_fwd in one pass (dh_xbd_seg_terms_bwd): fp32 like x.  sums: the forward's third result;
    upstream: a device scalar fp32 [1] that multiplies the gradient, or None for 1.  A zero weight costs nothing."""
    if sums is None:
        raise ValueError("xbd_seg_terms_bwd: sums is None; it is xbd_seg_terms_fwd's third result")
    _, B, C, HW, kind = _seg_loss_args("xbd_seg_terms_bwd", x, target, channel_weights_dev,
                                       (("sums", sums, 4 * x.shape[1] if torch.is_tensor(x) and x.dim() > 1 else 0),
                                        ("upstream", upstream, 1)))
    dx = torch.empty_like(x)
    _call("dh_xbd_seg_terms_bwd", P(x), P(target), kind, int(bool(probs)), P(sums), P(channel_weights_dev), P(upstream),
          float(jaccard), float(bce), float(mask_bceavg), float(dice), float(focal), B, C, HW, P(dx), S())
    return dx


# ---- loader of xBD_code/train_adapt.py (csrc/xbd_adapt.hip) ------------------------------------------------------
def xbd_adapt_batch(pre_u8, post_u8, pre_mask_u8, post_label_u8, idx, origins, crop, train=True):
    """One batch of the adaptation script's TrainData / ValData in ONE launch (dh_xbd_adapt_batch_u8).  pre_u8, post_u8
    [n_src, H, W, 3] and pre_mask_u8, post_label_u8 [n_src, H, W]: the resident uint8 sources; idx int32 [N]: the source of
    every sample; origins int32 [N, 2] = (x0, y0) of every crop window, or None for (0, 0).  Returns (img fp32 [N, 6, crop, crop]
    = x / 127 - 1, msk uint8 [N, 4, crop, crop], lbl uint8 [N, crop, crop]); the planes are stated at the entry's declaration.
    train=False reads the pre mask for plane 0 (ValData).  ValueError for whatever does not fit, before the launch; the caller
    range-checks idx and origins (they are device memory: the kernel clamps them into the sources)."""
    a = _Args("xbd_adapt_batch")
    n_src, H, W, _ = a.tensor("pre_u8", pre_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[3] == 3 and t.numel() > 0,
                              "[n_src, H, W, 3], not empty").shape
    a.tensor("post_u8", post_u8, torch.uint8, (n_src, H, W, 3))
    a.tensor("pre_mask_u8", pre_mask_u8, torch.uint8, (n_src, H, W))
    a.tensor("post_label_u8", post_label_u8, torch.uint8, (n_src, H, W))
    N = a.tensor("idx", idx, torch.int32, lambda t: t.dim() == 1 and t.numel() > 0, "[N], not empty").shape[0]
    if origins is not None:
        a.tensor("origins", origins, torch.int32, (N, 2), "[%d, 2]: a row per entry of idx" % N)
    a.placed()
    if isinstance(crop, bool) or not isinstance(crop, int) or not 1 <= crop <= min(H, W):
        raise ValueError("xbd_adapt_batch: crop %r does not fit the %dx%d sources" % (crop, H, W))
    dev = pre_u8.device
    img = torch.empty(N, 6, crop, crop, dtype=torch.float32, device=dev)
    msk = torch.empty(N, 4, crop, crop, dtype=torch.uint8, device=dev)
    lbl = torch.empty(N, crop, crop, dtype=torch.uint8, device=dev)
    _call("dh_xbd_adapt_batch_u8", P(pre_u8), P(post_u8), P(pre_mask_u8), P(post_label_u8), P(idx), P(origins), N, n_src, H, W,
          crop, 0 if train else 1, P(img), P(msk), P(lbl), S())
    return img, msk, lbl


# ---- xBD validation count (csrc/xbd_eval.hip) -----------------------------------------------------------
XBD_VAL_SELECT = {"reference": 0, "building": 1}


XBD_VAL_CLASSES = (3, 4)          # damage classes: 4 (train.py's five-output net) or 3 (train_adapt.py's four-output net)


def _xbd_val_args(what, logits, msk, lbl, select, classes=4):
    """the tensors of xbd_val_count / xbd_val_sweep: ValueError for shapes or dtypes that do not fit.  Returns the mask plane and
    the labels as the kernel reads them (uint8), the plane's image stride in bytes, and B, H, W.  classes: the damage classes;
    logits and a four-dimensional msk have classes + 1 channels"""
    if select not in XBD_VAL_SELECT:
        raise ValueError("%s: select %r is not one of %s" % (what, select, sorted(XBD_VAL_SELECT)))
    if classes not in XBD_VAL_CLASSES:
        raise ValueError("%s: classes %r is not one of %s" % (what, classes, list(XBD_VAL_CLASSES)))
    C = classes + 1
    if logits.dim() != 4 or logits.shape[1] != C:
        raise ValueError("%s: logits %s are not [B, %d, H, W]" % (what, tuple(logits.shape), C))
    if logits.dtype != torch.float32:
        raise ValueError("%s: logits are %s, the sigmoid is taken in float32" % (what, logits.dtype))
    B, _, H, W = logits.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("%s: empty logits %s" % (what, tuple(logits.shape),))
    if msk.dim() == 4:
        if tuple(msk.shape) != (B, C, H, W):
            raise ValueError("%s: msk %s does not match logits %s" % (what, tuple(msk.shape), tuple(logits.shape)))
        msk = msk[:, 0]
    if tuple(msk.shape) != (B, H, W):
        raise ValueError("%s: msk %s is neither [B, %d, H, W] nor [B, H, W] of logits %s"
                         % (what, tuple(msk.shape), C, tuple(logits.shape)))
    if tuple(lbl.shape) != (B, H, W):
        raise ValueError("%s: lbl_msk %s is not [B, H, W] of logits %s" % (what, tuple(lbl.shape), tuple(logits.shape)))
    if select == "reference" and H != W:
        raise ValueError("%s: the reference's selection lbl_msk[j][lbl_msk[j, 0] > 0] indexes rows by the first row "
                         "and needs H == W, got %dx%d (numpy raises IndexError there)" % (what, H, W))
    for name, t in (("msk", msk), ("lbl_msk", lbl)):
        if t.dtype not in (torch.uint8, torch.int64, torch.bool):
            raise ValueError("%s: %s is %s, expected uint8 (or the reference's long)" % (what, name, t.dtype))
    if msk.dtype != torch.uint8:
        msk = (msk != 0).to(torch.uint8)
    if lbl.dtype != torch.uint8:
        lbl = lbl.clamp(0, 255).to(torch.uint8)
    # channel 0 of a contiguous [B, C, H, W] mask: planes contiguous, images C * H * W bytes apart -- read without a copy
    if not (msk.stride(2) == 1 and msk.stride(1) == W and (B == 1 or msk.stride(0) >= H * W)):
        msk = msk.contiguous()
    stride = msk.stride(0) if B > 1 else H * W
    return msk, lbl, stride, B, H, W


def xbd_val_count(logits, msk, lbl, image_counts, class_counts, thr=0.3, select="reference", classes=4):
    """The counts of the reference's validate() (xBD_code/train.py:258-279) for one batch, on the device, no host read.
    logits [B, 5, H, W] fp32; msk: the batch's mask [B, 5, H, W] (channel 0 is read in place) or its localisation plane
    [B, H, W] / msk[:, 0], uint8 as the device loader gives it; lbl [B, H, W] uint8 (classes 0 .. 3).  A long tensor (the
    reference's dtype) is converted once.  image_counts int64 [B, 3] = |gt0|, |loc|, |gt0 & loc| is written, class_counts int64
    [4, 3] = tp, fn, fp of each class is accumulated.  select: 'reference' (train.py:271-274: row r counts iff
    lbl[j, 0, r] > 0; H == W) or 'building' (pixel p counts iff msk[j, 0, p] > 0).
    classes: the damage classes, 4 (default: all of the above, dh_xbd_val_count) or 3 -- the pass of
    xBD_code/train_adapt.py:262-280 for its four-output net (dh_xbd_val_count_n): logits and msk [B, 4, H, W], lbl 0 .. 2,
    class_counts [3, 3].  ValueError for shapes or dtypes that do not fit, before the call."""
    msk, lbl, stride, B, H, W = _xbd_val_args("xbd_val_count", logits, msk, lbl, select, classes)
    if tuple(image_counts.shape) != (B, 3) or image_counts.dtype != torch.int64:
        raise ValueError("xbd_val_count: image_counts %s %s is not int64 [%d, 3]" % (tuple(image_counts.shape), image_counts.dtype, B))
    if tuple(class_counts.shape) != (classes, 3) or class_counts.dtype != torch.int64:
        raise ValueError("xbd_val_count: class_counts %s %s is not int64 [%d, 3]" % (tuple(class_counts.shape), class_counts.dtype,
                                                                                      classes))
    if not 0.0 < float(thr) < 1.0:
        raise ValueError("xbd_val_count: thr=%r must lie inside (0, 1)" % (thr,))
    for t in (logits, msk, lbl, image_counts, class_counts):
        if not t.is_cuda:
            raise _lib.HipLibraryError("xbd_val_count runs on MI355X only (no CPU fallback)")
    if classes == 4:
        _call("dh_xbd_val_count", P(logits.contiguous()), _vp(msk.data_ptr()), stride, P(lbl.contiguous()), B, H, W, float(thr),
              XBD_VAL_SELECT[select], P(image_counts), P(class_counts), S())
    else:
        _call("dh_xbd_val_count_n", P(logits.contiguous()), _vp(msk.data_ptr()), stride, P(lbl.contiguous()), classes, B, H, W,
              float(thr), XBD_VAL_SELECT[select], P(image_counts), P(class_counts), S())


XBD_SWEEP_MAX = 64          # thresholds per call: they travel by value in the kernel's arguments


def xbd_sweep_thresholds(thresholds, what="xbd_val_sweep"):
    """a threshold grid as the kernel takes it: a contiguous float32 array of 1 .. XBD_SWEEP_MAX values inside (0, 1), strictly
    ascending AFTER the conversion to float32 (two float64 neighbours may round to one float32).  ValueError otherwise."""
    try:
        thr = np.asarray(thresholds.detach().cpu().numpy() if torch.is_tensor(thresholds) else thresholds, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("%s: thresholds %r are not a sequence of numbers" % (what, thresholds))
    if thr.ndim != 1 or not 1 <= thr.size <= XBD_SWEEP_MAX:
        raise ValueError("%s: thresholds of shape %s, expected a 1-D sequence of 1 .. %d values" % (what, thr.shape, XBD_SWEEP_MAX))
    thr = np.ascontiguousarray(thr)
    if not bool(np.all((thr > 0) & (thr < 1))):          # (a nan fails too)
        raise ValueError("%s: every threshold must lie inside (0, 1), got %s" % (what, thr.tolist()))
    if not bool(np.all(thr[1:] > thr[:-1])):
        raise ValueError("%s: the thresholds must ascend strictly as float32, got %s" % (what, thr.tolist()))
    return thr


def xbd_val_sweep(logits, msk, lbl, image_hist, class_hist, thresholds, select="reference"):
    """xbd_val_count for a whole grid of localisation thresholds in the same single pass over the logits: instead of counting
    against one threshold, every pixel is filed under bin = the number of thresholds its localisation sigmoid exceeds (strict,
    float32), 0 .. T, so `bin > k` is xbd_val_count's `loc` at thresholds[k].  logits, msk, lbl and select as xbd_val_count.
    image_hist int64 [B, T + 1, 4, 2], indexed [j, bin, arg, g0] over every pixel of image j (arg: the first maximum of the
    damage sigmoids, g0: msk[j, 0] != 0), is written; class_hist int64 [T + 1, 4, 5], indexed [bin, arg, t] over the selected
    pixels with t = min(lbl, 4), is accumulated.  models/xbd.sweep_counts reduces the two to xbd_val_count's counts for any
    threshold of the grid or any per-class rule.  thresholds: 1 .. XBD_SWEEP_MAX floats, inside (0, 1) and strictly ascending as
    float32.  ValueError for whatever does not fit, before the call."""
    msk, lbl, stride, B, H, W = _xbd_val_args("xbd_val_sweep", logits, msk, lbl, select)
    thr = xbd_sweep_thresholds(thresholds)
    T = int(thr.size)
    if tuple(image_hist.shape) != (B, T + 1, 4, 2) or image_hist.dtype != torch.int64:
        raise ValueError("xbd_val_sweep: image_hist %s %s is not int64 [%d, %d, 4, 2]"
                         % (tuple(image_hist.shape), image_hist.dtype, B, T + 1))
    if tuple(class_hist.shape) != (T + 1, 4, 5) or class_hist.dtype != torch.int64:
        raise ValueError("xbd_val_sweep: class_hist %s %s is not int64 [%d, 4, 5]" % (tuple(class_hist.shape), class_hist.dtype, T + 1))
    for t in (logits, msk, lbl, image_hist, class_hist):
        if not t.is_cuda:
            raise _lib.HipLibraryError("xbd_val_sweep runs on MI355X only (no CPU fallback)")
    _call("dh_xbd_val_sweep", P(logits.contiguous()), _vp(msk.data_ptr()), stride, P(lbl.contiguous()), B, H, W, _vp(thr.ctypes.data),
          T, XBD_VAL_SELECT[select], P(image_hist), P(class_hist), S())


# ---- xBD prediction: 4-flip test-time augmentation (csrc/xbd_predict.hip) ---------------------------------
XBD_TTA_ORDER = {"rgb": 0, "bgr": 1}


def _tta_pack_args(what, pre_u8, post_u8, order, views, out):
    """the arguments of xbd_tta_pack (views None: its four flips) and xbd_tta_pack_views: returns N, H, W, V and `out`"""
    if order not in XBD_TTA_ORDER:
        raise ValueError("%s: order %r is not one of %s" % (what, order, sorted(XBD_TTA_ORDER)))
    a = _Args(what)
    N, H, W, _ = a.tensor("pre_u8", pre_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[3] == 3, "[N, H, W, 3]").shape
    V = 4 if views is None else _tta_views(what, views, H, W)
    a.tensor("post_u8", post_u8, torch.uint8, (N, H, W, 3), "[%d, %d, %d, 3] like pre_u8" % (N, H, W))
    out = a.out(out, torch.float32, (V * N, 6, H, W))
    a.placed()
    return N, H, W, V, out


def _tta_merge_args(what, named, views, out):
    """the arguments of xbd_tta_merge (views None: four flips) and xbd_tta_merge_multi; named: (name, logits) of every model.
    Returns N, H, W, V and `out`"""
    a = _Args(what)
    first = a.tensor(named[0][0], named[0][1], torch.float32, lambda t: t.dim() == 4 and t.shape[1] == 5,
                     "[%s, 5, H, W]" % ("4N" if views is None else "views N"))
    B, _, H, W = first.shape
    V = 4 if views is None else _tta_views(what, views, H, W)
    if B % V:
        raise ValueError("%s: a batch of %d logits is not %s per image" % (what, B, "four flips" if views is None else "%d views" % V))
    for name, t in named[1:]:
        a.tensor(name, t, torch.float32, first.shape, "%s like %s" % (list(first.shape), named[0][0]))
    out = a.out(out, torch.uint8, (B // V, H, W, 5))
    a.placed()
    return B // V, H, W, V, out


def xbd_tta_pack(pre_u8, post_u8, order="bgr", out=None):
    """The input batch of the reference's predictor (xBD_code/predict_test_cls.py:62-75) on the device.
    pre_u8, post_u8 [N, H, W, 3] uint8 -> [4N, 6, H, W] float32: image 4n + k is flip_k of concat(pre_n, post_n), every byte as
    float32(v) / 127 - 1; flip_0 identity, flip_1 rows reversed, flip_2 columns reversed, flip_3 both.
    order: 'bgr' (default) reverses the three channels of pre and of post -- what the script executes, because cv2.imread
    returns BGR while these sources hold RGB; 'rgb' keeps them, the order train.py's PIL loader and this project's loader feed
    the net.  out: a [4N, 6, H, W] float32 buffer to write into.  ValueError, before any launch, for a wrong rank, dtype or
    device, non-contiguous storage or an unknown order."""
    N, H, W, _, out = _tta_pack_args("xbd_tta_pack", pre_u8, post_u8, order, None, out)
    _call("dh_xbd_tta_pack_u8", _vp(pre_u8.data_ptr()), _vp(post_u8.data_ptr()), N, H, W, XBD_TTA_ORDER[order],
          _vp(out.data_ptr()), S())
    return out


def xbd_tta_merge(logits, out=None):
    """The merge of the reference's predictor (predict_test_cls.py:83-94) on the device.  logits [4N, 5, H, W] float32, image
    4n + k the net's answer to flip_k -> [N, H, W, 5] uint8, channels last: sigmoid in float32, each map flipped back,
    (((u_0 + u_1) + u_2) + u_3) / 4 in float32 in that order (numpy's mean over the stack), uint8(trunc(mean * 255)).  A NaN
    logit gives 0.  out: a [N, H, W, 5] uint8 buffer to write into.  ValueError, before any launch, for a wrong rank, dtype or
    device, non-contiguous storage or a batch that is no multiple of 4."""
    N, H, W, _, out = _tta_merge_args("xbd_tta_merge", [("logits", logits)], None, out)
    _call("dh_xbd_tta_merge_u8", _vp(logits.data_ptr()), N, H, W, _vp(out.data_ptr()), S())
    return out


# ---- xBD prediction for several snapshots and 4 or 8 views (csrc/xbd_ensemble.hip) -------------------------
XBD_TTA_VIEWS = (4, 8)
XBD_TTA_MAX_MODELS = 8


def _tta_views(what, views, H, W):
    if isinstance(views, bool) or views not in XBD_TTA_VIEWS:
        raise ValueError("%s: views=%r is not one of %s" % (what, views, list(XBD_TTA_VIEWS)))
    if views == 8 and H != W:
        raise ValueError("%s: views=8 adds the transposes, which need a square image; got %dx%d" % (what, H, W))
    return int(views)


def xbd_tta_pack_views(pre_u8, post_u8, order="bgr", views=4, out=None):
    """xbd_tta_pack for 4 or 8 views.  pre_u8, post_u8 [N, H, W, 3] uint8 -> [views * N, 6, H, W] float32: image views * n + v is
    view_v of concat(pre_n, post_n), every byte as float32(b) / 127 - 1.  view_v = flip_v for v < 4 (xbd_tta_pack's flips: with
    views=4 the same bytes as that call); view_{4+k} is the transpose of flip_k, so the eight views are the symmetries of the
    square: identity, the two flips, rot180, transpose, anti-transpose and both rot90.  views=8 needs H == W.  order and out as
    in xbd_tta_pack.  ValueError, before any launch, for a wrong rank, dtype or device, non-contiguous storage, an unknown
    order, views outside {4, 8} or views=8 on an image that is not square."""
    N, H, W, V, out = _tta_pack_args("xbd_tta_pack_views", pre_u8, post_u8, order, views, out)
    _call("dh_xbd_tta_pack_views_u8", _vp(pre_u8.data_ptr()), _vp(post_u8.data_ptr()), N, H, W, XBD_TTA_ORDER[order], V,
          _vp(out.data_ptr()), S())
    return out


def xbd_tta_merge_multi(logits_list, views=4, out=None):
    """xbd_tta_merge for a list of models and 4 or 8 views.  logits_list: 1 .. 8 tensors [views * N, 5, H, W] float32 of one
    shape on one device, entry m the answers of model m to xbd_tta_pack_views' batch -> [N, H, W, 5] uint8, channels last.
    Per pixel and channel in float32: every sigmoid with its view undone, added one after the other, model-major and
    view-minor (the order in which the script appends to its stack, which numpy's mean(axis=0) then adds in), divided by
    float32(M * views), uint8(trunc(mean * 255)).  A NaN gives 0.  With one model and views=4 the same bytes as xbd_tta_merge.
    ValueError, before any launch, for an empty or too long list, a wrong rank, dtype or device, non-contiguous storage,
    tensors of different shapes, views outside {4, 8}, a batch that is no multiple of views or views=8 with H != W."""
    what = "xbd_tta_merge_multi"
    if not isinstance(logits_list, (list, tuple)) or not 1 <= len(logits_list) <= XBD_TTA_MAX_MODELS:
        raise ValueError("%s: logits_list is not a list of 1 .. %d tensors (%s)" % (
            what, XBD_TTA_MAX_MODELS, len(logits_list) if isinstance(logits_list, (list, tuple)) else type(logits_list)))
    N, H, W, V, out = _tta_merge_args(what, [("logits_list[%d]" % m, t) for m, t in enumerate(logits_list)], views, out)
    table = (ctypes.c_void_p * len(logits_list))(*[t.data_ptr() for t in logits_list])      # read by the entry, not the kernel
    _call("dh_xbd_tta_merge_multi_u8", ctypes.cast(table, ctypes.c_void_p), len(logits_list), V, N, H, W, _vp(out.data_ptr()), S())
    return out


# ---- xBD damage map and visual grid (csrc/xbd_visual.hip) --------------------------------------------------
XBD_LOC_THR = (0.38, 0.13, 0.14)          # _thr of xBD_code/visualize_results.py


_XBD_BYTE_P = [v / 255 for v in range(256)]          # the script's loc_preds for each byte, float64, increasing


def xbd_loc_bounds(loc):
    """The localisation rule of visualize_results.py:209 in the kernel's terms: (use_loc, b0, b1, b2).  loc None: no rule,
    (0, 0, 0, 0).  loc one number t (a float, a 0-d array or tensor): (t, t, t); else three thresholds (t0, t1, t2).  b_i is the
    smallest byte v with v / 255 > t_i in float64 -- the script's own comparison: the position of t_i among the 256 quotients,
    which increase with v -- or 256 if no byte exceeds t_i, so that the kernel's v >= b_i is the script's v / 255 > t_i.
    (Not ceil(t * 255): 0.2 * 255 rounds to 51.0 while 51 / 255 > 0.2 is false.)  ValueError for a non-finite threshold or
    another count than three."""
    if loc is None:
        return (0, 0, 0, 0)
    try:
        thr = [float(t) for t in loc] if isinstance(loc, (tuple, list)) else [float(loc)] * 3
    except (TypeError, ValueError):
        try:
            thr = [float(t) for t in loc]          # any other iterable of numbers, such as a 1-d array
        except (TypeError, ValueError):
            raise ValueError("xbd_loc_bounds: loc %r is neither None, a number nor three numbers" % (loc,))
    if len(thr) != 3:
        raise ValueError("xbd_loc_bounds: loc %r holds %d thresholds, the rule has three" % (loc, len(thr)))
    if not all(math.isfinite(t) for t in thr):
        raise ValueError("xbd_loc_bounds: loc %r holds a non-finite threshold" % (loc,))
    return (1,) + tuple(bisect.bisect_right(_XBD_BYTE_P, t) for t in thr)


def xbd_damage_map(msk_u8, loc=None, out=None):
    """The damage class of visualize_results.py:206-211 per pixel, on the device.  msk_u8 [N, H, W, 5] uint8, channels last
    (what xbd_tta_merge returns) -> [N, H, W] uint8: 1 + the index of the first maximum of channels 1 .. 4, the script's
    msk[..., 1:].argmax(axis=2) + 1, so 1 .. 4 and a tie goes to the lowest channel.
    loc: None (default) stops there, as the script executes (its line 211 is commented out).  Three thresholds (t0, t1, t2), or
    one float for all three, multiply the class by the script's rule with p = msk_u8[..., 0] / 255 in float64,
        (p > t0) | ((p > t1) & (dmg > 1) & (dmg < 4)) | ((p > t2) & (dmg > 1)),
    so a dropped pixel is class 0; XBD_LOC_THR holds the script's _thr.  The script takes p from a separate localisation net;
    here it is channel 0 of the same prediction.  out: a [N, H, W] uint8 buffer to write into.  ValueError, before any launch,
    for a wrong rank, dtype or device, non-contiguous storage or a non-finite threshold."""
    use, b0, b1, b2 = xbd_loc_bounds(loc)
    a = _Args("xbd_damage_map")
    N, H, W = a.tensor("msk_u8", msk_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[3] == 5, "[N, H, W, 5]").shape[:3]
    out = a.out(out, torch.uint8, (N, H, W))
    a.placed()
    _call("dh_xbd_damage_map_u8", _vp(msk_u8.data_ptr()), N, H, W, use, b0, b1, b2, _vp(out.data_ptr()), S())
    return out


def xbd_vis_grid(pre_u8, post_u8, gt_u8, msk_u8, loc=None, out=None):
    """The picture of visualize_results.py:213-220 on the device: [N, H, 4W, 3] uint8, RGB, the four panels side by side,
        pre_u8 | post_u8 | colour(gt_u8) | colour(class of msk_u8)
    pre_u8, post_u8 [N, H, W, 3] uint8 as stored; gt_u8 [N, H, W] uint8, classes 0 .. 4; msk_u8 [N, H, W, 5] uint8 and loc as in
    xbd_damage_map (the class is computed inside the kernel, no class map is written).  Colours, RGB: 0 (0, 0, 0), 1 (0, 255, 0),
    2 (255, 255, 0), 3 (255, 127, 0), 4 (255, 0, 0) -- the script's color_dict, which is in cv2's BGR; its array is this one with
    the last axis reversed.  A label above 4, a KeyError in the script, is painted (255, 0, 255) here; models/xbd.visual_grid
    raises.  out: a [N, H, 4W, 3] uint8 buffer to write into.  ValueError, before any launch, for a wrong rank, dtype or device,
    non-contiguous storage, shapes that do not agree or a non-finite threshold."""
    use, b0, b1, b2 = xbd_loc_bounds(loc)
    a = _Args("xbd_vis_grid")
    N, H, W = a.tensor("msk_u8", msk_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[3] == 5, "[N, H, W, 5]").shape[:3]
    for name, t, tail in (("pre_u8", pre_u8, (3,)), ("post_u8", post_u8, (3,)), ("gt_u8", gt_u8, ())):
        a.tensor(name, t, torch.uint8, (N, H, W) + tail, "%s like msk_u8" % list((N, H, W) + tail))
    out = a.out(out, torch.uint8, (N, H, 4 * W, 3))
    a.placed()
    _call("dh_xbd_vis_grid_u8", _vp(pre_u8.data_ptr()), _vp(post_u8.data_ptr()), _vp(gt_u8.data_ptr()), _vp(msk_u8.data_ptr()),
          N, H, W, use, b0, b1, b2, _vp(out.data_ptr()), S())
    return out


# ---- xBD buildings: components, statistics, vote, paint (csrc/xbd_buildings.hip) --------------------------
XBD_CC_TILE = (32, 64)           # (TH, TW) of the tile-local pass: dh_xbd_cc_tile_h / dh_xbd_cc_tile_w
XBD_CC_COLS = 10                 # area, h0 .. h4, y0, x0, y1, x1
XBD_CC_MODES = {"damage": 0, "all": 1}


def _cc_image(what, name, t, dtype):
    return _Args(what).image(name, t, dtype)


def _cc_cap(what, cap):
    if isinstance(cap, bool) or not isinstance(cap, int) or cap < 1:
        raise ValueError("%s: cap %r is not an integer >= 1" % (what, cap))


def _out_pair(what, out, names):
    """`out` of a call that returns two tensors: the pair given, or (None, None)"""
    if out is None:
        return None, None
    if not (isinstance(out, (tuple, list)) and len(out) == 2):
        raise ValueError("%s: out is a pair (%s)" % (what, names))
    return out


def xbd_cc_ws_bytes(N, H, W):
    """bytes of the workspace xbd_cc_label needs for [N, H, W]: parents int32 [N, H W] + block counts [N, ceil(H W / 1024)]"""
    return _ws_bytes("dh_xbd_cc_ws_bytes", N, H, W)


def xbd_cc_label(key_u8, connectivity=8, keyed=False, out=None, ws=None):
    """Connected components on the device.  key_u8 [N, H, W] uint8 -> (labels [N, H, W] int32, count [N] int32).  Neighbours
    (connectivity 4, or 8 with the diagonals) belong together when both keys are nonzero, with keyed=True when they are nonzero
    and equal.  labels is 0 where the key is 0 and 1 .. count[n] elsewhere, numbered per image in raster order of each
    component's first pixel -- scipy.ndimage.label's numbering.  Six launches whatever the data, nothing read back, bit-exact.
    out: (labels, count) buffers to write into.  ws: a uint8 device buffer of xbd_cc_ws_bytes(N, H, W) bytes or more (default:
    a fresh one).  ValueError, before any launch, for a wrong rank, dtype or device, non-contiguous storage, a connectivity
    other than 4 or 8 or an `out` / `ws` that does not fit."""
    what = "xbd_cc_label"
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity %r is neither 4 nor 8" % (what, connectivity))
    a = _Args(what)
    N, H, W = a.image("key_u8", key_u8, torch.uint8)
    labels, count = _out_pair(what, out, "labels, count")
    labels = a.out(labels, torch.int32, (N, H, W), "out[0]", "labels %s" % [N, H, W])
    count = a.out(count, torch.int32, (N,), "out[1]", "count %s" % [N])
    a.workspace(ws)
    a.placed()
    ws = _workspace(what, ws, xbd_cc_ws_bytes(N, H, W), key_u8.device)
    _call("dh_xbd_cc_label", _vp(key_u8.data_ptr()), N, H, W, connectivity, int(bool(keyed)), _vp(labels.data_ptr()),
          _vp(count.data_ptr()), _vp(ws.data_ptr()), ws.numel(), S())
    return labels, count


def xbd_cc_stats(labels, vote_u8, cap, out=None):
    """Per-component statistics: labels [N, H, W] int32 (xbd_cc_label's), vote_u8 [N, H, W] uint8, cap >= 1 -> table
    [N, cap, 10] int32; row i describes label i + 1: area, h0 .. h4 (pixels whose vote is 0 .. 4; a larger byte counts in the area
    only), y0, x0, y1, x1 (inclusive box).  Rows of labels that do not exist: area 0, h 0, y0 = H, x0 = W, y1 = x1 = -1.  Labels
    above cap are ignored.  Every int of the table is written.  out: a [N, cap, 10] int32 buffer to write into."""
    what = "xbd_cc_stats"
    _cc_cap(what, cap)
    a = _Args(what)
    N, H, W = a.image("labels", labels, torch.int32)
    a.tensor("vote_u8", vote_u8, torch.uint8, (N, H, W), "%s like labels" % [N, H, W])
    out = a.out(out, torch.int32, (N, cap, XBD_CC_COLS))
    a.placed()
    _call("dh_xbd_cc_stats", _vp(labels.data_ptr()), _vp(vote_u8.data_ptr()), N, H, W, cap, _vp(out.data_ptr()), S())
    return out


def xbd_cc_vote(table, min_area=0, mode="damage", out=None):
    """The class of every table row: table [N, cap, 10] int32 -> cls [N, cap] uint8.  mode 'damage': 1 + the first maximum of
    h1 .. h4, 0 when all four are zero; mode 'all': the first maximum of h0 .. h4; a tie goes to the lowest class.  Rows with
    area 0 or area < min_area get 0.  out: a [N, cap] uint8 buffer to write into."""
    what = "xbd_cc_vote"
    if mode not in XBD_CC_MODES:
        raise ValueError("%s: mode %r is neither 'damage' nor 'all'" % (what, mode))
    if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 0:
        raise ValueError("%s: min_area %r is not an integer >= 0" % (what, min_area))
    a = _Args(what)
    a.tensor("table", table, torch.int32, lambda t: t.dim() == 3 and t.shape[2] == XBD_CC_COLS and t.numel() > 0,
             "[N, cap, %d], not empty" % XBD_CC_COLS)
    N, cap = table.shape[:2]
    out = a.out(out, torch.uint8, (N, cap))
    a.placed()
    _call("dh_xbd_cc_vote", _vp(table.data_ptr()), N, cap, min_area, XBD_CC_MODES[mode], _vp(out.data_ptr()), S())
    return out


def xbd_cc_paint(labels, cls_u8, out=None):
    """The one-class-per-component map: labels [N, H, W] int32, cls_u8 [N, cap] uint8 -> [N, H, W] uint8, cls_u8[n, l - 1] for a
    pixel with label l, 0 for l = 0 or l > cap.  Every byte is written.  out: a [N, H, W] uint8 buffer to write into."""
    what = "xbd_cc_paint"
    a = _Args(what)
    N, H, W = a.image("labels", labels, torch.int32)
    a.tensor("cls_u8", cls_u8, torch.uint8, lambda t: t.dim() == 2 and t.shape[0] == N and t.shape[1] >= 1, "[%d, cap >= 1]" % N)
    out = a.out(out, torch.uint8, (N, H, W))
    a.placed()
    _call("dh_xbd_cc_paint", _vp(labels.data_ptr()), _vp(cls_u8.data_ptr()), N, H, W, cls_u8.shape[1], _vp(out.data_ptr()), S())
    return out


XBD_CC_MATCH_COLS = 5            # area, maj, inter, maj_area, match
XBD_CC_MATCH_MAX_DEN = 32768


def _cc_iou(what, iou):
    """(num, den) of an IoU threshold given as a pair of ints, 1 <= num <= den <= 32768 and num / den >= 1 / 2.  A float is
    refused: 0.5 and 2 / 3 have to be exact."""
    ok = isinstance(iou, (tuple, list)) and len(iou) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in iou)
    if not ok or not (1 <= iou[0] <= iou[1] <= XBD_CC_MATCH_MAX_DEN and 2 * iou[0] >= iou[1]):
        raise ValueError("%s: iou %r is not a pair of ints (num, den) with 1 <= num <= den <= %d and 2 num >= den"
                         % (what, iou, XBD_CC_MATCH_MAX_DEN))
    return int(iou[0]), int(iou[1])


def xbd_cc_match_ws_bytes(N, cap_a, cap_b):
    """bytes of the workspace xbd_cc_match needs: int32 rows [N, cap_a, NB + 1] with NB = cap_b.bit_length(), the areas of B
    [N, cap_b], candidates and intersections [N, cap_a] each"""
    return _ws_bytes("dh_xbd_cc_match_ws_bytes", N, cap_a, cap_b)


def xbd_cc_match(labels_a, labels_b, cap_a, cap_b, iou=(1, 2), out=None, ws=None):
    """Two label maps matched by intersection over union, on the device.  labels_a (predicted buildings, 1 .. cap_a) and
    labels_b (true buildings, 1 .. cap_b), both [N, H, W] int32 as xbd_cc_label writes them; labels outside 1 .. cap are
    background.  Returns (match_a [N, cap_a, 5] int32, match_b [N, cap_b] int32).  Row i of match_a describes label i + 1 of A:
    area, maj (the label of B that covers more than half of it, or 0), inter and maj_area (its intersection with maj and maj's
    area, 0 without one) and match = maj if inter * den > num * (area + maj_area - inter), else 0, with iou = (num, den) ints,
    1 <= num <= den <= 32768, 2 num >= den (strict, exact; one-to-one).  match_b[n, j] is the label of A matched to label j + 1 of
    B, or 0.  Rows of labels that do not exist are 0; every int is written.  Five launches whatever the data, nothing read back,
    bit-exact.  out: (match_a, match_b) buffers to write into.  ws: a uint8 device buffer of xbd_cc_match_ws_bytes(N, cap_a,
    cap_b) bytes or more (default: a fresh one).  ValueError, before any launch, for a wrong rank, dtype, device or shape,
    non-contiguous storage, a bad cap or iou (a float among them) or an `out` / `ws` that does not fit."""
    what = "xbd_cc_match"
    _cc_cap(what, cap_a)
    _cc_cap(what, cap_b)
    num, den = _cc_iou(what, iou)
    a = _Args(what)
    N, H, W = a.image("labels_a", labels_a, torch.int32)
    a.tensor("labels_b", labels_b, torch.int32, (N, H, W), "%s like labels_a" % [N, H, W])
    match_a, match_b = _out_pair(what, out, "match_a, match_b")
    match_a = a.out(match_a, torch.int32, (N, cap_a, XBD_CC_MATCH_COLS), "out[0]", "match_a %s" % [N, cap_a, XBD_CC_MATCH_COLS])
    match_b = a.out(match_b, torch.int32, (N, cap_b), "out[1]", "match_b %s" % [N, cap_b])
    a.workspace(ws)
    a.placed()
    ws = _workspace(what, ws, xbd_cc_match_ws_bytes(N, cap_a, cap_b), labels_a.device)
    _call("dh_xbd_cc_match", _vp(labels_a.data_ptr()), _vp(labels_b.data_ptr()), N, H, W, cap_a, cap_b, num, den,
          _vp(match_a.data_ptr()), _vp(match_b.data_ptr()), _vp(ws.data_ptr()), ws.numel(), S())
    return match_a, match_b


# ---- xBD masks: morphology, the dilated training masks, hole filling (csrc/xbd_morph.hip) -------------------
XBD_MORPH_TILE = (32, 64)        # (TH, TW) of the window kernel's output tile: dh_xbd_morph_tile_h / dh_xbd_morph_tile_w
XBD_MORPH_MAX_K = 31
XBD_MORPH_OPS = {"dilate": 0, "erode": 1}


def _morph_k(what, k, lo=1):
    if isinstance(k, bool) or not isinstance(k, int) or k < lo or k > XBD_MORPH_MAX_K or k % 2 == 0:
        raise ValueError("%s: k %r is not an odd integer of %d .. %d" % (what, k, lo, XBD_MORPH_MAX_K))


def _morph_apart(what, name, src, out):
    """an output that shares bytes with its input: a window reads its neighbours"""
    if out is not None and src.numel() and out.numel():
        a, b = src.data_ptr(), out.data_ptr()
        if a < b + out.numel() * out.element_size() and b < a + src.numel() * src.element_size():
            raise ValueError("%s: out overlaps %s" % (what, name))


def xbd_morph(map_u8, op, k, out=None):
    """Binary morphology with a k x k square on the device.  map_u8 [N, H, W] uint8 (nonzero = set) -> [N, H, W] uint8, 0 / 1.
    op 'dilate': set where any pixel of the window centred on it is set, everything outside the image clear --
    scipy.ndimage.binary_dilation(a, structure=ones((k, k))), skimage's dilation(a, square(k)).  op 'erode': set where every pixel
    of the window is set, everything outside the image set -- binary_erosion(a, structure=ones((k, k)), border_value=1), skimage's
    erosion.  k: odd, 1 .. 31 (1 is `map_u8 != 0`).  One launch, bit-exact.  out: a [N, H, W] uint8 buffer to write into, not the
    input.  ValueError, before any launch, for a wrong rank, dtype or device, non-contiguous storage, an even k, a k outside
    1 .. 31 or a bool or float, an unknown op, or an `out` that is the input or does not fit."""
    what = "xbd_morph"
    if not isinstance(op, str) or op not in XBD_MORPH_OPS:
        raise ValueError("%s: op %r is neither 'dilate' nor 'erode'" % (what, op))
    _morph_k(what, k)
    a = _Args(what)
    N, H, W = a.image("map_u8", map_u8, torch.uint8)
    out = a.out(out, torch.uint8, (N, H, W))
    a.placed()
    _morph_apart(what, "map_u8", map_u8, out)
    _call("dh_xbd_morph_u8", _vp(map_u8.data_ptr()), N, H, W, k, XBD_MORPH_OPS[op], _vp(out.data_ptr()), S())
    return out


def xbd_msk_dilate(msk_u8, k=5, out=None):
    """The dilated, prioritised training masks of xBD_code/train_unettransformer.py:262-273 on the device.  msk_u8 [N, 5, H, W]
    uint8 mask channels (what the loader's augment launch writes; nonzero = set) -> [N, 5, H, W] uint8, 0 / 1: with
    d_c = dilation(msk[c], square(k)) for c = 1 .. 4 (channel 0 is not read),
        out[2] = d2, out[3] = d3 & ~d2, out[4] = d4 & ~d2 & ~d3, out[1] = d1 & ~(d2 | d3 | d4), out[0] = out[1] | .. | out[4].
    k: odd, 1 .. 31; 5 is the script's square(5).  One launch, bit-exact.  out: a [N, 5, H, W] uint8 buffer, not the input.
    ValueError, before any launch, as xbd_morph."""
    what = "xbd_msk_dilate"
    _morph_k(what, k)
    a = _Args(what)
    a.tensor("msk_u8", msk_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[1] == 5 and t.numel() > 0, "[N, 5, H, W], not empty")
    N, _, H, W = msk_u8.shape
    out = a.out(out, torch.uint8, (N, 5, H, W))
    a.placed()
    _morph_apart(what, "msk_u8", msk_u8, out)
    _call("dh_xbd_msk_dilate_u8", _vp(msk_u8.data_ptr()), N, H, W, k, _vp(out.data_ptr()), S())
    return out


# ---- xBD class table: the bytes of every class in every resident label (csrc/xbd_classes.hip) ----------------
XBD_CLASS_COLUMNS = ("class0", "class1", "class2", "class3", "class4", "above4")


def xbd_class_table(labels_u8, out=None):
    """How many bytes of every label equal 0, 1, 2, 3, 4 or lie above 4, in one pass on the device (dh_xbd_class_table_u8).
    labels_u8 [n, H, W] uint8, contiguous -- GpuXbdPipeline's post_label stack, or a slice of it along the first axis: no
    alignment is asked -- -> int32 [n, 6], columns XBD_CLASS_COLUMNS; a row sums to H * W.  The training scripts' file_classes
    (fl[c - 1] = c in msk1) is table[:, 1:5] > 0.  A memset node and one launch; integer adds only, so the table is exact and the
    same bits on every call.  out: an [n, 6] int32 buffer to write into; every word of it is overwritten.
    ValueError, before any launch, for a wrong rank or dtype, n == 0 or an empty image, H * W > 2^31 - 1, tensors on different
    devices or non-contiguous storage; HipLibraryError for CPU tensors (there is no CPU path)."""
    a = _Args("xbd_class_table", cpu_error=True)
    n, H, W = a.tensor("labels_u8", labels_u8, torch.uint8, lambda t: t.dim() == 3 and t.numel() > 0 and t.shape[1] * t.shape[2] < 2 ** 31,
                       "[n, H, W], not empty, H * W <= 2^31 - 1").shape
    out = a.out(out, torch.int32, (n, len(XBD_CLASS_COLUMNS)))
    a.placed()
    _call("dh_xbd_class_table_u8", P(labels_u8), n, H * W, P(out), S())
    return out


# ---- device loaders: the pair loader and xBD_code/train.py's (csrc/pointwise.hip, augment_blur.hip, augment_xbd.hip) --------
def augment_pairs(a_u8, b_u8, l_u8, idx, params, h, w, blur=None, out_a=None, out_b=None, out_l=None):
    """One batch of the change-detection pair loader in ONE launch (dh_augment_pairs_u8; with `blur` dh_augment_pairs_blur_u8).
    a_u8, b_u8 [S, H, W, 3] and l_u8 [S, H, W], or None for no labels: the resident uint8 sources; idx int32 [N]: the source of
    every sample; params int32 [N, 4] = (x0, y0, hflip, vflip) of its h x w window; blur int32 [N, 2] = the (ww, fw) rows of
    datasets/gpu_pipeline.blur_table, which checks their bounds, or None.  Returns (out_a, out_b fp32 [N, 3, h, w], out_l uint8
    [N, 1, h, w]), the given buffers or fresh ones; out_l is None without l_u8.  ValueError for whatever does not fit, before
    the launch; the caller range-checks idx and the windows (they are device memory)."""
    a = _Args("augment_pairs")
    n_src, H, W, _ = a.tensor("a_u8", a_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[3] == 3 and t.numel() > 0,
                              "[S, H, W, 3], not empty").shape
    a.tensor("b_u8", b_u8, torch.uint8, (n_src, H, W, 3))
    if l_u8 is not None:
        a.tensor("l_u8", l_u8, torch.uint8, (n_src, H, W))
    N = a.tensor("idx", idx, torch.int32, lambda t: t.dim() == 1, "[N]").shape[0]
    a.tensor("params", params, torch.int32, (N, 4), "[%d, 4]: a row per entry of idx" % N)
    if blur is not None:
        a.tensor("blur", blur, torch.int32, (N, 2), "[%d, 2]: a row per entry of idx" % N)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (h, w)) or not (1 <= h <= H and 1 <= w <= W):
        raise ValueError("augment_pairs: a %r x %r window does not fit the %dx%d sources" % (h, w, H, W))
    h, w = int(h), int(w)
    out_a = a.out(out_a, torch.float32, (N, 3, h, w), "out_a", "[%d, 3, %d, %d]: idx's N, h, w" % (N, h, w))
    out_b = a.out(out_b, torch.float32, (N, 3, h, w), "out_b", "[%d, 3, %d, %d]: idx's N, h, w" % (N, h, w))
    if l_u8 is not None:          # (the plain kernel reads l wherever it is given an out_l)
        out_l = a.out(out_l, torch.uint8, (N, 1, h, w), "out_l", "[%d, 1, %d, %d]: idx's N, h, w" % (N, h, w))
    elif out_l is not None:
        raise ValueError("augment_pairs: out_l is given and l_u8 is None: there is no label to cut")
    a.placed()
    if blur is None:
        _call("dh_augment_pairs_u8", P(a_u8), P(b_u8), P(l_u8), P(idx), P(params), N, H, W, h, w, P(out_a), P(out_b), P(out_l), S())
    else:
        _call("dh_augment_pairs_blur_u8", P(a_u8), P(b_u8), P(l_u8), P(idx), P(params), P(blur), N, H, W, h, w, P(out_a), P(out_b),
              P(out_l), S())
    return out_a, out_b, out_l


XBD_JITTER_WORDS = 8             # int32 words of a row of dh_xbd_augment_jitter_u8's table


def xbd_augment_jitter_ws_bytes(n, crop):
    """bytes of dh_xbd_augment_jitter_u8's workspace for n samples of crop x crop: the device copy of the table, then one
    partial sum of L per tile and image"""
    return n * 2 * (XBD_JITTER_WORDS + _lib.lib().dh_xbd_augment_jitter_tiles(crop)) * 4


def xbd_augment(pre_u8, post_u8, pre_mask_u8, post_label_u8, idx, params, coef, crop, train=True, jitter=None, out_img=None,
                out_msk=None, out_lbl=None, ws=None):
    """One batch of xBD_code/train.py's TrainData (train=True) or ValData in ONE launch (dh_xbd_augment_u8; the header states the
    arithmetic).  pre_u8, post_u8 [n_src, H, W, 3] and pre_mask_u8, post_label_u8 [n_src, H, W]: the resident uint8 sources;
    idx int32 [N]; params int32 [N, 9] rows in datasets/xbd_pipeline.PARAM_FIELDS order; coef int32 [N, 2, crop, 4], its
    coef_table, or None (no sample resizes).  Returns (out_img fp32 [N, 6, crop, crop], out_msk uint8 [N, 5, crop, crop],
    out_lbl uint8 [N, crop, crop]), the given buffers or fresh ones.  Train mode reads no pre mask and does NOT write out_lbl:
    it is what the caller passes (the pipeline's shared zero tensor).
    jitter: a C-contiguous int32 HOST array [N, 2, 8] (xbd_pipeline.jitter_table; train mode only) makes the call
    dh_xbd_augment_jitter_u8 -- ColorJitter on the samples whose rows are enabled, a second launch for contrast's mean; the
    entry checks the rows and copies them into the workspace before it returns.  ws: a uint8 device buffer of
    xbd_augment_jitter_ws_bytes(N, crop) bytes or more for that call (default: a fresh one).
    ValueError for whatever does not fit, before the launch; the caller range-checks idx and the rows (check_params)."""
    what = "xbd_augment"
    a = _Args(what)
    n_src, H, W, _ = a.tensor("pre_u8", pre_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[3] == 3 and t.numel() > 0,
                              "[n_src, H, W, 3], not empty").shape
    a.tensor("post_u8", post_u8, torch.uint8, (n_src, H, W, 3))
    a.tensor("pre_mask_u8", pre_mask_u8, torch.uint8, (n_src, H, W))
    a.tensor("post_label_u8", post_label_u8, torch.uint8, (n_src, H, W))
    N = a.tensor("idx", idx, torch.int32, lambda t: t.dim() == 1, "[N]").shape[0]
    a.tensor("params", params, torch.int32, (N, 9), "[%d, 9]: a row per entry of idx" % N)
    if isinstance(crop, bool) or not isinstance(crop, (int, np.integer)) or not 1 <= crop <= min(H, W):
        raise ValueError("%s: crop %r does not fit the %dx%d sources" % (what, crop, H, W))
    crop = int(crop)
    if coef is not None:
        a.tensor("coef", coef, torch.int32, (N, 2, crop, 4), "[%d, 2, %d, 4]: idx's N, crop" % (N, crop))
    out_img = a.out(out_img, torch.float32, (N, 6, crop, crop), "out_img", "[%d, 6, %d, %d]: idx's N, crop" % (N, crop, crop))
    out_msk = a.out(out_msk, torch.uint8, (N, 5, crop, crop), "out_msk", "[%d, 5, %d, %d]: idx's N, crop" % (N, crop, crop))
    if out_lbl is not None or not train:
        out_lbl = a.out(out_lbl, torch.uint8, (N, crop, crop), "out_lbl", "[%d, %d, %d]: idx's N, crop" % (N, crop, crop))
    if jitter is not None:
        if not train:
            raise ValueError("%s: jitter belongs to the training augmentation (train=False)" % what)
        if not (isinstance(jitter, np.ndarray) and jitter.dtype == np.int32 and jitter.shape == (N, 2, XBD_JITTER_WORDS)
                and jitter.flags.c_contiguous):
            raise ValueError("%s: jitter %s %s is not a C-contiguous int32 host array [%d, 2, %d]"
                             % (what, getattr(jitter, "shape", ()), getattr(jitter, "dtype", type(jitter)), N, XBD_JITTER_WORDS))
    a.workspace(ws)
    a.placed()
    src = (P(pre_u8), P(post_u8), P(None if train else pre_mask_u8), P(post_label_u8), P(idx), P(params), P(coef))
    dst = (N, H, W, crop, 0 if train else 1, P(out_img), P(out_msk), P(None if train else out_lbl))
    if jitter is None:
        _call("dh_xbd_augment_u8", *src, *dst, S())
    else:
        ws = _workspace(what, ws, xbd_augment_jitter_ws_bytes(N, crop), pre_u8.device)
        _call("dh_xbd_augment_jitter_u8", *src, _vp(jitter.ctypes.data), *dst, P(ws), ws.numel(), S())
    return out_img, out_msk, out_lbl


XBD_WARP_TILE = (32, 32)         # (TH, TW) of dh_xbd_augment_warp_u8's output tile: dh_xbd_augment_warp_tile_h / _tile_w
XBD_WARP_PARAM_WORDS = 12        # x0, y0, vflip, rot, sx, sy, warp, chan, dR, dG, dB, 0


def xbd_augment_warp(pre_u8, post_u8, label_u8, idx, params, tab, crop, out_img=None, out_msk=None):
    """One batch of xBD_code/train_unettransformer.py's TrainData.__getitem__ on the device (dh_xbd_augment_warp_u8; the header
    states the arithmetic): pre_u8, post_u8 [n_src, H, W, 3] uint8 RGB, label_u8 [n_src, H, W] uint8, idx [N] int32, params
    [N, 12] int32 rows, tab [N, 4, crop] int32 warp tables or None (no sample warps) -> (out_img fp32 [N, 6, crop, crop],
    out_msk uint8 [N, 5, crop, crop]).  One launch.  The rows and tables are datasets/xbd_pipeline's (unet_param_rows, unet_warp_table), which
    checks them; the kernel reads inside its sources whatever they hold.  ValueError, before any launch, for a wrong rank,
    dtype, shape or device or non-contiguous storage."""
    a = _Args("xbd_augment_warp")
    a.tensor("pre_u8", pre_u8, torch.uint8, lambda t: t.dim() == 4 and t.shape[3] == 3 and t.numel() > 0, "[n_src, H, W, 3], not empty")
    n_src, H, W, _ = pre_u8.shape
    a.tensor("post_u8", post_u8, torch.uint8, (n_src, H, W, 3))
    a.tensor("label_u8", label_u8, torch.uint8, (n_src, H, W))
    a.tensor("idx", idx, torch.int32, lambda t: t.dim() == 1 and t.numel() > 0, "[N], not empty")
    N = idx.numel()
    a.tensor("params", params, torch.int32, (N, XBD_WARP_PARAM_WORDS), "[%d, %d]: a row per entry of idx" % (N, XBD_WARP_PARAM_WORDS))
    if tab is not None:
        a.tensor("tab", tab, torch.int32, (N, 4, crop))
    out_img = a.out(out_img, torch.float32, (N, 6, crop, crop), "out_img")
    out_msk = a.out(out_msk, torch.uint8, (N, 5, crop, crop), "out_msk")
    a.placed()
    _call("dh_xbd_augment_warp_u8", P(pre_u8), P(post_u8), P(label_u8), P(idx), P(params), P(tab), N, H, W, crop, P(out_img),
          P(out_msk), S())
    return out_img, out_msk


XBD_COLOUR_TILE = 32             # the side of dh_xbd_unet_colour_u8's square tile: dh_xbd_unet_colour_tile
XBD_COLOUR_JOB_WORDS = 12        # sample, image, hsv flag, h, s, v, op, factor bits (low, high), noise plane, 0, 0


def xbd_unet_colour_ws_bytes(J, crop):
    """bytes of the workspace xbd_unet_colour needs for J jobs on crop x crop images: their bytes [J, 3, crop, crop] and one
    int32 sum per tile and channel"""
    return _ws_bytes("dh_xbd_unet_colour_ws_bytes", J, crop)


def xbd_unet_colour(img, jobs, noise, ws=None):
    """The colour stage of xBD_code/train_unettransformer.py's TrainData (lines 211-244: change_hsv, then gauss_noise, cv2.blur,
    saturation, brightness or contrast) on the device, IN PLACE on img fp32 [N, 6, S, S] as xbd_augment_warp wrote it
    (dh_xbd_unet_colour_u8; the header states the arithmetic).  jobs [J, 12] int32 rows, one per (sample, image) that drew
    anything, and noise [K, S, S, 3] uint8 or None, both datasets/xbd_pipeline.unet_colour_jobs'.  Two launches whatever the
    jobs; samples without a row are not touched.  Returns img.  ws: a uint8 device buffer of xbd_unet_colour_ws_bytes(J, S)
    bytes or more (default: a fresh one).  The kernels stay inside their buffers whatever the rows hold.  ValueError, before
    any launch, for a wrong rank, dtype, shape or device, non-contiguous storage or a `ws` that does not fit."""
    what = "xbd_unet_colour"
    a = _Args(what)
    a.tensor("img", img, torch.float32, lambda t: t.dim() == 4 and t.shape[1] == 6 and t.shape[2] == t.shape[3] and t.numel() > 0,
             "[N, 6, S, S], not empty")
    N, _, side, _ = img.shape
    a.tensor("jobs", jobs, torch.int32, lambda t: t.dim() == 2 and t.shape[1] == XBD_COLOUR_JOB_WORDS and t.shape[0] > 0,
             "[J, %d], not empty" % XBD_COLOUR_JOB_WORDS)
    J, K = jobs.shape[0], 0
    if noise is not None:
        a.tensor("noise", noise, torch.uint8, lambda t: t.dim() == 4 and tuple(t.shape[1:]) == (side, side, 3) and t.shape[0] > 0,
                 "[K, %d, %d, 3], not empty" % (side, side))
        K = noise.shape[0]
    a.workspace(ws)
    a.placed()
    ws = _workspace(what, ws, xbd_unet_colour_ws_bytes(J, side), img.device)
    _call("dh_xbd_unet_colour_u8", P(img), P(jobs), P(noise), N, side, J, K, P(ws), ws.numel(), S())
    return img


def xbd_fill_holes_ws_bytes(N, H, W):
    """bytes of the workspace xbd_fill_holes needs for [N, H, W]: labels int32 [N, H W] and count [N], xbd_cc_label's own
    workspace, the key uint8 [N, H W] and the marks uint8 [N, H W + 1] (each padded to four bytes)"""
    return _ws_bytes("dh_xbd_fill_holes_ws_bytes", N, H, W)


def xbd_fill_holes(map_u8, background=4, out=None, ws=None):
    """Hole filling on the device.  map_u8 [N, H, W] uint8 (nonzero = set) -> [N, H, W] uint8, 0 / 1: the set pixels, plus every
    component of the clear ones (connectivity `background`, 4 or 8) that has no pixel on the image border --
    scipy.ndimage.binary_fill_holes(a, structure=generate_binary_structure(2, 1)) for 4 (scipy's default), (2, 2) for 8.  Nine
    launches whatever the data (xbd_cc_label's six among them), nothing read back, no cap on the number of holes, bit-exact.
    out: a [N, H, W] uint8 buffer to write into, not the input.  ws: a uint8 device buffer of xbd_fill_holes_ws_bytes(N, H, W)
    bytes or more (default: a fresh one).  ValueError, before any launch, for a wrong rank, dtype or device, non-contiguous
    storage, a background other than 4 or 8, an `out` that is the input or does not fit, or a short or misaligned `ws`."""
    what = "xbd_fill_holes"
    if isinstance(background, bool) or not isinstance(background, int) or background not in (4, 8):
        raise ValueError("%s: background connectivity %r is neither 4 nor 8" % (what, background))
    a = _Args(what)
    N, H, W = a.image("map_u8", map_u8, torch.uint8)
    out = a.out(out, torch.uint8, (N, H, W))
    a.workspace(ws)
    a.placed()
    _morph_apart(what, "map_u8", map_u8, out)
    ws = _workspace(what, ws, xbd_fill_holes_ws_bytes(N, H, W), map_u8.device)
    _call("dh_xbd_fill_holes_u8", _vp(map_u8.data_ptr()), N, H, W, int(background), _vp(out.data_ptr()), _vp(ws.data_ptr()),
          ws.numel(), S())
    return out


# ---- the change-detection evaluator's picture (csrc/cd_visual.hip) -----------------------------------------
def cd_vis_shape(N, H, W):
    """the shape of the evaluator's picture of N images H x W: make_grid's min(8, N) tiles per row, padding 0, four bands"""
    cols = min(8, N)
    return (4 * ((N + cols - 1) // cols) * H, cols * W, 3)


def cd_eval_vis(a, b, logits, label, out=None):
    """The picture of the reference's models/evaluator.py:118-131 for one batch, on the device: [4 * rows * H, cols * W, 3] uint8
    RGB (cd_vis_shape), the grids of A, B, the prediction and the ground truth stacked top to bottom, 8 images per row.
    a, b float32 [N, 3, H, W] as the net receives them: byte = trunc(clip(x * 0.5 + 0.5, 0, 1) * 255), truncated as
    plt.imsave truncates; logits float32 [N, C, H, W]: white where argmax_nchw's class is >= 1; label int64 [N, H, W] or
    [N, 1, H, W]: white where it is >= 1.  Tile positions beyond N are black.  out: a uint8 buffer of that shape to write into.
    One launch writes every byte.  ValueError, before any launch, for a wrong rank or dtype, shapes that do not agree, tensors
    on different devices or non-contiguous storage; HipLibraryError for CPU tensors (there is no CPU path)."""
    args = _Args("cd_eval_vis", cpu_error=True)
    args.tensor("a", a, torch.float32, lambda t: t.dim() == 4 and t.shape[1] == 3 and t.numel() > 0, "[N, 3, H, W]")
    N, _, H, W = a.shape
    args.tensor("b", b, torch.float32, (N, 3, H, W), "%s like a" % [N, 3, H, W])
    args.tensor("logits", logits, torch.float32, lambda t: t.dim() == 4 and t.shape[1] >= 1 and (t.shape[0],) + tuple(t.shape[2:]) == (N, H, W),
                "[%d, C, %d, %d] like a" % (N, H, W))
    args.tensor("label", label, torch.int64, lambda t: tuple(t.shape) in ((N, H, W), (N, 1, H, W)),
                "%s or %s like a" % ([N, H, W], [N, 1, H, W]))
    out = args.out(out, torch.uint8, cd_vis_shape(N, H, W))
    args.placed()
    _call("dh_cd_eval_vis_u8", _vp(a.data_ptr()), _vp(b.data_ptr()), _vp(logits.data_ptr()), _vp(label.data_ptr()), N,
          logits.shape[1], H, W, _vp(out.data_ptr()), S())
    return out


# ---- whole-tile change maps (tiles.TilePlan; csrc/cd_tile.hip) -----------------------------------------------
_TILE_TABLES = {}        # (plan, device) -> the plan's tables on that device, built once


def tile_tables(plan, device):
    """The tables dh_cd_tile_stitch reads for `plan`, on `device`: {'ys', 'xs', 'flips', 'rows', 'cols'} int32 and {'wy', 'wx'}
    float32, views into one buffer each, built on the host from the plan once per (plan, device) and kept."""
    key = (plan, str(torch.device(device)))
    t = _TILE_TABLES.get(key)
    if t is None:
        import numpy as np
        rows, cols = plan.cover()
        wy, wx = plan.weights()
        ints = [("ys", np.asarray(plan.ys, dtype=np.int32)), ("xs", np.asarray(plan.xs, dtype=np.int32)),
                ("flips", np.asarray(plan.flips, dtype=np.int32)), ("rows", rows.reshape(-1)), ("cols", cols.reshape(-1))]
        flat_i = torch.from_numpy(np.concatenate([a for _, a in ints])).to(device)
        flat_f = torch.from_numpy(np.concatenate([wy, wx])).to(device)
        t, o = {"_keep": (flat_i, flat_f)}, 0
        for name, a in ints:
            t[name] = flat_i[o:o + a.size]
            o += a.size
        t["wy"], t["wx"] = flat_f[:plan.h], flat_f[plan.h:]
        _TILE_TABLES[key] = t
    return t


def cd_tile_stitch(logits, plan, out_logits=None, out_mask=None, label=None, counts=None, label_index=None):
    """The change map of a whole tile from the net's answers to its windows (tiles.TilePlan), on the device.
    logits float32 [P, C, h, w], view p of `plan` each, still flipped -> (mask uint8 [H, W], blended logits float32 [C, H, W]).
    Per pixel and class the covering views are taken iy ascending, ix ascending, f in plan order: acc = acc + g * v,
    ws = ws + g with g = wy[ly] * wx[lx] at the view's un-flipped position, every operation rounded to float32 on its own,
    out = acc / ws; the mask is argmax_nchw's rule on out.  One gathering launch, no floating-point atomics: the same bits on
    every run.  out_logits, out_mask: buffers to write into (every element is written).  label uint8 [H, W] with counts int64
    [C, C]: counts[label, class] += 1 per pixel (confusion_matrix's orientation), accumulated.  label_index: a device int32
    tensor of one element; label is then [S, H, W] and that plane is read (a recorded graph follows its tile).  Its VALUE is
    on the device and is not range-checked: the caller keeps it inside 0 .. S - 1 (graph.TileBuffers.aim checks on the host).
    ValueError, before any launch, for a plan that is not stitchable, a wrong rank, dtype or shape, tensors on different
    devices or non-contiguous storage; HipLibraryError for CPU tensors (there is no CPU path)."""
    what = "cd_tile_stitch"
    plan._need_stitchable(what)
    a = _Args(what, cpu_error=True)
    P, h, w, H, W = plan.P, plan.h, plan.w, plan.H, plan.W
    a.tensor("logits", logits, torch.float32, lambda t: t.dim() == 4 and 1 <= t.shape[1] <= 8 and (t.shape[0],) + tuple(t.shape[2:]) == (P, h, w),
             "[%d, C <= 8, %d, %d] as the plan has it" % (P, h, w))
    C = logits.shape[1]
    out_logits = a.out(out_logits, torch.float32, (C, H, W), "out_logits")
    out_mask = a.out(out_mask, torch.uint8, (H, W), "out_mask")
    if (label is None) != (counts is None):
        raise ValueError("%s: a label tile and counts come together" % what)
    if label_index is not None and label is None:
        raise ValueError("%s: a label index without labels" % what)
    if label is not None:
        if label_index is None:
            a.tensor("label", label, torch.uint8, (H, W))
        else:
            a.tensor("label", label, torch.uint8, lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (H, W), "[S, %d, %d]" % (H, W))
            a.tensor("label_index", label_index, torch.int32, lambda t: t.numel() == 1, "of one element")
        a.tensor("counts", counts, torch.int64, (C, C))
    a.placed()
    t = tile_tables(plan, logits.device)
    vp = lambda x: _vp(x.data_ptr()) if x is not None else _vp(0)
    _call("dh_cd_tile_stitch", vp(logits), P, C, h, w, vp(t["ys"]), plan.ny, vp(t["xs"]), plan.nx, vp(t["flips"]), plan.nf,
          vp(t["wy"]), vp(t["wx"]), vp(t["rows"]), vp(t["cols"]), plan.x_align(), H, W, vp(out_logits), vp(out_mask), vp(label),
          vp(label_index), vp(counts), S())
    return out_mask, out_logits


def cd_view_counts(logits, labels, counts):
    """counts int64 [P, C, C] += the confusion matrix of each view: logits float32 [P, C, h, w] against labels uint8 [P, h, w] or
    [P, 1, h, w] (what GpuPairPipeline.window_batch cuts; no int64 copy), class by argmax_nchw's rule, confusion_matrix's
    orientation counts[p, label, class].  One launch for what P evaluators each keep.  ValueError, before any launch, for a
    wrong rank, dtype or shape, tensors on different devices or non-contiguous storage; HipLibraryError for CPU tensors."""
    what = "cd_view_counts"
    a = _Args(what, cpu_error=True)
    a.tensor("logits", logits, torch.float32, lambda t: t.dim() == 4 and 1 <= t.shape[1] <= 8 and t.numel() > 0, "[P, C <= 8, h, w]")
    P, C, h, w = logits.shape
    a.tensor("labels", labels, torch.uint8, lambda t: tuple(t.shape) in ((P, h, w), (P, 1, h, w)),
             "%s or %s like logits" % ([P, h, w], [P, 1, h, w]))
    a.tensor("counts", counts, torch.int64, (P, C, C))
    a.placed()
    _call("dh_cd_view_counts", _vp(logits.data_ptr()), _vp(labels.data_ptr()), P, C, h, w, _vp(counts.data_ptr()), S())
    return counts


# ---- variants writing into caller-provided (contiguous) buffers ------------------------------------
def stem_space_to_depth_into(x_nchw, out):
    N, C, H, W = x_nchw.shape
    assert C == 3 and out.is_contiguous()
    _call("dh_stem_space_to_depth", dt(out), P(x_nchw), P(out), N, H, W, out.shape[-1], S())


def absdiff_upsample4_bwd_into(a, b, dy, da, db):
    N, H, W, C = a.shape
    _call("dh_absdiff_upsample4_bwd", dt(a), P(a), P(b), P(dy), P(da), P(db), N, H, W, C, S())


def reduce_rows(partial, nt, n, out, accumulate=False, scale=1.0):
    _call("dh_reduce_partials", P(partial), nt, n, scale, P(out), accumulate, S())


def scale_into(src, scalar_dev, dst):
    """dst = src * scalar (a 0-d / 1-element device tensor), no host sync"""
    _call("dh_scale_by_scalar", P(src), P(scalar_dev.reshape(1).float().contiguous()), P(dst), src.numel(), S())


def absdiff_halves(tok3, out):
    """out[b] = |tok3[b, 1] - tok3[b, 0]| for tok3 [B, 2, n] (token difference, networks.py:1311)"""
    B = tok3.shape[0]
    n = out.numel() // B
    assert tok3.is_contiguous() and out.is_contiguous()
    if tok3.dtype == torch.float32 and _ew_record(EW_ABSDIFF_HALVES, tok3, None, out, B, 0, n):
        return
    _call("dh_absdiff_halves", dt(tok3), P(tok3), P(out), B, n, S())


def absdiff_halves_bwd(tok3, dout, dtok3):
    B = tok3.shape[0]
    n = dout.numel() // B
    assert tok3.is_contiguous() and dout.is_contiguous() and dtok3.is_contiguous()
    if tok3.dtype == torch.float32 and _ew_record(EW_ABSDIFF_HALVES_BWD, tok3, dout, dtok3, B, 0, n):
        return
    _call("dh_absdiff_halves_bwd", dt(tok3), P(tok3), P(dout), P(dtok3), B, n, S())
