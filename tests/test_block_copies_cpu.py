"""Host side of the residual blocks' single-reader tensors (tests/test_block_copies_gpu.py has the kernels): the C entry of the
affine residual refuses incomplete arguments before anything is launched, and the engine's one switch reads as documented."""
import ctypes

import pytest


def test_affine_residual_entry_is_declared_exported_and_checks_its_arguments():
    from dahitra_amd import _lib
    assert "dh_bn_apply_res_affine" in _lib.declared_symbols()
    L = _lib.lib()
    mark = ctypes.c_char_p(b"\0" * 64)
    ptr = ctypes.cast(mark, ctypes.c_void_p)

    def call(res, rs, rb, groups=1):
        return L.dh_bn_apply_res_affine(1, None, res, rs, rb, None, None, None, 4 * max(groups, 1), 32, groups, 0, None, None)
    for res, rs, rb in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None), (None, None, None)):
        with pytest.raises(_lib.HipLibraryError, match=r"bn_apply_res_affine: residual, res_scale and res_shift are all required"):
            _lib.check(call(res, rs, rb), "dh_bn_apply_res_affine")
    # ... and takes the group counts of every other BatchNorm entry point
    for groups in (3, 5, 0):
        with pytest.raises(_lib.HipLibraryError, match=r"bn_\w+: 1, 2 or 4 statistics groups, got %d" % groups):
            _lib.check(call(ptr, ptr, ptr, groups), "dh_bn_apply_res_affine")


@pytest.mark.parametrize("value,want", [(None, False), ("0", False), ("1", True)])
def test_one_switch_restores_both_copies(value, want, monkeypatch):
    from dahitra_amd.engine import Engine
    if value is None:
        monkeypatch.delenv("DAHITRA_BLOCK_COPIES", raising=False)
    else:
        monkeypatch.setenv("DAHITRA_BLOCK_COPIES", value)
    assert Engine("base_transformer_pos_s4").block_copies is want


def test_lazy_shortcut_output_looks_like_its_tensor():
    import torch
    from dahitra_amd import ops
    y = torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16)
    r = ops.BnResidual(y, torch.ones(1, 8), torch.zeros(1, 8), 1)
    assert r.shape == y.shape and r.dtype == y.dtype and r.groups == 1


# ---- the plan of a convolution with a masked residual (host only: dh_conv2d_fwd_describe entry 5) -------------------------------
def _describe(L, dtype, N, H, W, C, frag=True, wreg_mode=-1):
    out = (ctypes.c_int * 30)()
    prev = L.dh_conv_wreg_mode(wreg_mode)
    try:
        rc = L.dh_conv2d_fwd_describe(5, dtype, N, H, W, C, H, W, C, C, 3, 1, 1, 0, 0, 0, 1, 1, 1, 0, 32 if frag else 0, 256, out)
    finally:
        L.dh_conv_wreg_mode(prev)
    return rc, list(out)


def test_masked_residual_plans_the_stream_at_the_bench_shapes_and_the_tap_kernel_on_ragged_ones():
    from dahitra_amd import _lib
    L = _lib.lib()
    # the 3x3 stride-1 data gradients of the bench step (64 images): layer1 64 x 64 x 64, layer2 128 x 32 x 32, layer3 256 x 32 x 32
    for C, HW, family in ((64, 64, 6), (128, 32, 7), (256, 32, 8)):
        rc, plan = _describe(L, 1, 64, HW, HW, C)
        assert rc == 0 and plan[0] == family and plan[18] == 1 and plan[19] == 0, (C, plan)
        assert L.dh_conv3x3_res_bits_supported(1, 64, HW, HW, C, C, C, 1) == 1
    rc, plan = _describe(L, 1, 2, 20, 20, 64)
    assert rc == 0 and plan[0] == 0 and plan[7] == 1, plan            # tap kernel bf16, compact epilogue
    rc, plan = _describe(L, 0, 2, 20, 20, 64, frag=False)
    assert rc == 0 and plan[0] == 1 and plan[7] == 1, plan            # exact fp32 tap kernel


def test_masked_residual_is_refused_by_the_families_without_a_mask_path():
    from dahitra_amd import _lib
    L = _lib.lib()
    # 32 -> 32 channels on enough whole tiles: the plan is the 32-channel stream form, which does not read the bytes
    out = (ctypes.c_int * 30)()
    assert L.dh_conv2d_fwd_describe(0, 1, 32, 256, 256, 32, 256, 256, 32, 32, 3, 1, 1, 0, 0, 0, 1, 1, 1, 0, 1, 256, out) == 0 and out[0] == 9
    rc, _ = _describe(L, 1, 32, 256, 256, 32, frag=False)
    assert rc != 0 and "mask bytes" in L.dh_last_error().decode()
    assert L.dh_conv3x3_res_bits_supported(1, 32, 256, 256, 32, 32, 32, 0) == 0
    # (a 1x1 or strided layer cannot be asked for at all: the entry point is 3x3 / stride 1 / pad 1; Cin not a whole 64-byte chunk)
    assert L.dh_conv3x3_res_bits_supported(1, 2, 16, 16, 48, 64, 64, 0) == 0
    # the call itself wants every tensor
    mark = ctypes.cast(ctypes.c_char_p(b"\0" * 64), ctypes.c_void_p)
    rc = L.dh_conv3x3_res_bits_fwd(1, mark, mark, None, mark, None, mark, 2, 16, 16, 64, 64, 64, None)
    with pytest.raises(_lib.HipLibraryError, match="conv3x3_res_bits_fwd: bad arguments"):
        _lib.check(rc, "dh_conv3x3_res_bits_fwd")
